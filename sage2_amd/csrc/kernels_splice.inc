// sage2_amd/csrc/kernels_splice.inc -- a batch of edge-disjoint splices over the resident step-4 graph: a splice makes a new pair of half-edges from two operand
// half-edges and retires the operands.  Its two plans: the merge of ContigExtender::mergeEdgesAndUpdate (matePair/mergeContigs.cpp:1260-1288, overlapGraph.cpp:165-186,
// :259-266, :299-336; DESIGN.md 5.16; k_mg_plan, below) and the join of ScaffoldMaker::mergeDisconnectedEdges (k_sc_plan, kernels_scaffold.inc; DESIGN.md 5.17).
// Part of sage2ov_device.hip (included inside namespace s2, after kernels_simplify.inc); not a translation unit of its own.
//
// Both plan kernels write one SplicePlan per splice (sage2ov_internal.h: the host reads it too) and lens[2 i], lens[2 i + 1], the lengths of its two new lists (0 when
// refused); everything after them reads the record.  Direction 0 of splice i is the forward list (first = a, second = b), direction 1 the twin's (first = b ^ 1,
// second = a ^ 1).  The new pair is half-edges nh + 2 r, nh + 2 r + 1 with r = the number of splices in front of i that were made: the forward half a.from -> b.to and
// its twin, in the order insertEdge makes them.  No thread walks a list: the lists are written one thread per output entry.

__device__ __forceinline__ int mg_combined_type(u32 t1, u32 t2) {                     // overlapGraph.cpp:259-266
    if ((t1 == 0 && t2 == 0) || (t1 == 1 && t2 == 2)) return 0;
    if ((t1 == 0 && t2 == 1) || (t1 == 1 && t2 == 3)) return 1;
    if ((t1 == 2 && t2 == 0) || (t1 == 3 && t2 == 2)) return 2;
    if ((t1 == 2 && t2 == 1) || (t1 == 3 && t2 == 3)) return 3;
    return -1;
}
// one thread per merge (a enters the shared node, b leaves it: to[a] == from[b], checked by the caller): refused or made, type, flow, delete or keep
// (mergeContigs.cpp:1262-1289, :1378); one middle entry, no distances.  isNew[i]: 1 when a pair is created (scanned: the rank).  flow null: every flow is 0
__global__ void k_mg_plan(S4Graph g, const float* __restrict__ flow, const u32* __restrict__ ha, const u32* __restrict__ hb, u32 n, int typeOfMerge, SplicePlan* plan, u32* lens, u32* isNew) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
    const u32 a = ha[i], b = hb[i];
    SplicePlan p = {}; p.a = a; p.b = b; p.extra = 1;
    const int t = mg_combined_type(g.type[a], g.type[b]);
    if (a != b && a != (b ^ 1u) && g.alive[a] && g.alive[b] && t >= 0) {
        const float f1 = flow ? flow[a] : 0.f, f2 = flow ? flow[b] : 0.f;
        float f = 0.f;
        if (!(f1 == 0.f && f2 == 0.f)) f = typeOfMerge == 1 ? 1.f : (f1 <= f2 ? f1 : f2);
        p.flow = f; p.type = (uint8_t)t; p.made = 1; p.del1 = f1 <= f; p.del2 = f2 <= f;
        p.lenF = g.len[a] + g.len[b]; p.lenT = g.len[a ^ 1u] + g.len[b ^ 1u];
    }
    plan[i] = p;
    const u32 l = p.made ? g.cnt[a] + g.cnt[b] + 1u : 0u;
    lens[2 * i] = l; lens[2 * i + 1] = l; isNew[i] = p.made;
}
// one thread per entry of the new lists, both lists of every splice in one launch: the list of `first`, the middle, the list of `second` (getListOfReads,
// overlapGraph.cpp:299-336; getListOfReadsInDisconnectedEdges, :861-881).  The middle is node1 = to[first] alone (extra 1), or node1 and node2 = from[second] with the
// plan's distances between them (extra 2); an operand without a list stands in with its length (merges only: a join's operands are composite).
// lo: the exclusive scan of lens (2 n values); the entry's list is the last one that starts at or before it
__global__ void k_sp_lists(S4Graph g, const SplicePlan* __restrict__ plan, const u32* __restrict__ lo, u32 n2, u64 total, u32 base) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (t >= total) return;
    u32 l = 0, r = n2;                                                              // the largest j with lo[j] <= t (lists of length 0 share their start with the next one)
    while (r - l > 1) { const u32 m = l + ((r - l) >> 1); if ((u64)lo[m] <= t) l = m; else r = m; }
    const SplicePlan* __restrict__ p = plan + (l >> 1); const u32 d = l & 1u;       // (read field by field: a copied entry needs a, b and extra only)
    const u32 pa = p->a, pb = p->b, extra = p->extra;
    const u32 first = d ? (pb ^ 1u) : pa, second = d ? (pa ^ 1u) : pb;
    const u32 c1 = g.cnt[first], c2 = g.cnt[second], x = (u32)(t - lo[l]);          // (c2 beside c1: in the middle branch a load would wait for it)
    u64 e;
    if (x < c1) e = g.lists[(u64)g.off[first] + x];
    else if (x >= c1 + extra) e = g.lists[(u64)g.off[second] + (x - c1 - extra)];
    else {
        // every load that needs first and second only stands in front of the selects, so that they are issued together (a load inside an arm of ?: is a branch of
        // its own and waits for the one before it; these launches are a few blocks and all latency).  Entry 0 of the pool (there: the new entries are in it) stands
        // in where an operand has no list
        const u32 o1 = g.off[first], o2 = g.off[second], ty1 = g.type[first], ty2 = g.type[second], node1 = g.to[first], node2 = g.from[second], len1 = g.len[first], len2 = g.len[second];
        const u32 d1 = d ? p->dNext1[1] : p->dNext1[0], d2 = d ? p->dPrev2[1] : p->dPrev2[0];      // (selects, not a run-time index into the record)
        const u64 last1 = g.lists[c1 ? (u64)o1 + c1 - 1 : 0], head2 = g.lists[c2 ? (u64)o2 : 0];
        const u32 dPrev1 = c1 ? s4_dnext(last1) : len1, dNext2 = c2 ? s4_dprev(head2) : len2;
        e = x == c1 ? s4_entry(node1, (ty1 == 1u || ty1 == 3u) ? 1u : 0u, dPrev1, extra == 1u ? dNext2 : d1) : s4_entry(node2, (ty2 == 2u || ty2 == 3u) ? 1u : 0u, d2, dNext2);
    }
    g.lists[(u64)base + t] = e;
}
// one thread per splice: the new halves (insertEdge with the plan's flow and lengths), then the operands: both halves deleted, or both lose the new edge's flow (each
// half its own float).  rank null: nothing was refused, splice i makes pair i.  flow null: every flow is 0 and stays so
__global__ void k_sp_commit(S4Graph g, float* flow, const SplicePlan* __restrict__ plan, const u32* __restrict__ lo, const u32* __restrict__ rank, u32 n, u32 nh, u32 base) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
    const SplicePlan p = plan[i]; if (!p.made) return;
    const u32 a = p.a, b = p.b, h = nh + 2 * (rank ? rank[i] : i), c = g.cnt[a] + g.cnt[b] + p.extra;
    g.from[h] = g.from[a]; g.to[h] = g.to[b]; g.len[h] = p.lenF; g.cnt[h] = c; g.off[h] = base + lo[2 * i]; g.type[h] = p.type; g.alive[h] = 1;
    g.from[h + 1] = g.to[b]; g.to[h + 1] = g.from[a]; g.len[h + 1] = p.lenT; g.cnt[h + 1] = c; g.off[h + 1] = base + lo[2 * i + 1];
    g.type[h + 1] = (uint8_t)s4_rev_type(p.type); g.alive[h + 1] = 1;
    if (flow) { flow[h] = p.flow; flow[h + 1] = p.flow; }
    if (p.del1) { g.alive[a] = 0; g.alive[a ^ 1u] = 0; } else if (flow) { flow[a] -= p.flow; flow[a ^ 1u] -= p.flow; }
    if (p.del2) { g.alive[b] = 0; g.alive[b ^ 1u] = 0; } else if (flow) { flow[b] -= p.flow; flow[b ^ 1u] -= p.flow; }
}
