// sage2_amd/csrc/kernels_merge.inc -- ContigExtender::mergeEdgesAndUpdate for a batch of edge-disjoint merges (matePair/mergeContigs.cpp:1260-1288,
// overlapGraph.cpp:165-186, :259-266, :299-336) over the resident step-4 graph (DESIGN.md 5.16).
// Part of sage2ov_device.hip (included inside namespace s2, after kernels_simplify.inc); not a translation unit of its own.
//
// A merge is (a, b): half-edge a = e1 enters the shared node, half-edge b = e2 leaves it (to[a] == from[b], checked by the caller, as is that no record pair is
// named twice).  The new pair of merge i is half-edges nh + 2 r, nh + 2 r + 1 with r = the number of merges in front of i that were not refused: the forward
// half e1.from -> e2.to and its twin, in the order insertEdge makes them.  No thread walks a list: the lists are written one thread per output entry.

struct MgPlan { u32 a, b; float flow; uint8_t type, merged, del1, del2; };            // 16 bytes; type: combinedEdgeType
__device__ __forceinline__ int mg_combined_type(u32 t1, u32 t2) {                     // overlapGraph.cpp:259-266
    if ((t1 == 0 && t2 == 0) || (t1 == 1 && t2 == 2)) return 0;
    if ((t1 == 0 && t2 == 1) || (t1 == 1 && t2 == 3)) return 1;
    if ((t1 == 2 && t2 == 0) || (t1 == 3 && t2 == 2)) return 2;
    if ((t1 == 2 && t2 == 1) || (t1 == 3 && t2 == 3)) return 3;
    return -1;
}
// one thread per merge: refused or merged, type, flow, delete or keep (mergeContigs.cpp:1262-1289, :1378); lens[2 i], lens[2 i + 1]: the lengths of the two new
// lists (0 when refused), isNew[i]: 1 when a pair is created.  flow null: every flow is 0
__global__ void k_mg_plan(S4Graph g, const float* __restrict__ flow, const u32* __restrict__ ha, const u32* __restrict__ hb, u32 n, int typeOfMerge, MgPlan* plan, u32* lens, u32* isNew) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
    const u32 a = ha[i], b = hb[i];
    MgPlan p; p.a = a; p.b = b; p.flow = 0.f; p.type = 0; p.merged = p.del1 = p.del2 = 0;
    const int t = mg_combined_type(g.type[a], g.type[b]);
    if (a != b && a != (b ^ 1u) && g.alive[a] && g.alive[b] && t >= 0) {
        const float f1 = flow ? flow[a] : 0.f, f2 = flow ? flow[b] : 0.f;
        float f = 0.f;
        if (!(f1 == 0.f && f2 == 0.f)) f = typeOfMerge == 1 ? 1.f : (f1 <= f2 ? f1 : f2);
        p.flow = f; p.type = (uint8_t)t; p.merged = 1; p.del1 = f1 <= f; p.del2 = f2 <= f;
    }
    plan[i] = p;
    const u32 l = p.merged ? g.cnt[a] + g.cnt[b] + 1u : 0u;
    lens[2 * i] = l; lens[2 * i + 1] = l; isNew[i] = p.merged;
}
// one thread per entry of the new lists, forward and twin lists of every merge in one launch: getListOfReads(e1, e2) and getListOfReads(e2.twin, e1.twin)
// (overlapGraph.cpp:299-336).  lo: the exclusive scan of lens (2 n values); the entry's list is the last one that starts at or before it
__global__ void k_mg_lists(S4Graph g, const MgPlan* __restrict__ plan, const u32* __restrict__ lo, u32 n2, u64 total, u32 base) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (t >= total) return;
    u32 l = 0, r = n2;                                                              // the largest j with lo[j] <= t (lists of length 0 share their start with the next one)
    while (r - l > 1) { const u32 m = l + ((r - l) >> 1); if ((u64)lo[m] <= t) l = m; else r = m; }
    const MgPlan p = plan[l >> 1];
    const u32 first = (l & 1u) ? (p.b ^ 1u) : p.a, second = (l & 1u) ? (p.a ^ 1u) : p.b;
    const u32 c1 = g.cnt[first], c2 = g.cnt[second], x = (u32)(t - lo[l]);
    u64 e;
    if (x < c1) e = g.lists[(u64)g.off[first] + x];
    else if (x > c1) e = g.lists[(u64)g.off[second] + (x - c1 - 1)];
    else {
        const u32 ty = g.type[first];
        const u32 dPrev = c1 ? s4_dnext(g.lists[(u64)g.off[first] + c1 - 1]) : g.len[first];
        const u32 dNext = c2 ? s4_dprev(g.lists[(u64)g.off[second]]) : g.len[second];
        e = s4_entry(g.to[first], (ty == 1 || ty == 3) ? 1u : 0u, dPrev, dNext);
    }
    g.lists[(u64)base + t] = e;
}
// one thread per merge: the new halves (insertEdge), then the operands: both halves deleted, or both lose the new edge's flow (each half its own float)
__global__ void k_mg_commit(S4Graph g, float* flow, const MgPlan* __restrict__ plan, const u32* __restrict__ lo, const u32* __restrict__ rank, u32 n, u32 nh, u32 base) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
    const MgPlan p = plan[i]; if (!p.merged) return;
    const u32 a = p.a, b = p.b, h = nh + 2 * rank[i], c = g.cnt[a] + g.cnt[b] + 1u;
    g.from[h] = g.from[a]; g.to[h] = g.to[b]; g.len[h] = g.len[a] + g.len[b]; g.cnt[h] = c; g.off[h] = base + lo[2 * i]; g.type[h] = p.type; g.alive[h] = 1;
    g.from[h + 1] = g.to[b]; g.to[h + 1] = g.from[a]; g.len[h + 1] = g.len[a ^ 1u] + g.len[b ^ 1u]; g.cnt[h + 1] = c; g.off[h + 1] = base + lo[2 * i + 1];
    g.type[h + 1] = (uint8_t)s4_rev_type(p.type); g.alive[h + 1] = 1;
    if (flow) { flow[h] = p.flow; flow[h + 1] = p.flow; }
    if (p.del1) { g.alive[a] = 0; g.alive[a ^ 1u] = 0; } else if (flow) { flow[a] -= p.flow; flow[a ^ 1u] -= p.flow; }
    if (p.del2) { g.alive[b] = 0; g.alive[b ^ 1u] = 0; } else if (flow) { flow[b] -= p.flow; flow[b ^ 1u] -= p.flow; }
}
