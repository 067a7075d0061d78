// sage2_amd/csrc/kernels_copycount.inc -- step 5 around its solver (CopyCountEstimator, overlapGraph/copycountEstimator.cpp:29-417; checkIfAllReadsPresent,
// overlapGraph.cpp:445-493): the sums of the genome-size rounds, the classes and arcs of the flow network and a solver's flows back onto the resident graph.
// Part of sage2ov_device.hip (included inside namespace s2, in this order).

// =============================================================================================
// The state restated is the reference's after loadOverlapGraphFromFile of the file sage2ov_graph4_save would write: a node's edge list is the reverse of file
// order over the records that start at the node.  File position of a record: 2 x + s for the x-th record pair of the save order, s = 0 for the half the writer
// visits (from <= to), 1 for its twin; both halves of a loop are visited, so a loop has two record pairs and four records.
//   k_sl_halves, (scan)   the list length of every alive half-edge: the work items of the per-entry kernels (kernels_links.inc)
//   k_cc_nodes       present[from] = 1 for every alive half
//   k_cc_entries     one thread per list entry (it finds its half by rm_owner: no thread walks a list): present[read] = 1; the entries of the even half of a
//                    pair add frequency[read] to k[pair] -- summed across the lanes of a wave that share the half, one atomic per run of lanes.  Integers: exact
//   k_cc_present     sum of frequency over the present reads (numberOfReads as step 5 sees it)
//   k_cc_round       one round's deltaSum and kSum over the halves with from < to; the float test runs here (:83-84)
//   k_cc_select, (scan), k_cc_compact, sort by from   the save order (per node, ascending half index)
//   k_cc_filekeys, sort by from   the records in descending file position, stably sorted by their start node: the nodes' loaded lists, one after the other;
//                    k_mate_heads, (scan) + k_headpos: where each node's list begins = the node ranks (node_index = 3 + 4 rank)
//   k_cc_ranks, k_cc_rank_of   node of every rank, rank of every node
//   k_cc_classes     per record r of the lists: the half, and for the records with from >= to (:130, :229) class, flow_lb and arc count; the counters the reference logs
//   k_cc_node_arcs   arc 0 and the six arcs of every node
//   k_cc_edge_arcs   one wave per record, the waves of a capped grid striding over the records: the two arcs of a simple / once edge, or the costs and the six arcs of a many edge.  The cost fold (:325-332) is sequential
//                    by contract: a lane per entry loads the entry (coalesced), gathers its frequency and computes the three terms; the fold then runs across the lanes
//                    of the chunk, every lane folding the same values in the same order.  Only IEEE multiply, add, convert and divide; every log comes from the host
//   k_cc_apply       one thread per solver line: the first record of from_node's list whose other end is to_node (:380-387) gets the flow, integer atomics
//   k_cc_average     both halves of a pair = (f + f_twin) / 2 (:392-403); the pairs whose halves differed
// No contraction into fma: the reference's build has none.  Every function with float arithmetic opens with `#pragma clang fp contract(off)`.
// =============================================================================================

struct CcConst {                 // the constants of a launch, every log computed on the host as the reference spells it
    float ratio;                 // (float)n / (float)G
    float lj[21];                // lj[j] = log((float)((float)(j + 1) / (float)j)), j = 1..20
    float l1, l3, l5, l1000;     // log((float)1), 3, 5, 1000
    float fN1, fN3, fN5;         // log((float)(N - 1)), (N - 3), (N - 5)
    double dN3, dN1000;          // log(N - 3), log(N - 1000): the integer argument takes the double overload
    u64 n;                       // numberOfReads
};
struct CcArc { u32 from, to; int lower, upper; float cost; };
constexpr u32 CC_SIMPLE = 0, CC_ONCE = 1, CC_MANY = 2, CC_NONE = 3;

__device__ __forceinline__ float cc_a(u32 delta, u64 k, float ratio, float lg) {
    #pragma clang fp contract(off)
    const float t1 = (float)delta * ratio;
    const float t2 = (float)k * lg;
    return t1 - t2;
}

__global__ void k_cc_nodes(S4Graph g, u32 nh, uint8_t* present, u32 N) {
    const u32 h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h < nh && g.alive[h] && g.from[h] <= N) present[g.from[h]] = 1;
}
__global__ void k_cc_entries(S4Graph g, u32 nh, const u32* __restrict__ hOff, u32 W, u64 listUsed, const unsigned short* __restrict__ freq, u32 N, uint8_t* present,
                             unsigned long long* kPair) {
    const u32 w = blockIdx.x * blockDim.x + threadIdx.x;
    u32 h = ~0u; u64 f = 0;
    if (w < W) {
        const u32 o = rm_owner(hOff, nh, w);
        if (o < nh) {
            const u64 p = (u64)g.off[o] + (w - hOff[o]);
            if (p < listUsed) {                                                        // (always, on a consistent graph: nothing is read out of bounds)
                const u64 id = g.lists[p] & ((1ull << 40) - 1);
                if (id <= N) { present[id] = 1; if (!(o & 1u)) { h = o; f = freq[id]; } }
            }
        }
    }
    // lanes of one half are neighbours: the first lane of a run adds the run's sum
    const u32 lane = lane_id();
    const u32 hPrev = __shfl_up(h, 1);
    const bool head = lane == 0 || hPrev != h;
    const u64 heads = __ballot(head);
    const u64 above = lane == 63 ? 0ull : (heads >> (lane + 1));
    const u32 runLen = above ? (u32)__ffsll((unsigned long long)above) : 64u - lane;      // lanes from this one to the end of its run
    u64 s = f;
    for (int d = 1; d < 64; d <<= 1) { const u64 t = __shfl_down(s, d); if ((u32)d < runLen) s += t; }      // s covers [lane, min(lane + 2 d, end of the run))
    if (head && h != ~0u && s) atomicAdd(&kPair[h >> 1], (unsigned long long)s);
}
__global__ void k_cc_present(const uint8_t* __restrict__ present, const unsigned short* __restrict__ freq, u32 N, unsigned long long* out) {
    u64 s = 0;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i <= N; i += (u64)gridDim.x * blockDim.x) if (i >= 1 && present[i]) s += freq[i];
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d);
    if (lane_id() == 0 && s) atomicAdd(out, (unsigned long long)s);
}
// out[0] += delta, out[1] += k of the halves with from < to that qualify; first: the round without a previous estimate (:90)
__global__ void k_cc_round(S4Graph g, u32 nh, const unsigned long long* __restrict__ kPair, int first, float ratio, float l2, unsigned long long* out) {
    const u32 h = blockIdx.x * blockDim.x + threadIdx.x;
    u64 ds = 0, ks = 0;
    if (h < nh && g.alive[h] && g.from[h] < g.to[h]) {
        const u32 len = g.len[h], delta = len - 1u; const u64 k = kPair[h >> 1];
        const bool ok = first ? len > 500u : (cc_a(delta, k, ratio, l2) >= 3.0f && delta >= 1000u);
        if (ok) { ds = delta; ks = k; }
    }
    for (int d = 32; d >= 1; d >>= 1) { ds += __shfl_down(ds, d); ks += __shfl_down(ks, d); }
    if (lane_id() == 0 && (ds | ks)) { atomicAdd(&out[0], (unsigned long long)ds); atomicAdd(&out[1], (unsigned long long)ks); }
}
__global__ void k_cc_select(S4Graph g, u32 nh, u32* sel) { const u32 h = blockIdx.x * blockDim.x + threadIdx.x; if (h < nh) sel[h] = (g.alive[h] && g.from[h] <= g.to[h]) ? 1u : 0u; }
__global__ void k_cc_compact(S4Graph g, u32 nh, const u32* __restrict__ sel, const u32* __restrict__ pos, u64* key, u32* half) {
    const u32 h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h < nh && sel[h]) { key[pos[h]] = g.from[h]; half[pos[h]] = h; }
}
// the records in descending file position: j -> position F - 1 - j, the half order[position / 2] (through the sort's index) or its twin; key = its start node
__global__ void k_cc_filekeys(S4Graph g, const u32* __restrict__ half, const u32* __restrict__ idx, u32 F, u64* key, u32* rec) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x; if (j >= F) return;
    const u32 fp = F - 1u - j, h = half[idx[fp >> 1]] ^ (fp & 1u);
    key[j] = g.from[h]; rec[j] = h;
}
__global__ void k_cc_gather(const u32* __restrict__ idx, const u32* __restrict__ rec, u32 F, u32* adj) { const u32 r = blockIdx.x * blockDim.x + threadIdx.x; if (r < F) adj[r] = rec[idx[r]]; }
__global__ void k_cc_ranks(const u64* __restrict__ keys, const u32* __restrict__ hp, u32 E, u32* nodeOf) { const u32 e = blockIdx.x * blockDim.x + threadIdx.x; if (e < E) nodeOf[e] = (u32)keys[hp[e]]; }
__global__ void k_cc_rank_of(const u32* __restrict__ nodeOf, u32 E, u32* rankOf, u32 N) { const u32 e = blockIdx.x * blockDim.x + threadIdx.x; if (e < E && nodeOf[e] <= N) rankOf[nodeOf[e]] = e; }
// ctr: edges, simple, once, many
__global__ void k_cc_classes(S4Graph g, const u32* __restrict__ adj, u32 F, const unsigned long long* __restrict__ kPair, CcConst C, uint8_t* cls, uint8_t* lbOut, u32* arcs, unsigned long long* ctr) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    u32 c = CC_NONE, lb = 0;
    if (r < F) {
        const u32 h = adj[r];
        if (g.from[h] >= g.to[h]) {
            const u32 cnt = g.cnt[h];
            if (!cnt) c = CC_SIMPLE;
            else {
                const u32 delta = g.len[h] - 1u; const u64 k = kPair[h >> 1];
                if (cc_a(delta, k, C.ratio, C.lj[1]) >= 3.0f && delta >= 1000u) c = CC_ONCE;
                else {
                    c = CC_MANY;
                    if (delta > 1000u) {
                        float a = cc_a(delta, k, C.ratio, C.lj[1]);
                        for (int j = 1; j <= 19; j++) { const float b = cc_a(delta, k, C.ratio, C.lj[j + 1]); if (a < -3.0f && b > 3.0f) { lb = (u32)j + 1u; break; } a = b; }
                    } else if (cnt > 35u) lb = 1;
                }
            }
        }
        cls[r] = (uint8_t)c; lbOut[r] = (uint8_t)lb; arcs[r] = c == CC_NONE ? 0u : (c == CC_MANY ? 6u : 2u);
    }
    const u64 mE = __ballot(c != CC_NONE), mS = __ballot(c == CC_SIMPLE), mO = __ballot(c == CC_ONCE), mM = __ballot(c == CC_MANY);
    if (lane_id() == 0 && mE) {
        atomicAdd(&ctr[0], (unsigned long long)__popcll(mE));
        if (mS) atomicAdd(&ctr[1], (unsigned long long)__popcll(mS));
        if (mO) atomicAdd(&ctr[2], (unsigned long long)__popcll(mO));
        if (mM) atomicAdd(&ctr[3], (unsigned long long)__popcll(mM));
    }
}
// arc 0 (its upper bound, 100 * network nodes, saturates in the record: the writer prints the exact number) and the six arcs of every node (:210-222)
__global__ void k_cc_node_arcs(u32 E, CcArc* out) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e == 0) { const u64 cap = 100ull * (4ull * E + 2ull); out[0] = CcArc{2u, 1u, 1, cap > 0x7FFFFFFFull ? 0x7FFFFFFF : (int)cap, 0.0f}; }
    if (e >= E) return;
    const u32 c = 3u + 4u * e; const float big = 1000000.0f * 10.0f, one = 1.0f * 10.0f;
    CcArc* o = out + 1 + 6ull * e;
    o[0] = CcArc{1u, c, 0, 100, big}; o[1] = CcArc{c + 1u, 2u, 0, 100, big}; o[2] = CcArc{1u, c + 2u, 0, 100, big}; o[3] = CcArc{c + 3u, 2u, 0, 100, big};
    o[4] = CcArc{c, c + 1u, 0, 100, one}; o[5] = CcArc{c + 2u, c + 3u, 0, 100, one};
}
// the arcs of record r, by one wave (every branch and return is the same for all its lanes); base: arcs in front of the edge arcs
__device__ __forceinline__ void cc_edge_record(const S4Graph& g, u32 r, u32 lane, const u32* __restrict__ adj, const uint8_t* __restrict__ cls, const uint8_t* __restrict__ lbIn,
                                               const u32* __restrict__ apos, u64 base, const u32* __restrict__ rankOf, const unsigned short* __restrict__ freq, u32 N, u64 listUsed,
                                               const CcConst& C, CcArc* out) {
    #pragma clang fp contract(off)
    const u32 c = cls[r]; if (c == CC_NONE) return;
    const u32 h = adj[r];
    const u32 u = 3u + 4u * rankOf[g.from[h]], v = 3u + 4u * rankOf[g.to[h]], ty = g.type[h];
    u32 n1, n2, n3, n4;                                                                // :258-285
    if (ty == 0) { n1 = v + 1; n2 = u; n3 = u + 3; n4 = v + 2; }
    else if (ty == 1) { n1 = u + 3; n2 = v; n3 = v + 3; n4 = u; }
    else if (ty == 2) { n1 = u + 1; n2 = v + 2; n3 = v + 1; n4 = u + 2; }
    else { n1 = u + 1; n2 = v; n3 = v + 3; n4 = u + 2; }
    CcArc* o = out + base + apos[r];
    if (c != CC_MANY) {
        const int lo = c == CC_ONCE ? 1 : 0, up = c == CC_ONCE ? 1 : 100; const float cost = (c == CC_ONCE ? 1.0f : 10000.0f) * 10.0f;
        if (lane == 0) o[0] = CcArc{n1, n2, lo, up, cost};
        if (lane == 1) o[1] = CcArc{n3, n4, lo, up, cost};
        return;
    }
    const u32 cnt = g.cnt[h]; const u64 off = g.off[h];
    float c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
    for (u32 b0 = 0; b0 < cnt; b0 += 64u) {
        const u32 i = b0 + lane; double t1 = 0.0, t3 = 0.0; float t2 = 0.0f;
        if (i < cnt && off + i < listUsed) {
            const u64 id = g.lists[off + i] & ((1ull << 40) - 1);
            const int xi = id <= N ? (int)freq[id] : 0;
            const u64 m = C.n - (u64)(long long)xi;
            const float xf = (float)xi, mf = (float)m; const double md = (double)m;
            {   // cost_1 (:329)
                const float a = xf * C.l3; const double b = md * C.dN3; const double t = (double)(-a) - b;
                const float cc = xf * C.l1; const float dd = mf * C.fN1; const float inner = (-cc) - dd;
                t1 = t - (double)inner;
            }
            {   // cost_2 (:330): float throughout
                const float a = xf * C.l5; const float b = mf * C.fN5; const float t = (-a) - b;
                const float cc = xf * C.l3; const float dd = mf * C.fN3; const float inner = (-cc) - dd;
                t2 = t - inner;
            }
            {   // cost_3 (:331)
                const float a = xf * C.l1000; const double b = md * C.dN1000; const double t = (double)(-a) - b;
                const float cc = xf * C.l5; const float dd = mf * C.fN5; const float inner = (-cc) - dd;
                t3 = t - (double)inner;
            }
        }
        const u32 m = cnt - b0 < 64u ? cnt - b0 : 64u;
        for (u32 l = 0; l < m; l++) {                                                  // the fold: every lane the same values in list order
            const double v1 = __shfl(t1, (int)l); const float v2 = __shfl(t2, (int)l); const double v3 = __shfl(t3, (int)l);
            c1 = (float)((double)c1 + v1);
            c2 = c2 + v2;
            c3 = (float)((double)c3 + v3);
        }
    }
    c1 = c1 / 2.0f; c2 = c2 / 2.0f; c3 = c3 / 995.0f;                                   // :340-342
    const int lb = (int)lbIn[r];
    const int lb1 = lb < 3 ? lb : 3, lb2 = (lb < 5 ? lb : 5) - 3 > 0 ? (lb < 5 ? lb : 5) - 3 : 0, lb3 = (lb < 1000 ? lb : 1000) - 5 > 0 ? (lb < 1000 ? lb : 1000) - 5 : 0;
    if (lane < 6) {
        const u32 q = lane >> 1; const bool second = lane & 1u;
        const float cost = (q == 0 ? c1 : (q == 1 ? c2 : c3)) * 10.0f;
        o[lane] = CcArc{second ? n3 : n1, second ? n4 : n2, q == 0 ? lb1 : (q == 1 ? lb2 : lb3), q == 0 ? 3 : (q == 1 ? 2 : 995), cost};
    }
}
// a wave per record, the waves striding over the records: the host caps the grid (CC_ARC_BLOCKS blocks of 256 threads), so the launch stays far below the 2^32
// threads at which this runtime cuts a launch down without an error, whatever F is
constexpr u32 CC_ARC_BLOCKS = 4096;
__global__ void k_cc_edge_arcs(S4Graph g, const u32* __restrict__ adj, u32 F, const uint8_t* __restrict__ cls, const uint8_t* __restrict__ lbIn, const u32* __restrict__ apos, u64 base,
                               const u32* __restrict__ rankOf, const unsigned short* __restrict__ freq, u32 N, u64 listUsed, CcConst C, CcArc* out) {
    const u32 lane = lane_id(), wpb = blockDim.x >> 6;
    for (u64 r = (u64)blockIdx.x * wpb + (threadIdx.x >> 6); r < F; r += (u64)gridDim.x * wpb)
        cc_edge_record(g, (u32)r, lane, adj, cls, lbIn, apos, base, rankOf, freq, N, listUsed, C, out);
}
// line i: cs2 nodes fr -> to with a flow; the caller has checked 1 <= node <= 4 E + 2
__global__ void k_cc_apply(S4Graph g, const u32* __restrict__ adj, const u32* __restrict__ hp, const u32* __restrict__ nodeOf, u32 E, const u64* __restrict__ fr, const u64* __restrict__ to,
                           const u64* __restrict__ fl, u64 n, unsigned long long* acc, unsigned long long* ctr) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
    const u64 a = fr[i], b = to[i];
    if (a <= 2 || b <= 2) return;
    const u64 ra = (a - 3) >> 2, rb = (b - 3) >> 2;
    if (ra >= E || rb >= E || ra == rb) return;
    const u32 target = nodeOf[rb];
    for (u32 r = hp[ra], end = hp[ra + 1]; r < end; r++) {                             // the node's loaded list, newest first
        const u32 h = adj[r];
        if (g.to[h] == target) { atomicAdd(&acc[h], (unsigned long long)fl[i]); atomicAdd(&ctr[0], 1ull); return; }
    }
}
__global__ void k_cc_average(S4Graph g, u32 nh, const unsigned long long* __restrict__ acc, float* flow, unsigned long long* ctr) {
    #pragma clang fp contract(off)
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    bool diff = false;
    if (2u * p + 1u < nh) {
        const u32 h = 2u * p;
        if (g.alive[h]) {
            const float f0 = flow[h] + (float)acc[h], f1 = flow[h + 1] + (float)acc[h + 1];
            const float avg = (f0 + f1) / 2.0f;
            diff = f0 != f1;
            flow[h] = avg; flow[h + 1] = avg;
        }
    }
    const u64 m = __ballot(diff);
    if (lane_id() == 0 && m) atomicAdd(&ctr[1], (unsigned long long)__popcll(m));
}
