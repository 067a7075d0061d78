// sage2_amd/csrc/kernels_support.inc -- the sweep of ContigExtender::findMatepairSupports (matePair/mergeContigs.cpp:959-1030): getSupportOfEdges (:1032-1097) and
// isUniqueInEdge (:1102-1110) for every (incoming, outgoing) pair of composite edges of every node, as a sort-and-reduce job over the read-list pool, the
// read-to-edge table (kernels_readmap.inc) and the mate tables (kernels_mates.inc).  Part of sage2ov_device.hip (included inside namespace s2, in this order).

// =============================================================================================
// The reference tries, per node, every in-edge against every out-edge and walks the in-edge's list once per out-edge.  Here a mate entry finds ITS out-edge: the
// mate is unique on at most one pair, and of that pair at most one half leaves the node.  The work is the list entries within the bound times their mates, not
// times the out-degree.
//   k_ms_nodes       nodeFlag[i] = 1 when an alive half-edge leaves i (then read i is a node, never "unique")
//   k_ms_unique      one thread per read: uniq[r] = pair + 1 when r has exactly one read-to-edge entry and is no node, else 0
//   k_ms_roles       one thread per half-edge: 1 = in-half (alive, flow >= 1, a list, no loop, type 0 or 1: its twin enters the node), 2 = out-half (type 2 or 3),
//                    0 = none; the list length of the in-halves (the records' work items); ins and outs per node
//   k_ms_cand        ins x outs per node (saturating); (scan): the candidate count of the statistics
//   k_rm_dprev, (scan)   the running sums (pool_running_sums)
//   k_ms_records<false / true>   one thread per list entry of an in-half (it finds its half by rm_owner: no thread walks a list).  Out unless the running sum is
//                    within the bound and the read is unique on the half's pair.  Then the read's mate entries of every library, found by binary search in the
//                    library's sorted keys (a per-read offset array would cost N + 2 words per library for the few reads that are asked), and per entry: the
//                    mate's pair, its half that leaves this node, the location test.  false: the count of every thread; (scan); true: key = a:32 | b:32
//   k_mate_iota, radix_sort_pairs, k_mate_heads, (scan) + k_headpos   only the passes whose digit can be non-zero
//   k_ms_reduce      entry e: the key of head e, support = the run's length
// Every count is kept below 2^32 - RS_TILE by the driver.
// =============================================================================================
// one library of either sweep's record kernel.  thr = upperBoundOfInsert + minOverlap - 2 * averageReadLength (:1073-1076; scaffolding.cpp:866), 0 for a library that is
// not valid; gbase = Mean[L] - 2 * averageReadLength mod 2^32 (scaffolding.cpp:878: the link sweep's, 0 here)
struct MsLib { const u64* key; u64 n; long long thr; u32 gbase, pad; };
struct MsTable { const u32* readOff; const u32* ePair; const u32* eNf; const u32* eNr; const u32* eLoc; const int* locs; u32 N; };
constexpr u32 MS_NONE = 0xFFFFFFFFu;
__global__ void k_ms_nodes(S4Graph g, u32 nh, uint8_t* nodeFlag) { const u32 h = blockIdx.x * blockDim.x + threadIdx.x; if (h < nh && g.alive[h]) nodeFlag[g.from[h]] = 1; }
__global__ void k_ms_unique(MsTable T, const uint8_t* __restrict__ nodeFlag, u32* uniq) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x; if (r > T.N) return;
    const u32 a = T.readOff[r], b = T.readOff[r + 1];
    uniq[r] = (b - a == 1u && !nodeFlag[r]) ? T.ePair[a] + 1u : 0u;
}
// ctr: [0] in-halves, [1] out-halves
__global__ void k_ms_roles(S4Graph g, u32 nh, const float* __restrict__ flow, uint8_t* role, u32* inCnt, u32* nIn, u32* nOut, unsigned long long* ctr) {
    const u32 h = blockIdx.x * blockDim.x + threadIdx.x;
    u32 r = 0;
    if (h < nh) {
        const u32 f = g.from[h];
        if (g.alive[h] && flow[h] >= 1.0f && g.cnt[h] > 0u && f != g.to[h]) r = g.type[h] <= 1 ? 1u : 2u;      // mergeContigs.cpp:979-986
        role[h] = (uint8_t)r; inCnt[h] = r == 1u ? g.cnt[h] : 0u;
        if (r == 1u) atomicAdd(&nIn[f], 1u); else if (r == 2u) atomicAdd(&nOut[f], 1u);
    }
    const u64 mi = __ballot(r == 1u), mo = __ballot(r == 2u);
    if (lane_id() == 0) { if (mi) atomicAdd(&ctr[0], (unsigned long long)__popcll(mi)); if (mo) atomicAdd(&ctr[1], (unsigned long long)__popcll(mo)); }
}
__global__ void k_ms_cand(const u32* __restrict__ nIn, const u32* __restrict__ nOut, u32 N, u32* prod) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x; if (i > N) return;
    const u64 p = (u64)nIn[i] * nOut[i]; prod[i] = p > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)p;
}
// the smallest |x| among the negative and among the positive locations of a table entry on one side (findDistanceOnEdge, matePair.cpp:575-609); MS_NONE: none
__device__ __forceinline__ void ms_min_locs(const MsTable& T, u32 e, bool forward, u32& neg, u32& pos) {
    const u32 nf = T.eNf[e], a = T.eLoc[e] + (forward ? 0u : nf), n = forward ? nf : T.eNr[e];
    neg = pos = MS_NONE;
    for (u32 x = a; x < a + n; x++) { const int v = T.locs[x]; if (v < 0) neg = min(neg, rm_abs(v)); else if (v > 0) pos = min(pos, (u32)v); }
}
// WRITE = false: cnt[w] = records of entry w, within += entries inside the bound; WRITE = true: the keys of entry w from pos[w] on
template <bool WRITE>
__global__ void k_ms_records(S4Graph g, u32 nh, const u32* __restrict__ inOff, u32 W, const u32* __restrict__ scan, u64 listUsed, u64 bound, const uint8_t* __restrict__ role,
                             const u32* __restrict__ uniq, MsTable T, const MsLib* __restrict__ libs, u32 nlib, u32* cnt, const u32* __restrict__ pos, u64* key, unsigned long long* within) {
    const u32 w = blockIdx.x * blockDim.x + threadIdx.x;
    bool inside = false; u32 c = 0;
    if (w < W) {
        const u32 h = rm_owner(inOff, nh, w);
        const u64 start = h < nh ? g.off[h] : 0, p = start + (w - (h < nh ? inOff[h] : 0u));
        if (h < nh && p < listUsed) {                                                 // (always, on a consistent graph: nothing is read out of bounds)
            const u64 e = g.lists[p];
            const u32 run = scan[p] + s4_dprev(e) - scan[start], m1 = (u32)(e & ((1ull << 40) - 1));
            inside = (u64)run <= bound;                                                // :1043 (the sums never fall: within the bound = in front of the first entry beyond it)
            if (inside && m1 <= T.N && uniq[m1] == (h >> 1) + 1u) {
                const u32 node = g.from[h], o = WRITE ? pos[w] : 0u;
                u32 neg1, pos1; ms_min_locs(T, T.readOff[m1], node < g.to[h], neg1, pos1);
                for (u32 L = 1; L <= nlib; L++) {
                    const MsLib lib = libs[L]; if (!lib.n || lib.thr <= 0) continue;
                    u64 lo = 0, hi = lib.n; const u64 want = (u64)m1 << 32;
                    while (lo < hi) { const u64 mid = lo + ((hi - lo) >> 1); if (lib.key[mid] < want) lo = mid + 1; else hi = mid; }
                    for (u64 i = lo; i < lib.n; i++) {
                        const u64 k = lib.key[i]; if ((u32)(k >> 32) != m1) break;
                        const u32 m2 = (u32)(k >> 2) & 0x3FFFFFFFu, q = m2 <= T.N ? uniq[m2] : 0u; if (!q) continue;
                        u32 hb = 2u * (q - 1u); if (g.from[hb] != node) hb++;
                        if (g.from[hb] != node || role[hb] != 2) continue;
                        const u32 x = ((k >> 1) & 1) ? neg1 : pos1; if (x == MS_NONE) continue;          // s1 * x < 0
                        u32 neg2, pos2; ms_min_locs(T, T.readOff[m2], node < g.to[hb], neg2, pos2);
                        const u32 y = (k & 1) ? neg2 : pos2; if (y == MS_NONE) continue;
                        if ((long long)((u64)x + y) < lib.thr) { if (WRITE) key[o + c] = ((u64)h << 32) | hb; c++; }
                    }
                }
            }
        }
        if (!WRITE) cnt[w] = c;
    }
    if (!WRITE) { const u64 m = __ballot(inside); if (lane_id() == 0 && m) atomicAdd(within, (unsigned long long)__popcll(m)); }
}
// ctr[2] += keys with support >= 2
__global__ void k_ms_reduce(const u64* __restrict__ keys, const u32* __restrict__ hp, u32 E, u64* outKey, u32* outSup, unsigned long long* ctr) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    bool two = false;
    if (e < E) { const u32 i = hp[e], s = hp[e + 1] - i; outKey[e] = keys[i]; outSup[e] = s; two = s >= 2u; }
    const u64 m = __ballot(two);
    if (lane_id() == 0 && m) atomicAdd(&ctr[2], (unsigned long long)__popcll(m));
}
