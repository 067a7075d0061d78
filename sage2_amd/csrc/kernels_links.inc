// sage2_amd/csrc/kernels_links.inc -- the sweep that opens every round of ScaffoldMaker::mergeFinal / mergeFinalSmall (matePair/scaffolding.cpp:786-935, :981-1130):
// support and mean gap of every ordered pair of half-edges that mate pairs link, through a node or not, as a sort-and-reduce job over the read-list pool, the
// read-to-edge table (kernels_readmap.inc) and the mate tables (kernels_mates.inc).  Part of sage2ov_device.hip (included inside namespace s2, in this order).

// =============================================================================================
// The reference asks, per composite edge, which edges its mates reach (getListOfFeasibleEdges, :148-234) and then walks the edge's list once per reached edge and
// direction.  Here a mate entry finds ITS partner: the mate is unique on at most one pair, so an entry within the bound is tried against the two halves of that pair
// and nothing else.  LINK(a, b) of include/sage2ov.h is the run of the key a:32 | b:32.
//   k_ms_nodes, k_ms_unique   uniq[r] = pair + 1 when r has exactly one read-to-edge entry and is no node (kernels_support.inc)
//   k_sl_halves      the list length of every alive half-edge (the records' work items); (scan)
//   k_rm_dprev, (scan)   the running sums (pool_running_sums)
//   k_sl_records<false / true>   one thread per list entry of an alive half (it finds its half by rm_owner: no thread walks a list).  Out unless the running sum is
//                    within the bound and the read is unique on the half's pair.  Then the read's mate entries of every valid library, found by binary search in the
//                    library's sorted keys, and per entry: the mate's pair q (not the thread's own), and for BOTH halves of q the first (x, y) in list order that
//                    passes (:850-874).  false: the count of every thread; (scan); true: key = a:32 | b:32, value = Mean[L] - (dist + 2 * averageReadLength) mod 2^32
//   k_mate_iota, radix_sort_pairs   only the passes whose digit can be non-zero
//   k_sl_gather      the values in sorted order, and one 0 behind them; (scan, mod 2^32): gapSum of a run is the difference of two scanned values
//   k_mate_heads, (scan) + k_headpos
//   k_sl_reduce      row e: the key of head e, support = the run's length, gap = (int32_t)gapSum / support (:892), and gapSum itself (mergeContigs.cpp:1587 reads it)
// A library is the MsLib of kernels_support.inc.  Every count is kept below 2^32 - RS_TILE by the driver.  No kernel uses LDS or scratch; the d1 x d2 loops read the locations from memory, no array is indexed.
// =============================================================================================
constexpr u32 SL_NO_SIGN = 10000000u;                                        // distance_all of an (x, y) that fails the sign test (:854)
// E of a pair: the half leaving the smaller node; of a loop the half with the higher index (k_rm_records' side 0)
__device__ __forceinline__ bool sl_is_E(u32 f, u32 t, u32 h) { return f < t || (f == t && (h & 1u)); }
// ctr[0] += alive halves with a list
__global__ void k_sl_halves(S4Graph g, u32 nh, u32* cnt, unsigned long long* ctr) {
    const u32 h = blockIdx.x * blockDim.x + threadIdx.x;
    u32 c = 0;
    if (h < nh) { c = g.alive[h] ? g.cnt[h] : 0u; cnt[h] = c; }
    const u64 m = __ballot(c > 0u);
    if (lane_id() == 0 && m) atomicAdd(&ctr[0], (unsigned long long)__popcll(m));
}
// the first (x, y), x over [a1, a1 + n1) outside and y over [a2, a2 + n2) inside, whose distance passes (:850-874); neg: the sign the location must have (type 1)
__device__ __forceinline__ bool sl_first_hit(const int* __restrict__ locs, u32 a1, u32 n1, u32 a2, u32 n2, bool neg1, bool neg2, long long thr, u32& dist) {
    for (u32 i = 0; i < n1; i++) {
        const int x = locs[a1 + i]; const bool okx = neg1 ? x < 0 : x > 0;
        for (u32 j = 0; j < n2; j++) {
            const int y = locs[a2 + j]; const bool oky = neg2 ? y < 0 : y > 0;
            const u32 d = (okx && oky) ? rm_abs(x) + rm_abs(y) : SL_NO_SIGN;
            if ((long long)d < thr) { dist = d; return true; }
        }
    }
    return false;
}
// WRITE = false: cnt[w] = records of entry w; ctr[1] += entries inside the bound, ctr[2] += unique ones, ctr[3] += mate entries probed.  WRITE = true: the records of
// entry w from pos[w] on
template <bool WRITE>
__global__ void k_sl_records(S4Graph g, u32 nh, const u32* __restrict__ hOff, u32 W, const u32* __restrict__ scan, u64 listUsed, u64 bound, const u32* __restrict__ uniq,
                             MsTable T, const MsLib* __restrict__ libs, u32 nlib, u32* cnt, const u32* __restrict__ pos, u64* key, u32* val, unsigned long long* ctr) {
    const u32 w = blockIdx.x * blockDim.x + threadIdx.x;
    bool inside = false, un = false; u32 c = 0, probed = 0;
    if (w < W) {
        const u32 h = rm_owner(hOff, nh, w);
        const u64 start = h < nh ? g.off[h] : 0, p = start + (w - (h < nh ? hOff[h] : 0u));
        if (h < nh && p < listUsed) {                                                 // (always, on a consistent graph: nothing is read out of bounds)
            const u64 e = g.lists[p];
            const u32 run = scan[p] + s4_dprev(e) - scan[start], m1 = (u32)(e & ((1ull << 40) - 1)), own = (h >> 1) + 1u;
            inside = (u64)run <= bound;                                                // :833-835 (the sums never fall: within the bound = in front of the first entry beyond it)
            un = inside && m1 <= T.N && uniq[m1] == own;                               // :837
            if (un) {
                const u32 o = WRITE ? pos[w] : 0u, e1 = T.readOff[m1], nf1 = T.eNf[e1];
                const bool E1 = sl_is_E(g.from[h], g.to[h], h);
                const u32 a1 = T.eLoc[e1] + (E1 ? 0u : nf1), n1 = E1 ? nf1 : T.eNr[e1];
                for (u32 L = 1; L <= nlib; L++) {
                    const MsLib lib = libs[L]; if (!lib.n || lib.thr <= 0) continue;
                    u64 lo = 0, hi = lib.n; const u64 want = (u64)m1 << 32;
                    while (lo < hi) { const u64 mid = lo + ((hi - lo) >> 1); if (lib.key[mid] < want) lo = mid + 1; else hi = mid; }
                    for (u64 i = lo; i < lib.n; i++) {
                        const u64 k = lib.key[i]; if ((u32)(k >> 32) != m1) break;
                        probed++;
                        const u32 m2 = (u32)(k >> 2) & 0x3FFFFFFFu, q = m2 <= T.N ? uniq[m2] : 0u; if (!q || q == own) continue;      // :843; pair(a) != pair(b)
                        const u32 e2 = T.readOff[m2], nf2 = T.eNf[e2], nr2 = T.eNr[e2], l2 = T.eLoc[e2];
                        for (u32 side = 0; side < 2u; side++) {
                            const u32 hb = 2u * (q - 1u) + side; if (hb >= nh || !g.alive[hb]) continue;
                            const bool E2 = sl_is_E(g.from[hb], g.to[hb], hb);
                            u32 dist = 0;
                            if (sl_first_hit(T.locs, a1, n1, l2 + (E2 ? 0u : nf2), E2 ? nf2 : nr2, ((k >> 1) & 1) != 0, (k & 1) != 0, lib.thr, dist)) {
                                if (WRITE) { key[o + c] = ((u64)h << 32) | hb; val[o + c] = lib.gbase - dist; }
                                c++;
                            }
                        }
                    }
                }
            }
        }
        if (!WRITE) cnt[w] = c;
    }
    if (!WRITE) {
        const u64 mi = __ballot(inside), mu = __ballot(un);
        if (lane_id() == 0) { if (mi) atomicAdd(&ctr[1], (unsigned long long)__popcll(mi)); if (mu) atomicAdd(&ctr[2], (unsigned long long)__popcll(mu)); }
        if (probed) atomicAdd(&ctr[3], (unsigned long long)probed);
    }
}
// out[i] = the value of the i-th sorted record; out[n] = 0 (so that the scan's last value is the sum of all)
__global__ void k_sl_gather(const u32* __restrict__ idx, const u32* __restrict__ val, u32 n, u32* out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x; if (i > n) return;
    out[i] = i < n ? val[idx[i]] : 0u;
}
// sc: the exclusive scan, mod 2^32, of the n + 1 gathered values
__global__ void k_sl_reduce(const u64* __restrict__ keys, const u32* __restrict__ hp, const u32* __restrict__ sc, u32 E, u64* outKey, u32* outSup, int* outGap, int* outSum) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x; if (e >= E) return;
    const u32 i = hp[e], j = hp[e + 1], s = j - i;
    const int sum = (int)(sc[j] - sc[i]);                                              // int32_t gapSum (:782, :878)
    outKey[e] = keys[i]; outSup[e] = s; outGap[e] = (int)((long long)sum / (long long)s);      // :892 (s >= 1; the division truncates towards zero)
    outSum[e] = sum;
}
