// sage2_amd/csrc/kernels_paths.inc -- the sweep of ContigExtender::findPathSupports / findPathSupportsNew (matePair/mergeContigs.cpp:118-353, :2148-): the claim of
// reads by nodes (:190-216), exploreGraph / checkFlow / savePath (:359-429) and findPathsBetweenMatepairs / insertPath (:539-743), as a sort-and-reduce job over the
// read-list pool, the read-to-edge table (kernels_readmap.inc) and the mate tables (kernels_mates.inc).  Part of sage2ov_device.hip (included inside namespace s2, in
// this order).  The contract is PATH SUPPORTS in include/sage2ov.h (DESIGN.md 5.18).

// =============================================================================================
// The reference walks the nodes in ascending order with one flag per read: a read belongs to the first node that meets it within the bound.  That is a minimum, so
//   k_sl_halves, (scan), k_rm_dprev, (scan)   the list entries of the alive halves as work items, the running sums (pool_running_sums)
//   k_pt_claim       one thread per list entry within the bound: atomicMin(claim[read], min(from, to))
//   k_pt_starts<false / true>   one thread per read: a claimed read gives (claiming node, end node) twice per read-to-edge entry; count, (scan), write
//   k_mate_iota, radix_sort_pairs, k_mate_heads, (scan) + k_headpos   the distinct (claiming node, start node), ascending
//   k_pt_take        the start node of every distinct record, and a flag where the claiming node changes; (scan) + k_headpos: where every claiming node's start
//                    nodes begin; k_pt_seg_nodes: the claiming node of every stretch
//   k_s4_degree, (scan), k_s4_fill, k_s4_sortadj   the alive halves of every node by ascending index (walked backwards: newest first)
//   k_pt_walk<false / true>   one lane per claiming node: the capped depth-first walk from its start nodes in ascending order.  false: paths per start node; (scan);
//                    true: every path as its halves and its length, in enumeration order -- the paths of one start node are one stretch of the pool, so "the paths that
//                    start at node to[edge1]" is a search among the node's start nodes and no sort.  The stack (half, cursor, length per level) is a per-lane slice of LDS
//   k_pt_vote        one lane per mate entry of a library: eligibility, the four combinations, the distance test, the intersection over the qualifying paths.  It
//                    leaves (first qualifying path, its edge1, the survivor mask); the survivors' count is the record count
//   (scan), k_pt_emit   the survivors as (half a : 32 | half b : 32)
//   k_mate_iota, radix_sort_pairs, k_mate_heads, (scan) + k_headpos, k_ms_reduce   one row per distinct key, its support the length of the run
// No kernel indexes a private array at run time: the walk's stack is LDS, the vote reads paths from memory into scalars of unrolled loops.  Every count is kept below
// 2^32 - RS_TILE by the driver.
// =============================================================================================
constexpr u32 PT_NONE = 0xFFFFFFFFu;
constexpr u32 PT_LEVELS = 7;                                                 // exploreGraph returns at level > 7 (:362)
constexpr u32 PT_CAP = 1000;                                                 // ... and when the node has saved more than 1000 paths
constexpr u32 PT_NO_SIGN = 100000u;                                          // `distance` of an (x, y) that fails the sign test (:614)
constexpr u32 PT_BLOCK = 64;
struct PtPath { u32 h[PT_LEVELS]; u32 len; };                                // the halves (PT_NONE behind the last) and the summed lengths of all but the last (savePath)
struct PtLib { const u64* key; const unsigned char* flag; u64 n; long long lower, upper; };      // one valid library with its estimate flags
// what the vote reads of the walk: the claiming nodes (ascending), where their start nodes begin, the start nodes, where their paths begin, the paths
struct PtIndex { const u32* segNode; const u32* segOff; u32 C; const u32* startNode; const u32* pathOff; const PtPath* paths; };
__device__ __forceinline__ bool pt_match(u32 t1, u32 t2) { return ((t1 & 1u) && t2 >= 2u) || (!(t1 & 1u) && t2 <= 1u); }      // matchEdgeType (:392-397)

// claim[r] = the smallest min(from, to) over the halves on whose list r stands within the bound (:190-216)
__global__ void k_pt_claim(S4Graph g, u32 nh, const u32* __restrict__ hOff, u32 W, const u32* __restrict__ scan, u64 listUsed, u64 bound, u32 N, u32* claim) {
    const u32 w = blockIdx.x * blockDim.x + threadIdx.x; if (w >= W) return;
    const u32 h = rm_owner(hOff, nh, w); if (h >= nh) return;
    const u64 start = g.off[h], p = start + (w - hOff[h]); if (p >= listUsed) return;            // (never, on a consistent graph: nothing is read out of bounds)
    const u64 e = g.lists[p];
    const u32 run = scan[p] + s4_dprev(e) - scan[start], m = (u32)(e & ((1ull << 40) - 1));
    if ((u64)run <= bound && m <= N) atomicMin(&claim[m], min(g.from[h], g.to[h]));
}
// WRITE = false: cnt[r] = start records of read r, ctr[0] += claimed reads; WRITE = true: the records from pos[r] on
template <bool WRITE>
__global__ void k_pt_starts(S4Graph g, MsTable T, const u32* __restrict__ claim, u32* cnt, const u32* __restrict__ pos, u64* key, unsigned long long* ctr) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    bool claimed = false;
    if (r <= T.N) {
        const u32 i = claim[r], a = T.readOff[r], b = T.readOff[r + 1];
        claimed = i != PT_NONE;
        if (!WRITE) cnt[r] = claimed ? 2u * (b - a) : 0u;
        else if (claimed) {
            u32 o = pos[r];
            for (u32 e = a; e < b; e++) { const u32 h = 2u * T.ePair[e]; key[o++] = ((u64)i << 32) | g.from[h]; key[o++] = ((u64)i << 32) | g.to[h]; }      // :224-237
        }
    }
    if (!WRITE) { const u64 m = __ballot(claimed); if (lane_id() == 0 && m) atomicAdd(&ctr[0], (unsigned long long)__popcll(m)); }
}
// the distinct keys: (claiming node, start node)
__global__ void k_pt_take(const u64* __restrict__ keys, const u32* __restrict__ hp, u32 S, u32* startNode, u32* flag) {
    const u32 s = blockIdx.x * blockDim.x + threadIdx.x; if (s >= S) return;
    const u64 k = keys[hp[s]];
    startNode[s] = (u32)k;
    flag[s] = (s == 0 || (u32)(keys[hp[s - 1]] >> 32) != (u32)(k >> 32)) ? 1u : 0u;
}
__global__ void k_pt_seg_nodes(const u64* __restrict__ keys, const u32* __restrict__ hp, const u32* __restrict__ segOff, u32 C, u32* segNode) {
    const u32 c = blockIdx.x * blockDim.x + threadIdx.x; if (c < C) segNode[c] = (u32)(keys[hp[segOff[c]]] >> 32);
}
// The walk of one claiming node (exploreGraph with its cap, :359-387).  g.deg / g.adjOff / g.adj: the alive halves of every node, oldest first.  FILL = false:
// pathCnt[s] = paths saved from start record s, ctr[1] += paths, ctr[2] += nodes that saved more than PT_CAP; FILL = true: the paths of start record s from pathOff[s] on
template <bool FILL>
__global__ void __launch_bounds__(PT_BLOCK) k_pt_walk(S4Graph g, const float* __restrict__ flow, u32 C, const u32* __restrict__ segOff, const u32* __restrict__ startNode, u64 bound,
                                                      u32* pathCnt, const u32* __restrict__ pathOff, PtPath* paths, u64 pathTotal, unsigned long long* ctr) {
    __shared__ u32 stHalf[PT_LEVELS + 1][PT_BLOCK], stCur[PT_LEVELS + 1][PT_BLOCK], stLen[PT_LEVELS + 1][PT_BLOCK];      // level 1 .. 7 of every lane: 8 x 3 dwords x 64
    const u32 t = threadIdx.x, c = blockIdx.x * PT_BLOCK + t;
    u32 total = 0;
    if (c < C) {
        for (u32 si = segOff[c]; si < segOff[c + 1]; si++) {
            u32 saved = 0;
            if (total <= PT_CAP) {                                                     // :362, the call at level 1
                const u32 s = startNode[si]; const u64 base = FILL ? pathOff[si] : 0;
                u32 L = 1; stCur[1][t] = g.adjOff[s] + g.deg[s];
                while (L >= 1u) {
                    const u32 node = L == 1u ? s : g.to[stHalf[L - 1][t]];
                    u32 cur = stCur[L][t];
                    if (cur == g.adjOff[node]) { L--; continue; }
                    cur--; stCur[L][t] = cur;
                    const u32 v = g.adj[cur];
                    u64 pl = 0; bool ok;
                    if (L == 1u) ok = g.cnt[v] != 0u && flow[v] > 0.0f;                // :370
                    else {
                        const u32 pv = stHalf[L - 1][t];
                        pl = (u64)stLen[L - 1][t] + g.len[pv];
                        ok = pt_match(g.type[pv], g.type[v]) && pl < bound;            // :378
                        if (ok) {                                                      // checkFlow (:403-415)
                            u32 uses = 0;
                            for (u32 k = 1; k < L; k++) { const u32 hk = stHalf[k][t]; uses += (hk == v || hk == (v ^ 1u)) ? 1u : 0u; }
                            const float f = flow[v];
                            ok = g.cnt[v] == 0u ? (float)uses <= f : (float)uses < f;
                        }
                    }
                    if (!ok) continue;
                    stHalf[L][t] = v; stLen[L][t] = (u32)pl;
                    if (FILL && base + saved < pathTotal) {                            // savePath (:420-429)
                        PtPath* P = paths + base + saved;
                        for (u32 k = 1; k <= PT_LEVELS; k++) P->h[k - 1] = k <= L ? stHalf[k][t] : PT_NONE;
                        P->len = (u32)pl;
                    }
                    saved++; total++;
                    if (L < PT_LEVELS && total <= PT_CAP) { const u32 nx = g.to[v]; L++; stCur[L][t] = g.adjOff[nx] + g.deg[nx]; }
                }
            }
            if (!FILL) pathCnt[si] = saved;
        }
    }
    if (!FILL) {
        if (total) atomicAdd(&ctr[1], (unsigned long long)total);
        const u64 m = __ballot(total > PT_CAP);
        if (lane_id() == 0 && m) atomicAdd(&ctr[2], (unsigned long long)__popcll(m));
    }
}
// some x in [a1, a1 + n1), y in [a2, a2 + n2) with lower < distance < upper (:610-625); neg: the sign the location must have (type 1)
__device__ __forceinline__ bool pt_distance_ok(const int* __restrict__ locs, u32 a1, u32 n1, u32 a2, u32 n2, bool neg1, bool neg2, u32 plen, long long lower, long long upper) {
    for (u32 i = 0; i < n1; i++) {
        const int x = locs[a1 + i]; const bool okx = neg1 ? x < 0 : x > 0;
        for (u32 j = 0; j < n2; j++) {
            const int y = locs[a2 + j]; const bool oky = neg2 ? y < 0 : y > 0;
            const long long d = (okx && oky) ? (long long)rm_abs(x) + rm_abs(y) + plen : (long long)PT_NO_SIGN;
            if (d < upper && d > lower) return true;
        }
    }
    return false;
}
// One mate entry (:254-300, :539-670, :699-743).  first[m] = the first qualifying path, fe1[m] = its edge1, mask[m] = the survivors among its pairs (bit k: the pair
// (sequence[k], sequence[k + 1]) of edge1, path[1 ..]); cnt[m] = their number.  ctr[3] += eligible entries, ctr[4] += voting ones, ctr[5] += survivors that a
// qualifying path held in the mirrored form only
__global__ void k_pt_vote(S4Graph g, u32 nh, MsTable T, const u32* __restrict__ uniq, const u32* __restrict__ claim, PtLib lib, PtIndex X, u32* first, u32* fe1, u32* mask, u32* cnt,
                          unsigned long long* ctr) {
    const u32 m = blockIdx.x * blockDim.x + threadIdx.x;
    bool eligible = false; u32 surv = 0, mirrored = 0, fpath = 0, fedge = 0;
    if ((u64)m < lib.n) {
        const u64 k = lib.key[m];
        const u32 m1 = (u32)(k >> 32), m2 = (u32)(k >> 2) & 0x3FFFFFFFu;
        if (lib.flag[m] == 1 && m1 <= T.N && m2 <= T.N) {
            const u32 i = claim[m1], i2 = claim[m2], q1 = uniq[m1], q2 = uniq[m2];
            eligible = i != PT_NONE && (i2 == PT_NONE || i2 > i) && q1 != 0u && q2 != 0u && 2u * q1 - 1u < nh && 2u * q2 - 1u < nh;      // :262, :563
            if (eligible) {
                u32 lo = 0, hi = X.C;                                                  // the node's stretch of start nodes
                while (lo < hi) { const u32 mid = lo + ((hi - lo) >> 1); if (X.segNode[mid] < i) lo = mid + 1u; else hi = mid; }
                const u32 s0 = lo < X.C && X.segNode[lo] == i ? X.segOff[lo] : 0u, s1 = lo < X.C && X.segNode[lo] == i ? X.segOff[lo + 1] : 0u;
                const u32 hA = 2u * (q1 - 1u), hB = 2u * (q2 - 1u);
                const u32 E1 = sl_is_E(g.from[hA], g.to[hA], hA) ? hA : hA + 1u, E2 = sl_is_E(g.from[hB], g.to[hB], hB) ? hB : hB + 1u;
                const u32 e1 = T.readOff[m1], e2 = T.readOff[m2];
                const u32 nf1 = T.eNf[e1], nr1 = T.eNr[e1], l1 = T.eLoc[e1], nf2 = T.eNf[e2], nr2 = T.eNr[e2], l2 = T.eLoc[e2];
                const bool neg1 = ((k >> 1) & 1) != 0, neg2 = (k & 1) != 0;
                bool have = false; u32 f0 = 0, f1 = 0, f2 = 0, f3 = 0, f4 = 0, f5 = 0, f6 = 0, f7 = 0;      // the first qualifying path: edge1, path[1 .. 7]
                for (u32 x = 0; x < 4u; x++) {                                         // :565-586
                    const u32 edge1 = E1 ^ (x >> 1), edge2 = E2 ^ (x & 1u);
                    const bool fw1 = (x >> 1) != 0, fw2 = (x & 1u) == 0;               // findDistanceOnEdge(twin of edge1), (edge2): forward where that half is E
                    const u32 a1 = l1 + (fw1 ? 0u : nf1), n1 = fw1 ? nf1 : nr1, a2 = l2 + (fw2 ? 0u : nf2), n2 = fw2 ? nf2 : nr2;
                    if (!n1 || !n2) continue;
                    const u32 want = g.to[edge1]; const u32 t1 = g.type[edge1];
                    u32 a = s0, b = s1;
                    while (a < b) { const u32 mid = a + ((b - a) >> 1); if (X.startNode[mid] < want) a = mid + 1u; else b = mid; }
                    if (a >= s1 || X.startNode[a] != want) continue;
                    for (u32 j = X.pathOff[a]; j < X.pathOff[a + 1]; j++) {
                        const PtPath* P = X.paths + j;
                        const u32 p1 = P->h[0], p2 = P->h[1], p3 = P->h[2], p4 = P->h[3], p5 = P->h[4], p6 = P->h[5], p7 = P->h[6];
                        const u32 last = p7 != PT_NONE ? p7 : (p6 != PT_NONE ? p6 : (p5 != PT_NONE ? p5 : (p4 != PT_NONE ? p4 : (p3 != PT_NONE ? p3 : (p2 != PT_NONE ? p2 : p1)))));
                        if (last != edge2 || !pt_match(t1, g.type[p1])) continue;       // :607
                        if (!pt_distance_ok(T.locs, a1, n1, a2, n2, neg1, neg2, P->len, lib.lower, lib.upper)) continue;
                        if (!have) {                                                   // insertPath, the first path (:702-712)
                            have = true; fpath = j; fedge = edge1;
                            f0 = edge1; f1 = p1; f2 = p2; f3 = p3; f4 = p4; f5 = p5; f6 = p6; f7 = p7;
                            surv = 1u | (p2 != PT_NONE ? 2u : 0u) | (p3 != PT_NONE ? 4u : 0u) | (p4 != PT_NONE ? 8u : 0u) | (p5 != PT_NONE ? 16u : 0u) | (p6 != PT_NONE ? 32u : 0u) | (p7 != PT_NONE ? 64u : 0u);
                            continue;
                        }
                        const u32 fs[8] = {f0, f1, f2, f3, f4, f5, f6, f7}, qs[8] = {edge1, p1, p2, p3, p4, p5, p6, p7};      // (constant indices below: registers)
                        #pragma unroll
                        for (int kk = 0; kk < 7; kk++) {                               // :715-728
                            if (!((surv >> kk) & 1u)) continue;
                            bool direct = false, mirror = false;
                            #pragma unroll
                            for (int l = 0; l < 7; l++) {
                                if (qs[l + 1] == PT_NONE) continue;
                                direct = direct || (fs[kk] == qs[l] && fs[kk + 1] == qs[l + 1]);
                                mirror = mirror || (fs[kk] == (qs[l + 1] ^ 1u) && fs[kk + 1] == (qs[l] ^ 1u));
                            }
                            if (!direct && !mirror) surv &= ~(1u << kk);
                            if (!direct && mirror) mirrored |= 1u << kk;
                        }
                    }
                }
            }
        }
        first[m] = fpath; fe1[m] = fedge; mask[m] = surv; cnt[m] = __popc(surv);
    }
    const u64 me = __ballot(eligible), mv = __ballot(surv != 0u);
    if (lane_id() == 0) { if (me) atomicAdd(&ctr[3], (unsigned long long)__popcll(me)); if (mv) atomicAdd(&ctr[4], (unsigned long long)__popcll(mv)); }
    const u32 mm = __popc(surv & mirrored); if (mm) atomicAdd(&ctr[5], (unsigned long long)mm);
}
__global__ void k_pt_emit(const u32* __restrict__ first, const u32* __restrict__ fe1, const u32* __restrict__ mask, const u32* __restrict__ pos, u32 n, const PtPath* __restrict__ paths, u64 R, u64* key) {
    const u32 m = blockIdx.x * blockDim.x + threadIdx.x; if (m >= n) return;
    const u32 s = mask[m]; if (!s) return;
    const PtPath* P = paths + first[m];
    u64 o = pos[m]; u32 a = fe1[m];
    for (u32 k = 0; k < PT_LEVELS; k++) {
        const u32 b = P->h[k]; if (b == PT_NONE) break;
        if (((s >> k) & 1u) && o < R) key[o++] = ((u64)a << 32) | b;
        a = b;
    }
}
