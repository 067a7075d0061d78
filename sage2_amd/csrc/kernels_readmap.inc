// sage2_amd/csrc/kernels_readmap.inc -- MatePair::mapReadsToEdges / mapReadLocations / computeMeanSD (matePair.cpp:318-569) as a sort-and-reduce job over
// the read-list pool of step 4 and a join with the mate table.  Part of sage2ov_device.hip (included inside namespace s2, in this order); not a translation unit of its own.

// =============================================================================================
// The reference hangs a linked list of (edge, locations) on every read and grows the location arrays with realloc, one location at a time.  Here:
//   k_rm_dprev       distPrevious of every entry of the pool, dead lists included, as u32
//   (scan)           exclusive scan of them, mod 2^32: the running sum of an entry inside its list is scan[entry] + dprev[entry] - scan[list start]
//   k_rm_count       entries per alive half-edge; (scan): the position of its records
//   k_rm_records     one thread per record (it finds its half-edge by binary search in the scanned counts: no thread walks a list):
//                    key = read:30 | pair:31 | side:1 (side 0: the half mapReadsToEdges visits first, E; 1: its twin), payload = the signed location.
//                    Records are written in half-edge order and list order: the stable sort keeps list order inside a key
//   k_mate_iota, radix_sort_pairs   only the passes whose digit can be non-zero
//   k_rm_heads       a record is a head when (read, pair) differs from its predecessor's; (scan) + k_headpos
//   k_rm_entries     entry e: read, pair, n_forward (binary search for the first side-1 record of the run), n_reverse, location offset = head position
//   k_rm_gather      the locations in sorted order
//   k_rm_offsets     first entry of every read (binary search, as k_mate_offsets)
//   k_rm_join        a group of RM_GROUP lanes per mate entry: the two reads' entry lists (sorted by pair, almost always of length 0 or 1) are intersected --
//                    lane x takes entries x, x + RM_GROUP, ... of `from` and searches each in the list of `to`; flag = no common pair; for from < to the
//                    number of common pairs where both reads have exactly one forward location
//   (scan) + k_rm_join again with the positions: the distances, with the mate entry and pair of each (the export orders them by the pair's ordinal)
//   k_rm_round       count, sum d and the 128-bit sum (mu - d)^2 over the d < 4 mu: a wave64 DPP reduction, one partial of four words per block, added by the host
// Every count is kept below 2^32 - RS_TILE by the driver.
// =============================================================================================
constexpr int RM_GROUP = 8;
__global__ void k_rm_dprev(const u64* __restrict__ lists, u64 n, u32* out) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) out[i] = s4_dprev(lists[i]);
}
__global__ void k_rm_count(S4Graph g, u32 nh, u32* cnt) { const u32 h = blockIdx.x * blockDim.x + threadIdx.x; if (h < nh) cnt[h] = g.alive[h] ? g.cnt[h] : 0u; }
// the half-edge whose records hold record r: the last h with recOff[h] <= r (half-edges without records share their offset with the next one)
__device__ __forceinline__ u32 rm_owner(const u32* __restrict__ recOff, u32 nh, u32 r) {
    u32 lo = 0, hi = nh;
    while (lo < hi) { const u32 mid = lo + ((hi - lo) >> 1); if (recOff[mid] <= r) lo = mid + 1u; else hi = mid; }
    return lo - 1u;
}
__global__ void k_rm_records(S4Graph g, u32 nh, const u32* __restrict__ recOff, u32 R, const u32* __restrict__ scan, u64 listUsed, u64* key, u32* loc) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x; if (r >= R) return;
    const u32 h = rm_owner(recOff, nh, r);
    if (h >= nh) { key[r] = ~0ull; loc[r] = 0; return; }                             // (cannot happen: recOff[0] = 0)
    const u64 start = g.off[h], pos = start + (r - recOff[h]);
    if (pos >= listUsed) { key[r] = ~0ull; loc[r] = 0; return; }                     // (cannot happen on a consistent graph: nothing is read out of bounds)
    const u64 e = g.lists[pos];
    const u32 run = scan[pos] + s4_dprev(e) - scan[start];
    const u32 f = g.from[h], t = g.to[h];
    const u32 side = f < t ? 0u : (f > t ? 1u : ((h & 1u) ? 0u : 1u));               // a loop: the half with the higher index comes first in the node's list
    key[r] = ((e & ((1ull << 40) - 1)) << 32) | ((u64)(h >> 1) << 1) | side;
    loc[r] = ((e >> 40) & 1) ? run : 0u - run;                                       // matePair.cpp:521-524
}
__global__ void k_rm_heads(const u64* __restrict__ keys, u32 n, u32* flag) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
    flag[i] = (i == 0 || (keys[i - 1] >> 1) != (keys[i] >> 1)) ? 1u : 0u;
}
__global__ void k_rm_entries(const u64* __restrict__ keys, const u32* __restrict__ hp, u32 E, u32* eRead, u32* ePair, u32* eNf, u32* eNr, u32* eLoc) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x; if (e >= E) return;
    const u32 a = hp[e], b = hp[e + 1]; const u64 k = keys[a];
    u32 lo = a, hi = b;
    while (lo < hi) { const u32 mid = lo + ((hi - lo) >> 1); if ((keys[mid] & 1ull) == 0) lo = mid + 1u; else hi = mid; }
    eRead[e] = (u32)(k >> 32); ePair[e] = (u32)(k >> 1) & 0x7FFFFFFFu; eNf[e] = lo - a; eNr[e] = b - lo; eLoc[e] = a;
}
__global__ void k_rm_gather(const u32* __restrict__ vals, const u32* __restrict__ loc, u32 n, int* out) { const u32 i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) out[i] = (int)loc[vals[i]]; }
__global__ void k_rm_offsets(const u32* __restrict__ eRead, u32 E, u32 N, u32* offsets) {
    const u32 a = blockIdx.x * blockDim.x + threadIdx.x; if (a > N + 1u) return;
    u32 lo = 0, hi = E;
    if (a == N + 1u) lo = E;
    else while (lo < hi) { const u32 mid = lo + ((hi - lo) >> 1); if (eRead[mid] < a) lo = mid + 1u; else hi = mid; }
    offsets[a] = lo;
}
struct RmTable { const u32* readOff; const u32* ePair; const u32* eNf; const u32* eLoc; const int* locs; u32 N; };
__device__ __forceinline__ u32 rm_abs(int v) { return v < 0 ? 0u - (u32)v : (u32)v; }
// WRITE = false: flag[m] and dcount[m]; WRITE = true: the distances of entry m from dpos[m] on, in the order of `from`'s entries
template <bool WRITE>
__global__ void k_rm_join(const u64* __restrict__ mkey, u32 n, RmTable T, unsigned char* flag, u32* dcount, const u32* __restrict__ dpos, u32* dist, u32* dEntry, u32* dPair) {
    const u32 m = blockIdx.x * (blockDim.x / RM_GROUP) + threadIdx.x / RM_GROUP, gl = threadIdx.x & (RM_GROUP - 1), gshift = lane_id() & ~(u32)(RM_GROUP - 1);
    const bool live = m < n;
    u32 a0 = 0, a1 = 0, b0 = 0, b1 = 0; bool ordered = false;
    if (live) {
        const u64 k = mkey[m]; const u32 from = (u32)(k >> 32), to = (u32)(k >> 2) & 0x3FFFFFFFu;
        if (from <= T.N && to <= T.N) { a0 = T.readOff[from]; a1 = T.readOff[from + 1]; b0 = T.readOff[to]; b1 = T.readOff[to + 1]; }
        ordered = from < to;
    }
    u32 common = 0, written = 0;
    for (u32 base = a0; __any(base < a1); base += RM_GROUP) {                        // (the ballots below want every lane of the wave)
        const u32 i = base + gl; bool hit = false, counts = false; u32 j = 0;
        if (i < a1) {
            const u32 p = T.ePair[i]; u32 lo = b0, hi = b1;
            while (lo < hi) { const u32 mid = lo + ((hi - lo) >> 1); if (T.ePair[mid] < p) lo = mid + 1u; else hi = mid; }
            hit = lo < b1 && T.ePair[lo] == p; j = lo;
            counts = hit && ordered && T.eNf[i] == 1u && T.eNf[j] == 1u;
        }
        const u32 hm = (u32)(__ballot(hit) >> gshift) & ((1u << RM_GROUP) - 1), cm = (u32)(__ballot(counts) >> gshift) & ((1u << RM_GROUP) - 1);
        common += __popc(hm);
        if (WRITE && counts) {
            const u32 o = dpos[m] + written + __popc(cm & ((1u << gl) - 1));
            const u32 x = rm_abs(T.locs[T.eLoc[i]]), y = rm_abs(T.locs[T.eLoc[j]]);
            dist[o] = x > y ? x - y : y - x; dEntry[o] = m; dPair[o] = T.ePair[i];
        }
        written += __popc(cm);
    }
    if (!WRITE && live && gl == 0) { flag[m] = common ? 0 : 1; dcount[m] = written; }
}
// ---- one round of computeMeanSD: {count, sum, sq low, sq high} of the d < thr, per block
template <int CTRL, int ROWMASK>
__device__ __forceinline__ u64 dpp_mov64(u64 v) { return (u64)dpp_mov<CTRL, ROWMASK>(0, (u32)v) | ((u64)dpp_mov<CTRL, ROWMASK>(0, (u32)(v >> 32)) << 32); }
template <int CTRL, int ROWMASK>
__device__ __forceinline__ void rm_dpp_step(u64& c, u64& s, u64& ql, u64& qh) {     // lanes the step does not reach receive 0
    c += dpp_mov64<CTRL, ROWMASK>(c); s += dpp_mov64<CTRL, ROWMASK>(s);
    const u64 ol = dpp_mov64<CTRL, ROWMASK>(ql), oh = dpp_mov64<CTRL, ROWMASK>(qh);
    const u64 nl = ql + ol; qh += oh + (nl < ql ? 1ull : 0ull); ql = nl;
}
__global__ void __launch_bounds__(256) k_rm_round(const u32* __restrict__ dist, u64 n, u64 thr, long long mu, u64* partial) {
    __shared__ u64 sh[4][4];
    u64 c = 0, s = 0, ql = 0, qh = 0;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 d = dist[i];
        if (d < thr) {
            const long long df = mu - (long long)d; const u64 a = (u64)(df < 0 ? -df : df);          // < 2^34: the square needs 68 bits
            const u64 lo = a * a, nl = ql + lo; qh += __umul64hi(a, a) + (nl < ql ? 1ull : 0ull); ql = nl;
            c++; s += d;
        }
    }
    rm_dpp_step<0x111, 0xF>(c, s, ql, qh); rm_dpp_step<0x112, 0xF>(c, s, ql, qh); rm_dpp_step<0x114, 0xF>(c, s, ql, qh); rm_dpp_step<0x118, 0xF>(c, s, ql, qh);
    rm_dpp_step<0x142, 0xA>(c, s, ql, qh); rm_dpp_step<0x143, 0xC>(c, s, ql, qh);                  // lane 63 holds the wave's sums
    const u32 w = threadIdx.x >> 6;
    if (lane_id() == 63) { sh[w][0] = c; sh[w][1] = s; sh[w][2] = ql; sh[w][3] = qh; }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 C = 0, S = 0, L = 0, H = 0;
        for (int x = 0; x < 4; x++) { C += sh[x][0]; S += sh[x][1]; const u64 nl = L + sh[x][2]; H += sh[x][3] + (nl < L ? 1ull : 0ull); L = nl; }
        u64* o = partial + 4ull * blockIdx.x; o[0] = C; o[1] = S; o[2] = L; o[3] = H;
    }
}
