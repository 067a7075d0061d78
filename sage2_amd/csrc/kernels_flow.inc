// sage2_amd/csrc/kernels_flow.inc -- step 5's solver (main_cs2, copycountEstimator.cpp:359; cs2/): min-cost flow by Goldberg-Tarjan cost scaling with
// round-synchronous push-relabel (DESIGN.md 5.20; tests/flow_model.py is the same method in numpy).  Part of sage2ov_device.hip (included inside namespace s2).
//
// Integers only: 64-bit prices, excesses and scaled costs, 32-bit residual capacities.  Nodes are 1..n; arrays per node have n + 2 words.
// The kernels of the rounds and of the price update are templates on the price type P: long long, or __int128 for networks whose prices leave +-2^62 (prices,
// reduced costs, eps and the floor are P; excess, delta, distances and residuals keep their widths).  With P = __int128 an entry's cost stays the unscaled 64-bit
// cost and is multiplied by scale (< 2^32) where it is read, so that the entry arrays streamed every round do not grow; a price is one aligned 16-byte load.
// Entry 2 i is arc i forwards (residual upper - lower, cost * scale), entry 2 i + 1 backwards (residual 0, -cost * scale); the entries are sorted stably by
// tail (the project's radix sort), so a node's list is start[v] .. start[v + 1] in ascending entry number; sis[s] is the position of the entry's sister.
//   k_mf_from_cc     the resident network's records: the float cost truncated towards zero, as `%lld` reads the printed text (parser_cs2.h:257)
//   k_mf_check       bad arcs and max |cost| into the counter block
//   k_mf_keys        the sort keys (the tails) and the excess of the lower bounds
//   k_mf_pos, k_mf_entries, k_mf_starts   the sorted layout
//   k_mf_saturate    start of a refine: every entry with residual > 0 and negative reduced cost is saturated
//   k_mf_push        every node with excess > 0 walks its list in order and pushes min(residual, what is left of the excess it had when the phase began) along
//                    every admissible entry.  What a node receives goes to delta[], not to excess[]: no decision depends on another node's pushes of the same phase.
//                    Lists of up to MF_LANE_DEG entries: a lane per node.  Longer lists: the workgroup walks the list MF_BLOCK entries at a time, an exclusive
//                    scan of the admissible residuals clipped to the excess -- the same amounts as the serial walk.  Lists longer than hubDeg (an argument;
//                    SAGE2OV_MCF_HUB_DEG) are left to the hub form below.
//   k_mf_relabel     excess += delta.  A node with excess > 0 and no admissible entry: p = max over residual entries of p(head) - cost - eps, read from the prices
//                    of the phase's start and written to the other price buffer (every node writes its price there).  Below the floor: the infeasible flag.
//   k_mf_hub_count, k_mf_hub_mark, k_mf_hub_tables   the hubs of a solve -- the nodes whose list is longer than hubDeg -- found once behind k_mf_starts: counted,
//                    then ranked by the project's scan (ascending node number, the same tables on every run): per hub its node and its first tile, per tile of
//                    MF_HUB_TILE consecutive entries its hub and its first entry.
//   k_mf_hub_sum, k_mf_hub_push   the push of a hub's list by a workgroup per tile, in two launches over the tile table: per tile the sum of its admissible
//                    residuals and per hub a snapshot of its excess; then every tile adds up the sums of the hub's earlier tiles (its base), and clips its entries'
//                    amounts against the snapshot behind that base -- the serial walk's amounts, number for number.
//   k_mf_hub_rel, k_mf_hub_rel_fin   the relabel of a hub with excess > 0, behind k_mf_relabel: per tile the pair (any admissible entry, max of p(head) - cost - eps
//                    over residual entries), then a workgroup per hub combines the pairs and writes as k_mf_relabel does.
//   k_mf_pu_init, k_mf_pu_relax, k_mf_pu_apply   the price update: distances to the nodes with excess < 0, one thread per entry and an integer atomic min
//                    per improvement, launched until a launch changes nothing; the distances are unique, so the order of the improvements does not matter.
//   k_mf_lds         the whole solve by one workgroup between __syncthreads(), for networks of at most MF_LDS_NODES nodes and MF_LDS_ENTRIES entries; the same
//                    rounds and price updates; the round budget is its loop bound.  64-bit prices only: its LDS does not double into a workgroup's share.
//   k_mf_flows, k_mf_triples   flow per arc (lower + residual of the backward entry); the `from to flow` lines for k_cc_apply
// No kernel waits for another workgroup; every loop is bounded by a list length, an argument or the round budget.
// =============================================================================================

struct McfArc { u32 from, to; int lower, upper; long long cost; };                    // = sage2ov_mcf_arc
constexpr u32 MF_BLOCK = 256, MF_LANE_DEG = 64;
constexpr u32 MF_HUB_TILE = 2048;                                                      // entries of a hub's list per workgroup of the hub form
static_assert(MF_HUB_TILE % MF_BLOCK == 0, "a tile is whole chunks of the workgroup's walk");
constexpr u32 MF_NO_HUBS = 0xFFFFFFFFu;                                                // hubDeg of the round kernels when the hub form is off: no list is longer
constexpr u32 MF_LDS_NODES = 512, MF_LDS_ENTRIES = 2048;
constexpr int MF_ALPHA = 8;
constexpr u32 MF_PERIOD = 64;                                                          // rounds of a refine between two price updates; the first precedes its first round
constexpr u32 MF_BATCH = 32;                                                           // rounds between two reads of the counter block
// the counter block
constexpr u32 MF_ACT = 0, MF_PUSHES = MF_BATCH, MF_RELABELS = MF_BATCH + 1, MF_FLAGS = MF_BATCH + 2, MF_MAXC = MF_BATCH + 3, MF_ROUNDS = MF_BATCH + 4, MF_PHASES = MF_BATCH + 5,
              MF_TTS = MF_BATCH + 6, MF_UPDATES = MF_BATCH + 7, MF_HUBS = MF_BATCH + 8, MF_HUB_TILES = MF_BATCH + 9, MF_HUB_PUSHES = MF_BATCH + 10, MF_HUB_RELABELS = MF_BATCH + 11,
              MF_CTRS = MF_BATCH + 12;
constexpr unsigned long long MF_F_BADARC = 1, MF_F_NAN = 2, MF_F_INFEASIBLE = 4, MF_F_RANGE = 8, MF_F_LIMIT = 16;
constexpr long long MF_INF = 1ll << 62;                                                // the distance of a node that reaches no deficit; the bound of 64-bit prices
typedef __int128 i128;
template <class P> __host__ __device__ constexpr P mf_inf() { return (P)1 << (8 * sizeof(P) - 2); }      // the bound of the prices: 2^62, 2^126

struct MfNet {                   // the sorted layout and the state of a solve.  cost: scaled for 64-bit prices, unscaled for 128-bit ones (scale: the factor)
    const u32 *head, *sis, *tail, *start; const long long* cost; int* rcap;
    long long *excess, *delta; u32 n, M; long long scale;
};
template <class P> __device__ __forceinline__ P mf_cost(const MfNet& N, u32 s) {
    if constexpr (sizeof(P) == 16) return (P)N.cost[s] * (P)N.scale; else return N.cost[s];
}
__device__ __forceinline__ long long mf_shfl_down(long long x, int d) { return __shfl_down(x, d); }
__device__ __forceinline__ i128 mf_shfl_down(i128 x, int d) {                          // as two 64-bit halves
    const unsigned long long lo = __shfl_down((unsigned long long)x, d); const long long hi = __shfl_down((long long)(x >> 64), d);
    return ((i128)hi << 64) | (i128)lo;
}
// the length of an entry in the price update, for cp >= 0: min(cp / eps + 1, cap), exactly.  capEps = cap * eps
__device__ __forceinline__ long long mf_len(long long cp, long long eps, long long, long long cap) { const long long len = cp / eps + 1; return len > cap ? cap : len; }
// 128 bits: at cap * eps or above the length is cap.  Below it the quotient is under cap < 2^36: a quotient of doubles (relative error below 2^-49, so off by
// less than one) is within one of it, and the remainder says which way; two steps either way are allowed for.  q * eps <= cp + 2 eps: no overflow.
__device__ __forceinline__ long long mf_len(i128 cp, i128 eps, i128 capEps, long long cap) {
    if (cp >= capEps) return cap;
    const double two64 = 18446744073709551616.0;
    const double a = (double)(unsigned long long)(cp >> 64) * two64 + (double)(unsigned long long)cp, b = (double)(unsigned long long)(eps >> 64) * two64 + (double)(unsigned long long)eps;
    long long q = (long long)(a / b);
    i128 r = cp - (i128)q * eps;
    for (int i = 0; i < 2; i++) { if (r < 0) { q--; r += eps; } else if (r >= eps) { q++; r -= eps; } }
    return q + 1;                                                                      // (q < cap)
}

__global__ void k_mf_from_cc(const CcArc* __restrict__ in, u64 m, McfArc* out, unsigned long long* ctr) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (i >= m) return;
    const CcArc a = in[i]; long long c = 0;
    if (!(fabsf(a.cost) < 4.0e18f)) atomicOr(&ctr[MF_FLAGS], a.cost != a.cost || fabsf(a.cost) > 3.0e38f ? MF_F_NAN : MF_F_RANGE);
    else c = (long long)a.cost;                                                        // truncation towards zero
    out[i] = McfArc{a.from, a.to, a.lower, a.upper, c};
}
__global__ void k_mf_check(const McfArc* __restrict__ a, u64 m, u32 n, unsigned long long* ctr) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long mx = 0; bool bad = false;
    if (i < m) {
        const McfArc x = a[i];
        bad = x.from < 1 || x.from > n || x.to < 1 || x.to > n || x.from == x.to || x.lower < 0 || x.lower > x.upper;
        mx = x.cost < 0 ? 0ull - (unsigned long long)x.cost : (unsigned long long)x.cost;
    }
    for (int d = 32; d >= 1; d >>= 1) { const unsigned long long t = __shfl_down(mx, d); mx = t > mx ? t : mx; }
    const u64 anyBad = __ballot(bad);
    if (lane_id() == 0) { if (mx) atomicMax(&ctr[MF_MAXC], mx); if (anyBad) atomicOr(&ctr[MF_FLAGS], MF_F_BADARC); }
}
// (after k_mf_check has passed: every node number is inside 1..n)
__global__ void k_mf_keys(const McfArc* __restrict__ a, u64 m, u64* key, long long* excess) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (i >= m) return;
    const McfArc x = a[i];
    key[2 * i] = x.from; key[2 * i + 1] = x.to;
    if (x.lower) { atomicAdd((unsigned long long*)&excess[x.from], 0ull - (unsigned long long)x.lower); atomicAdd((unsigned long long*)&excess[x.to], (unsigned long long)x.lower); }
}
__global__ void k_mf_pos(const u32* __restrict__ idx, u32 M, u32* pos) { const u32 s = blockIdx.x * blockDim.x + threadIdx.x; if (s < M) pos[idx[s]] = s; }
__global__ void k_mf_entries(const McfArc* __restrict__ a, const u32* __restrict__ idx, const u32* __restrict__ pos, const u64* __restrict__ ks, u32 M, long long scale,
                             u32* head, u32* sis, u32* tail, long long* cost, int* rcap) {
    const u32 s = blockIdx.x * blockDim.x + threadIdx.x; if (s >= M) return;
    const u32 e = idx[s]; const McfArc x = a[e >> 1]; const bool back = e & 1u;
    head[s] = back ? x.from : x.to; tail[s] = (u32)ks[s]; sis[s] = pos[e ^ 1u];
    cost[s] = (back ? -x.cost : x.cost) * scale; rcap[s] = back ? 0 : x.upper - x.lower;
}
// start[v], v = 0 .. n + 1: the first sorted entry whose tail is v or more
__global__ void k_mf_starts(const u64* __restrict__ ks, u32 M, u32 n, u32* start) {
    const u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (v > (u64)n + 1) return;
    u32 lo = 0, hi = M;
    while (lo < hi) { const u32 mid = lo + ((hi - lo) >> 1); if (ks[mid] < v) lo = mid + 1; else hi = mid; }
    start[v] = lo;
}

__device__ __forceinline__ void mf_add(long long* p, long long x) { atomicAdd((unsigned long long*)p, (unsigned long long)x); }

template <class P> __global__ void k_mf_saturate(MfNet N, const P* __restrict__ p) {
    const u32 s = blockIdx.x * blockDim.x + threadIdx.x; if (s >= N.M) return;
    const int r = N.rcap[s]; if (r <= 0) return;
    const u32 v = N.tail[s], w = N.head[s];
    if (mf_cost<P>(N, s) + p[v] - p[w] >= 0) return;
    N.rcap[s] = 0; N.rcap[N.sis[s]] += r;                                              // (the sister's reduced cost is positive: its own thread leaves it alone)
    mf_add(&N.excess[v], -(long long)r); mf_add(&N.excess[w], (long long)r);
}

// exclusive scan of x over the MF_BLOCK threads of the workgroup; *total: the sum.  wsum: MF_BLOCK / 64 words of LDS
__device__ __forceinline__ long long mf_block_scan(long long x, long long* wsum, long long* total) {
    const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    long long inc = x;
    for (int d = 1; d < 64; d <<= 1) { const long long t = __shfl_up(inc, d); if (lane >= (u32)d) inc += t; }
    if (lane == 63u) wsum[w] = inc;
    __syncthreads();
    long long base = 0, tot = 0;
    for (u32 i = 0; i < MF_BLOCK / 64; i++) { const long long s = wsum[i]; if (i < w) base += s; tot += s; }
    __syncthreads();
    *total = tot; return base + inc - x;
}

template <class P> __global__ void __launch_bounds__(MF_BLOCK) k_mf_push(MfNet N, const P* __restrict__ p, u32 hubDeg, unsigned long long* ctr) {
    __shared__ u32 hv[MF_BLOCK]; __shared__ u32 nhv, sPush; __shared__ long long wsum[MF_BLOCK / 64];
    const u32 tid = threadIdx.x; const u64 v64 = (u64)blockIdx.x * MF_BLOCK + tid + 1;
    if (tid == 0) { nhv = 0; sPush = 0; }
    __syncthreads();
    u32 np = 0;
    if (v64 <= N.n) {
        const u32 v = (u32)v64; long long e = N.excess[v];
        if (e > 0) {
            const u32 s0 = N.start[v], s1 = N.start[v + 1];
            if (s1 - s0 > MF_LANE_DEG) { if (s1 - s0 <= hubDeg) hv[atomicAdd(&nhv, 1u)] = v; }      // (a hub: k_mf_hub_sum / k_mf_hub_push)
            else {
                const P pv = p[v];
                for (u32 s = s0; s < s1 && e > 0; s++) {
                    const int r = N.rcap[s]; if (r <= 0) continue;
                    const u32 w = N.head[s];
                    if (mf_cost<P>(N, s) + pv - p[w] >= 0) continue;
                    const long long d = (long long)r < e ? (long long)r : e;
                    N.rcap[s] = r - (int)d; N.rcap[N.sis[s]] += (int)d;                // (only this node writes either: the sister is not admissible)
                    mf_add(&N.delta[w], d); e -= d; np++;
                }
                N.excess[v] = e;
            }
        }
    }
    __syncthreads();
    const u32 cnt = nhv;
    for (u32 k = 0; k < cnt; k++) {                                                    // the long lists of this workgroup's nodes, one after the other
        const u32 v = hv[k]; const long long e = N.excess[v]; const P pv = p[v]; const u32 s0 = N.start[v], s1 = N.start[v + 1];
        long long carry = 0;
        for (u32 b = s0; b < s1 && carry < e; b += MF_BLOCK) {
            const u32 s = b + tid; long long amt = 0; u32 w = 0; int r = 0;
            if (s < s1) { r = N.rcap[s]; if (r > 0) { w = N.head[s]; if (mf_cost<P>(N, s) + pv - p[w] < 0) amt = r; } }
            long long tot; const long long ex = mf_block_scan(amt, wsum, &tot);
            const long long room = e - (carry + ex); long long d = amt < room ? amt : room; if (d < 0) d = 0;
            if (d > 0) { N.rcap[s] = r - (int)d; N.rcap[N.sis[s]] += (int)d; mf_add(&N.delta[w], d); np++; }
            carry += tot;
        }
        __syncthreads();
        if (tid == 0) N.excess[v] = e - (carry < e ? carry : e);
    }
    if (np) atomicAdd(&sPush, np);
    __syncthreads();
    if (tid == 0 && sPush) atomicAdd(&ctr[MF_PUSHES], (unsigned long long)sPush);
}

// act: the word that counts the nodes with excess > 0 of this round
template <class P> __global__ void __launch_bounds__(MF_BLOCK) k_mf_relabel(MfNet N, const P* __restrict__ p, P* pn, P eps, P floor, u32 hubDeg, unsigned long long* act, unsigned long long* ctr) {
    __shared__ u32 hv[MF_BLOCK]; __shared__ u32 nhv, sAct, sRel, sBad; __shared__ P wbest[MF_BLOCK / 64]; __shared__ u32 wadm[MF_BLOCK / 64];
    const u32 tid = threadIdx.x; const u64 v64 = (u64)blockIdx.x * MF_BLOCK + tid + 1;
    if (tid == 0) { nhv = 0; sAct = 0; sRel = 0; sBad = 0; }
    __syncthreads();
    if (v64 <= N.n) {
        const u32 v = (u32)v64; const long long dl = N.delta[v]; long long e = N.excess[v];
        if (dl) { e += dl; N.excess[v] = e; N.delta[v] = 0; }
        P pv = p[v];
        if (e > 0) {
            atomicAdd(&sAct, 1u);
            const u32 s0 = N.start[v], s1 = N.start[v + 1];
            if (s1 - s0 > MF_LANE_DEG) { if (s1 - s0 <= hubDeg) hv[atomicAdd(&nhv, 1u)] = v; }      // (a hub: k_mf_hub_rel / k_mf_hub_rel_fin)
            else {
                bool adm = false; P best = -mf_inf<P>();
                for (u32 s = s0; s < s1; s++) {
                    if (N.rcap[s] <= 0) continue;
                    const P pw = p[N.head[s]], c = mf_cost<P>(N, s);
                    if (c + pv - pw < 0) { adm = true; break; }
                    const P x = pw - c - eps; best = x > best ? x : best;
                }
                if (!adm) { if (best < floor) atomicOr(&sBad, 1u); else { pv = best; atomicAdd(&sRel, 1u); } }
            }
        }
        pn[v] = pv;                                                                    // (a long list's node: overwritten below, a hub's by k_mf_hub_rel_fin, when it is relabelled)
    }
    __syncthreads();
    const u32 cnt = nhv;
    for (u32 k = 0; k < cnt; k++) {
        const u32 v = hv[k]; const P pv = p[v]; const u32 s0 = N.start[v], s1 = N.start[v + 1];
        bool adm = false; P best = -mf_inf<P>();
        for (u32 s = s0 + tid; s < s1; s += MF_BLOCK) {
            if (N.rcap[s] <= 0) continue;
            const P pw = p[N.head[s]], c = mf_cost<P>(N, s);
            if (c + pv - pw < 0) { adm = true; break; }
            const P x = pw - c - eps; best = x > best ? x : best;
        }
        for (int d = 32; d >= 1; d >>= 1) { const P t = mf_shfl_down(best, d); best = t > best ? t : best; }
        const u64 anyAdm = __ballot(adm);
        if ((tid & 63u) == 0) { wbest[tid >> 6] = best; wadm[tid >> 6] = anyAdm ? 1u : 0u; }
        __syncthreads();
        if (tid == 0) {
            bool a = false; P b = -mf_inf<P>();
            for (u32 i = 0; i < MF_BLOCK / 64; i++) { a = a || wadm[i]; b = wbest[i] > b ? wbest[i] : b; }
            if (!a) { if (b < floor) sBad = 1u; else { pn[v] = b; sRel += 1u; } }
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (sAct) atomicAdd(act, (unsigned long long)sAct);
        if (sRel) atomicAdd(&ctr[MF_RELABELS], (unsigned long long)sRel);
        if (sBad) atomicOr(&ctr[MF_FLAGS], MF_F_INFEASIBLE);
    }
}

// ---- the hub form: lists longer than hubDeg, a workgroup per tile of MF_HUB_TILE entries.  The method and every number it produces are k_mf_push's and
// k_mf_relabel's; what differs is who walks the list.  As everywhere in this file no workgroup waits for another: what one launch hands to the next goes through
// memory and the order of the launches in the stream.
struct MfHubs {                  // node[h]: the h-th hub in ascending node number; tile0[h] .. tile0[h + 1]: its tiles; tileHub[t], tileBeg[t]: a tile's hub, its first entry
    const u32 *node, *tile0, *tileHub, *tileBeg; long long *snap, *tsum; u32 H, T;
};
__device__ __forceinline__ u32 mf_hub_tiles(u32 deg) { return (deg + MF_HUB_TILE - 1) / MF_HUB_TILE; }
// the two counts, for the host to size the tables by (sums of integers: the same on every run)
__global__ void k_mf_hub_count(const u32* __restrict__ start, u32 n, u32 hubDeg, unsigned long long* ctr) {
    const u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x + 1;
    u32 tiles = 0;
    if (v <= n) { const u32 deg = start[v + 1] - start[v]; if (deg > hubDeg) tiles = mf_hub_tiles(deg); }
    const u64 hubs = __ballot(tiles != 0);
    u32 t = tiles; for (int d = 32; d >= 1; d >>= 1) t += __shfl_down(t, d);
    if (lane_id() == 0 && hubs) { atomicAdd(&ctr[MF_HUBS], (unsigned long long)__popcll(hubs)); atomicAdd(&ctr[MF_HUB_TILES], (unsigned long long)t); }
}
// isHub[v - 1], nTiles[v - 1]: the inputs of the two scans
__global__ void k_mf_hub_mark(const u32* __restrict__ start, u32 n, u32 hubDeg, u32* isHub, u32* nTiles) {
    const u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x + 1; if (v > n) return;
    const u32 deg = start[v + 1] - start[v]; const bool hub = deg > hubDeg;
    isHub[v - 1] = hub ? 1u : 0u; nTiles[v - 1] = hub ? mf_hub_tiles(deg) : 0u;
}
// rank, tileRank: the exclusive scans of the two.  A hub's thread fills its own tiles: at most list length / MF_HUB_TILE + 1 of them
__global__ void k_mf_hub_tables(const u32* __restrict__ start, u32 n, u32 hubDeg, const u32* __restrict__ rank, const u32* __restrict__ tileRank, u32 H, u32 T,
                                u32* node, u32* tile0, u32* tileHub, u32* tileBeg) {
    const u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x + 1; if (v > n) return;
    if (v == 1) tile0[H] = T;
    const u32 s0 = start[v], deg = start[v + 1] - s0; if (deg <= hubDeg) return;
    const u32 h = rank[v - 1], t0 = tileRank[v - 1], nt = mf_hub_tiles(deg);
    if (h >= H || t0 > T || nt > T - t0) return;                                       // (the counts the tables were sized by are sums of the same numbers)
    node[h] = (u32)v; tile0[h] = t0;
    for (u32 t = 0; t < nt; t++) { tileHub[t0 + t] = h; tileBeg[t0 + t] = s0 + t * MF_HUB_TILE; }
}

// the sum of x over the workgroup, in every thread.  wsum: MF_BLOCK / 64 words of LDS
__device__ __forceinline__ long long mf_block_sum(long long x, long long* wsum) {
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d);
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = x;
    __syncthreads();
    long long tot = 0; for (u32 i = 0; i < MF_BLOCK / 64; i++) tot += wsum[i];
    __syncthreads();
    return tot;
}
// The push over a hub, first launch (grid: the tiles).  tsum[t]: the admissible residuals of tile t (residual > 0, reduced cost < 0, the prices of the round's
// start); snap[h]: the hub's excess as this round found it.  Tiles of a hub without excess write no sum: nobody reads it.
template <class P> __global__ void __launch_bounds__(MF_BLOCK) k_mf_hub_sum(MfNet N, MfHubs Hb, const P* __restrict__ p) {
    __shared__ long long wsum[MF_BLOCK / 64];
    const u32 b = blockIdx.x, tid = threadIdx.x; if (b >= Hb.T) return;
    const u32 h = Hb.tileHub[b], v = Hb.node[h];
    const long long e = N.excess[v];                                                   // (nobody writes it in this launch)
    if (tid == 0 && b == Hb.tile0[h]) Hb.snap[h] = e;
    if (e <= 0) return;
    const P pv = p[v]; const u32 t0 = Hb.tileBeg[b], end = N.start[v + 1], s1 = end - t0 > MF_HUB_TILE ? t0 + MF_HUB_TILE : end;
    long long sum = 0;
    for (u32 s = t0 + tid; s < s1; s += MF_BLOCK) { const int r = N.rcap[s]; if (r > 0 && mf_cost<P>(N, s) + pv - p[N.head[s]] < 0) sum += r; }
    sum = mf_block_sum(sum, wsum);
    if (tid == 0) Hb.tsum[b] = sum;
}
// Second launch (grid: the tiles).  A tile's base is the sum of its hub's earlier tile sums, added up by the tile's own workgroup; behind that base the tile walks its
// entries as k_mf_push walks a long list: the amounts are the serial walk's.  Two things make this exact:
//  1. every tile clips against the snapshot, never against excess[v], which one thread of this same launch -- the hub's last tile -- overwrites;
//  2. both launches see the same admissible set.  An entry admissible for the hub has a sister of positive reduced cost, which nobody pushes along, so its residual
//     word has no writer in the round but the tile that owns it here, whatever k_mf_push does to the hub's other entries through their sisters.
template <class P> __global__ void __launch_bounds__(MF_BLOCK) k_mf_hub_push(MfNet N, MfHubs Hb, const P* __restrict__ p, unsigned long long* ctr) {
    __shared__ long long wsum[MF_BLOCK / 64]; __shared__ u32 sPush;
    const u32 b = blockIdx.x, tid = threadIdx.x; if (b >= Hb.T) return;
    const u32 h = Hb.tileHub[b], v = Hb.node[h];
    const long long e = Hb.snap[h]; if (e <= 0) return;
    if (tid == 0) sPush = 0;
    const u32 first = Hb.tile0[h], last = Hb.tile0[h + 1] - 1;
    long long base = 0;
    for (u32 t = first + tid; t < b; t += MF_BLOCK) base += Hb.tsum[t];
    base = mf_block_sum(base, wsum);
    if (tid == 0 && b == last) { const long long total = base + Hb.tsum[b]; N.excess[v] = e - (total < e ? total : e); }
    if (base >= e) return;                                                             // the excess ends in front of this tile
    const P pv = p[v]; const u32 t0 = Hb.tileBeg[b], end = N.start[v + 1], s1 = end - t0 > MF_HUB_TILE ? t0 + MF_HUB_TILE : end;
    long long carry = base; u32 np = 0;
    for (u32 c = t0; c < s1 && carry < e; c += MF_BLOCK) {
        const u32 s = c + tid; long long amt = 0; u32 w = 0; int r = 0;
        if (s < s1) { r = N.rcap[s]; if (r > 0) { w = N.head[s]; if (mf_cost<P>(N, s) + pv - p[w] < 0) amt = r; } }
        long long tot; const long long ex = mf_block_scan(amt, wsum, &tot);
        const long long room = e - (carry + ex); long long d = amt < room ? amt : room; if (d < 0) d = 0;
        if (d > 0) { N.rcap[s] = r - (int)d; N.rcap[N.sis[s]] += (int)d; mf_add(&N.delta[w], d); np++; }
        carry += tot;
    }
    if (np) atomicAdd(&sPush, np);
    __syncthreads();
    if (tid == 0 && sPush) { atomicAdd(&ctr[MF_PUSHES], (unsigned long long)sPush); atomicAdd(&ctr[MF_HUB_PUSHES], (unsigned long long)sPush); }
}
// The relabel over a hub, behind k_mf_relabel (which has added delta to the excess and written pn[v] = p[v]).  First launch (grid: the tiles): k_mf_relabel's pair per
// tile.  Tiles of a hub without excess write nothing.
template <class P> __global__ void __launch_bounds__(MF_BLOCK) k_mf_hub_rel(MfNet N, MfHubs Hb, const P* __restrict__ p, P eps, P* tbest, u32* tadm) {
    __shared__ P wbest[MF_BLOCK / 64]; __shared__ u32 wadm[MF_BLOCK / 64];
    const u32 b = blockIdx.x, tid = threadIdx.x; if (b >= Hb.T) return;
    const u32 h = Hb.tileHub[b], v = Hb.node[h];
    if (N.excess[v] <= 0) return;
    const P pv = p[v]; const u32 t0 = Hb.tileBeg[b], end = N.start[v + 1], s1 = end - t0 > MF_HUB_TILE ? t0 + MF_HUB_TILE : end;
    bool adm = false; P best = -mf_inf<P>();
    for (u32 s = t0 + tid; s < s1; s += MF_BLOCK) {
        if (N.rcap[s] <= 0) continue;
        const P pw = p[N.head[s]], c = mf_cost<P>(N, s);
        if (c + pv - pw < 0) { adm = true; break; }
        const P x = pw - c - eps; best = x > best ? x : best;
    }
    for (int d = 32; d >= 1; d >>= 1) { const P t = mf_shfl_down(best, d); best = t > best ? t : best; }      // (128 bits: as two halves)
    const u64 anyAdm = __ballot(adm);
    if ((tid & 63u) == 0) { wbest[tid >> 6] = best; wadm[tid >> 6] = anyAdm ? 1u : 0u; }
    __syncthreads();
    if (tid == 0) {
        bool a = false; P m = -mf_inf<P>();
        for (u32 i = 0; i < MF_BLOCK / 64; i++) { a = a || wadm[i]; m = wbest[i] > m ? wbest[i] : m; }
        tbest[b] = m; tadm[b] = a ? 1u : 0u;
    }
}
// Second launch (grid: the hubs): the pairs of a hub's tiles combined, and the result written as k_mf_relabel writes it
template <class P> __global__ void __launch_bounds__(MF_BLOCK) k_mf_hub_rel_fin(MfNet N, MfHubs Hb, const P* __restrict__ tbest, const u32* __restrict__ tadm, P floor, P* pn, unsigned long long* ctr) {
    __shared__ P wbest[MF_BLOCK / 64]; __shared__ u32 wadm[MF_BLOCK / 64];
    const u32 h = blockIdx.x, tid = threadIdx.x; if (h >= Hb.H) return;
    const u32 v = Hb.node[h];
    if (N.excess[v] <= 0) return;
    bool adm = false; P best = -mf_inf<P>();
    for (u32 t = Hb.tile0[h] + tid, t1 = Hb.tile0[h + 1]; t < t1; t += MF_BLOCK) { adm = adm || tadm[t]; const P x = tbest[t]; best = x > best ? x : best; }
    for (int d = 32; d >= 1; d >>= 1) { const P t = mf_shfl_down(best, d); best = t > best ? t : best; }
    const u64 anyAdm = __ballot(adm);
    if ((tid & 63u) == 0) { wbest[tid >> 6] = best; wadm[tid >> 6] = anyAdm ? 1u : 0u; }
    __syncthreads();
    if (tid == 0) {
        bool a = false; P m = -mf_inf<P>();
        for (u32 i = 0; i < MF_BLOCK / 64; i++) { a = a || wadm[i]; m = wbest[i] > m ? wbest[i] : m; }
        if (!a) {
            if (m < floor) atomicOr(&ctr[MF_FLAGS], MF_F_INFEASIBLE);
            else { pn[v] = m; atomicAdd(&ctr[MF_RELABELS], 1ull); atomicAdd(&ctr[MF_HUB_RELABELS], 1ull); }
        }
    }
}

// ---- the price update
__global__ void k_mf_pu_init(const long long* __restrict__ excess, u32 n, long long* dist) {
    const u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (v > (u64)n + 1) return;
    dist[v] = (v >= 1 && v <= n && excess[v] < 0) ? 0 : MF_INF;
}
// one pass over the entries; changed: the improvements of this launch
template <class P> __global__ void k_mf_pu_relax(MfNet N, const P* __restrict__ p, P eps, P capEps, long long cap, long long* dist, unsigned long long* changed) {
    const u32 s = blockIdx.x * blockDim.x + threadIdx.x;
    bool ch = false;
    if (s < N.M && N.rcap[s] > 0) {
        const u32 v = N.tail[s], w = N.head[s];
        const long long dw = dist[w];
        if (dw < cap) {
            const P cp = mf_cost<P>(N, s) + p[v] - p[w];
            long long len = 0; if (cp >= 0) len = mf_len(cp, eps, capEps, cap);
            const long long c = dw + len;
            if (c < dist[v]) { atomicMin((unsigned long long*)&dist[v], (unsigned long long)c); ch = true; }      // (distances are never negative)
        }
    }
    const u64 m = __ballot(ch);
    if (lane_id() == 0 && m) atomicAdd(changed, (unsigned long long)__popcll(m));
}
template <class P> __global__ void k_mf_pu_apply(const long long* __restrict__ excess, const long long* __restrict__ dist, u32 n, P eps, long long cap, P* p, unsigned long long* ctr) {
    const u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (v < 1 || v > n) return;
    long long d = dist[v];
    if (d >= MF_INF && excess[v] > 0) atomicOr(&ctr[MF_FLAGS], MF_F_INFEASIBLE);       // excess that reaches no deficit
    if (d > cap) d = cap;
    p[v] -= eps * (P)d;
}

// ---- the single-workgroup form
struct MfLdsArgs { long long cmax, scale; unsigned long long maxRounds; u32 period; };
__global__ void __launch_bounds__(MF_BLOCK) k_mf_lds(MfNet N, long long* pOut, MfLdsArgs A, unsigned long long* ctr) {
    __shared__ long long cost[MF_LDS_ENTRIES]; __shared__ int rcap[MF_LDS_ENTRIES]; __shared__ unsigned short head[MF_LDS_ENTRIES], sis[MF_LDS_ENTRIES], tail[MF_LDS_ENTRIES];
    __shared__ long long price[2][MF_LDS_NODES + 2], excess[MF_LDS_NODES + 2], delta[MF_LDS_NODES + 2]; __shared__ u32 start[MF_LDS_NODES + 3];
    __shared__ long long dist[MF_LDS_NODES + 2];
    __shared__ u32 sAct, sBad, sChg; __shared__ unsigned long long sPush, sRel;
    const u32 tid = threadIdx.x, n = N.n, M = N.M;
    if (n > MF_LDS_NODES || M > MF_LDS_ENTRIES) return;                                 // (the host does not launch it then)
    for (u32 s = tid; s < M; s += MF_BLOCK) { cost[s] = N.cost[s]; rcap[s] = N.rcap[s]; head[s] = (unsigned short)N.head[s]; sis[s] = (unsigned short)N.sis[s]; tail[s] = (unsigned short)N.tail[s]; }
    for (u32 v = tid; v <= n + 1; v += MF_BLOCK) { price[0][v] = 0; price[1][v] = 0; excess[v] = N.excess[v]; delta[v] = 0; start[v] = N.start[v]; }
    if (tid == 0) { sAct = 0; sBad = 0; sChg = 0; sPush = 0; sRel = 0; }
    __syncthreads();
    const long long cap = (long long)(1 + MF_ALPHA) * A.scale;
    unsigned long long rounds = 0, phases = 0, flags = 0, updates = 0; u32 cur = 0; long long floor = 0;
    for (long long eps = A.cmax;;) {
        phases++; floor -= (long long)(1 + MF_ALPHA) * A.scale * eps;
        {
            const long long* p = price[cur];
            for (u32 s = tid; s < M; s += MF_BLOCK) {
                const int r = rcap[s]; if (r <= 0) continue;
                const u32 v = tail[s], w = head[s];
                if (cost[s] + p[v] - p[w] >= 0) continue;
                rcap[s] = 0; rcap[sis[s]] += r; mf_add(&excess[v], -(long long)r); mf_add(&excess[w], (long long)r);
            }
        }
        __syncthreads();
        u32 since = A.period;
        for (;;) {
            if (rounds == A.maxRounds) { flags |= MF_F_LIMIT; break; }
            if (A.period && since >= A.period) {                                       // the price update (k_mf_pu_*)
                since = 0; floor -= cap * eps;
                if (floor < -(MF_INF - 2 * A.cmax - 1)) { flags |= MF_F_RANGE; break; }
                long long* pc = price[cur];
                for (u32 v = tid; v <= n + 1; v += MF_BLOCK) dist[v] = (v >= 1 && v <= n && excess[v] < 0) ? 0 : MF_INF;
                __syncthreads();
                for (u32 it = 0; it <= n + 1; it++) {                                  // (a shortest path has at most n - 1 entries)
                    bool ch = false;
                    for (u32 s = tid; s < M; s += MF_BLOCK) {
                        if (rcap[s] <= 0) continue;
                        const u32 v = tail[s], w = head[s]; const long long dw = dist[w]; if (dw >= cap) continue;
                        const long long cp = cost[s] + pc[v] - pc[w];
                        long long len = 0; if (cp >= 0) { len = cp / eps + 1; if (len > cap) len = cap; }
                        const long long c = dw + len;
                        if (c < dist[v]) { atomicMin((unsigned long long*)&dist[v], (unsigned long long)c); ch = true; }
                    }
                    if (ch) atomicOr(&sChg, 1u);
                    __syncthreads();
                    const u32 c = sChg;
                    __syncthreads();
                    if (tid == 0) sChg = 0;
                    if (!c) break;
                }
                for (u32 v = 1 + tid; v <= n; v += MF_BLOCK) {
                    long long d = dist[v];
                    if (d >= MF_INF && excess[v] > 0) atomicOr(&sBad, 1u);
                    if (d > cap) d = cap;
                    pc[v] -= eps * d;
                }
                updates++;
                __syncthreads();
                if (sBad) { flags |= MF_F_INFEASIBLE; break; }
            }
            since++;
            rounds++;
            const long long* p = price[cur]; long long* pn = price[cur ^ 1u];
            u32 np = 0, nr = 0;
            for (u32 v = 1 + tid; v <= n; v += MF_BLOCK) {                             // push
                long long e = excess[v]; if (e <= 0) continue;
                const long long pv = p[v];
                for (u32 s = start[v], s1 = start[v + 1]; s < s1 && e > 0; s++) {
                    const int r = rcap[s]; if (r <= 0) continue;
                    const u32 w = head[s];
                    if (cost[s] + pv - p[w] >= 0) continue;
                    const long long d = (long long)r < e ? (long long)r : e;
                    rcap[s] = r - (int)d; rcap[sis[s]] += (int)d; mf_add(&delta[w], d); e -= d; np++;
                }
                excess[v] = e;
            }
            __syncthreads();
            for (u32 v = 1 + tid; v <= n; v += MF_BLOCK) {                             // relabel
                const long long e = excess[v] + delta[v]; excess[v] = e; delta[v] = 0;
                long long pv = p[v];
                if (e > 0) {
                    atomicAdd(&sAct, 1u);
                    bool adm = false; long long best = -MF_INF;
                    for (u32 s = start[v], s1 = start[v + 1]; s < s1; s++) {
                        if (rcap[s] <= 0) continue;
                        const long long pw = p[head[s]], c = cost[s];
                        if (c + pv - pw < 0) { adm = true; break; }
                        const long long x = pw - c - eps; best = x > best ? x : best;
                    }
                    if (!adm) { if (best < floor) atomicOr(&sBad, 1u); else { pv = best; nr++; } }
                }
                pn[v] = pv;
            }
            if (np) atomicAdd(&sPush, (unsigned long long)np);
            if (nr) atomicAdd(&sRel, (unsigned long long)nr);
            __syncthreads();
            const u32 act = sAct, bad = sBad;
            __syncthreads();
            if (tid == 0) sAct = 0;
            cur ^= 1u;
            if (bad) { flags |= MF_F_INFEASIBLE; break; }
            if (!act) break;
        }
        if (flags || eps == 1) break;
        eps = eps / MF_ALPHA; if (eps < 1) eps = 1;
    }
    __syncthreads();
    for (u32 s = tid; s < M; s += MF_BLOCK) N.rcap[s] = rcap[s];
    for (u32 v = tid; v <= n + 1; v += MF_BLOCK) pOut[v] = price[cur][v];
    if (tid == 0) { ctr[MF_ROUNDS] = rounds; ctr[MF_PHASES] = phases; ctr[MF_PUSHES] = sPush; ctr[MF_RELABELS] = sRel; ctr[MF_UPDATES] = updates; if (flags) atomicOr(&ctr[MF_FLAGS], flags); }
}

// flow[i] = lower + what the backward entry holds
__global__ void k_mf_flows(const McfArc* __restrict__ a, const u32* __restrict__ pos, const int* __restrict__ rcap, u64 m, long long* flow) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (i >= m) return;
    flow[i] = (long long)a[i].lower + (long long)rcap[pos[2 * i + 1]];
}
// the lines of output.cs2 for k_cc_apply: arcs with upper > 0 (cs2.cpp prints no other); an arc without a line becomes `1 1 0`, which the apply path skips as
// it skips every line on node 1.  ctr[MF_TTS]: the flow of the `2 1` arc
__global__ void k_mf_triples(const McfArc* __restrict__ a, const long long* __restrict__ flow, u64 m, u64* fr, u64* to, u64* fl, unsigned long long* ctr) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (i >= m) return;
    const McfArc x = a[i]; const bool line = x.upper > 0;
    fr[i] = line ? x.from : 1; to[i] = line ? x.to : 1; fl[i] = line ? (u64)flow[i] : 0;
    if (line && ((x.from == 2 && x.to == 1) || (x.from == 1 && x.to == 2))) ctr[MF_TTS] = (unsigned long long)flow[i];
}
