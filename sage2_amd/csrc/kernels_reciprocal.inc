// sage2_amd/csrc/kernels_reciprocal.inc -- reciprocal pass and reduce-phase support kernels.
// Part of sage2ov_device.hip (included inside namespace s2, in this order); not a translation unit of its own.

// =============================================================================================
// reciprocal pass (economyGraph.cpp:455-480), order-independent restatement:
//   cond(i) does not depend on the serial order; the `exploredReads[x]!=4` test at the time read i
//   is visited is true iff NOT (x < i and cond(x)).
// =============================================================================================
constexpr u64 ID_MASK = (1ull << 40) - 1;
constexpr int COND_PER_THREAD = 8;                // reads per thread: the three log counters cost three atomics per 2048 reads
// Round 3: the per-read records (right / left / conn / cflag) are indexed by POSITION in the locality order and name their neighbours by position, as the
// probe kernels produce them: a read's two neighbours are its neighbours in the genome, hence (mostly) a few lines away -- round 2 gathered their records
// by id, two random 128-byte lines per read, 2.3 ms at BASELINE configs[2] (now 1.1).  cond() is a statement about a read and its neighbours: the same in
// either numbering.  The status goes out by position (statusP: what the emit half, the hit-list kernels and the unresolved list read).  The copy by id that
// the reduce phase's by-id readers index is a random one-byte store per read: BY_ID = true writes it here (SAGE2OV_STATUS_EAGER=1, the A/B route); by default
// it is gathered from statusP when a reader first asks for it (k_status_by_id, ensure_status_by_id) -- on clean data nobody does.
template <bool BY_ID>
__global__ __launch_bounds__(256) void k_recip_cond(u64 N, const u64* __restrict__ right, const u64* __restrict__ left, const u32* __restrict__ conn,
                             const u32* __restrict__ cflag, const u32* __restrict__ idOf, uint8_t* status, uint8_t* statusP, u64* counters) {
    u64 ovs = 0; u32 ncond = 0, n6 = 0, n0 = 0;
#pragma unroll
    for (int it = 0; it < COND_PER_THREAD; it++) {
        const u64 p = (u64)blockIdx.x * (256 * COND_PER_THREAD) + (u64)it * 256 + threadIdx.x + 1;
        if (p <= N) {
            const u32 c = conn[p], cf = cflag[p]; const bool over = c > CONN_LIMIT;
            const bool is6 = (cf & 1u) || ((cf & 2u) && !over);        // single-thread outcome of the :444 / :735 writes
            const u64 l = left[p], r = right[p]; const u64 lp = l & ID_MASK, rp = r & ID_MASK;
            bool cond = false;
            if (!is6 && (l >> 42) != 0 && (r >> 42) != 0) {
                const bool lrec = ((right[lp] & ID_MASK) == p) || ((left[lp] & ID_MASK) == p);
                const bool rrec = ((right[rp] & ID_MASK) == p) || ((left[rp] & ID_MASK) == p);
                cond = lrec && rrec;
            }
            const uint8_t st = cond ? 4 : (is6 ? 6 : (over ? 5 : 0));
            statusP[p] = st; if (BY_ID) status[idOf[p]] = st;
            ovs += c; ncond += cond; n6 += is6; n0 += st == 0;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { statusP[0] = 0xFF; if (BY_ID) status[0] = 0; }     // (position 0: never unresolved; id 0 does not exist)
    // block reductions of the log counters and of the number of unresolved reads (what collect_unresolved sizes its list by): one atomic per counter per block
    __shared__ u64 red[4][4];
    u64 v0 = ovs, v1 = ncond, v2 = n6, v3 = n0;
    for (int d = 32; d; d >>= 1) { v0 += __shfl_xor(v0, d); v1 += __shfl_xor(v1, d); v2 += __shfl_xor(v2, d); v3 += __shfl_xor(v3, d); }
    const u32 w = threadIdx.x >> 6;
    if (lane_id() == 0) { red[0][w] = v0; red[1][w] = v1; red[2][w] = v2; red[3][w] = v3; }
    __syncthreads();
    if (threadIdx.x < 4) {
        u64 t = 0; for (u32 x = 0; x < 4; x++) t += red[threadIdx.x][x];
        if (t) atomicAdd(&counters[1 + threadIdx.x], t);
    }
}
__device__ __forceinline__ u32 flip_type(u32 t) { return t == 0 ? 3u : (t == 3 ? 0u : t); }   // utils.cpp:212
// read length: a constant when the data set has a single length (the usual case), else the low 9 bits of the slot's last word
__device__ __forceinline__ int read_len(const u64* __restrict__ reads, int S, u64 id, int uniL) { return uniL ? uniL : (int)(reads[id * S + S - 1] & slot_len_mask(S)); }
// (u, v: ids; Lu, Lv: their lengths)
__device__ __forceinline__ EdgeCand make_edge(int Lu, int Lv, u64 u, u64 v, u32 delta, u32 type) {
    EdgeCand e;
    if (u < v) { e.from = (u32)u; e.to = (u32)v; e.len = delta & 0xFFFFFu; e.type = type; }
    else { e.from = (u32)v; e.to = (u32)u; e.len = (u32)(Lu - (Lv - (int)delta)) & 0xFFFFFu; e.type = flip_type(type); }   // the twin lives in the smaller id's list (economyGraph.cpp:821)
    return e;
}
constexpr int EMIT_PER_THREAD = 16;               // reads per thread: a block of 256 threads reserves space for 4096 reads with ONE atomic
// positions [elo, ehi) of the locality order; `readsLoc`: the store in that order (lengths of mixed-length data sets).  (Walking the emitters in ID order
// instead -- candidates then come out with ascending `from`, which convert's atomics like: 3.4 instead of 4.9 ms -- costs the emit kernel 6.4 instead of 1.0 ms
// in scattered record loads: measured, dropped.)
__global__ __launch_bounds__(256) void k_recip_emit(u64 N, const u64* __restrict__ readsLoc, int S, int uniL, const u64* __restrict__ right, const u64* __restrict__ left,
                             const uint8_t* __restrict__ statusP, const u32* __restrict__ idOf, EdgeCand* cand, u64 cap, u64* counters, u64 elo, u64 ehi) {
    __shared__ u32 sh[4]; __shared__ u64 shBase;
    const u64 tile0 = (u64)blockIdx.x * (256 * EMIT_PER_THREAD) + elo;
    u32 flags = 0, mine = 0;
#pragma unroll
    for (int it = 0; it < EMIT_PER_THREAD; it++) {
        const u64 p = tile0 + (u64)it * 256 + threadIdx.x;
        if (p < ehi && p <= N && statusP[p] == 4) {
            const u64 l = left[p], r = right[p], lp = l & ID_MASK, rp = r & ID_MASK;
            const u32 i = idOf[p], lid = idOf[lp], rid = idOf[rp];
            const bool eL = lid != i && !(lid < i && statusP[lp] == 4);                     // :462-467 (and u != v, :815)
            const bool eR = rid != i && !(rid < i && statusP[rp] == 4);                     // :468-473
            flags |= ((eL ? 1u : 0u) | (eR ? 2u : 0u)) << (2 * it); mine += (eL ? 1u : 0u) + (eR ? 1u : 0u);
        }
    }
    u32 total; const u32 excl = block_excl_scan(mine, sh, total);
    if (total == 0) return;
    if (threadIdx.x == 0) shBase = atomicAdd(&counters[0], (u64)total);
    __syncthreads();
    u64 q = shBase + excl;
#pragma unroll
    for (int it = 0; it < EMIT_PER_THREAD; it++) {
        const u32 f = (flags >> (2 * it)) & 3u; if (!f) continue;
        const u64 p = tile0 + (u64)it * 256 + threadIdx.x;
        const u64 l = left[p], r = right[p], lp = l & ID_MASK, rp = r & ID_MASK;
        const u32 i = idOf[p]; const int Li = read_len(readsLoc, S, p, uniL);
        if (f & 1u) { if (q < cap) cand[q] = make_edge(Li, read_len(readsLoc, S, lp, uniL), i, idOf[lp], (u32)(l >> 42), ((l >> 40) & 3) == 0 ? 0u : 1u); q++; }
        if (f & 2u) { if (q < cap) cand[q] = make_edge(Li, read_len(readsLoc, S, rp, uniL), i, idOf[rp], (u32)(r >> 42), ((r >> 40) & 3) == 0 ? 3u : 2u); q++; }
    }
}

// reduce-phase support: the host replay needs the lists of unresolved reads and of their neighbours
__global__ void k_red_mark(const EdgeCand* __restrict__ cand, u64 n, const uint8_t* __restrict__ status, uint8_t* need) {
    u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (x >= n) return;
    EdgeCand e = cand[x];
    if (status[e.from] == 0 || status[e.to] == 0) { need[e.from] = 1; need[e.to] = 1; }
}
__global__ void k_red_collect(EdgeCand* cand, u64 n, const uint8_t* __restrict__ status, const uint8_t* __restrict__ need, EdgeCand* out, u64 cap, u64* counter) {
    u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (x >= n) return;
    EdgeCand e = cand[x];
    if (need[e.from] || need[e.to]) { u64 p = atomicAdd(counter, 1ull); if (p < cap) out[p] = e; }
    if (status[e.from] == 0) cand[x].type = e.type | 0x80u;    // list of an unresolved read: rewritten by the replay
}
// A handful of unresolved reads (error-free data: the two ends of the genome): the candidates the replay needs are those that touch a read of a short list
// -- the unresolved reads and their left / right extension partners (a candidate that touches an unresolved read u was emitted by a status-4 read x whose
// partners point back at x, economyGraph.cpp:460, so x is one of u's two partners) -- which lives in LDS: ONE streaming pass over the candidates, no
// per-candidate look-ups in global memory (the general form above scans the list three times with two random byte gathers per candidate: 2.0 of the 2.3 ms
// of the reduce phase at BASELINE configs[2]).  need / unres: ascending ids.
constexpr int FEW_MAX = 3072;
__device__ __forceinline__ bool few_has(const u32* a, u32 n, u32 v) { u32 lo = 0, hi = n; while (lo < hi) { const u32 m = (lo + hi) >> 1; if (a[m] < v) lo = m + 1; else hi = m; } return lo < n && a[lo] == v; }
__global__ __launch_bounds__(256) void k_red_collect_few(EdgeCand* cand, u64 n, const u32* __restrict__ need, u32 nNeed, const u32* __restrict__ unres, u32 nUn, EdgeCand* out, u64 cap, u64* counter) {
    __shared__ u32 sNeed[FEW_MAX]; __shared__ u32 sUn[FEW_MAX / 3];
    for (u32 x = threadIdx.x; x < nNeed; x += 256) sNeed[x] = need[x];
    for (u32 x = threadIdx.x; x < nUn; x += 256) sUn[x] = unres[x];
    __syncthreads();
    const u32 nlo = sNeed[0], nhi = sNeed[nNeed - 1];
    for (u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += (u64)gridDim.x * blockDim.x) {
        const EdgeCand e = cand[x];
        const bool inRange = (e.from >= nlo && e.from <= nhi) || (e.to >= nlo && e.to <= nhi);      // (almost every candidate stops here)
        if (!inRange) continue;
        if (few_has(sNeed, nNeed, e.from) || few_has(sNeed, nNeed, e.to)) { const u64 p = atomicAdd((unsigned long long*)counter, 1ull); if (p < cap) { EdgeCand o = e; o.type &= 0x7Fu; out[p] = o; } }
        if (few_has(sUn, nUn, e.from)) cand[x].type = e.type | 0x80u;                                   // list of an unresolved read: rewritten by the replay
    }
}
__global__ void k_gather_records(const u32* __restrict__ ids, u32 n, const u32* __restrict__ posOf, const u32* __restrict__ idOf, const u64* __restrict__ right, const u64* __restrict__ left, u64* out) {
    const u32 x = blockIdx.x * blockDim.x + threadIdx.x; if (x >= n) return;
    const u32 p = posOf[ids[x]]; const u64 r = right[p], l = left[p];                     // (the records live in position space; the caller wants ids)
    out[2 * x] = (r & ~ID_MASK) | idOf[r & ID_MASK]; out[2 * x + 1] = (l & ~ID_MASK) | idOf[l & ID_MASK];
}
// per-read results for the C ABI (arrays indexed by id, neighbours named by id: economyGraph.h:24-30)
__global__ void k_records_to_ids(u64 N, const u32* __restrict__ idOf, const u64* __restrict__ right, const u64* __restrict__ left, const u32* __restrict__ conn, u64* rightI, u64* leftI, u32* connI) {
    const u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (p > N) return;
    if (p == 0) { rightI[0] = 0; leftI[0] = 0; connI[0] = 0; return; }
    const u32 i = idOf[p]; const u64 r = right[p], l = left[p];
    rightI[i] = (r & ~ID_MASK) | idOf[r & ID_MASK]; leftI[i] = (l & ~ID_MASK) | idOf[l & ID_MASK]; connI[i] = conn[p];
}
// the by-id copy of the status, on demand (ensure_status_by_id): coalesced byte stores, random byte loads
__global__ __launch_bounds__(256) void k_status_by_id(u64 N, const u32* __restrict__ posOf, const uint8_t* __restrict__ statusP, uint8_t* status) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (i > N) return; status[i] = i ? statusP[posOf[i]] : (uint8_t)0;
}
// the unresolved reads: the positions with status 0, listed by id, in any order
constexpr int UNRES_PER_THREAD = 16;
__global__ __launch_bounds__(256) void k_red_unresolved(u64 N, const uint8_t* __restrict__ statusP, const u32* __restrict__ idOf, u32* out, u64 cap, u64* counter) {
    __shared__ u32 sh[4]; __shared__ u64 shBase;
    const u64 tile0 = (u64)blockIdx.x * (256 * UNRES_PER_THREAD) + 1;
    u32 flags = 0, mine = 0;
#pragma unroll
    for (int it = 0; it < UNRES_PER_THREAD; it++) { const u64 i = tile0 + (u64)it * 256 + threadIdx.x; if (i <= N && statusP[i] == 0) { flags |= 1u << it; mine++; } }
    u32 total; const u32 excl = block_excl_scan(mine, sh, total);
    if (total == 0) return;
    if (threadIdx.x == 0) shBase = atomicAdd(counter, (u64)total);                 // one atomic per 4096 reads (most reads are unresolved on noisy data)
    __syncthreads();
    u64 p = shBase + excl;
#pragma unroll
    for (int it = 0; it < UNRES_PER_THREAD; it++) if (flags & (1u << it)) { if (p < cap) out[p] = idOf[tile0 + (u64)it * 256 + threadIdx.x]; p++; }
}

