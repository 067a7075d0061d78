// sage2_amd/csrc/kernels_partition.inc -- radix partitioning of (key, payload) tuples: per-tile histogram + stable scatter.
// Part of sage2ov_device.hip (included inside namespace s2, in this order); not a translation unit of its own.

// =============================================================================================
// The index build and the locality order move every tuple to the place its key decides; done with one atomic per tuple on the
// destination that is a random 128-byte-line read-modify-write at the memory side per tuple (19.7 GB of line requests for 0.87 GB
// of useful bytes at BASELINE configs[1], 1.7 % of the HBM roofline).  Here the tuples are SORTED by the high bits of the key
// instead -- an LSD radix sort over <= 9-bit digits, every pass a streaming read and a scatter whose destinations of one
// (tile, digit) pair are contiguous -- until all tuples of one LDS-sized window of the destination table are contiguous; the
// window is then built in LDS by one workgroup (kernels_index.inc) and written out whole.  No global atomics on data.
//   k_pt_hist     per-tile digit histogram, cnt[digit * ntiles + tile] (digit-major: ONE exclusive scan gives every base)
//   k_pt_scatter  stable scatter: a wave ranks 64 consecutive tuples with one ballot per digit bit (match-any), waves of a tile are
//                 ordered through LDS, so equal digits keep their input order and the previous (lower) digits' order survives
//   k_pt_bounds_search   first position of every window id in the sorted keys, by binary search (k_pt_bounds: by a pass over all keys, A/B runs)
// Tuples are arrays of structures of 3 or 4 dwords (see k_pt_scatter); the digit is (dword KEYW >> shift) & mask.
// =============================================================================================
template <int NWAVES> __device__ __forceinline__ u32 block_excl_scan(u32 v, u32* sh, u32& total);
// Tile of a radix pass.  Round 3: 8192 tuples / 512 threads (one workgroup of eight waves per CU, 146 KB of LDS with 16-byte tuples) instead of
// 4096 / 256 (two workgroups of four): the runs a (tile, digit) pair writes are twice as long -- 5.2 -> 4.75 ms for the two table passes at configs[2].
// (PT_THREADS: the histogram kernel and the tuple kernel; PT_SC_*: the scatter kernel -- same tile.  Round 3, PT_SC_THREADS: sixteen waves on the one tile a CU holds
//  instead of eight -- 100 VGPRs, same LDS with 16-bit counters: index build -0.8 ms, convert -0.1 ms at configs[2])
constexpr int PT_TILE = 8192, PT_THREADS = 512, PT_NB_MAX = 512;
constexpr int PT_SC_THREADS = 1024, PT_WAVES = PT_SC_THREADS / 64, PT_ROUNDS = PT_TILE / PT_SC_THREADS;
constexpr int PT_DPT = PT_NB_MAX / PT_SC_THREADS > 0 ? PT_NB_MAX / PT_SC_THREADS : 1;       // digits a thread owns in the (digit, wave) scan (threads beyond the digits own none)
static_assert(PT_TILE <= 65536 && PT_TILE % PT_SC_THREADS == 0 && PT_TILE % PT_THREADS == 0 && PT_TILE / PT_WAVES <= 65535, "partition tile");
typedef unsigned short pt_cnt_t;                     // per wave and digit: at most PT_TILE / PT_WAVES tuples, then a position inside the tile (< 65536)
__device__ __forceinline__ u32 pt_digit(u32 k, int shift, u32 mask) { return shift >= 32 ? 0u : ((k >> shift) & mask); }

// (K points at the key dword of the first tuple, stride = dwords per tuple)
__global__ __launch_bounds__(PT_THREADS) void k_pt_hist(const u32* __restrict__ K, u32 n, int shift, u32 mask, u32* cnt, u32 ntiles, u32 stride) {
    __shared__ u32 h[PT_NB_MAX];
    for (u32 x = threadIdx.x; x <= mask; x += PT_THREADS) h[x] = 0;
    __syncthreads();
    const u32 t0 = blockIdx.x * PT_TILE;
#pragma unroll 4
    for (int r = 0; r < PT_TILE / PT_THREADS; r++) { const u32 i = t0 + r * PT_THREADS + threadIdx.x; if (i < n) atomicAdd(&h[pt_digit(K[(u64)i * stride], shift, mask)], 1u); }
    __syncthreads();
    for (u32 x = threadIdx.x; x <= mask; x += PT_THREADS) cnt[(u64)x * ntiles + blockIdx.x] = h[x];
}

// Round 3: tuples are ARRAYS OF STRUCTURES of W dwords (W = 4: {K, M, P.lo, P.hi}, W = 3: {K, P.lo, P.hi}); the digit comes from dword KEYW.  With
// structure-of-arrays tuples a (tile, digit) run was 32 + 64 + 32 bytes in three places; now it is one run of W x 4 x (tuples per run) bytes -- 256 bytes in
// the first table pass -- and a tuple moves with one load, one LDS write, one LDS read and one store instead of three of each.
// Tried in round 3 and dropped: staging only a permutation in LDS (34 KB, four workgroups per CU instead of two) and gathering the payloads of the
// sorted tile from the input tile in phase B -- 6.5 instead of 5.2 ms for the two table passes at configs[2]: 64 distinct lines per wave load
// cost the L1 more than the occupancy returns.
template <int W> struct PtElem;
template <> struct PtElem<4> { u32 d[4]; __device__ __forceinline__ static PtElem ld(const u32* p) { const uint4 v = *(const uint4*)p; PtElem e; e.d[0] = v.x; e.d[1] = v.y; e.d[2] = v.z; e.d[3] = v.w; return e; }
                               __device__ __forceinline__ void st(u32* p) const { *(uint4*)p = make_uint4(d[0], d[1], d[2], d[3]); } };
template <> struct PtElem<3> { u32 d[3]; __device__ __forceinline__ static PtElem ld(const u32* p) { PtElem e; e.d[0] = p[0]; e.d[1] = p[1]; e.d[2] = p[2]; return e; }
                               __device__ __forceinline__ void st(u32* p) const { p[0] = d[0]; p[1] = d[1]; p[2] = d[2]; } };
template <int W, int KEYW>
__global__ __launch_bounds__(PT_SC_THREADS) void k_pt_scatter(const u32* __restrict__ in, u32 n, int shift, u32 mask, const u32* __restrict__ base, u32 ntiles, u32* out) {
    __shared__ pt_cnt_t cntw[PT_WAVES][PT_NB_MAX];  // per wave and digit: count, then position of the wave's first tuple of that digit inside the sorted tile
    __shared__ u32 gdst[PT_NB_MAX];                 // per digit: global position of the tile's first tuple of that digit MINUS its position inside the sorted tile
    __shared__ __attribute__((aligned(16))) u32 sE[PT_TILE * W];     // the tile sorted by digit: the stores below are coalesced runs
    __shared__ u32 shw[PT_WAVES];
    const u32 tid = threadIdx.x, lane = tid & 63u, w = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    for (u32 x = tid; x < PT_WAVES * PT_NB_MAX; x += PT_SC_THREADS) (&cntw[0][0])[x] = 0;
    __syncthreads();
    // wave w owns the w-th part of the tile, 64 consecutive tuples per round: input order = (wave, round, lane)
    const u32 t0 = blockIdx.x * PT_TILE + w * (PT_TILE / PT_WAVES);
    PtElem<W> e[PT_ROUNDS]; u32 loc[PT_ROUNDS];
#pragma unroll
    for (int r = 0; r < PT_ROUNDS; r++) {
        const u32 i = t0 + r * 64 + lane;
        e[r] = PtElem<W>::ld(in + (u64)(i < n ? i : 0u) * W);
    }
    const u64 below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < PT_ROUNDS; r++) {
        const bool v = t0 + r * 64 + lane < n;
        const u32 d = pt_digit(e[r].d[KEYW], shift, mask);
        u64 peers = __ballot(v);
        for (int b = 0; (mask >> b) != 0u; b++) { const u64 mb = __ballot((d >> b) & 1u); peers &= ((d >> b) & 1u) ? mb : ~mb; }    // lanes with my digit (mask is uniform)
        const u32 old = cntw[w][d];
        wave_sync();
        if (v && (peers >> lane) == 1ull) cntw[w][d] = (pt_cnt_t)(old + (u32)__popcll(peers));                                                  // the highest lane of the set
        wave_sync();
        loc[r] = old + (u32)__popcll(peers & below);
    }
    __syncthreads();
    // exclusive scan over (digit, wave): position inside the sorted tile
    {
        u32 mine[PT_DPT][PT_WAVES]; u32 sum = 0;                         // thread t owns digits PT_DPT * t ..
#pragma unroll
        for (int q = 0; q < PT_DPT; q++)
#pragma unroll
            for (int ww = 0; ww < PT_WAVES; ww++) { const u32 d = PT_DPT * tid + q; mine[q][ww] = d <= mask ? cntw[ww][d] : 0u; sum += mine[q][ww]; }
        u32 total; u32 run = block_excl_scan<PT_WAVES>(sum, shw, total);
#pragma unroll
        for (int q = 0; q < PT_DPT; q++) {
            const u32 d = PT_DPT * tid + q;
            if (d <= mask) gdst[d] = base[(u64)d * ntiles + blockIdx.x] - run;
#pragma unroll
            for (int ww = 0; ww < PT_WAVES; ww++) { if (d <= mask) cntw[ww][d] = (pt_cnt_t)run; run += mine[q][ww]; }
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PT_ROUNDS; r++) {
        if (t0 + r * 64 + lane < n) {
            const u32 pos = cntw[w][pt_digit(e[r].d[KEYW], shift, mask)] + loc[r];
            e[r].st(sE + pos * W);
        }
    }
    __syncthreads();
    const u32 nt = min((u32)PT_TILE, n - blockIdx.x * PT_TILE);
#pragma unroll
    for (int r = 0; r < PT_ROUNDS; r++) {
        const u32 pos = r * PT_SC_THREADS + tid;
        if (pos < nt) {
            const PtElem<W> x = PtElem<W>::ld(sE + pos * W);
            const u32 dst = gdst[pt_digit(x.d[KEYW], shift, mask)] + pos;
            x.st(out + (u64)dst * W);
        }
    }
}

// The same scatter as TWO workgroups of eight waves per CU: the same 8192-tuple tile, the same (wave, round, lane) input order and the same stable ranking, so
// cnt / base and the output are those of k_pt_scatter byte for byte.  What makes two fit is that the sorted tile is staged in LDS in two HALVES: after the
// (digit, wave) scan every tuple knows its position in the sorted tile; phase 0 stages and stores positions [0, 4096), phase 1 the rest -- a (tile, digit) run
// across the boundary is written in two pieces to the same contiguous place.  One workgroup's loads and stores then run under the other's ranking.
// Registers (four waves per SIMD: 128): the tile's loads go through ONE address with immediate offsets under the lanes' validity, and the sixteen tile
// positions of a thread are kept as 16-bit pairs (0xFFFF: no tuple).
constexpr int PT2_THREADS = 512, PT2_WAVES = PT2_THREADS / 64, PT2_ROUNDS = PT_TILE / PT2_THREADS, PT2_HALF = PT_TILE / 2, PT2_LOG_HALF = 12;
static_assert(PT_NB_MAX <= PT2_THREADS && PT2_ROUNDS % 2 == 0 && (1 << PT2_LOG_HALF) == PT2_HALF && PT2_HALF % PT2_THREADS == 0 && PT_TILE < 65535, "partition tile, two workgroups");
template <int W, int KEYW>
__global__ __launch_bounds__(PT2_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4)))
void k_pt_scatter2(const u32* __restrict__ in, u32 n, int shift, u32 mask, const u32* __restrict__ base, u32 ntiles, u32* out) {
    __shared__ pt_cnt_t cntw[PT2_WAVES][PT_NB_MAX];
    __shared__ u32 gdst[PT_NB_MAX];
    __shared__ __attribute__((aligned(16))) u32 sE[PT2_HALF * W];    // one half of the tile sorted by digit
    __shared__ u32 shw[PT2_WAVES];
    const u32 tid = threadIdx.x, lane = tid & 63u, w = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    for (u32 x = tid; x < PT2_WAVES * PT_NB_MAX; x += PT2_THREADS) (&cntw[0][0])[x] = 0;
    __syncthreads();
    const u32 tile0 = blockIdx.x * PT_TILE, nt = min((u32)PT_TILE, n - tile0);
    const u32 l0 = w * (PT_TILE / PT2_WAVES) + lane;                 // my first tuple inside the tile; round r: l0 + 64 r
    const u32* tb = in + (u64)tile0 * W;                             // (uniform: the loads are this base + a 32-bit lane offset + an immediate)
    PtElem<W> e[PT2_ROUNDS]; u32 pos2[PT2_ROUNDS / 2];
    if (nt == PT_TILE) {
#pragma unroll
        for (int r = 0; r < PT2_ROUNDS; r++) e[r] = PtElem<W>::ld(tb + (l0 + r * 64) * W);
    } else {
#pragma unroll
        for (int r = 0; r < PT2_ROUNDS; r++) { const u32 l = l0 + r * 64; e[r] = PtElem<W>::ld(tb + (l < nt ? l : 0u) * W); }
    }
    const u64 below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < PT2_ROUNDS; r++) {
        const bool v = l0 + r * 64 < nt;
        const u32 d = pt_digit(e[r].d[KEYW], shift, mask);
        u64 peers = __ballot(v);
        for (int b = 0; (mask >> b) != 0u; b++) { const u64 mb = __ballot((d >> b) & 1u); peers &= ((d >> b) & 1u) ? mb : ~mb; }
        const u32 old = cntw[w][d];
        wave_sync();
        if (v && (peers >> lane) == 1ull) cntw[w][d] = (pt_cnt_t)(old + (u32)__popcll(peers));
        wave_sync();
        const u32 loc = old + (u32)__popcll(peers & below);          // < PT_TILE / PT2_WAVES
        pos2[r / 2] = (r & 1) ? (pos2[r / 2] | (loc << 16)) : loc;
        asm volatile("" : "+v"(pos2[r / 2]));                        // packed HERE: left to the scheduler, old and peers (three registers) stay live per round instead
    }
    __syncthreads();
    // exclusive scan over (digit, wave): thread t owns digit t
    {
        u32 mine[PT2_WAVES]; u32 sum = 0;
#pragma unroll
        for (int ww = 0; ww < PT2_WAVES; ww++) { mine[ww] = tid <= mask ? cntw[ww][tid] : 0u; sum += mine[ww]; }
        u32 total; u32 run = block_excl_scan<PT2_WAVES>(sum, shw, total);
        if (tid <= mask) gdst[tid] = base[(u64)tid * ntiles + blockIdx.x] - run;
#pragma unroll
        for (int ww = 0; ww < PT2_WAVES; ww++) { if (tid <= mask) cntw[ww][tid] = (pt_cnt_t)run; run += mine[ww]; }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PT2_ROUNDS; r++) {                           // position inside the sorted tile
        const u32 loc = (r & 1) ? (pos2[r / 2] >> 16) : (pos2[r / 2] & 0xFFFFu);
        const u32 pos = l0 + r * 64 < nt ? cntw[w][pt_digit(e[r].d[KEYW], shift, mask)] + loc : 0xFFFFu;
        pos2[r / 2] = (r & 1) ? ((pos2[r / 2] & 0xFFFFu) | (pos << 16)) : ((pos2[r / 2] & 0xFFFF0000u) | pos);
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {
        if (h) __syncthreads();                                      // the first half has been read
#pragma unroll
        for (int r = 0; r < PT2_ROUNDS; r++) {
            const u32 pos = (r & 1) ? (pos2[r / 2] >> 16) : (pos2[r / 2] & 0xFFFFu);
            if ((pos >> PT2_LOG_HALF) == (u32)h) e[r].st(sE + (pos & (PT2_HALF - 1)) * W);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PT2_HALF / PT2_THREADS; q++) {
            const u32 hp = q * PT2_THREADS + tid, pos = h * PT2_HALF + hp;
            if (pos < nt) {
                const PtElem<W> x = PtElem<W>::ld(sE + hp * W);
                const u32 dst = gdst[pt_digit(x.d[KEYW], shift, mask)] + pos;
                x.st(out + (u64)dst * W);
            }
        }
    }
}

// K is sorted by (K >> shiftW): off[w] = first position whose window id is >= w, off[nW] = n.  (n == 0: the host zeroes off.)
__global__ void k_pt_bounds(const u32* __restrict__ K, u32 n, int shiftW, u32 nW, u32* off, u32 stride) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
    const u32 w = shiftW >= 32 ? 0u : (K[(u64)i * stride] >> shiftW);
    const u32 lo = i ? (shiftW >= 32 ? 0u : (K[(u64)(i - 1) * stride] >> shiftW)) + 1u : 0u;
    for (u32 x = lo; x <= w; x++) off[x] = i;
    if (i == n - 1) for (u32 x = w + 1; x <= nW; x++) off[x] = n;
}

// the same off[] by search: one thread per window id w in [0, nW] finds the lower bound of w among the n sorted window ids -- log2(n) dependent loads per
// window (83 k windows at BASELINE configs[2]) where k_pt_bounds reads all 170 M keys again at the tuples' stride
__global__ void k_pt_bounds_search(const u32* __restrict__ K, u32 n, int shiftW, u32 nW, u32* off, u32 stride) {
    const u32 w = blockIdx.x * blockDim.x + threadIdx.x; if (w > nW) return;
    u32 lo = 0, hi = n;
    if (w == nW) lo = n;
    else if (shiftW >= 32) lo = w ? n : 0u;                        // (every key is in window 0)
    else while (lo < hi) { const u32 mid = lo + ((hi - lo) >> 1); if ((K[(u64)mid * stride] >> shiftW) < w) lo = mid + 1u; else hi = mid; }
    off[w] = lo;
}

// self-check (SAGE2OV_VERIFY_PARTITION): the window ids of the sorted tuples must not decrease; out[0] = violations, out[1] = largest window population
__global__ void k_pt_verify(const u32* __restrict__ K, u32 n, int shiftW, u32 stride, const u32* __restrict__ off, u32 nW, u64* out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && i > 0) { if ((K[(u64)i * stride] >> shiftW) < (K[(u64)(i - 1) * stride] >> shiftW)) atomicAdd((unsigned long long*)&out[0], 1ull); }
    if (i < nW) { const u32 c = off[i + 1] - off[i]; atomicMax((unsigned long long*)&out[1], (unsigned long long)c); if (off[i + 1] < off[i]) atomicAdd((unsigned long long*)&out[2], 1ull); }
}
