// sage2_amd/csrc/kernels_scan.inc -- exclusive scan of u32: the kernels of scan_u32 (sage2ov_device.hip), the one driver every phase scans with.
// Part of sage2ov_device.hip (included inside namespace s2, in this order); not a translation unit of its own.

// =============================================================================================
// exclusive scan of u32.  partial: one word per block and one for the total, the caller's buffer.
//   k_scan_reduce<I, T>         partial[b] = sum of block b's I x T items
//   k_scan_final<I, T, true>    block b adds up partial[0, b) ITSELF and scans its items; the last block leaves the total -- two launches, as long as the
//                               blocks are few enough (SCAN_DIRECT_MAX_BLOCKS: a handful of words per thread out of the L2); nothing waits for another workgroup
//   k_scan_partials + k_scan_final<I, T, false>   beyond that, and for the callers that want the block prefixes themselves (scan_block_sums): one block turns
//                               partial[] into its exclusive scan in between
// A thread's items are consecutive and read as 16-byte vectors where the thread's stretch is whole and aligned, else one by one under the bound.
// scan_u32 runs blocks of 16 x 512 = 8192 items (1.3 - 10.6 M items per scan at BASELINE configs[2]: 160 - 1300 blocks); scan_block_sums keeps 8 x 256 = 2048,
// the block k_conv_emit ranks by itself.
// =============================================================================================
constexpr int SCAN_ITEMS = 8, SCAN_THREADS = 256, SCAN_BLOCK = SCAN_ITEMS * SCAN_THREADS;
constexpr int SCAN2_ITEMS = 16, SCAN2_THREADS = 512, SCAN2_BLOCK = SCAN2_ITEMS * SCAN2_THREADS, SCAN_DIRECT_MAX_BLOCKS = 4 * SCAN2_THREADS;
template <int NWAVES = 4>
__device__ __forceinline__ u32 block_excl_scan(u32 v, u32* sh, u32& total) {   // sh: one word per wave (NWAVES = waves of the block: compile time, the loop unrolls)
    u32 incl = wave_incl_scan(v); u32 w = threadIdx.x >> 6;
    if (lane_id() == 63) sh[w] = incl;
    __syncthreads();
    u32 add = 0, t = 0;
#pragma unroll
    for (u32 x = 0; x < (u32)NWAVES; x++) { u32 s = sh[x]; if (x < w) add += s; t += s; }
    __syncthreads();
    total = t;
    return add + incl - v;
}
template <int ITEMS>
__device__ __forceinline__ void scan_load(const u32* __restrict__ in, u64 base, u64 n, u32 (&v)[ITEMS]) {       // base: a multiple of ITEMS, ITEMS of 4
    if (base + ITEMS <= n && ((size_t)(in + base) & 15u) == 0) {
#pragma unroll
        for (int q = 0; q < ITEMS / 4; q++) { const uint4 x = ((const uint4*)(in + base))[q]; v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w; }
    } else {
#pragma unroll
        for (int i = 0; i < ITEMS; i++) v[i] = base + i < n ? in[base + i] : 0u;
    }
}
template <int ITEMS, int THREADS>
__global__ __launch_bounds__(THREADS) void k_scan_reduce(const u32* __restrict__ in, u64 n, u64* partial) {
    __shared__ u32 sh[THREADS / 64];
    const u64 base = ((u64)blockIdx.x * THREADS + threadIdx.x) * ITEMS; u32 v[ITEMS]; u32 s = 0;
    scan_load<ITEMS>(in, base, n, v);
#pragma unroll
    for (int i = 0; i < ITEMS; i++) s += v[i];
    u32 total; block_excl_scan<THREADS / 64>(s, sh, total);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}
__global__ void k_scan_partials(u64* partial, u64 nb, u64* total_out) {   // single block
    __shared__ u64 carry; __shared__ u64 shw[16];
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (u64 base = 0; base < nb; base += blockDim.x) {
        u64 i = base + threadIdx.x; u64 v = i < nb ? partial[i] : 0;
        // wave inclusive scan (u64)
        u64 incl = v; u32 lane = lane_id();
        for (int d = 1; d < 64; d <<= 1) { u64 t = __shfl_up(incl, d); if (lane >= (u32)d) incl += t; }
        u32 w = threadIdx.x >> 6;
        if (lane == 63) shw[w] = incl;
        __syncthreads();
        u64 add = 0, tot = 0;
        for (u32 x = 0; x < blockDim.x / 64; x++) { u64 s = shw[x]; if (x < w) add += s; tot += s; }
        u64 c = carry;
        if (i < nb) partial[i] = c + add + incl - v;
        __syncthreads();
        if (threadIdx.x == 0) carry = c + tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total_out = carry;
}
// DIRECT: partial[] holds the blocks' sums (k_scan_reduce) and the last block writes *total_out; else partial[] holds their exclusive scan (k_scan_partials)
template <int ITEMS, int THREADS, bool DIRECT>
__global__ __launch_bounds__(THREADS) void k_scan_final(const u32* __restrict__ in, u64 n, const u64* __restrict__ partial, u32* out, u64* total_out) {
    __shared__ u32 sh[THREADS / 64]; __shared__ u64 shp[THREADS / 64];
    const u64 base = ((u64)blockIdx.x * THREADS + threadIdx.x) * ITEMS; u32 v[ITEMS]; u32 s = 0;
    scan_load<ITEMS>(in, base, n, v);
#pragma unroll
    for (int i = 0; i < ITEMS; i++) s += v[i];
    u64 before;
    if (DIRECT) {
        u64 pre = 0;
        for (u32 x = threadIdx.x; x < blockIdx.x; x += THREADS) pre += partial[x];
        for (int d = 32; d; d >>= 1) pre += __shfl_xor(pre, d);
        if (lane_id() == 0) shp[threadIdx.x >> 6] = pre;
        __syncthreads();
        before = 0;
#pragma unroll
        for (int x = 0; x < THREADS / 64; x++) before += shp[x];
    } else before = partial[blockIdx.x];
    u32 total; u32 ex = block_excl_scan<THREADS / 64>(s, sh, total) + (u32)before;
    if (DIRECT && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *total_out = before + total;
    if (base + ITEMS <= n && ((size_t)(out + base) & 15u) == 0) {
#pragma unroll
        for (int q = 0; q < ITEMS / 4; q++) { uint4 x; x.x = ex; ex += v[4 * q]; x.y = ex; ex += v[4 * q + 1]; x.z = ex; ex += v[4 * q + 2]; x.w = ex; ex += v[4 * q + 3]; ((uint4*)(out + base))[q] = x; }
    } else {
#pragma unroll
        for (int i = 0; i < ITEMS; i++) { if (base + i < n) out[base + i] = ex; ex += v[i]; }
    }
}

