// sage2_amd/csrc/kernels_scan.inc -- exclusive scan of u32: the three kernels of scan_u32 (sage2ov_device.hip), the one driver every phase scans with.
// Part of sage2ov_device.hip (included inside namespace s2, in this order); not a translation unit of its own.

// =============================================================================================
// exclusive scan of u32 (3 kernels, 2048 items per block; partial: one word per block and one for the total, the caller's buffer)
// =============================================================================================
constexpr int SCAN_ITEMS = 8, SCAN_THREADS = 256, SCAN_BLOCK = SCAN_ITEMS * SCAN_THREADS;
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
__global__ void k_scan_reduce(const u32* __restrict__ in, u64 n, u64* partial) {
    __shared__ u32 sh[4];
    u64 base = (u64)blockIdx.x * SCAN_BLOCK + (u64)threadIdx.x * SCAN_ITEMS; u32 s = 0;
    for (int i = 0; i < SCAN_ITEMS; i++) if (base + i < n) s += in[base + i];
    u32 total; block_excl_scan(s, sh, total);
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
__global__ void k_scan_final(const u32* __restrict__ in, u64 n, const u64* __restrict__ partial, u32* out) {
    __shared__ u32 sh[4];
    u64 base = (u64)blockIdx.x * SCAN_BLOCK + (u64)threadIdx.x * SCAN_ITEMS; u32 v[SCAN_ITEMS]; u32 s = 0;
    for (int i = 0; i < SCAN_ITEMS; i++) { v[i] = base + i < n ? in[base + i] : 0; s += v[i]; }
    u32 total; u32 ex = block_excl_scan(s, sh, total) + (u32)partial[blockIdx.x];
    for (int i = 0; i < SCAN_ITEMS; i++) { if (base + i < n) out[base + i] = ex; ex += v[i]; }
}

