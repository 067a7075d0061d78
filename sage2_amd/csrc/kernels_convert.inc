// sage2_amd/csrc/kernels_convert.inc -- sort + convert of the candidate list.
// Part of sage2ov_device.hip (included inside namespace s2, in this order); not a translation unit of its own.

// =============================================================================================
// sortEconomyGraph + convertGraph (economyGraph.cpp:896, overlapGraph.cpp:84-111) on the candidate list
// =============================================================================================
// `sorted`: the candidate list in a stable order by `from` (dev_convert).  The first candidate of every read orders the read's list -- a handful of
// entries; the lists of unresolved reads on noisy data reach a hundred -- by compareIdBased (economyGraph.cpp:875) and marks the first entry of every
// (to, type) (overlapGraph.cpp:101); candidates the reduce phase dropped (0x80) sort behind the read's live ones and are never kept.
__global__ __launch_bounds__(256) void k_conv_group(const EdgeCand* __restrict__ sorted, u64 n, u64* keys, u32* keep) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    const EdgeCand e = sorted[x];
    if (x && sorted[x - 1].from == e.from) return;                                  // not the head of its read's list
    auto key_of = [](const EdgeCand& c) -> u64 { return (c.type & 0x80u) ? ~0ull : (((u64)c.to << 22) | ((u64)(c.type & 3u) << 20) | c.len); };
    u64* a = keys + x; u32* kp = keep + x;
    a[0] = key_of(e);
    u32 g = 1;
    for (; x + g < n; g++) {                                                        // insertion sort while the list is read
        const EdgeCand c = sorted[x + g]; if (c.from != e.from) break;
        const u64 v = key_of(c); int j = (int)g - 1; while (j >= 0 && a[j] > v) { a[j + 1] = a[j]; j--; } a[j + 1] = v;
    }
    for (u32 y = 0; y < g; y++) kp[y] = (a[y] != ~0ull && (y == 0 || (a[y] >> 20) != (a[y - 1] >> 20))) ? 1u : 0u;
}
// The compaction of the kept entries, in the order of x: a block takes the SCAN_BLOCK candidates that one word of k_scan_reduce's partial sums stands for
// (partial[b]: kept entries in front of block b, after k_scan_partials), a wave 512 consecutive ones of them as 8 rows of 64.  keep[] is 0 / 1, so the rank
// of an entry within its row is a population count of the row's ballot: no scan over the flags, no array of positions.
constexpr int CONV_ROWS = SCAN_BLOCK / SCAN_THREADS;
static_assert(SCAN_THREADS == 256 && CONV_ROWS * 64 * 4 == SCAN_BLOCK, "k_conv_emit: 4 waves of CONV_ROWS rows cover one block of the scan's partial sums");
__global__ __launch_bounds__(256) void k_conv_emit(u64 n, const u64* __restrict__ keys, const u32* __restrict__ keep, const u64* __restrict__ partial, const EdgeCand* __restrict__ sorted,
                            const u64* __restrict__ reads, int S, int uniL, FinalEdge* out) {
    __shared__ u32 sh[4];
    const u32 w = threadIdx.x >> 6, lane = lane_id();
    const u64 x0 = (u64)blockIdx.x * SCAN_BLOCK + (u64)w * (CONV_ROWS * 64) + lane;
    u32 mine = 0, before[CONV_ROWS], waveTotal = 0;                                          // bit r of mine: keep[x0 + 64 r]; before[r]: kept entries of the wave in front of mine in rows <= r
#pragma unroll
    for (int r = 0; r < CONV_ROWS; r++) {
        const u64 x = x0 + (u64)r * 64; const bool k = x < n && keep[x] != 0;
        const u64 b = __ballot(k);
        before[r] = waveTotal + (u32)__popcll(b & ((1ull << lane) - 1)); waveTotal += (u32)__popcll(b); mine |= (k ? 1u : 0u) << r;
    }
    if (lane == 0) sh[w] = waveTotal;
    __syncthreads();
    u64 base = partial[blockIdx.x]; for (u32 y = 0; y < w; y++) base += sh[y];
#pragma unroll
    for (int r = 0; r < CONV_ROWS; r++) {
        if (!(mine & (1u << r))) continue;
        const u64 x = x0 + (u64)r * 64;
        u64 kx = keys[x]; FinalEdge f; f.from = sorted[x].from; f.to = (u32)(kx >> 22); f.type = (u32)(kx >> 20) & 3u; f.len = (u32)(kx & 0xFFFFFu);
        const u32 Lu = (u32)read_len(reads, S, f.from, uniL), Lv = (u32)read_len(reads, S, f.to, uniL);
        f.len_twin = Lu - (Lv - f.len);                                                         // overlapGraph.cpp:145-148 (u32 arithmetic)
        out[base + before[r]] = f;
    }
}
