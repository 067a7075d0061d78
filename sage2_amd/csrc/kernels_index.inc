// sage2_amd/csrc/kernels_index.inc -- index build by partitioning: tuples -> windows built in LDS -> minimiser groups built in LDS.
// Part of sage2ov_device.hip (included inside namespace s2, in this order); not a translation unit of its own.

// =============================================================================================
// hashTable.cpp:70-128 semantics: multimap key -> entries in (id,type) order; >= 100 entries = long (never found).
//
// The uniform table (slots[T], linear probing, slot = tag:24 | cnt:7 | payload:33) is cut into WINDOWS of IX_W slots; a probe
// sequence wraps inside its window (ix_next_pair), so a window is a closed hash table small enough for LDS.  Build:
//   k_ix_tuples   the four keys of every read (hashTable.cpp:96-104) -> hash -> tuple {K = home pair index, P = tag | entry, M = hash of the key's minimiser},
//                 written in read order, + the first digit histogram.  8-word layout: a quad of lanes per read, one key per lane (other layouts: one thread
//                 per read); k_ix_tuples_loc is the same visit of the id-ordered store that also writes the locality-ordered copy
//   k_pt_*        LSD radix passes over the window id (kernels_partition.inc) until every window's tuples are contiguous
//   k_ix_window   one workgroup per window: claim / count with LDS atomics, CSR space for the window's multi-entry buckets drawn with
//                 ONE global atomic, entries placed and sorted by (id,type) in LDS, the window's slot words and CSR segment written
//                 out whole (coalesced; the table needs no memset).  Every distinct key also emits a group tuple {minimiser hash,
//                 final slot word} for the second access path:
//   k_pt_* again  over the group-table window id, then
//   k_mi_window   one workgroup per window of the group table mi1[TL] (mtag:24 | n:8 | start:32): claim / count by minimiser tag in
//                 LDS, records of a group contiguous in krec[] (its index space IS the sorted tuple order: no allocation at all).
// =============================================================================================
// (window sizes IX_W / IX_GW and the wrapping probe steps ix_next_*: kernels_common.inc)

__device__ __forceinline__ void entry_key(const u64* __restrict__ reads, int S, int h, u64 id, int t, u64& hi, u64& lo) {
    const u64* w = reads + id * S;
    int L = (int)(w[S - 1] & slot_len_mask(S));
    u64 phi, plo;
    if (t == 0 || t == 3) key_at(w, S, 0, h, phi, plo); else key_at(w, S, L - h, h, phi, plo);
    if (t >= 2) rc_key(phi, plo, h, hi, lo); else { hi = phi; lo = plo; }   // hashTable.cpp:96-104
}

// ---- tuples, quad form (8-word layout).  A slot is four 16-byte pieces and a quad of lanes holds one slot, lane c piece c (words 2c, 2c + 1): the access
// pattern of k_loc_scatter, every load coalesced.  Lane t builds key t of hashTable.cpp:96-104 and writes tuple 4 (id - 1) + t, so a wave writes 64 consecutive
// tuples (768 or 1024 contiguous bytes) where one thread per read put the four tuples of 64 reads at 64 places 48 bytes apart; the tuple index, and with
// it the (id, type) order inside every bucket, is what it was.
__device__ __forceinline__ u64 quad_word(const ulonglong2& v, int q) {         // word q (0..7) of the quad's slot (all four lanes of the quad are here)
    const u64 a = __shfl(v.x, q >> 1, 4), b = __shfl(v.y, q >> 1, 4);
    return (q & 1) ? b : a;
}
// the h-base key at base j of the quad's slot, as key_at gives it: its 2h bits lie in three consecutive words at most
__device__ __forceinline__ void quad_key_at(const ulonglong2& v, int j, int h, u64& hi, u64& lo) {
    const int q = (2 * j) >> 6, r = (2 * j) & 63;
    const u64 w0 = quad_word(v, q);
    u64 w1 = quad_word(v, q + 1 < 8 ? q + 1 : q); w1 = q + 1 < 8 ? w1 : 0ull;          // (words beyond the slot read as 0: bits64)
    const u64 a = (w0 << r) | ((w1 >> 1) >> (63 - r));                                   // bits [2j, 2j + 64)
    if (h <= 32) { hi = 0; lo = a >> (64 - 2 * h); return; }                             // (h is uniform)
    u64 w2 = quad_word(v, q + 2 < 8 ? q + 2 : q); w2 = q + 2 < 8 ? w2 : 0ull;
    const u64 b = (w1 << r) | ((w2 >> 1) >> (63 - r));                                   // bits [2j + 64, 2j + 128)
    const int d = 2 * h - 64;                                                            // 1..64
    hi = a >> (64 - d); lo = d == 64 ? b : ((a << d) | (b >> (64 - d)));                 // lo = bits [2j + 2h - 64, 2j + 2h)
}
// one tuple per lane: v = this lane's piece of read id0 + 1 (position pos of the locality order), t = lane in the quad = the key's type
__device__ __forceinline__ void ix_quad_tuple(const ulonglong2& v, u32 id0, u32 pos, int t, int h, u64 seed, u32 Th, int wantMI, int shift0, u32 mask0, int doHist, u32* T, u32* hst) {
    const int L = (int)(__shfl((u32)v.y, 3, 4) & slot_len_mask(8));                     // the slot's last word is in lane 3's piece
    u64 phi, plo, khi, klo;
    quad_key_at(v, (t == 0 || t == 3) ? 0 : L - h, h, phi, plo);                        // prefix (types 0, 3) or suffix (1, 2) of the forward strand
    rc_key(phi, plo, h, khi, klo);
    if (t < 2) { khi = phi; klo = plo; }                                                // types 2, 3: the reverse complement (hashTable.cpp:96-104)
    const u64 hv = hash_key(khi, klo, h, seed);
    const u32 kk = __umulhi((u32)(hv >> 32), Th), tag = tag_of(hv), entry = (u32)((u64)pos * 4 + (u64)t);
    if (doHist) atomicAdd(&hst[pt_digit(kk, shift0, mask0)], 1u);
    const u64 ti = 4 * (u64)id0 + (u64)t;
    if (wantMI) { u32 k0, k1, k2, k3; key_left_align(khi, klo, h, k0, k1, k2, k3);
                  ((uint4*)T)[ti] = make_uint4(kk, minim_hash(key_min_hash(k0, k1, k2, k3, h), (u32)seed), entry, tag); }
    else { u32* o = T + 3 * ti; o[0] = kk; o[1] = entry; o[2] = tag; }
}
// one tile of PT_TILE tuples = PT_TILE / 4 reads by one workgroup, PT_THREADS / 4 reads per step, two steps' loads in flight.  COPY: the slot also goes to its
// position in the locality-ordered store (k_loc_scatter's job) in the same visit.
template <bool COPY>
__device__ __forceinline__ void ix_quad_tile(const u64* __restrict__ reads, const u32* __restrict__ posOf, int byPos, u32 N, int h, u64 seed, u32 Th, int wantMI, int shift0, u32 mask0, int doHist,
                                             u32* T, u32* hst, u64* loc) {
    constexpr int RPS = PT_THREADS / 4, STEPS = PT_TILE / 4 / RPS, U = 2;
    static_assert(STEPS % U == 0 && PT_THREADS % 64 == 0, "quad tile");
    const int c = (int)(threadIdx.x & 3u);
#pragma unroll 1
    for (int j = 0; j < STEPS; j += U) {
        ulonglong2 v[U]; u32 id0[U], pos[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            id0[u] = blockIdx.x * (u32)(PT_TILE / 4) + (u32)((j + u) * RPS) + (threadIdx.x >> 2);
            if (id0[u] < N) { pos[u] = posOf[id0[u] + 1u]; v[u] = ((const ulonglong2*)reads)[(u64)(byPos ? pos[u] : id0[u] + 1u) * 4 + c]; }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (id0[u] >= N) continue;                                                  // (a quad is one read: in or out as a whole)
            if (COPY) ((ulonglong2*)loc)[(u64)pos[u] * 4 + c] = v[u];
            ix_quad_tuple(v[u], id0[u], pos[u], c, h, seed, Th, wantMI, shift0, mask0, doHist, T, hst);
        }
    }
}

// ---- tuples.  One workgroup = PT_TILE / 4 reads = one tile of the first radix pass (its histogram is taken on the fly).
// Reads are visited in ID order and the entry carries the read's POSITION in the locality-ordered store (what the probe kernels gather
// from): the radix passes are stable, so inside a window the tuples of one key stay in (id, type) order -- the bucket order of
// hashTable.cpp:94-109 -- and k_ix_window orders a bucket by tuple index, without ever looking an id up.
// (byPos: `reads` is the LOCALITY-ordered store -- the id-ordered one has been released, memory-diet mode -- and read id sits at slot posOf[id])
__global__ __launch_bounds__(PT_THREADS) void k_ix_tuples(const u64* __restrict__ reads, const u32* __restrict__ posOf, int byPos, u32 N, int S, int h, u64 seed, u32 Th, int wantMI, int shift0, u32 mask0, int doHist,
                                                         u32* T, u32* cnt, u32 ntiles) {      // T: tuples of 4 dwords {K, M, entry, tag} with the minimiser hash, else 3 {K, entry, tag}
    __shared__ u32 hst[PT_NB_MAX];
    if (doHist) { for (u32 x = threadIdx.x; x <= mask0; x += PT_THREADS) hst[x] = 0; __syncthreads(); }
    if (S == 8) ix_quad_tile<false>(reads, posOf, byPos, N, h, seed, Th, wantMI, shift0, mask0, doHist, T, hst, nullptr);      // (S is uniform; the other layouts: one thread per read)
    else {
#pragma unroll 1
    for (int j = 0; j < PT_TILE / 4 / PT_THREADS; j++) {
        const u32 id0 = blockIdx.x * (PT_TILE / 4) + j * PT_THREADS + threadIdx.x;
        if (id0 >= N) continue;
        const u64 id = (u64)id0 + 1;
        const u64 pos = posOf[id]; const u64 ent4 = pos * 4;
        const u64* w = reads + (byPos ? pos : id) * S;
        const int L = (int)(w[S - 1] & slot_len_mask(S));
        u64 khi[4], klo[4];
        key_at(w, S, 0, h, khi[0], klo[0]); key_at(w, S, L - h, h, khi[1], klo[1]);                     // prefix, suffix of the forward strand
        rc_key(khi[1], klo[1], h, khi[2], klo[2]); rc_key(khi[0], klo[0], h, khi[3], klo[3]);           // prefix, suffix of the reverse complement (hashTable.cpp:96-104)
        u32 kk[4], mm[4]; u64 pp[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const u64 hv = hash_key(khi[t], klo[t], h, seed);
            kk[t] = __umulhi((u32)(hv >> 32), Th);
            pp[t] = ((u64)tag_of(hv) << 32) | (u64)(u32)(ent4 + (u64)t);
            mm[t] = 0;
            if (wantMI) { u32 k0, k1, k2, k3; key_left_align(khi[t], klo[t], h, k0, k1, k2, k3); mm[t] = minim_hash(key_min_hash(k0, k1, k2, k3, h), (u32)seed); }
            if (doHist) atomicAdd(&hst[pt_digit(kk[t], shift0, mask0)], 1u);
        }
        if (wantMI) {
#pragma unroll
            for (int t = 0; t < 4; t++) ((uint4*)T)[4 * (u64)id0 + t] = make_uint4(kk[t], mm[t], (u32)pp[t], (u32)(pp[t] >> 32));
        } else {
            u32* o = T + 12 * (u64)id0;                          // 48 contiguous bytes per read
#pragma unroll
            for (int t = 0; t < 4; t++) { o[3 * t] = kk[t]; o[3 * t + 1] = (u32)pp[t]; o[3 * t + 2] = (u32)(pp[t] >> 32); }
        }
    }
    }
    if (doHist) { __syncthreads(); for (u32 x = threadIdx.x; x <= mask0; x += PT_THREADS) cnt[(u64)x * ntiles + blockIdx.x] = hst[x]; }
}
// k_loc_scatter and k_ix_tuples in one visit of the id-ordered store (8-word layout, first attempt of a build): every slot is loaded once, goes to its position in
// the locality-ordered store `loc` and gives its four tuples.  Workgroup b has the reads b * PT_TILE / 4 + 1 .., workgroup 0 also slot 0 (all zero, position 0).
__global__ __launch_bounds__(PT_THREADS) void k_ix_tuples_loc(const u64* __restrict__ reads, const u32* __restrict__ posOf, u32 N, int h, u64 seed, u32 Th, int wantMI, int shift0, u32 mask0, int doHist,
                                                             u32* T, u32* cnt, u32 ntiles, u64* loc) {
    __shared__ u32 hst[PT_NB_MAX];
    if (doHist) { for (u32 x = threadIdx.x; x <= mask0; x += PT_THREADS) hst[x] = 0; __syncthreads(); }
    if (blockIdx.x == 0 && threadIdx.x < 4) ((ulonglong2*)loc)[(u64)posOf[0] * 4 + threadIdx.x] = ((const ulonglong2*)reads)[threadIdx.x];
    ix_quad_tile<true>(reads, posOf, 0, N, h, seed, Th, wantMI, shift0, mask0, doHist, T, hst, loc);
    if (doHist) { __syncthreads(); for (u32 x = threadIdx.x; x <= mask0; x += PT_THREADS) cnt[(u64)x * ntiles + blockIdx.x] = hst[x]; }
}

__global__ void k_debug_table(const u64* __restrict__ slots, u64 T, u64* out) {
    for (u64 idx = (u64)blockIdx.x * blockDim.x + threadIdx.x; idx < T; idx += (u64)gridDim.x * blockDim.x) {       // (grid-stride: T passes 2^32 at 0.5 G reads)
        u64 s = slots[idx]; if (s == 0) continue;
        u32 c7 = (u32)(s >> SLOT_CNT_SHIFT) & 127u;
        atomicAdd(&out[0], 1ull);
        if (c7 == 1) atomicAdd(&out[1], 1ull);
        if (c7 == 0) atomicAdd(&out[2], 1ull);                 // claimed, never filled
        if ((s >> SLOT_TAG_SHIFT) == 0) atomicAdd(&out[3], 1ull);
        if (c7 >= 2 && c7 < 127) atomicAdd(&out[4], (u64)c7);
    }
}
__global__ void k_debug_keys(const u64* __restrict__ reads, u64 N, int S, int h, u64* out) {
    u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 4 * N) return;
    u64 hi, lo; entry_key(reads, S, h, (e >> 2) + 1, (int)(e & 3), hi, lo);
    out[2 * e] = hi; out[2 * e + 1] = lo;
}
template <int NWAVES> __device__ __forceinline__ u32 block_excl_scan(u32 v, u32* sh, u32& total);

// ---- one window of the uniform table.
// LDS word while counting: tag:24 | fp:20 | entries so far:20.  fp = 20 bits of the claiming key's minimiser hash: an arrival that finds
// its tag under another fp is a DIFFERENT key merged into the bucket (same 24-bit tag on the same probe chain, about once per ten
// million reads; look-ups verify every candidate, so the merge itself is exact) -- the minimiser groups are per key, so that arrival
// files a record of the bucket under its own minimiser too (or its windows would never find the bucket in their group).
// counters: [0] CSR entries, [1] occupied slots, [2] long buckets, [3] impurity flag, [4] pure long buckets, [5] group tuples, [6] groups,
//           [7] group table crowded, [8] errors (a window or a bucket counter overflowed), [9] cursor of the heavy windows' scratch words
// The 40 bits under the tag are split at run time (IxWinArgs::cntBits): 20 | 20 by default -- a key in more than 2^20 - 9 reads (adaptor or low-complexity k-mers of a
// billion-read set) makes the host build again with 10 | 30 (ADVICE round 3: it used to fail with SAGE2OV_ERR_LIMIT; such a bucket is long, hashTable.cpp:111-123,
// and never read in order, but its entries are counted, kept and purity-checked like any other's).
constexpr int IXW_CNT_BITS_DEFAULT = 20, IXW_CNT_BITS_WIDE = 30;
// fingerprint of the claiming key (20 bits of its minimiser hash).  Tests shrink it (SAGE2OV_TEST_FP_BITS) the way they shrink the tags: a second
// key that merges into a bucket AND shares the fingerprint files no group record -- 2^-20 per merge, a merge about once per ten million reads.
__device__ u32 g_fp_mask = 0xFFFFFu;
constexpr int IXW_T = 256;                       // threads of a window's workgroup.  With 256 a thread carries 12 tuples (161 VGPRs: three waves per SIMD, which is also what 51 KB of LDS per
                                                 // workgroup allow); 512 threads carry 6 each (110 VGPRs, four waves) and 1024 carry 3 (93) -- measured at BASELINE configs[2]: index build
                                                 // 19.6-19.8 / 19.5-19.7 / 20.4 ms.  The kernel is bound by its LDS atomics, not by occupancy: 256 stays.
constexpr int IXW_R = 3072 / IXW_T;              // tuples a thread carries in registers from the counting pass to the placing pass (IXW_T x IXW_R = 3072 per window; mean 2048)
constexpr int IXW_CSR_CAP = 3072;      // CSR entries of a window staged and sorted in LDS (beyond: straight to global memory, sorted there)
constexpr u32 GT_INVALID = 0x80000000u;   // key of a group tuple that carries no record (valid keys are minimiser hashes >> 1)
struct IxWinArgs {
    const u32* T; int W;               // sorted tuples: W = 4 dwords {K, M, entry, tag} or 3 {K, entry, tag}
    const u32* winOff; u32 nW;
    u64* slots; u32* csr; u64* counters; u64* big; u32 big_cap;
    const u32* idOf;                   // entries are POSITIONS in the locality-ordered store; the order inside a bucket is by read id (hashTable.cpp:94-109)
    u32* G;                            // group tuples out, 3 dwords {minimiser hash >> 1, record.lo, record.hi} at the tuple's position (null: no minimiser index)
    u32 cntBits;                       // entries-so-far field of the counting word (the fingerprint takes the other 40 - cntBits bits)
    u64* wh; u64 wh_cap;               // scratch for windows with more than 256 * IXW_R tuples (a key in thousands of reads): such a window draws one word per surplus
                                       // tuple from the buffer (counters[9] is the cursor; round 2 kept a word per tuple position: 32 bytes per read)
};
constexpr int IXW_WAVES = 1;           // occupancy bound of k_ix_window's __launch_bounds__ (the registers are not squeezed: 161 VGPRs, see IXW_T)
__global__ __launch_bounds__(IXW_T, IXW_WAVES) void k_ix_window(IxWinArgs A) {
    __shared__ u64 tbl[IX_W];
    __shared__ u32 csrL[IXW_CSR_CAP];
    __shared__ unsigned short csrT[IXW_CSR_CAP];   // tuple index (relative to the window) of every staged entry: the order inside a bucket
    __shared__ u32 sh[IXW_T / 64]; __shared__ u64 shWh;
    const u32 tid = threadIdx.x;
    const bool hasM = A.G != nullptr;
    auto tuple = [&](u64 i, u32& k, u64& p, u32& m) {            // (W is uniform)
        if (A.W == 4) { const uint4 v = ((const uint4*)A.T)[i]; k = v.x; m = v.y; p = ((u64)v.w << 32) | v.z; }
        else { const u32* q = A.T + 3 * i; k = q[0]; m = 0; p = ((u64)q[2] << 32) | q[1]; }
    };
    const int IXW_FP_SHIFT = (int)A.cntBits; const u64 IXW_CNT = (1ull << A.cntBits) - 1ull, IXW_FP_MASK = (1ull << (40 - A.cntBits)) - 1ull;
    const u32 fpMask = g_fp_mask & (u32)IXW_FP_MASK;  // (read once: inside the insert loop the load is not hoisted past the LDS atomics and cost the kernel 40 %)
    u64 accCsr = 0, accOcc = 0;                       // (thread 0) statistics of this workgroup's windows: one atomic each at the end
    for (u32 w = blockIdx.x; w < A.nW; w += gridDim.x) {
        for (u32 x = tid; x < (u32)IX_W; x += IXW_T) tbl[x] = 0ull;
        __syncthreads();
        const u32 b = A.winOff[w], e = A.winOff[w + 1];
        u64 whBase = 0;                                                                   // heavy window: its surplus tuples' scratch words
        if (e - b > (u32)IXW_R * (u32)IXW_T) {
            if (tid == 0) { const u64 need = (u64)(e - b) - (u64)IXW_R * (u64)IXW_T; u64 at = atomicAdd((unsigned long long*)&A.counters[9], (unsigned long long)need);
                            if (at + need > A.wh_cap) { atomicAdd(&A.counters[8], 1ull << 40); at = ~0ull; } shWh = at; }
            __syncthreads();
            whBase = shWh;
            __syncthreads();
            if (whBase == ~0ull) continue;                                                // (the host reports the overflow: SAGE2OV_ERR_LIMIT)
        }
        // ---------------- pass A: claim and count; (slot, rank, files) of every tuple is kept for pass B
        auto insert = [&](u32 k, u64 p, u32 m, u32& info, u32& rank) {
            const u64 tag = p >> 32; const u64 fp = (u64)((m ^ (m >> 20)) & fpMask);
            u32 idx = (k & (u32)(IX_WP - 1)) * 2u; bool files = false; u32 rk = 0; u32 steps = 0;
            for (;;) {
                u64 s = tbl[idx];
                if (s == 0) {
                    s = atomicCAS((unsigned long long*)&tbl[idx], 0ull, (unsigned long long)((tag << SLOT_TAG_SHIFT) | (fp << IXW_FP_SHIFT) | 1ull));
                    if (s == 0) { files = true; break; }                               // claimed: rank 0
                }
                if ((s >> SLOT_TAG_SHIFT) == tag) {
                    rk = (u32)(atomicAdd((unsigned long long*)&tbl[idx], 1ull) & IXW_CNT);
                    if (rk >= (u32)IXW_CNT - 8u) atomicAdd(&A.counters[8], 1ull << 20);      // the counter field is full: the host builds again with the wide split
                    files = ((s >> IXW_FP_SHIFT) & IXW_FP_MASK) != fp;                 // another key's bucket
                    break;
                }
                idx = (idx + 1u) & (u32)(IX_W - 1);
                if (++steps > (u32)IX_W) { atomicAdd(&A.counters[8], 1ull); idx = ~0u; break; }   // a full window (never with T = 8N)
            }
            info = idx == ~0u ? ~0u : (idx | (files ? 0x80000000u : 0u)); rank = rk;
        };
        u64 cp[IXW_R]; u32 cm[IXW_R], ci[IXW_R], cr[IXW_R]; u32 ck[IXW_R];
#pragma unroll
        for (int r = 0; r < IXW_R; r++) {
            const u32 i = b + (u32)r * (u32)IXW_T + tid; const bool v = i < e;
            ck[r] = 0; cp[r] = 0; cm[r] = 0; if (v) tuple(i, ck[r], cp[r], cm[r]);
        }
#pragma unroll
        for (int r = 0; r < IXW_R; r++) {
            ci[r] = ~0u; cr[r] = 0;
            if (b + (u32)r * (u32)IXW_T + tid < e) insert(ck[r], cp[r], cm[r], ci[r], cr[r]);
        }
        for (u64 i = (u64)b + (u64)IXW_R * (u64)IXW_T + tid; i < e; i += IXW_T) {                 // a heavy window (a key in thousands of reads): through global scratch
            u32 info, rank; u32 tk, tm; u64 tp; tuple(i, tk, tp, tm); insert(tk, tp, tm, info, rank);
            A.wh[whBase + (i - b - (u64)IXW_R * (u64)IXW_T)] = (u64)info | ((u64)rank << 32);
        }
        __syncthreads();
        // ---------------- CSR space for the multi-entry buckets (one atomic per window), slot words into their final form
        u32 c[IX_W / IXW_T]; u32 need = 0, occ = 0;
#pragma unroll
        for (int x = 0; x < IX_W / IXW_T; x++) { c[x] = (u32)(tbl[x * IXW_T + tid] & IXW_CNT); need += c[x] >= 2 ? c[x] : 0u; occ += c[x] != 0; }
        u32 total; const u32 excl = block_excl_scan<IXW_T / 64>(need, sh, total);
        u32 occTotal; block_excl_scan<IXW_T / 64>(occ, sh, occTotal);
        // The window's CSR segment and its group tuples live at the window's own range [b, e) of the sorted tuple order (a bucket with
        // >= 2 entries has that many tuples, so the segment fits): no allocation, no returning atomic anywhere in the build.
        accCsr += total; accOcc += occTotal;
        const u64 csrBase = b;
        const bool staged = total <= (u32)IXW_CSR_CAP && (e - b) <= 65535u;
        {
            u64 start = csrBase + excl;
#pragma unroll
            for (int x = 0; x < IX_W / IXW_T; x++) {
                if (c[x] == 0) continue;
                const u32 idx = x * IXW_T + tid; const u64 tagbits = tbl[idx] & (~0ull << SLOT_TAG_SHIFT);
                if (c[x] == 1) tbl[idx] = tagbits | (1ull << SLOT_CNT_SHIFT);                           // the entry itself is OR-ed in by pass B
                else {
                    const u32 c7 = c[x] >= HASH_THRESHOLD ? SLOT_CNT_LONG : c[x];
                    tbl[idx] = tagbits | ((u64)c7 << SLOT_CNT_SHIFT) | start;
                    if (c[x] >= HASH_THRESHOLD) {
                        const u64 bb = atomicAdd((unsigned long long*)&A.counters[2], 1ull);
                        if (bb < A.big_cap) { A.big[3 * bb] = (u64)w * IX_W + idx; A.big[3 * bb + 1] = start; A.big[3 * bb + 2] = c[x]; }
                    }
                    start += c[x];
                }
            }
        }
        __syncthreads();
        // ---------------- pass B: entries into the buckets, one group tuple per distinct key
        // group tuple of tuple i at position i (coalesced): {minimiser hash >> 1, final slot word} for the one tuple per distinct key that
        // files, {GT_INVALID, 0} for the others -- the invalid ones sort behind every group window
        auto place = [&](u64 i, u64 p, u32 m, u32 info, u32 rank) {
            bool files = false; u64 word = 0;
            if (info != ~0u) {
                const u32 idx = info & 0x7FFFFFFFu; files = (info >> 31) != 0;
                word = tbl[idx]; const u32 c7 = (u32)(word >> SLOT_CNT_SHIFT) & 127u; const u32 entry = (u32)p;
                if (c7 == 1) { word |= (u64)entry; tbl[idx] = word; }
                else { const u64 pos = (word & SLOT_PAY_MASK) + rank; if (staged) { csrL[(u32)(pos - csrBase)] = entry; csrT[(u32)(pos - csrBase)] = (unsigned short)(i - b); } else A.csr[pos] = entry; }
            }
            if (hasM) { u32* g = A.G + 3 * i; g[0] = files ? (m >> 1) : GT_INVALID; g[1] = files ? (u32)word : 0u; g[2] = files ? (u32)(word >> 32) : 0u; }
        };
#pragma unroll
        for (int r = 0; r < IXW_R; r++) { const u64 i = (u64)b + (u64)r * (u64)IXW_T + tid; if (i < e) place(i, cp[r], cm[r], ci[r], cr[r]); }
        for (u64 i = (u64)b + (u64)IXW_R * (u64)IXW_T + tid; i < e; i += IXW_T) { const u64 wv = A.wh[whBase + (i - b - (u64)IXW_R * (u64)IXW_T)]; u32 tk, tm; u64 tp; tuple(i, tk, tp, tm); place(i, tp, tm, (u32)wv, (u32)(wv >> 32)); }
        __syncthreads();
        // ---------------- buckets in (id,type) order (hashTable.cpp:94-109 inserts in that order); long buckets are never read in order.
        // An entry is position * 4 + type, the order is by (id, type): that is the order of the tuples (see k_ix_tuples), so a staged bucket is
        // ordered by tuple index; the rare bucket that lives in global memory (a heavy window) by the ids themselves (A.idOf).
        auto okey = [&](u32 en) -> u64 { return ((u64)A.idOf[en >> 2] << 2) | (u64)(en & 3u); };
#pragma unroll 1
        for (int x = 0; x < IX_W / IXW_T; x++) {
            if (c[x] < 2 || c[x] >= HASH_THRESHOLD) continue;
            const u64 st = tbl[x * IXW_T + tid] & SLOT_PAY_MASK;
            if (staged) {
                u32* a = csrL + (u32)(st - csrBase); unsigned short* ti = csrT + (u32)(st - csrBase);
                for (u32 i = 1; i < c[x]; i++) { const u32 v = a[i]; const unsigned short kv = ti[i]; int j = (int)i - 1; while (j >= 0 && ti[j] > kv) { a[j + 1] = a[j]; ti[j + 1] = ti[j]; j--; } a[j + 1] = v; ti[j + 1] = kv; }
            } else {
                u32* a = A.csr + st;
                for (u32 i = 1; i < c[x]; i++) { const u32 v = a[i]; const u64 kv = okey(v); int j = (int)i - 1; while (j >= 0 && okey(a[j]) > kv) { a[j + 1] = a[j]; j--; } a[j + 1] = v; }
            }
        }
        __syncthreads();
        // ---------------- the window leaves LDS: slot words (zeros included: the table is never cleared) and the CSR segment, coalesced
#pragma unroll
        for (int x = 0; x < IX_W / IXW_T; x++) A.slots[(u64)w * IX_W + x * IXW_T + tid] = tbl[x * IXW_T + tid];
        if (staged) for (u32 x = tid; x < total; x += IXW_T) A.csr[csrBase + x] = csrL[x];
        __syncthreads();
    }
    if (tid == 0) { if (accCsr) atomicAdd((unsigned long long*)&A.counters[0], (unsigned long long)accCsr); if (accOcc) atomicAdd((unsigned long long*)&A.counters[1], (unsigned long long)accOcc); }
}

// one wave per big bucket: every entry must carry the same true key, else two keys were merged by
// their 24-bit tags and the ">= 100 entries" verdict is not trustworthy -> ask for a reseed.
__global__ void k_index_purity(const u64* __restrict__ reads, int S, int h, const u64* __restrict__ big, u64 nbig, const u32* __restrict__ csr, u64* counters) {
    u64 b = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (b >= nbig) return;
    u64 start = big[3 * b + 1], c = big[3 * b + 2];
    u32 e0 = csr[start]; u64 hi0, lo0; entry_key(reads, S, h, e0 >> 2, e0 & 3, hi0, lo0);
    bool bad = false;
    for (u64 x = lane_id(); x < c; x += 64) { u32 e = csr[start + x]; u64 hi, lo; entry_key(reads, S, h, e >> 2, e & 3, hi, lo); if (hi != hi0 || lo != lo0) bad = true; }
    if (__ballot(bad)) { if (lane_id() == 0) atomicAdd(&counters[3], 1ull); }
    else if (lane_id() == 0) atomicAdd(&counters[4], 1ull);
}

// ---- one window of the group table: group tuples {minimiser hash, record} sorted by the table position of the minimiser.
// LDS word while counting: mtag:24 | records so far:40.  Records of a window stay inside the window's range of the sorted tuple order,
// which is krec's index space: group start = window start + exclusive scan of the group sizes.
constexpr u64 BUILD_CNT_MASK = (1ull << SLOT_TAG_SHIFT) - 1;
constexpr int MIW_R = 8;               // tuples per thread carried in registers (256 x 8 = 2048 per window)
constexpr int MIW_REC_CAP = 3064;      // records of a window staged in LDS (with the 16 KB of group words: 40 920 bytes -- FOUR workgroups fit a CU's 160 KB; 3072 made it 40 984 = three)
// (G: sorted group tuples, 3 dwords {minimiser hash >> 1, record.lo, record.hi})
struct MiWinArgs { const u32* G; const u32* gOff; u32 gW; int tlBits; u64* mi1; u64* krec; u64* counters; u64* wh; u64 wh_cap; };
__global__ __launch_bounds__(256) void k_mi_window(MiWinArgs A) {
    __shared__ u64 tbl[IX_GW];
    __shared__ u64 recL[MIW_REC_CAP];
    __shared__ u32 sh[4]; __shared__ u64 shWh;
    const u32 tid = threadIdx.x; const u32 mtagMask = g_mtag_mask;
    u64 accOcc = 0, accRec = 0;
    for (u32 w = blockIdx.x; w < A.gW; w += gridDim.x) {
        for (u32 x = tid; x < (u32)IX_GW; x += 256) tbl[x] = 0ull;
        __syncthreads();
        const u32 b = A.gOff[w], e = A.gOff[w + 1];
        u64 whBase = 0;
        if (e - b > (u32)MIW_R * 256u) {
            if (tid == 0) { const u64 need = (u64)(e - b) - (u64)MIW_R * 256u; u64 at = atomicAdd((unsigned long long*)&A.counters[9], (unsigned long long)need);
                            if (at + need > A.wh_cap) { atomicAdd(&A.counters[7], 1ull); at = ~0ull; } shWh = at; }       // (no room: the caller gives the groups up, like a crowded table)
            __syncthreads();
            whBase = shWh;
            __syncthreads();
            if (whBase == ~0ull) continue;
        }
        auto insert = [&](u32 mh1, u32& info, u32& rank) {          // mh1 = minimiser hash >> 1 (the tag ignores the lowest bit)
            const u64 mt = minim_tag_m(mh1 << 1, mtagMask);
            u32 idx = (mh1 >> (31 - A.tlBits)) & (u32)(IX_GW - 1); u32 rk = 0, steps = 0;
            for (;;) {
                u64 s = tbl[idx];
                if (s == 0) { s = atomicCAS((unsigned long long*)&tbl[idx], 0ull, (unsigned long long)((mt << SLOT_TAG_SHIFT) | 1ull)); if (s == 0) break; }
                if ((s >> SLOT_TAG_SHIFT) == mt) { rk = (u32)(atomicAdd((unsigned long long*)&tbl[idx], 1ull) & BUILD_CNT_MASK); break; }
                idx = (idx + 1u) & (u32)(IX_GW - 1);
                if (++steps > (u32)IX_GW) { atomicAdd(&A.counters[7], 1ull); idx = ~0u; break; }   // more distinct minimisers than group words: the caller gives the groups up
            }
            info = idx; rank = rk;
        };
        u64 cp[MIW_R]; u32 ck[MIW_R], ci[MIW_R], cr[MIW_R];
#pragma unroll
        for (int r = 0; r < MIW_R; r++) { const u32 i = b + (u32)r * 256u + tid; const bool v = i < e; const u32* g = A.G + 3 * (u64)(v ? i : 0u); ck[r] = v ? g[0] : 0u; cp[r] = v ? (((u64)g[2] << 32) | g[1]) : 0ull; }
#pragma unroll
        for (int r = 0; r < MIW_R; r++) { ci[r] = ~0u; cr[r] = 0; if (b + (u32)r * 256u + tid < e) insert(ck[r], ci[r], cr[r]); }
        for (u64 i = (u64)b + (u64)MIW_R * 256u + tid; i < e; i += 256) { u32 info, rank; insert(A.G[3 * i], info, rank); A.wh[whBase + (i - b - (u64)MIW_R * 256u)] = (u64)info | ((u64)rank << 32); }
        __syncthreads();
        u32 c[IX_GW / 256]; u32 need = 0, occ = 0;
#pragma unroll
        for (int x = 0; x < IX_GW / 256; x++) { const u64 cc = tbl[x * 256 + tid] & BUILD_CNT_MASK; c[x] = cc > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)cc; need += c[x]; occ += c[x] != 0; }
        u32 total; const u32 excl = block_excl_scan<4>(need, sh, total);
        u32 occTotal; block_excl_scan<4>(occ, sh, occTotal);
        accOcc += occTotal; accRec += e - b;
        const bool staged = (e - b) <= (u32)MIW_REC_CAP;
        {
            u32 start = b + excl;
#pragma unroll
            for (int x = 0; x < IX_GW / 256; x++) {
                if (c[x] == 0) continue;
                const u32 idx = x * 256 + tid;
                tbl[idx] = (tbl[idx] & (~0ull << SLOT_TAG_SHIFT)) | ((u64)(c[x] >= MI_BIG ? MI_BIG : c[x]) << 32) | (u64)start;
                start += c[x];
            }
        }
        __syncthreads();
        auto place = [&](u64 rec, u32 info, u32 rank) {
            if (info == ~0u) return;
            const u32 pos = (u32)tbl[info] + rank;
            if (staged) recL[pos - b] = rec; else A.krec[pos] = rec;
        };
#pragma unroll
        for (int r = 0; r < MIW_R; r++) place(cp[r], ci[r], cr[r]);
        for (u64 i = (u64)b + (u64)MIW_R * 256u + tid; i < e; i += 256) { const u64 wv = A.wh[whBase + (i - b - (u64)MIW_R * 256u)]; place(((u64)A.G[3 * i + 2] << 32) | A.G[3 * i + 1], (u32)wv, (u32)(wv >> 32)); }
        __syncthreads();
#pragma unroll
        for (int x = 0; x < IX_GW / 256; x++) A.mi1[(u64)w * IX_GW + x * 256 + tid] = tbl[x * 256 + tid];
        if (staged) for (u32 x = tid; x < e - b; x += 256) A.krec[b + x] = recL[x];
        __syncthreads();
    }
    if (tid == 0) { if (accOcc) atomicAdd((unsigned long long*)&A.counters[6], (unsigned long long)accOcc); if (accRec) atomicAdd((unsigned long long*)&A.counters[5], (unsigned long long)accRec); }
}
// self-check of the minimiser groups (SAGE2OV_VERIFY_MI): every entry's key must find, in the group of its own minimiser, a record that
// is the word of the slot the entry went to.  counters: [0] entries without such a record, [1] entries checked
__global__ void k_mi_verify(const u64* __restrict__ reads, u64 N, int S, int h, u64 seed, const u64* __restrict__ slots, u64 T,
                            const u64* __restrict__ mi1, u64 TL, const u64* __restrict__ krec, u64* out) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (e >= 4 * N) return;
    u64 hi, lo; entry_key(reads, S, h, (e >> 2) + 1, (int)(e & 3), hi, lo);
    u32 k0, k1, k2, k3; key_left_align(hi, lo, h, k0, k1, k2, k3);
    const u32 mh = minim_hash(key_min_hash(k0, k1, k2, k3, h), (u32)seed); const u64 mt = minim_tag(mh);
    u32 idx = __umulhi(mh, (u32)TL); u64 gv = 0;
    for (u32 step = 0; step < (u32)IX_GW; step++) { gv = mi1[idx]; if (gv == 0 || (gv >> SLOT_TAG_SHIFT) == mt) break; idx = ix_next_group(idx); }
    const u64 want = table_find(slots, T, hash_key(hi, lo, h, seed));
    bool ok = false;
    if (gv != 0 && (gv >> SLOT_TAG_SHIFT) == mt) { const u32 n = (u32)(gv >> 32) & 255u, st = (u32)gv; if (n == MI_BIG) ok = true; else for (u32 x = 0; x < n; x++) if (krec[st + x] == want) ok = true; }
    atomicAdd(&out[1], 1ull);
    if (!ok) { if (atomicAdd(&out[0], 1ull) < 8) printf("[verify-mi] e=%llu want=%llx gv=%llx\n", (unsigned long long)e, (unsigned long long)want, (unsigned long long)gv); }
}
// (entries leave as id * 4 + type: inside the index they are positions in the locality-ordered store)
__global__ void k_lookup(const u64* __restrict__ slots, u64 T, const u32* __restrict__ csr, const u32* __restrict__ idOf, u64 seed, int h, u64 hi, u64 lo, u64* out, u32 cap) {
    u64 s = table_find(slots, T, hash_key(hi, lo, h, seed));
    u32 c7 = (u32)(s >> SLOT_CNT_SHIFT) & 127u;
    if (s == 0 || c7 == SLOT_CNT_LONG) { out[0] = 0; return; }
    out[0] = c7;
    auto ext = [&](u32 e) -> u64 { return ((u64)idOf[e >> 2] << 2) | (u64)(e & 3u); };
    if (c7 == 1) { if (cap) out[1] = ext((u32)(s & SLOT_PAY_MASK)); return; }
    for (u32 x = 0; x < c7 && x < cap; x++) out[1 + x] = ext(csr[(s & SLOT_PAY_MASK) + x]);
}

