// sage2_amd/csrc/kernels_organize.inc -- step 1 on the device: canonical orientation, radix sort, unique, ids.
// Part of sage2ov_device.hip (included inside namespace s2, in this order); not a translation unit of its own.

// =============================================================================================
// Step 1 on the device (readLoader.cpp:179-260): canonical orientation, sort, unique + frequency, read ids.
// Input: the good reads as the host staged them (forward strand, 2-bit big-endian words, variable length).
//   k_org_canon   read < revcomp ? read : revcomp (:195), written as an S-word slot with the length in the low 9 bits of
//                 the last word: comparing slots word by word IS stringCompareInBytes (utils.cpp:224: bytes, then length)
//   k_rs_*        stable LSD radix sort of (first word, read index), 8 passes of 8 bits, one wave per 2048-element tile (driven by radix_sort_pairs,
//                 sage2ov_device.hip, which the mate table uses too: kernels_mates.inc)
//   k_org_ties    runs of equal first words ordered by the remaining words (insertion sort; duplicates cost one compare each)
//   k_org_heads   first read of every run of equal slots = a unique read; exclusive scan = id - 1; run length = frequency (u16 wrap)
//   k_headpos     position of head e in the sorted pairs, hp[E] = n (head_positions, sage2ov_device.hip; the mate table's heads go through it too)
//   k_org_gather  the HBM read store in id order (slot 0 = zeros)
// =============================================================================================
constexpr int RS_TILE = 2048;
// fwd (pairing, DESIGN.md 5.21; else null): fwd[i] = the read as staged is its canonical form -- the sign of its id (k_org_ids)
__global__ void k_org_canon(const u64* __restrict__ pool, const u64* __restrict__ off, const unsigned short* __restrict__ len, u64 n, int S, u64* img, u64* key0, u32* val, unsigned char* fwd) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
    const int L = len[i], nw = (L + 31) / 32; const u64* f = pool + off[i];
    u64 fw[SLOT_MAX_WORDS + 1], rw[SLOT_MAX_WORDS];
#pragma unroll 1
    for (int c = 0; c < SLOT_MAX_WORDS + 1; c++) fw[c] = c < nw ? f[c] : 0ull;
    bool useF = false, decided = false;                                  // readLoader.cpp:195 (tie: the reverse complement, same bytes)
#pragma unroll 1
    for (int c = 0; c < nw; c++) {
        const int rem = L - 32 * c; u64 r;
        if (rem >= 32) r = ~rev2(bits64(fw, SLOT_MAX_WORDS + 1, 2 * (rem - 32)));
        else r = (~rev2(fw[0] >> (64 - 2 * rem))) & mask_top(rem);
        rw[c] = r;
        if (!decided && fw[c] != r) { useF = fw[c] < r; decided = true; }
    }
    u64* o = img + i * S;
#pragma unroll 1
    for (int c = 0; c < S; c++) { u64 v = c < nw ? (useF ? fw[c] : rw[c]) : 0ull; if (c == S - 1) v |= (u64)L; o[c] = v; if (c == 0) key0[i] = v; }
    val[i] = (u32)i;
    if (fwd) fwd[i] = useF ? 1 : 0;
}
// ---- ASCII front end (sage2ov_reads_add_ascii on a GPU context): filter + 2-bit pack + canonical orientation on the device.
//   k_org_classify  isGoodRead (utils.cpp:144-166: longer than minOverlap, only ACGTacgt) -> flag; counters: [0] longest good read, [1] good
//                   reads, [2] their bases, [3] reads not longer than minOverlap (readLoader.cpp:145-158), [4] shortest good read
//   k_org_pack      charsToBytes (utils.cpp:96-119: A0 C1 G2 T3, first base in the top bits) of every good read into its slot of the
//                   organiser's image, already in canonical orientation (readLoader.cpp:195), at the compacted position (scan of the flags)
__device__ __forceinline__ u32 base_code(unsigned char ch) {              // 0..3, or 4 for anything that is not ACGTacgt
    const unsigned char u = ch & 0xDFu;                                   // upper case
    return u == 'A' ? 0u : (u == 'C' ? 1u : (u == 'G' ? 2u : (u == 'T' ? 3u : 4u)));
}
__global__ void k_org_classify(const unsigned char* __restrict__ bases, const u64* __restrict__ off, u64 n, u32 minOverlap, u32 maxLen, u32* flag, u64* counters) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 good = 0, small = 0; u64 len = 0;
    if (i < n) {
        const u64 a = off[i]; len = off[i + 1] - a;
        if (len <= minOverlap) small = 1;
        else {
            good = len <= maxLen ? 1u : 2u;                               // 2: too long for any layout (the caller reports the limit)
            for (u64 x = 0; x < len; x++) if (base_code(bases[a + x]) > 3u) { good = 0; break; }
        }
        flag[i] = good == 1 ? 1u : 0u;
    }
    if (good == 2) atomicAdd(&counters[5], 1ull);
    const u64 mg = __ballot(good == 1), ms = __ballot(small != 0);
    u64 bp = good == 1 ? len : 0; u32 mx = good == 1 ? (u32)len : 0u, mn = good == 1 ? (u32)len : ~0u;
    for (int d = 32; d > 0; d >>= 1) { bp += __shfl_down(bp, d); mx = max(mx, (u32)__shfl_down((int)mx, d)); mn = min(mn, (u32)__shfl_down((int)mn, d)); }
    if (lane_id() == 0) {
        if (mg) { atomicAdd(&counters[1], (u64)__popcll(mg)); atomicAdd(&counters[2], bp); atomicMax(&counters[0], (u64)mx); atomicMin(&counters[4], (u64)mn); }
        if (ms) atomicAdd(&counters[3], (u64)__popcll(ms));
    }
}
// Word c of a read given as ASCII (32 bases from base 32c on, the first one in the top bits, zero padded), or of its reverse complement (RC): straight from
// the characters, so that neither strand is ever held as an array (no scratch memory: registers only, whatever the layout)
template <bool RC> __device__ __forceinline__ u64 org_ascii_word(const unsigned char* __restrict__ bases, u64 a, int L, int c) {
    const int p0 = 32 * c, m = min(32, L - p0); u64 w = 0;
    for (int x = 0; x < m; x++) {
        const u32 cd = RC ? 3u - base_code(bases[a + (u64)(L - 1 - p0 - x)]) : base_code(bases[a + (u64)(p0 + x)]);
        w |= (u64)cd << (62 - 2 * x);
    }
    return w;
}
// charsToBytes of the good read bases[a, a + L) in canonical orientation as an S-word slot at o (the length in the low bits of the last word); true: the read as
// given is the canonical form (read < reverse complement, readLoader.cpp:195, :325), false: its reverse complement is -- a tie is never decided and stays with
// the reverse complement (same bytes).  Shared by the organiser (k_org_pack) and the read-id lookup (k_find_pack, kernels_find.inc); w0 = word 0 as written.
__device__ __forceinline__ bool org_pack_slot(const unsigned char* __restrict__ bases, u64 a, int L, int S, u64* o, u64& w0) {
    const int nw = (L + 31) / 32;
    bool useF = false;
#pragma unroll 1
    for (int c = 0; c < nw; c++) {
        const u64 f = org_ascii_word<false>(bases, a, L, c), r = org_ascii_word<true>(bases, a, L, c);
        if (f != r) { useF = f < r; break; }
    }
#pragma unroll 1
    for (int c = 0; c < S; c++) {
        u64 v = c < nw ? (useF ? org_ascii_word<false>(bases, a, L, c) : org_ascii_word<true>(bases, a, L, c)) : 0ull;
        if (c == S - 1) v |= (u64)L;
        o[c] = v; if (c == 0) w0 = v;
    }
    return useF;
}
__global__ void k_org_pack(const unsigned char* __restrict__ bases, const u64* __restrict__ off, u64 n, const u32* __restrict__ flag, const u32* __restrict__ pos, int S,
                           u64* img, u64* key0, u32* val, unsigned char* fwd) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (i >= n || !flag[i]) return;
    const u64 a = off[i]; const int L = (int)(off[i + 1] - a);
    const u64 o0 = pos[i]; u64 w0 = 0;
    const bool useF = org_pack_slot(bases, a, L, S, img + o0 * S, w0);
    key0[o0] = w0; val[o0] = (u32)o0;
    if (fwd) fwd[o0] = useF ? 1 : 0;
}
__global__ __launch_bounds__(64) void k_rs_hist(const u64* __restrict__ keys, u64 n, int shift, u32* hist, u32 nb) {
    __shared__ u32 h[256];
    for (int x = threadIdx.x; x < 256; x += 64) h[x] = 0;
    __syncthreads();
    const u64 base = (u64)blockIdx.x * RS_TILE;
    for (int c = 0; c < RS_TILE; c += 64) { const u64 x = base + c + threadIdx.x; if (x < n) atomicAdd(&h[(u32)(keys[x] >> shift) & 255u], 1u); }
    __syncthreads();
    for (int x = threadIdx.x; x < 256; x += 64) hist[(u64)x * nb + blockIdx.x] = h[x];
}
__global__ __launch_bounds__(64) void k_rs_scatter(const u64* __restrict__ keys, const u32* __restrict__ vals, u64 n, int shift, const u32* __restrict__ hscan, u32 nb,
                                                  u64* keysOut, u32* valsOut) {
    __shared__ u32 cnt[256];
    const u32 lane = threadIdx.x;
    for (int x = lane; x < 256; x += 64) cnt[x] = hscan[(u64)x * nb + blockIdx.x];
    wave_sync();
    const u64 base = (u64)blockIdx.x * RS_TILE;
    for (int c = 0; c < RS_TILE; c += 64) {
        const u64 x = base + c + lane; const bool valid = x < n;
        const u64 k = valid ? keys[x] : 0ull; const u32 v = valid ? vals[x] : 0u;
        const u32 dgt = (u32)(k >> shift) & 255u;
        u64 peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; b++) { const u64 m = __ballot((dgt >> b) & 1u); peers &= ((dgt >> b) & 1u) ? m : ~m; }
        const u32 rank = (u32)__popcll(peers & ((1ull << lane) - 1ull));
        const u32 old = cnt[dgt];
        wave_sync();
        if (valid && rank == 0) cnt[dgt] = old + (u32)__popcll(peers);
        wave_sync();
        if (valid) { keysOut[old + rank] = k; valsOut[old + rank] = v; }
    }
}
__device__ __forceinline__ int org_cmp(const u64* __restrict__ img, int S, u32 a, u32 b) {          // words 1.. (word 0 is known equal)
    const u64 *pa = img + (u64)a * S, *pb = img + (u64)b * S;
    for (int c = 1; c < S; c++) { const u64 x = pa[c], y = pb[c]; if (x != y) return x < y ? -1 : 1; }
    return 0;
}
// Long runs of equal first words (adapter dimers, low-complexity reads, amplicons: thousands of reads with the same first 32 bases) would
// make the per-run insertion sort quadratic: if any run is longer than ORG_RUN_LIMIT the host sorts on all words instead (LSD, last word first).
constexpr u32 ORG_RUN_LIMIT = 256;
__global__ void k_org_longrun(const u64* __restrict__ keys, u64 n, u32* flag) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
    const u64 k = keys[i];
    if (i > 0 && keys[i - 1] == k) return;                               // not the first of its run
    u64 e = i + 1; while (e < n && e - i <= ORG_RUN_LIMIT && keys[e] == k) e++;
    if (e - i > ORG_RUN_LIMIT) *flag = 1;
}
__global__ void k_org_wordkeys(const u64* __restrict__ img, int S, int c, const u32* __restrict__ vals, u64 n, u64* keys) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (x >= n) return;
    keys[x] = img[(u64)vals[x] * S + c];
}
__global__ void k_org_ties(const u64* __restrict__ keys, u32* vals, u64 n, const u64* __restrict__ img, int S) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
    const u64 k = keys[i];
    if (i > 0 && keys[i - 1] == k) return;                               // not the first of its run
    u64 e = i + 1; while (e < n && keys[e] == k) e++;
    for (u64 x = i + 1; x < e; x++) {
        const u32 v = vals[x]; u64 j = x;
        while (j > i && org_cmp(img, S, vals[j - 1], v) > 0) { vals[j] = vals[j - 1]; j--; }
        vals[j] = v;
    }
}
__global__ void k_org_heads(const u64* __restrict__ keys, const u32* __restrict__ vals, u64 n, const u64* __restrict__ img, int S, u32* flag) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
    flag[i] = (i == 0 || keys[i - 1] != keys[i] || org_cmp(img, S, vals[i - 1], vals[i]) != 0) ? 1u : 0u;
}
__global__ void k_headpos(const u32* __restrict__ flag, const u32* __restrict__ pos, u64 n, u32* hp, u64 E) {      // pos: exclusive scan of flag; E: its total
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && flag[i]) hp[pos[i]] = (u32)i;
    if (i == 0) hp[E] = (u32)n;
}
// ---- pairing (sage2ov_reads_pair_library, DESIGN.md 5.21): the id of every STAGED read, from what the pass above has already made.  One thread per sorted position
// j: uid is the exclusive scan of the head flags, so the read at j has id uid[j] + flag[j] (a head is the first of its id; the others count the heads up to
// theirs) -- whichever way the runs were ordered (k_org_ties or the full sort).  The sign is that of sage2ov_reads_find_ids: + when the read as given is strictly
// smaller than its reverse complement (fwd, from k_org_canon / k_org_pack).  k_org_ids_raw (ASCII route): the same per raw input record, back through the scan
// of k_org_classify's flags; 0 for a record that was not staged.
__global__ void k_org_ids(const u32* __restrict__ vals, const u32* __restrict__ flag, const u32* __restrict__ uid, u64 n, const unsigned char* __restrict__ fwd, int* idOf) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (j >= n) return;
    const u32 v = vals[j]; const int id = (int)(uid[j] + flag[j]);
    idOf[v] = fwd[v] ? id : -id;
}
__global__ void k_org_ids_raw(const u32* __restrict__ gflag, const u32* __restrict__ gpos, u64 nin, const int* __restrict__ idOf, int* rawId) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (i >= nin) return;
    rawId[i] = gflag[i] ? idOf[gpos[i]] : 0;
}
__global__ void k_org_gather(const u32* __restrict__ vals, const u32* __restrict__ headPos, u64 N, const u64* __restrict__ img, int S, u64* reads, unsigned short* freq) {
    // grid-stride: a launch of more than 2^32 threads is cut down to its size modulo 2^32 WITHOUT an error (found at 1.02 G reads x 8 words: the last 2^29
    // reads of the store stayed zero), so the grid is capped by the host (grid_for_capped) and every thread walks
    for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < N * (u64)S; t += (u64)gridDim.x * blockDim.x) {
        const u64 id = t / S + 1; const int c = (int)(t % S);
        const u32 hp = headPos[id - 1];
        reads[id * S + c] = img[(u64)vals[hp] * S + c];
        if (c == 0) freq[id] = (unsigned short)(headPos[id] - hp);          // u16 wrap like the reference (readLoader.cpp:232)
    }
}

