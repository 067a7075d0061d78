// sage2_amd/csrc/kernels_mates.inc -- MatePair::processMatePairs (matePair.cpp:161-239) as a sort-and-reduce job: the table of mate links between read ids.
// Part of sage2ov_device.hip (included inside namespace s2, in this order); not a translation unit of its own.

// =============================================================================================
// The reference walks a linked list per pair (and, with more than one thread, inserts into shared lists without a lock).  Here, per chunk of an even
// number of queries whose ids k_find_search left in HBM (kernels_find.inc):
//   k_mate_keep      one thread per pair: 2 records when both mates have an id, else 0; the skipped pairs counted by kind (a mate that is not a good
//                    read, utils.cpp:144-166 / a good read that is not in the store)
//   (scan)           position of every pair's records among the chunk's records: the records stay in record-ordinal order
//   k_mate_records   key = from:30 | to:30 | t_from:1 | t_to:1 (bits 61..32, 31..2, 1, 0; a context holds at most 2^30 - 1 reads) and the record
//                    ordinal 2 * p + side, appended to the pending buffer
// and per flush of the pending buffer (at a bound, and at the end of every call):
//   k_mate_iota, k_rs_hist / k_rs_scatter (kernels_organize.inc; radix_sort_pairs)   stable LSD radix sort of (key, index), only the passes whose digit can be non-zero
//   k_mate_heads     a record is a head when its key differs from its predecessor's
//   (scan) + k_headpos (kernels_organize.inc; head_positions)    position of head e in the sorted records; hp[E] = n
//   k_mate_reduce    entry e: count = hp[e + 1] - hp[e]; first = the ordinal of the head itself -- the sort is stable and the records were written in
//                    ordinal order, so inside a run of equal keys the ordinals ascend.  No thread walks a run.
//   k_mate_merge     the library's table (sorted, unique) and the new entries (sorted, unique), concatenated and sorted by the same passes: runs of
//                    length <= 2; counts summed, the smaller first kept
//   k_mate_offsets   offsets[a] = first entry whose `from` is >= a (a = 0 .. N + 1): one thread per read id, binary search (the pattern of
//                    k_pt_bounds_search); run when an export asks for it
// Every count below is kept under 2^32 by the driver (dev_mates_add), so one thread per item with grid_for is exact.
// =============================================================================================
__global__ void k_mate_keep(const long long* __restrict__ ids, const signed char* __restrict__ sign, const unsigned char* __restrict__ bases, const u64* __restrict__ off,
                            u32 npairs, u32 minOverlap, u32 maxLen, u32* keep, unsigned long long* cnt) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false, lost = false;
    if (j < npairs) {
#pragma unroll 1
        for (u32 m = 2 * j; m < 2 * j + 2; m++) {
            if (sign[m]) { lost |= ids[m] == 0; continue; }
            // sign 0: not a good read -- or a good one longer than the store's longest read, which k_org_classify keeps out of the search: not found
            const u64 a = off[m], len = off[m + 1] - a;
            bool good = len > minOverlap && len > maxLen;
            for (u64 x = 0; good && x < len; x++) good = base_code(bases[a + x]) <= 3u;
            if (good) lost = true; else bad = true;
        }
        lost = lost && !bad;
        keep[j] = (bad || lost) ? 0u : 2u;
    }
    const u64 mb = __ballot(bad), ml = __ballot(lost);
    if (lane_id() == 0) { if (mb) atomicAdd(&cnt[0], (unsigned long long)__popcll(mb)); if (ml) atomicAdd(&cnt[1], (unsigned long long)__popcll(ml)); }
}
__device__ __forceinline__ u64 mate_key(u64 from, u64 to, u64 tf, u64 tt) { return (from << 32) | (to << 2) | (tf << 1) | tt; }
__global__ void k_mate_records(const long long* __restrict__ ids, const u32* __restrict__ keep, const u32* __restrict__ pos, u32 npairs, u64 ord0, u64* key, u64* ord) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x; if (j >= npairs || !keep[j]) return;
    const long long a = ids[2 * j], b = ids[2 * j + 1];
    const u64 id1 = (u64)(a < 0 ? -a : a), id2 = (u64)(b < 0 ? -b : b), t1 = a > 0, t2 = b > 0;      // matePair.cpp:180-189
    const u64 o = pos[j];
    key[o] = mate_key(id1, id2, t1, t2); ord[o] = ord0 + 2ull * j;
    key[o + 1] = mate_key(id2, id1, t2, t1); ord[o + 1] = ord0 + 2ull * j + 1ull;
}
// ---- the pairs of one reads_add_* call from step 1's own by-products (sage2ov_mates_from_reads, DESIGN.md 5.21): no file is read and no store searched.
//   k_pair_slots   slotOf[ordinal] = staging index + 1, scattered from the ordinals the host kept per staged read (slotOf zeroed before: 0 = not staged)
//   k_pair_keep    one thread per pair p of a chunk: the ids of records rec0 + 2 p and rec0 + 2 p + 1 (through slotOf, or -- slotOf null, the ASCII route --
//                  straight from the per-record ids), laid out per pair as k_find_search leaves them; 2 records when both were staged, else the pair is one
//                  with a mate that is not a good read (only such a read is not staged).  k_mate_records then writes the records.
// Ordinals inside a call stay below 2^32 - 2048 (the host refuses more); the record ordinals k_mate_records writes are 64-bit.
__global__ void k_pair_slots(const u32* __restrict__ ord, u64 n, u32 first, u32* slotOf) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (x < n) slotOf[ord[x]] = first + (u32)x + 1u;
}
__device__ __forceinline__ int pair_id(const int* __restrict__ idOf, const u32* __restrict__ slotOf, u64 o) {
    if (!slotOf) return idOf[o];
    const u32 s = slotOf[o]; return s ? idOf[s - 1u] : 0;
}
__global__ void k_pair_keep(const int* __restrict__ idOf, const u32* __restrict__ slotOf, u64 rec0, u32 npairs, long long* ids, u32* keep, unsigned long long* cnt) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (j < npairs) {
        const u64 o = rec0 + 2ull * j;
        const int a = pair_id(idOf, slotOf, o), b = pair_id(idOf, slotOf, o + 1ull);
        bad = a == 0 || b == 0;
        ids[2ull * j] = a; ids[2ull * j + 1ull] = b; keep[j] = bad ? 0u : 2u;
    }
    const u64 mb = __ballot(bad);
    if (lane_id() == 0 && mb) atomicAdd(&cnt[0], (unsigned long long)__popcll(mb));
}
__global__ void k_mate_iota(u32* v, u32 n) { const u32 i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) v[i] = i; }
__global__ void k_mate_heads(const u64* __restrict__ keys, u32 n, u32* flag) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
    flag[i] = (i == 0 || keys[i - 1] != keys[i]) ? 1u : 0u;
}
__global__ void k_mate_reduce(const u64* __restrict__ keys, const u32* __restrict__ vals, const u64* __restrict__ ord, const u32* __restrict__ hp, u32 E,
                              u64* outKey, u64* outCnt, u64* outFirst) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x; if (e >= E) return;
    const u32 i = hp[e];
    outKey[e] = keys[i]; outCnt[e] = (u64)(hp[e + 1] - i); outFirst[e] = ord[vals[i]];
}
__global__ void k_mate_merge(const u64* __restrict__ keys, const u32* __restrict__ vals, const u64* __restrict__ cntIn, const u64* __restrict__ firstIn,
                             const u32* __restrict__ hp, u32 E, u64* outKey, u64* outCnt, u64* outFirst) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x; if (e >= E) return;
    const u32 i = hp[e], len = hp[e + 1] - i;                             // 1 or 2: both inputs hold a key once
    const u32 v0 = vals[i]; u64 c = cntIn[v0], f = firstIn[v0];
    if (len > 1u) { const u32 v1 = vals[i + 1]; c += cntIn[v1]; f = min(f, firstIn[v1]); }
    outKey[e] = keys[i]; outCnt[e] = c; outFirst[e] = f;
}
__global__ void k_mate_offsets(const u64* __restrict__ keys, u32 E, u32 N, u64* offsets) {
    const u32 a = blockIdx.x * blockDim.x + threadIdx.x; if (a > N + 1u) return;
    u32 lo = 0, hi = E;
    if (a == N + 1u) lo = E;
    else while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if ((u32)(keys[mid] >> 32) < a) lo = mid + 1u; else hi = mid;
    }
    offsets[a] = lo;
}
