// sage2_amd/csrc/kernels_find.inc -- ReadLoader::getIdOfRead (readLoader.cpp:319-353) for a batch of queries: which id and orientation did a read receive?
// Part of sage2ov_device.hip (included inside namespace s2, in this order); not a translation unit of its own.

// =============================================================================================
// The reference canonicalises the query, packs it and binary-searches the sorted read list with stringCompareInBytes (utils.cpp:224).  Here:
//   k_org_classify   (kernels_organize.inc) isGoodRead of every query; maxLen = the store's longest read (nothing longer can be in it)
//   k_find_pack      every good query as an S-word slot in canonical orientation at ITS OWN position r (no compaction: result r belongs to query r)
//                    + one sign byte: +1 the query is its own canonical form, -1 its reverse complement is, 0 not a good read
//   k_find_dir       dir[b] = first id whose word 0 has top B bits >= b (b = 0 .. 2^B; dir[2^B] = N + 1): one thread per bucket, binary search over
//                    word 0 of the store (the pattern of k_pt_bounds_search).  Built once per read set, kept on the device object.
//   k_find_search    a query's bucket [dir[b], dir[b + 1]) is a handful of reads for ordinary data; inside it a binary search with the full slot
//                    compare (words in order, the last one carrying the length = stringCompareInBytes).  A group of S/2 lanes serves one query: lane c keeps
//                    16-byte piece c of the query in registers and loads piece c of the probed slot (one contiguous request of the slot's size per
//                    probe); the first differing piece decides, found by a ballot inside the group.  Any bucket size is exact; a large one only costs
//                    log2(size) probes.
// BYPOS: the id-ordered store was released (memory-diet mode, reads of one length); slot id is then slot posOf[id] of the locality-ordered store.
// =============================================================================================
constexpr int FIND_B_MIN = 4, FIND_B_MAX = 24;             // directory bits: ceil(log2 N) - 1 clamped to this range (64 bytes .. 64 MB of directory)

__global__ void k_find_pack(const unsigned char* __restrict__ bases, const u64* __restrict__ off, u64 n, const u32* __restrict__ flag, int S, u64* img, signed char* sign) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
    if (!flag[i]) { sign[i] = 0; return; }
    const u64 a = off[i]; const int L = (int)(off[i + 1] - a); u64 w0;
    sign[i] = org_pack_slot(bases, a, L, S, img + i * S, w0) ? (signed char)1 : (signed char)-1;
}
template <bool BYPOS> __global__ void k_find_dir(const u64* __restrict__ store, const u32* __restrict__ posOf, u32 N, int S, int B, u32* dir) {
    const u32 b = blockIdx.x * blockDim.x + threadIdx.x, nb = 1u << B; if (b > nb) return;
    u32 lo = 1, hi = N + 1;
    if (b == nb) lo = N + 1;
    else while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        const u64 w0 = store[(u64)(BYPOS ? posOf[mid] : mid) * S];
        if ((u32)(w0 >> (64 - B)) < b) lo = mid + 1u; else hi = mid;
    }
    dir[b] = lo;
}
template <int S, bool BYPOS> __global__ __launch_bounds__(256) void k_find_search(const u64* __restrict__ store, const u32* __restrict__ posOf, const u32* __restrict__ dir, int B,
                                                                                  const u64* __restrict__ img, const signed char* __restrict__ sign, u32 n, long long* ids,
                                                                                  unsigned long long* found) {
    constexpr int G = S / 2;                                             // lanes per query: 2, 4, 8, 16 (a group never straddles a wave)
    static_assert(G >= 2 && G <= 16 && (G & (G - 1)) == 0, "group");
    const u32 t = blockIdx.x * 256u + threadIdx.x, q = t / G; const int c = (int)(t % G);
    const u32 gbase = lane_id() & ~(u32)(G - 1); constexpr u32 gmask = (1u << G) - 1u;
    const bool live = q < n; const int sg = live ? (int)sign[q] : 0;
    ulonglong2 qv = {0ull, 0ull}; u32 lo = 0, hi = 0, res = 0;
    if (sg) {
        qv = ((const ulonglong2*)img)[(u64)q * G + c];
        const u32 b = (u32)(img[(u64)q * S] >> (64 - B));
        lo = dir[b]; hi = dir[b + 1];
    }
    // (the loop is uniform over the wave: groups that are done idle through the remaining rounds, so every ballot is taken by all 64 lanes)
    while (__ballot(lo < hi)) {
        const bool act = lo < hi; const u32 mid = lo + ((hi - lo) >> 1);
        ulonglong2 sv = qv;
        if (act) sv = ((const ulonglong2*)store)[(u64)(BYPOS ? posOf[mid] : mid) * G + c];
        const bool ne = sv.x != qv.x || sv.y != qv.y, lt = sv.x != qv.x ? sv.x < qv.x : sv.y < qv.y;          // lt: this piece of the slot < the query's
        const u32 mne = (u32)(__ballot(ne) >> gbase) & gmask, mlt = (u32)(__ballot(lt) >> gbase) & gmask;
        if (act) {
            if (!mne) { res = mid; lo = hi; }                              // every piece equal: bytes and length (the store holds a read once)
            else if ((mlt >> (__ffs((int)mne) - 1)) & 1u) lo = mid + 1u;   // the first differing piece decides
            else hi = mid;
        }
    }
    const bool lead = live && c == 0;
    if (lead) ids[q] = sg > 0 ? (long long)res : -(long long)res;
    const u64 mf = __ballot(lead && res != 0);
    if (lane_id() == 0 && mf) atomicAdd(found, (unsigned long long)__popcll(mf));
}
