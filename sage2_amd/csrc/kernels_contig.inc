// sage2_amd/csrc/kernels_contig.inc -- OverlapGraph::printGraph's contig table and saveContigsToFile's strings (overlapGraph.cpp:507-593, :607-784) over the
// resident step-4 graph and the 2-bit read store; the contract is stated in include/sage2ov.h.  Part of sage2ov_device.hip (included inside namespace s2, in this order).

// =============================================================================================
// The reference walks every node's list, sorts the edge pointers and spells one contig after the other, character by character, on one thread.  Here:
//   k_ct_degree      deg[i] = alive half-edges leaving i (getDegree, :595-602)
//   k_ct_select      one thread per half-edge: selected = alive, from >= to, len >= threshold, of a loop the half with the higher index; the longest selected edge
//   (scan)           the position of a selected half among the selected
//   k_ct_keys        the selected halves by DESCENDING index, key = (longest - len):32 | from:32
//   k_mate_iota, radix_sort_pairs   stable, only the passes whose digit can be non-zero: rows by (len descending, from ascending, index descending)
//   k_ct_gather      row -> half-edge
//   k_rm_dprev, k_ct_gaps, (scan) x 3   the running distPrevious, gap count and N count of every entry of the pool: a row's totals are two differences (a segmented
//                    reduction by scan; the longest edge holds millions of entries)
//   k_ct_layout      one thread per row: string length, trim, gap and N counts, consistency; its 16-byte chunks; (scan): where its chunks begin
//   k_ct_spell       one thread per 16 characters, stored with one 16-byte store.  The thread finds its row by binary search in the scanned chunk counts and its first
//                    list entry by binary search in the running distPrevious of the row's list, then steps entry by entry (with distPrevious = 1 sixteen entries meet
//                    in one chunk): no thread walks a list from its start.  No LDS, no scratch.
// Every count is kept below 2^32 - RS_TILE by the driver; list totals stay below 2^32.
// =============================================================================================
struct CtReads { const u64* store; const u32* posOf; int byPos; int S; u32 uniL, N, lenMask; };      // byPos: the locality-ordered store, read id at slot posOf[id] (memory-diet mode)
struct CtRow { u32 h, stringLength, contigLength, start, gapCount, nCount, flags, pad; };            // flags: CT_INCONSISTENT, CT_WRAPPED, CT_LIMIT
constexpr u32 CT_INCONSISTENT = 1u, CT_WRAPPED = 2u, CT_LIMIT = 4u;
__device__ __forceinline__ u32 ct_slot(const CtReads& R, u64 id) { return id > R.N ? 0u : (R.byPos ? R.posOf[id] : (u32)id); }      // (slot 0 is all zero: a read of no bases)
__device__ __forceinline__ u32 ct_len(const CtReads& R, u32 slot) { return slot == 0u ? 0u : (R.uniL ? R.uniL : ((u32)R.store[(u64)slot * R.S + (R.S - 1)] & R.lenMask)); }
__global__ void k_ct_degree(S4Graph g, u32 nh, u32* deg) { const u32 h = blockIdx.x * blockDim.x + threadIdx.x; if (h < nh && g.alive[h]) atomicAdd(&deg[g.from[h]], 1u); }
// ctr[0]: the longest selected edge
__global__ void k_ct_select(S4Graph g, u32 nh, u32 threshold, u32* sel, unsigned long long* ctr) {
    const u32 h = blockIdx.x * blockDim.x + threadIdx.x; if (h >= nh) return;
    const u32 f = g.from[h], t = g.to[h], len = g.len[h];
    const bool s = g.alive[h] && f >= t && len >= threshold && (f != t || (h & 1u));      // overlapGraph.cpp:533-547, :572
    sel[h] = s ? 1u : 0u;
    if (s) atomicMax(&ctr[0], (unsigned long long)len);
}
__global__ void k_ct_keys(S4Graph g, u32 nh, const u32* __restrict__ sel, const u32* __restrict__ pos, u32 R, u32 longest, u64* key, u32* hs) {
    const u32 h = blockIdx.x * blockDim.x + threadIdx.x; if (h >= nh || !sel[h]) return;
    const u32 i = R - 1u - pos[h];
    key[i] = ((u64)(longest - g.len[h]) << 32) | g.from[h]; hs[i] = h;
}
__global__ void k_ct_gather(const u32* __restrict__ vals, const u32* __restrict__ hs, u32 R, u32* rowH) { const u32 i = blockIdx.x * blockDim.x + threadIdx.x; if (i < R) rowH[i] = hs[vals[i]]; }
// per entry of the pool: 1 and distPrevious - L when distPrevious > L (a gap, overlapGraph.cpp:666-669), else 0 and 0
__global__ void k_ct_gaps(const u64* __restrict__ lists, u64 n, CtReads R, u32* gap, u32* ns) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 e = lists[i]; const u64 id = e & ((1ull << 40) - 1);
        const u32 L = ct_len(R, ct_slot(R, id)), dp = s4_dprev(e);
        gap[i] = dp > L ? 1u : 0u; ns[i] = dp > L ? dp - L : 0u;
    }
}
// dScan, gScan, nScan: exclusive scans over listUsed + 1 items (the last item is 0: scan[listUsed] is the total)
__global__ void k_ct_layout(S4Graph g, const u32* __restrict__ rowH, u32 R, CtReads Rd, const u32* __restrict__ deg, const u32* __restrict__ dScan, const u32* __restrict__ gScan,
                            const u32* __restrict__ nScan, u64 listUsed, CtRow* rows, u32* chunks) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x; if (i > R) return;
    if (i == R) { chunks[R] = 0; return; }
    const u32 h = rowH[i], f = g.from[h], t = g.to[h], len = g.len[h], off = g.off[h];
    u32 n = g.cnt[h], flags = 0;
    if ((u64)off + n > listUsed) { n = 0; flags |= CT_INCONSISTENT; }                        // (cannot happen on a consistent graph: nothing is read out of bounds)
    const u32 Lf = ct_len(Rd, ct_slot(Rd, f)), Lt = ct_len(Rd, ct_slot(Rd, t));
    const u64 sl = (u64)len + Lf;
    if (sl > 0xFFFFFFF0ull) flags |= CT_LIMIT;
    const u32 total = n ? dScan[off + n] - dScan[off] : 0u, nd = n ? s4_dnext(g.lists[off + n - 1]) : len;
    if ((u64)total + nd != len) flags |= CT_INCONSISTENT;
    const bool oneF = deg[f] == 1u, oneT = deg[t] == 1u;
    u32 cl, st;                                                                               // overlapGraph.cpp:699-724
    if (oneF && oneT) { cl = (u32)sl; st = 0; }
    else if (oneF) { if (len < Lt / 2) { flags |= CT_WRAPPED; cl = 0; } else cl = Lf + (len - Lt / 2); st = 0; }
    else if (oneT) { cl = (Lf - Lf / 2) + len; st = Lf - Lf / 2; }
    else { st = Lf - Lf / 2; if (len < Lt / 2) { flags |= CT_WRAPPED; cl = 0; } else cl = st + (len - Lt / 2); }
    CtRow r; r.h = h; r.stringLength = (u32)sl; r.contigLength = cl; r.start = st; r.gapCount = n ? gScan[off + n] - gScan[off] : 0u; r.nCount = n ? nScan[off + n] - nScan[off] : 0u;
    r.flags = flags; r.pad = 0;
    rows[i] = r; chunks[i] = (flags & CT_LIMIT) ? 0u : (u32)((sl + 15) >> 4);
}
// the read a segment of the string is copied from: character at string position q is base (q + delta) of the read as it is spelled (reverse-complemented when rc);
// a negative index is a gap's N
struct CtSeg { u32 end, slot, L; int delta; bool rc, valid; };
__global__ void __launch_bounds__(256) k_ct_spell(S4Graph g, CtReads R, const CtRow* __restrict__ rows, const u32* __restrict__ chunkOff, u32 first, u32 count,
                                                  const u32* __restrict__ dScan, u64 listUsed, uint4* out, u32 nChunks) {
    const u32 c = blockIdx.x * blockDim.x + threadIdx.x; if (c >= nChunks) return;
    const u32 base = chunkOff[first];
    u32 lo = first, hi = first + count;
    while (lo < hi) { const u32 mid = lo + ((hi - lo) >> 1); if (chunkOff[mid] - base <= c) lo = mid + 1u; else hi = mid; }
    const u32 row = lo - 1u;
    const u32 q0 = (c - (chunkOff[row] - base)) * 16u;
    const u32 h = rows[row].h, SL = rows[row].stringLength;
    const u32 f = g.from[h], t = g.to[h], ty = g.type[h], len = g.len[h], off = g.off[h];
    const u32 n = (u64)off + g.cnt[h] > listUsed ? 0u : g.cnt[h];
    const u32 slotF = ct_slot(R, f), Lf = ct_len(R, slotF);
    const u64* __restrict__ lst = g.lists + off;
    CtSeg s; u32 k;                                                                           // k: the entry the next advance loads; n: the last read; n + 1: nothing more
    auto entry = [&](u32 x, u32 segStart) {
        const u64 e = lst[x]; const u64 id = e & ((1ull << 40) - 1); const u32 dp = s4_dprev(e);
        s.slot = ct_slot(R, id); s.L = ct_len(R, s.slot);
        s.end = segStart + dp; s.delta = (int)s.L - (int)dp - (int)segStart; s.rc = ((e >> 40) & 1ull) == 0; s.valid = true;      // :655-679
    };
    auto last = [&](u32 segStart) {
        const u32 nd = n ? s4_dnext(lst[n - 1]) : len;
        s.slot = ct_slot(R, t); s.L = ct_len(R, s.slot);
        const bool copies = nd <= s.L;                                                        // :696: the unsigned loop start wraps otherwise and nothing is copied
        s.end = copies ? segStart + nd : segStart; s.delta = (int)s.L - (int)nd - (int)segStart; s.rc = !(ty == 1u || ty == 3u); s.valid = true;
    };
    auto advance = [&]() {
        if (k < n) entry(k, s.end); else if (k == n) last(s.end); else { s.end = 0xFFFFFFFFu; s.valid = false; }
        k++;
    };
    if (q0 < Lf) { s.end = Lf; s.slot = slotF; s.L = Lf; s.delta = 0; s.rc = ty <= 1u; s.valid = true; k = 0; }      // :641-647
    else {
        const u32 r = q0 - Lf, d0 = dScan[off], total = n ? dScan[off + n] - d0 : 0u;
        if (r >= total) { last(Lf + total); k = n + 1u; }
        else {
            u32 a = 0, b = n;                                                                 // the last entry whose running sum in front of it is <= r
            while (a < b) { const u32 mid = a + ((b - a) >> 1); if (dScan[off + mid] - d0 <= r) a = mid + 1u; else b = mid; }
            entry(a - 1u, Lf + (dScan[off + a - 1u] - d0)); k = a;
        }
    }
    u32 w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    u64 cw = 0, cwAt = ~0ull;                                                                 // the word of the read store the previous character came from
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const u32 q = q0 + (u32)i;
        while (q >= s.end) advance();
        u32 ch = 'N';
        const int idx = (int)q + s.delta;
        if (s.valid && q < SL && idx >= 0 && (u32)idx < s.L) {
            const u32 p = s.rc ? s.L - 1u - (u32)idx : (u32)idx;
            const u64 at = (u64)s.slot * R.S + (p >> 5);
            if (at != cwAt) { cw = R.store[at]; cwAt = at; }
            u32 bs = (u32)(cw >> (62u - 2u * (p & 31u))) & 3u; if (s.rc) bs = 3u - bs;
            ch = (0x54474341u >> (8u * bs)) & 0xFFu;                                          // "ACGT"
        }
        const u32 v = ch << (8 * (i & 3));
        if (i < 4) w0 |= v; else if (i < 8) w1 |= v; else if (i < 12) w2 |= v; else w3 |= v;
    }
    out[c] = make_uint4(w0, w1, w2, w3);
}
