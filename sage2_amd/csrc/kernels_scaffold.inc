// sage2_amd/csrc/kernels_scaffold.inc -- ScaffoldMaker::mergeDisconnectedEdges for a batch of edge-disjoint joins (matePair/scaffolding.cpp:281-482,
// OverlapGraph::getListOfReadsInDisconnectedEdges and stringOverlapSize, overlapGraph.cpp:789-907) over the resident step-4 graph and the 2-bit read store
// (DESIGN.md 5.17; the contract is JOIN in include/sage2ov.h).
// Part of sage2ov_device.hip (included inside namespace s2, after kernels_contig.inc: CtReads, ct_slot, ct_len, and kernels_splice.inc); not a translation unit of its own.
//
// A join is (a, b, gap): half-edge a = e1 and half-edge b = e2 need not share a node.  Direction 0 of join i is the forward list (first = a, second = b),
// direction 1 the twin's (first = b ^ 1, second = a ^ 1); node1 = to[first], node2 = from[second].  node1 == node2 holds in both directions or in neither.
// The new pair of join i is half-edges nh + 2 i, nh + 2 i + 1 (nothing is refused).  This file holds the overlap search and the join's plan kernel; the lists and
// the commit are the splice's (kernels_splice.inc).

constexpr int SC_WORDS = SLOT_MAX_WORDS + 2;      // a read is at most 32 words of 32 bases; a funnel shift reads one word past the last one
// bases p .. p + 31 of the stored (forward) read in `slot`, MSB first like the store, positions outside [0, L) as zero bits; p may be negative
__device__ __forceinline__ u64 sc_fwd_bits(const CtReads& R, u32 slot, int L, int p) {
    const int lowT = p < 0 ? -p : 0, highT = (L - p) < 32 ? (L - p) : 32;
    if (highT <= lowT) return 0;
    const int wi = p >> 5; const u32 sh = 2u * (u32)(p & 31);
    const u64* __restrict__ w = R.store + (u64)slot * R.S;
    const u64 hi = (wi >= 0 && wi < R.S) ? w[wi] : 0ull, lo = (wi + 1 >= 0 && wi + 1 < R.S) ? w[wi + 1] : 0ull;
    const u64 x = sh ? (hi << sh) | (lo >> (64u - sh)) : hi;
    const u64 from = ~0ull >> (2 * lowT), upto = highT >= 32 ? 0ull : (~0ull >> (2 * highT));
    return x & from & ~upto;
}
// word w (bases 32 w .. 32 w + 31) of the read as the reference spells it: the stored read, or its reverse complement; bases from L on are zero bits
__device__ __forceinline__ u64 sc_oriented_word(const CtReads& R, u32 slot, int L, bool forward, int w) {
    if (forward) return sc_fwd_bits(R, slot, L, 32 * w);
    u64 x = sc_fwd_bits(R, slot, L, L - 32 - 32 * w);                                // stored bases L - 32 w - 32 .. L - 32 w - 1: reversed they are bases 32 w .. of the other strand
    x = __brevll(x); x = ((x & 0x5555555555555555ull) << 1) | ((x >> 1) & 0x5555555555555555ull);      // the 2-bit groups in reverse order, each group's bits in place
    const int n = L - 32 * w;                                                        // complement (3 - base) where there is a base
    const u64 valid = n >= 32 ? ~0ull : (n <= 0 ? 0ull : ~(~0ull >> (2 * n)));
    return ~x & valid;
}
// stringOverlapSize(string1, string2, L1, L2) (overlapGraph.cpp:884-907): the smallest shift i in [0, L1 - 10) with L2 - i >= 0 at which the bases string1[i + j] !=
// string2[j], j in [0, L2 - i), number at most (L2 - i) / 10 + 1; a position of string1 from L1 on counts as a mismatch (the reference reads past its string there:
// equality with it is claimed for L2 <= L1); -1 when no shift passes.
// One wave (one block of 64) per search: search s = 2 i + direction of join i.  The wave spells both reads into LDS, 32 bases a word (lanes 0-31 string1, lanes
// 32-63 string2), then lane l takes shift base + l: word by word, XOR of string2's word with the funnel-shifted words of string1, the two bits of a base folded into
// one, popcount.  The smallest passing shift of the 64 is the lowest bit of the ballot; the next 64 shifts are tried only when none passed.
// ov[s]: the shift, -1, or SC_NO_SEARCH when node1 == node2 (the reference does not search there)
constexpr int SC_NO_SEARCH = -2;
__global__ void __launch_bounds__(64) k_sc_overlap(S4Graph g, CtReads R, const u32* __restrict__ ha, const u32* __restrict__ hb, u32 n2, int* __restrict__ ov) {
    __shared__ u64 A[SC_WORDS], B[SC_WORDS];
    const u32 s = blockIdx.x; if (s >= n2) return;
    const u32 lane = threadIdx.x;
    const u32 a = ha[s >> 1], b = hb[s >> 1];
    const u32 first = (s & 1u) ? (b ^ 1u) : a, second = (s & 1u) ? (a ^ 1u) : b;
    const u32 node1 = g.to[first], node2 = g.from[second];
    if (node1 == node2) { if (lane == 0) ov[s] = SC_NO_SEARCH; return; }
    const u32 t1 = g.type[first], t2 = g.type[second];
    const bool fwd1 = t1 == 1u || t1 == 3u, fwd2 = t2 == 2u || t2 == 3u;             // overlapGraph.cpp:800-824
    const u32 slot1 = ct_slot(R, node1), slot2 = ct_slot(R, node2);
    const int L1 = min((int)ct_len(R, slot1), 32 * SLOT_MAX_WORDS), L2 = min((int)ct_len(R, slot2), 32 * SLOT_MAX_WORDS);      // (a stored read is shorter: the LDS words bound every index)
    {
        const int w = (int)(lane & 31u);
        const u64 v = lane < 32u ? sc_oriented_word(R, slot1, L1, fwd1, w) : sc_oriented_word(R, slot2, L2, fwd2, w);
        if (lane < 32u) A[w] = v; else B[w] = v;
        if (lane < (u32)(SC_WORDS - 32)) { A[32 + lane] = 0; B[32 + lane] = 0; }
    }
    __syncthreads();
    const int shifts = L1 - 10, common = L1 < L2 ? L1 : L2, beyond = L2 > L1 ? L2 - L1 : 0;      // beyond: positions of string2 that always face the end of string1
    int found = -1;
    for (int base = 0; base < shifts; base += 64) {
        const int i = base + (int)lane;
        bool pass = false;
        if (i < shifts && L2 - i >= 0) {
            const int cmp = common - i;                                              // bases compared: j in [0, cmp)
            const u32 wi = (u32)i >> 5, sh = 2u * ((u32)i & 31u);
            int mis = beyond;
            for (int w = 0; 32 * w < cmp; w++) {
                const u64 hi = A[wi + w], lo = A[wi + w + 1];
                const u64 x = (sh ? (hi << sh) | (lo >> (64u - sh)) : hi) ^ B[w];
                u64 m = (x | (x >> 1)) & 0x5555555555555555ull;
                const int left = cmp - 32 * w;
                if (left < 32) m &= ~(~0ull >> (2 * left));
                mis += __popcll(m);
            }
            pass = mis <= (L2 - i) / 10 + 1;
        }
        const u64 hit = __ballot(pass);
        if (hit) { found = base + (int)__ffsll((unsigned long long)hit) - 1; break; }
    }
    if (lane == 0) ov[s] = found;
}

constexpr uint8_t SC_EQUAL = 0, SC_OVERLAP = 1, SC_CONCAT = 2, SC_GAPPED = 3;          // SplicePlan::how, per direction
// one thread per join: the type by the four-way rule (scaffolding.cpp:290-297), delete or keep at flow 1.0 (:301, :344), the distances and both edge lengths
// (overlapGraph.cpp:827-859; unwrapped: the entry keeps 11 bits, the length all), into the splice record (kernels_splice.inc: nothing is refused, two middle entries
// unless the end nodes are equal); lens[2 i], lens[2 i + 1]: the lengths of the two new lists
__global__ void k_sc_plan(S4Graph g, CtReads R, const float* __restrict__ flow, const u32* __restrict__ ha, const u32* __restrict__ hb, const int* __restrict__ gaps,
                          const int* __restrict__ ov, u32 n, SplicePlan* plan, u32* lens) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
    const u32 a = ha[i], b = hb[i]; const int gap = gaps[i];
    SplicePlan p = {}; p.a = a; p.b = b; p.made = 1; p.flow = 1.0f;
    const u32 t1 = g.type[a], t2 = g.type[b];
    p.type = (uint8_t)(((t1 == 2u || t1 == 3u) ? 2u : 0u) | ((t2 == 1u || t2 == 3u) ? 1u : 0u));
    p.del1 = (flow ? flow[a] : 0.f) <= 1.0f; p.del2 = (flow ? flow[b] : 0.f) <= 1.0f;      // flow null: every flow is 0
    const bool equal = g.to[a] == g.from[b];
    p.extra = equal ? 1 : 2;
    u32 len[2];
#pragma unroll
    for (int d = 0; d < 2; d++) {
        const u32 first = d ? (b ^ 1u) : a, second = d ? (a ^ 1u) : b;
        u32 add = 0, d1 = 0, d2 = 0; uint8_t how = SC_EQUAL;
        if (!equal) {
            const u32 L1 = ct_len(R, ct_slot(R, g.to[first])), L2 = ct_len(R, ct_slot(R, g.from[second]));
            const int o = ov[2 * i + d];
            if (o > 0) { d1 = d2 = (u32)o; how = SC_OVERLAP; }                       // (a shift of 0 is "no overlap" to the reference, :837)
            else if (gap < 0) { d1 = L1; d2 = L2; how = SC_CONCAT; }
            else { d1 = (u32)gap + L1; d2 = (u32)gap + L2; how = SC_GAPPED; }
            add = d1;
        }
        p.dNext1[d] = d1; p.dPrev2[d] = d2; p.how[d] = how;
        len[d] = g.len[first] + g.len[second] + add;
    }
    p.lenF = len[0]; p.lenT = len[1];
    plan[i] = p;
    const u32 l = g.cnt[a] + g.cnt[b] + p.extra;
    lens[2 * i] = l; lens[2 * i + 1] = l;
}
