// sage2_amd/csrc/kernels_probe_seq.inc -- sequential probe kernel (exact state machine; hit lists).
// Part of sage2ov_device.hip (included inside namespace s2, in this order); not a translation unit of its own.

// =============================================================================================
// probe + verify + extension state machine  (economyGraph.cpp:72-451), one wavefront per read.
// MODE 0: initial pass.  MODE 1: directional hit lists of status-0 reads (economyGraph.cpp:591-633).
// =============================================================================================
template <int S>
struct WaveLds {
    u64 x[2][S + 1];        // this read: forward strand, reverse complement (+1 zero pad word)
    u64 y[S + 1][64];       // candidate reads, word-major so lane-consecutive (row S = zero pad)
    u32 candJ[64], candE[64];
    u32 hitR2[64], hitA[64], hitB[64];   // A: side | o<<1 | L2<<2 | j<<18 ; B: overhang length
    u64 hitOv[S][64];       // overhang strings, left aligned
};

template <int S>
__device__ __forceinline__ u64 ybits(const u64 (*y)[64], u32 lane, int bitpos) {
    const int q = bitpos >> 6, r = bitpos & 63;
    const u64 a = y[q][lane], b = y[q + 1][lane];          // row S is a zero pad
    return (a << r) | ((b >> 1) >> (63 - r));
}
// n bases of X from xa equal n bases of candidate (lane column of y) from ya
template <int S>
__device__ __forceinline__ bool eq_range(const u64* x, int xa, const u64 (*y)[64], u32 lane, int ya, int n) {
    for (int c = 0; c * 32 < n; c++) {
        u64 a = bits64(x, S + 1, 2 * xa + 64 * c), b = ybits<S>(y, lane, 2 * ya + 64 * c);
        if ((a ^ b) & mask_top(n - 32 * c)) return false;
    }
    return true;
}

struct ProbeArgs {
    const u64* reads; u64 N; int S, k, h;                  // reads: the LOCALITY-ORDERED store (slot p = the read at position p; index entries are positions)
    const u32* idOf; const uint8_t* statusP;               // position -> read id (idOf[0] = 0); MODE 1: exploredReads by position
    const unsigned short* meta;                            // per position: (255 - offset of the read's global minimiser) | strand << 8, 0xFFFF = unknown (fast kernel: window reuse)
    const u64* slots; u64 T; const u32* csr; u64 seed;
    u64 lo, hi;                    // range of POSITIONS [lo, hi)
    u64* right; u64* left; u32* conn; u32* cflag;         // MODE 0 outputs
    Hit* hits; u64 hits_cap; u64* counters;                // MODE 1
    u32* hitcount;                                         // MODE 1, optional: number of hits of every read (written for status-0 reads)
    u64* hitBase;                                          // fast kernel, TAIL = 2, optional: the read's hits are written out in the initial pass; where they start (~0: not written)
    const u32* ids; u64 n_ids;                             // optional explicit list of positions (replaces [lo,hi))
    const u64* mi1; u64 TL; const u64* krec;               // minimiser index (may be null)
    u32* slow; u64 slow_cap;                               // fast kernel: reads handed to the sequential kernel (count in counters[CTR_HANDED])
    int uniL;                                              // the common read length when all reads have one (else 0): no length gathers
    u64* stamps;                                           // diagnostic build (-DSAGE2OV_STAMPS): wave cycles per phase
    // fast kernel: the grid in up to four PHASES {first block, blocks, rounds, first chunk}: a block of phase p walks chunks first chunk + (block - first block) + r * blocks,
    // r < rounds.  Later phases have fewer rounds, so the blocks that are dispatched last are short and the launch has no long tail (plan_fast_grid).
    u32 phase[4][4];
    u32 chunkShift;      // log2 of the positions a block takes per visit: FAST_CHUNK_LOG or FAST_CHUNK_LOG + 1 (plan_fast_grid)
    u32 noRun;           // 1: the sequential-groups form does not enter run mode (tests: both ways must give the same records; SAGE2OV_NO_RUN_MODE)
    u32 noParTail;       // 1: the state machine of the fast kernel steps through the hits one by one, never in its parallel form (tests: both ways, the same records; SAGE2OV_NO_PAR_TAIL)
    u32 runLanesMin;     // run mode: planned steps of this many reads and more compute their records with a lane per read; 0: plan, own-entry checks and records loop over the reads
                         // (RUN_LANES_MIN; tests: SAGE2OV_RUN_LANES=0, SAGE2OV_RUN_LANES_MIN=<n>: the same records every way)
};
#ifdef SAGE2OV_STAMPS
#define STAMP(k) do { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); const u64 t_ = __builtin_amdgcn_s_memtime(); st_acc[k] += t_ - st_prev; st_prev = t_; } while (0)
#else
#define STAMP(k) do { } while (0)
#endif

template <int S, int MODE, int WPB>
__global__ __launch_bounds__(64 * WPB) void k_probe(ProbeArgs A) {
    __shared__ WaveLds<S> lds_all[WPB];
    WaveLds<S>& W = lds_all[threadIdx.x >> 6];
    const u32 lane = lane_id();
    const u64 wave0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((u64)gridDim.x * blockDim.x) >> 6;
    const int k = A.k, h = A.h;
    if (lane <= 64 - 1) W.y[S][lane] = 0;

    const u64 first = A.ids ? 0 : A.lo, last = A.ids ? A.n_ids : A.hi;
    for (u64 it = first + wave0; it < last; it += nwaves) {
        const u64 i = A.ids ? (u64)A.ids[it] : it;
        const u32 iid = A.idOf[i];                                  // i is a position in the locality-ordered store
        if (MODE == 1) { if (A.statusP[i] != 0) continue; }         // (exploredReads by position: the copy by id exists on demand only, ensure_status_by_id)
        // ---- stage the read and its reverse complement in LDS
        wave_sync();
        if (lane < S) W.x[0][lane] = A.reads[i * S + lane];
        if (lane == S) { W.x[0][S] = 0; W.x[1][S] = 0; }
        wave_sync();
        const int L1 = (int)(W.x[0][S - 1] & slot_len_mask(S));
        if (lane < S) {
            int rem = L1 - 32 * (int)lane; u64 r;
            if (rem <= 0) r = 0;
            else if (rem >= 32) r = ~rev2(bits64(W.x[0], S + 1, 2 * (rem - 32)));
            else r = (~rev2(W.x[0][0] >> (64 - 2 * rem))) & mask_top(rem);
            W.x[1][lane] = r;
        }
        wave_sync();

        // ---- extension state (uniform across the wave)
        u64 rightId = 0, leftId = 0; u32 rightO = 0, leftO = 0, rightLen = 0, leftLen = 0;
        u32 pRL = 0, pRov = 0, pLL = 0, pLov = 0; u64 pR[S], pL[S];
#pragma unroll
        for (int c = 0; c < S; c++) { pR[c] = 0; pL[c] = 0; }
        int curJ = -1; bool mAR = false, mAL = false, mFR = false, ambR = false, ambL = false;
        u32 connections = 0; u32 seq = 0;

        const int nwin = L1 - h + 1;
        for (int jb = 0; jb < nwin; jb += 64) {
            // ---- probe: one window per lane
            const int j = jb + (int)lane;
            u32 cnt = 0; u32 pay = 0; bool inl = false;
            if (j < nwin) {
                u64 khi, klo; key_at(W.x[0], S + 1, j, h, khi, klo);
                u64 s = table_find(A.slots, A.T, hash_key(khi, klo, h, A.seed));
                u32 c7 = (u32)(s >> SLOT_CNT_SHIFT) & 127u;
                if (s != 0 && c7 != SLOT_CNT_LONG) { cnt = c7; pay = (u32)(s & SLOT_PAY_MASK); inl = (c7 == 1); }
            }
            // ---- expand buckets into candidates, 64 at a time, in (window, bucket) order
            u32 rem = cnt, cur = 0;
            for (;;) {
                u32 incl = wave_incl_scan(rem); u32 total = __shfl(incl, 63);
                if (total == 0) break;
                u32 excl = incl - rem, take = 0;
                if (excl < 64 && rem) {
                    take = min(rem, 64u - excl);
                    for (u32 e = 0; e < take; e++) { W.candJ[excl + e] = (u32)j | (inl ? 0u : 0x80000000u); W.candE[excl + e] = inl ? pay : pay + cur + e; }
                }
                rem -= take; cur += take;
                const u32 nb = min(total, 64u);
                wave_sync();
                // ---- verify: one candidate per lane
                bool isHit = false; u32 hr2 = 0, hA = 0, hov = 0; u64 ovw[S];
#pragma unroll
                for (int c = 0; c < S; c++) ovw[c] = 0;
                int hlen = 0; u32 htype = 0;
                if (lane < nb) {
                    u32 cj = W.candJ[lane], ce = W.candE[lane];
                    u32 entry = (cj & 0x80000000u) ? A.csr[ce] : ce;
                    const int jj = (int)(cj & 0x7FFFFFFFu);
                    const u64 r2 = entry >> 2; const int t = entry & 3;
                    const bool rightSide = (t == 0 || t == 2);
                    bool gate = (r2 != i) && (rightSide ? (jj <= L1 - k) : (jj >= k - h));
                    if (MODE == 1 && gate) gate = (A.statusP[r2] == 0);
                    if (gate) {
                        const u64* yp = A.reads + r2 * S;
#pragma unroll
                        for (int c = 0; c < S; c++) W.y[c][lane] = yp[c];
                        const int L2 = (int)(W.y[S - 1][lane] & slot_len_mask(S));
                        // overlap geometry (see DESIGN.md "mirrored compares"): region length n on both reads
                        const int span = rightSide ? (L1 - jj) : (jj + h);      // bases of read i from the window to its end
                        const bool cont = (L2 <= span);                          // read 2 ends inside read i
                        const int n = cont ? L2 : span;
                        bool eq;
                        if (t == 0)      eq = eq_range<S>(W.x[0], jj, W.y, lane, 0, n);
                        else if (t == 3) eq = eq_range<S>(W.x[1], L1 - jj - h, W.y, lane, 0, n);
                        else if (t == 2) eq = eq_range<S>(W.x[1], L1 - jj - n, W.y, lane, L2 - n, n);
                        else             eq = eq_range<S>(W.x[0], jj + h - n, W.y, lane, L2 - n, n);
                        if (MODE == 0) {
                            if (eq && cont) { const u32 id2 = A.idOf[r2]; atomicOr(&A.cflag[r2], iid > id2 ? 1u : 2u); }     // economyGraph.cpp:735
                            if (eq && !cont) {
                                isHit = true; hr2 = (u32)r2; hov = (u32)(L2 - n);
                                hA = (rightSide ? 0u : 1u) | ((u32)((t == 2 || t == 3) ? 1 : 0) << 1) | ((u32)L2 << 2) | ((u32)jj << 18);
                                const int ov = L2 - n;
                                if (t == 0 || t == 3) {   // overhang = tail of read 2
#pragma unroll
                                    for (int c = 0; c < S; c++) if (32 * c < ov) ovw[c] = ybits<S>(W.y, lane, 2 * n + 64 * c) & mask_top(ov - 32 * c);
                                } else {                  // overhang = reverse complement of the head of read 2
#pragma unroll
                                    for (int c = 0; c < S; c++) {
                                        int rm = ov - 32 * c;
                                        if (rm >= 32) ovw[c] = ~rev2(ybits<S>(W.y, lane, 2 * (rm - 32)));
                                        else if (rm > 0) ovw[c] = (~rev2(W.y[0][lane] >> (64 - 2 * rm))) & mask_top(rm);
                                    }
                                }
                            }
                        } else {
                            if (eq) {   // economyGraph.cpp:607-626: contained-and-equal counts as a hit here
                                isHit = true; hr2 = (u32)r2;
                                hlen = rightSide ? (L2 - (L1 - jj)) : (L2 - jj - h);
                                htype = t == 0 ? 3u : (t == 1 ? 0u : (t == 2 ? 2u : 1u));
                            }
                        }
                    }
                }
                const u64 hb = __ballot(isHit);
                const u32 nh = (u32)__popcll(hb);
                const u32 hidx = (u32)__popcll(hb & ((1ull << lane) - 1ull));
                if (MODE == 1) {
                    if (nh) {
                        u64 base = 0; if (lane == 0) base = atomicAdd(&A.counters[CTR_HIT_CURSOR], (u64)nh); base = __shfl(base, 0);
                        if (isHit && base + hidx < A.hits_cap) {
                            Hit hh; hh.from = iid; hh.to = A.idOf[hr2]; hh.len = hlen; hh.type = htype & 3u; hh.seq = seq + hidx;
                            A.hits[base + hidx] = hh;
                        }
                        seq += nh;
                    }
                    wave_sync();
                    continue;
                }
                if (isHit) {
                    W.hitR2[hidx] = hr2; W.hitA[hidx] = hA; W.hitB[hidx] = hov;
#pragma unroll
                    for (int c = 0; c < S; c++) W.hitOv[c][hidx] = ovw[c];
                }
                wave_sync();
                // ---- sequential extension state machine over the verified hits (economyGraph.cpp:95-438)
                for (u32 x = 0; x < nh; x++) {
                    const u32 a = W.hitA[x], ov = W.hitB[x]; const u64 r2 = W.hitR2[x];
                    const bool isLeft = a & 1; const u32 o = (a >> 1) & 1, L2 = (a >> 2) & 0xFFFF; const int jj = (int)(a >> 18);
                    u64 q[S];
#pragma unroll
                    for (int c = 0; c < S; c++) q[c] = W.hitOv[c][x];
                    if (jj != curJ) { curJ = jj; mAR = mAL = mFR = false; }
                    connections++;
                    if (!isLeft) {
                        if (rightId == 0) { rightId = r2; rightO = o; rightLen = ov; pRL = L2; pRov = ov; mAR = true; mFR = true;
#pragma unroll
                            for (int c = 0; c < S; c++) pR[c] = q[c];
                        } else {
                            const int m = (int)min(pRov, ov); bool cons = true;
#pragma unroll
                            for (int c = 0; c < S; c++) if (32 * c < m && ((pR[c] ^ q[c]) & mask_top(m - 32 * c))) cons = false;
                            if (cons) {
                                bool upd = false;
                                if (mAR) { if (L2 > pRL) { if (mFR) { rightId = r2; rightO = o; rightLen = ov; } upd = true; } }
                                else { upd = true; mAR = true; }
                                if (upd) { pRL = L2; pRov = ov;
#pragma unroll
                                    for (int c = 0; c < S; c++) pR[c] = q[c];
                                }
                            } else ambR = true;
                        }
                    } else {
                        if (leftId == 0) { leftId = r2; leftO = o; leftLen = ov; pLL = L2; pLov = ov; mAL = true;
#pragma unroll
                            for (int c = 0; c < S; c++) pL[c] = q[c];
                        } else {
                            const int m = (int)min(pLov, ov); bool cons = true;
#pragma unroll
                            for (int c = 0; c < S; c++) if (32 * c < m && ((pL[c] ^ q[c]) & mask_top(m - 32 * c))) cons = false;
                            if (cons) {
                                bool upd = false;
                                if (mAL) { if (L2 > pLL) upd = true; } else { upd = true; mAL = true; }
                                if (upd) { leftId = r2; leftO = o; leftLen = ov; pLL = L2; pLov = ov;
#pragma unroll
                                    for (int c = 0; c < S; c++) pL[c] = q[c];
                                }
                            } else ambL = true;
                        }
                    }
                }
                wave_sync();
            }
        }
        if (MODE == 1 && A.hitcount && lane == 0) A.hitcount[iid] = seq;
        if (MODE == 0 && lane == 0) {
            if (ambR || ambL) { rightLen = 0; leftLen = 0; }                                        // economyGraph.cpp:446-450
            A.right[i] = (u64)rightId | ((u64)rightO << 40) | ((u64)(rightLen & 0x3FFFFFu) << 42);      // (records by position, neighbours as positions)
            A.left[i] = (u64)leftId | ((u64)leftO << 40) | ((u64)(leftLen & 0x3FFFFFu) << 42);
            A.conn[i] = connections;
        }
    }
}


