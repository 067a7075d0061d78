// sage2_amd/csrc/kernels_probe_fast.inc -- the hot kernel: fast probe + verify + extension, hit-list form, in-kernel state machine.
// Part of sage2ov_device.hip (included inside namespace s2, in this order); not a translation unit of its own.
// (What the kernel is fed with decides its traffic as much as its code does; the recorded PMC figures under profiles/ are keyed by a hash of this file, so the
//  layout the host hands it is noted here -- revision 2, end of round 3: locality order on all 32 bits of the minimiser hash, minimiser groups by the share of reads without a predecessor.)

// =============================================================================================
// FAST probe + verify kernel (the hot kernel), all-32-bit arithmetic.
// Same results as k_probe<S,0> for every read whose verified hits are mutually consistent (every right
// overhang is a prefix of the longest one, same on the left): then the extension state machine of
// economyGraph.cpp:95-438 never raises an ambiguity flag and reduces to
//     right = in the FIRST window with a right hit, the hit with the largest L2 (first in bucket order on ties)
//     left  = in the LAST  window with a left  hit, the hit with the largest L2 (first in bucket order on ties)
//     connections = number of verified hits
// which needs no sequential pass.  Anything else (an inconsistent hit, more than 128 candidates, a failed
// speculation) sends the read to the sequential kernel.  One wavefront per read:
//   1. WPL windows per lane: key (funnel shifts out of LDS) -> lookup3 hash -> open-addressed probes, all
//      chains of a lane in flight together
//   2. bucket sizes -> DPP wave scan -> <= 128 candidates, two per lane, both 64-byte gathers in flight
//   3. speculation: the candidate reaching furthest right (left) is the longest-overhang hit if it verifies;
//      the read extended by its overhang is written to LDS in both orientations (lanes 0-31 right, 32-63 left)
//   4. every candidate compared ONCE, over its whole length, with that extended string: the first mismatch
//      position classifies it as hit+consistent / not a hit / hit but inconsistent
//   5. DPP wave reductions pick the extension records
// Forms (template parameters): HITS (hit lists for the reduce phase), TAIL (0: inconsistent reads are listed; 1: their state machine is part of the kernel; 2: every read
// goes through it), UNI (one read length: no per-candidate length registers), QN / SEQ (round 3: QN groups of 64 candidate slots, gathered and compared one after the other
// into the same registers -- the reach of a candidate is known before it is fetched when all reads have one length -- : eight waves per SIMD with two groups, 256 candidates
// with four).  Register budgets, occupancy and the measurements behind them: DESIGN.md 5.2.
// =============================================================================================
constexpr u64 MI_SCAN_PAD = 272;   // records behind krec[]: the scan of a small group runs up to the wave's largest group (< 255) rounded up to 16
constexpr int FAST_CAP = 128;
// dwords per stored overhang in the in-kernel state machine: 8 (128 bases) for the 10-dword layouts, 16 for the 16-dword layout
// (251-bp reads overhang by up to 210 bases); longer overhangs go to the sequential kernel
// (round 3: the 16-word layout keeps whole-candidate overhangs -- a 300-base read overhangs by up to 260 bases, and with the 255-base limit of the
// 16-dword form nearly every inconsistent 300-base read went to the sequential kernel -- and the packed geometry 10 bits of the length)
template <int NW> struct TailOvw { static constexpr int value = NW <= 10 ? 8 : (NW <= 16 ? 16 : NW); };
constexpr int FAST_CHUNK = 128;                    // reads per block visit, the small size (ProbeArgs::chunkShift = log2 of the launch's size: this one or twice as many).
                                                   // A wave's first read of a visit has no predecessor to take windows over from; with the locality order on 32 hash bits and
                                                   // every look-up through the uniform table such a read costs 111 random table lines: 128 / 256 / 512 positions per visit ->
                                                   // 60.0 / 59.1 / 59.9 ms per pass at BASELINE configs[2], but 11.8 / 13.0 at configs[1] (coarser grid): the host picks per launch
constexpr int FAST_CHUNK_LOG = FAST_CHUNK == 64 ? 6 : (FAST_CHUNK == 128 ? 7 : (FAST_CHUNK == 256 ? 8 : 9));
static_assert((1 << FAST_CHUNK_LOG) == FAST_CHUNK, "FAST_CHUNK: 64, 128, 256 or 512");
#ifdef SAGE2OV_CUT     // diagnostic builds: a read is dropped after stage SAGE2OV_CUT (its live values go to a sink that never fires): instruction counts per stage by PMC difference
#define CUT(n, expr) if (SAGE2OV_CUT == (n)) { const u32 sk_ = (u32)(expr); if (sk_ == 0x9E3779B9u) A.conn[0] = sk_; continue; } else (void)0    /* (no do-while: `continue` must reach the read loop) */
#else
#define CUT(n, expr) do { } while (0)
#endif
constexpr int SCAN_U = 3;                          // group records a lane compares per round of the scan (all loads of a round in flight).  (Round 3: 8 records per window in flight
                                                   // were the kernel's register peak -- 16 x u64 per lane; with 3 the 10-dword layouts fit 96 VGPRs = five waves per SIMD)
constexpr int DIRECT_MAX = 16;                     // a reuse read with at most this many windows left looks them up in the uniform table directly
// RUN MODE (round 4; the sequential-groups form only: one read length).  The locality order lines the reads of one stretch of genome up, each starting a few bases after
// the one before; the per-read algorithm above re-derives for every one of them what its predecessor already knew: 58 of its 62 candidates, all verified against the same
// bases.  In run mode a wave keeps, across the reads of a run, (1) a FRAME: the genome as far as it has been verified, forward (G) and reverse complement (RCG), anchored
// RUN_OFF bases in front of the run's first read; (2) the SLOT LIST of the current read -- entry and window of every bucket entry of its windows, in window / bucket order,
// as a ring (a read's step drops the slots of its first d windows and appends those of d new ones); every slot in it is a read that has been compared with the frame over
// its WHOLE length at the frame position its window and type imply (or is the current read itself).  The next read of the run then (a) finds its own prefix entry among the
// slots of window d -- which proves that it IS the frame from there on, without loading a base of it --, (b) looks up its d new windows with keys cut out of the frame,
// (c) compares the handful of new entries with the frame, dword-parallel (16 lanes per candidate, one dword each), growing the frame by the one that reaches furthest,
// and (d) reads its extension records and its connection count off the list.  No staging, no reverse complement, no speculated reads, no strings, no gather of 60
// candidates: ~0.3 of the instructions of the general path.  Exactness: the general path accepts a read iff every gated candidate equals the read's extended strings over its
// whole length; those strings are pieces of the frame (the read, its furthest-reaching neighbours: all verified against it), so "every slot equals the frame" is the same
// statement, and the records follow from the list by the same tie rules (first window / last window, bucket order).  Anything else -- a candidate that does not verify, a
// read whose entry is not where it should be, a long shift, k > 64 (gates that depend on the window), a palindromic own entry -- ends the run and the read takes the
// general path, whose successful end starts the next run.  DESIGN.md 5.2.
constexpr int PAR_MAXIT = 8;                       // rounds of the state machine's parallel form before a read is handed to the steps
constexpr int RUN_OFF = 160;                       // frame position of the run's first read (>= L - k: the furthest start of a left neighbour)
constexpr int RUN_FD = 64, RUN_F = 16 * RUN_FD;    // dwords / bases of a frame: RUN_OFF + read + the shifts of a run (minimiser offsets: < read) + right overhang -- and, after a mirror
                                                   // (the second strand of the minimiser), the same again from the other end: 1024 bases, one dword per lane
constexpr int RUN_DMAX = 64;                       // largest shift of a step in run mode (lanes that look the new windows up: at most 64)
constexpr u32 RUN_NMAX = 64;                       // most new slots per step (compared four per pass; at most 64)
constexpr int RUN_NPRE = 3;                        // passes of a step's new-slot compare whose dwords are loaded up front (a pass beyond them is one more dependent round trip)
constexpr u32 RUN_MMAX = 16;                       // most reads per step (the plan: 2 words each in LDS)
constexpr int RUN_PF = 16;                         // windows behind a step's whose table pairs are fetched ahead
constexpr int RUN_PW = 256;                        // window numbers are told apart mod this: the <= 128 windows of a read + the RUN_DMAX of a step fit
constexpr u32 RUN_LANES_MIN = 3;                   // reads of a planned step from which its records are computed with a lane per read (fewer: a loop over the reads; DESIGN.md 5.2)
constexpr int RSX_CNT = 2 * RUN_MMAX, RSX_LMIN = RSX_CNT + 4, RSX_WORDS = RSX_LMIN + 2;      // rsx[] behind the plan: the wave's four run counters (CTR_RUNSTATS), the threshold above as the launch set it
static_assert(RUN_DMAX <= 64 && RUN_NMAX <= 64 && RUN_MMAX >= 1 && RUN_MMAX <= 64 && 128 + RUN_DMAX <= RUN_PW, "run mode limits");
// SPEC: the form speculates (extended strings e[], the two furthest-reaching reads m[]); the form that sends every read through the state machine (TAIL = 2) does not,
// and its LDS decides its occupancy: without them and with candidate rows of NW + 1 dwords it keeps 8.0 KB per wave at NW = 10 -- five waves per SIMD instead of four.
template <int S, int NW, bool TAILED, int WPL, int CAPS = FAST_CAP, bool RUN = false, bool SPEC = true>
struct FastLds {                   // every string has one zero dword in front (index 0) so that bit positions down to -32 are readable
    u32 xf[2][1 + 2 * S + 2];      // forward, reverse complement as big-endian dwords (+ zero pad behind)
    u32 e[4][SPEC ? 1 + 6 * S + 2 : 1];       // XR0 = fwd ++ right overhang, XR1 = rc(XR0), XL0 = rc ++ left overhang, XL1 = rc(XL0)
    u32 m[2][SPEC ? 1 + 2 * S + 2 : 1];       // the two speculated longest-reach reads
    u32 xp[1 + 2 * S + 2];         // the PREVIOUS read of this wave (forward strand): window reuse
    u64 psl[64 * WPL];             // ... and the slot word of each of its windows (window j at index j): read back by window number, no lane shuffles, no registers across reads
    u32 candJ[CAPS], candSrc[TAILED ? CAPS : 1];   // (after the entries are resolved the two arrays hold the packed geometry / read id of the verified hits)
    // inconsistent reads only (the in-kernel state machine): one padded row per lane to cut overhangs out of a candidate, and the
    // overhang of every verified hit (<= 128 bases) in this read's orientation
    // run mode: the slot ring (entry, absolute window of every slot), per absolute window (mod RUN_PW) {first slot of the ring | count << 8}, the frame, a row for the read that
    // extends it, and the state {on, minimiser offset and strand of the current read, its frame position, frame end, ring start, slots, frame start}
    u32 pent[RUN ? CAPS : 1]; unsigned short sJ[RUN ? CAPS : 1]; unsigned short pcw[RUN ? RUN_PW : 1]; u32 rst[8]; int rsx[RUN ? RSX_WORDS : 1];      // (rsx: the plan of a step for several reads: cumulative shifts, offset words; behind it the wave's run counters and the lane-form threshold)
    u32 G[RUN ? 1 + RUN_FD + 2 : 1], RCG[RUN ? 1 + RUN_FD + 2 : 1], mrow[RUN ? 1 + NW + 3 : 1];
    uint8_t tslotIdx[TAILED ? FAST_CAP : 4];          // slot number of the x-th verified hit (visiting order)
    // per candidate slot: one dword in front, the candidate's NW dwords, then its overhang in place.  Rows of NW + 1 dwords (odd: a lane per row is conflict-free; NW + 3
    // with two zero dwords behind until round 4): the extraction reads one dword in front of and one behind the bases it keeps -- the neighbouring rows' dwords, whatever
    // they hold, under a mask that drops them (get32 with 0 <= p < 2 L2) -- so neither pad's VALUE is ever used; tpad keeps the last row's look behind inside the block.
    u32 tslot[TAILED ? FAST_CAP : 1][TAILED ? NW + 1 : 1]; u32 tpad[TAILED ? 2 : 1];
};
// lane shuffle over the whole wave, `src` in 0..63: HIP's __shfl adds the caller's own lane number and a width mask (an mbcnt pair kept in two registers for the whole
// kernel and three extra instructions per shuffle); ds_bpermute takes the byte address of the source lane's register directly
__device__ __forceinline__ int shfl64(int v, int src) { return __builtin_amdgcn_ds_bpermute(src << 2, v); }
__device__ __forceinline__ u32 rev2_32(u32 x) { x = __brev(x); return ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1); }
// the top 2 x nb bits (nb bases), nb clamped to 0 .. 16: the 32 - 2 nb low bits go in two shifts of at most 16 (v_med3 + two shifts + not, where two compares and two selects
// around one shift were seven instructions)
__device__ __forceinline__ u32 mask_top32(int nb) { const int t = 16 - min(max(nb, 0), 16); return ~0u << t << t; }
__device__ __forceinline__ u32 range_mask32(int lo, int hi) { return mask_top32(hi) & ~mask_top32(lo); }
__device__ __forceinline__ u32 funnel32(u32 a, u32 b, int r) { return (u32)(((((u64)a) << 32) | b) >> (32 - r)); }   // r in [0,31]
// 32 bits at bit position p of a big-endian dword string whose dword 0 sits at D[0]; p >= -32 when D[-1] is the zero pad
// One v_alignbit_b32 ({hi,lo} >> s, s in [0,31]): with q = (p-1)>>5 and s = (-p)&31 the aligned case (p%32 == 0) reads
// the wanted dword as `lo` with s = 0, every other case is the usual funnel.  (D[q] is touched but unused when aligned.)
__device__ __forceinline__ u32 get32(const u32* D, int p) { const int q = (p - 1) >> 5; return __builtin_amdgcn_alignbit(D[q], D[q + 1], (u32)(-p) & 31u); }
// The masked overlap compares use get32(X, max(p, -32)): wherever the mask of a dword is non-zero its window starts at p >= -32 (the
// overlap region maps to non-negative positions of this read and a dword reaches at most 16 bases in front of it), and it ends
// inside the padded string (2*(16*9 + L1 - h) + 32 <= 32*(D+2)); fully masked dwords may read anything.
// same with bounds: anything outside [0, 32*n) reads as zero, p may be any negative number (slow, rare paths only)
__device__ __forceinline__ u32 get32z(const u32* D, int n, int p) {
    const int pp = p < 0 ? 0 : p, sh = pp - p, q = pp >> 5;
    const int q0 = q < n ? q : n - 1, q1 = q + 1 < n ? q + 1 : n - 1;
    u32 a = D[q0], b = D[q1]; a = q < n ? a : 0u; b = q + 1 < n ? b : 0u;
    const u32 v = funnel32(a, b, pp & 31);
    return sh >= 32 ? 0u : (v >> sh);
}
// ---- DPP wave primitives (gfx9 row_shr / row_bcast)
template <int CTRL, int ROWMASK>
__device__ __forceinline__ u32 dpp_mov(u32 old, u32 v) { return (u32)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROWMASK, 0xF, false); }
__device__ __forceinline__ u32 wave_incl_scan_dpp(u32 v) {
    v += dpp_mov<0x111, 0xF>(0, v); v += dpp_mov<0x112, 0xF>(0, v); v += dpp_mov<0x114, 0xF>(0, v); v += dpp_mov<0x118, 0xF>(0, v);
    v += dpp_mov<0x142, 0xA>(0, v); v += dpp_mov<0x143, 0xC>(0, v);
    return v;
}
__device__ __forceinline__ u32 wave_incl_max_dpp(u32 v) {          // inclusive running maximum over the lanes (values >= 0: the fill value 0 is neutral)
    v = max(v, dpp_mov<0x111, 0xF>(0, v)); v = max(v, dpp_mov<0x112, 0xF>(0, v)); v = max(v, dpp_mov<0x114, 0xF>(0, v)); v = max(v, dpp_mov<0x118, 0xF>(0, v));
    v = max(v, dpp_mov<0x142, 0xA>(0, v)); v = max(v, dpp_mov<0x143, 0xC>(0, v));
    return v;
}
__device__ __forceinline__ u32 half_incl_max_dpp(u32 v) {          // the same over each half of the wave (lanes 0-31, 32-63) by itself: no step across the halves
    v = max(v, dpp_mov<0x111, 0xF>(0, v)); v = max(v, dpp_mov<0x112, 0xF>(0, v)); v = max(v, dpp_mov<0x114, 0xF>(0, v)); v = max(v, dpp_mov<0x118, 0xF>(0, v));
    v = max(v, dpp_mov<0x142, 0xA>(0, v));
    return v;
}
// two unsigned 16-bit minima in one register (v_pk_min_u16): the right and the left selection key of the sequential-groups form (one read length: a key is window and slot)
__device__ __forceinline__ u32 pk_min_u16(u32 a, u32 b) {
    typedef unsigned short us2_ __attribute__((ext_vector_type(2)));
    const us2_ r = __builtin_elementwise_min(__builtin_bit_cast(us2_, a), __builtin_bit_cast(us2_, b)); return __builtin_bit_cast(u32, r);
}
__device__ __forceinline__ u32 wave_pk_min_dpp(u32 v) {              // both halves reduced over the wave; result broadcast from lane 63
    v = pk_min_u16(v, dpp_mov<0x111, 0xF>(~0u, v)); v = pk_min_u16(v, dpp_mov<0x112, 0xF>(~0u, v)); v = pk_min_u16(v, dpp_mov<0x114, 0xF>(~0u, v)); v = pk_min_u16(v, dpp_mov<0x118, 0xF>(~0u, v));
    v = pk_min_u16(v, dpp_mov<0x142, 0xA>(~0u, v)); v = pk_min_u16(v, dpp_mov<0x143, 0xC>(~0u, v));
    return (u32)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ u32 wave_min_dpp(u32 v) {                 // result valid in lane 63, returned broadcast
    v = min(v, dpp_mov<0x111, 0xF>(~0u, v)); v = min(v, dpp_mov<0x112, 0xF>(~0u, v)); v = min(v, dpp_mov<0x114, 0xF>(~0u, v)); v = min(v, dpp_mov<0x118, 0xF>(~0u, v));
    v = min(v, dpp_mov<0x142, 0xA>(~0u, v)); v = min(v, dpp_mov<0x143, 0xC>(~0u, v));
    return (u32)__builtin_amdgcn_readlane((int)v, 63);
}

// OR of all differences between Y[0..L2) and E at base offset d (>= 0).  cl / tailMask describe L2: dword cl is the
// partial one, tailMask its valid bits.  UNIFORM: they are the same for the whole wave (all reads have one length) and are
// moved to scalar registers, so that the per-dword mask is a scalar select and a dword costs alignbit + xor + and-or.
template <int NW, bool UNIFORM>
__device__ __forceinline__ u32 any_mismatch(const u32 (&Y)[NW], const u32* E, int d, int cl, u32 tailMask) {
    const int q = (2 * d - 1) >> 5; const u32 sh = (u32)(-2 * d) & 31u;       // see get32
    if (UNIFORM) { cl = __builtin_amdgcn_readfirstlane(cl); tailMask = (u32)__builtin_amdgcn_readfirstlane((int)tailMask); }
    u32 acc = 0, nxt = E[q + NW];
#pragma unroll
    for (int c = NW - 1; c >= 0; c--) {
        const u32 cur = E[q + c];
        const u32 diff = Y[c] ^ __builtin_amdgcn_alignbit(cur, nxt, sh);
        if (UNIFORM) { const u32 mk = (c < cl) ? ~0u : (c == cl ? tailMask : 0u); acc |= diff & mk; }
        else acc |= (c < cl) ? diff : (c == cl ? (diff & tailMask) : 0u);
        nxt = cur;
    }
    return acc;
}

constexpr int FAST_WPB = 4;    // waves per block of k_probe_fast (round 3: blocks of four waves, five blocks per CU; eight: +3.5 % at the same occupancy)
// Kernel arguments of the RARE paths (containment marks, the list of reads handed to the other kernels) are read from the kernel-argument segment where they are used
// instead of living in scalar registers for the whole kernel: the kernel holds ~50 dwords of arguments and spills ~40 SGPRs to VGPR lanes (v_writelane / v_readlane
// on the hot path).  The asm makes the pointer opaque, so the scalar loads cannot be hoisted out of the rare branch.  (Round 2 did this to the per-read result
// pointers too: +7 %, their loads wait in line with the LDS traffic -- those stay in registers.)
typedef const __attribute__((address_space(4))) ProbeArgs* ColdArgs;
__device__ __forceinline__ ColdArgs cold_args() { ColdArgs p = (ColdArgs)__builtin_amdgcn_kernarg_segment_ptr(); asm volatile("" : "+s"(p)); return p; }
#define COLD(A, f) (cold_args()->f)
// HITS = 1: the same look-up and gather machinery emits the directional hit lists of the status-0 reads for the reduce phase
// (economyGraph.cpp:591-633) instead of extension records: every candidate is compared directly with this read.
constexpr u32 HITS_CHUNK = 2048;   // hit slots a wave reserves at a time (one atomic per ~30 reads instead of one per read)
// TAIL = 2: like 1, and every read goes through the state machine (no speculation first: the general algorithm, exact for every read).
// TAIL = 1: the exact state machine for inconsistent reads is part of the kernel (its rows take 6.7 KB of LDS per wave at NW = 10 and its
// registers weigh on the whole kernel: -10 % on error-free data); TAIL = 0: such reads are put on the `slow` list instead.  The host picks per
// data set (dev_probe): clean data runs TAIL = 0 and sends the few listed reads through the TAIL = 1 kernel afterwards.
// UNI (clean-data form only): every read has the length A.uniL -- no per-candidate length registers.  QN: groups of 64 candidate slots a read may have (2: 128 candidates);
// SEQ: the groups are gathered and compared ONE AFTER THE OTHER into the same registers -- the reach of every candidate is known from its window and the common length before
// anything is fetched, the two speculated reads are fetched by lanes 0-2 straight into LDS -- so a read's candidates cost 10 dwords per lane however many groups there are
// (the wide form, QN = 4, for the reads of high-coverage data the 128-slot forms hand over: tests/diag/coverage_sweep.py).  UNI clean-data form only.
// (waves per SIMD the register allocator must leave room for: four for the 10-dword layouts = 128 VGPRs; the 16-dword layouts hold 32 more
// candidate dwords per lane and were spilling ~46 VGPRs and ~25 SGPRs at that budget -- slow, and the one place where a hit's overhang length came
// out of a reload wrong (found by the stress generator, 161-bp reads in repeats): they get two waves' worth of registers and spill nothing)
// Likewise three waves' worth for the instantiations that still spilled a few VGPRs at four (three windows per lane; the hit-list form).
constexpr int FAST_WAVES = 4;
// Round 3: SIX waves per SIMD for the form that carries neither the state machine nor the hit lists (TAIL = 0, HITS = 0: the clean-data kernel) with the 8- and
// 10-dword layouts.  After two rounds of instruction diet the kernel waited more than it issued (71 % VALU busy at four waves per SIMD, 123 VGPRs):
//   * the record scan keeps 3 instead of 8 records per window in flight (its 16 x u64 were the register peak): 95 VGPRs = five waves, 87.5 -> 76.7 ms per pass at configs[2];
//   * the lane number goes through an optimisation barrier once per read (see the read loop): the compiler had hoisted some twenty lane-derived expressions (LDS
//     addresses, half-wave indices, masks) out of the loop, each a register for the whole kernel -- 95 -> 79 VGPRs, SGPR spills 20 -> 3: six waves, 67.9 ms;
//   * shuffles as plain ds_bpermute (shfl64), the previous read's slot words in LDS instead of registers (psl): 77 VGPRs.
// Seven waves (72 VGPRs) still spill 3 registers in the compare loop: 72.5 ms with 5 spilled -- spills cost more than the occupancy returns.
constexpr int FAST_WAVES_CLEAN = 7, FAST_WAVES_SEQ = 8;
template <int S, int NW, int WPL, int WPB, int HITS, int TAIL, bool UNI = false, int QN = 2, bool SEQ = false>
__global__ __launch_bounds__(64 * WPB, (NW > 20 ? 1 : (NW > 10 ? 2 : (WPL >= 3 ? 3 : ((HITS == 0 && TAIL == 0) ? (SEQ ? (QN <= 2 ? FAST_WAVES_SEQ : 6) : ((NW <= 8 && UNI) ? 8 : FAST_WAVES_CLEAN)) : FAST_WAVES))))) void k_probe_fast(ProbeArgs A) {      // (32-dword candidates, two per lane: one wave's worth of registers per SIMD, or the kernel spills)
    // the in-kernel state machine for inconsistent reads needs 6.7 KB of LDS per wave at NW = 10; the long-read layouts keep their
    // occupancy instead and hand such reads to the sequential kernel
    constexpr bool TAILED = (HITS == 0) && (TAIL != 0);
    // (round 3: the per-read records are indexed by POSITION and name their neighbours by position -- the kernel translates nothing when it writes them; a read's own
    //  id is needed by the forms that write hits (HITS, TAIL = 2) and, otherwise, only when a containment is found: loaded there)
    constexpr bool NEED_IID = HITS != 0 || TAIL == 2;
    constexpr bool ALWAYS_TAIL = TAILED && TAIL == 2;  // noisy data: nearly every read ends in the state machine, the speculation in front of it is skipped
    constexpr int OVW = TailOvw<NW>::value;
    static_assert(QN == 2 || (HITS == 0 && TAIL == 0 && UNI), "more than two slot groups: clean-data uniform-length form only");
    static_assert(!SEQ || (HITS == 0 && TAIL == 0 && UNI), "sequential slot groups: clean-data uniform-length form only");
    constexpr int CAP = 64 * QN, NY = SEQ ? 1 : QN;      // candidate slots of a read; candidates a lane holds at a time
    constexpr bool RUN = SEQ;                            // run mode (see FastLds)
    constexpr bool SPEC = !ALWAYS_TAIL;                  // (speculation strings in LDS: see FastLds)
    __shared__ FastLds<S, NW, TAILED, WPL, CAP, RUN, SPEC> lds_all[WPB];
    FastLds<S, NW, TAILED, WPL, CAP, RUN, SPEC>& L = lds_all[threadIdx.x >> 6];
    const u32 lane = lane_id();
    const int k = A.k, h = A.h;
    constexpr int D = 2 * S;                       // dwords per read slot
    u32* const X0 = L.xf[0] + 1; u32* const X1 = L.xf[1] + 1;
    const u32* reads32 = (const u32*)A.reads;
    const int nk = (2 * h + 31) >> 5;              // key dwords
    const bool four = nk > 3;
    const u32 lastKeyMask = (2 * h) & 31 ? (~0u << (32 - ((2 * h) & 31))) : ~0u;
    const u32 Th = (u32)(A.T >> 1), seed32 = (u32)A.seed;      // T/2 slot pairs
    const u32 tagMask = g_tag_mask, mtagMask = g_mtag_mask;    // (device globals: read once, not per read)
    const uint4* pairs = (const uint4*)A.slots;

    // a block owns FAST_CHUNK consecutive positions of the (locality ordered) id list at a time, so reads that share
    // keys and neighbours run on one CU, back to back
    const u64 nItems = A.ids ? A.n_ids : (A.hi > A.lo ? A.hi - A.lo : 0);
    const u32 wib = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));     // wave-uniform: loop bookkeeping stays on the scalar unit
#ifdef SAGE2OV_STAMPS
    u64 st_acc[32]; for (int x_ = 0; x_ < 32; x_++) st_acc[x_] = 0;
    u64 st_prev = __builtin_amdgcn_s_memtime();
#endif
    if (lane == 0) { L.xf[0][0] = 0; L.xf[1][0] = 0; L.m[0][0] = 0; L.m[1][0] = 0; L.e[0][0] = 0; L.e[1][0] = 0; L.e[2][0] = 0; L.e[3][0] = 0; L.xp[0] = 0; L.rst[0] = 0;
                     if constexpr (RUN) { for (int x_ = 0; x_ < 4; x_++) L.rsx[RSX_CNT + x_] = 0; L.rsx[RSX_LMIN] = (int)A.runLanesMin; L.G[0] = 0; L.RCG[0] = 0; L.mrow[0] = 0; L.G[RUN_FD + 1] = 0; L.G[RUN_FD + 2] = 0; L.RCG[RUN_FD + 1] = 0; L.RCG[RUN_FD + 2] = 0; } }
    // (run mode needs gates that do not depend on the window -- k <= 64, so that every window of a read is a key of k bases --, one read length, and a frame that holds a run)
    // (evaluated where it is needed, out of the kernel-argument segment: as a value computed in front of the loop it is one more scalar register pair that lives across the
    //  whole loop -- the form spills ~65 scalars into the lanes of ONE spare vector register, and a 65th lane is a second register)
    auto runCapable = [&]() -> bool { if constexpr (!RUN) return false; else { const int uL = COLD(A, uniL), kk = COLD(A, k), hh = COLD(A, h);
        return uL != 0 && hh == kk && uL - kk <= RUN_OFF && uL <= 16 * NW && RUN_OFF + 2 * uL - kk <= RUN_F && uL - hh + 1 <= 128 && COLD(A, meta) != nullptr && COLD(A, noRun) == 0u; } };
    // Window reuse.  Consecutive positions of the locality order are reads with one minimiser on one strand, each starting a few bases after the one
    // before (build_locality_order).  If this read equals the wave's previous read shifted by d bases over their whole overlap (checked base by base),
    // its window j IS the previous read's window j + d: the slot word found then is the slot word now, and only the last d windows are looked up.
    bool prevValid = false; int prevOff = 0, prevStrand = 0, prevL1 = 0;
    u32* const Xp = L.xp + 1;
    // the wave's n-th item: chunk blockIdx.x + (n / PER) * gridDim.x, position wave * PER + n % PER of it (PER = positions of a visit / waves of the block).  Two-deep software pipeline:
    // the id of item n+2 and the bases of item n+1 are fetched while item n is processed (both chains off the critical path)
    static_assert(WPB == 2 || WPB == 4 || WPB == 8, "waves per block");
    const u32 chunkShift = (u32)__builtin_amdgcn_readfirstlane((int)A.chunkShift), perShift = chunkShift - (WPB == 2 ? 1u : (WPB == 4 ? 2u : 3u)), perMask = (1u << perShift) - 1u;     // (wave-uniform: scalar registers)
    // this block's phase of the grid (ProbeArgs::phase)
    u32 phFirst = 0, phBlocks = gridDim.x, phRounds = ~0u, phChunk0 = 0;
#pragma unroll
    for (int p_ = 0; p_ < 4; p_++) if (A.phase[p_][1] != 0 && blockIdx.x >= A.phase[p_][0]) { phFirst = A.phase[p_][0]; phBlocks = A.phase[p_][1]; phRounds = A.phase[p_][2]; phChunk0 = A.phase[p_][3]; }
    const u32 phBlock = blockIdx.x - phFirst;
    // The wave's items, one VISIT per round: visit g = chunk * (waves of the block) + wave covers items [vb(g), vb(g + 1)), consecutive positions (window reuse, run mode);
    // vb(g) is g * 2^perShift -- or, in the form with run mode (round 4), the first read of that nominal range that has ANOTHER minimiser hash than its predecessor (bit 9 of
    // its meta word, k_loc_index): the first read of a visit has no run to continue and takes the general path (111 look-ups, 62 gathers), so the boundary goes where a run
    // ends anyway.  The visits still tile the range (vb is monotone, vb(0) = 0), a visit has between 1 and 2^(perShift + 1) - 1 items.
    (void)perMask;
    u32 vRd = ~0u, vIt = 0, vEnd = 0; bool vDone = false;      // (items are below 2^30: 32-bit, and made scalar explicitly -- as 64-bit values of unproven uniformity they sat in vector register pairs)
    const bool alignVisits = RUN && A.ids == nullptr && perShift <= 6u && runCapable();
    auto vb = [&](u64 g, u32 ln) -> u32 {                      // (ln: the caller's lane number -- the read loop's is recomputed per read, see there; a lane number taken here would be hoisted)
        const u64 s0 = g << perShift;
        if (s0 >= nItems) return (u32)nItems;
        if (!alignVisits || g == 0) return (u32)s0;
        const bool in = ln < (1u << perShift) && s0 + ln < nItems;
        const u32 m = in ? (u32)A.meta[A.lo + s0 + ln] : 0xFFFFu;
        const u64 b = __ballot(in && m != 0xFFFFu && (m & 0x200u) != 0u);
        return (u32)s0 + (b ? (u32)__builtin_ctzll(b) : 0u);
    };
    auto advance = [&](u32 ln) -> u32 {                        // the wave's next item (a position of the locality order), 0 when there is none left
        if (vIt >= vEnd) {
            if (vDone) return 0u;
            vRd++;
            const u64 chunk = (u64)phChunk0 + phBlock + (u64)vRd * phBlocks, g = (chunk << (chunkShift - perShift)) + wib;
            if (vRd >= phRounds || (g << perShift) >= nItems) { vDone = true; return 0u; }
            vIt = (u32)__builtin_amdgcn_readfirstlane((int)vb(g, ln)); vEnd = (u32)__builtin_amdgcn_readfirstlane((int)vb(g + 1, ln));
        }
        const u64 it = vIt++;
        return A.ids ? A.ids[it] : (u32)(A.lo + it);
    };
    u64 hBase = 0; u32 hLeft = 0; u64 hTotal = 0;              // HITS (and TAIL = 2 with A.hitBase): this wave's current chunk of the hit buffer
    const u32 ldw = (lane < (u32)D ? lane : 0u) ^ 1u;
    u32 idCur = advance(lane), idNext = advance(lane);
    // (the form with run mode answers nine reads in ten without looking at their bases: it does not prefetch them -- the register the prefetch holds across the whole loop
    //  body is one the eight-wave form does not have -- and keeps the minimiser word of the next read in a scalar register)
    u32 wNext = RUN ? 0u : reads32[(u64)idCur * D + ldw];
    u32 metaNext = A.meta ? (u32)A.meta[idCur] : 0xFFFFu, iidNext = NEED_IID ? A.idOf[idCur] : 0u;       // (position 0: meta 0xFFFF, id 0)
    if constexpr (RUN) metaNext = (u32)__builtin_amdgcn_readfirstlane((int)metaNext);
    // the hits of one read (<= 2 per lane, in candidate-slot order) appended to the wave's chunk of the hit buffer: one atomic per chunk of 2048
    // slots; `base` = where the read's hits start (they are contiguous).  Over capacity: dropped, the host sees the cursor beyond the buffer.
    auto emit_hits = [&](const bool (&hit)[2], const int (&hlen)[2], const u32 (&htype)[2], const u32 (&ent)[2], u32 from, u64& base) -> u32 {   // (`to` is left as a POSITION: k_hits_filter translates)
        const u64 b0 = __ballot(hit[0]), b1 = __ballot(hit[1]);
        const u32 n0 = (u32)__popcll(b0), nh = n0 + (u32)__popcll(b1);
        base = 0;
        if (nh) {
            if (nh > hLeft) {                                               // next chunk; the rest of the old one is marked empty
                for (u32 x = lane; x < hLeft; x += 64) A.hits[hBase + x].from = 0;
                u64 nb_ = 0; if (lane == 0) nb_ = atomicAdd(&A.counters[CTR_HIT_CURSOR], (u64)HITS_CHUNK);
                hBase = ((u64)__builtin_amdgcn_readfirstlane((int)(nb_ >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)(u32)nb_);
                hLeft = hBase + HITS_CHUNK <= A.hits_cap ? HITS_CHUNK : 0u;
            }
            base = hBase;
            if (nh <= hLeft) {
                const u64 lt = (1ull << lane) - 1ull;
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    if (hit[q]) {
                        const u32 sq = q == 0 ? (u32)__popcll(b0 & lt) : n0 + (u32)__popcll(b1 & lt);
                        Hit hh; hh.from = from; hh.to = ent[q] >> 2; hh.len = hlen[q]; hh.type = htype[q] & 3u; hh.seq = sq;
                        A.hits[hBase + sq] = hh;
                    }
                }
                hBase += nh; hLeft -= nh;
            }
            hTotal += nh;
        }
        return nh;
    };
    for (;;) {
        // (the lane number behind an optimisation barrier, once per read: expressions derived from it -- LDS addresses, lane masks, half-wave indices: some twenty of them --
        //  are then recomputed where they are used instead of being hoisted out of the read loop, where each holds a vector register for the whole kernel)
        // (recomputed per read from an opaque zero: the two mbcnt are loop-invariant, and the compiler otherwise computes them once in front of the loop and keeps -- or
        //  spills -- the result: found in round 4 when the eight-wave form was 3 registers over its 64; every instantiation lost 3 registers)
        u32 lane; { u32 z_ = 0u; asm volatile("" : "+v"(z_)); lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z_)); }
        // (the wave's LDS block behind an optimisation barrier too, once per read: the address of every array of it that is indexed at run time -- e[][], the ring's tables --
        //  is otherwise computed in front of the loop and holds a vector register for the whole kernel; round 4, run mode: five of them were spilled)
        u32 wq_ = wib; asm volatile("" : "+s"(wq_));
        FastLds<S, NW, TAILED, WPL, CAP, RUN, SPEC>& L = lds_all[wq_];
        u32* const X0 = L.xf[0] + 1; u32* const X1 = L.xf[1] + 1; u32* const Xp = L.xp + 1;
        const u64 i = idCur; const u32 wCur = wNext;                // i: this read's POSITION in the locality-ordered store (its id: A.idOf[i])
        const u32 iid = iidNext, metaI = metaNext;
        idCur = idNext; idNext = advance(lane);
        // (the next read's bases: scalar base of its slot + this lane's dword -- the lane's offset is made here, not kept as a 64-bit vector address across the loop)
        if constexpr (!RUN) { const u32* np_ = reads32 + (u64)idCur * D; wNext = np_[(lane < (u32)D ? lane : 0u) ^ 1u]; }
        metaNext = A.meta ? (u32)A.meta[idCur] : 0xFFFFu; iidNext = NEED_IID ? A.idOf[idCur] : 0u;
        if constexpr (RUN) metaNext = (u32)__builtin_amdgcn_readfirstlane((int)metaNext);
        if (i == 0) break;                                          // (positions are 1-based: the wave has no item left)
        if (HITS) { if (A.statusP[i] != 0) continue; }
        STAMP(0);
        STAMP(20);                                                  // (diagnostic builds: the cost of a stamp itself)
        // ================================================================ RUN MODE: the next read of a run, off the frame and the slot ring (see FastLds)
        if constexpr (RUN) {
            if ((L.rst[0] & 2u) != 0u) {
                // a run was started by the previous read (general path): the frame is its strings laid end to end around it -- left overhang (XL1 = the mirror of XL0, from
                // gstart on) | read | right overhang (XR0, or the read itself when nothing overlapped its right end); RUN_OFF is a multiple of 16, so the right part is dword
                // aligned.  Both candidates of a dword are read and the VALUE is selected (a select between the rows' addresses would hold both in registers across the loop).
                const u32 fl = L.rst[0]; const int gstart = (int)L.rst[7], gend = (int)L.rst[4];
                const int g = (int)lane;
                if (g < RUN_FD) {
                    u32 v = 0;
                    if (16 * g >= RUN_OFF) { const int c_ = g - RUN_OFF / 16; const u32 a_ = L.e[0][1 + min(c_, 6 * S + 1)], b_ = L.xf[0][1 + min(c_, D + 1)];
                                             v = ((fl & 4u) ? a_ : b_) & mask_top32(gend - 16 * g); }
                    else if ((fl & 8u) && 16 * g + 16 > gstart) v = get32(L.e[3] + 1, 2 * max(16 * g - gstart, -16)) & ~mask_top32(gstart - 16 * g);
                    L.G[1 + g] = v;
                }
                wave_sync();
                if (g < RUN_FD) L.RCG[1 + g] = ~rev2_32(get32(L.G + 1, 2 * (RUN_F - 16 * g - 16))) & mask_top32(RUN_F - gstart - 16 * g) & ~mask_top32(RUN_F - gend - 16 * g);
                if (lane == 0) { L.rst[3] = (u32)RUN_OFF; L.rst[5] = 0u; L.rst[0] = 1u; }
                wave_sync();
            }
            if (L.rst[0] != 0u) {
                constexpr u32 RM = (u32)(CAP - 1);
                const int Lr = A.uniL, nwinR = Lr - h + 1;
                // The run's state lives in LDS (wave-uniform words; every piece of code below loads what it needs and stores what it changes -- as variables captured by the
                // lambdas they were ~25 scalar registers live across everything, and the form spills scalars into ONE vector register's lanes):
                //   rst[1] minimiser offset word of the current read, rst[2] its strand | mirrored << 1 (the frame has been mirrored: G lives in the RCG array and vice versa),
                //   rst[3] J0 = the read's frame position, rst[4] glen / rst[7] gstart = frame end / start, rst[5] base / rst[6] tot = ring start / size
                const int offR = (int)(metaI & 255u), strandR = (int)((metaI >> 8) & 1u);       // meta holds 255 - offset: a LATER start has a LARGER value
                bool ok = metaI != 0xFFFFu;
                // Same strand of the minimiser: the read starts d1 = (difference of the offsets) bases later.  OTHER strand: the reads of a minimiser's second strand follow those of
                // its first in the order, and the first of them covers the same stretch of genome as the last read of the first strand -- reverse complemented.  The bucket of a
                // reverse-complemented key holds the same reads with mirrored types (hashTable.cpp:96-104: prefix of the forward strand <-> suffix of the reverse complement), so
                // the ring of that stretch, MIRRORED, is the ring of the new read: no look-up, no compare.  The minimiser occupies frame positions [Mpos, Mpos + 16); the new read's
                // reverse complement then starts at a1: d1 > 0 = a forward step to there first, d2 > 0 = a forward step after the mirror (in the mirrored coordinates).
                int d1, d2 = 0; bool flipReq;
                { const int rOff = (int)L.rst[1], rStrand = (int)(L.rst[2] & 1u), J0 = (int)L.rst[3];
                  flipReq = strandR != rStrand; d1 = offR - rOff;
                  if (flipReq) { const int Mpos = J0 + (255 - rOff), a1 = Mpos + 16 + (255 - offR) - Lr, dl = a1 - J0; d1 = dl > 0 ? dl : 0; d2 = dl < 0 ? -dl : 0; ok = ok && d1 <= RUN_DMAX && d2 <= RUN_DMAX;
#ifdef SAGE2OV_STAMPS
                                 if (!ok && metaI != 0xFFFFu && lane == 0) st_acc[29] += 1;
#endif
                  }
                  else ok = ok && d1 >= 1 && d1 <= RUN_DMAX; }
                // is `key` (position * 4 + type) among the slots of the frame window `dq` windows behind the current read's first?  It is in the list, so that read has been
                // compared with the frame there.
                const u32 lane0r_ = lane;
                auto in_window = [&](int dq, u32 key) -> bool {
                    u32 lane = lane0r_; asm volatile("" : "+v"(lane));      // (opaque per call: what is derived from the lane number is computed here, not in front of the loop the call sits in)
                    const u32 pc = L.pcw[((int)L.rst[3] + dq) & (RUN_PW - 1)]; const u32 wf = pc & 255u, wc = pc >> 8;
                    const u32 e_ = L.pent[(wf + (lane < wc ? lane : 0u)) & RM];
                    return wc <= 64u && __any(lane < wc && e_ == key);
                };
                // ---- the ring moves on: the slots of the first dDrop windows leave, dr windows are (b) looked up with keys out of the frame, (c) their slots put behind the
                //      ring, (d) the frame grown, (e) the new slots compared with it.  0 = done, 1 = a slot does not equal the frame / the frame is full, 2 = no room in the ring or
                //      too many new slots (nothing has been touched: the caller may try a shorter step).  J0 stays (the caller moves it).
                auto step = [&](int dDrop, int dr) -> int {
                    u32 lane = lane0r_; asm volatile("" : "+v"(lane));      // (opaque per call: what is derived from the lane number is computed here, not in front of the loop the call sits in)
                    const int J0 = (int)L.rst[3]; int glen = (int)L.rst[4]; const u32 base = L.rst[5], tot = L.rst[6]; const int gstart = (int)L.rst[7]; const u32 flp = (L.rst[2] >> 1) & 1u;
                    const u32 dropped = ((L.pcw[(J0 + dDrop) & (RUN_PW - 1)] & 255u) - base) & RM;          // the slots of the windows in front leave the list
                    u32* const Gp = (flp ? L.RCG : L.G) + 1; u32* const Rp = (flp ? L.G : L.RCG) + 1;
                    // (b) lane w takes window J0 + nwin + w of the frame, key -> hash -> pair probes, as in 1c
                    // (lanes behind the step's windows fetch the table pairs of the windows the NEXT step is going to look up, as far as the frame has their keys: the same load
                    //  instruction, nobody waits for them -- the next step finds the lines in the L2)
                    const bool isW = lane < (u32)dr; const int Jw = J0 + nwinR + (int)lane;
                    const bool isPF = !isW && lane < (u32)dr + (u32)RUN_PF && Jw + h <= glen;
                    const int p = 2 * ((isW || isPF) ? Jw : RUN_OFF);
                    u32 k0 = get32(Gp, p), k1 = nk > 1 ? get32(Gp, p + 32) : 0u, k2 = nk > 2 ? get32(Gp, p + 64) : 0u, k3 = nk > 3 ? get32(Gp, p + 96) : 0u;
                    if (nk == 1) k0 &= lastKeyMask; else if (nk == 2) k1 &= lastKeyMask; else if (nk == 3) k2 &= lastKeyMask; else k3 &= lastKeyMask;
                    const u64 hv = hash4(k0, k1, k2, k3, seed32, four);
                    u32 px = (isW || isPF) ? __umulhi((u32)(hv >> 32), Th) : 0u; const u32 tgw = tag_of_m(hv, tagMask);
                    u64 slw = 0; bool pendw = isW;
                    for (;;) {
                        if (!__any(pendw)) break;
                        const uint4 pv = pairs[px];
                        if (pendw) {
                            const u64 s0 = ((u64)pv.y << 32) | pv.x, s1 = ((u64)pv.w << 32) | pv.z;
                            if (s0 == 0 || (pv.y >> (SLOT_TAG_SHIFT - 32)) == tgw) { slw = s0; pendw = false; }
                            else if (s1 == 0 || (pv.w >> (SLOT_TAG_SHIFT - 32)) == tgw) { slw = s1; pendw = false; }
                            else px = ix_next_pair(px);
                        }
                    }
                    STAMP(14);                                           // (diagnostic builds: 14 = a step's table look-ups, 15 = its slots and the frame, 22 = its compares)
                    const u32 c7 = (u32)(slw >> SLOT_CNT_SHIFT) & 127u;
                    const u32 cntw = (slw != 0 && c7 != SLOT_CNT_LONG) ? c7 : 0u, payw = (u32)(slw & SLOT_PAY_MASK);
                    // (c) window -> first slot by a scan, slot -> window by the running maximum of 1c's trick, entry from the slot word or csr[]
                    const u32 inc = wave_incl_scan_dpp(cntw); const u32 nNew = (u32)__builtin_amdgcn_readlane((int)inc, 63); const u32 cbw = inc - cntw;
                    const u32 tail = (base + tot) & RM;
                    if (nNew > RUN_NMAX || tot - dropped + nNew > (u32)CAP) return 2;
                    if (isW) L.pcw[Jw & (RUN_PW - 1)] = (unsigned short)(((tail + cbw) & RM) | (cntw << 8));
                    L.candJ[lane] = 0;
                    wave_sync();
                    if (isW && cntw) L.candJ[cbw] = lane + 1u;
                    wave_sync();
                    const u32 wsc = wave_incl_max_dpp(L.candJ[lane]); const u32 wl = wsc ? wsc - 1u : 0u;
                    const u32 cwv = (u32)shfl64((int)(cbw | (cntw << 8)), (int)wl), plv = (u32)shfl64((int)payw, (int)wl);
                    const bool isS = lane < nNew;
                    const u32 cn = (cwv >> 8) & 127u, eoff = lane - (cwv & 255u);
                    const u32 ce = A.csr[(isS && cn != 1u) ? plv + eoff : 0u];
                    const u32 en = cn == 1u ? plv : ce; const int Jx = J0 + nwinR + (int)wl;
                    if (isS) { L.pent[(tail + lane) & RM] = en; L.sJ[(tail + lane) & RM] = (unsigned short)Jx; }
                    wave_sync();
                    bool good = true;
                    if (nNew) {
                        // (the new slots' dwords for the first two passes of (e): issued now, in flight while the frame is extended)
                        constexpr u32 CP = 64u / (u32)NW;                      // candidates of a pass: NW lanes each (6 of 10 dwords, 8 of 8)
                        u32 yv[RUN_NPRE];
#pragma unroll
                        for (int p_ = 0; p_ < RUN_NPRE; p_++) {
                            yv[p_] = 0u;
                            if (CP * p_ >= nNew) continue;
                            const u32 xl = lane / (u32)NW; const u32 x = CP * p_ + xl, c = lane - xl * (u32)NW; const bool a0 = x < nNew && xl < CP;
                            const u32 e2 = L.pent[(tail + (a0 ? x : 0u)) & RM];
                            yv[p_] = reads32[(a0 ? (u64)(e2 >> 2) : 0ull) * D + ((a0 ? c : 0u) ^ 1u)];
                        }
                        // (d) the frame grows by the new right-hand neighbour that reaches furthest (the last right-type slot: windows ascend): from the frame's end on its bases
                        //     ARE the frame from now on (its bases in front of that are compared in (e) like any other new slot's); an entry of type 2 is taken in reverse complement
                        const u64 rb = __ballot(isS && (en & 1u) == 0u);
                        if (rb) {
                            const int xM = 63 - (int)__builtin_clzll(rb);
                            const int JM = __builtin_amdgcn_readlane(Jx, xM); const u32 eM = (u32)__builtin_amdgcn_readlane((int)en, xM);
                            const int reach = JM + Lr;
                            if (reach > glen) {
                                if (reach > RUN_F) good = false;
                                else {
                                    u32* Mr = L.mrow + 1;
                                    u32 y = lane < (u32)NW ? reads32[(u64)(eM >> 2) * D + (lane ^ 1u)] : 0u;
                                    if (NW == D && lane == (u32)(NW - 1)) y &= ~SLOT_LEN_MASK;
                                    if (lane < (u32)(NW + 3)) Mr[lane] = y;
                                    wave_sync();
                                    if ((eM & 3u) == 2u) {
                                        const int rem = Lr - 16 * (int)lane;
                                        const u32 rcv = (lane < (u32)NW && rem > 0) ? (~rev2_32(get32(Mr, 2 * (rem - 16))) & mask_top32(rem)) : 0u;
                                        wave_sync();
                                        if (lane < (u32)(NW + 3)) Mr[lane] = rcv;
                                        wave_sync();
                                    }
                                    // frame dwords [glen / 16, (reach - 1) / 16]: the old bases below glen stay, the read's bases from there to its end come in
                                    const int g = (int)lane;
                                    if (g < RUN_FD && 16 * g + 16 > glen && 16 * g < reach) {
                                        const u32 keep = mask_top32(glen - 16 * g), lim = mask_top32(reach - 16 * g);
                                        Gp[g] = (Gp[g] & keep) | (get32(Mr, 2 * (16 * g - JM)) & ~keep & lim);
                                    }
                                    wave_sync();
                                    // ... and the mirror image: position p of the other strand's array is the complement of position RUN_F - 1 - p
                                    if (g < RUN_FD && RUN_F - 16 * g > glen && RUN_F - 16 * g - 16 < reach)
                                        Rp[g] = ~rev2_32(get32(Gp, 2 * (RUN_F - 16 * g - 16))) & mask_top32(RUN_F - gstart - 16 * g) & ~mask_top32(RUN_F - reach - 16 * g);
                                    wave_sync();
                                    glen = reach;
                                }
                            }
                        }
                        // (e) every new slot against the frame over its whole length, dword-parallel: lanes NW x .. NW x + NW - 1 take slot x of a pass (64 / NW slots a pass), one dword each.  Type 0 / 1: the
                        //     read as stored against the frame at its start; type 2 / 3: against the other strand's array.  (An entry of the current read itself is compared like any
                        //     other: a look-up by tag can return the bucket of another key of the same tag, and an own entry in a foreign window must not enter the list.)
                        STAMP(15);
                        const int clU = Lr >> 4; const u32 tailU = mask_top32(Lr & 15);
                        for (u32 p_ = 0; good && CP * p_ < nNew; p_++) {
                            const u32 xl = lane / (u32)NW; const u32 x = CP * p_ + xl, c = lane - xl * (u32)NW; const bool act = x < nNew && xl < CP;
                            const u32 ph = (tail + (act ? x : 0u)) & RM; const u32 e2 = L.pent[ph]; const int J2 = (int)L.sJ[ph]; const int t2 = (int)(e2 & 3u);
                            const int st_ = (t2 & 1) == 0 ? J2 : J2 + h - Lr;                              // where the candidate starts in the frame
                            const bool fw = t2 < 2; const bool inside = st_ >= gstart && st_ + Lr <= glen;
                            const int pos = inside ? (fw ? st_ : RUN_F - (st_ + Lr)) : 0;
                            u32 y;
                            if (p_ < (u32)RUN_NPRE) { y = yv[0];
#pragma unroll
                                                  for (int z = 1; z < RUN_NPRE; z++) if (p_ == (u32)z) y = yv[z]; }
                            else y = reads32[(act ? (u64)(e2 >> 2) : 0ull) * D + ((act ? c : 0u) ^ 1u)];
                            if (NW == D && c == (u32)(NW - 1)) y &= ~SLOT_LEN_MASK;
                            const u32* row = fw ? Gp : Rp;
                            const int q_ = (2 * pos - 1) >> 5; const u32 sh = (u32)(-2 * pos) & 31u;
                            const u32 diff = y ^ __builtin_amdgcn_alignbit(row[q_ + (int)c], row[q_ + (int)c + 1], sh);
                            const u32 mk = (int)c < clU ? ~0u : ((int)c == clU ? tailU : 0u);
                            if (__any(act && (!inside || (diff & mk) != 0u))) good = false;
                        }
                    }
                    if (lane == 0) { L.rst[4] = (u32)glen; L.rst[5] = (base + dropped) & RM; L.rst[6] = tot - dropped + nNew; }
                    wave_sync();
                    return good ? 0 : 1;
                };
                // ---- (f) a read's records off the ring: its slots are those of the windows [Jk, Jk + nwin) (a step for several reads leaves the windows of the others in the ring
                //      too), all of them verified neighbours or the read itself: right = the first right-type slot, left = the first slot of the last window with a left-type slot
                //      (the tie rules of the general path: first / last window, then bucket order), connections = the others' count
                // (the slots are read out of LDS once for all the reads of a step; both sides' selection keys go through ONE wave reduction: right key = slot number in ring order,
                //  left key = (last window first) << 8 | slot number, 16 bits each)
                // A LANE PER READ (the 128-slot form, planned steps of lanesMin reads and more): the ring is in window order and a window's slots are contiguous, so the slots of
                // read r are ONE range [sa, sb) of ring-relative slot numbers -- from the first slot of its first window to the end of its last, both out of pcw[], which has a word
                // for every window of the ring, empty ones included.  Once per step the wave reads the ring in that order and ballots which slots are right-type (128 wave-uniform
                // bits; the others are left-type), and every slot that is an entry of one of the step's reads ORs its bit into that read's 128-bit word in candJ[] (free here: 16
                // reads x 4 dwords; own entries may sit in any window -- a look-up by tag --, not only the first and the last).  Lane r then has valid = range & ~own and reads its
                // records off it: connections = its population, right = its lowest right-type bit, left = the lowest left-type bit inside the window of the highest one ("last
                // window with a left-type slot, then bucket order").  Three coalesced stores per step.  Returns whether this form answered.
                auto records = [&](u32 pos0, u32 mReads, bool planned) -> bool {      // (planned: the reads start at the cumulative shifts of the step's plan; else: one read at the current position)
                    u32 lane = lane0r_; asm volatile("" : "+v"(lane));      // (opaque per call: what is derived from the lane number is computed here, not in front of the loop the call sits in)
                    const int J0r = (int)L.rst[3]; const u32 base = L.rst[5], tot = L.rst[6];
                    if constexpr (QN == 2) {
                        const u32 lm_ = (u32)L.rsx[RSX_LMIN];
                        if (planned && lm_ != 0u && mReads >= lm_) {
                            u32 e3[2]; u64 rt[2];
                            L.candJ[lane] = 0;
#pragma unroll
                            for (int q = 0; q < 2; q++) { const u32 sx = lane + 64u * q; e3[q] = L.pent[(base + sx) & RM]; rt[q] = __ballot(sx < tot && (e3[q] & 1u) == 0u); }
                            wave_sync();
#pragma unroll
                            for (int q = 0; q < 2; q++) { const u32 r_ = (e3[q] >> 2) - pos0; if (lane + 64u * q < tot && r_ < mReads) atomicOr(&L.candJ[4u * r_ + 2u * q + (lane >> 5)], 1u << (lane & 31u)); }
                            wave_sync();
                            const bool act = lane < mReads; const u32 r = act ? lane : 0u;
                            const int Jk = J0r + L.rsx[r], Jl = Jk + nwinR - 1;
                            const u32 pcA = L.pcw[Jk & (RUN_PW - 1)], pcB = L.pcw[Jl & (RUN_PW - 1)];
                            u32 sa = ((pcA & 255u) - base) & RM, sb = ((pcB & 255u) - base) & RM;
                            // (a full ring: the first slot of an empty window behind all CAP slots reads as 0.  Told apart by the window of the ring's first slot.)
                            const bool ambA = tot == (u32)CAP && sa == 0u && (pcA >> 8) == 0u, ambB = tot == (u32)CAP && sb == 0u && (pcB >> 8) == 0u;
                            if (__any(ambA || ambB)) { const int Jf = (int)L.sJ[base & RM]; if (ambA && Jf < Jk) sa = (u32)CAP; if (ambB && Jf < Jl) sb = (u32)CAP; }
                            sb += pcB >> 8;
                            auto below = [](u32 x) -> u64 { return x >= 64u ? ~0ull : ((1ull << x) - 1ull); };      // the bits under x
                            const u64 o0 = (u64)L.candJ[4u * r] | ((u64)L.candJ[4u * r + 1u] << 32), o1 = (u64)L.candJ[4u * r + 2u] | ((u64)L.candJ[4u * r + 3u] << 32);
                            const u64 v0 = act ? (below(sb) & ~below(sa) & ~o0) : 0ull, v1 = act ? (below(sb > 64u ? sb - 64u : 0u) & ~below(sa > 64u ? sa - 64u : 0u) & ~o1) : 0ull;
                            const u32 nconn = (u32)__popcll(v0) + (u32)__popcll(v1);
                            const u64 r0 = v0 & rt[0], r1 = v1 & rt[1], l0 = v0 & ~rt[0], l1 = v1 & ~rt[1];
                            const bool hasR = (r0 | r1) != 0ull, hasL = (l0 | l1) != 0ull;
                            const u32 keyR = r0 ? (u32)__builtin_ctzll(r0) : (r1 ? 64u + (u32)__builtin_ctzll(r1) : 0u);
                            const u32 hiL = l1 ? 127u - (u32)__builtin_clzll(l1) : (l0 ? 63u - (u32)__builtin_clzll(l0) : 0u);
                            const u32 pcH = L.pcw[(u32)L.sJ[(base + hiL) & RM] & (u32)(RUN_PW - 1)]; const u32 ha = ((pcH & 255u) - base) & RM;      // (that window holds a slot: no full-ring case)
                            const u64 m0 = l0 & ~below(ha), m1 = l1 & ~below(ha > 64u ? ha - 64u : 0u);
                            const u32 keyL = m0 ? (u32)__builtin_ctzll(m0) : (m1 ? 64u + (u32)__builtin_ctzll(m1) : 0u);
                            u64 rv = 0, lv = 0;
                            { const u32 ph = (base + keyR) & RM, e = L.pent[ph]; const int j3 = (int)L.sJ[ph] - Jk;
                              if (hasR) rv = (u64)(e >> 2) | ((u64)((e & 3u) == 2u ? 1 : 0) << 40) | ((u64)((u32)j3 & 0x3FFFFFu) << 42); }
                            { const u32 ph = (base + keyL) & RM, e = L.pent[ph]; const int j3 = (int)L.sJ[ph] - Jk;
                              if (hasL) lv = (u64)(e >> 2) | ((u64)((e & 3u) == 3u ? 1 : 0) << 40) | ((u64)((u32)(Lr - j3 - h) & 0x3FFFFFu) << 42); }
                            if (act) { A.right[pos0 + lane] = rv; A.left[pos0 + lane] = lv; A.conn[pos0 + lane] = nconn; }
                            return true;
                        }
                    }
                    u32 e3[QN], sx[QN]; int sj[QN];
#pragma unroll
                    for (int q = 0; q < QN; q++) {
                        const u32 ph = lane + 64u * q; sx[q] = (ph - base) & RM;
                        e3[q] = L.pent[ph]; sj[q] = sx[q] < tot ? (int)L.sJ[ph] : -0x10000;      // (a slot outside the ring is in no read's windows)
                    }
#pragma unroll 1
                    for (u32 k2 = 0; k2 < mReads; k2++) {
                        const u32 pos = pos0 + k2; const int Jk = J0r + (planned ? L.rsx[k2] : 0);
                        u32 key = ~0u, nconn = 0;
#pragma unroll
                        for (int q = 0; q < QN; q++) {
                            const int j3 = sj[q] - Jk;
                            const bool g3 = (u32)j3 < (u32)nwinR && (e3[q] >> 2) != pos;
                            nconn += (u32)__popcll(__ballot(g3));
                            const u32 kq = (e3[q] & 1u) == 0u ? (0xFFFF0000u | sx[q]) : ((((u32)(0x7F - j3) << 8) | sx[q]) << 16 | 0xFFFFu);
                            key = pk_min_u16(key, g3 ? kq : ~0u);
                        }
                        key = wave_pk_min_dpp(key);
                        if (lane == 0) {
                            const u32 keyR = key & 0xFFFFu, keyL = key >> 16;
                            u64 rv = 0, lv = 0;
                            if (keyR != 0xFFFFu) { const u32 ph = (base + keyR) & RM, e = L.pent[ph]; const int j3 = (int)L.sJ[ph] - Jk;
                                                   rv = (u64)(e >> 2) | ((u64)((e & 3u) == 2u ? 1 : 0) << 40) | ((u64)((u32)j3 & 0x3FFFFFu) << 42); }
                            if (keyL != 0xFFFFu) { const u32 ph = (base + (keyL & 255u)) & RM, e = L.pent[ph]; const int j3 = (int)L.sJ[ph] - Jk;
                                                   lv = (u64)(e >> 2) | ((u64)((e & 3u) == 3u ? 1 : 0) << 40) | ((u64)((u32)(Lr - j3 - h) & 0x3FFFFFu) << 42); }
                            A.right[pos] = rv; A.left[pos] = lv; A.conn[pos] = nconn;
                        }
                    }
                    return false;
                };
                // ---- the ring of the current stretch, mirrored: windows in reverse order (window J -> RUN_F - (J + h)), slots of a window in their order, types 0 <-> 3 and
                //      1 <-> 2; the two arrays of the frame change roles.  Not if a window holds one read twice (the mirrored bucket orders its two types the other way round).
                auto mirror = [&]() -> bool {
                    u32 lane = lane0r_; asm volatile("" : "+v"(lane));      // (opaque per call: what is derived from the lane number is computed here, not in front of the loop the call sits in)
                    const int J0 = (int)L.rst[3], glen = (int)L.rst[4], gstart = (int)L.rst[7]; const u32 base = L.rst[5], tot = L.rst[6], st2 = L.rst[2];
                    u32 me[QN], mj[QN], ns[QN]; bool dup = false;
#pragma unroll
                    for (int q = 0; q < QN; q++) {
                        const u32 ph = lane + 64u * q, sx = (ph - base) & RM; const bool v = sx < tot;
                        const u32 e = L.pent[ph]; const int J = (int)L.sJ[ph];
                        const u32 pc = L.pcw[J & (RUN_PW - 1)]; const u32 wfl = ((pc & 255u) - base) & RM, c = pc >> 8;
                        ns[q] = v ? (tot - (wfl + c)) + (sx - wfl) : ~0u;
                        const u32 en_ = L.pent[(ph + 1u) & RM]; const int Jn = (int)L.sJ[(ph + 1u) & RM];
                        dup |= v && sx + 1u < tot && Jn == J && (en_ >> 2) == (e >> 2);
                        me[q] = (e & ~3u) | (3u - (e & 3u)); mj[q] = (u32)(RUN_F - (J + h));
                    }
                    u32 wn_[2], wj_[2]; bool wv_[2];
#pragma unroll
                    for (int q = 0; q < 2; q++) {
                        const int wi = 64 * q + (int)lane; wv_[q] = wi < nwinR; const int J = J0 + (wv_[q] ? wi : 0);
                        const u32 pc = L.pcw[J & (RUN_PW - 1)]; const u32 wfl = ((pc & 255u) - base) & RM, c = pc >> 8;
                        wn_[q] = ((tot - (wfl + c)) & 255u) | (c << 8); wj_[q] = (u32)(RUN_F - (J + h));
                    }
                    if (__any(dup)) return false;
                    wave_sync();
#pragma unroll
                    for (int q = 0; q < QN; q++) if (ns[q] != ~0u) { L.pent[ns[q]] = me[q]; L.sJ[ns[q]] = (unsigned short)mj[q]; }
#pragma unroll
                    for (int q = 0; q < 2; q++) if (wv_[q]) L.pcw[wj_[q] & (u32)(RUN_PW - 1)] = (unsigned short)wn_[q];
                    if (lane == 0) { L.rst[5] = 0u; L.rst[2] = st2 ^ 2u; L.rst[7] = (u32)(RUN_F - glen); L.rst[4] = (u32)(RUN_F - gstart); L.rst[3] = (u32)(RUN_F - (J0 + Lr)); }
                    wave_sync();
                    return true;
                };
                // SEVERAL READS PER STEP (same strand): the reads behind this one in the wave's visit (consecutive positions) continue the run as long as they have the same
                // minimiser on the same strand and start later; their new windows are looked up, appended and compared in ONE step (one hash / probe pass, one scan, one frame
                // extension, the compare passes shared), then each reads its own records off the ring.  Up to RUN_MMAX reads, RUN_DMAX windows.  The plan -- cumulative shifts
                // rsx[0..RUN_MMAX), offset words behind them -- lives in LDS too.
                u32 m = 1;
                // (0: the plan, the own-entry checks and the records loop over the reads of a step, SAGE2OV_RUN_LANES=0; else they take a lane per read: see RUN_LANES_MIN)
                static_assert(RUN_MMAX <= 16, "a lane per read of a step: one DPP row in the plan, 16 x 4 dwords of own-slot masks in candJ[]");
                // (the wide form, QN = 4, keeps the loops: it sits at its register budget and sees the few reads the 128-slot form lists)
                const u32 lanesMin = QN == 2 ? (u32)__builtin_amdgcn_readfirstlane(L.rsx[RSX_LMIN]) : 0u;
                if (lane == 0) { L.rsx[0] = d1; L.rsx[RUN_MMAX] = offR; }
                if (ok && !flipReq && A.ids == nullptr) {
                    const bool a1 = idCur == (u32)i + 1u, a2 = a1 && idNext == (u32)i + 2u, a3 = a2 && vIt < vEnd && (u32)(A.lo + vIt) == (u32)i + 3u;
                    const u32 avail = min(RUN_MMAX - 1u, a3 ? 2u + (vEnd - vIt) : (a2 ? 2u : (a1 ? 1u : 0u)));      // (the reads behind this one that are consecutive items of the visit)
                    const u32 mk_ = avail ? (u32)A.meta[(u64)i + 1u + (lane < avail ? lane : 0u)] : 0xFFFFu;
                    const int rStrand = (int)(L.rst[2] & 1u);
                    if (lanesMin != 0u) {
                        // (a lane per candidate read: the running sum of the shifts telescopes to d1 + (its offset - this read's), the predecessor's offset comes from the
                        //  lane below -- avail < 16: one DPP row -- and the plan ends in front of the first lane that fails a test; offsets ascend strictly up to there,
                        //  so the sum is monotone and "first lane beyond RUN_DMAX" is where the loop below stops)
                        const int o_ = (int)(mk_ & 255u), oPrev = (int)dpp_mov<0x111, 0xF>((u32)offR, (u32)o_), DPk = d1 + (o_ - offR);
                        const bool bad = lane >= avail || mk_ == 0xFFFFu || (mk_ & 0x200u) != 0u || (int)((mk_ >> 8) & 1u) != rStrand || o_ - oPrev < 1 || DPk > RUN_DMAX;
                        m = 1u + (u32)__builtin_ctzll(__ballot(bad));          // (avail < RUN_MMAX <= 64: some lane is bad)
                        if (lane + 1u < m) { L.rsx[lane + 1u] = DPk; L.rsx[RUN_MMAX + 1u + lane] = o_; }
                    } else {
                    int oP = offR, DP = d1;
                    for (u32 k2 = 0; k2 < avail; k2++) {
                        const u32 mw = (u32)__builtin_amdgcn_readlane((int)mk_, (int)k2);      // (k2 is wave-uniform: a scalar-indexed readlane)
                        const int o_ = (int)(mw & 255u), dk = o_ - oP;
                        if (mw == 0xFFFFu || (mw & 0x200u) != 0u || (int)((mw >> 8) & 1u) != rStrand || dk < 1 || DP + dk > RUN_DMAX) break;
                        oP = o_; DP += dk; m = k2 + 2u;
                        if (lane == 0) { L.rsx[k2 + 1] = DP; L.rsx[RUN_MMAX + 1u + k2] = oP; }
                    }
                    }
                }
                wave_sync();
                // every read of the step must be in the list where it should start: (position * 4 + type 0) among the slots of its window; the read of the other strand: its
                // reverse-complement prefix entry (type 2) at the start of the stretch it covers (when that lies in front of the ring, d2 > 0, its entry is looked for after the mirror)
                if (ok && !flipReq && lanesMin != 0u) {
                    // (a lane per read of the plan: it walks the slots of its start window -- as many rounds as the largest of these windows has slots, typically 1 to 3 --
                    //  and the step keeps the reads in front of the first one that did not find itself.  The ring as it stands holds every start window: rsx <= RUN_DMAX < nwin.)
                    const bool act = lane < m;
                    const u32 pc = L.pcw[((int)L.rst[3] + L.rsx[act ? lane : 0u]) & (RUN_PW - 1)]; const u32 wf = pc & 255u, wc = pc >> 8, key = ((u32)i + lane) << 2;
                    bool pend = act && wc != 0u && wc <= 64u, found = false;
                    for (u32 s = 0; __any(pend); s++) { const u32 e_ = L.pent[(wf + s) & RM]; found = found || (pend && e_ == key); pend = pend && !found && s + 1u < wc; }
                    m = (u32)__builtin_ctzll(__ballot(!found)); ok = m >= 1u;          // (m <= RUN_MMAX <= 64 before: the lanes behind it found nothing)
                }
                else if (ok && !flipReq) { u32 mm = 0; for (; mm < m; mm++) if (!in_window(L.rsx[mm], ((u32)i + mm) << 2)) break; m = mm; ok = m >= 1u; }
                else if (ok && d2 == 0) { ok = in_window(d1, ((u32)i << 2) | 2u);
#ifdef SAGE2OV_STAMPS
                    if (!ok && lane == 0) st_acc[30] += 1;
#endif
                }
                // phase 0: the forward step (several reads; or, other strand, to the stretch the read covers); phase 1 (other strand only): the mirror, then a forward step in the
                // mirrored coordinates if the read starts behind the mirrored ring's first window
                STAMP(21);                                               // (diagnostic builds: 21 = the run's plan and own-entry checks, 22 = the step, 23 = the records)
                for (int ph = 0; ph < 2 && ok; ph++) {
                    if (ph == 1) { if (!flipReq) break; ok = mirror();
#ifdef SAGE2OV_STAMPS
                                   if (!ok && lane == 0) st_acc[31] += 1;
#endif
                                   if (ok && d2 > 0) { ok = in_window(d2, (u32)i << 2);
#ifdef SAGE2OV_STAMPS
                                       if (!ok && lane == 0) st_acc[30] += 1;
#endif
                                   }
                                   if (!ok || d2 == 0) break; }
                    const int dd = ph == 0 ? d1 : d2, dn = ph == 0 ? (flipReq ? d1 : L.rsx[m - 1u]) : d2;
                    if (dn == 0) continue;                                   // (other strand, the read covers exactly the current stretch: nothing to step)
                    const int rc_ = step(dd, dn);
                    if (rc_ == 2 && !flipReq && m > 1u) { m = 1; ph--; continue; }      // (no room for the windows of several reads: this read alone)
                    ok = rc_ == 0;
                    if (ok && flipReq) { if (lane == 0) L.rst[3] += (u32)dd; wave_sync(); }   // (a one-read step moves the current position; the step for several reads keeps it until the records are out)
                }
                STAMP(22);
                u32 nDone = 0; bool byLanes = false;
                if (ok && !flipReq) {
                    byLanes = records((u32)i, m, true);
                    wave_sync();
                    if (lane == 0) { const int J0n = (int)L.rst[3] + L.rsx[m - 1u]; const u32 base = L.rst[5]; const u32 drop2 = ((L.pcw[J0n & (RUN_PW - 1)] & 255u) - base) & RM;      // (the windows of the reads before the last one leave)
                                     L.rst[3] = (u32)J0n; L.rst[5] = (base + drop2) & RM; L.rst[6] -= drop2; L.rst[1] = (u32)L.rsx[RUN_MMAX - 1u + m]; }
                    nDone = m;
                } else if (ok) { records((u32)i, 1u, false); if (lane == 0) { L.rst[1] = (u32)offR; L.rst[2] = (L.rst[2] & 2u) | (u32)strandR; } nDone = 1; }
                STAMP(23);
#ifdef SAGE2OV_STAMPS
                if (flipReq && lane == 0) st_acc[ok ? 26 : 27] += 1;
#endif
                if (ok) {
#ifdef SAGE2OV_STAMPS
                    if (lane == 0) { st_acc[24] += nDone; st_acc[28] += 1; }
#endif
                    // (the wave's run counters, CTR_RUNSTATS: reads answered off the ring, steps; of them with a lane per read.  Four LDS words, one ds_add per step.)
                    if (lane < (byLanes ? 4u : 2u)) atomicAdd(&L.rsx[RSX_CNT + lane], (int)((lane & 1u) ? 1u : nDone));
                    // (the reads answered with this one are taken off the wave's items.  They are consecutive items of the visit -- a1, a2, a3 of the plan --: idCur and idNext
                    //  hold the first two, the others are skipped where they stand and the last two calls fetch what follows; the plan's `avail` keeps vIt <= vEnd)
                    if (nDone > 3u) vIt += nDone - 3u;
                    for (u32 k2 = 1; k2 < min(nDone, 3u); k2++) { idCur = idNext; idNext = advance(lane); }
                    if (nDone > 1u) { metaNext = A.meta ? (u32)A.meta[idCur] : 0xFFFFu; if constexpr (RUN) metaNext = (u32)__builtin_amdgcn_readfirstlane((int)metaNext); }
                    wave_sync();
                    continue;
                }
                if (lane == 0) L.rst[0] = 0;                             // the run ends here; the general path takes this read (and starts the next run if it can)
#ifdef SAGE2OV_STAMPS
                if (lane == 0) st_acc[25] += 1;
#endif
                wave_sync();
            }
            // (the run is off: its state words are free.  What a run started by THIS read needs of its minimiser information is put there now -- offset, strand; offset
            //  0xFFFF = none -- so that the word itself need not live in a register until the read's end)
            if (lane == 0) { L.rst[1] = metaI == 0xFFFFu ? 0xFFFFu : (metaI & 255u); L.rst[2] = (metaI >> 8) & 1u; }
        }
        // ---------------------------------------------------------------- stage the read (big-endian dwords) + its reverse complement
        wave_sync();
        if constexpr (RUN) { const u32* rp_ = reads32 + (u64)i * D; const u32 w_ = rp_[(lane < (u32)D ? lane : 0u) ^ 1u]; if (lane < D) X0[lane] = w_; }
        else
        if (lane < D) X0[lane] = wCur;
        else if (lane < D + 2) { u32 z_; asm volatile("v_mov_b32 %0, 0" : "=v"(z_)); X0[lane] = z_; X1[lane] = z_; }     // (a zero made here: the constant otherwise sits in a register for the whole kernel)
        wave_sync();
        const int L1 = (int)(X0[D - 1] & SLOT_LEN_MASK);
        if (lane == 0) X0[D - 1] &= ~SLOT_LEN_MASK;
        wave_sync();
        if (lane < D) { const int rem = L1 - 16 * (int)lane; X1[lane] = rem > 0 ? (~rev2_32(get32(X0, 2 * (rem - 16))) & mask_top32(rem)) : 0u; }
        wave_sync();
        const int nwin = L1 - h + 1;
        bool slowpath = nwin > 64 * WPL;
        // ---- window reuse: is this read the previous one shifted by d >= 0 bases?
        const int offI = (int)(metaI & 255u), strandI = (int)((metaI >> 8) & 1u);
        int dsh = 0; bool reuse = false;
        if (prevValid && metaI != 0xFFFFu && strandI == prevStrand && !slowpath) {
            dsh = offI - prevOff;                                   // meta holds 255 - offset: a LATER start has a LARGER value
            if (dsh >= 0 && dsh < prevL1 - h) {
                const int ov = min(L1, prevL1 - dsh);               // bases of this read that lie inside the previous one
                const bool dif = lane < (u32)D && ((X0[lane] ^ get32(Xp, min(2 * (16 * (int)lane + dsh), 32 * D))) & mask_top32(ov - 16 * (int)lane)) != 0;
                reuse = !__any(dif);
            }
        }
        const int prevNwin = prevL1 - h + 1;
#ifdef SAGE2OV_STAMPS
        if (lane == 0) { st_acc[10] += 1; st_acc[11] += reuse ? 1 : 0; st_acc[12] += reuse ? (u64)dsh : 0; st_acc[13] += (prevValid && metaI != 0xFFFFu && strandI == prevStrand) ? 1 : 0; }
#endif

        STAMP(1);
        CUT(1, (u32)L1 ^ X1[lane & 15u] ^ (u32)reuse ^ (u32)dsh);
        // ---------------------------------------------------------------- 1. lookups
        int jj[WPL]; u32 pidx[WPL], tg[WPL]; u64 sl[WPL]; bool pend[WPL]; bool needQ[WPL];
#pragma unroll
        for (int q = 0; q < WPL; q++) {
            jj[q] = 64 * q + (int)lane; pend[q] = jj[q] < nwin; sl[q] = 0;
            if (reuse) {                                            // slot word of window jj + d of the previous read (registers of lane (jj+d) & 63)
                const int ws = jj[q] + dsh; const bool ok = pend[q] && ws < prevNwin && ws < 64 * WPL;
                const u64 got = L.psl[ok ? ws : 0];
                if (ok) { sl[q] = got; pend[q] = false; }
            }
            needQ[q] = __any(pend[q]);                              // wave-uniform: a pass in which no lane has a window left is skipped
            pidx[q] = 0; tg[q] = 0;
            if (!needQ[q]) continue;
            const int p = 2 * (pend[q] ? jj[q] : 0);
            u32 k0 = get32(X0, p), k1 = nk > 1 ? get32(X0, p + 32) : 0u, k2 = nk > 2 ? get32(X0, p + 64) : 0u, k3 = nk > 3 ? get32(X0, p + 96) : 0u;
            if (nk == 1) k0 &= lastKeyMask; else if (nk == 2) k1 &= lastKeyMask; else if (nk == 3) k2 &= lastKeyMask; else k3 &= lastKeyMask;
            const u64 hv = hash4(k0, k1, k2, k3, seed32, four);
            pidx[q] = pend[q] ? __umulhi((u32)(hv >> 32), Th) : 0u; tg[q] = tag_of_m(hv, tagMask);      // (lanes without a window to look up read pair 0 / word 0 below: cached)
        }
        bool anyNeed = false;
#pragma unroll
        for (int q = 0; q < WPL; q++) anyNeed |= needQ[q];
        bool ambAny = false;
        STAMP(2);
        CUT(2, pidx[0] ^ tg[0] ^ (u32)sl[0] ^ pidx[WPL - 1] ^ tg[WPL - 1] ^ (u32)sl[WPL - 1] ^ (u32)anyNeed);
        // After a reuse only the last few windows are left: they go straight to the uniform table (1c: one 16-byte load per window) -- the
        // minimiser path (w-mer hashes, sliding minimum, group word, record scan: three dependent steps, all 64 lanes busy for a handful
        // of windows) pays off when MANY windows share few groups, i.e. for the reads that start a run.
        const bool directFew = reuse && (nwin - max(prevNwin - dsh, 0)) <= DIRECT_MAX;
        if (A.TL && anyNeed && !directFew) {                          // (TL != 0 iff the minimiser index exists; its two tables are arguments of this block only: COLD)
            const u64* const mi1_ = COLD(A, mi1); const u64* const krec_ = COLD(A, krec);
            // 1a. minimiser of every window: hash all w-mers once (position 64c+lane in register c), then a sliding minimum of
            //     width m = h-w+1 by doubling across lanes (ds_bpermute; no LDS storage, no barriers)
            u32 winMin[WPL];
            const int w = h < 16 ? h : 16, m = h - w + 1, npos = L1 - w + 1;
            // after a reuse only the last few windows are left: their w-mers fit ONE register (positions base .. base+63), the sliding minimum
            // runs on that register alone and a shuffle hands window j the value of lane j - base
            const int baseW = reuse ? max(prevNwin - dsh, 0) : 0;
            if (reuse && (nwin - baseW) + m - 1 <= 64) {
                const int p0 = baseW + (int)lane;
                u32 a = p0 < npos ? wmer_hash(get32(X0, 2 * p0) >> (32 - 2 * w)) : ~0u;
                int width = 1;
                for (; 2 * width <= m; width *= 2) a = min(a, (u32)shfl64((int)a, (int)((lane + (u32)width) & 63u)));   // lanes that wrap are not windows of interest
                if (m > width) a = min(a, (u32)shfl64((int)a, (int)((lane + (u32)(m - width)) & 63u)));
#pragma unroll
                for (int q = 0; q < WPL; q++) winMin[q] = (u32)shfl64((int)a, (jj[q] - baseW) & 63);
            } else
            {
                constexpr int NC = (16 * NW - 15 + 63) / 64;                      // 64-position chunks that can hold a w-mer start
                u32 a[NC];
#pragma unroll
                for (int c = 0; c < NC; c++) { const int p0 = 64 * c + (int)lane; a[c] = p0 < npos ? wmer_hash(get32(X0, 2 * p0) >> (32 - 2 * w)) : ~0u; }
                int width = 1;
                for (; 2 * width <= m; width *= 2) {                              // a[c][l] = min over positions [p, p + 2*width)
                    const u32 src = (lane + (u32)width) & 63u; const bool wrap = lane + (u32)width >= 64u;
                    u32 t[NC];
#pragma unroll
                    for (int c = 0; c < NC; c++) t[c] = (u32)shfl64((int)a[c], (int)src);
#pragma unroll
                    for (int c = 0; c < NC; c++) a[c] = min(a[c], wrap ? (c + 1 < NC ? t[c + 1] : ~0u) : t[c]);
                }
                if (m > width) {                                                  // [p, p+m) = [p, p+width) U [p+m-width, p+m)
                    const u32 sh = (u32)(m - width), src = (lane + sh) & 63u; const bool wrap = lane + sh >= 64u;
                    u32 t[NC];
#pragma unroll
                    for (int c = 0; c < NC; c++) t[c] = (u32)shfl64((int)a[c], (int)src);
#pragma unroll
                    for (int q = 0; q < WPL; q++) winMin[q] = q < NC ? min(a[q < NC ? q : 0], wrap ? (q + 1 < NC ? t[q + 1 < NC ? q + 1 : 0] : ~0u) : t[q < NC ? q : 0]) : ~0u;   // (windows past the last chunk do not exist)
                } else {
#pragma unroll
                    for (int q = 0; q < WPL; q++) winMin[q] = q < NC ? a[q < NC ? q : 0] : ~0u;
                }
            }
            STAMP(3);
            CUT(3, winMin[0] ^ winMin[WPL - 1] ^ pidx[0] ^ tg[0] ^ (u32)sl[0] ^ pidx[WPL - 1] ^ tg[WPL - 1] ^ (u32)sl[WPL - 1]);
            // 1b. group of the minimiser (lanes that share a minimiser read the same words), then a scan of the group
            u32 goff[WPL], gn[WPL]; const u32 TL32 = (u32)A.TL;
            {
                u32 gi[WPL], mt[WPL]; bool gp[WPL];
#pragma unroll
                for (int q = 0; q < WPL; q++) {
                    gi[q] = 0; mt[q] = 0; gp[q] = false; goff[q] = 0; gn[q] = 0;
                    if (!needQ[q]) continue;
                    const u32 mh = minim_hash(winMin[q], seed32); gi[q] = pend[q] ? __umulhi(mh, TL32) : 0u; mt[q] = minim_tag_m(mh, mtagMask); gp[q] = pend[q];
                }
                for (;;) {
                    bool any = false;
#pragma unroll
                    for (int q = 0; q < WPL; q++) any |= gp[q];
                    if (!__any(any)) break;
                    u64 gv[WPL];
#pragma unroll
                    for (int q = 0; q < WPL; q++) gv[q] = needQ[q] ? mi1_[gi[q]] : 0ull;
#pragma unroll
                    for (int q = 0; q < WPL; q++) {
                        if (!needQ[q]) continue;
                        if (gp[q]) {
                            if (gv[q] == 0) { gp[q] = false; pend[q] = false; }                              // no key has this minimiser: a miss
                            else if ((u32)(gv[q] >> SLOT_TAG_SHIFT) == mt[q]) { gp[q] = false; gn[q] = (u32)(gv[q] >> 32) & 255u; goff[q] = (u32)gv[q]; }
                            else gi[q] = ix_next_group(gi[q]);
                        }
                    }
                }
            }
            STAMP(4);
            CUT(4, goff[0] ^ gn[0] ^ goff[WPL - 1] ^ gn[WPL - 1] ^ tg[0] ^ (u32)sl[0] ^ tg[WPL - 1] ^ (u32)sl[WPL - 1] ^ pidx[0] ^ pidx[WPL - 1]);
            u32 nmax = 0;
#pragma unroll
            for (int q = 0; q < WPL; q++) { if (gn[q] == MI_BIG) gn[q] = 0; else if (pend[q]) { pend[q] = false; nmax = max(nmax, gn[q]); } else gn[q] = 0; }
            // (lanes of an oversized / ambiguous group keep pend = true and fall through to the uniform table below)
            u32 wmax = nmax;
            wmax = max(wmax, dpp_mov<0x111, 0xF>(0, wmax)); wmax = max(wmax, dpp_mov<0x112, 0xF>(0, wmax)); wmax = max(wmax, dpp_mov<0x114, 0xF>(0, wmax)); wmax = max(wmax, dpp_mov<0x118, 0xF>(0, wmax));
            wmax = max(wmax, dpp_mov<0x142, 0xA>(0, wmax)); wmax = max(wmax, dpp_mov<0x143, 0xC>(0, wmax));
            wmax = (u32)__builtin_amdgcn_readlane((int)wmax, 63);
            // The scan reads whole records, SCAN_U per window in flight off one base pointer (immediate offsets, no address arithmetic; the
            // matching record is kept, so no dependent load follows).  It does not stop at the end of the group: a record
            // of a neighbouring group that happens to carry the tag (2^-24) only adds candidates that fail verification, like
            // any merged tag, or makes the window ambiguous (-> sequential kernel).  krec[] is padded by 16 records for this.
            u32 nmatch[WPL]; u64 mrec[WPL];
#pragma unroll
            for (int q = 0; q < WPL; q++) { nmatch[q] = 0; mrec[q] = 0; }
            {
                const u64* kp[WPL]; u32 tgs[WPL];
#pragma unroll
                for (int q = 0; q < WPL; q++) { kp[q] = krec_ + goff[q]; tgs[q] = tg[q] << (SLOT_TAG_SHIFT - 32); }
                for (u32 x = 0; x < wmax; x += SCAN_U) {
                    u64 r[WPL][SCAN_U];
#pragma unroll
                    for (int q = 0; q < WPL; q++)
                        if (needQ[q])
#pragma unroll
                            for (int u = 0; u < SCAN_U; u++) r[q][u] = kp[q][u];
#pragma unroll
                    for (int q = 0; q < WPL; q++) {
                        if (!needQ[q]) continue;
#pragma unroll
                        for (int u = 0; u < SCAN_U; u++) { const bool hit = ((u32)(r[q][u] >> 32) ^ tgs[q]) < (1u << (SLOT_TAG_SHIFT - 32)); mrec[q] = hit ? r[q][u] : mrec[q]; nmatch[q] += hit ? 1u : 0u; }
                        kp[q] += SCAN_U;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < WPL; q++) if (nmatch[q] && gn[q]) sl[q] = mrec[q];
            // two records of one group with the same tag (two keys, ~2^-24 per pair): the scan cannot tell them apart
            bool amb = false;
#pragma unroll
            for (int q = 0; q < WPL; q++) amb |= gn[q] != 0 && nmatch[q] > 1;
            if (__any(amb)) { slowpath = true; ambAny = true; }
        }
        // 1c. uniform table (everything when there is no minimiser index; otherwise only windows of oversized groups)
        for (;;) {
            bool any = false;
#pragma unroll
            for (int q = 0; q < WPL; q++) any |= pend[q];
            if (!__any(any)) break;
            uint4 pv[WPL];
#pragma unroll
            for (int q = 0; q < WPL; q++) pv[q] = pairs[pidx[q]];               // unconditional: idle lanes re-read their last pair
#pragma unroll
            for (int q = 0; q < WPL; q++) {
                if (pend[q]) {
                    const u64 s0 = ((u64)pv[q].y << 32) | pv[q].x, s1 = ((u64)pv[q].w << 32) | pv[q].z;
                    if (s0 == 0 || (pv[q].y >> (SLOT_TAG_SHIFT - 32)) == tg[q]) { sl[q] = s0; pend[q] = false; }
                    else if (s1 == 0 || (pv[q].w >> (SLOT_TAG_SHIFT - 32)) == tg[q]) { sl[q] = s1; pend[q] = false; }
                    else pidx[q] = ix_next_pair(pidx[q]);
                }
            }
        }
        // ---- remember this read's windows for the next read of the wave
        prevValid = metaI != 0xFFFFu && nwin <= 64 * WPL && !ambAny; prevOff = offI; prevStrand = strandI; prevL1 = L1;
#pragma unroll
        for (int q = 0; q < WPL; q++) L.psl[64 * q + (int)lane] = jj[q] < nwin ? sl[q] : 0ull;
        if (lane < (u32)(D + 2)) Xp[lane] = X0[lane];
        wave_sync();
        STAMP(5);
        CUT(5, (u32)sl[0] ^ (u32)(sl[0] >> 32) ^ (u32)sl[WPL - 1] ^ (u32)(sl[WPL - 1] >> 32) ^ (u32)slowpath);
        // ---------------------------------------------------------------- 2. candidates
        u32 cnt[WPL], pay[WPL], mine = 0;
#pragma unroll
        for (int q = 0; q < WPL; q++) {
            const u32 c7 = (u32)(sl[q] >> SLOT_CNT_SHIFT) & 127u;
            cnt[q] = (sl[q] != 0 && c7 != SLOT_CNT_LONG) ? c7 : 0u; pay[q] = (u32)(sl[q] & SLOT_PAY_MASK);
            // the read's own prefix / suffix entry (r2 == i never counts, economyGraph.cpp:95): no candidate slot for it -- except in the form with run mode, whose slot lists
            // are handed from read to read (the next read of the run needs this read's suffix entry as a slot; the gate below keeps it out of this read's count)
            if (!RUN && c7 == 1u && (pay[q] >> 2) == (u32)i) cnt[q] = 0;
            mine += cnt[q];
        }
        // candidate slots in window order (j ascending, bucket order inside a window = the order the reference visits them):
        // window q of lane l is j = 64q + l, so all q = 0 windows come first; two 16-bit prefix sums ride in one DPP scan
        u32 cbase[WPL]; u32 total = 0;
#pragma unroll
        for (int q0 = 0; q0 < WPL; q0 += 2) {
            const u32 pk = cnt[q0] | ((q0 + 1 < WPL ? cnt[q0 + 1 < WPL ? q0 + 1 : q0] : 0u) << 16);
            const u32 inc = wave_incl_scan_dpp(pk);
            const u32 tot = (u32)__builtin_amdgcn_readlane((int)inc, 63);
            cbase[q0] = total + (inc & 0xFFFFu) - cnt[q0]; total += tot & 0xFFFFu;
            if (q0 + 1 < WPL) { cbase[q0 + 1 < WPL ? q0 + 1 : q0] = total + (inc >> 16) - cnt[q0 + 1 < WPL ? q0 + 1 : q0]; total += tot >> 16; }
        }
        (void)mine;
        const bool capOver = total > (u32)CAP;                   // more candidates than this form has slots (wave-uniform): counted apart, the host may pick the wide form for the rest
        if (capOver) slowpath = true;
        u32 nhits = 0; u32 selR = ~0u, selL = ~0u;
        u32 myEnt[QN]; int myJ[QN], myL2[QN];
#pragma unroll
        for (int q = 0; q < QN; q++) { myEnt[q] = 0; myJ[q] = 0; myL2[q] = 0; }
        // (lane `ol_` of the registers of slot group `oq_`, both wave-uniform: every group's lane is read and the choice is made among scalars -- a select among the
        //  registers themselves is turned into an indexed access by the compiler, which puts the arrays into scratch memory)
        auto pick_lane = [&](const auto (&arr)[QN], u32 oq_, int ol_) -> int { int r_ = __builtin_amdgcn_readlane((int)arr[0], ol_);
#pragma unroll
            for (int q = 1; q < QN; q++) { const int x_ = __builtin_amdgcn_readlane((int)arr[q], ol_); r_ = oq_ == (u32)q ? x_ : r_; }
            return r_; };
        // (UNI: a candidate's length is the common length -- only gated candidates' lengths are ever looked at -- and the array is never written)
        auto L2of = [&](int q) -> int { if constexpr (UNI) return A.uniL; else return myL2[q]; };
        if (!slowpath) {
            // Candidate slot -> window, without a loop over bucket sizes (a wave ran as many rounds as its largest bucket): every window with
            // entries marks its FIRST slot with its number + 1, a running maximum over the slots gives every slot its window (slots are in
            // window order), the window's (first slot, count, payload) come from its lane's registers by shuffle.
#pragma unroll
            for (int q = 0; q < QN; q++) L.candJ[lane + 64 * q] = 0;
            wave_sync();
            u32 cwin[WPL];                               // per window: first slot | count << 8 | payload bit 32 << 15
#pragma unroll
            for (int q = 0; q < WPL; q++) { cwin[q] = cbase[q] | (cnt[q] << 8) | ((u32)((sl[q] >> 32) & 1u) << 15); if (cnt[q]) L.candJ[cbase[q]] = (u32)jj[q] + 1u; }
            if constexpr (RUN) {      // (the ring's window table, should this read start a run: the run is off while the general path works, so the tables are free)
                if (runCapable()) {
#pragma unroll
                    for (int q = 0; q < WPL; q++) if (jj[q] < nwin && 64 * q < 128) L.pcw[(RUN_OFF + jj[q]) & (RUN_PW - 1)] = (unsigned short)((cbase[q] & 255u) | (cnt[q] << 8));
                }
            }
            wave_sync();
            // ---- gather: entry (CSR for multi-entry buckets), then the 64-byte read slot, two candidates per lane
            u32 Y[NY][NW]; bool gate[QN];
            const bool two = total > 64u;                // the second slot of every lane is empty otherwise: skip its work (wave-uniform)
#pragma unroll
            for (int q = 1; q < QN; q++) gate[q] = false;
#pragma unroll
            for (int q = 1; q < NY; q++)
#pragma unroll
                for (int c = 0; c < NW; c++) Y[q][c] = 0;
            u32 carryW = 0;
#pragma unroll
            for (int q = 0; q < QN; q++) {
                if (q >= 1 && total <= 64u * q) continue;
                const u32 ci = lane + 64 * q; const bool have = ci < total;
                const u32 wsc = max(wave_incl_max_dpp(L.candJ[ci]), carryW);          // window number + 1 of slot ci
                carryW = (u32)__builtin_amdgcn_readlane((int)wsc, 63);
                const u32 wn = wsc ? wsc - 1u : 0u;
                u32 cw = 0, pl = 0;
#pragma unroll
                for (int sq = 0; sq < WPL; sq++) {
                    const u32 a_ = (u32)shfl64((int)cwin[sq], (int)(wn & 63u)), b_ = (u32)shfl64((int)pay[sq], (int)(wn & 63u));
                    if ((int)(wn >> 6) == sq) { cw = a_; pl = b_; }
                }
                const u32 cn = (cw >> 8) & 127u, eoff = ci - (cw & 255u);
                const bool isCsr = cn != 1u;
                const u32 src = isCsr ? pl + eoff : pl;   // (CSR offsets and inline entries fit 32 bits: fewer than 2^30 reads, tuple positions below 2^32)
                const u32 ce = A.csr[(have && isCsr) ? src : 0u];
                myEnt[q] = isCsr ? ce : src; myJ[q] = (int)wn;
                const u32 r2 = myEnt[q] >> 2; const int t = myEnt[q] & 3;
                gate[q] = have && (r2 != (u32)i) && ((t == 0 || t == 2) ? (myJ[q] <= L1 - k) : (myJ[q] >= k - h));
                if (HITS) { const uint8_t st2 = A.statusP[gate[q] ? r2 : 0u]; gate[q] = gate[q] && st2 == 0; }     // economyGraph.cpp:605 (statusP[0] is never 0)
#ifdef SAGE2OV_TRAFFIC_PROBE      // diagnostic build: no candidate read is fetched (results are meaningless; the PMC traffic of the rest is what is measured)
                gate[q] = false;
#endif
            }
            u32 ngate = 0;                                       // gated slots (run mode starts only where every one of them verified)
            if constexpr (RUN) {
                if (runCapable()) {
#pragma unroll
                    for (int q = 0; q < QN; q++) {
                        if (q >= 1 && total <= 64u * q) continue;
                        ngate += (u32)__popcll(__ballot(gate[q]));
                        if (lane + 64u * q < total) { L.pent[lane + 64 * q] = myEnt[q]; L.sJ[lane + 64 * q] = (unsigned short)(RUN_OFF + myJ[q]); }
                    }
                }
            }
            STAMP(16);
            CUT(16, myEnt[0] ^ myEnt[1] ^ (u32)myJ[0] ^ (u32)myJ[1] ^ (u32)gate[0] ^ ((u32)gate[1] << 1));
            // 16-byte loads of the (at least 32-byte aligned) slot; gated-off lanes read slot 0 (zeros, always cached)
            auto gather = [&](int q, u32 (&Yd)[NW]) {
                const uint4* yp = (const uint4*)(A.reads + (gate[q] ? (u64)(myEnt[q] >> 2) : 0ull) * S);
#pragma unroll
                for (int c = 0; c < (NW + 3) / 4; c++) {
                    const uint4 v = yp[c];                       // memory dwords 4c..4c+3 = (lo,hi) of words 2c, 2c+1
                    if (4 * c + 0 < NW) Yd[4 * c + 0] = v.y;
                    if (4 * c + 1 < NW) Yd[4 * c + 1] = v.x;
                    if (4 * c + 2 < NW) Yd[4 * c + 2] = v.w;
                    if (4 * c + 3 < NW) Yd[4 * c + 3] = v.z;
                }
                // one load instruction over 64 different lines costs the L1 64 cycles whatever its width (tools/ubench/vmem_rate.hip):
                // the length gather is skipped when all reads have one length
                if constexpr (!UNI) {
                    if (A.uniL) myL2[q] = gate[q] ? A.uniL : 0;
                    else myL2[q] = (int)(((const u32*)yp)[2 * S - 2] & SLOT_LEN_MASK);     // low dword of the last word
                }
                if (NW == D) Yd[NW - 1] &= ~SLOT_LEN_MASK;
            };
            if constexpr (HITS == 0 && !SEQ) {                   // both candidates of a lane in flight together (the hit-list form fetches them one after
#pragma unroll                                                   // the other into the same registers: 128 VGPRs are its budget for four waves per SIMD)
                for (int q = 0; q < QN; q++) { if (q >= 1 && total <= 64u * q) continue; gather(q, Y[q]); }
            }
            // (the first group is in flight while the reach is found and the strings are built)
            if constexpr (SEQ) gather(0, Y[0]);
            STAMP(6);
            CUT(6, Y[0][0] ^ Y[0][NW - 1] ^ Y[1][0] ^ Y[1][NW - 1] ^ Y[0][NW / 2] ^ Y[1][NW / 2] ^ (u32)L2of(0) ^ (u32)L2of(1) ^ myEnt[0] ^ myEnt[1]);
            if constexpr (HITS != 0) {
                // ---------------------------------------------------------------- hit lists: direct masked compare of the overlap region
                bool hit[2] = {false, false}; int hlen[2] = {0, 0}; u32 htype[2] = {0, 0};
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    if (q == 1 && !two) continue;
                    gather(q, Y[0]);
                    if (gate[q]) {
                        const int t = myEnt[q] & 3, j = myJ[q], L2 = L2of(q);
                        const bool rightSide = (t == 0 || t == 2);
                        const int span = rightSide ? (L1 - j) : (j + h);
                        const int n = L2 <= span ? L2 : span;
                        const int off = L1 - j - h;
                        const u32* X = (t == 0 || t == 1) ? X0 : X1;
                        int dd, lo, hi;
                        if (t == 0) { dd = j; lo = 0; hi = n; } else if (t == 3) { dd = off; lo = 0; hi = n; }
                        else if (t == 2) { dd = L1 - j - L2; lo = L2 - n; hi = L2; } else { dd = j + h - L2; lo = L2 - n; hi = L2; }
                        u32 diff = 0;
#pragma unroll
                        for (int c = 0; c < NW; c++) diff |= (Y[0][c] ^ get32(X, min(max(2 * (16 * c + dd), -32), 32 * D))) & range_mask32(lo - 16 * c, hi - 16 * c);
                        hit[q] = diff == 0;                                         // :607-626 (contained-and-equal counts here)
                        hlen[q] = rightSide ? (L2 - (L1 - j)) : (L2 - j - h);
                        htype[q] = t == 0 ? 3u : (t == 1 ? 0u : (t == 2 ? 2u : 1u));
                    }
                }
                const u64 b0 = __ballot(hit[0]), b1 = __ballot(hit[1]);
                const u32 n0 = (u32)__popcll(b0), nh = n0 + (u32)__popcll(b1);
                if (nh) {
                    if (nh > hLeft) {                                               // next chunk; the rest of the old one is marked empty
                        for (u32 x = lane; x < hLeft; x += 64) A.hits[hBase + x].from = 0;
                        u64 nb_ = 0; if (lane == 0) nb_ = atomicAdd(&A.counters[CTR_HIT_CURSOR], (u64)HITS_CHUNK);
                        hBase = ((u64)__builtin_amdgcn_readfirstlane((int)(nb_ >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)(u32)nb_);
                        hLeft = hBase + HITS_CHUNK <= A.hits_cap ? HITS_CHUNK : 0u;     // over capacity: dropped, the host retries with a larger buffer
                    }
                    if (nh <= hLeft) {
                        const u64 lt = (1ull << lane) - 1ull;
#pragma unroll
                        for (int q = 0; q < 2; q++) {
                            if (hit[q]) {
                                const u32 sq = q == 0 ? (u32)__popcll(b0 & lt) : n0 + (u32)__popcll(b1 & lt);
                                Hit hh; hh.from = iid; hh.to = A.idOf[myEnt[q] >> 2]; hh.len = hlen[q]; hh.type = htype[q] & 3u; hh.seq = sq;
                                A.hits[hBase + sq] = hh;
                            }
                        }
                        hBase += nh; hLeft -= nh;
                    }
                    hTotal += nh;
                }
                if (lane == 0) A.hitcount[iid] = nh;
                continue;
            }
            bool tail = ALWAYS_TAIL;                // exact state machine over the verified hits, inside this kernel (see the tail below)
            if constexpr (!ALWAYS_TAIL) {
            // ---------------------------------------------------------------- 3. speculation: furthest reach per side
            u32 reachR = ~0u, reachL = ~0u; bool sameLen = true;
#pragma unroll
            for (int q = 0; q < QN; q++) {
                if (q >= 1 && total <= 64u * q) continue;
                if (gate[q]) {
                    const int t = myEnt[q] & 3; const u32 ci = lane + 64 * q;
                    if (t == 0 || t == 2) reachR = min(reachR, ((u32)(0x7FF - (myJ[q] + L2of(q))) << 8) | ci);
                    else reachL = min(reachL, ((u32)(0x7FF - (L1 - myJ[q] - h + L2of(q))) << 8) | ci);
                    sameLen &= (L2of(q) == L1);
                }
            }
            reachR = wave_min_dpp(reachR); reachL = wave_min_dpp(reachL);
            const bool uniformLen = UNI ? true : __all(sameLen);
            STAMP(17);
            CUT(17, reachR ^ reachL ^ (u32)uniformLen ^ Y[0][0] ^ Y[0][NW - 1] ^ Y[1][0] ^ Y[1][NW - 1]);
            // (t, j, L2) of the two speculated reads, broadcast with readlane (EXEC independent); they publish their bases
            u32 mEnt[2] = {0, 0}; int mJ[2] = {0, 0}, mL2[2] = {0, 0};
#pragma unroll
            for (int sd = 0; sd < 2; sd++) {
                const u32 rk = sd ? reachL : reachR;
                if (rk != ~0u) {
                    const int ol = (int)(rk & 63u); const u32 oqn = (rk >> 6) & 3u; const bool oq = oqn != 0; (void)oq;
                    mEnt[sd] = (u32)pick_lane(myEnt, oqn, ol);
                    mJ[sd] = pick_lane(myJ, oqn, ol);
                    mL2[sd] = UNI ? A.uniL : pick_lane(myL2, oqn, ol);
                    if constexpr (SEQ) {
                        // the speculated read straight from the store (its position is wave-uniform): lanes 0 .. 2 fetch 16 bytes each, lanes 0 .. 4 write the D + 2 dwords of M
                        u32* M = L.m[sd] + 1;
                        if (lane < (u32)((D + 2 + 3) / 4)) {
                            uint4 v = make_uint4(0u, 0u, 0u, 0u);
                            if (lane < (u32)((NW + 3) / 4)) v = ((const uint4*)(A.reads + (u64)(mEnt[sd] >> 2) * S))[lane];
                            u32 w4[4] = {v.y, v.x, v.w, v.z};
#pragma unroll
                            for (int k4 = 0; k4 < 4; k4++) {
                                const int c = 4 * (int)lane + k4;
                                u32 x = c < NW ? w4[k4] : 0u; if (NW == D && c == NW - 1) x &= ~SLOT_LEN_MASK;
                                if (c < D + 2) M[c] = x;
                            }
                        }
                    } else if constexpr (QN != 2) {
                        if ((int)lane == ol) {
                            u32* M = L.m[sd] + 1;
#pragma unroll
                            for (int qq = 0; qq < QN; qq++) if (oqn == (u32)qq) {
#pragma unroll
                                for (int c = 0; c < NW; c++) M[c] = Y[qq][c];
                            }
#pragma unroll
                            for (int c = NW; c < D + 2; c++) M[c] = 0;
                        }
                    } else
                    if ((int)lane == ol) {
                        u32* M = L.m[sd] + 1;
#pragma unroll
                        for (int c = 0; c < NW; c++) M[c] = (NW % 4 == 0) ? Y[0][c] : (oq ? Y[1][c] : Y[0][c]);
                        if constexpr (NW % 4 == 0) {                                    // (8- and 16-dword layouts: the compiler turns the wave-uniform select between the
                            if (oq) {                                                   //  two arrays into an indexed access, which puts Y into scratch memory -- two copies
#pragma unroll
                                for (int c = 0; c < NW; c++) M[c] = Y[1][c];            //  with constant indices instead; the 10-dword layout keeps the select: no room for more)
                            }
                        }
                        { u32 z_; asm volatile("v_mov_b32 %0, 0" : "=v"(z_));       // (a zero made here, see the staging of the read)
#pragma unroll
                          for (int c = NW; c < D + 2; c++) M[c] = z_; }
                    }
                }
            }
            STAMP(18);
            CUT(18, mEnt[0] ^ mEnt[1] ^ (u32)mJ[0] ^ (u32)mJ[1] ^ (u32)mL2[0] ^ (u32)mL2[1] ^ L.m[0][1 + (lane & 7u)] ^ Y[0][0] ^ Y[1][0]);
            const int posR = mJ[0], posL = L1 - mJ[1] - h;                                  // offsets in the side's own coordinates
            const int LR = reachR != ~0u ? posR + mL2[0] : 0, LL = reachL != ~0u ? posL + mL2[1] : 0;
            // a speculated read that ends inside this read (containment) or that does not reach its end is left to the sequential kernel
            if ((reachR != ~0u && LR <= L1) || (reachL != ~0u && LL <= L1)) tail = true;
            wave_sync();
            if (!tail) {
                // ---- extended strings: lanes 0-31 build the right side, lanes 32-63 the left side, one dword per lane and round (one round of 32 dwords = 512
                // bases covers read + overhang of the 4- and 8-word layouts; the 16-word layout, reads up to 504 bases, takes two)
                {
                    constexpr int ROW = 6 * S + 2;                                          // dwords of a row (with the 4-word layout a round would run past it)
                    constexpr int ROUNDS = S > 8 ? 2 : 1;
                    const int side = lane >> 5, c0 = (int)(lane & 31);
                    const u32 rk = side ? reachL : reachR;
                    bool mbad = false;
                    if (rk != ~0u) {
                        const int t = (side ? mEnt[1] : mEnt[0]) & 3, L2M = side ? mL2[1] : mL2[0], posM = side ? posL : posR, tot = posM + L2M;
                        const bool straight = side ? (t == 3) : (t == 0);
                        const u32* own = side ? X1 : X0; const u32* oth = side ? X0 : X1; const u32* M = L.m[side] + 1;
                        u32* dstA = L.e[2 * side + (straight ? 0 : 1)] + 1; u32* dstB = L.e[2 * side + (straight ? 1 : 0)] + 1;
                        // straight: own[0,posM) ++ M ; mirrored: M ++ other strand [L1-posM, L1).  B is shifted right by sB >= 0 bases.
                        const u32* Aa = straight ? own : M; const int lenA = straight ? posM : L2M;
                        const u32* Bb = straight ? M : oth; const int sB = straight ? posM : (tot - L1);
#pragma unroll
                        for (int rd = 0; rd < ROUNDS; rd++) {
                            const int c = c0 + 32 * rd, cb = 16 * c;
                            const int pB = 2 * (cb - sB);                                   // bit position in B; >= -32 is readable (front pad)
                            const u32 va = c < D + 2 ? Aa[c < D + 2 ? c : 0] : 0u;          // (A is a read or a speculated read: D + 2 dwords, zero behind its bases)
                            const u32 vb = (pB > -32 && pB < 32 * (D + 1)) ? get32(Bb, pB) : 0u;
                            const u32 mA = mask_top32(lenA - cb);
                            if (c < ROW) dstA[c] = ((va & mA) | (vb & ~mA)) & mask_top32(tot - cb);
                        }
                        wave_sync();
#pragma unroll
                        for (int rd = 0; rd < ROUNDS; rd++) {
                            const int c = c0 + 32 * rd, rem = tot - 16 * c;
                            if (c < ROW) dstB[c] = rem > 0 ? (~rev2_32(get32(dstA, 2 * (rem - 16))) & mask_top32(rem)) : 0u;
                        }
                        wave_sync();
                        // the speculated read must really overlap: the straight string equals the own strand on [posM, L1)
                        const u32* Es = L.e[2 * side] + 1;
#pragma unroll
                        for (int rd = 0; rd < ROUNDS; rd++) { const int c = c0 + 32 * rd; if (c < D + 2) mbad |= ((Es[c] ^ own[c]) & range_mask32(posM - 16 * c, L1 - 16 * c)) != 0; }
                    } else { wave_sync(); wave_sync(); }
                    if (__any(mbad)) tail = true;
                }
                wave_sync();
            }
            STAMP(7);
            CUT(7, (u32)tail ^ L.e[lane & 3u][1 + (lane & 15u)] ^ Y[0][0] ^ Y[0][NW - 1] ^ Y[1][0] ^ Y[1][NW - 1] ^ (u32)uniformLen);
            if (!tail) {
                // ---------------------------------------------------------------- 4. one whole-length compare per candidate
                bool bad = false;
                const int clU = L1 >> 4; const u32 tailU = mask_top32(L1 & 15);
#pragma unroll
                for (int q = 0; q < QN; q++) {
                    if (q >= 1 && total <= 64u * q) continue;
                    if constexpr (SEQ) { if (q >= 1) gather(q, Y[0]); }      // (the next group into the same registers)
                    u32 (&Yq)[NW] = Y[SEQ ? 0 : q];
                    bool hit = false;
                    if (gate[q]) {
                        const int t = myEnt[q] & 3, j = myJ[q], L2 = L2of(q);
                        const bool rightSide = (t == 0 || t == 2);
                        const int span = rightSide ? (L1 - j) : (j + h);
                        const bool cont = L2 <= span; const int n = cont ? L2 : span;
                        const int off = L1 - j - h;
                        const u32* E = L.e[t == 0 ? 0 : (t == 2 ? 1 : (t == 3 ? 2 : 3))] + 1;
                        const int d = t == 0 ? j : (t == 2 ? LR - j - L2 : (t == 3 ? off : LL - off - L2));
                        const bool usable = !cont && d >= 0;
                        u32 acc = 1;
                        if (usable) { if constexpr (UNI) acc = any_mismatch<NW, true>(Yq, E, d, clU, tailU); else acc = uniformLen ? any_mismatch<NW, true>(Yq, E, d, clU, tailU) : any_mismatch<NW, false>(Yq, E, d, L2 >> 4, mask_top32(L2 & 15)); }
                        if (acc == 0) hit = true;                                                  // verified and consistent
                        else {
                            // rare: decide between "not an overlap" and "overlap, but inconsistent / contained"
                            const u32* X = (t == 0 || t == 1) ? X0 : X1;
                            int dd, lo, hi;
                            if (t == 0) { dd = j; lo = 0; hi = n; } else if (t == 3) { dd = off; lo = 0; hi = n; }
                            else if (t == 2) { dd = L1 - j - L2; lo = L2 - n; hi = L2; } else { dd = j + h - L2; lo = L2 - n; hi = L2; }
                            u32 diff = 0;
#pragma unroll
                            for (int c = 0; c < NW; c++) diff |= (Yq[c] ^ get32(X, min(max(2 * (16 * c + dd), -32), 32 * D))) & range_mask32(lo - 16 * c, hi - 16 * c);
                            if (diff == 0) {
                                if (cont) { const u32* io_ = COLD(A, idOf); const u32 id2 = io_[myEnt[q] >> 2], id1 = NEED_IID ? iid : io_[i]; atomicOr(&COLD(A, cflag)[myEnt[q] >> 2], id1 > id2 ? 1u : 2u); }   // economyGraph.cpp:735
                                else bad = true;                                                    // a true overlap that disagrees with the longest one
                            }
                        }
                    }
                    const u64 hb = __ballot(hit);
                    nhits += (u32)__popcll(hb);
                    if (hit) {
                        const int t = myEnt[q] & 3; const u32 ci = lane + 64 * q;
                        if constexpr (SEQ) {
                            // (one read length, at most 128 windows, at most 256 slots: a key is window:7 | slot:8 -- both sides' keys share one register, high half right,
                            //  low half left: one register and one wave reduction less in the form that has no register to spare)
                            const u32 kk_ = (t == 0 || t == 2) ? ((((u32)myJ[q] << 8) | ci) << 16) | 0xFFFFu : 0xFFFF0000u | ((u32)(0x7F - myJ[q]) << 8) | ci;
                            selR = pk_min_u16(selR, kk_);
                        } else {
                        if (t == 0 || t == 2) selR = min(selR, ((u32)myJ[q] << 18) | ((u32)(0x3FF - L2of(q)) << 8) | ci);
                        else selL = min(selL, ((u32)(0x1FF - myJ[q]) << 18) | ((u32)(0x3FF - L2of(q)) << 8) | ci);
                        }
                    }
                }
                if (__any(bad)) tail = true;
                if constexpr (RUN) {
                    // ---- a run starts here: the read took the consistent path and EVERY gated slot verified, i.e. equals the extended strings over its whole length.  The frame
                    // is those strings laid end to end around the read -- left overhang (XL1 = the mirror of XL0) | read | right overhang (XR0) --, the ring is this read's slot
                    // list (pent / sJ / pcw were written as the slots were resolved).  Not with an own entry of type 2 / 3 (a palindromic key: see the run-mode block).
                    bool start = runCapable() && !tail && L.rst[1] != 0xFFFFu && nhits == ngate && total >= 1u && RUN_OFF + max(LR, L1) <= RUN_F && (reachL == ~0u || LL - L1 <= RUN_OFF);
                    if (start) {
                        // (this read's own entries are the slots the general path never compares: they may only be its prefix entry in window 0 and its suffix entry in the last
                        //  window -- where the read IS the frame.  A look-up by tag can return another key's bucket, e.g. the read's own prefix bucket for a window that has no
                        //  key of its own (found at 50 M reads with the minimiser groups: 13 reads in 42.5 M); and a reverse-complement own entry is a palindromic key)
                        bool pal = false;
#pragma unroll
                        for (int q = 0; q < QN; q++) { if (q >= 1 && total <= 64u * q) continue;
                            const u32 t_ = myEnt[q] & 3u;
                            pal |= (lane + 64u * q < total) && (myEnt[q] >> 2) == (u32)i && !((t_ == 0u && myJ[q] == 0) || (t_ == 1u && myJ[q] == nwin - 1)); }
                        start = !__any(pal);
                    }
                    if (start) {
                        // (the frame itself is laid out at the top of the next read, out of the rows this read leaves in LDS -- here the registers are full; rst[0] = 2 | has a
                        //  right string << 2 | has a left string << 3 asks for it)
                        const int gstart = reachL != ~0u ? RUN_OFF - (LL - L1) : RUN_OFF, gend = RUN_OFF + (reachR != ~0u ? LR : L1);
                        // (the constants of a fresh run -- frame position RUN_OFF, ring start 0 -- are written where the frame is built: as immediates of this block the compiler
                        //  keeps them in a register pair across the whole loop)
                        if (lane == 0) { L.rst[4] = (u32)gend; L.rst[6] = total; L.rst[7] = (u32)gstart;
                                         L.rst[0] = 2u | (reachR != ~0u ? 4u : 0u) | (reachL != ~0u ? 8u : 0u); }
                    }
                }
            }
            }   // !ALWAYS_TAIL
            STAMP(19);
            CUT(19, (u32)tail ^ nhits ^ selR ^ selL);
            if (tail && !TAILED) slowpath = true;
            if constexpr (TAILED) if (tail) {
                nhits = 0;
                // ------------------------------------------------------------ tail: some verified hit disagrees with the longest one (read errors,
                // repeats) or the speculation did not hold.  The reference's state machine (economyGraph.cpp:95-438) is then evaluated as it is
                // written, hit by hit in window / bucket order, but on data this wave already holds: every candidate is compared directly with
                // this read, the overhang of every hit goes to LDS, and one step of the machine is a dword-parallel prefix compare of two overhangs.
                bool thit[2] = {false, false}; bool tooLong = false; u32 nR = 0, nL = 0;
                int tov[2] = {0, 0}; u32 ttype[2] = {0, 0};                          // (TAIL = 2 with A.hitBase: the hits are also written out, see below)
                uint8_t* const tailSlot = L.tslotIdx;
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    if (q == 1 && !two) continue;
                    const u32 ci = lane + 64 * q;
                    u32* row = L.tslot[ci] + 1;
                    L.tslot[ci][0] = 0;
#pragma unroll
                    for (int c = 0; c < NW; c++) row[c] = Y[q][c];
                    u32 meta = 0; u32 ovd[OVW]; int ovq = 0, nq = 0;      // (ovq, nq: a hit's overhang and the bases of read 2 inside this read)
#pragma unroll
                    for (int c = 0; c < OVW; c++) ovd[c] = 0;
                    if (gate[q]) {
                        const int t = myEnt[q] & 3, j = myJ[q], L2 = L2of(q);
                        const bool rightSide = (t == 0 || t == 2);
                        const int span = rightSide ? (L1 - j) : (j + h);
                        const bool cont = L2 <= span; const int n = cont ? L2 : span;
                        const int off = L1 - j - h;
                        const u32* X = (t == 0 || t == 1) ? X0 : X1;
                        int dd, lo, hi;
                        if (t == 0) { dd = j; lo = 0; hi = n; } else if (t == 3) { dd = off; lo = 0; hi = n; }
                        else if (t == 2) { dd = L1 - j - L2; lo = L2 - n; hi = L2; } else { dd = j + h - L2; lo = L2 - n; hi = L2; }
                        u32 diff = 0;
#pragma unroll
                        for (int c = 0; c < NW; c++) diff |= (Y[q][c] ^ get32(X, min(max(2 * (16 * c + dd), -32), 32 * D))) & range_mask32(lo - 16 * c, hi - 16 * c);
                        if (diff == 0) {
                            if (cont) { const u32* io_ = COLD(A, idOf); const u32 id2 = io_[myEnt[q] >> 2], id1 = NEED_IID ? iid : io_[i]; atomicOr(&COLD(A, cflag)[myEnt[q] >> 2], id1 > id2 ? 1u : 2u); }   // economyGraph.cpp:735
                            else {
                                const int ov = L2 - n;                                                   // bases of read 2 beyond this read
                                thit[q] = true; tooLong |= ov > (OVW <= 16 ? (16 * OVW < 255 ? 16 * OVW : 255) : 16 * OVW);      // (the packed geometry keeps 10 bits of it; the 8- and 16-dword forms stop at 128 / 255 bases)
                                tov[q] = ov; ttype[q] = t == 0 ? 3u : (t == 1 ? 0u : (t == 2 ? 2u : 1u));
                                meta = 0x80000000u | (rightSide ? 0u : 1u) | ((u32)((t == 2 || t == 3) ? 1 : 0) << 1) | ((u32)L2 << 2) | ((u32)j << 11) | ((u32)(ov & 0x3FF) << 20);
                                ovq = ov; nq = n;
                            }
                        }
                    }
                    // The overhangs, cut out for the whole wave without control flow (round 4, end: written as `if (rm > 0) { if (tail) ... else if (rm >= 16) ... else ... }`
                    // per dword it compiled to four nested exec-mask regions per dword, each with an LDS read and a wait of its own -- 8 dwords x 2 passes of them).  The tail of
                    // read 2 from base n on (types 0, 3), or the reverse complement of its head (types 1, 2): 16 bases ending at base rm of the head -- for rm < 16 that window
                    // starts in the dword in front of the row, whose bases the reversal puts LAST, where the mask drops them.  A lane without a hit has ovq = 0: every mask empty.
                    if (__any(ovq > 0)) {
                        const u32 fwdM = 0u - ((0x9u >> (myEnt[q] & 3u)) & 1u);          // types 0 and 3, as a mask (a `||` of two compares came back as branches around every select)
#pragma unroll
                        for (int c = 0; c < OVW; c++) {
                            const int rm = ovq - 16 * c;
                            const u32 posA = (u32)(2 * min(nq + 16 * c, 16 * NW)), posB = (u32)(2 * (max(rm, 0) - 16));
                            const u32 v = get32(row, (int)((fwdM & posA) | (~fwdM & posB)));
                            ovd[c] = ((fwdM & v) | (~fwdM & ~rev2_32(v))) & mask_top32(rm);
                        }
                    }
                    // the overhang replaces the candidate's dwords in its own slot; geometry, read id and slot of the hits are compacted in
                    // visiting order (candidate slots are in window / bucket order, so a ballot prefix is the position), the right hits
                    // upwards from entry 0, the left hits downwards from the last entry: the two sides are two independent chains (below)
#pragma unroll
                    for (int c = 0; c < OVW; c++) L.tslot[ci][c] = ovd[c];
                    const bool isL = (meta & 1u) != 0;
                    const u64 hbR = __ballot(thit[q] && !isL), hbL = __ballot(thit[q] && isL), below = (1ull << lane) - 1ull;
                    if (thit[q]) {
                        const u32 hx = isL ? (u32)(FAST_CAP - 1) - (nL + (u32)__popcll(hbL & below)) : nR + (u32)__popcll(hbR & below);
                        L.candJ[hx] = meta; L.candSrc[hx] = myEnt[q] >> 2; tailSlot[hx] = (uint8_t)ci;
                    }
                    nR += (u32)__popcll(hbR); nL += (u32)__popcll(hbL);
                }
                nhits = nR + nL;
                if (__any(tooLong)) slowpath = true;
                wave_sync();
                STAMP(21);                                                   // (diagnostic builds, forms without run mode: 21 = direct compares + overhangs cut out, 22 = hits written, 23 = the machine's steps)
                if (!slowpath) {
                    if (ALWAYS_TAIL && A.hitBase) {
                        // Noisy data: nearly every read stays unresolved and the reduce phase wants exactly these hits (economyGraph.cpp:591-633: the
                        // true overlaps that are not containments) -- written out here, the reduce phase only has to drop those whose ends turn
                        // out resolved (k_hits_filter) instead of looking everything up and comparing it a second time.
                        u64 hb_; const u32 nhE = emit_hits(thit, tov, ttype, myEnt, iid, hb_);
                        if (lane == 0) { A.hitBase[iid] = hb_; A.hitcount[iid] = nhE; }
                    }
                    STAMP(22);
                    // One step = compare the hit's overhang with the overhang of the side's current `prev` over their common length
                    // (economyGraph.cpp:95-438).  Right and left hits never touch each other's state -- the flags that a change of window
                    // resets belong to one side each, and the hits of a window are contiguous in the visiting order, so "the window changed
                    // since this side's previous hit" is all a side needs to know -- so the two chains run side by side: lanes 0-31 step
                    // through the right hits, lanes 32-63 through the left hits, lane c < OVW of either half holds dword c of its side's prev
                    // overhang, and one ballot gives both sides' verdicts.  The next hit's geometry and overhang come from LDS one and two
                    // steps ahead.  Half as many steps as hits on the longer side, no scalar branches in a step.
                    // Round 4, end: the step is written WITHOUT control flow -- every condition is a 32-bit mask, every conditional assignment a bit-field insert.  As nested ifs
                    // over bools the compiler turned it into ~150 instructions with nine exec-mask branches per step, and the loop was 52 % of the kernel's wave cycles on noisy
                    // data (stamp build: tests/diag/noisy_step.py, stages 21-23).
                    const u32 side = lane >> 5, l5 = lane & 31u, lc = l5 < (u32)OVW ? l5 : 0u;
                    const u32 sideM = side ? ~0u : 0u;
                    // a dword's bases beyond the common length min(pov, ov) are shifted out (2 x t bits, t = 0 .. 16 in two shifts); lanes that hold no dword: always 16
                    const int k16 = l5 < (u32)OVW ? 16 + 16 * (int)l5 : 0x4000;
                    const u32 nS = side ? nL : nR, nmax = max(nR, nL);
                    // the x-th hit of a side: right hits upwards from entry 0, left hits downwards from the last one.  Entries past a side's last hit are read (inside the
                    // wave's block, whatever they hold) and never acted upon: every use below is under actM
                    const u32 dirv = side ? ~0u : 1u; auto at = [&](u32 x) -> u32 { return (side ? (u32)(FAST_CAP - 1) - x : x) & (u32)(FAST_CAP - 1); };
                    auto ins = [](u32 m_, u32 a_, u32 b_) -> u32 { return (m_ & a_) | (~m_ & b_); };                  // v_bfi_b32
                    u32 Id = 0, Oo = 0, Len = 0; bool amb = false, parDone = false;
                    // THE PARALLEL FORM (round 4, end; sides of at most 32 hits, overhangs of at most 16 dwords).  What a step decides is a function of three things that can be
                    // stated without stepping: (1) the `prev` a hit is compared with is the ACCEPTED hit before it with the largest (window, length, earliest) -- a new window's
                    // first accepted hit replaces prev whatever its length, inside a window only a strictly longer one does, and the hits come in window order: one exclusive
                    // prefix maximum of a packed key over the accepted hits of the side; (2) a hit is accepted iff it equals its prev over their common length (the first hit
                    // always; a rejected hit changes nothing but `amb` -- the window flags it resets are functions of the windows alone); (3) the right extension is the
                    // final prev of the FIRST window (`take` needs mF), the left one the final prev of all.  Fixed point from "every hit accepted": lane x holds hit x of its
                    // side (right hits in lanes 0-31, left hits in 32-63), prefix maximum, one compare of OVW dwords per lane, the flagged hits whose prev lies before the
                    // first flagged hit are rejected for good (everything before it is classified correctly, so their prev is the true one), again until nothing is flagged:
                    // rejections + 1 rounds of ~100 instructions instead of max(nR, nL) steps of 66.  More rounds than PAR_MAXIT: the steps below, from the start.
                    // Sides of 33 .. 64 hits: the same with a lane per hit of ONE side over the whole wave, the right side first, then the left one.
                    if constexpr (OVW <= 16) {
                        auto par_form = [&](auto half_c, const u32 fs, u32& oId, u32& oO, u32& oLen, bool& oAmb) -> bool {       // fs: the side of a whole-wave pass
                            constexpr bool HALF = decltype(half_c)::value;
                            constexpr u32 XB = HALF ? 5u : 6u, XM = (1u << XB) - 1u;
                            const u32 sd = HALF ? side : fs;
                            const u32 x = HALF ? l5 : lane, nn = sd ? nL : nR; const bool hv = x < nn;
                            const u32 hx = (sd ? (u32)(FAST_CAP - 1) - x : x) & (u32)(FAST_CAP - 1);
                            const u32 a_ = L.candJ[hx], rid_ = L.candSrc[hx], sl_ = tailSlot[hx] & (u32)(FAST_CAP - 1);
                            const u32 o_ = (a_ >> 1) & 1u, L2_ = (a_ >> 2) & 0x1FFu, ov_ = (a_ >> 20) & 0x3FFu, jw_ = (a_ >> 11) & 0x1FFu;
                            const u32 K_ = hv ? ((jw_ << (9u + XB)) | (L2_ << XB) | (XM - x)) : 0u;       // (L2 >= k > 0: a valid hit's key is never 0)
                            u32 own[OVW];
#pragma unroll
                            for (int c = 0; c < OVW; c++) own[c] = L.tslot[sl_][c];
                            bool rej = false, conv = false; u32 inc_ = 0;
                            for (int it = 0; it < PAR_MAXIT; it++) {
                                const u32 Ka = rej ? 0u : K_;
                                inc_ = HALF ? half_incl_max_dpp(Ka) : wave_incl_max_dpp(Ka);
                                u32 P = (u32)shfl64((int)inc_, (int)((lane - 1u) & 63u)); if (x == 0u) P = 0u;
                                const u32 px = XM - (P & XM), pl = HALF ? ((lane & 32u) | px) : px;        // prev: hit px of this side, in lane pl
                                const u32 ovp = (u32)shfl64((int)ov_, (int)pl), slp = (u32)shfl64((int)sl_, (int)pl);
                                const int m = (int)min(ov_, ovp);
                                u32 d = 0;
#pragma unroll
                                for (int c = 0; c < OVW; c++) d |= (own[c] ^ L.tslot[slp][c]) & mask_top32(m - 16 * c);
                                const bool flag = Ka != 0u && P != 0u && d != 0u;
                                const u64 fb = __builtin_amdgcn_ballot_w64(flag);
                                if (fb == 0ull) { conv = true; break; }
                                u32 x1;                                                                     // this side's first flagged hit
                                if constexpr (HALF) { const u32 fh = side ? (u32)(fb >> 32) : (u32)fb; x1 = fh ? (u32)__builtin_ctz(fh) : 32u; }
                                else x1 = (u32)__builtin_ctzll(fb);
                                rej |= flag && px < x1;
                            }
                            if (!conv) return false;
                            // (inc_: inclusive maxima over the accepted hits of the last round)
                            const u64 rb = __builtin_amdgcn_ballot_w64(rej);
                            const u32 jw0 = (u32)__builtin_amdgcn_readlane((int)jw_, 0);
                            if constexpr (HALF) {
                                const u32 nFirst = (u32)__popcll(__builtin_amdgcn_ballot_w64(lane < nR && jw_ == jw0));      // right hits in the window of the first one: a prefix
                                const u32 Pr = nR ? (u32)__builtin_amdgcn_readlane((int)inc_, (int)(nFirst ? nFirst - 1u : 0u)) : 0u;
                                const u32 Pt = nL ? (u32)__builtin_amdgcn_readlane((int)inc_, 63) : 0u;
                                const int wr = (int)(31u - (Pr & 31u)), wl = (int)(32u + 31u - (Pt & 31u));
                                const u32 rId = nR ? (u32)__builtin_amdgcn_readlane((int)rid_, wr) : 0u, rO = nR ? (u32)__builtin_amdgcn_readlane((int)o_, wr) : 0u, rLen = nR ? (u32)__builtin_amdgcn_readlane((int)ov_, wr) : 0u;
                                const u32 lId = nL ? (u32)__builtin_amdgcn_readlane((int)rid_, wl) : 0u, lO = nL ? (u32)__builtin_amdgcn_readlane((int)o_, wl) : 0u, lLen = nL ? (u32)__builtin_amdgcn_readlane((int)ov_, wl) : 0u;
                                oId = side ? lId : rId; oO = side ? lO : rO; oLen = side ? lLen : rLen; oAmb = (side ? (u32)(rb >> 32) : (u32)rb) != 0u;
                            } else {
                                u32 Pw;
                                if (fs == 0u) { const u32 nFirst = (u32)__popcll(__builtin_amdgcn_ballot_w64(hv && jw_ == jw0)); Pw = nn ? (u32)__builtin_amdgcn_readlane((int)inc_, (int)(nFirst ? nFirst - 1u : 0u)) : 0u; }
                                else Pw = nn ? (u32)__builtin_amdgcn_readlane((int)inc_, 63) : 0u;
                                const int ww = (int)(XM - (Pw & XM));
                                oId = nn ? (u32)__builtin_amdgcn_readlane((int)rid_, ww) : 0u; oO = nn ? (u32)__builtin_amdgcn_readlane((int)o_, ww) : 0u; oLen = nn ? (u32)__builtin_amdgcn_readlane((int)ov_, ww) : 0u;
                                oAmb = rb != 0ull;
                            }
                            return true;
                        };
                        if (COLD(A, noParTail) == 0u) {
                            if (nmax <= 32u) parDone = par_form(std::true_type{}, 0u, Id, Oo, Len, amb);
                            else if (nmax <= 64u) {
                                u32 rI = 0, rO = 0, rL = 0, lI = 0, lO = 0, lL = 0; bool rA = false, lA = false;
                                if (par_form(std::false_type{}, 0u, rI, rO, rL, rA) && par_form(std::false_type{}, 1u, lI, lO, lL, lA)) {
                                    Id = side ? lI : rI; Oo = side ? lO : rO; Len = side ? lL : rL; amb = side ? lA : rA; parDone = true;
                                }
                            }
                        }
                    }
                    if (!parDone) {
                        u32 pL = 0, pov = 0, pw = 0, ambM = 0, mAm = 0, mFm = 0, curJ = ~0u;
                        u32 a0 = L.candJ[at(0)], r20 = L.candSrc[at(0)], a1 = L.candJ[at(1)], r21 = L.candSrc[at(1)];
                        u32 s1 = tailSlot[at(1)] & (u32)(FAST_CAP - 1);
                        u32 cw0 = L.tslot[tailSlot[at(0)] & (u32)(FAST_CAP - 1)][lc];
                        u32 xn = at(1);
                        for (u32 x = 0; x < nmax; x++) {
                            xn = (xn + dirv) & (u32)(FAST_CAP - 1);                               // at(x + 2)
                            const u32 a2 = L.candJ[xn], r22 = L.candSrc[xn], s2 = tailSlot[xn] & (u32)(FAST_CAP - 1);
                            const u32 cw1 = L.tslot[s1][lc];
                            const u32 actM = x < nS ? ~0u : 0u;
                            const u32 a = a0, r2 = r20, cw = cw0;
                            const u32 o = (a >> 1) & 1u, L2 = (a >> 2) & 0x1FFu, ov = (a >> 20) & 0x3FFu, jw = (a >> 11) & 0x1FFu;
                            const u32 nwM = actM & (jw != curJ ? ~0u : 0u);                      // the window changed since this side's previous hit
                            curJ = ins(nwM, jw, curJ); mAm &= ~nwM; mFm &= ~nwM;
                            const int t = min(max(k16 - (int)min(pov, ov), 0), 16);
                            const u64 db = __builtin_amdgcn_ballot_w64(((((pw ^ cw) >> t) >> t) & actM) != 0u);
                            const u32 consM = (side ? (u32)(db >> 32) : (u32)db) == 0u ? ~0u : 0u;
                            const u32 firstM = actM & (Id == 0u ? ~0u : 0u), restM = actM & ~firstM;
                            const u32 c2 = restM & consM;                                         // consistent with the side's prev
                            ambM |= restM & ~consM;
                            const u32 longerM = L2 > pL ? ~0u : 0u;
                            const u32 updI = longerM | ~mAm;                                      // :  a longer read 2 in the same window, or the first hit of a new window
                            const u32 updM = c2 & updI;
                            const u32 takeM = c2 & ((sideM & updI) | (~sideM & mAm & longerM & mFm));   // the right extension follows only inside the window of its first hit
                            const u32 set1 = firstM | takeM, set2 = firstM | updM;
                            Id = ins(set1, r2, Id); Oo = ins(set1, o, Oo); Len = ins(set1, ov, Len);
                            pw = ins(set2, cw, pw); pL = ins(set2, L2, pL); pov = ins(set2, ov, pov);
                            mAm |= firstM | c2; mFm |= firstM;
                            a0 = a1; r20 = r21; cw0 = cw1; a1 = a2; r21 = r22; s1 = s2;
                        }
                        amb = ambM != 0u;
                    }
                    const bool ambAny = __ballot(amb) != 0ull;                                              // economyGraph.cpp:446-450
                    const u32 rightId = (u32)__builtin_amdgcn_readlane((int)Id, 0), leftId = (u32)__builtin_amdgcn_readlane((int)Id, 32);
                    const u32 rightO = (u32)__builtin_amdgcn_readlane((int)Oo, 0), leftO = (u32)__builtin_amdgcn_readlane((int)Oo, 32);
                    const u32 rightLen = ambAny ? 0u : (u32)__builtin_amdgcn_readlane((int)Len, 0), leftLen = ambAny ? 0u : (u32)__builtin_amdgcn_readlane((int)Len, 32);
                    if (lane == 0) {                                                                        // (records by position, neighbours as positions)
                        A.right[i] = (u64)rightId | ((u64)rightO << 40) | ((u64)(rightLen & 0x3FFFFFu) << 42);
                        A.left[i] = (u64)leftId | ((u64)leftO << 40) | ((u64)(leftLen & 0x3FFFFFu) << 42);
                        A.conn[i] = nhits;
                    }
                    STAMP(23);
                    continue;
                }
            }
        }
        STAMP(8);
        if (slowpath) {
            if (lane == 0) { u64* cn_ = COLD(A, counters); u64 p = atomicAdd(&cn_[CTR_HANDED], 1ull); if (p < COLD(A, slow_cap)) COLD(A, slow)[p] = (u32)i; if (capOver) atomicAdd(&cn_[CTR_HANDED + 1], 1ull); }
        } else if (HITS) {
            // (not reached: the hit-list variant leaves the loop body above)
        } else {
            // ---------------------------------------------------------------- 5. extension records
            if constexpr (SEQ) { const u32 pk_ = wave_pk_min_dpp(selR); const u32 kr_ = pk_ >> 16, kl_ = pk_ & 0xFFFFu;      // (back to the other forms' layout: slot in the low 8 bits)
                                 selR = kr_ == 0xFFFFu ? ~0u : (kr_ & 0xFFu); selL = kl_ == 0xFFFFu ? ~0u : (kl_ & 0xFFu); }
            else { selR = wave_min_dpp(selR); selL = wave_min_dpp(selL); }
            u64 rv = 0, lv = 0; u32 pr = 0, pl = 0;                                  // (neighbours as positions)
            if (selR != ~0u) {
                const int ol = (int)(selR & 63u); const u32 oq = (selR >> 6) & 3u;
                const u32 en = (u32)pick_lane(myEnt, oq, ol);
                const int j = pick_lane(myJ, oq, ol), L2 = UNI ? A.uniL : pick_lane(myL2, oq, ol);
                pr = en >> 2; rv = ((u64)((en & 3) == 2 ? 1 : 0) << 40) | ((u64)((u32)(L2 - (L1 - j)) & 0x3FFFFFu) << 42);
            }
            if (selL != ~0u) {
                const int ol = (int)(selL & 63u); const u32 oq = (selL >> 6) & 3u;
                const u32 en = (u32)pick_lane(myEnt, oq, ol);
                const int j = pick_lane(myJ, oq, ol), L2 = UNI ? A.uniL : pick_lane(myL2, oq, ol);
                pl = en >> 2; lv = ((u64)((en & 3) == 3 ? 1 : 0) << 40) | ((u64)((u32)(L2 - j - h) & 0x3FFFFFu) << 42);
            }
            if (lane == 0) { A.right[i] = rv | (u64)pr; A.left[i] = lv | (u64)pl; A.conn[i] = nhits; }
        }
        STAMP(9);
    }
    if constexpr (RUN) {                                           // the wave's run counters go to the device's once, when it has run out of items
        wave_sync();
        const u32 rc_ = lane < 4u ? (u32)L.rsx[RSX_CNT + lane] : 0u;
        if (rc_ != 0u) atomicAdd(&COLD(A, counters)[CTR_RUNSTATS + lane], (u64)rc_);
    }
    if (HITS || (ALWAYS_TAIL && A.hitBase)) {
        for (u32 x = lane; x < hLeft; x += 64) A.hits[hBase + x].from = 0;
        if (lane == 0 && hTotal) atomicAdd(&A.counters[CTR_HIT_REAL], hTotal);
    }
#ifdef SAGE2OV_STAMPS
    if (A.stamps && lane == 0) for (int x = 0; x < 32; x++) atomicAdd(&A.stamps[x], st_acc[x]);
#endif
}

