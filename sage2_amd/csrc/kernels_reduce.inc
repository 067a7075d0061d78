// sage2_amd/csrc/kernels_reduce.inc -- reduce phase on the device (order-independent form).
// Part of sage2ov_device.hip (included inside namespace s2, in this order); not a translation unit of its own.

// =============================================================================================
// Reduce phase on the device (economyGraph.cpp:495-707) -- order-independent form, SURVEY A.6.
// Exact when discovery is symmetric, i.e. when no bucket is long (every S-S overlap is then seen from both
// sides, contained reads are never in S, and at the time markTransitiveEdge(r) runs in the serial BFS the lists
// of r and of all its neighbours are complete and unreduced).  The serial replay on the host remains the
// path for indexes with long buckets and for a handful of unresolved reads.
//   list[r] (all reads) = both directed entries of every reciprocal-pass candidate + for r in S its own hits;
//   for r in S: sort (len desc, id desc, type desc) (:853-871), mark (:643-679), drop marked (:681-707);
//   survivors with to > r replace the candidates owned by r.
// Entry = len:20 | to:32 | type:2 | position:9 (spare bits of the sort key carry the entry's place in the list).
// =============================================================================================
constexpr int RA_CAP = 512;                       // longest list handled on the device (connections <= 300 for S reads)
constexpr int RA_HT = 1024;
__device__ __forceinline__ u64 ra_key(u32 to, u32 type, u32 len) { return ((u64)(len & 0xFFFFFu) << 43) | ((u64)to << 11) | ((u64)(type & 3u) << 9); }
__device__ __forceinline__ u32 ra_to(u64 k) { return (u32)(k >> 11); }
__device__ __forceinline__ u32 ra_type(u64 k) { return (u32)(k >> 9) & 3u; }
__device__ __forceinline__ u32 ra_len(u64 k) { return (u32)(k >> 43) & 0xFFFFFu; }
__global__ void k_ra_degree_c(EdgeCand* cand, u64 n, const uint8_t* __restrict__ status, u32* deg) {
    u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (x >= n) return;
    EdgeCand e = cand[x]; e.type &= 0x7Fu;
    atomicAdd(&deg[e.from], 1u); atomicAdd(&deg[e.to], 1u);
    if (status[e.from] == 0) cand[x].type = e.type | 0x80u;            // list of an unresolved read: re-emitted after the reduction
}
// Hits written out by the initial pass (k_probe_fast<..., TAIL = 2>, every read, before anybody's status was known) -> the hit lists of the
// reduce phase (economyGraph.cpp:591-633: both ends unresolved): in place, one wave per read.  A dropped hit gets from = 0 (the mark of an
// unused slot that every consumer skips), the kept ones are renumbered, hitcount[r] = kept.  Reads the initial pass did not write out
// (base ~0: sample launch, listed reads, hand-overs) are listed by POSITION if unresolved: the hit-list kernel runs for them alone.
// counters: [0] kept hits, [1] listed reads
// (The initial pass leaves `to` as a POSITION in the locality order: a read's hits are its neighbours there, so statusP[] and idOf[] are read
// next to each other here instead of all over status[]; the kept hits get their read id.)
// (Round 4, end: a wave per read was a chain of three dependent round trips per read -- base, hits, neighbours' statuses -- and the launch was bound by that latency, not
// by bytes: 5.7 ms for 7.4 GB.  Now a wave takes 64 consecutive reads: one coalesced load of their bases / counts / statuses, then read by read with the next read's hits
// fetched while this read's neighbours are looked up -- one round trip per read.)
__global__ void k_hits_filter(Hit* hits, const u64* __restrict__ hitBase, const uint8_t* __restrict__ status, const uint8_t* __restrict__ statusP, const u32* __restrict__ idOf,
                              const u32* __restrict__ posOf, u64 N, u32* hitcount, u32* noneList, u64* counters) {
    const u32 lane = lane_id(); u64 keptTotal = 0;
    const u64 nChunks = (N + 63) >> 6, nWaves = ((u64)gridDim.x * blockDim.x) >> 6;
    auto load_hit = [&](u64 b, u32 n, u32 x0) -> Hit { Hit h; h.from = 0; h.to = 0; h.len = 0; h.seq = 0; h.type = 0; if (b != ~0ull && x0 + lane < n) h = hits[b + x0 + lane]; return h; };
    for (u64 c = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6; c < nChunks; c += nWaves) {
        const u64 r = 1 + (c << 6) + lane; const bool rv = r <= N;
        const u64 myB = rv ? hitBase[r] : ~0ull; const u32 myN = rv ? hitcount[r] : 0u; const bool myAlive = rv && status[r] == 0;
        const u64 aliveB = __ballot(myAlive);
        // reads the initial pass did not write out: listed by position if unresolved (one atomic per wave)
        { const u64 lb = __ballot(rv && myB == ~0ull && myAlive);
          if (lb) { u64 p0 = 0; if (lane == 0) p0 = atomicAdd((unsigned long long*)&counters[1], (unsigned long long)__popcll(lb));
                    p0 = ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(p0 >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)(u32)p0);
                    if ((lb >> lane) & 1ull) noneList[p0 + (u64)__popcll(lb & ((1ull << lane) - 1ull))] = posOf[r]; } }
        u32 myKept = 0;
        const u32 bLo = (u32)myB, bHi = (u32)(myB >> 32);
        auto base_of = [&](int j) -> u64 { return ((u64)(u32)__builtin_amdgcn_readlane((int)bHi, j) << 32) | (u32)__builtin_amdgcn_readlane((int)bLo, j); };
        Hit nxt = load_hit(base_of(0), (u32)__builtin_amdgcn_readlane((int)myN, 0), 0);
        for (int j = 0; j < 64; j++) {
            const u64 b = base_of(j); const u32 n = (u32)__builtin_amdgcn_readlane((int)myN, j); const bool alive = ((aliveB >> j) & 1ull) != 0;
            Hit h = nxt;
            const u32 tp0 = h.to; const bool v0 = b != ~0ull && lane < n;
            uint8_t st0 = 1; u32 id0 = 0; if (v0) { st0 = statusP[tp0]; id0 = idOf[tp0]; }            // (this read's gathers go out first ...)
            if (j + 1 < 64) nxt = load_hit(base_of(j + 1), (u32)__builtin_amdgcn_readlane((int)myN, j + 1), 0);   // (... the next read's hits ride along)
            if (b == ~0ull || n == 0) continue;
            u32 kept = 0;
            for (u32 x0 = 0; x0 < n; x0 += 64) {
                const u32 x = x0 + lane; const bool v = x < n;
                uint8_t st = st0; u32 id2 = id0;
                if (x0) { h = load_hit(b, n, x0); st = 1; id2 = 0; if (v) { st = statusP[h.to]; id2 = idOf[h.to]; } }
                const bool keep = v && alive && st == 0;
                const u64 bal = __ballot(keep);
                if (v) { if (keep) { h.to = id2; h.seq = kept + (u32)__popcll(bal & ((1ull << lane) - 1ull)); } else h.from = 0; hits[b + x] = h; }
                kept += (u32)__popcll(bal);
            }
            if (lane == (u32)j) myKept = kept;
            keptTotal += kept;
        }
        if (rv) hitcount[r] = myKept;
    }
    if (lane == 0 && keptTotal) atomicAdd((unsigned long long*)&counters[0], (unsigned long long)keptTotal);
}
__global__ void k_ra_degree_h(const u32* __restrict__ hitcount, u64 N, u32* deg) {       // deg[i] = candidate entries + own hits
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (i > N) return;
    deg[i] += hitcount[i];
}
// An entry goes into the list twice: the 64-bit key the marks' kernel sorts (len | to | type | index) and a 32-bit image (to:30 | type:2, ids stay below 2^30) at the same
// place -- what the kernel reads of the NEIGHBOURS' lists, where only (to, type) matter: half the bytes per list.  (Rounds 2-3 wrote the image in a pass of its own,
// partitioned by the high bit of the type so that the walk of every list fetched only the half that continues in its direction; since round 4 the marks come
// from 2-3 whole lists per read -- both halves: the other one names the list's potential markers -- and the pass, 3.1 ms at configs[1] + 0.1 % errors, is gone.)
__device__ __forceinline__ void ra_put(u64* ent, u32* ent32, u64 at, u32 to, u32 type, u32 len) { ent[at] = ra_key(to, type, len); ent32[at] = (to << 2) | (type & 3u); }
__global__ void k_ra_fill_c(const EdgeCand* __restrict__ cand, u64 n, const u64* __restrict__ reads, int S, int uniL, const u32* __restrict__ offs, u32* cursor, u64* ent, u32* ent32) {
    u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (x >= n) return;
    EdgeCand e = cand[x]; e.type &= 0x7Fu;
    const int Lf = read_len(reads, S, e.from, uniL), Lt = read_len(reads, S, e.to, uniL);
    ra_put(ent, ent32, (u64)offs[e.from] + atomicAdd(&cursor[e.from], 1u), e.to, e.type, e.len);
    ra_put(ent, ent32, (u64)offs[e.to] + atomicAdd(&cursor[e.to], 1u), e.from, flip_type(e.type), (u32)(Lf - (Lt - (int)e.len)));   // the twin (economyGraph.cpp:821)
}
__global__ void k_ra_fill_h(const Hit* __restrict__ hits, u64 n, const u32* __restrict__ offs, const u32* __restrict__ deg, const u32* __restrict__ hitcount, u64* ent, u32* ent32) {
    u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (x >= n) return;
    const Hit h = hits[x];                                               // the hits of a read are numbered 0.. by the probe kernel: no cursor
    if (h.from == 0) return;                                             // unused slot of a wave's chunk
    ra_put(ent, ent32, (u64)offs[h.from] + (deg[h.from] - hitcount[h.from]) + h.seq, h.to, h.type, (u32)h.len);
}
// Two sizes of the per-wave work space: lists of at most 128 entries (nearly all) take 2.5 KB and leave the CU to the register-bound six waves
// per SIMD; the 10 KB of the full size (RA_CAP entries) allow four.  The walk is a chain of dependent LDS accesses: waves in flight are its throughput.
template <int CAP, int HTLOG> struct RaLds { static constexpr int HT = 1 << HTLOG; u64 key[CAP]; u32 ht[HT]; uint8_t mk[HT]; unsigned short slot[CAP]; uint8_t ord[CAP <= 128 ? HT : 1]; };
template <int HTLOG> __device__ __forceinline__ u32 ra_hash(u32 id) { return (id * 2654435761u) >> (32 - HTLOG); }
template <int CAP, int HTLOG> __device__ __forceinline__ void ra_mark_one(RaLds<CAP, HTLOG>& L, u32 kb32, u32 t1) {
    constexpr int RA_HT = 1 << HTLOG;
    const u32 b = kb32 >> 2, t2 = kb32 & 3u;
    // (:654-666) the second edge continues in the direction the first one arrives: t1 in {0,2} with t2 in {0,1}, t1 in {1,3} with t2 in {2,3}
    if (((t1 ^ (t2 >> 1)) & 1u) != 0) return;                                   // (the low bit of t1 must equal the high bit of t2)
    u32 sidx = ra_hash<HTLOG>(b);
    u32 v = L.ht[sidx];
    while (v != 0 && v != b) { sidx = (sidx + 1) & (RA_HT - 1); v = L.ht[sidx]; }      // (the table is at most half full: almost never taken)
    if (v == b && L.mk[sidx] == 1) L.mk[sidx] = 2;
}
// slot of entry kb's target in the node table if the pair (t1, its type) continues in one direction (:654-666) and the target is a neighbour, else ~0
template <int CAP, int HTLOG> __device__ __forceinline__ u32 ra_find(const RaLds<CAP, HTLOG>& L, u32 kb32, u32 t1, bool valid) {
    constexpr int RA_HT = 1 << HTLOG;
    const u32 b = kb32 >> 2, t2 = kb32 & 3u;
    if (!valid || ((t1 ^ (t2 >> 1)) & 1u) != 0) return ~0u;
    u32 sidx = ra_hash<HTLOG>(b);
    u32 v = L.ht[sidx];
    while (v != 0 && v != b) { sidx = (sidx + 1) & (RA_HT - 1); v = L.ht[sidx]; }
    return v == b ? sidx : ~0u;
}
// THE SHORT CUT (round 4).  markTransitiveEdge (:643-679) walks r's list in the order of the sort -- the longest edge, i.e. the FARTHEST neighbour, first -- and a neighbour
// is eliminated by nearer ones, i.e. after its own turn: every list is walked (51.6 of 51.6 at configs[1] + 0.1 % errors).  The result does not need them all.  With
// C(a) = the nodes of r's list that a's list holds in the continuing direction, and the lists symmetric (every edge is stored with its twin, :821, so a's list also names
// the nodes that hold a: its POTENTIAL MARKERS, the entries whose twin continues the edge r -> that node):
//   (1) a node without potential markers is never eliminated -- and it is in play at its turn, so all of C(a) is;
//   (2) a node none of whose potential markers comes EARLIER in the order is in play at its turn whatever happens to it later: all of C(a) is eliminated;
//   (3) the eliminated nodes are a subset of the union of all C(a).
// So: take the unknown node nearest the end of the order (the nearest neighbour), read its list once -- C(a), its potential markers, whether one of them is earlier (then
// give up: the sequential rule matters) --, eliminate C(a); a node without potential markers is final; one with potential markers needs a witness: its marker nearest the end is read
// the same way.  When no unknown node is left the marks are those of the walk: 3-6 lists per read instead of all.  Anything unexpected (an earlier marker, two entries to one node,
// a mark on a node proven unmarkable = lists that are not symmetric, too many lists) leaves the read to the walk, marks reset.  mk: 1 unknown, 2 eliminated, 3 proven not eliminated.
constexpr int RA_SC_PRE = 8;                      // neighbours at the end of the order whose list extents the short cut fetches up front
constexpr int RA_SHORTCUT_LISTS = 24;             // most lists the short cut reads for one read before it leaves the read to the walk
template <int CAP, int HTLOG>
__device__ __forceinline__ bool ra_shortcut(RaLds<CAP, HTLOG>& L, u32 n, u32 lane, bool dupNode, u32 dgP, u32 ofP, const u32* __restrict__ deg, const u32* __restrict__ offs, const u32* __restrict__ ent32, u64& listsRead) {
    constexpr int RA_HT = 1 << HTLOG;
    if (__any(dupNode)) return false;
    for (u32 x = lane; x < n; x += 64) L.ord[L.slot[x]] = (uint8_t)x;
    wave_sync();
    bool bad = false;
    // one list: returns false when the sequential rule matters; pm = the node has potential markers, wmax = the one nearest the end of the order
    auto one = [&](u32 x, bool& pm, u32& wmax) -> bool {
        const u32 t1 = ra_type(L.key[x]);
        const u32 back = n - 1u - x; u32 dg, of;
        if (back < (u32)RA_SC_PRE) { dg = (u32)__builtin_amdgcn_readlane((int)dgP, (int)back); of = (u32)__builtin_amdgcn_readlane((int)ofP, (int)back); }
        else { const u32 a = ra_to(L.key[x]); dg = deg[a]; of = offs[a]; }
        bool anyPm = false, early = false; u32 wm = 0;
        u32 e0 = 0, s0 = ~0u;                                   // the first 64 entries stay in registers for the second pass
        for (u32 y0 = 0; y0 < dg; y0 += 64) {
            const u32 y = y0 + lane; const bool v = y < dg;
            const u32 e = ent32[of + (v ? y : 0u)];
            const u32 b = e >> 2;
            u32 sidx = ra_hash<HTLOG>(b); u32 hv = L.ht[sidx];
            while (v && hv != 0 && hv != b) { sidx = (sidx + 1) & (RA_HT - 1); hv = L.ht[sidx]; }
            const bool found = v && hv == b;
            if (found) {
                const u32 ob = L.ord[sidx]; const u32 t1b = ra_type(L.key[ob]);
                if ((t1b & 1u) == (flip_type(e & 3u) >> 1)) { anyPm = true; early |= ob < x; wm = max(wm, ob); }      // the twin b -> a continues r -> b
            }
            if (y0 == 0) { e0 = e; s0 = found ? sidx : ~0u; }
        }
        if (__any(early)) return false;
        pm = __any(anyPm);
        if (pm) { for (int dlt = 32; dlt; dlt >>= 1) wm = max(wm, (u32)__shfl_xor((int)wm, dlt)); }      // (the nearest neighbours have no marker: no reduction for them)
        wmax = wm;
        // in play at its turn: C(a) is eliminated
        bool contra = false;
        if (s0 != ~0u && ((t1 ^ ((e0 & 3u) >> 1)) & 1u) == 0u) { if (L.mk[s0] == 3) contra = true; else L.mk[s0] = 2; }
        for (u32 y0 = 64; y0 < dg; y0 += 64) {
            const u32 y = y0 + lane; const bool v = y < dg;
            const u32 e = ent32[of + (v ? y : 0u)];
            const u32 b = e >> 2;
            u32 sidx = ra_hash<HTLOG>(b); u32 hv = L.ht[sidx];
            while (v && hv != 0 && hv != b) { sidx = (sidx + 1) & (RA_HT - 1); hv = L.ht[sidx]; }
            if (v && hv == b && ((t1 ^ ((e & 3u) >> 1)) & 1u) == 0u) { if (L.mk[sidx] == 3) contra = true; else L.mk[sidx] = 2; }
        }
        wave_sync();
        return !__any(contra);
    };
    u32 lists = 0;
    for (;;) {
        const u64 b0 = __ballot(lane < n && L.mk[L.slot[lane < n ? lane : 0]] == 1), b1 = __ballot(lane + 64 < n && L.mk[L.slot[lane + 64 < n ? lane + 64 : 0]] == 1);
        if ((b0 | b1) == 0) break;
        const u32 x = b1 ? 64u + 63u - (u32)__builtin_clzll(b1) : 63u - (u32)__builtin_clzll(b0);
        if (++lists > (u32)RA_SHORTCUT_LISTS) { bad = true; break; }
        bool pm = false; u32 w = 0;
        if (!one(x, pm, w)) { bad = true; break; }
        const u32 sx = L.slot[x];
        if (!pm) { if (lane == 0 && L.mk[sx] == 1) L.mk[sx] = 3; wave_sync(); if (L.mk[sx] != 3) { bad = true; break; } continue; }    // (it marked itself and has no marker: impossible)
        if (L.mk[sx] == 2) continue;                            // (its own list eliminated it: a self edge, in play at its turn)
        // a witness: its marker nearest the end of the order must be in play at ITS turn
        if (w <= x || L.mk[L.slot[w]] != 2) { bad = true; break; }
        if (++lists > (u32)RA_SHORTCUT_LISTS) { bad = true; break; }
        bool pmw = false; u32 ww = 0;
        if (!one(w, pmw, ww) || L.mk[sx] != 2) { bad = true; break; }
    }
    listsRead += lists;
    if (bad) { for (u32 x = lane; x < n; x += 64) L.mk[L.slot[x]] = 1; wave_sync(); return false; }
    return true;
}
// counters: [0] lists longer than RA_CAP (-> k_ra_mark_big), [1] removed entries.  svn[w] = survivors with to > r of the w-th read.
// The reads whose list has more than NLO and at most CAP entries (NLO = 0: empty lists too); the last size class hands longer lists over.
constexpr int RA_B = 6;                           // neighbour lists fetched and looked up together
constexpr int RA_BLOCKS = 8;                      // occupancy bound of k_ra_mark's __launch_bounds__ for lists of at most 128 entries (longer lists: 4)
template <int CAP, int HTLOG, int NLO, bool LAST>
__global__ __launch_bounds__(256, (CAP <= 128 ? RA_BLOCKS : 4)) void k_ra_mark(const u32* __restrict__ ids, u64 nids, const u32* __restrict__ offs, const u32* __restrict__ deg,
                                                 const u64* __restrict__ ent, const u32* __restrict__ ent32, uint8_t* rm, u32* svn, u64* counters, u32* heavy, u64 heavyCap, u32 noShortcut, u32* mid) {
    constexpr int RA_HT = 1 << HTLOG;
    __shared__ RaLds<CAP, HTLOG> lds[4];
    u64 shortDone = 0, shortLists = 0;
    RaLds<CAP, HTLOG>& L = lds[threadIdx.x >> 6];
    const u32 lane = lane_id();
    u64 removedTotal = 0;
#ifdef RA_EXP_STAMPS
    u64 ra_t[8] = {0, 0, 0, 0, 0, 0, 0, 0}; u64 ra_prev = 0, ra_reads = 0, ra_nb = 0;
#define RA_STAMP(k) do { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); const u64 t_ = __builtin_amdgcn_s_memtime(); ra_t[k] += t_ - ra_prev; ra_prev = t_; } while (0)
#else
#define RA_STAMP(k) do { } while (0)
#endif
    // (the first size class lists the reads it leaves to the second -- mid[0 .. counters[4]) -- which then visits those alone instead of running over all the reads again)
    const u64 nloop = (NLO != 0 && mid) ? counters[4] : nids;
    // (Round 4, end.)  A read's marks are a chain of dependent round trips -- id -> list extent -> list -> extents of the nearest neighbours -> the 2.3 lists of the short cut --
    // and at eight waves per SIMD the kernel waits on that chain (stamp build: 42 % of a read's cycles before the sort, 42 % in the short cut's loads).  The first size class
    // therefore runs its first three links AHEAD: the id of the wave's read after next but one, the extent of the read after next and the list of the next read are in
    // flight while this read is worked on.  The wave number goes through readfirstlane so that ids / extents are scalar loads into scalar registers (the kernel sits at
    // 55 of the 64 vector registers that eight waves allow).
    constexpr bool PIPE = CAP <= 128 && NLO == 0;
    const u64 wstride = (u64)gridDim.x * 4;
    const u64 wx0 = (u64)blockIdx.x * 4 + (PIPE ? (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : (threadIdx.x >> 6));
    u32 pr_b = 0, pn_b = 0, po_b = 0, pr_c = 0, pr_a = 0, pn_a = 0, po_a = 0; u64 pk0 = 0, pk1 = 0;
    auto pl_id = [&](u64 x) -> u32 { return x < nloop ? ids[x] : 0u; };
    auto pl_list = [&](u32 n_, u32 o_, u64& k0_, u64& k1_) { const bool us = n_ != 0 && n_ <= (u32)CAP; k0_ = (us && lane < n_) ? (ent[o_ + lane] | (u64)lane) : 0ull; k1_ = (us && lane + 64u < n_) ? (ent[o_ + lane + 64u] | (u64)(lane + 64u)) : 0ull; };
    if constexpr (PIPE) {
        pr_a = pl_id(wx0); pr_b = pl_id(wx0 + wstride); pr_c = pl_id(wx0 + 2 * wstride);
        pn_a = wx0 < nloop ? deg[pr_a] : 0u; po_a = offs[pr_a]; pn_b = wx0 + wstride < nloop ? deg[pr_b] : 0u; po_b = offs[pr_b];
        pl_list(pn_a, po_a, pk0, pk1);
    }
    for (u64 wx = wx0; wx < nloop; wx += wstride) {
        const u64 w = (NLO != 0 && mid) ? (u64)mid[wx] : wx;
        u32 r, n, o; u64 k0p = 0, k1p = 0;
        if constexpr (PIPE) {
            r = pr_a; n = pn_a; o = po_a; k0p = pk0; k1p = pk1;
            const u32 r_d = pl_id(wx + 3 * wstride);
            const u32 n_c = wx + 2 * wstride < nloop ? deg[pr_c] : 0u, o_c = offs[pr_c];
            pl_list(pn_b, po_b, pk0, pk1);
            pr_a = pr_b; pn_a = pn_b; po_a = po_b; pr_b = pr_c; pn_b = n_c; po_b = o_c; pr_c = r_d;
        } else { r = ids[w]; n = deg[r]; o = offs[r]; }
        if (n == 0) { if (NLO == 0 && lane == 0) svn[w] = 0; continue; }
        if (n <= (u32)NLO) continue;                                               // (another size class)
        if (NLO == 0 && !LAST && n > (u32)CAP && mid) { if (lane == 0) mid[atomicAdd((unsigned long long*)&counters[4], 1ull)] = (u32)w; continue; }
        if (n > (u32)CAP) { if (LAST && lane == 0) { svn[w] = 0; const u64 at = atomicAdd((unsigned long long*)&counters[0], 1ull); if (heavy && at < heavyCap) heavy[at] = (u32)w; } continue; }   // -> k_ra_mark_big
        u32 P = 64; while (P < n) P <<= 1;
        wave_sync();
#ifdef RA_EXP_STAMPS
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); ra_prev = __builtin_amdgcn_s_memtime(); ra_reads++; ra_nb += n;
#endif
        bool sorted = false;
        if constexpr (CAP <= 128) {
            // (lists of at most 128 entries: sorted by COUNTING -- an entry's place is the number of keys greater than its own; the keys are distinct (their low bits are
            //  the entry's index) and go round as scalars, two entries per lane: no LDS round trip, no barrier, where the bitonic network below has 21-28 of each)
            u64 k0, k1; if constexpr (PIPE) { k0 = k0p; k1 = k1p; } else { k0 = lane < n ? (ent[o + lane] | (u64)lane) : 0ull; k1 = lane + 64u < n ? (ent[o + lane + 64u] | (u64)(lane + 64u)) : 0ull; }
            for (u32 x = lane; x < (u32)RA_HT; x += 64) { L.ht[x] = 0; L.mk[x] = 0; }
            u32 r0 = 0, r1 = 0;
            const u32 nlo = n < 64u ? n : 64u;
            if (n <= 64u) {                                   // (one entry per lane -- the mean list has 52: the second entry's count is not kept up; four keys per
                u32 ra = 0, rb = 0;                            //  trip, lanes past the list hold key 0, which is greater than nothing: no remainder loop)
                for (u32 j = 0; j < nlo; j += 4) {
                    const u32 k0h = (u32)(k0 >> 32), k0l = (u32)k0;
                    const u64 ka = ((u64)(u32)__builtin_amdgcn_readlane((int)k0h, (int)j) << 32) | (u32)__builtin_amdgcn_readlane((int)k0l, (int)j);
                    const u64 kb = ((u64)(u32)__builtin_amdgcn_readlane((int)k0h, (int)(j + 1u)) << 32) | (u32)__builtin_amdgcn_readlane((int)k0l, (int)(j + 1u));
                    const u64 kc = ((u64)(u32)__builtin_amdgcn_readlane((int)k0h, (int)(j + 2u)) << 32) | (u32)__builtin_amdgcn_readlane((int)k0l, (int)(j + 2u));
                    const u64 kd = ((u64)(u32)__builtin_amdgcn_readlane((int)k0h, (int)(j + 3u)) << 32) | (u32)__builtin_amdgcn_readlane((int)k0l, (int)(j + 3u));
                    ra += ka > k0 ? 1u : 0u; rb += kb > k0 ? 1u : 0u; ra += kc > k0 ? 1u : 0u; rb += kd > k0 ? 1u : 0u;
                }
                r0 = ra + rb;
            } else
            for (u32 j = 0; j < nlo; j++) {
                const u64 kj = ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(k0 >> 32), (int)j) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)k0, (int)j);
                r0 += kj > k0 ? 1u : 0u; r1 += kj > k1 ? 1u : 0u;
            }
            for (u32 j = 64; j < n; j++) {
                const u64 kj = ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(k1 >> 32), (int)(j - 64u)) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)k1, (int)(j - 64u));
                r0 += kj > k0 ? 1u : 0u; r1 += kj > k1 ? 1u : 0u;
            }
            if (lane < n) L.key[r0] = k0;
            if (lane + 64u < n) L.key[r1] = k1;
            for (u32 x = n + lane; x < P; x += 64) L.key[x] = 0ull;
            sorted = true;
        } else {
            for (u32 x = lane; x < P; x += 64) L.key[x] = x < n ? (ent[o + x] | (u64)x) : 0ull;
            for (u32 x = lane; x < (u32)RA_HT; x += 64) { L.ht[x] = 0; L.mk[x] = 0; }
        }
        wave_sync();
        RA_STAMP(0);
        // bitonic sort, descending: (len, id, type) as in compareEdges (:853-871)
#ifndef RA_EXP_NOSORT
        if (!sorted)
        for (u32 k = 2; k <= P; k <<= 1)
            for (u32 j = k >> 1; j > 0; j >>= 1) {
                for (u32 t = lane; t < P / 2; t += 64) {
                    const u32 i = ((t / j) * 2 * j) + (t % j), l = i + j;
                    const u64 a = L.key[i], b = L.key[l];
                    const bool desc = (i & k) == 0;
                    if (desc ? (a < b) : (a > b)) { L.key[i] = b; L.key[l] = a; }
                }
                wave_sync();
            }
#endif
        RA_STAMP(1);
        // node table: one mark per neighbour id (several entries may lead to the same read)
        bool dupNode = false;                                                      // (two entries lead to one read: the short cut below leaves such lists to the walk)
        for (u32 x = lane; x < n; x += 64) {
            const u32 id = ra_to(L.key[x]); u32 sidx = ra_hash<HTLOG>(id);
            for (;;) {
                const u32 old = atomicCAS(&L.ht[sidx], 0u, id);
                if (old == id) dupNode = true;
                if (old == 0 || old == id) break;
                sidx = (sidx + 1) & (RA_HT - 1);
            }
            L.slot[x] = (unsigned short)sidx; L.mk[sidx] = 1;
        }
        wave_sync();
        RA_STAMP(2);
        // markTransitiveEdge (:643-679): sequential over the sorted list.  A neighbour that an earlier one has eliminated is skipped (:648); with
        // the reference's order (longest overhang first) that is rare, so a read with 60 neighbours walks 60 lists.  The walk is a chain of
        // dependent accesses (LDS look-ups, two memory round trips per neighbour), which is taken out of the serial order where the order
        // does not matter: (1) list location and size of every neighbour are fetched once, up front (lane x holds those of positions x and
        // x + 64; longer lists fetch them per batch); (2) the neighbours in play at the start of a 64-position window are walked in batches
        // of RA_B: their entries (two per lane; a list beyond 128 entries is rare) are fetched together; (3) the node table is read-only
        // during the walk: the targets of all lists of a batch are looked up together, the marks are then set list by list, each list only
        // if its neighbour is still in play when its turn comes -- the serial order of :648.  (Measured: RA_B = 4 at eight waves per SIMD;
        // eight lists per batch need registers that cost the occupancy; fetching batch k + 1 during batch k likewise.)
        const bool small = n <= 128;
        // neighbour a's list (whole: the walk's per-entry test drops the entries that do not continue the edge r -> a of type t1)
        auto part = [&](u32 a, u32 t1, bool v, u32& cnt, u32& off) { (void)t1; cnt = v ? deg[a] : 0u; off = offs[a]; };
        u32 dA0 = 0, oA0 = 0, dA1 = 0, oA1 = 0;
        bool fastDone = false;
        if (small) {
            if constexpr (CAP <= 128) {
                if (!noShortcut) {
                    // (list location and size of the neighbours at the END of the order -- the nearest ones, the lists the short cut reads -- fetched together: lane j holds
                    //  those of position n - 1 - j; a list further up is located when it is read)
                    const bool pv = lane < (u32)RA_SC_PRE && lane < n; const u32 ap = ra_to(L.key[pv ? n - 1u - lane : 0u]);
                    const u32 dgP = pv ? deg[ap] : 0u, ofP = offs[ap];
                    fastDone = ra_shortcut<CAP, HTLOG>(L, n, lane, dupNode, dgP, ofP, deg, offs, ent32, shortLists); shortDone += fastDone ? 1 : 0;
                }
            }
            if (!fastDone) {
                const u64 k0 = L.key[lane < n ? lane : 0], k1 = L.key[lane + 64 < n ? lane + 64 : 0];
                part(lane < n ? ra_to(k0) : 0u, ra_type(k0), lane < n, dA0, oA0); part(lane + 64 < n ? ra_to(k1) : 0u, ra_type(k1), lane + 64 < n, dA1, oA1);
            }
        }
        RA_STAMP(3);
        auto take8 = [&](u64& bal, u32 x, u32 (&pa)[RA_B]) {
#pragma unroll
            for (int u = 0; u < RA_B; u++) { if (bal) { pa[u] = x + (u32)__builtin_ctzll(bal); bal &= bal - 1; } else pa[u] = ~0u; }
        };
        auto fetch = [&](const u32 (&pa)[RA_B], u32 (&na)[RA_B], u32 (&oa)[RA_B], u32 (&kb)[RA_B]) {
#pragma unroll
            for (int u = 0; u < RA_B; u++) {
                const bool v = pa[u] != ~0u; const u32 pp = v ? pa[u] : 0u;
                if (small) {
                    const int src = (int)(pp & 63u); const bool hi = pp >= 64u;
                    na[u] = v ? (u32)__builtin_amdgcn_readlane((int)(hi ? dA1 : dA0), src) : 0u; oa[u] = v ? (u32)__builtin_amdgcn_readlane((int)(hi ? oA1 : oA0), src) : 0u;
                } else { const u64 kk = L.key[pp]; part(v ? ra_to(kk) : 0u, ra_type(kk), v, na[u], oa[u]); }
            }
#pragma unroll
            for (int u = 0; u < RA_B; u++) kb[u] = ent32[oa[u] + (lane < na[u] ? lane : 0u)];
        };
        auto walk = [&](const u32 (&pa)[RA_B], const u32 (&na)[RA_B], const u32 (&oa)[RA_B], const u32 (&kb)[RA_B]) {
            u32 ts[RA_B], t1[RA_B];
#pragma unroll
            for (int u = 0; u < RA_B; u++) {
                t1[u] = pa[u] != ~0u ? ra_type(L.key[pa[u] != ~0u ? pa[u] : 0]) : 0u;
                ts[u] = ra_find(L, kb[u], t1[u], lane < na[u]);
            }
#pragma unroll
            for (int u = 0; u < RA_B; u++) {
                if (pa[u] == ~0u) break;
                if (L.mk[L.slot[pa[u]]] != 1) continue;                     // (wave-uniform) eliminated by an earlier neighbour
                if (ts[u] != ~0u) L.mk[ts[u]] = 2;
                for (u32 y = lane + 64; y < na[u]; y += 64) ra_mark_one(L, ent32[oa[u] + y], t1[u]);     // (a part beyond 64 entries: rare)
                wave_sync();
            }
        };
#ifndef RA_EXP_NOMARK
        for (u32 x = 0; x < n && !fastDone; x += 64) {
            const u32 pos = x + lane;
            u64 bal = __ballot(pos < n && L.mk[L.slot[pos < n ? pos : 0]] == 1);
            if (bal == 0) continue;
            while (bal) {
                u32 pa[RA_B], na[RA_B], oa[RA_B], kb[RA_B];
                take8(bal, x, pa); fetch(pa, na, oa, kb);
                walk(pa, na, oa, kb);
            }
        }
#endif
        RA_STAMP(4);
        u32 nrm = 0, nsv = 0;
        for (u32 x0 = 0; x0 < n; x0 += 64) {
            const u32 x = x0 + lane; const bool v = x < n;
            const u64 kx = L.key[v ? x : 0]; const bool gone = v && L.mk[L.slot[v ? x : 0]] == 2;
            if (v) rm[o + (u32)(kx & 511u)] = gone ? 1 : 0;
            nrm += (u32)__popcll(__ballot(gone)); nsv += (u32)__popcll(__ballot(v && !gone && ra_to(kx) > r));
        }
        if (lane == 0) svn[w] = nsv;
        removedTotal += nrm;
        RA_STAMP(5);
    }
#ifdef RA_EXP_STAMPS
    if (CAP <= 128 && blockIdx.x == 7 && threadIdx.x == 0 && ra_reads) printf("[k_ra_mark] reads %llu mean list %.1f | cycles per read: load+clear %.0f sort %.0f table %.0f upfront %.0f walk %.0f final %.0f\n", (unsigned long long)ra_reads, (double)ra_nb / ra_reads,
        (double)ra_t[0] / ra_reads, (double)ra_t[1] / ra_reads, (double)ra_t[2] / ra_reads, (double)ra_t[3] / ra_reads, (double)ra_t[4] / ra_reads, (double)ra_t[5] / ra_reads);
#endif
    if (lane == 0 && removedTotal) atomicAdd(&counters[1], removedTotal);       // one atomic per wave, not per read
    if (lane == 0 && shortDone) atomicAdd(&counters[3], shortDone);             // (reads whose marks came from the short cut)
    if (lane == 0 && shortLists) atomicAdd(&counters[2], shortLists);           // (lists it read, the given-up attempts included)
}
__global__ void k_ra_emit(const u32* __restrict__ ids, u64 nids, const u32* __restrict__ offs, const u32* __restrict__ deg, const u64* __restrict__ ent,
                          const uint8_t* __restrict__ rm, const u32* __restrict__ svoff, EdgeCand* cand, u64 base, u64 cap) {
    const u32 lane = lane_id();
    for (u64 w = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w < nids; w += ((u64)gridDim.x * blockDim.x) >> 6) {
        const u32 r = ids[w]; const u32 n = deg[r], o = offs[r];
        u64 pos0 = base + svoff[w];
        for (u32 x0 = 0; x0 < n; x0 += 64) {
            const u32 x = x0 + lane; bool keep = false; u64 k = 0;
            if (x < n) { k = ent[o + x]; keep = rm[o + x] == 0 && ra_to(k) > r; }
            const u64 bal = __ballot(keep);
            const u64 pos = pos0 + (u64)__popcll(bal & ((1ull << lane) - 1ull));
            if (keep && pos < cap) { EdgeCand e; e.from = r; e.to = ra_to(k); e.len = ra_len(k); e.type = ra_type(k); cand[pos] = e; }
            pos0 += (u64)__popcll(bal);
        }
    }
}


// =============================================================================================
// Reduce phase with long buckets (SURVEY A.7) -- "ranked" form.  A hidden (>= 100 entries) key makes discovery one-sided: r1 may see
// r2 while r2 does not see r1, and the serial BFS (economyGraph.cpp:513-564) inserts an edge only from the read that is explored
// FIRST (:605 "still unexplored").  Three facts make most of it parallel again:
//   * a read's list only grows while the read is unexplored, so it is final and sorted (:853-871) the moment the read is explored;
//   * the edge {a,b} exists iff the earlier-explored of the two sees the other; candidates of the reciprocal pass always exist;
//   * the marks (:643-679) are a function of the final lists (every list involved is complete and nothing has been removed yet).
// So only the exploration ORDER is serial: the host walks the BFS over "potential lists" (own hits + the twins of the hits that
// point at the read, sorted once here on the device), which costs a status test per entry, hands back the ranks, and the final
// lists, the marks and the removals are the same kernels as in the symmetric case, fed with the hits that the ranks let through.
// =============================================================================================
__global__ void k_rr_widx(const u32* __restrict__ ids, u64 nids, u32* widx) { const u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (w < nids) widx[ids[w]] = (u32)w + 1; }
__global__ void k_rr_incount(const Hit* __restrict__ hits, u64 n, u32* incount) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (x >= n) return;
    const Hit h = hits[x]; if (h.from == 0 || h.len < 0) return;                 // unused slot; the -1 sentinel is never inserted (:627)
    atomicAdd(&incount[h.to], 1u);
}
__global__ void k_rr_degp(const u32* __restrict__ ids, u64 nids, const u32* __restrict__ hitcount, const u32* __restrict__ incount, u32* degp) {
    const u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (w < nids) degp[w] = hitcount[ids[w]] + incount[ids[w]];
}
// potential list of read r = slots [offp[w], +hitcount) for its own hits (by hit number) and behind them the twins of the hits pointing at r
// (the lists are built for the unresolved reads [w0, w1) at a time, so that a slice stays below 2^32 entries: offp is relative to w0)
__global__ void k_rr_fillp(const Hit* __restrict__ hits, u64 n, const u64* __restrict__ reads, int S, int uniL, const u32* __restrict__ widx, u32 w0, u32 w1, const u32* __restrict__ offp,
                           const u32* __restrict__ hitcount, u32* cursor, u64* entp) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (x >= n) return;
    const Hit h = hits[x]; if (h.from == 0) return;
    const u32 wf = widx[h.from] - 1; const bool ownIn = wf >= w0 && wf < w1;
    if (h.len < 0) { if (ownIn) entp[offp[wf - w0] + h.seq] = 0; return; }      // sorts last and is dropped
    if (ownIn) entp[offp[wf - w0] + h.seq] = ra_key(h.to, h.type, (u32)h.len);
    const u32 wt = widx[h.to] - 1; if (wt < w0 || wt >= w1) return;
    const int Lf = read_len(reads, S, h.from, uniL), Lt = read_len(reads, S, h.to, uniL);
    entp[offp[wt - w0] + hitcount[h.to] + atomicAdd(&cursor[h.to], 1u)] = ra_key(h.from, flip_type(h.type), (u32)(Lf - (Lt - h.len))) | 1ull;   // bit 0: a twin
}
// the merged lists of a slice, packed back to back (coff = exclusive scan of lenp): what goes to the host
// (the neighbour's id is replaced by its position in the locality order: that is what the host's walk indexes its tables with)
__global__ __launch_bounds__(256) void k_rr_compact(u64 nids, const u32* __restrict__ offp, const u32* __restrict__ lenp, const u32* __restrict__ coff, const u32* __restrict__ outp,
                                                   const u32* __restrict__ loc, u32* outc) {
    const u32 lane = lane_id();
    for (u64 w = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w < nids; w += ((u64)gridDim.x * blockDim.x) >> 6)
        for (u32 x = lane, n = lenp[w], o = offp[w], c = coff[w]; x < n; x += 64) { const u32 e = outp[o + x]; outc[c + x] = loc[e & 0x3FFFFFFFu] | (e & 0xC0000000u); }
}
__global__ void k_rr_unres_flag(const u32* __restrict__ order, u64 n, const uint8_t* __restrict__ status, u32* flag) { const u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (p < n) flag[p] = status[order[p]] == 0 ? 1u : 0u; }
__global__ void k_rr_unres_pick(const u32* __restrict__ order, u64 n, const u32* __restrict__ flag, const u32* __restrict__ fpos, u32* ids) { const u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (p < n && flag[p]) ids[fpos[p]] = order[p]; }
// the walk's starts: positions of the unresolved reads in ASCENDING ID order (the order in which the serial loop starts its searches, economyGraph.cpp:513)
__global__ void k_rr_start_flag(u64 N, const uint8_t* __restrict__ status, u32* flag) { const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (x < N) flag[x] = status[x + 1] == 0 ? 1u : 0u; }
__global__ void k_rr_start_pick(u64 N, const u32* __restrict__ flag, const u32* __restrict__ fpos, const u32* __restrict__ posOf, u32* out) { const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (x < N && flag[x]) out[fpos[x]] = posOf[x + 1]; }
__global__ void k_rr_rank_by_id(const u32* __restrict__ rankByPos, const u32* __restrict__ loc, u64 n, u32* rankById) {
    const u64 id = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (id < n) rankById[id] = rankByPos[loc[id]];
}
constexpr int RR_CAP = 1024;                      // own hits (connections <= 300) + as many twins
struct RrLds { u64 key[RR_CAP]; };
// output entry: to | kind << 30, kind 0 = seen from both sides (always in the list), 1 = own hit only, 2 = twin only; lenp[w] entries
__global__ __launch_bounds__(256) void k_rr_sortp(u64 nids, const u32* __restrict__ offp, const u32* __restrict__ degp, const u64* __restrict__ entp, u32* outp, u32* lenp, u64* counters) {
    __shared__ RrLds lds[4];
    RrLds& L = lds[threadIdx.x >> 6];
    const u32 lane = lane_id();
    for (u64 w = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); w < nids; w += (u64)gridDim.x * 4) {
        const u32 n = degp[w], o = offp[w];
        if (n == 0 || n > (u32)RR_CAP) { if (lane == 0) { lenp[w] = 0; if (n) atomicAdd(&counters[0], 1ull); } continue; }
        u32 P = 64; while (P < n) P <<= 1;
        wave_sync();
        for (u32 x = lane; x < P; x += 64) L.key[x] = x < n ? entp[o + x] : 0ull;
        wave_sync();
        for (u32 k = 2; k <= P; k <<= 1)
            for (u32 j = k >> 1; j > 0; j >>= 1) {
                for (u32 t = lane; t < P / 2; t += 64) {
                    const u32 i = ((t / j) * 2 * j) + (t % j), l = i + j;
                    const u64 a = L.key[i], b = L.key[l];
                    const bool desc = (i & k) == 0;
                    if (desc ? (a < b) : (a > b)) { L.key[i] = b; L.key[l] = a; }
                }
                wave_sync();
            }
        // a pair seen from both sides is there twice, twin first (bit 0 sorts it in front of the own hit): one entry, always in the list.
        // Empty keys (the -1 sentinel hits) sort last and are dropped.
        u32 base = 0;
        for (u32 x0 = 0; x0 < n; x0 += 64) {
            const u32 x = x0 + lane; const u64 kx = x < n ? L.key[x] : 0ull;
            const u64 prev = (x > 0 && x < n) ? L.key[x - 1] : 0ull, next = (x + 1 < n) ? L.key[x + 1] : 0ull;
            const bool twin = (kx & 1ull) != 0;
            const bool dupOfPrev = kx != 0 && !twin && (prev & 1ull) && (prev >> 1) == (kx >> 1);          // own hit right behind its twin: merged into it
            const bool sym = kx != 0 && twin && next != 0 && !(next & 1ull) && (next >> 1) == (kx >> 1);
            const bool keep = kx != 0 && !dupOfPrev;
            const u64 m = __ballot(keep);
            if (keep) outp[o + base + (u32)__popcll(m & ((1ull << lane) - 1ull))] = ra_to(kx) | ((sym ? 0u : (twin ? 2u : 1u)) << 30);
            base += (u32)__popcll(m);
        }
        if (lane == 0) lenp[w] = base;
    }
}
// final lists: a hit enters (both directed entries) iff its source was explored before its target
__global__ void k_rr_degree_h(const Hit* __restrict__ hits, u64 n, const u32* __restrict__ rank, u32* deg, u64* counters) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    bool in = false;
    if (x < n) { const Hit h = hits[x]; in = h.from != 0 && h.len >= 0 && rank[h.from] < rank[h.to]; if (in) { atomicAdd(&deg[h.from], 1u); atomicAdd(&deg[h.to], 1u); } }
    const u64 m = __ballot(in);
    if (lane_id() == 0 && m) atomicAdd((unsigned long long*)&counters[2], (unsigned long long)__popcll(m));
}
__global__ void k_rr_fill_h(const Hit* __restrict__ hits, u64 n, const u32* __restrict__ rank, const u64* __restrict__ reads, int S, int uniL, const u32* __restrict__ offs, u32* cursor, u64* ent, u32* ent32) {
    const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (x >= n) return;
    const Hit h = hits[x]; if (h.from == 0 || h.len < 0 || !(rank[h.from] < rank[h.to])) return;
    const int Lf = read_len(reads, S, h.from, uniL), Lt = read_len(reads, S, h.to, uniL);
    ra_put(ent, ent32, (u64)offs[h.from] + atomicAdd(&cursor[h.from], 1u), h.to, h.type, (u32)h.len);
    ra_put(ent, ent32, (u64)offs[h.to] + atomicAdd(&cursor[h.to], 1u), h.from, flip_type(h.type), (u32)(Lf - (Lt - h.len)));      // the twin (economyGraph.cpp:821)
}

// A list beyond RA_CAP entries (a read next to a high-copy repeat that thousands of reads see): the same marking with the sorted list
// and the node table in global scratch, one wavefront per read.  scratch of the b-th heavy read at scr[b] (u64 units): key[P] u64, then
// ht[4P] u32, then mk[4P] u32 (P = list length rounded up to a power of two).  All scratch traffic goes through device-scope atomics
// (plain loads could be served from a stale L1 line after another lane's store).
__device__ __forceinline__ u32 g_ld(const u32* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void g_st(u32* p, u32 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u64 g_ld(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void g_st(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u32 ra_big_find(const u32* ht, u32 mask, int shift, u32 id) {                 // slot of `id`, or of the first empty slot
    u32 s = (id * 2654435761u) >> shift;
    for (;;) { const u32 v = g_ld(&ht[s]); if (v == 0 || v == id) return s; s = (s + 1) & mask; }
}
__global__ __launch_bounds__(64) void k_ra_mark_big(const u32* __restrict__ ids, const u32* __restrict__ heavy, const u64* __restrict__ scr, u64* scratch,
                                                    const u32* __restrict__ offs, const u32* __restrict__ deg, const u64* __restrict__ ent, uint8_t* rm, u32* svn, u64* counters) {
    const u32 lane = lane_id(), w = heavy[blockIdx.x], r = ids[w], n = deg[r], o = offs[r];
    u32 P = 64; int bits = 6; while (P < n) { P <<= 1; bits++; }
    const u32 HT = 4 * P, mask = HT - 1; const int shift = 32 - (bits + 2);
    u64* key = scratch + scr[blockIdx.x]; u32* ht = (u32*)(key + P); u32* mk = ht + HT;
    for (u32 x = lane; x < P; x += 64) g_st(&key[x], x < n ? ent[o + x] : 0ull);
    for (u32 x = lane; x < HT; x += 64) { g_st(&ht[x], 0u); g_st(&mk[x], 0u); }
    __threadfence(); wave_sync();
    for (u32 k = 2; k <= P; k <<= 1)                                             // bitonic sort, descending: (len, id, type) as in compareEdges (:853-871)
        for (u32 j = k >> 1; j > 0; j >>= 1) {
            for (u32 t = lane; t < P / 2; t += 64) {
                const u32 i = ((t / j) * 2 * j) + (t % j), l = i + j;
                const u64 a = g_ld(&key[i]), b = g_ld(&key[l]);
                if (((i & k) == 0) ? (a < b) : (a > b)) { g_st(&key[i], b); g_st(&key[l], a); }
            }
            __threadfence(); wave_sync();
        }
    for (u32 x = lane; x < n; x += 64) {
        const u32 id = ra_to(g_ld(&key[x])); u32 s = (id * 2654435761u) >> shift;
        for (;;) { const u32 old = atomicCAS(&ht[s], 0u, id); if (old == 0 || old == id) break; s = (s + 1) & mask; }
        g_st(&mk[s], 1u);
    }
    __threadfence(); wave_sync();
    for (u32 x = 0; x < n; x++) {                                                // markTransitiveEdge (:643-679), sequential over the sorted list
        const u64 kx = g_ld(&key[x]); const u32 a = ra_to(kx);
        if (g_ld(&mk[ra_big_find(ht, mask, shift, a)]) != 1) continue;           // (wave-uniform)
        const u32 t1 = ra_type(kx), na = deg[a], oa = offs[a];
        for (u32 y = lane; y < na; y += 64) {
            const u64 kb = ent[oa + y]; const u32 b = ra_to(kb), t2 = ra_type(kb);
            const bool compat = ((t1 == 0 || t1 == 2) && (t2 == 0 || t2 == 1)) || ((t1 == 1 || t1 == 3) && (t2 == 2 || t2 == 3));
            if (!compat) continue;
            const u32 s = ra_big_find(ht, mask, shift, b);
            if (g_ld(&ht[s]) == b && g_ld(&mk[s]) == 1) g_st(&mk[s], 2u);
        }
        __threadfence(); wave_sync();
    }
    u32 nrm = 0, nsv = 0;
    for (u32 x = lane; x < n; x += 64) {
        const u64 kx = ent[o + x]; const bool gone = g_ld(&mk[ra_big_find(ht, mask, shift, ra_to(kx))]) == 2;
        rm[o + x] = gone ? 1 : 0; nrm += gone; nsv += (!gone && ra_to(kx) > r);
    }
    for (int dlt = 32; dlt; dlt >>= 1) { nrm += __shfl_xor(nrm, dlt); nsv += __shfl_xor(nsv, dlt); }
    if (lane == 0) { svn[w] = nsv; if (nrm) atomicAdd((unsigned long long*)&counters[1], (unsigned long long)nrm); }
}
__global__ void k_ra_heavy_sizes(const u32* __restrict__ heavy, u32 n, const u32* __restrict__ ids, const u32* __restrict__ deg, u32* out) {
    const u32 b = blockIdx.x * blockDim.x + threadIdx.x; if (b < n) out[b] = deg[ids[heavy[b]]];
}
