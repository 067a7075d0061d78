// sage2_amd/csrc/sage2ov_device.hip -- hand-written HIP kernels for gfx950 (MI355X) and their launchers.
//
// The kernels live in kernels_*.inc (one file per phase of the path, included below in dependency order: common helpers,
// locality order, step 1, index build, scan, sequential probe, fast probe, reciprocal pass, device reduce, convert); this file
// holds the device state, the workspace arena and the host-side launchers.
// Integer / bit / index work only (no MFMA): everything here is bound by HBM gathers.  Design notes
// (layouts, algorithmic bytes, rooflines) are in DESIGN.md; reference citations are relative to the
// SAGE2 tree.  Wavefront = 64 lanes everywhere; one wavefront owns one read in the probe kernel.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>
#include <chrono>
#include <memory>
#include <atomic>
#include <thread>
#include <sched.h>
#include <pthread.h>
#include <sys/mman.h>
#include "sage2ov.h"
#include "sage2ov_internal.h"

namespace s2 {

#define HIPCHK(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            char b_[512];                                                                              \
            snprintf(b_, sizeof b_, "%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            err = b_;                                                                                  \
            return SAGE2OV_ERR_DEVICE;                                                                 \
        }                                                                                              \
    } while (0)

typedef unsigned long long u64;
typedef unsigned int u32;

enum { WS_SLOTS, WS_WHERE, WS_BIG, WS_CSR, WS_SLOW, WS_NEED, WS_CURSOR, WS_KEYS, WS_KEEP, WS_OWNER, WS_FINAL,
       WS_PARTIAL, WS_IDS, WS_NEAR, WS_HITS, WS_MINH, WS_OCUR, WS_MI1, WS_KREC, WS_RA_DEG, WS_RA_OFF, WS_RA_CUR, WS_RA_ENT, WS_RA_RM, WS_ORG_POOL, WS_ORG_OFF, WS_ORG_LEN, WS_ORG_IMG, WS_ORG_K0, WS_ORG_K1, WS_ORG_V0, WS_ORG_V1, WS_ORG_HIST, WS_ORG_HSCAN, WS_ORG_FLAG, WS_ORG_UID, WS_ORG_HEAD, WS_RR_IN, WS_RR_DEGP, WS_RR_OFFP, WS_RR_ENTP, WS_RR_OUTP, WS_RR_WIDX, WS_RR_RANK, WS_RR_CUR, WS_RA_HEAVY, WS_RA_HSIZE, WS_RA_HSCR, WS_RR_LEN, WS_RR_COFF, WS_RR_OUTC,
       WS_PT_K0, WS_PT_K1, WS_PT_CNT, WS_PT_BASE, WS_PT_OFF, WS_PT_GOFF, WS_RR_RANKL, WS_LOC_READS, WS_LOC_IDOF, WS_LOC_POSOF, WS_LOC_STATUS, WS_ORG_GFLAG, WS_ORG_GPOS, WS_LOC_META, WS_SLOW2, WS_RA_ENT32, WS_RA_SPLIT, WS_PRE_BASE, WS_PRE_NONE, WS_COUNT };   // ids of the workspace arena (Device::ws)
// Bases of the device counters (Device::d_counters, u64 words): who owns the words from each base on, how many, what each holds.  A kernel that is handed
// d_counters + base indexes from that base; the probe kernels are handed d_counters itself (ProbeArgs::counters) and use the CTR_HIT_* / CTR_HANDED names.
// Slots that two phases use in turn, never at once: CTR_LIST is CTR_HIT_REAL (a list is collected before or after the hit lists, not during them);
// CTR_INDEX, CTR_RANKED and CTR_MARKS share base 9 (index build, then within one reduce the ranked lists, read back and zeroed before the marks);
// the last two words of CTR_INDEX are the first two of CTR_ORG (step 1 is over when the index build starts);
// dev_reciprocal zeroes the 9 words from CTR_RECIP, the probe's four with them (the probe pass is over by then).
enum {
    CTR_RECIP = 0,        // reciprocal pass, 5 words: [0] cursor of the candidate list, [1] verified overlaps, [2] contained reads, [3] their summed size,
                          //   [4] unresolved reads (status 0): what collect_unresolved sizes its list by
    CTR_HIT_CURSOR = 5,   // probe kernels that write hits, 1 word: cursor in the Hit buffer (may pass the capacity: nothing is written beyond it)
    CTR_HIT_REAL = 6,     // fast kernel's hit-list form, 1 word: real hits among the chunks it took
    CTR_LIST = 6,         // cursor of a collected list, 1 word: k_red_unresolved, k_red_collect, k_red_collect_few (in turn with CTR_HIT_REAL)
    CTR_HANDED = 7,       // fast kernel, 2 words: [0] reads handed on to the next pass (the slow list), [1] of them: more candidates than the form has slots
    CTR_INDEX = 9,        // index build, 10 words: [0] csr entries, [1] keys, [2] long buckets, [3] impure long buckets, [4] pure ones, [5] group records, [6] groups,
                          //   [7] group windows given up, [8] failures (windows overflowed | keys beyond the count field << 20 | heavy windows without scratch << 40), [9] scratch cursor
    CTR_RANKED = 9,       // reduce phase, ranked lists, 4 words: [2] hits present in the final lists (k_rr_degree_h), [3] potential lists beyond RR_CAP (k_rr_sortp); [0], [1] unused
    CTR_MARKS = 9,        // reduce phase, marks, 5 words: [0] lists beyond RA_CAP, [1] removed entries, [2] lists the short cut read, [3] reads it settled, [4] reads listed for the second launch
    CTR_ORG = 17,         // step 1's ASCII front end (k_org_classify), 6 words: [0] longest good read, [1] good reads, [2] their bases, [3] reads not longer than
                          //   the minimum overlap, [4] shortest good read, [5] reads beyond the length limit
    CTR_FILTER = 23,      // reduce phase, pre-hits filter (k_hits_filter), 2 words: [0] kept hits, [1] unresolved reads without written hits
    CTR_RUNSTARTS = 25,   // locality order (k_loc_index), 64 words: run starts, spread over 64 words (Device::d_runStarts)
    CTR_RUNSTATS = 25 + 64,   // fast kernel, run mode, 4 words: [0] reads answered off the ring, [1] steps, [2] of those reads: records computed with a lane per read, [3] such steps
                          //   (zeroed by dev_probe, summed over its launches; read back on request only: dev_probe_run_stats)
    CTR_WORDS = 25 + 64 + 4   // what dev_create allocates
};
static_assert(CTR_RECIP + 5 <= CTR_HIT_CURSOR && CTR_HIT_CURSOR + 1 <= CTR_HIT_REAL && CTR_HIT_REAL + 1 <= CTR_HANDED && CTR_RECIP + 9 <= CTR_INDEX && CTR_HANDED + 2 <= CTR_INDEX && CTR_INDEX + 10 <= CTR_FILTER && CTR_MARKS + 5 <= CTR_ORG && CTR_ORG + 6 <= CTR_FILTER &&
              CTR_FILTER + 2 <= CTR_RUNSTARTS && CTR_RUNSTARTS + 64 <= CTR_RUNSTATS && CTR_RUNSTATS + 4 <= CTR_WORDS, "a counter group runs into the next one, or past the allocation");
struct MateLib { u64* key = nullptr; u64* cnt = nullptr; u64* first = nullptr; u64 n = 0; };      // one library's mate table: sorted by key, unique (kernels_mates.inc)
struct Mates { MateLib lib[128]; u64* pkey = nullptr; u64* pord = nullptr; u64 pn = 0, pcap = 0; };   // + the pending records of the call in progress (keys, record ordinals)
struct Device {
    int ordinal = 0;
    Options opt;                 // the environment switches, as the context read them when it was created (sage2ov_internal.h)
    hipStream_t stream = nullptr;
    hipEvent_t ev[8] = {};
    // reads
    u64 N = 0; int S = 0, maxL = 0, k = 0, h = 0; double probeShare = 1.0;
    u64* d_runStarts = nullptr; u64* h_runStarts = nullptr; hipEvent_t evRunStarts = nullptr; bool runStartsValid = false; double runStartFrac = 0.0;      // share of the reads without a predecessor in the locality order (counted by k_loc_index into d_runStarts)
    u64* reads = nullptr;        // (N+1)*S words, slot i = read id i
    Mates* mates = nullptr;      // the mate-pair table (dev_mates_add): allocations of its own, dropped with the read set
    // pairing (dev_organize_reads(..., pairing)): +-id of the pairN staged reads -- pairRaw: of the pairN raw records of the ASCII route, 0 for one
    // that was not staged --, an allocation of its own, dropped by dev_pairing_release and with the read set
    int* pairId = nullptr; u64 pairN = 0; bool pairRaw = false, pairValid = false;
    void* readmap = nullptr;     // the read-to-edge table, the mate flags and the distances (dev_readmap_build; ReadMap): allocations of its own, dropped with the graph and the read set
    u32* findDir = nullptr; int findDirBits = 0;      // read-id lookup (dev_find_ids): first id per value of the top bits of word 0, built by the first call, dropped with the read set
    // the same reads in LOCALITY order (slot p = the read at position p of the order by global minimiser): what the index entries point at and
    // what the probe kernels gather from -- a read's overlap partners are neighbours in the genome, hence (mostly) neighbours here
    u64* readsLoc = nullptr; u32* idOf = nullptr; u32* posOf = nullptr; uint8_t* statusP = nullptr; unsigned short* metaP = nullptr;
    // index
    u64 T = 0; u64* slots = nullptr; u32* csr = nullptr; u64 n_csr = 0; u64 seed = 0x5A6E2D0Full;
    u64 n_keys = 0, n_long = 0;
    u64* mi1 = nullptr; u64 TL = 0; u64* krec = nullptr; u64 n_groups = 0;      // minimiser index (fast kernel)
    int uniL = 0;                                                                // the common read length when all reads have one (else 0): no length gathers
    // per-read results
    u64* right = nullptr; u64* left = nullptr; u32* conn = nullptr; u32* cflag = nullptr; uint8_t* status = nullptr;
    // The status of the reciprocal pass: statusP (by position) is what k_recip_cond writes and is authoritative from then on; status (by id) follows it when a
    // by-id reader asks (ensure_status_by_id), or at once on the eager route.  statusByIdValid: the two agree.  statusGen: stamps the statuses (bumped by
    // dev_reciprocal and by everything else that writes one); nUnres: the status-0 reads k_recip_cond counted; unresGen: the statusGen whose unresolved reads
    // WS_IDS lists (nUnres of them, any order), 0 when it lists nothing of the kind.
    bool statusByIdValid = true; u64 statusGen = 1, nUnres = 0, unresGen = 0;
    // edge candidates
    EdgeCand* cand = nullptr; u64 cand_cap = 0; u64* d_counters = nullptr;  // CTR_WORDS words: see the CTR_ enum
    u64 n_cand = 0;
    // final edges (device resident)
    FinalEdge* final_edges = nullptr; u64 n_final = 0;
    DevTimings tm;
    u64 memLow = ~0ull;          // lowest free device memory seen at the sampling points (mem_sample)
    // Memory-diet mode (round 3, BASELINE configs[4]: a billion reads per GPU): transient buffers are released at the end of their phase instead of kept for
    // the next step, the id-ordered read store is released once the locality-ordered one exists (uniform read length only; rebuilt for the next index
    // build), no minimiser groups, the per-read result arrays and the candidate list are allocated when they are first needed.  On when the whole
    // footprint of the default mode (~640 bytes per read) would pass 70 % of the device's memory, or SAGE2OV_MEMORY_DIET=1 (0 forbids it).
    bool diet = false;
    // hits written out by the initial pass (k_probe_fast<..., TAIL = 2> on noisy data, one context probing everything): the reduce phase filters them
    struct PreHits { bool valid = false; Hit* hits = nullptr; u64 cap = 0, used = 0; u64* base = nullptr; } pre;
    void* support = nullptr;     // the mate-pair supports of edge pairs (dev_support_build; Support): allocations of its own, dropped with the read-to-edge table and the mate flags
    void* contigs = nullptr;     // the contig table and the spelling buffers (dev_contigs_build; Contigs): allocations of its own, dropped with the graph and the read set
    void* links = nullptr;       // the scaffold links of half-edge pairs (dev_links_build; Links): allocations of its own, dropped with the read-to-edge table and the mate flags
    void* paths = nullptr;       // the path supports of half-edge pairs (dev_paths_build; PathTable): allocations of its own, dropped with the mate-pair supports
    void* estflags = nullptr;    // every library's mate flags as of the last estimate (dev_estflags_keep; EstFlags): they outlive the read-to-edge table and go with the graph and the read set
    void* copycount = nullptr;   // step 5 around its solver (dev_copycount_prepare, dev_flownet_build; CopyCount): allocations of its own, dropped with the graph and the read set
    void* s4keep = nullptr;      // step 4: the simplified graph stays in HBM until the next call (S4Keep)
    // step 4: blocks a call released, kept for the next call (it asks for the same ~50 sizes; fresh HBM costs ~50 ms per GB to map, 0.7 s per call at BASELINE
    // configs[2]).  Emptied when the read set changes, when the workspace arena runs out of memory, and never filled in memory-diet mode.
    std::vector<std::pair<void*, size_t>> s4cache;
    u64 reduceStats[SAGE2OV_REDUCE_STATS] = {0};   // which way the last dev_reduce_device went (dev_reduce_stats; the layout of sage2ov_reduce_stats_get)
    void* rrStaging = nullptr;   // ranked reduce: the pinned 2 MB-page host buffers the potential lists are downloaded into, kept from step to step (RrStaging)
    // workspace arena: buffers of the timed path are allocated once and only ever grow (no hipMalloc/hipFree per step)
    struct Buf { void* p = nullptr; size_t cap = 0; u32 epoch = 0; };
    Buf ws[WS_COUNT];
    // MEMORY-DIET MODE (read sets that fill the HBM): the index build's sort buffers and the results of a step (records, candidates, final edges, convert's sort buffers)
    // take turns with the memory.  Until round 4 each side was hipFree'd when the other one came and hipMalloc'ed again a step later -- 3.4 of the 3.7 s of an index build
    // at 1.02 G reads, and erratic (tools/ubench/mempool.hip: the same 80 GB come back in 0.5 ms or in 5 s depending on their shape).  Now both sides are CARVED out of one
    // block that stays: phase A = the index build, phase B = everything from the probe pass to the next build; a phase starts with an empty block (ph_begin: the callers
    // have synchronised the stream, as they did in front of hipFree).  The first step sizes the block (what does not fit yet gets blocks of its own for that phase);
    // from the second step on nothing is allocated.
    struct Phase { char* blk = nullptr; size_t cap = 0, used = 0, virt = 0, need = 0; u32 epoch = 1; std::vector<void*> overflow; } ph;
    bool resCarved = false;      // right / left / conn / cflag / status / cand point into the phase block (diet mode): never hipFree'd
};
static void s4cache_release(Device* d) { for (auto& c : d->s4cache) hipFree(c.first); d->s4cache.clear(); }
static bool ws_phased(int id);
static void* ph_carve(Device* d, size_t bytes);
static void* ws_get(Device* d, int id, size_t bytes) {
    Device::Buf& b = d->ws[id];
    if (d->diet && ws_phased(id)) {
        if (b.p && b.epoch == d->ph.epoch && b.cap >= bytes) return b.p;
        if (b.p && !b.epoch) { hipFree(b.p); }                                 // (allocated before the context went on the diet)
        b.p = ph_carve(d, bytes + 256); b.cap = b.p ? bytes + 256 : 0; b.epoch = b.p ? d->ph.epoch : 0;
        return b.p;
    }
    if (b.epoch) { b.p = nullptr; b.cap = 0; b.epoch = 0; }                   // (a carved piece from an earlier diet: not ours to free)
    if (b.cap < bytes || !b.p) {
        if (b.p) hipFree(b.p);
        b.p = nullptr; b.cap = 0;
        size_t want = d->diet ? bytes + 256 : bytes + bytes / 16 + 256;        // (grow-only arena: 6 % of slack saves re-allocations; none when memory is what is short)
        if (hipMalloc(&b.p, want) != hipSuccess) {
            (void)hipGetLastError(); b.p = nullptr;
            if (d->s4cache.empty()) return nullptr;
            s4cache_release(d);                                                       // (step 4's spare blocks go first)
            if (hipMalloc(&b.p, want) != hipSuccess) { b.p = nullptr; return nullptr; }
        }
        b.cap = want;
    }
    return b.p;
}
// workspace ids that live in the phase block in diet mode (see Device::Phase)
static bool ws_phased(int id) {
    switch (id) { case WS_PT_K0: case WS_PT_K1: case WS_WHERE: case WS_MINH: case WS_OCUR: case WS_PT_CNT: case WS_PT_BASE: case WS_PARTIAL: case WS_PT_OFF:
                  case WS_KEYS: case WS_KEEP: case WS_FINAL: case WS_SLOW: case WS_SLOW2: return true; default: return false; }
}
static void* ph_carve(Device* d, size_t bytes) {
    Device::Phase& P = d->ph;
    const size_t a = (P.virt + 255) & ~(size_t)255; P.virt = a + bytes; P.need = std::max(P.need, P.virt);
    const size_t off = (P.used + 255) & ~(size_t)255;
    if (P.blk && off + bytes <= P.cap) { P.used = off + bytes; return P.blk + off; }
    void* p = nullptr;                                                     // (first step, or a phase that outgrew the block: a block of its own until the phase ends)
    if (hipMalloc(&p, std::max<size_t>(bytes, 256)) != hipSuccess) {
        (void)hipGetLastError(); s4cache_release(d);
        if (P.blk && P.used == 0) { hipFree(P.blk); P.blk = nullptr; P.cap = 0; }      // (a block too small for this phase and not in use yet stands in the way)
        if (hipMalloc(&p, std::max<size_t>(bytes, 256)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    }
    P.overflow.push_back(p);
    return p;
}
// a new phase: everything carved so far is dead (the caller has synchronised the stream); the block grows to what the largest phase so far needed
static void ph_begin(Device* d, bool mayGrow = true) {
    Device::Phase& P = d->ph;
    for (void* p : P.overflow) hipFree(p);
    P.overflow.clear();
    if (mayGrow && P.need > P.cap) { if (P.blk) hipFree(P.blk); P.blk = nullptr; P.cap = 0; const size_t want = P.need + P.need / 64 + 4096; void* p = nullptr;
                          if (hipMalloc(&p, want) == hipSuccess) { P.blk = (char*)p; P.cap = want; } else (void)hipGetLastError(); }
    P.used = 0; P.virt = 0; P.epoch++;
    for (int id = 0; id < WS_COUNT; id++) if (ws_phased(id)) { Device::Buf& b = d->ws[id]; if (b.epoch) { b.p = nullptr; b.cap = 0; b.epoch = 0; } }
    if (d->resCarved) { d->right = d->left = nullptr; d->conn = d->cflag = nullptr; d->status = nullptr; d->cand = nullptr; d->cand_cap = 0; d->n_cand = 0; d->resCarved = false; }
    d->final_edges = nullptr; d->n_final = 0;
}
static void ph_release(Device* d) {
    Device::Phase& P = d->ph;
    for (void* p : P.overflow) hipFree(p);
    P.overflow.clear(); if (P.blk) hipFree(P.blk); P.blk = nullptr; P.cap = P.used = P.virt = P.need = 0; P.epoch++;
    for (int id = 0; id < WS_COUNT; id++) { Device::Buf& b = d->ws[id]; if (b.epoch) { b.p = nullptr; b.cap = 0; b.epoch = 0; } }
    if (d->resCarved) { d->right = d->left = nullptr; d->conn = d->cflag = nullptr; d->status = nullptr; d->cand = nullptr; d->cand_cap = 0; d->resCarved = false; }
}
static void ws_free(Device* d, int id) { Device::Buf& b = d->ws[id]; if (b.epoch) return;      // (carved: it goes with its phase)
                                         if (b.p) hipFree(b.p); b.p = nullptr; b.cap = 0; }
// the edge candidates: a block of their own, or a piece of the phase block in diet mode (then the old piece is simply left behind)
static int cand_resize(Device* d, u64 ncap, u64 keep, std::string& err) {
    EdgeCand* nc = nullptr;
    if (d->diet) { nc = (EdgeCand*)ph_carve(d, ncap * sizeof(EdgeCand)); if (!nc) { err = "edge candidates: out of device memory"; return SAGE2OV_ERR_NOMEM; } }
    else HIPCHK(hipMalloc(&nc, ncap * sizeof(EdgeCand)));
    if (keep && d->cand) { HIPCHK(hipMemcpyAsync(nc, d->cand, keep * sizeof(EdgeCand), hipMemcpyDeviceToDevice, d->stream)); HIPCHK(hipStreamSynchronize(d->stream)); }
    if (d->cand && !d->resCarved) hipFree(d->cand);
    d->cand = nc; d->cand_cap = ncap; if (d->diet) d->resCarved = true;
    return 0;
}
static void decide_diet(Device* d) {
    size_t fr = 0, to = 0; d->diet = false;
    if (hipMemGetInfo(&fr, &to) == hipSuccess && to) d->diet = (double)(d->N + 1) * 640.0 > 0.7 * (double)to;
    if (const char* ev = d->opt.get("SAGE2OV_MEMORY_DIET")) d->diet = atoi(ev) != 0;
}
static void mem_sample(Device* d) { size_t fr = 0, to = 0; if (hipMemGetInfo(&fr, &to) == hipSuccess) d->memLow = std::min<u64>(d->memLow, (u64)fr); }
#define WS(var, type, id, count)                                                                     \
    type* var = (type*)ws_get(d, id, (size_t)(count) * sizeof(type));                                \
    if (!var) { err = std::string("workspace allocation failed: ") + #id; return SAGE2OV_ERR_NOMEM; }

#include "kernels_common.inc"
#include "kernels_order.inc"
#include "kernels_organize.inc"
#include "kernels_partition.inc"
#include "kernels_index.inc"
#include "kernels_scan.inc"
#include "kernels_probe_seq.inc"
#include "kernels_probe_fast.inc"
#include "kernels_reciprocal.inc"
#include "kernels_reduce.inc"
#include "kernels_convert.inc"
#include "kernels_simplify.inc"
#include "kernels_splice.inc"
#include "kernels_find.inc"
#include "kernels_mates.inc"
#include "kernels_readmap.inc"
#include "kernels_support.inc"
#include "kernels_links.inc"
#include "kernels_paths.inc"
#include "kernels_contig.inc"
#include "kernels_scaffold.inc"
#include "kernels_copycount.inc"
#include "kernels_flow.inc"

// =============================================================================================
// host primitives: what the launchers below share (grids, counters, transient buffers, a stream timer, scan, radix sort, heads)
// =============================================================================================
// one thread per item.  A launch of 2^32 threads or more does NOT fail on this runtime: its size is taken modulo 2^32 and the tail of the work silently
// never runs (round 3, 1.02 G reads).  grid_for is therefore only for item counts that the documented limits keep below 2^32 (asserted in debug
// builds by the limit checks of the callers: reads < 2^30, tuples < 2^32); kernels whose item count can pass it are grid-stride and use grid_for_capped.
static inline unsigned grid_for(u64 n, unsigned block) { return (unsigned)std::max<u64>(1, (n + block - 1) / block); }
static inline unsigned grid_for_capped(u64 n, unsigned block) { return (unsigned)std::max<u64>(1, std::min<u64>((n + block - 1) / block, ((1ull << 32) / block) - 1)); }
// out[0, n) = d_counters[first, first + n), once the stream has finished (first: a CTR_ base)
static int read_counters(Device* d, int first, int n, u64* out, std::string& err) {
    HIPCHK(hipMemcpyAsync(out, d->d_counters + first, n * sizeof(u64), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}
// Transient device buffers of one call, freed on every return path.  get: a buffer of its own (null: out of memory); slot: a numbered buffer, reused by the
// next request that fits into it (the chunks of one call); release: freed early; keep: the caller takes it over.
struct DevTmp {
    static constexpr int SLOTS = 8;
    std::vector<void*> own; struct { void* p = nullptr; size_t cap = 0; } slots[SLOTS];
    ~DevTmp() { for (void* q : own) hipFree(q); for (auto& b : slots) hipFree(b.p); }
    static void* alloc(size_t bytes) { void* q = nullptr; if (hipMalloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; } return q; }
    template <class T> T* get(u64 n) { void* q = alloc(std::max<u64>(n, 1) * sizeof(T)); if (q) own.push_back(q); return (T*)q; }
    template <class T> T* slot(int i, u64 n) { if (i < 0 || i >= SLOTS) return nullptr;
                                               auto& b = slots[i]; const size_t bytes = n * sizeof(T);
                                               if (!b.p || b.cap < bytes) { hipFree(b.p); b.p = alloc(bytes); b.cap = b.p ? bytes : 0; } return (T*)b.p; }
    void release(void* q) { for (void*& x : own) if (x == q) { hipFree(q); x = nullptr; } }
    void keep(void* q) { for (void*& x : own) if (x == q) x = nullptr; }
};
// HIP-event time of a stretch of the stream, added up in milliseconds: start, then stop (which synchronises) -- or end, and add once the caller has synchronised
struct StreamLap {
    hipEvent_t a = nullptr, b = nullptr; hipStream_t st;
    explicit StreamLap(hipStream_t s) : st(s) {}
    ~StreamLap() { if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); }
    hipError_t create() { const hipError_t e = hipEventCreate(&a); return e != hipSuccess ? e : hipEventCreate(&b); }
    hipError_t start() { return hipEventRecord(a, st); }
    hipError_t end() { return hipEventRecord(b, st); }
    void add(double& acc) const { float ms = 0; hipEventElapsedTime(&ms, a, b); acc += ms; }
    hipError_t stop(double& acc) { hipError_t e = end(); if (e == hipSuccess) e = hipStreamSynchronize(st); if (e == hipSuccess) add(acc); return e; }
};
// Exclusive scan of n u32 (kernels_scan.inc); partial: scan_partial_words(n) words.  total null: nothing is read back, nothing is synchronised; else the sum
// of the input comes back and the stream has finished.  n = 0: no block to launch, the total is 0.
static inline u64 scan_partial_words(u64 n) { return n / SCAN_BLOCK + 2; }
// for the callers that rank inside a block themselves (k_conv_emit): partial[b] = sum of the items in front of block b (SCAN_BLOCK items each), partial[nb] = the
// sum of all; returns nb
static u64 scan_block_sums(Device* d, const u32* in, u64 n, u64* partial) {
    const u64 nb = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
    if (nb) hipLaunchKernelGGL((k_scan_reduce<SCAN_ITEMS, SCAN_THREADS>), dim3((unsigned)nb), dim3(SCAN_THREADS), 0, d->stream, in, (u64)n, partial);
    hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(1024), 0, d->stream, partial, (u64)nb, partial + nb);
    return nb;
}
// two launches while every block can add up the sums of the blocks in front of it by itself, three (one block scans the sums in between) beyond
static int scan_u32(Device* d, const u32* in, u64 n, u32* out, u64* partial, u64* total, std::string& err) {
    const u64 nb = (n + SCAN2_BLOCK - 1) / SCAN2_BLOCK;
    if (nb) hipLaunchKernelGGL((k_scan_reduce<SCAN2_ITEMS, SCAN2_THREADS>), dim3((unsigned)nb), dim3(SCAN2_THREADS), 0, d->stream, in, (u64)n, partial);
    // (SAGE2OV_TEST_SCAN_DIRECT_BLOCKS=<b>: the bound, lowered -- tests: both forms and the step between them on a few thousand items)
    const u64 directMax = (u64)std::min<long long>(SCAN_DIRECT_MAX_BLOCKS, std::max<long long>(0, d->opt.num("SAGE2OV_TEST_SCAN_DIRECT_BLOCKS", SCAN_DIRECT_MAX_BLOCKS)));
    if (nb && nb <= directMax) hipLaunchKernelGGL((k_scan_final<SCAN2_ITEMS, SCAN2_THREADS, true>), dim3((unsigned)nb), dim3(SCAN2_THREADS), 0, d->stream, in, (u64)n, partial, out, partial + nb);
    else {
        hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(1024), 0, d->stream, partial, (u64)nb, partial + nb);
        if (nb) hipLaunchKernelGGL((k_scan_final<SCAN2_ITEMS, SCAN2_THREADS, false>), dim3((unsigned)nb), dim3(SCAN2_THREADS), 0, d->stream, in, (u64)n, partial, out, partial + nb);
    }
    HIPCHK(hipGetLastError());
    if (total) { HIPCHK(hipMemcpyAsync(total, partial + nb, sizeof(u64), hipMemcpyDeviceToHost, d->stream)); HIPCHK(hipStreamSynchronize(d->stream)); }
    return 0;
}
// the steps' form: the partial sums in the workspace arena (which the mate table never touches: it brings a buffer of its own)
static int scan_u32(Device* d, const u32* in, u64 n, u32* out, u64* total, std::string& err) { WS(partial, u64, WS_PARTIAL, scan_partial_words(n)); return scan_u32(d, in, n, out, partial, total, err); }
// Stable LSD radix sort of n > 0 (u64 key, u32 value) pairs by the 8-bit digits at shifts[0, np): k_rs_hist, scan, k_rs_scatter per digit (kernels_organize.inc).
// The pairs are in k[0] / v[0]; every pass writes the other side, *side = the one that holds the result.  hist, hscan: rs_hist_words(n) words each, partial:
// scan_partial_words of as many.  Nothing is synchronised.
struct RsBufs { u64* k[2]; u32* v[2]; u32 *hist, *hscan; u64* partial; };
constexpr int RS_ALL_DIGITS[] = {0, 8, 16, 24, 32, 40, 48, 56}; constexpr int RS_ALL_N = sizeof RS_ALL_DIGITS / sizeof RS_ALL_DIGITS[0];
static inline u64 rs_hist_words(u64 n) { return 256 * ((n + RS_TILE - 1) / RS_TILE) + 2; }
static int radix_sort_pairs(Device* d, const RsBufs& B, u64 n, const int* shifts, int np, int* side, std::string& err) {
    const u32 nb = (u32)((n + RS_TILE - 1) / RS_TILE); int cur = 0;
    for (int p = 0; p < np; p++, cur ^= 1) {
        hipLaunchKernelGGL(k_rs_hist, dim3(nb), dim3(64), 0, d->stream, B.k[cur], (u64)n, shifts[p], B.hist, nb);
        const int rc = scan_u32(d, B.hist, (u64)256 * nb, B.hscan, B.partial, nullptr, err); if (rc) return rc;
        hipLaunchKernelGGL(k_rs_scatter, dim3(nb), dim3(64), 0, d->stream, B.k[cur], B.v[cur], (u64)n, shifts[p], B.hscan, nb, B.k[cur ^ 1], B.v[cur ^ 1]);
    }
    HIPCHK(hipGetLastError());
    *side = cur; return 0;
}
// Heads to positions, second half: flag[i] = 1 where a run begins among n sorted items (the caller's predicate), pos = exclusive scan of the flags and E its total
// (scan_u32 with a read-back: the caller sizes hp, E + 1 words, by it); then hp[e] = position of head e and hp[E] = n (k_headpos)
static int head_positions(Device* d, const u32* flag, const u32* pos, u64 n, u32* hp, u64 E, std::string& err) {
    hipLaunchKernelGGL(k_headpos, dim3(grid_for(n, 256)), dim3(256), 0, d->stream, flag, pos, (u64)n, hp, (u64)E);
    HIPCHK(hipGetLastError());
    return 0;
}
// Host buffers on 2 MB pages where the kernel hands them out (transparent huge pages, madvise mode), pinned on request: what the exploration walk of the ranked
// reduce reads is spread over gigabytes, far beyond what a TLB of 4 KB pages covers
struct HugeBuf {
    void* p = nullptr; size_t bytes = 0; bool registered = false;
    void* get(size_t n) {
        bytes = (std::max<size_t>(n, 1) + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1);
        p = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (p == MAP_FAILED) { p = nullptr; return nullptr; }
        madvise(p, bytes, MADV_HUGEPAGE);
        return p;
    }
    ~HugeBuf() { if (p) { if (registered) hipHostUnregister(p); munmap(p, bytes); } }
};
// ranked reduce: the pinned buffers the potential lists are downloaded into (Device::rrStaging); slice s of a call reuses buffer s of the previous call when it is large enough
struct RrStaging {
    std::vector<std::unique_ptr<HugeBuf>> bufs; size_t next = 0;
    u32* get(size_t n) {
        const size_t want = (std::max<size_t>(n, 16) + 16) * sizeof(u32);
        if (next < bufs.size() && bufs[next]->p && bufs[next]->bytes >= want) return (u32*)bufs[next++]->p;
        std::unique_ptr<HugeBuf> b(new HugeBuf()); u32* p = (u32*)b->get(want + want / 8); if (!p) return nullptr;
        memset(p, 0, b->bytes);                                  // (touch: the pages exist before they are pinned)
        if (hipHostRegister(p, b->bytes, hipHostRegisterDefault) == hipSuccess) b->registered = true; else (void)hipGetLastError();
        if (next < bufs.size()) bufs[next] = std::move(b); else bufs.push_back(std::move(b));
        return (u32*)bufs[next++]->p;
    }
};
static void rr_staging_release(Device* d) { if (d->rrStaging) { delete (RrStaging*)d->rrStaging; d->rrStaging = nullptr; } }

// =============================================================================================
// host-side launchers
// =============================================================================================
void dev_set_options(Device* d, const Options& opt) { d->opt = opt; }
Device* dev_create(int ordinal, const Options& opt, std::string& err) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0) { err = std::string("no HIP device available: ") + hipGetErrorString(e); return nullptr; }
    int dev = ordinal;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
    if (dev >= count) { err = "device ordinal out of range"; return nullptr; }
    if (hipSetDevice(dev) != hipSuccess) { err = "hipSetDevice failed"; return nullptr; }
    Device* d = new Device(); d->ordinal = dev; d->opt = opt;
    if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) { err = "hipStreamCreate failed"; delete d; return nullptr; }
    { const char* tb = d->opt.get("SAGE2OV_TEST_TAG_BITS"); const int nb = tb ? atoi(tb) : 24;
      const u32 mask = (nb >= 1 && nb < 24) ? ((1u << nb) - 1u) : 0xFFFFFFu;
      if (hipMemcpyToSymbol(HIP_SYMBOL(g_tag_mask), &mask, sizeof mask) != hipSuccess) { err = "tag mask upload failed"; delete d; return nullptr; }
      const char* mb = d->opt.get("SAGE2OV_TEST_MTAG_BITS"); const int nm = mb ? atoi(mb) : 24;
      const u32 mmask = (nm >= 1 && nm < 24) ? ((1u << nm) - 1u) : 0xFFFFFFu;
      if (hipMemcpyToSymbol(HIP_SYMBOL(g_mtag_mask), &mmask, sizeof mmask) != hipSuccess) { err = "tag mask upload failed"; delete d; return nullptr; }
      const char* fb = d->opt.get("SAGE2OV_TEST_FP_BITS"); const int nf = fb ? atoi(fb) : 20;
      const u32 fmask = (nf >= 0 && nf < 20) ? ((1u << nf) - 1u) : 0xFFFFFu;
      if (hipMemcpyToSymbol(HIP_SYMBOL(g_fp_mask), &fmask, sizeof fmask) != hipSuccess) { err = "fingerprint mask upload failed"; delete d; return nullptr; } }
    for (auto& ev : d->ev) hipEventCreate(&ev);
    if (hipMalloc(&d->d_counters, CTR_WORDS * sizeof(u64)) != hipSuccess) { err = "hipMalloc(counters) failed"; delete d; return nullptr; }
    hipMemset(d->d_counters, 0, CTR_WORDS * sizeof(u64));
    d->d_runStarts = d->d_counters + CTR_RUNSTARTS;
    if (hipHostMalloc((void**)&d->h_runStarts, 64 * sizeof(u64), hipHostMallocDefault) != hipSuccess || hipEventCreateWithFlags(&d->evRunStarts, hipEventDisableTiming) != hipSuccess) {
        err = "hipHostMalloc / hipEventCreate failed"; hipFree(d->d_counters); delete d; return nullptr; }
    return d;
}
static void mates_release(Device* d);
static void free_reads(Device* d) {
    dev_estflags_release(d);                                            // (flags of mate entries that name read ids)
    dev_readmap_release(d);                                             // (read ids again)
    dev_contigs_release(d);                                             // (and the reads the strings are spelled from)
    dev_copycount_release(d);                                           // (the frequencies and the present reads are of this read set)
    rr_staging_release(d);                     // (pinned host buffers sized by the previous read set)
    hipFree(d->reads);
    hipFree(d->findDir); d->findDir = nullptr; d->findDirBits = 0;      // (the lookup directory describes the read set that goes)
    mates_release(d);                                                   // (so do the ids of the mate table)
    dev_pairing_release(d);                                             // (and the ids of the staged reads)
    if (!d->resCarved) { hipFree(d->right); hipFree(d->left); hipFree(d->conn); hipFree(d->cflag); hipFree(d->status); hipFree(d->cand); }     // slots / csr / final_edges live in the workspace arena
    ph_release(d);                                                              // (diet mode: the phase block and what was carved out of it)
    for (auto& b : d->ws) { if (b.p && !b.epoch) hipFree(b.p); b.p = nullptr; b.cap = 0; b.epoch = 0; }
    s4cache_release(d);
    d->runStartFrac = 0.0; d->runStartsValid = false;          // (measured on the read set that just went: a new one decides for itself)
    d->statusByIdValid = true; d->statusGen++; d->nUnres = 0; d->unresGen = 0;      // (no status of either kind is left)
    d->readsLoc = nullptr; d->idOf = d->posOf = nullptr; d->statusP = nullptr; d->metaP = nullptr; d->mi1 = d->krec = nullptr; d->cand_cap = 0; d->n_cand = 0;
    d->reads = d->slots = nullptr; d->csr = nullptr; d->right = d->left = nullptr; d->conn = d->cflag = nullptr; d->status = nullptr; d->cand = nullptr; d->final_edges = nullptr;
}
void dev_destroy(Device* d) {
    if (!d) return;
    hipSetDevice(d->ordinal);
    hipStreamSynchronize(d->stream);
    dev_simplify_release(d); rr_staging_release(d);
    free_reads(d); hipFree(d->d_counters); if (d->h_runStarts) hipHostFree(d->h_runStarts); if (d->evRunStarts) hipEventDestroy(d->evRunStarts);
    for (auto& ev : d->ev) if (ev) hipEventDestroy(ev);
    hipStreamDestroy(d->stream);
    delete d;
}
void* dev_stream(Device* d) { return (void*)d->stream; }
int dev_sync(Device* d, std::string& err) { HIPCHK(hipStreamSynchronize(d->stream)); return 0; }
void dev_timings(Device* d, DevTimings* t) { *t = d->tm; }
void dev_reset_timings(Device* d) { d->tm = DevTimings(); }

// per-read results + candidate list: allocated when the probe pass first needs them (after the index build's transients are gone in diet mode)
static int ensure_results(Device* d, std::string& err) {
    const u64 N = d->N;
    if (!d->right && d->diet) {                                                // (pieces of the phase block: Device::Phase)
        d->right = (u64*)ph_carve(d, (N + 1) * sizeof(u64)); d->left = (u64*)ph_carve(d, (N + 1) * sizeof(u64));
        d->conn = (u32*)ph_carve(d, (N + 1) * sizeof(u32)); d->cflag = (u32*)ph_carve(d, (N + 1) * sizeof(u32)); d->status = (uint8_t*)ph_carve(d, N + 1);
        d->resCarved = true;
        if (!d->right || !d->left || !d->conn || !d->cflag || !d->status) { err = "result buffers: out of device memory"; return SAGE2OV_ERR_NOMEM; }
    }
    if (!d->right) { HIPCHK(hipMalloc(&d->right, (N + 1) * sizeof(u64))); HIPCHK(hipMalloc(&d->left, (N + 1) * sizeof(u64)));
                     HIPCHK(hipMalloc(&d->conn, (N + 1) * sizeof(u32))); HIPCHK(hipMalloc(&d->cflag, (N + 1) * sizeof(u32))); HIPCHK(hipMalloc(&d->status, (N + 1))); }
    if (!d->cand && !d->diet) { d->cand_cap = 2 * N + 1024; HIPCHK(hipMalloc(&d->cand, d->cand_cap * sizeof(EdgeCand))); }      // (diet: sized by a counting pass of the reciprocal kernel)
    return 0;
}
int dev_upload_reads(Device* d, const uint64_t* words, uint64_t N, int S, int minL, int maxL, int k, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (S != 4 && S != 8 && S != 16 && S != 32) { err = "unsupported words-per-read (read length limit is 1018 bases)"; return SAGE2OV_ERR_LIMIT; }
    if (N >= (1ull << 30)) { err = "more than 2^30-1 unique reads per context is not supported yet"; return SAGE2OV_ERR_LIMIT; }
    free_reads(d);
    d->N = N; d->S = S; d->maxL = maxL; d->k = k; d->h = k > 64 ? 64 : k; d->uniL = (N && minL == maxL) ? maxL : 0;
    HIPCHK(hipMalloc(&d->reads, (N + 1) * S * sizeof(u64)));
    HIPCHK(hipMemcpyAsync(d->reads, words, (N + 1) * S * sizeof(u64), hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    decide_diet(d);
    if (!d->diet) { int rc = ensure_results(d, err); if (rc) return rc; }
    return 0;
}

struct PtBufs { u32* E[2]; int W; const u32* src0 = nullptr; };      // two buffers of n tuples of W dwords each (kernels_partition.inc); src0: the first pass reads the tuples there (left untouched) and writes E[0]
static int partition_by_window(Device* d, PtBufs& B, int keyw, u32 n, int shiftW, u64 nWin, bool digit0Counted, u32* cnt, u32* base, u32* off, int* cur_out, std::string& err);
// Step 1 on the device: see k_org_canon.  On return the read store is resident exactly as after dev_upload_reads, and the
// host receives the image (for the .reads writer, lengths) and the frequencies.
int dev_organize_reads(Device* d, const uint64_t* pool, uint64_t pool_words, const uint64_t* off, const uint16_t* len, uint64_t n, int S, int minL, int maxL, int k,
                       uint64_t* N_out, RawU64& words_out, RawU16& freq_out, std::string& err, OrgAscii* ascii, bool pairing) {
    HIPCHK(hipSetDevice(d->ordinal));
    DevTmp PB; unsigned char* fwd = nullptr; int* pairId = nullptr; u64 pairN = 0;      // pairing: nothing of it is allocated or launched when it is off
    StreamLap whole(d->stream); HIPCHK(whole.create());
    const bool timing = d->opt.get("SAGE2OV_TIMING") != nullptr; auto tp = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) { if (!timing) return; hipStreamSynchronize(d->stream); auto t = std::chrono::steady_clock::now(); fprintf(stderr, "[step 1/device] %-30s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(t - tp).count()); tp = t; };
    HIPCHK(whole.start());
    // ASCII input (sage2ov_reads_add_ascii): filter, 2-bit pack and canonical orientation on the device (utils.cpp:144-166, :96-119, readLoader.cpp:195)
    unsigned char* dbases = nullptr; u64* doffA = nullptr; u32* gflag = nullptr; u32* gpos = nullptr;
    if (ascii) {
        const u64 nin = ascii->n_in;
        if (nin >= (1ull << 32) - RS_TILE) { err = "too many reads for the device organiser"; return SAGE2OV_ERR_LIMIT; }
        WS(db, unsigned char, WS_ORG_POOL, ascii->nbytes + 64); WS(dof, u64, WS_ORG_OFF, nin + 2); WS(gf, u32, WS_ORG_GFLAG, nin + 2); WS(gp, u32, WS_ORG_GPOS, nin + 2);
        dbases = db; doffA = dof; gflag = gf; gpos = gp;
        HIPCHK(hipMemcpyAsync(dbases, ascii->bases, ascii->nbytes, hipMemcpyHostToDevice, d->stream));
        HIPCHK(hipMemcpyAsync(doffA, ascii->off, (nin + 1) * sizeof(u64), hipMemcpyHostToDevice, d->stream));
        u64 init[6] = {0, 0, 0, 0, ~0ull, 0}; HIPCHK(hipMemcpyAsync(d->d_counters + CTR_ORG, init, sizeof init, hipMemcpyHostToDevice, d->stream));
        if (nin) hipLaunchKernelGGL(k_org_classify, dim3(grid_for(nin, 256)), dim3(256), 0, d->stream, dbases, doffA, (u64)nin, (u32)k, 1018u, gflag, d->d_counters + CTR_ORG);
        u64 cc[6]; { int rc = read_counters(d, CTR_ORG, 6, cc, err); if (rc) return rc; }
        if (cc[5]) { err = "reads longer than 1018 bases are not supported"; return SAGE2OV_ERR_LIMIT; }
        ascii->good = cc[1]; ascii->total_bp = cc[2]; ascii->small = cc[3]; ascii->maxL = (int)cc[0]; ascii->minL = cc[1] ? (int)cc[4] : 0;
        n = cc[1]; maxL = ascii->maxL; minL = ascii->minL;
        { int need = (2 * std::max(maxL, 1) + 9 + 63) / 64; S = 4; while (S < need) S *= 2; } ascii->S = S;
        if (nin) { u64 tot = 0; int rc = scan_u32(d, gflag, nin, gpos, &tot, err); if (rc) return rc; }
    }
    if (S != 4 && S != 8 && S != 16 && S != 32) { err = "unsupported words-per-read (read length limit is 1018 bases)"; return SAGE2OV_ERR_LIMIT; }
    if (n >= (1ull << 32) - RS_TILE) { err = "too many reads for the device organiser"; return SAGE2OV_ERR_LIMIT; }
    u64 N = 0;
    u64* reads = nullptr; unsigned short* dfreq = nullptr;
    if (n) {
        // (the whole work space before the first kernel is queued: the host no longer waits for every pass of the sort, and would otherwise allocate while it runs)
        WS(img, u64, WS_ORG_IMG, n * S); WS(k0, u64, WS_ORG_K0, n); WS(k1, u64, WS_ORG_K1, n); WS(v0, u32, WS_ORG_V0, n); WS(v1, u32, WS_ORG_V1, n);
        WS(hist, u32, WS_ORG_HIST, rs_hist_words(n)); WS(hscan, u32, WS_ORG_HSCAN, rs_hist_words(n)); WS(flag, u32, WS_ORG_FLAG, n + 2); WS(uid, u32, WS_ORG_UID, n + 2);
        WS(partial, u64, WS_PARTIAL, scan_partial_words(std::max<u64>(n, rs_hist_words(n))));      // (the sort's scans and the one over the heads)
        if (pairing) { fwd = PB.get<unsigned char>(n); if (!fwd) { err = "pairing: out of device memory"; return SAGE2OV_ERR_NOMEM; } }
        if (ascii) hipLaunchKernelGGL(k_org_pack, dim3(grid_for(ascii->n_in, 256)), dim3(256), 0, d->stream, dbases, doffA, (u64)ascii->n_in, gflag, gpos, S, img, k0, v0, fwd);
        else {
            WS(dpool, u64, WS_ORG_POOL, pool_words + 17); WS(doff, u64, WS_ORG_OFF, n); WS(dlen, unsigned short, WS_ORG_LEN, n);
            HIPCHK(hipMemcpyAsync(dpool, pool, pool_words * sizeof(u64), hipMemcpyHostToDevice, d->stream));
            HIPCHK(hipMemsetAsync(dpool + pool_words, 0, 17 * sizeof(u64), d->stream));
            HIPCHK(hipMemcpyAsync(doff, off, n * sizeof(u64), hipMemcpyHostToDevice, d->stream));
            HIPCHK(hipMemcpyAsync(dlen, len, n * sizeof(uint16_t), hipMemcpyHostToDevice, d->stream));
            lap("work space + upload");
            hipLaunchKernelGGL(k_org_canon, dim3(grid_for(n, 256)), dim3(256), 0, d->stream, dpool, doff, dlen, (u64)n, S, img, k0, v0, fwd);
        }
        static_assert(RS_ALL_N % 2 == 0, "an even number of passes: every sort below leaves the pairs where it found them, in k0 / v0");
        const RsBufs B = {{k0, k1}, {v0, v1}, hist, hscan, partial}; int side = 0; u64* const ka = k0; u32* const va = v0;
        { const int rc = radix_sort_pairs(d, B, n, RS_ALL_DIGITS, RS_ALL_N, &side, err); if (rc) return rc; }
        u32 longrun = 0;
        HIPCHK(hipMemsetAsync(flag, 0, sizeof(u32), d->stream));
        hipLaunchKernelGGL(k_org_longrun, dim3(grid_for(n, 256)), dim3(256), 0, d->stream, ka, (u64)n, flag);
        HIPCHK(hipMemcpyAsync(&longrun, flag, sizeof longrun, hipMemcpyDeviceToHost, d->stream)); HIPCHK(hipStreamSynchronize(d->stream));
        if (longrun || d->opt.get("SAGE2OV_TEST_FULL_SORT")) {
            // many reads share their first 32 bases: order on every word instead (stable LSD radix, last word first; the pairs arrive
            // sorted by the first word, which the last eight passes simply reproduce)
            for (int c = S - 1; c >= 0; c--) {
                hipLaunchKernelGGL(k_org_wordkeys, dim3(grid_for(n, 256)), dim3(256), 0, d->stream, img, S, c, va, (u64)n, ka);
                { const int rc = radix_sort_pairs(d, B, n, RS_ALL_DIGITS, RS_ALL_N, &side, err); if (rc) return rc; }
            }
        } else hipLaunchKernelGGL(k_org_ties, dim3(grid_for(n, 256)), dim3(256), 0, d->stream, ka, va, (u64)n, img, S);
        hipLaunchKernelGGL(k_org_heads, dim3(grid_for(n, 256)), dim3(256), 0, d->stream, ka, va, (u64)n, img, S, flag);
        { int rc = scan_u32(d, flag, n, uid, partial, &N, err); if (rc) return rc; }
        if (N >= (1ull << 30)) { err = "more than 2^30-1 unique reads per context is not supported yet"; return SAGE2OV_ERR_LIMIT; }
        WS(headPos, u32, WS_ORG_HEAD, N + 2);
        { int rc = head_positions(d, flag, uid, n, headPos, N, err); if (rc) return rc; }
        lap("canonical, sort, heads");
        if (pairing) {                                                      // the ids of the staged reads, while flag / uid / va still stand
            int* idOf = PB.get<int>(n); if (!idOf) { err = "pairing: out of device memory"; return SAGE2OV_ERR_NOMEM; }
            hipLaunchKernelGGL(k_org_ids, dim3(grid_for(n, 256)), dim3(256), 0, d->stream, va, flag, uid, (u64)n, fwd, idOf);
            pairId = idOf; pairN = n;
        }
        HIPCHK(hipMalloc(&reads, (N + 1) * S * sizeof(u64))); HIPCHK(hipMalloc(&dfreq, (N + 1) * sizeof(unsigned short)));
        HIPCHK(hipMemsetAsync(reads, 0, S * sizeof(u64), d->stream)); HIPCHK(hipMemsetAsync(dfreq, 0, sizeof(unsigned short), d->stream));
        hipLaunchKernelGGL(k_org_gather, dim3(grid_for_capped(N * S, 256)), dim3(256), 0, d->stream, va, headPos, (u64)N, img, S, reads, dfreq);
    } else {
        HIPCHK(hipMalloc(&reads, S * sizeof(u64))); HIPCHK(hipMalloc(&dfreq, sizeof(unsigned short)));
        HIPCHK(hipMemsetAsync(reads, 0, S * sizeof(u64), d->stream)); HIPCHK(hipMemsetAsync(dfreq, 0, sizeof(unsigned short), d->stream));
    }
    if (pairing && ascii) {                                                 // ASCII route: per raw record, back through the scan of the classifier's flags
        const u64 nin = ascii->n_in; int* rawId = PB.get<int>(nin); if (!rawId) { err = "pairing: out of device memory"; return SAGE2OV_ERR_NOMEM; }
        if (n) hipLaunchKernelGGL(k_org_ids_raw, dim3(grid_for(nin, 256)), dim3(256), 0, d->stream, gflag, gpos, (u64)nin, pairId, rawId);
        else if (nin) HIPCHK(hipMemsetAsync(rawId, 0, nin * sizeof(int), d->stream));
        pairId = rawId; pairN = nin;                                        // (the by-staging-index ids go with PB)
    }
    HIPCHK(hipGetLastError());
    HIPCHK(whole.end());
    lap("read store allocation + gather");
    words_out.resize((N + 1) * S); freq_out.resize(N + 1);
    touch_pages(words_out.data(), words_out.size() * sizeof(u64), 8);
    lap("host vectors (resize, first touch)");
    HIPCHK(hipMemcpyAsync(words_out.data(), reads, (N + 1) * S * sizeof(u64), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipMemcpyAsync(freq_out.data(), dfreq, (N + 1) * sizeof(unsigned short), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    lap("download of the store");
    whole.add(d->tm.organize_ms);
    hipFree(dfreq);
    // the organised store becomes the context's read store (same state as after dev_upload_reads)
    free_reads(d);
    d->N = N; d->S = S; d->maxL = maxL; d->k = k; d->h = k > 64 ? 64 : k; d->reads = reads; d->uniL = (N && minL == maxL) ? maxL : 0;
    if (pairing) { PB.keep(pairId); d->pairId = pairId; d->pairN = pairN; d->pairRaw = ascii != nullptr; d->pairValid = true; }
    mem_sample(d);
    // the organiser's work space (the staged reads, their slot image, the sort's key / value pairs: ~180 bytes per read) is not needed again
    for (int id : {WS_ORG_POOL, WS_ORG_OFF, WS_ORG_LEN, WS_ORG_IMG, WS_ORG_K0, WS_ORG_K1, WS_ORG_V0, WS_ORG_V1, WS_ORG_HIST, WS_ORG_HSCAN, WS_ORG_FLAG, WS_ORG_UID, WS_ORG_HEAD, WS_ORG_GFLAG, WS_ORG_GPOS}) ws_free(d, id);
    decide_diet(d);
    if (!d->diet) { int rc = ensure_results(d, err); if (rc) return rc; }
    lap("release + result buffers");
    *N_out = N;
    return 0;
}

// processing order of ids [lo,hi): grouped by the reads' global minimiser (see k_minimizer)
static int build_locality_order(Device* d, u64 lo, u64 hi, const u32** order_out, std::string& err) {
    const u64 n = hi - lo;
    // reads sorted by (their global minimiser's hash, strand of the minimiser, start of the read relative to it): LSD radix passes
    // (kernels_partition.inc), first the 9 bits of strand + offset, then the hash -- reads with one minimiser end up next to each
    // other, each starting a few bases after the one before.  Measured at BASELINE configs[2]: probe kernel 149 -> 142 ms from the finer processing
    // order alone, 120 ms with the read store in that order too.  *order_out: per position, meta << 32 | id.
    // ALL 32 bits of the hash since the end of round 3 (four passes of 8 bits; 27 bits = three passes of 9 before): two minimisers that share a bucket interleave
    // their reads and break each other's runs of shifted reads (window reuse, 5.2) -- hash bits -> probe pass at configs[2]: 18 -> 97.2 ms, 24 -> 78.8, 27 -> 62.5,
    // 30 -> 57.2, 32 -> 56.5, for 0.3 ms more of index build.
    constexpr int lg = 32;
    const u32 ntiles = (u32)((n + PT_TILE - 1) / PT_TILE);
    PtBufs B; B.W = 3;                                                        // {hash, id, meta}
    { WS(a, u32, WS_MINH, 3 * (n + 4)); B.E[0] = a; } { WS(a, u32, WS_OCUR, 3 * (n + 4)); B.E[1] = a; }
    WS(cnt, u32, WS_PT_CNT, (u64)PT_NB_MAX * std::max<u32>(ntiles, 1) + 2); WS(base, u32, WS_PT_BASE, (u64)PT_NB_MAX * std::max<u32>(ntiles, 1) + 2);
    // one element format for all four passes, written by the minimiser kernel itself (round 2 had a pack and a re-key kernel in between): pass 1 sorts by
    // the meta (dword 2), passes 2-4 by the hash (dword 0)
    if (d->S == 4) hipLaunchKernelGGL((k_minimizer_t<4>), dim3(grid_for(n, 256)), dim3(256), 0, d->stream, d->reads, (u64)lo, (u64)hi, B.E[0]);
    else if (d->S == 8) hipLaunchKernelGGL((k_minimizer_t<8>), dim3(grid_for(n, 256)), dim3(256), 0, d->stream, d->reads, (u64)lo, (u64)hi, B.E[0]);
    else hipLaunchKernelGGL(k_minimizer, dim3(grid_for(n, 256)), dim3(256), 0, d->stream, d->reads, (u64)lo, (u64)hi, d->S, B.E[0]);
    int cur = 0; int rc = partition_by_window(d, B, 2, (u32)n, 0, 1ull << 9, false, cnt, base, nullptr, &cur, err); if (rc) return rc;
    PtBufs C; C.W = 3; C.E[0] = B.E[cur]; C.E[1] = B.E[cur ^ 1];
    int cur2 = 0; rc = partition_by_window(d, C, 0, (u32)n, 32 - lg, 1ull << lg, false, cnt, base, nullptr, &cur2, err); if (rc) return rc;
    *order_out = C.E[cur2];
    return 0;
}
// The locality-ordered copy of the read store + the two translation tables (see Device::readsLoc).  Part of the index build (timed with it).
// Round 3: two kernels.  k_loc_index writes the translation tables from the order; k_loc_scatter then STREAMS the id-ordered store (coalesced reads) and
// writes every slot to its position (whole 32 / 64 / 128-byte slots: no read-modify-write at the memory side).  The gather it replaces pulled every
// 64-byte slot as a 128-byte line request: 5.4 GB of reads for 2.7 GB of reads at configs[2].
// runStarts (64 words, zeroed by the host; their sum, over every eighth block): positions whose read has another minimiser or another strand of it than the read before -- reads that cannot take their windows
// over from a predecessor (kernels_probe_fast.inc); their share decides whether the minimiser groups are built (dev_build_index)
__global__ void k_loc_index(const u32* __restrict__ order, u64 N, u32* idOf, u32* posOf, unsigned short* meta, unsigned long long* runStarts) {      // order: 3 dwords per position {hash, id, meta}
    const u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p == 0) { idOf[0] = 0; posOf[0] = 0; idOf[N + 1] = 0; posOf[N + 1] = 0; meta[0] = 0xFFFF; meta[N + 1] = 0xFFFF; }
    if ((blockIdx.x & 7u) == 0) {                                         // (every eighth block of 256 positions: a sample is all the decision needs; one atomic per sampled block)
        const bool start = order && p < N && (p == 0 || order[3 * p] != order[3 * (p - 1)] || ((order[3 * p + 2] ^ order[3 * (p - 1) + 2]) & 0x100u) != 0);
        const int c = __syncthreads_count(start);
        if (threadIdx.x == 0 && c) atomicAdd(runStarts + ((blockIdx.x >> 3) & 63u), (unsigned long long)c);
    }
    if (p >= N) return;
    const u32 id = order ? order[3 * p + 1] : (u32)(p + 1); u32 mt = order ? order[3 * p + 2] : 0xFFFFu;
    // (bit 9, round 4: this read has ANOTHER minimiser hash than the read before it -- nothing of that read's run can be carried over; the fast probe kernel moves the
    //  boundaries of its waves' visits there)
    if (order && (p == 0 || order[3 * p] != order[3 * (p - 1)])) mt |= 0x200u;
    idOf[p + 1] = id; posOf[id] = (u32)(p + 1); meta[p + 1] = (unsigned short)mt;       // meta 0xFFFF: no minimiser information (no window reuse)
}
__global__ void k_loc_scatter(const u64* __restrict__ reads, const u32* __restrict__ posOf, u64 N, int S, u64* out) {
    // one 16-byte piece of a slot per thread and step; grid-stride: (N + 1) * S / 2 pieces reach 2^32 from 2^29 reads of the 16-word layout on, and a launch
    // of 2^32 threads or more runs modulo 2^32 (grid_for_capped)
    const int H = S / 2; const u64 total = (N + 1) * H, stride = (u64)gridDim.x * blockDim.x;
    for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const u64 id = t / H; const int c = (int)(t % H);
        const ulonglong2 v = ((const ulonglong2*)reads)[t];        // (slot 0 is all zero and stays at position 0: posOf[0] = 0)
        ((ulonglong2*)out)[(u64)posOf[id] * H + c] = v;
    }
}
__global__ void k_status_by_pos(const u32* __restrict__ idOf, const uint8_t* __restrict__ status, u64 N, uint8_t* statusP) {
    const u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (p > N) return; statusP[p] = p ? status[idOf[p]] : (uint8_t)0xFF;
}
__global__ void k_ids_to_pos(const u32* __restrict__ ids, u64 n, const u32* __restrict__ posOf, u32* out) { const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (x < n) out[x] = posOf[ids[x]]; }
// deferCopy: the caller writes the copy itself, in the same visit of the id-ordered store that makes the index tuples (k_ix_tuples_loc, dev_build_index)
static int build_locality_store(Device* d, bool deferCopy, std::string& err) {
    const u64 N = d->N;
    WS(rl, u64, WS_LOC_READS, (N + 1) * d->S); WS(io, u32, WS_LOC_IDOF, N + 2); WS(po, u32, WS_LOC_POSOF, N + 2); WS(sp, uint8_t, WS_LOC_STATUS, N + 2);
    WS(me, unsigned short, WS_LOC_META, N + 2);
    d->readsLoc = rl; d->idOf = io; d->posOf = po; d->statusP = sp; d->metaP = me;
    const u32* order = nullptr;
    if (N) { int rc = build_locality_order(d, 1, N + 1, &order, err); if (rc) return rc; }
    HIPCHK(hipMemsetAsync(d->d_runStarts, 0, 64 * sizeof(u64), d->stream));                   // run starts of the order (k_loc_index)
    hipLaunchKernelGGL(k_loc_index, dim3(grid_for(std::max<u64>(N, 1), 256)), dim3(256), 0, d->stream, order, (u64)N, io, po, me, (unsigned long long*)d->d_runStarts);
    d->runStartsValid = order != nullptr;
    if (!order) d->runStartFrac = 0.0;
    // (the count travels to a pinned word while k_loc_scatter below runs: dev_build_index waits for the copy's event, not for the stream)
    if (d->runStartsValid) { HIPCHK(hipMemcpyAsync(d->h_runStarts, d->d_runStarts, 64 * sizeof(u64), hipMemcpyDeviceToHost, d->stream)); HIPCHK(hipEventRecord(d->evRunStarts, d->stream)); }
    if (d->diet) { HIPCHK(hipStreamSynchronize(d->stream)); ph_begin(d, false); }       // the order's sort buffers (24 bytes per read) go before the tuples come: a phase of their own
    if (!deferCopy) hipLaunchKernelGGL(k_loc_scatter, dim3(grid_for_capped((N + 1) * (d->S / 2), 256)), dim3(256), 0, d->stream, d->reads, po, (u64)N, d->S, rl);
    HIPCHK(hipGetLastError());
    return 0;
}
static int refresh_status_by_pos(Device* d, std::string& err) {
    hipLaunchKernelGGL(k_status_by_pos, dim3(grid_for(d->N + 1, 256)), dim3(256), 0, d->stream, d->idOf, d->status, (u64)d->N, d->statusP);
    HIPCHK(hipGetLastError()); return 0;
}
// In front of every reader of d->status: the by-id copy of what k_recip_cond left by position, gathered once (the clean-data step never gets here)
static int ensure_status_by_id(Device* d, std::string& err) {
    if (d->statusByIdValid) return 0;
    if (!d->status || !d->statusP || !d->posOf) { err = "status by id: no reciprocal pass to take it from"; return SAGE2OV_ERR_INTERNAL; }
    hipLaunchKernelGGL(k_status_by_id, dim3(grid_for(d->N + 1, 256)), dim3(256), 0, d->stream, (u64)d->N, d->posOf, d->statusP, d->status);
    HIPCHK(hipGetLastError()); d->statusByIdValid = true; return 0;
}
static int pt_digits(u64 nWin, int* bits, int* nd) {            // window id bits, number of <= 9-bit digits
    int wb = 0; while ((1ull << wb) < nWin) wb++;
    *bits = wb; *nd = wb == 0 ? 0 : (wb + 8) / 9; return 0;
}
// One scatter pass: two workgroups of eight waves per CU on half-staged tiles (k_pt_scatter2), same output as the one workgroup of sixteen (k_pt_scatter), which
// keeps two cases.  (1) Thin runs: where the digits of the window id or the hash (dword 0: spread evenly) leave a (tile, digit) pair less than two 128-byte lines, the
// pass is at the limit of its partial-line writes and a second workgroup on the CU gives it nothing to overlap -- measured, the table's first pass at BASELINE configs[2]
// (170 M 12-byte tuples, 9 bits: 192 bytes) 1.39 ms with one workgroup, 1.55 with two; every other pass 5 - 19 % faster with two.  The order's
// meta digit (dword 2) has 9 bits too but takes some 270 of its values: runs of 360 bytes.  (2) SAGE2OV_PT_ONE_BLOCK: every pass, for A/B runs and the tests.
template <int W, int KEYW>
static void pt_launch_scatter(Device* d, u32 ntiles, const u32* in, u32 n, int shift, u32 mask, const u32* base, u32* out) {
    const bool thinRuns = KEYW == 0 && (u64)PT_TILE * W * sizeof(u32) / ((u64)mask + 1) < 256;
    if (thinRuns || d->opt.flag("SAGE2OV_PT_ONE_BLOCK")) hipLaunchKernelGGL((k_pt_scatter<W, KEYW>), dim3(ntiles), dim3(PT_SC_THREADS), 0, d->stream, in, n, shift, mask, base, ntiles, out);
    else hipLaunchKernelGGL((k_pt_scatter2<W, KEYW>), dim3(ntiles), dim3(PT2_THREADS), 0, d->stream, in, n, shift, mask, base, ntiles, out);
}
// The tuples are sorted by the window id (dword keyw >> shiftW); `digit 0 counted` tells that cnt already holds the first digit's per-tile histogram (taken
// by the kernel that wrote the tuples).  On return B.E[*cur_out] is the sorted array and off[0..nWin] (if given) holds the window boundaries.
static int partition_by_window(Device* d, PtBufs& B, int keyw, u32 n, int shiftW, u64 nWin, bool digit0Counted, u32* cnt, u32* base, u32* off, int* cur_out, std::string& err) {
    int wb, nd; pt_digits(nWin, &wb, &nd);
    const u32 ntiles = (u32)((n + PT_TILE - 1) / PT_TILE);
    int cur = 0;
    if (n) {
        const int bper = nd ? (wb + nd - 1) / nd : 0;
        const u32* in = B.src0 ? B.src0 : B.E[0];
        if (B.src0 && nd == 0) { HIPCHK(hipMemcpyAsync(B.E[0], B.src0, (size_t)n * B.W * sizeof(u32), hipMemcpyDeviceToDevice, d->stream)); in = B.E[0]; }
        for (int j = 0; j < nd; j++) {
            const int shift = shiftW + j * bper; const int bj = std::min(bper, wb - j * bper); const u32 mask = (1u << bj) - 1u;
            if (!(j == 0 && digit0Counted)) hipLaunchKernelGGL(k_pt_hist, dim3(ntiles), dim3(PT_THREADS), 0, d->stream, in + keyw, n, shift, mask, cnt, ntiles, (u32)B.W);
            int rc = scan_u32(d, cnt, (u64)(mask + 1) * ntiles, base, nullptr, err); if (rc) return rc;      // (no read-back: nothing synchronises)
            const int o = (j == 0 && B.src0) ? 0 : (cur ^ 1);
            if (B.W == 4 && keyw == 0) pt_launch_scatter<4, 0>(d, ntiles, in, n, shift, mask, base, B.E[o]);
            else if (B.W == 3 && keyw == 0) pt_launch_scatter<3, 0>(d, ntiles, in, n, shift, mask, base, B.E[o]);
            else if (B.W == 3 && keyw == 2) pt_launch_scatter<3, 2>(d, ntiles, in, n, shift, mask, base, B.E[o]);
            else { err = "partition: unsupported tuple format"; return SAGE2OV_ERR_INTERNAL; }
            cur = o; in = B.E[o];
        }
        // window boundaries: a binary search per window (SAGE2OV_INDEX_SEPARATE_PASSES, A/B runs: the pass over all keys)
        if (off && d->opt.get("SAGE2OV_INDEX_SEPARATE_PASSES")) hipLaunchKernelGGL(k_pt_bounds, dim3(grid_for(n, 256)), dim3(256), 0, d->stream, B.E[cur] + keyw, n, shiftW, (u32)nWin, off, (u32)B.W);
        else if (off) hipLaunchKernelGGL(k_pt_bounds_search, dim3(grid_for(nWin + 1, 256)), dim3(256), 0, d->stream, B.E[cur] + keyw, n, shiftW, (u32)nWin, off, (u32)B.W);
    } else if (off) HIPCHK(hipMemsetAsync(off, 0, (nWin + 1) * sizeof(u32), d->stream));
    HIPCHK(hipGetLastError());
    *cur_out = cur;
    return 0;
}
// first-digit parameters of the tuple kernel (must agree with partition_by_window)
static void pt_first_digit(u64 nWin, int shiftW, int* shift0, u32* mask0, int* doHist) {
    int wb, nd; pt_digits(nWin, &wb, &nd);
    if (!nd) { *shift0 = 0; *mask0 = 0; *doHist = 0; return; }
    const int bper = (wb + nd - 1) / nd; *shift0 = shiftW; *mask0 = (1u << std::min(bper, wb)) - 1u; *doHist = 1;
}

// (probe time the minimiser groups save) / (what they cost to build) at full share, as a function of the share f of reads without a predecessor: see dev_build_index
static inline double RUN_START_RULE(double f) { return f > 0.1 ? 27.0 * (f - 0.1) : 0.0; }
int dev_build_index(Device* d, uint64_t* slots_out, uint64_t* keys_out, uint64_t* csr_out, uint64_t* nlong_out, uint32_t* rebuilds, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    const u64 N = d->N; if (!d->reads && !d->readsLoc) { err = "reads not resident"; return SAGE2OV_ERR_ARG; }
    s4cache_release(d);                                                   // (a new step 2: step 4's spare blocks must not stand in the way of steps 2-3; empty unless step 4 ran since)
    HIPCHK(hipEventRecord(d->ev[0], d->stream));                          // (the locality store is part of the build and of index_ms)
    if (d->diet) {                                                            // phase A: the previous step's results go before the sort's buffers come (Device::Phase)
        HIPCHK(hipStreamSynchronize(d->stream));
        if (!d->resCarved) { hipFree(d->right); hipFree(d->left); hipFree(d->conn); hipFree(d->cflag); hipFree(d->status); hipFree(d->cand);     // (from before the context went on the diet)
                             d->right = d->left = nullptr; d->conn = d->cflag = nullptr; d->status = nullptr; d->cand = nullptr; d->cand_cap = 0; d->n_cand = 0; }
        ph_begin(d);
    }
    // One visit of the id-ordered store writes the locality-ordered copy AND the tuples of the first attempt (k_ix_tuples_loc) where that store is resident, the
    // layout has 8 words and the context is not on the diet; everything else -- reseed attempts, diet mode (byPos), other layouts, SAGE2OV_INDEX_SEPARATE_PASSES --
    // keeps k_loc_scatter and k_ix_tuples.  (The fused launch is one workgroup per tile of 4N < 2^32 tuples: 2^28 threads at most, far inside the 2^32-thread rule.)
    const u64 fusedThreads = ((4 * N + PT_TILE - 1) / PT_TILE) * PT_THREADS;
    bool copyPending = d->reads && d->S == 8 && !d->diet && N > 0 && fusedThreads < (1ull << 32) && !d->opt.get("SAGE2OV_INDEX_SEPARATE_PASSES");
    if (d->reads) { int rc = build_locality_store(d, copyPending, err); if (rc) return rc; }
    // (diet mode, second and later builds: the id-ordered store was released after the first one; the locality-ordered store and its tables are what
    //  this build would produce again -- the order is a function of the reads -- so they are kept)
    if (d->diet && d->reads && d->uniL) { HIPCHK(hipStreamSynchronize(d->stream)); hipFree(d->reads); d->reads = nullptr; }      // every later reader takes lengths from uniL
    const bool byPos = d->reads == nullptr;
    // (diet mode: the previous step's results -- per-read records, candidates, final edges: ~60 bytes per read -- went when this build began, ph_begin above)
    d->T = std::max<u64>(IX_W, (8 * N + IX_W - 1) / IX_W * IX_W);            // load <= 0.5, as hashTable.cpp:83 sizes it; whole windows
    // (tests: SAGE2OV_TEST_TABLE_SLOTS forces a larger table, e.g. beyond 2^32 slots -- slot indices are 64-bit, pair indices and window ids 32-bit)
    if (const char* ev = d->opt.get("SAGE2OV_TEST_TABLE_SLOTS")) { const u64 want = strtoull(ev, nullptr, 10); if (want > d->T) d->T = (want + IX_W - 1) / IX_W * IX_W; }
    if ((d->T >> 1) >= (1ull << 32)) {
        if (copyPending) hipLaunchKernelGGL(k_loc_scatter, dim3(grid_for_capped((N + 1) * (d->S / 2), 256)), dim3(256), 0, d->stream, d->reads, d->posOf, (u64)N, d->S, d->readsLoc);    // (the store stays whole)
        err = "table too large: more than 2^32 slot pairs"; return SAGE2OV_ERR_LIMIT; }
    const u64 nW = d->T / IX_W; const u32 n = (u32)(4 * N);
    const u32 big_cap = 1u << 20;
    WS(slots_ws, u64, WS_SLOTS, d->T); d->slots = slots_ws;
    WS(big, u64, WS_BIG, (u64)big_cap * 3);
    WS(csr_ws, u32, WS_CSR, std::max<u64>(1, 4 * N)); d->csr = csr_ws;
    // The minimiser groups (second access path of the fast kernel) serve the reads that START a run of the locality order -- reads with another minimiser, or another
    // strand of it, than the read before: every one of their windows is a random line of the uniform table otherwise.  How many there are is a property of the data
    // (coverage: a minimiser's reads are a run per strand), counted by k_loc_index.  Measured at the end of round 3 with the order on all 32 hash bits
    // (tests/diag/groups_by_coverage.py, groups_by_size.py; share of such reads -> probe time saved at full share / build time, ms): 34-39 M reads at 10x / 20x / 30x / 50x
    // coverage 30.5 % -> 35.3 / 6.2, 18.8 % -> 13.0 / 5.8, 13.9 % -> 6.6 / 5.5, 9.4 % -> 2.0 / 5.2; 8.5-9.7 M reads 32.2 % -> 6.8 / 1.7, 19.4 % -> 2.2 / 1.5, 14.2 % -> 0.9 / 1.4,
    // 9.5 % -> -0.1 / 1.3; 50x (9.5 %) at 42.5 M, 68 M and 102 M reads 4.2 / 6.1, 8.5 / 10.0 and 12.1 / 16.2.  The ratio is close to 27 (f - 0.1) from 20 M reads on and 0.72
    // of that below (RUN_START_RULE); the saving scales with the share of the reads this context probes, the build does not: built iff share x ratio >= 1.
    // (with the fused kernel this wait is in front of its launch -- the tuple width depends on wantMI -- and the GPU idles for the event's round trip; k_loc_scatter used to cover it)
    if (d->runStartsValid) {
        HIPCHK(hipEventSynchronize(d->evRunStarts));
        u64 rs = 0; for (int x = 0; x < 64; x++) rs += d->h_runStarts[x];
        u64 sampled = 0; for (u64 b0 = 0; b0 * 256 < N; b0 += 8) sampled += std::min<u64>(256, N - b0 * 256);      // positions of the sampled blocks
        d->runStartFrac = sampled ? (double)rs / (double)sampled : 0.0; d->runStartsValid = false;      // (kept: a diet-mode rebuild reuses the order)
    }
    const double f_ = d->runStartFrac, sizeFactor = N >= 20000000ull ? 1.0 : 0.72;
    bool wantMI = !d->diet && N >= 2000000ull && d->probeShare * sizeFactor * RUN_START_RULE(f_) >= 1.0;
    if (d->opt.get("SAGE2OV_TIMING")) fprintf(stderr, "[index] reads without a predecessor in the locality order: %.1f %% -> minimiser groups %s\n", 100.0 * f_, wantMI ? "built" : "not built");
    if (const char* ev = d->opt.get("SAGE2OV_MINIMIZER_INDEX")) wantMI = atoi(ev) != 0;
    if ((d->h - std::min(d->h, 16) + 1) < 8) wantMI = false;
    u64 TL = 0; int tlBits = 0; u64 gW = 0;
    // >= 3N group words (round 3; 2N before): a group window takes 256 x MIW_R = 2048 group tuples in registers and ~3N distinct keys spread over TL / 2048 windows, so with
    // TL in [2N, 3N) most windows overflowed into the global scratch, the scratch ran out, and the groups were built and then given up ("crowded") for every read set
    // between 24 M and 33 M unique reads -- 4 ms of build for nothing, found by timing sizes between configs[1] and configs[2] (tests/diag/groups_by_size.py)
    if (wantMI) { TL = IX_GW; tlBits = IX_GWLOG; while (TL < d->T / 8 * 3) { TL <<= 1; tlBits++; } gW = TL / IX_GW; }
    const u64 nAlloc = std::max<u64>(4, (u64)n + 4);
    const u32 ntiles = (u32)((n + PT_TILE - 1) / PT_TILE);
    PtBufs B; B.W = wantMI ? 4 : 3;                                          // {K, M, entry, tag} with the groups, {K, entry, tag} without
    { WS(a, u32, WS_PT_K0, nAlloc * B.W); B.E[0] = a; } { WS(a, u32, WS_PT_K1, nAlloc * B.W); B.E[1] = a; }
    WS(cnt, u32, WS_PT_CNT, (u64)PT_NB_MAX * std::max<u32>(ntiles, 1) + 2); WS(base, u32, WS_PT_BASE, (u64)PT_NB_MAX * std::max<u32>(ntiles, 1) + 2);
    WS(winOff, u32, WS_PT_OFF, nW + 2);
    u64* mi1 = nullptr; u64* krec = nullptr; u32* gOff = nullptr;
    if (wantMI) {
        WS(m1, u64, WS_MI1, TL); mi1 = m1;
        WS(kr_, u64, WS_KREC, 4 * N + MI_SCAN_PAD); krec = kr_;              // one record per distinct key (<= 4N)
        WS(go, u32, WS_PT_GOFF, gW + 3); gOff = go;
    }
    *rebuilds = 0;
    const bool timing = d->opt.get("SAGE2OV_TIMING") != nullptr; auto tp = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) { if (!timing) return; hipStreamSynchronize(d->stream); auto t = std::chrono::steady_clock::now(); fprintf(stderr, "[index] %-34s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - tp).count()); tp = t; };
    u64 c[9]; u32 ixCntBits = (u32)IXW_CNT_BITS_DEFAULT;
    for (int attempt = 0;; attempt++) {
        HIPCHK(hipMemsetAsync(d->d_counters + CTR_INDEX, 0, 10 * sizeof(u64), d->stream));
        // ---- tuples of the 4N entries, sorted by the window of their home slot
        int shift0, doHist; u32 mask0; pt_first_digit(nW, IX_WPLOG, &shift0, &mask0, &doHist);
        if (copyPending) { hipLaunchKernelGGL(k_ix_tuples_loc, dim3(ntiles), dim3(PT_THREADS), 0, d->stream, d->reads, d->posOf, (u32)N, d->h, d->seed, (u32)(d->T >> 1), wantMI ? 1 : 0, shift0, mask0, doHist,
                                              B.E[0], cnt, ntiles, d->readsLoc); copyPending = false; }
        else if (n) hipLaunchKernelGGL(k_ix_tuples, dim3(ntiles), dim3(PT_THREADS), 0, d->stream, byPos ? d->readsLoc : d->reads, d->posOf, byPos ? 1 : 0, (u32)N, d->S, d->h, d->seed, (u32)(d->T >> 1), wantMI ? 1 : 0, shift0, mask0, doHist,
                                  B.E[0], cnt, ntiles);
        lap("tuples");
        int cur = 0;
        { int rc = partition_by_window(d, B, 0, n, IX_WPLOG, nW, doHist != 0, cnt, base, winOff, &cur, err); if (rc) return rc; }
        lap("partition by table window");
        if (d->opt.get("SAGE2OV_VERIFY_PARTITION") && n) {
            u64* vo = nullptr; HIPCHK(hipMalloc(&vo, 3 * sizeof(u64))); HIPCHK(hipMemsetAsync(vo, 0, 3 * sizeof(u64), d->stream));
            hipLaunchKernelGGL(k_pt_verify, dim3(grid_for(n, 256)), dim3(256), 0, d->stream, B.E[cur], n, IX_WPLOG, (u32)B.W, winOff, (u32)nW, vo);
            u64 hv[3]; HIPCHK(hipMemcpyAsync(hv, vo, sizeof hv, hipMemcpyDeviceToHost, d->stream)); HIPCHK(hipStreamSynchronize(d->stream)); hipFree(vo);
            fprintf(stderr, "[verify-partition] %llu tuples, %llu windows: %llu order violations, largest window %llu tuples, %llu negative windows\n", (unsigned long long)n, (unsigned long long)nW,
                    (unsigned long long)hv[0], (unsigned long long)hv[1], (unsigned long long)hv[2]);
        }
        // ---- the windows of the uniform table, built in LDS; group tuples into the free buffer set
        IxWinArgs A; A.T = B.E[cur]; A.W = B.W; A.winOff = winOff; A.nW = (u32)nW; A.slots = d->slots; A.csr = d->csr;
        A.counters = d->d_counters + CTR_INDEX; A.big = big; A.big_cap = big_cap; A.idOf = d->idOf; A.G = wantMI ? B.E[cur ^ 1] : nullptr; A.wh = nullptr; A.cntBits = ixCntBits;     // (group tuples, 12 bytes each, into the free 16-byte buffer)
        // (the scratch words of heavy windows need a buffer of their own)
        // one word per SURPLUS tuple of a heavy window (more than 3072 tuples where the mean is 2048: keys in thousands of reads); small inputs get the
        // worst case (every tuple in one window), big ones an eighth of it
        { const u64 whCap = n <= (64u << 20) ? nAlloc : nAlloc / 8; WS(whs, u64, WS_WHERE, whCap); A.wh = whs; A.wh_cap = whCap; }
        hipLaunchKernelGGL(k_ix_window, dim3((unsigned)std::min<u64>(nW, 256ull * 6)), dim3(IXW_T), 0, d->stream, A);      // persistent: two rounds of 3 workgroups per CU, each with ONE pair of statistics atomics
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c, d->d_counters + CTR_INDEX, sizeof c, hipMemcpyDeviceToHost, d->stream));
        u64 c9 = 0; HIPCHK(hipMemcpyAsync(&c9, d->d_counters + CTR_INDEX + 9, sizeof c9, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
        lap("table windows"); mem_sample(d);
        if (c[8] && (c[8] & 0xFFFFFull) == 0 && (c[8] >> 40) == 0 && ixCntBits == (u32)IXW_CNT_BITS_DEFAULT) {      // only the per-key counter ran over: again, with 30 bits of count
            if (timing) fprintf(stderr, "[index] a key occurs in more than 2^20 reads: building again with the wide counter split\n");
            ixCntBits = (u32)IXW_CNT_BITS_WIDE; attempt--; continue; }
        if (c[8]) { char b_[256]; snprintf(b_, sizeof b_, "index build: %llu table windows overflowed, %llu keys occur in more than 2^30 reads, %llu heavy windows found no scratch (cursor %llu of %llu)",
                             (unsigned long long)(c[8] & 0xFFFFF), (unsigned long long)((c[8] >> 20) & 0xFFFFF), (unsigned long long)(c[8] >> 40), (unsigned long long)c9, (unsigned long long)A.wh_cap);
                    err = b_; return SAGE2OV_ERR_LIMIT; }
        if (c[2] > big_cap) { err = "too many long buckets"; return SAGE2OV_ERR_LIMIT; }
        if (c[2]) {
            hipLaunchKernelGGL(k_index_purity, dim3(grid_for(c[2] * 64, 256)), dim3(256), 0, d->stream, d->readsLoc, d->S, d->h, big, c[2], d->csr, d->d_counters + CTR_INDEX);
            HIPCHK(hipMemcpyAsync(c, d->d_counters + CTR_INDEX, 5 * sizeof(u64), hipMemcpyDeviceToHost, d->stream));
            HIPCHK(hipStreamSynchronize(d->stream));
        }
        if (c[3] == 0) { d->n_csr = c[0]; d->n_keys = c[1]; d->n_long = c[2];
            // ---- stage B: the group tuples sorted by the window of their group word, the windows of the group table built in LDS
            d->mi1 = nullptr; d->krec = nullptr; d->TL = 0; d->n_groups = 0;
            if (wantMI && d->n_keys > 0) {
                const u32 nG = n;                                        // one group tuple per entry tuple position; those without a record (GT_INVALID) sort behind window gW - 1
                PtBufs G; G.W = 3; G.E[0] = B.E[cur ^ 1]; G.E[1] = B.E[cur];                                // (the entry tuples are no longer needed)
                int gcur = 0; const int gshift = 31 - (tlBits - IX_GWLOG);                                  // keys are minimiser hashes >> 1
                { int rc = partition_by_window(d, G, 0, nG, gshift, gW + 1, false, cnt, base, gOff, &gcur, err); if (rc) return rc; }
                lap("partition by group window");
                MiWinArgs MA; MA.G = G.E[gcur]; MA.gOff = gOff; MA.gW = (u32)gW; MA.tlBits = tlBits; MA.mi1 = mi1; MA.krec = krec; MA.counters = d->d_counters + CTR_INDEX; MA.wh = A.wh; MA.wh_cap = A.wh_cap;
                HIPCHK(hipMemsetAsync(d->d_counters + CTR_INDEX + 9, 0, sizeof(u64), d->stream));                  // (the scratch cursor starts over)
                hipLaunchKernelGGL(k_mi_window, dim3((unsigned)std::min<u64>(gW, 256ull * 8)), dim3(256), 0, d->stream, MA);
                // the probe scan may run past the last group: empty records behind ALL records
                u64 mc[3];
                HIPCHK(hipMemcpyAsync(mc, d->d_counters + CTR_INDEX + 5, sizeof mc, hipMemcpyDeviceToHost, d->stream));
                HIPCHK(hipStreamSynchronize(d->stream));
                HIPCHK(hipMemsetAsync(krec + mc[0], 0, MI_SCAN_PAD * sizeof(u64), d->stream));   // (mc[0] records, at krec[0 .. mc[0]))
                lap("group windows"); mem_sample(d);
                d->n_groups = mc[1];
                if (d->opt.get("SAGE2OV_VERIFY_MI")) {
                    u64* vo = nullptr; HIPCHK(hipMalloc(&vo, 2 * sizeof(u64))); HIPCHK(hipMemsetAsync(vo, 0, 2 * sizeof(u64), d->stream));
                    hipLaunchKernelGGL(k_mi_verify, dim3(grid_for(4 * N, 256)), dim3(256), 0, d->stream, d->readsLoc, N, d->S, d->h, d->seed, d->slots, d->T, mi1, TL, krec, vo);
                    u64 hv2[2]; HIPCHK(hipMemcpyAsync(hv2, vo, sizeof hv2, hipMemcpyDeviceToHost, d->stream)); HIPCHK(hipStreamSynchronize(d->stream)); hipFree(vo);
                    fprintf(stderr, "[verify-mi] %llu of %llu entries do not find their bucket in their key's group\n", (unsigned long long)hv2[0], (unsigned long long)hv2[1]);
                }
                if (mc[2] == 0 && mc[1] * 10 <= TL * 7) { d->mi1 = mi1; d->krec = krec; d->TL = TL; }   // else: too crowded, the fast kernel uses the uniform table
                if (timing) fprintf(stderr, "[index] minimiser groups: %llu groups, %llu records, %llu group words (load %.2f), crowded windows %llu -> %s\n", (unsigned long long)mc[1], (unsigned long long)mc[0],
                                    (unsigned long long)TL, (double)mc[1] / (double)TL, (unsigned long long)mc[2], d->mi1 ? "used" : "NOT used");
            }
            break;
        }
        if (attempt >= 8) { err = "index build: tag collisions in long buckets persist after 8 reseeds"; return SAGE2OV_ERR_INTERNAL; }
        d->seed = d->seed * 0x9E3779B97F4A7C15ull + 12345; (*rebuilds)++;
    }
    HIPCHK(hipEventRecord(d->ev[1], d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    float ms = 0; hipEventElapsedTime(&ms, d->ev[0], d->ev[1]); d->tm.index_ms += ms;
    if (d->diet) ph_begin(d);                                                 // phase B: the sort's buffers (~150 bytes per read) go, the step's results come
    *slots_out = d->T; *keys_out = d->n_keys; *csr_out = d->n_csr; *nlong_out = d->n_long;
    return 0;
}

int dev_lookup(Device* d, uint64_t hi, uint64_t lo, uint64_t* entries, uint32_t cap, uint32_t* count, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (!d->slots) { err = "index not built"; return SAGE2OV_ERR_ARG; }
    u64* out = nullptr; const u32 c2 = std::min<u32>(cap, 128);
    HIPCHK(hipMalloc(&out, (129) * sizeof(u64)));
    hipLaunchKernelGGL(k_lookup, dim3(1), dim3(1), 0, d->stream, d->slots, d->T, d->csr, d->idOf, d->seed, d->h, (u64)hi, (u64)lo, out, c2);
    u64 host[129];
    HIPCHK(hipMemcpyAsync(host, out, sizeof host, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    hipFree(out);
    *count = (u32)host[0];
    for (u32 x = 0; x < *count && x < c2; x++) entries[x] = host[1 + x];
    return 0;
}

template <int MODE>
static int launch_probe(Device* d, ProbeArgs& A, std::string& err) {
    const u64 nreads = A.ids ? A.n_ids : A.hi - A.lo; if (nreads == 0) return 0;
    // one wave per read, 4 waves per block (2 for the 16-word layout, 1 for the 32-word layout: LDS); enough blocks to fill
    // 256 CUs several times over, grid-stride beyond
    const unsigned wpb = d->S == 32 ? 1 : (d->S == 16 ? 2 : 4);
    const unsigned blocks = (unsigned)std::min<u64>((nreads + wpb - 1) / wpb, 256ull * 32);
    switch (d->S) {
        case 4: hipLaunchKernelGGL((k_probe<4, MODE, 4>), dim3(blocks), dim3(256), 0, d->stream, A); break;
        case 8: hipLaunchKernelGGL((k_probe<8, MODE, 4>), dim3(blocks), dim3(256), 0, d->stream, A); break;
        case 16: hipLaunchKernelGGL((k_probe<16, MODE, 2>), dim3(blocks), dim3(128), 0, d->stream, A); break;
        case 32: hipLaunchKernelGGL((k_probe<32, MODE, 1>), dim3(blocks), dim3(64), 0, d->stream, A); break;     // 505 .. 1018 bases: 34 KB of LDS per wave
        default: err = "bad S"; return SAGE2OV_ERR_INTERNAL;
    }
    HIPCHK(hipGetLastError());
    return 0;
}
static ProbeArgs base_args(Device* d) {
    ProbeArgs A; memset(&A, 0, sizeof A);
    A.reads = d->readsLoc; A.idOf = d->idOf; A.statusP = d->statusP; A.meta = d->metaP; A.N = d->N; A.S = d->S; A.k = d->k; A.h = d->h; A.slots = d->slots; A.T = d->T; A.csr = d->csr; A.seed = d->seed;
    A.right = d->right; A.left = d->left; A.conn = d->conn; A.cflag = d->cflag; A.counters = d->d_counters;
    A.mi1 = d->mi1; A.TL = d->TL; A.krec = d->krec; A.uniL = d->uniL;
    A.chunkShift = (u32)FAST_CHUNK_LOG;      // (plan_fast_grid may double the positions per block visit)
    A.noRun = d->opt.get("SAGE2OV_NO_RUN_MODE") ? 1u : 0u; A.noParTail = d->opt.get("SAGE2OV_NO_PAR_TAIL") ? 1u : 0u;
    // (run mode with a lane per read: RUN_LANES_MIN; the switches are for the tests -- every setting gives the same records)
    A.runLanesMin = d->opt.num("SAGE2OV_RUN_LANES", 1) == 0 ? 0u : (u32)std::max<long long>(1, std::min<long long>(RUN_MMAX + 1, d->opt.num("SAGE2OV_RUN_LANES_MIN", RUN_LANES_MIN)));
    return A;
}

template <int S, int NW, int WPL, int WPB, int HITS, int TAIL>
static void launch_fast(Device* d, ProbeArgs& A, unsigned blocks) {
    if constexpr (HITS == 0 && TAIL == 0 && NW <= 10) {               // the clean-data form has an instantiation for read sets of ONE length (no per-candidate length registers)
        if (A.uniL) { hipLaunchKernelGGL((k_probe_fast<S, NW, WPL, WPB, HITS, TAIL, true>), dim3(blocks), dim3(64 * WPB), 0, d->stream, A); return; }
    }
    hipLaunchKernelGGL((k_probe_fast<S, NW, WPL, WPB, HITS, TAIL, false>), dim3(blocks), dim3(64 * WPB), 0, d->stream, A);
}
// The sequential-groups form of the clean-data kernel (k_probe_fast<..., UNI, QN, SEQ>): read sets of one length in the 4- and 8-word layouts only; qn = 2 (128 candidates,
// as the standard form) or 4 (256: the reads of high-coverage data the standard form lists).  false: no such instantiation for these reads.
static bool launch_fast_seq_any(Device* d, ProbeArgs& A, unsigned blocks, int qn) {
    constexpr int FW = FAST_WPB;
    const int nwinMax = d->maxL - d->h + 1;
    if (!d->uniL || nwinMax > 128) return false;
    if (d->S == 4) { if (qn == 4) hipLaunchKernelGGL((k_probe_fast<4, 8, 2, FW, 0, 0, true, 4, true>), dim3(blocks), dim3(64 * FW), 0, d->stream, A);
                     else hipLaunchKernelGGL((k_probe_fast<4, 8, 2, FW, 0, 0, true, 2, true>), dim3(blocks), dim3(64 * FW), 0, d->stream, A); return true; }
    if (d->S == 8 && d->maxL <= 160) { if (qn == 4) hipLaunchKernelGGL((k_probe_fast<8, 10, 2, FW, 0, 0, true, 4, true>), dim3(blocks), dim3(64 * FW), 0, d->stream, A);
                                       else hipLaunchKernelGGL((k_probe_fast<8, 10, 2, FW, 0, 0, true, 2, true>), dim3(blocks), dim3(64 * FW), 0, d->stream, A); return true; }
    return false;
}
// picks the instantiation for the resident reads; false: the 32-word layout (505 .. 1018 bases) has no fast kernel
template <int HITS, int TAIL>
static bool launch_fast_any(Device* d, ProbeArgs& A, unsigned blocks) {
    constexpr int FW = FAST_WPB;      // waves per block: a whole CU's worth works on one locality chunk
    const int nwinMax = d->maxL - d->h + 1;                               // windows of the longest read
    if (d->S == 4 && nwinMax <= 128) launch_fast<4, 8, 2, FW, HITS, TAIL>(d, A, blocks);
    else if (d->S == 8 && d->maxL <= 160 && nwinMax <= 128) launch_fast<8, 10, 2, FW, HITS, TAIL>(d, A, blocks);
    else if (d->S == 8 && d->maxL <= 160) launch_fast<8, 10, 3, 4, HITS, TAIL>(d, A, blocks);       // 129..160 windows, e.g. 150-bp reads with k <= 22 (three waves per SIMD: blocks of four)
    // (the 16-dword layout's state-machine rows take 12 KB of LDS per wave: four waves per block keep three blocks on a CU)
    else if (d->S == 8 && nwinMax <= 128) launch_fast<8, 16, 2, ((HITS || !TAIL) ? FW : 4), HITS, TAIL>(d, A, blocks);
    else if (d->S == 8) launch_fast<8, 16, 4, ((HITS || !TAIL) ? FW : 4), HITS, TAIL>(d, A, blocks);
    // 16-word layout (252 .. 504 bases, round 3): 20-dword compares and five windows per lane up to 320 bases / 320 windows (2 x 300 MiSeq reads), 32-dword
    // compares and eight windows per lane beyond; blocks of four waves (the state machine's rows take 10 / 18 KB of LDS per wave)
    else if (d->S == 16 && d->maxL <= 320 && nwinMax <= 320) launch_fast<16, 20, 5, 4, HITS, TAIL>(d, A, blocks);
    else if (d->S == 16 && nwinMax <= 512) launch_fast<16, 32, 8, 4, HITS, TAIL>(d, A, blocks);
    else return false;
    return true;
}
// The forms of the fast kernel that the passes ask for:
//   Clean  TAIL = 0: inconsistent reads and reads with more candidates than slots are listed; the sequential-groups form where it exists (eight waves per SIMD:
//          -2.4 % at configs[2]), unless SAGE2OV_PROBE_SEQ=0
//   Wide   the sequential-groups form with 256 candidate slots (QN = 4), no state machine
//   Tail1  TAIL = 1: the state machine for inconsistent reads          Tail2  TAIL = 2: every read through the state machine
//   Hits   the hit-list form of the reduce phase (HITS = 1)
enum class Form { Clean, Wide, Tail1, Tail2, Hits };
// false: the resident layout has no instantiation of that form (nothing was launched)
static bool launch_form(Device* d, Form f, ProbeArgs& A, unsigned blocks) {
    switch (f) {
        case Form::Clean: {
            const char* ev = d->opt.get("SAGE2OV_PROBE_SEQ");
            return ((!ev || atoi(ev) != 0) && launch_fast_seq_any(d, A, blocks, 2)) || launch_fast_any<0, 0>(d, A, blocks);
        }
        case Form::Wide: return launch_fast_seq_any(d, A, blocks, 4);
        case Form::Tail1: return launch_fast_any<0, 1>(d, A, blocks);
        case Form::Tail2: return launch_fast_any<0, 2>(d, A, blocks);
        case Form::Hits: return launch_fast_any<1, 0>(d, A, blocks);
    }
    return false;
}
// The grid of the fast kernel.  Every block walks its chunks in a fixed round-robin order and is resident until its slowest wave is done, so the grid's granularity
// decides how long CUs idle at the end of the launch.  Measured at BASELINE configs[2] (round 3, uniform grids, blocks per CU -> kernel ms): 4 -> 92.2, 8 -> 90.8, 16 -> 89.6
// (rounds 1-2), 32 -> 88.7, 64 -> 88.0, 256 -> 88.4, one chunk per block -> 93.2 (a block's start and drain cost ~5 us).  Hence a TAPERED grid: up to three phases of 4096
// blocks that take 3/4 of what is left each (60 / 15 / ... rounds at configs[2]), then the rest in blocks of a few chunks -- the blocks the hardware dispatches last are short.
// Launches that write hits out reserve a 2048-slot chunk of the hit buffer per wave at a time: they keep one phase of 16 blocks per CU, or the buffer's slack quadruples.
// SAGE2OV_TEST_PHASE_BLOCKS=<b>: phases of b blocks instead of 4096 (tests: several phases on a few thousand reads).
static unsigned plan_fast_grid(const Options& O, ProbeArgs& A, u64 n, bool writesHits = false) {
    const char* ep = O.get("SAGE2OV_TEST_PHASE_BLOCKS"); const u64 PB = ep ? (u64)std::max(1, atoi(ep)) : 4096;
    memset(A.phase, 0, sizeof A.phase);
    // positions per block visit: twice FAST_CHUNK for launches big enough that the coarser grid does not show (kernels_probe_fast.inc: 24 M positions and more;
    // SAGE2OV_FAST_CHUNK_SHIFT = 7 / 8 overrides); launches that write hits out keep the small size
    u32 cs = (u32)FAST_CHUNK_LOG + ((n >= 24000000ull && !writesHits) ? 1u : 0u);
    if (const char* ec = O.get("SAGE2OV_FAST_CHUNK_SHIFT")) cs = (u32)std::max(FAST_CHUNK_LOG, std::min(FAST_CHUNK_LOG + 3, atoi(ec)));
    A.chunkShift = cs;
    const u64 CH = 1ull << cs, C = (n + CH - 1) / CH;
    if (writesHits || C <= PB * 8) {
        const u64 nb = std::max<u64>(1, std::min<u64>(C, 256ull * 16));
        A.phase[0][0] = 0; A.phase[0][1] = (u32)nb; A.phase[0][2] = (u32)((C + nb - 1) / nb); A.phase[0][3] = 0;
        return (unsigned)nb;
    }
    u64 rem = C, chunk0 = 0, block0 = 0; int p = 0;
    for (; p < 3 && rem > PB * 8; p++) {
        const u64 r = rem * 3 / 4 / PB;
        A.phase[p][0] = (u32)block0; A.phase[p][1] = (u32)PB; A.phase[p][2] = (u32)r; A.phase[p][3] = (u32)chunk0;
        block0 += PB; chunk0 += PB * r; rem -= PB * r;
    }
    const u64 nb = std::min<u64>(rem, 2 * PB);
    A.phase[p][0] = (u32)block0; A.phase[p][1] = (u32)nb; A.phase[p][2] = (u32)((rem + nb - 1) / nb); A.phase[p][3] = (u32)chunk0;
    return (unsigned)(block0 + nb);
}

// the run counters of the last dev_probe (CTR_RUNSTATS)
int dev_probe_run_stats(Device* d, uint64_t out[4], std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    u64 c[4]; { int rc = read_counters(d, CTR_RUNSTATS, 4, c, err); if (rc) return rc; }
    for (int x = 0; x < 4; x++) out[x] = c[x];
    return 0;
}
// which way the last dev_reduce_device went: the words of sage2ov_reduce_stats_get (form 0 when it left the phase to the caller's replay)
void dev_reduce_stats(Device* d, uint64_t out[SAGE2OV_REDUCE_STATS]) { for (int x = 0; x < SAGE2OV_REDUCE_STATS; x++) out[x] = d->reduceStats[x]; }
void dev_set_probe_share(Device* d, double share) { d->probeShare = share; }
bool dev_has_minimiser_groups(Device* d) { return d->mi1 != nullptr && d->TL != 0; }

// What dev_probe runs, decided on the host (no device calls).  The TAIL = 1 form is 10 % slower on every read, and on error-free data a read in a thousand
// needs it.  So the first 1/128 of the range (nsample) runs the clean form, which lists such reads; the share it listed picks the main form for the rest
// (plan_after_sample).  The listed reads then go through the passes over the list: the wide form when there are many (high coverage:
// tests/diag/coverage_sweep.py), the TAIL = 1 form, and what that cannot settle either (more than 128 candidates, overhangs beyond its rows) ends in the
// sequential kernel.
struct ProbePlan {
    u64 nsample = 0;          // reads of the sample pass at the start of the range (0: no sample, the main pass takes the whole range)
    Form main = Form::Tail1;  // the main pass's form (Wide: the clean form where the layout has no wide one)
    bool listed = false;      // the main pass lists reads for the passes over the list
    bool wide = false;        // ... and the wide pass runs over the list first when it holds wideMin reads or more
    u64 wideMin = 4096;
};
static void plan_wide_pass(const Options& O, int uniL, ProbePlan& P) {
    P.wide = P.listed && P.main != Form::Tail2 && P.main != Form::Wide && uniL != 0 && !O.get("SAGE2OV_NO_WIDE");
    if (const char* ev = O.get("SAGE2OV_PROBE_WIDE_MIN")) P.wideMin = strtoull(ev, nullptr, 10);
}
static ProbePlan plan_probe(const Options& O, int uniL, u64 nreads) {
    ProbePlan P;
    const char* evs = O.get("SAGE2OV_PROBE_SAMPLE_MIN");                       // tests: sample on small inputs too
    const u64 sampleMin = evs ? strtoull(evs, nullptr, 10) : (128u << 10);
    const char* evt = O.get("SAGE2OV_PROBE_TAIL");                             // "0" / "1" / "2": no sample, that form for everything
    u64 ns = (nreads >= 4 * sampleMin && !evt) ? std::max<u64>(nreads / 128, sampleMin) : 0;      // (on noisy data the sample is work done twice)
    ns = (ns + 2 * FAST_CHUNK - 1) / (2 * FAST_CHUNK) * (2 * FAST_CHUNK);
    P.nsample = ns < nreads ? ns : 0;
    const int tail = evt ? atoi(evt) : 1;
    P.main = tail == 2 ? Form::Tail2 : (tail == 1 ? Form::Tail1 : Form::Clean);
    P.listed = evt && tail == 0;
    plan_wide_pass(O, uniL, P);
    return P;
}
// The sample listed `listed` reads, `capped` of them for having more candidates than slots.  Inconsistent reads: more than half -> the state machine for every
// read; more than 1/32 -> the form that carries it.  Capped reads, more than 1/32 (one-length read sets): the rest runs the wide form right away instead of
// listing a fifth of the reads again.
static void plan_after_sample(const Options& O, int uniL, ProbePlan& P, u64 listed, u64 capped) {
    const u64 ns = P.nsample, nInc = listed - std::min(listed, capped);
    P.main = nInc * 2 > ns ? Form::Tail2 : (nInc * 32 > ns ? Form::Tail1 : Form::Clean);
    if (P.main == Form::Clean && capped * 32 > ns && uniL != 0 && !O.get("SAGE2OV_NO_WIDE")) P.main = Form::Wide;
    P.listed = true;
    plan_wide_pass(O, uniL, P);
}

int dev_probe(Device* d, uint64_t lo, uint64_t hi, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (!d->slots) { err = "index not built"; return SAGE2OV_ERR_ARG; }
    const u64 N = d->N;
    { int rc = ensure_results(d, err); if (rc) return rc; }
    HIPCHK(hipEventRecord(d->ev[0], d->stream));
    HIPCHK(hipMemsetAsync(d->right, 0, (N + 1) * sizeof(u64), d->stream)); HIPCHK(hipMemsetAsync(d->left, 0, (N + 1) * sizeof(u64), d->stream));
    HIPCHK(hipMemsetAsync(d->conn, 0, (N + 1) * sizeof(u32), d->stream)); HIPCHK(hipMemsetAsync(d->cflag, 0, (N + 1) * sizeof(u32), d->stream));
    HIPCHK(hipMemsetAsync(d->d_counters + CTR_HANDED, 0, 2 * sizeof(u64), d->stream));
    HIPCHK(hipMemsetAsync(d->d_counters + CTR_RUNSTATS, 0, 4 * sizeof(u64), d->stream));
    ProbeArgs A = base_args(d); A.lo = lo; A.hi = hi;
    const u64 nreads = hi > lo ? hi - lo : 0;
    d->pre.valid = false;
    if (nreads) {
        WS(slow, u32, WS_SLOW, nreads);
        A.slow = slow; A.slow_cap = nreads;
        // (positions [lo, hi) of the locality order: consecutive items are neighbours in the genome AND in the read store)
#ifdef SAGE2OV_STAMPS
        static u64* d_stamps = nullptr;
        if (!d_stamps) HIPCHK(hipMalloc(&d_stamps, 32 * sizeof(u64)));
        HIPCHK(hipMemsetAsync(d_stamps, 0, 32 * sizeof(u64), d->stream)); A.stamps = d_stamps;
#endif
        ProbePlan P = plan_probe(d->opt, d->uniL, nreads);
        float kms = 0;
        // noisy data, and this context probes every read: the hits of the unresolved reads ARE the verified hits of this pass -- written out
        // now (the main pass in its TAIL = 2 form, with hitBase), filtered by the final statuses in the reduce phase (k_hits_filter)
        const bool prehits = d->probeShare == 1.0 && lo == 1 && hi == N + 1 && !d->opt.get("SAGE2OV_NO_PREHITS");
        struct FastPass { bool launched = false; u64 listed = 0, capped = 0; };
        // One timed pass of the fast kernel in form f over B's range or id list of n reads: its grid, the launch between two events, what it listed
        // (CTR_HANDED).  The main pass: its wide form falls back to the clean one, its TAIL = 2 form writes the hits out (prehits).
        auto pass = [&](Form f, ProbeArgs& B, u64 n, bool mainPass, FastPass& r) -> int {
            const unsigned nb = plan_fast_grid(d->opt, B, n, f == Form::Tail2);
            bool armed = false;
            if (mainPass && f == Form::Tail2 && prehits) {
                const u64 hcap = n * 72 + (u64)nb * FAST_WPB * HITS_CHUNK;
                Hit* hb = (Hit*)ws_get(d, WS_HITS, hcap * sizeof(Hit));                  // (72 hits per read: 49 GB at 42 M reads -- no room: the reduce phase makes its own lists)
                if (!hb) (void)hipGetLastError();
                else {
                    WS(hbase, u64, WS_PRE_BASE, N + 2); WS(hcnt, u32, WS_RA_CUR, N + 2);
                    HIPCHK(hipMemsetAsync(hbase, 0xFF, (N + 2) * sizeof(u64), d->stream)); HIPCHK(hipMemsetAsync(hcnt, 0, (N + 2) * sizeof(u32), d->stream));
                    HIPCHK(hipMemsetAsync(d->d_counters + CTR_HIT_CURSOR, 0, 2 * sizeof(u64), d->stream));      // (and CTR_HIT_REAL)
                    B.hits = hb; B.hits_cap = hcap; B.hitBase = hbase; B.hitcount = hcnt; armed = true;
                    d->pre.hits = hb; d->pre.cap = hcap; d->pre.base = hbase;
                }
            }
            HIPCHK(hipEventRecord(d->ev[2], d->stream));
            r.launched = launch_form(d, f, B, nb) || (mainPass && f == Form::Wide && launch_form(d, Form::Clean, B, nb));
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(d->ev[3], d->stream));
            u64 c[2]; { int rc = read_counters(d, CTR_HANDED, 2, c, err); if (rc) return rc; } r.listed = c[0]; r.capped = c[1];
            float ms = 0; hipEventElapsedTime(&ms, d->ev[2], d->ev[3]); kms += ms; d->tm.probe_fast_launches++;      // (counted even when nothing was launched)
            if (d->opt.get("SAGE2OV_TIMING")) fprintf(stderr, "[probe] fast kernel launch %.3f ms, listed so far %llu\n", ms, (unsigned long long)r.listed);
            if (armed && r.launched) {
                u64 used = 0; { int rc = read_counters(d, CTR_HIT_CURSOR, 1, &used, err); if (rc) return rc; }
                d->pre.used = used; d->pre.valid = used <= d->pre.cap;                  // (a chunk beyond the buffer: hits were dropped, the reduce phase makes its own lists)
            }
            return 0;
        };
        // a pass over the listed reads (slow): what it cannot settle in turn is listed in WS_SLOW2
        u32* list = slow; u64 nslow = 0;
        auto list_pass = [&](Form f, u32** out, FastPass& r) -> int {
            WS(slow2, u32, WS_SLOW2, nslow);
            HIPCHK(hipMemsetAsync(d->d_counters + CTR_HANDED, 0, 2 * sizeof(u64), d->stream));
            ProbeArgs B = base_args(d); B.ids = slow; B.n_ids = nslow; B.slow = slow2; B.slow_cap = nslow;
#ifdef SAGE2OV_STAMPS
            if (f == Form::Tail1) B.stamps = A.stamps;
#endif
            *out = slow2;
            return pass(f, B, nslow, false, r);
        };
        bool launched = false;
        {
            FastPass r;
            if (P.nsample) {
                ProbeArgs As = A; As.hi = lo + P.nsample;
                { int rc = pass(Form::Clean, As, P.nsample, false, r); if (rc) return rc; }
                launched = r.launched;
                if (launched) {
                    plan_after_sample(d->opt, d->uniL, P, r.listed, r.capped);
                    ProbeArgs Ar = A; Ar.lo = lo + P.nsample;
                    int rc = pass(P.main, Ar, nreads - P.nsample, true, r); if (rc) return rc;
                }
            } else {
                ProbeArgs Aw = A;
                int rc = pass(P.main, Aw, nreads, true, r); if (rc) return rc;
                launched = r.launched;
            }
            nslow = r.listed;
        }
        if (!launched) {                                                       // 32-word layout: no fast form, the sequential kernel for every read
            HIPCHK(hipEventRecord(d->ev[2], d->stream));
            int rc = launch_probe<0>(d, A, err); if (rc) return rc;
            HIPCHK(hipEventRecord(d->ev[3], d->stream)); HIPCHK(hipStreamSynchronize(d->stream));
            float ms = 0; hipEventElapsedTime(&ms, d->ev[2], d->ev[3]); kms += ms; nslow = 0;
        } else {
            if (P.wide && nslow >= P.wideMin) {                                   // many listed: the wide form first; the survivors' list becomes the list
                u32* slow2 = nullptr; FastPass r; { int rc = list_pass(Form::Wide, &slow2, r); if (rc) return rc; }
                if (r.launched) { nslow = r.listed; if (nslow) HIPCHK(hipMemcpyAsync(slow, slow2, nslow * sizeof(u32), hipMemcpyDeviceToDevice, d->stream)); }
            }
            if (P.listed && nslow) {                                              // the state machine, in the TAIL = 1 form
                FastPass r; { int rc = list_pass(Form::Tail1, &list, r); if (rc) return rc; }
                nslow = r.listed;
            }
        }
        d->tm.probe_kernel_ms += kms; d->tm.probe_launches++;
        d->tm.slow_reads += nslow;
#ifdef SAGE2OV_STAMPS
        { u64 st[32]; HIPCHK(hipMemcpy(st, d_stamps, sizeof st, hipMemcpyDeviceToHost)); u64 tot = 0; for (int x = 0; x < 24; x++) if (x < 10 || x >= 14) tot += st[x];
          // stages 0-9 in order of the code; 16 = slot -> window -> entry (before the gathers), 17 = reach, 18 = broadcast of the speculated reads, 19 = compares (8 = what follows them)
          fprintf(stderr, "[stamps] kernel %.2f ms; share of wave cycles (cycles per read):", kms); for (int x = 0; x < 24; x++) if (x < 10 || x >= 14) fprintf(stderr, " %d:%.1f%% (%.0f)", x, 100.0 * (double)st[x] / (double)tot, st[10] ? (double)st[x] / (double)st[10] : 0.0);
          fprintf(stderr, "; window reuse: %llu of %llu reads (same minimiser strand as the previous read: %llu), mean shift %.1f\n", (unsigned long long)st[11], (unsigned long long)st[10], (unsigned long long)st[13], st[11] ? (double)st[12] / (double)st[11] : 0.0);
          fprintf(stderr, "[stamps] run mode: %llu reads off the frame, %llu runs ended on a read the general path took; strand changes carried over by mirroring the ring: %llu (refused: %llu -- too far %llu, own entry not in the ring %llu, a window with one read twice %llu), steps: %llu\n", (unsigned long long)st[24], (unsigned long long)st[25], (unsigned long long)st[26], (unsigned long long)st[27], (unsigned long long)st[29], (unsigned long long)st[30], (unsigned long long)st[31], (unsigned long long)st[28]); }
#endif
        if (nslow) {                                                          // the end of the cascade: what is still listed, in the sequential state machine
            ProbeArgs B = base_args(d); B.ids = list; B.n_ids = nslow;
            int rc = launch_probe<0>(d, B, err); if (rc) return rc;
        }
    }
    HIPCHK(hipEventRecord(d->ev[1], d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    float ms = 0; hipEventElapsedTime(&ms, d->ev[0], d->ev[1]); d->tm.probe_ms += ms;
    mem_sample(d);
    return 0;
}

// The wire form of a read's record, 16 bytes (24 until the end of round 3: the record all-gather is the largest exchange of a multi-GPU step).  Exact because a
// position is < 2^30 (the context's limit), an extension length < 2^22, the flags are two bits, and the connection count is at most (windows of a read) x (bucket cap
// of 101 entries, hashTable.cpp:178) < 2^18:   w0 = right pos:30 | type:2 | len:22 | flags:2 | conn[7:0]:8      w1 = left pos:30 | type:2 | len:22 | conn[17:8]:10
struct Record { u64 w0, w1; };
__device__ __forceinline__ u64 rec_half(u64 e) { return (e & 0x3FFFFFFFull) | (((e >> 40) & 3ull) << 30) | (((e >> 42) & 0x3FFFFFull) << 32); }
__device__ __forceinline__ u64 rec_entry(u64 w) { return (w & 0x3FFFFFFFull) | (((w >> 30) & 3ull) << 40) | (((w >> 32) & 0x3FFFFFull) << 42); }
// (a rank probes a range of POSITIONS of the locality order; since round 3 the per-read arrays are indexed by position too and name neighbours by position --
//  every rank computes the same order -- so a rank's records are a contiguous slice)
__global__ void k_pack_records(u64 lo, u64 hi, const u64* right, const u64* left, const u32* conn, const u32* cflag, Record* out) {
    u64 p = lo + (u64)blockIdx.x * blockDim.x + threadIdx.x; if (p >= hi) return;
    const u32 c = min(conn[p], (1u << 18) - 1u), f = cflag[p] & 3u;
    Record r; r.w0 = rec_half(right[p]) | ((u64)f << 54) | ((u64)(c & 0xFFu) << 56); r.w1 = rec_half(left[p]) | ((u64)(c >> 8) << 54); out[p - lo] = r;
}
__global__ void k_unpack_records(u64 first, u64 n, const Record* in, u64* right, u64* left, u32* conn, u32* cflag) {
    u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (x >= n) return;
    Record r = in[x]; const u64 p = first + x; right[p] = rec_entry(r.w0); left[p] = rec_entry(r.w1); conn[p] = (u32)(r.w0 >> 56) | ((u32)(r.w1 >> 54) << 8);
    cflag[p] |= (u32)(r.w0 >> 54) & 3u;   // containment marks (economyGraph.cpp:735) are OR-ed, never overwritten: the local probe may have marked this read too
}
// containment flags travel as two byte planes (bit0 plane, bit1 plane) so that a MAX all-reduce is a bitwise OR
__global__ void k_flags_export(u64 n, const u32* __restrict__ cflag, uint8_t* out) {
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
    u32 f = cflag[i]; out[i] = f & 1u; out[n + i] = (f >> 1) & 1u;
}
__global__ void k_flags_import(u64 n, const uint8_t* __restrict__ in, u32* cflag) {
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
    cflag[i] = (in[i] ? 1u : 0u) | (in[n + i] ? 2u : 0u);
}
int dev_export_flags(Device* d, void* dst, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    hipLaunchKernelGGL(k_flags_export, dim3(grid_for(d->N + 1, 256)), dim3(256), 0, d->stream, (u64)(d->N + 1), d->cflag, (uint8_t*)dst);
    HIPCHK(hipStreamSynchronize(d->stream)); return 0;
}
int dev_import_flags(Device* d, const void* src, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    hipLaunchKernelGGL(k_flags_import, dim3(grid_for(d->N + 1, 256)), dim3(256), 0, d->stream, (u64)(d->N + 1), (const uint8_t*)src, d->cflag);
    HIPCHK(hipStreamSynchronize(d->stream)); return 0;
}
uint64_t dev_cand_count(Device* d) { return d->n_cand; }
int dev_export_cands(Device* d, void* dst, uint64_t cap, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (d->n_cand > cap) { err = "candidate export buffer too small"; return SAGE2OV_ERR_ARG; }
    if (d->n_cand) HIPCHK(hipMemcpyAsync(dst, d->cand, d->n_cand * sizeof(EdgeCand), hipMemcpyDeviceToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream)); return 0;
}
int dev_set_cands(Device* d, const void* src, uint64_t n, std::string& err) {      // replace the candidate list (device source)
    HIPCHK(hipSetDevice(d->ordinal));
    if (n > d->cand_cap) { int rc = cand_resize(d, n + 1024, 0, err); if (rc) return rc; }
    if (n) HIPCHK(hipMemcpyAsync(d->cand, src, n * sizeof(EdgeCand), hipMemcpyDeviceToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream)); d->n_cand = n; return 0;
}
// survivor buckets of a sharded reduce phase: candidates [first, first + n) of the list (what this rank's marks re-emitted)
int dev_export_cand_range(Device* d, void* dst, uint64_t first, uint64_t n, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (first + n > d->n_cand) { err = "candidate range out of bounds"; return SAGE2OV_ERR_ARG; }
    if (n) HIPCHK(hipMemcpyAsync(dst, d->cand + first, n * sizeof(EdgeCand), hipMemcpyDeviceToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream)); return 0;
}
// the list becomes its first `keep` candidates followed by the n candidates at src (device memory)
int dev_replace_cand_tail(Device* d, uint64_t keep, const void* src, uint64_t n, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (keep > d->n_cand) { err = "candidate range out of bounds"; return SAGE2OV_ERR_ARG; }
    if (keep + n > d->cand_cap) {
        HIPCHK(hipStreamSynchronize(d->stream));
        { int rc = cand_resize(d, keep + n + 1024, keep, err); if (rc) return rc; }
    }
    if (n) HIPCHK(hipMemcpyAsync(d->cand + keep, src, n * sizeof(EdgeCand), hipMemcpyDeviceToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream)); d->n_cand = keep + n; return 0;
}
int dev_export_records(Device* d, void* dst, uint64_t lo, uint64_t hi, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (hi > lo) hipLaunchKernelGGL(k_pack_records, dim3(grid_for(hi - lo, 256)), dim3(256), 0, d->stream, (u64)lo, (u64)hi, d->right, d->left, d->conn, d->cflag, (Record*)dst);
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}
int dev_import_records(Device* d, const void* src, uint64_t first, uint64_t n, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (n) hipLaunchKernelGGL(k_unpack_records, dim3(grid_for(n, 256)), dim3(256), 0, d->stream, (u64)first, (u64)n, (const Record*)src, d->right, d->left, d->conn, d->cflag);
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}

int dev_reciprocal(Device* d, uint64_t emit_lo, uint64_t emit_hi, uint64_t* n_ov, uint64_t* contained, uint64_t* contained_size, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    const u64 N = d->N;
    HIPCHK(hipEventRecord(d->ev[0], d->stream));
    HIPCHK(hipMemsetAsync(d->d_counters + CTR_RECIP, 0, 9 * sizeof(u64), d->stream));      // (its five words and the probe pass's four)
    // (records by position; the status goes out by position -- statusP, what the emit half and the hit-list kernels read; by id on demand, or here on the A/B route)
    const bool eager = d->opt.get("SAGE2OV_STATUS_EAGER") != nullptr;
    if (eager) hipLaunchKernelGGL(k_recip_cond<true>, dim3(grid_for(N, 256 * COND_PER_THREAD)), dim3(256), 0, d->stream, N, d->right, d->left, d->conn, d->cflag, d->idOf, d->status, d->statusP, d->d_counters + CTR_RECIP);
    else hipLaunchKernelGGL(k_recip_cond<false>, dim3(grid_for(N, 256 * COND_PER_THREAD)), dim3(256), 0, d->stream, N, d->right, d->left, d->conn, d->cflag, d->idOf, d->status, d->statusP, d->d_counters + CTR_RECIP);
    d->statusByIdValid = eager; d->statusGen++; d->unresGen = 0;
    HIPCHK(hipEventRecord(d->ev[4], d->stream));
    if (d->diet && emit_hi > emit_lo) {                                     // the list is sized by a counting pass (capacity 0: nothing is written, the cursor counts)
        hipLaunchKernelGGL(k_recip_emit, dim3(grid_for(emit_hi - emit_lo, 256 * EMIT_PER_THREAD)), dim3(256), 0, d->stream, N, d->readsLoc, d->S, d->uniL, d->right, d->left, d->statusP, d->idOf, (EdgeCand*)nullptr, (u64)0, d->d_counters + CTR_RECIP, (u64)emit_lo, (u64)emit_hi);
        u64 want = 0; { int rc = read_counters(d, CTR_RECIP, 1, &want, err); if (rc) return rc; }
        if (want + 1024 > d->cand_cap || !d->cand) { int rc = cand_resize(d, want + 1024, 0, err); if (rc) return rc; }
        HIPCHK(hipMemsetAsync(d->d_counters + CTR_RECIP, 0, sizeof(u64), d->stream));
    }
    if (emit_hi > emit_lo)
        hipLaunchKernelGGL(k_recip_emit, dim3(grid_for(emit_hi - emit_lo, 256 * EMIT_PER_THREAD)), dim3(256), 0, d->stream, N, d->readsLoc, d->S, d->uniL, d->right, d->left, d->statusP, d->idOf, d->cand, d->cand_cap, d->d_counters + CTR_RECIP, (u64)emit_lo, (u64)emit_hi);
    u64 c[8];
    HIPCHK(hipMemcpyAsync(c, d->d_counters + CTR_RECIP, sizeof c, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipEventRecord(d->ev[1], d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    float ms = 0; hipEventElapsedTime(&ms, d->ev[0], d->ev[1]); d->tm.reciprocal_ms += ms;
    hipEventElapsedTime(&ms, d->ev[0], d->ev[4]); d->tm.recip_cond_ms += ms;
    if (c[0] > d->cand_cap) { err = "edge candidate buffer overflow"; return SAGE2OV_ERR_INTERNAL; }
    d->n_cand = c[0]; *n_ov = c[1]; *contained = c[2]; *contained_size = c[3]; d->nUnres = c[4];
    return 0;
}

int dev_download_initial(Device* d, uint64_t* right, uint64_t* left, uint8_t* status, uint32_t* conn, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    const u64 N = d->N;
    if (right || left || conn) {                                           // the C ABI's arrays are indexed by id and name neighbours by id (economyGraph.h:24-30)
        u64* ri = nullptr; u64* li = nullptr; u32* ci = nullptr;
        struct Free { u64*& a; u64*& b; u32*& c; ~Free() { hipFree(a); hipFree(b); hipFree(c); } } fr{ri, li, ci};
        HIPCHK(hipMalloc(&ri, (N + 1) * sizeof(u64))); HIPCHK(hipMalloc(&li, (N + 1) * sizeof(u64))); HIPCHK(hipMalloc(&ci, (N + 1) * sizeof(u32)));
        hipLaunchKernelGGL(k_records_to_ids, dim3(grid_for(N + 1, 256)), dim3(256), 0, d->stream, (u64)N, d->idOf, d->right, d->left, d->conn, ri, li, ci);
        HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(d->stream));
        if (right) HIPCHK(hipMemcpy(right, ri, (N + 1) * sizeof(u64), hipMemcpyDeviceToHost));
        if (left) HIPCHK(hipMemcpy(left, li, (N + 1) * sizeof(u64), hipMemcpyDeviceToHost));
        if (conn) HIPCHK(hipMemcpy(conn, ci, (N + 1) * sizeof(u32), hipMemcpyDeviceToHost));
    }
    if (status) { int rc = ensure_status_by_id(d, err); if (rc) return rc; HIPCHK(hipStreamSynchronize(d->stream)); HIPCHK(hipMemcpy(status, d->status, N + 1, hipMemcpyDeviceToHost)); }
    return 0;
}
int dev_download_status(Device* d, std::vector<uint8_t>& status, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    status.resize(d->N + 1);
    { int rc = ensure_status_by_id(d, err); if (rc) return rc; } HIPCHK(hipStreamSynchronize(d->stream));
    HIPCHK(hipMemcpy(status.data(), d->status, d->N + 1, hipMemcpyDeviceToHost));
    return 0;
}

// the unresolved reads (status 0), any order, left in WS_IDS: *ids, *n.  k_recip_cond counted them, so the list has its size before it is written and a step
// without any launches nothing; the list is stamped with the statuses it was taken from, and the next caller of the same reciprocal pass gets it as it is.
static int collect_unresolved(Device* d, u32** ids, u64* n, std::string& err) {
    const u64 cnt = d->nUnres;
    WS(buf, u32, WS_IDS, std::max<u64>(cnt, 1));
    *ids = buf; *n = cnt;
    if (d->unresGen == d->statusGen) return 0;
    d->unresGen = 0;
    if (cnt) {
        HIPCHK(hipMemsetAsync(d->d_counters + CTR_LIST, 0, sizeof(u64), d->stream));
        hipLaunchKernelGGL(k_red_unresolved, dim3(grid_for(d->N, 256 * UNRES_PER_THREAD)), dim3(256), 0, d->stream, (u64)d->N, d->statusP, d->idOf, buf, cnt, d->d_counters + CTR_LIST);
        u64 got = 0; { int rc = read_counters(d, CTR_LIST, 1, &got, err); if (rc) return rc; }
        if (got != cnt) { err = "unresolved read count changed"; return SAGE2OV_ERR_INTERNAL; }
    }
    d->unresGen = d->statusGen;
    return 0;
}
int dev_unresolved_ids(Device* d, std::vector<uint32_t>& ids, std::string& err) {      // (the list stays in WS_IDS: dev_unresolved_hits probes it)
    HIPCHK(hipSetDevice(d->ordinal));
    ids.clear();
    u32* buf = nullptr; u64 cnt = 0; { int rc = collect_unresolved(d, &buf, &cnt, err); if (rc) return rc; }
    ids.resize(cnt); if (cnt) { HIPCHK(hipMemcpyAsync(ids.data(), buf, cnt * sizeof(u32), hipMemcpyDeviceToHost, d->stream)); HIPCHK(hipStreamSynchronize(d->stream)); }
    std::sort(ids.begin(), ids.end());
    return 0;
}
int dev_unresolved_hits(Device* d, std::vector<Hit>& hits, uint64_t* n_unresolved, std::string& err, std::vector<uint32_t>* ids_out) {
    HIPCHK(hipSetDevice(d->ordinal));
    HIPCHK(hipEventRecord(d->ev[0], d->stream));
    std::vector<uint32_t> ids; int rc = dev_unresolved_ids(d, ids, err); if (rc) return rc;
    u64 nun = ids.size();
    *n_unresolved = nun; hits.clear(); if (ids_out) *ids_out = ids;
    if (nun == 0) return 0;
    u64 cap = std::max<u64>(1 << 16, nun * 80);
    for (int attempt = 0; attempt < 4; attempt++) {
        WS(dh, Hit, WS_HITS, cap);
        HIPCHK(hipMemsetAsync(d->d_counters + CTR_HIT_CURSOR, 0, sizeof(u64), d->stream));
        ProbeArgs A = base_args(d); A.hits = dh; A.hits_cap = cap;
        { WS(idbuf, u32, WS_IDS, nun); WS(pbuf, u32, WS_SLOW, nun + 1);      // the list dev_unresolved_ids left on the device, as positions: only these reads are probed
          hipLaunchKernelGGL(k_ids_to_pos, dim3(grid_for(nun, 256)), dim3(256), 0, d->stream, idbuf, (u64)nun, d->posOf, pbuf); A.ids = pbuf; A.n_ids = nun; }
        rc = launch_probe<1>(d, A, err); if (rc) return rc;
        u64 nh = 0; rc = read_counters(d, CTR_HIT_CURSOR, 1, &nh, err); if (rc) return rc;
        if (nh <= cap) {
            hits.resize(nh);
            if (nh) HIPCHK(hipMemcpy(hits.data(), dh, nh * sizeof(Hit), hipMemcpyDeviceToHost));
            HIPCHK(hipEventRecord(d->ev[1], d->stream)); HIPCHK(hipStreamSynchronize(d->stream));
            float ms = 0; hipEventElapsedTime(&ms, d->ev[0], d->ev[1]); d->tm.hits_ms += ms;
            return 0;
        }
        cap = nh + 1024;
    }
    err = "hit buffer sizing failed"; return SAGE2OV_ERR_INTERNAL;
}

// The hit-list pass over A's range or id list (A.hits, A.hitcount set; CTR_HIT_CURSOR, CTR_HIT_REAL and CTR_HANDED[0] preset by the caller): the fast kernel's hit-list form, then the exact
// sequential kernel, appending behind, for the reads it handed over into A.slow -- or for all of A when the layout has no such form.  c[0..2] = those three
// after the fast kernel (its cursor in the hit buffer, its count of real hits, the reads it handed over; the caller's preset when there was no fast kernel),
// *used = the cursor at the end.  A cursor beyond A.hits_cap: the sequential kernel does not run, *used = c[0].
static int hit_list_pass(Device* d, ProbeArgs& A, unsigned blocks, u64 c[3], u64* used, std::string& err) {
    if (launch_form(d, Form::Hits, A, blocks)) {
        HIPCHK(hipGetLastError());
        { int rc = read_counters(d, CTR_HIT_CURSOR, 3, c, err); if (rc) return rc; }
        if (c[0] > A.hits_cap) { *used = c[0]; return 0; }                        // some chunk did not fit
        if (c[2]) {
            ProbeArgs B = base_args(d); B.hits = A.hits; B.hits_cap = A.hits_cap; B.hitcount = A.hitcount; B.ids = A.slow; B.n_ids = c[2];
            int rc = launch_probe<1>(d, B, err); if (rc) return rc;
        }
    } else {
        A.slow = nullptr;
        int rc = launch_probe<1>(d, A, err); if (rc) return rc;
    }
    return read_counters(d, CTR_HIT_CURSOR, 1, used, err);
}
// Reduce phase on the device (see k_ra_mark): dev_reduce_device is the sequence of the stages below.  *done = 0 when the preconditions do not hold (too few
// unresolved reads to be worth it, more than 2^16 lists longer than RA_CAP, 32-bit offsets exhausted; a list longer than RA_CAP alone goes to k_ra_mark_big): the caller then runs the serial replay on the host; nothing but the
// idempotent 0x80 flags has been changed in that case.  A stage says so by returning REDUCE_REPLAY.
// When some bucket is long (ranked: one-sided discovery, economyGraph.cpp:513-564) the order in which the unresolved reads are explored decides which edges
// exist: the potential lists are built here, the order is found by the host's walk (explore_order, sage2ov_walk.cpp) and comes back as ranks.
// Multi-rank contexts (shareRank / shareWorld): hit lists, adjacency and -- with long buckets -- the exploration order are computed for ALL unresolved
// reads on every rank (they are read by everybody's marks), but the marks (:643-707), the removals and the re-emission of the surviving edges run for this
// rank's share of the unresolved reads only (a contiguous part of the list): d->n_cand grows by this rank's survivors, *removed counts this rank's
// removals; the caller all-gathers the survivor buckets (dev_export_survivors / dev_set_survivors) and sums the counters.
constexpr int REDUCE_REPLAY = 1;
struct ReduceRun {                                                                   // one call: the unresolved reads, their hit lists, the final lists -- what one stage leaves for the next
    u32* ids = nullptr; u64 nun = 0;                                                 // the unresolved reads (WS_IDS), all ranks' shares
    u64 wlo = 0, whi = 0; u32 shareWorld = 1;                                        // this rank's share: entries [wlo, whi) of ids (any contiguous cut is exact: a read's marks depend on the lists only)
    bool ranked = false;                                                             // some bucket is long: the exploration order decides which edges exist
    Hit* dh = nullptr; u64 nh = 0, nslots = 0; u32* hitcount = nullptr;              // hit lists: nh real hits in slots [0, nslots) of dh; hits per read position
    u32 *deg = nullptr, *offs = nullptr, *cur = nullptr, *rankDev = nullptr; u64* ent = nullptr; u32* ent32 = nullptr; uint8_t* rm = nullptr; u64 present = 0;      // final lists
    u32 *svn = nullptr, *svoff = nullptr; u64 removed = 0;                           // marks: survivors per read of the share, this rank's removals
    u64 nMid = 0, nHeavy = 0, scLists = 0, scReads = 0, potBeyond = 0, slices = 0;   // which way it went (Device::reduceStats): CTR_MARKS [4] [0] [2] [3], CTR_RANKED[3], slices of potential lists
    u64 gridCap = 256ull * 256;                                                      // SAGE2OV_TEST_MARK_BLOCKS=<b>: at most b blocks for marks and emission (tests: a wave walks many reads of a small input)
    bool timing = false; std::chrono::steady_clock::time_point tp;
    void lap(Device* d, const char* what) { if (!timing) return; hipStreamSynchronize(d->stream); auto t = std::chrono::steady_clock::now(); fprintf(stderr, "[reduce/device] %-30s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(t - tp).count()); tp = t; }
    // (the grid of marks and emission: a wave per read, blocks walk the list round-robin; blocks per CU -> reduce phase at configs[1] + 0.1 % errors: 16 -> 69.5 ms, 64 -> 66.0, 256 -> 65.2, 1024 -> 65.2: the tail again)
    unsigned share_grid() const { return (unsigned)std::max<u64>(1, std::min<u64>((whi - wlo + 3) / 4, gridCap)); }
};
// Hit lists: directional hits of the unresolved reads, device resident: the fast kernel in its hit-list form (locality order, minimiser
// groups), the sequential kernel for the few reads it hands over (> 128 candidates, ambiguous tags) and for the 16-word layout
static int reduce_hit_lists(Device* d, ReduceRun& R, std::string& err) {
    const u64 N = d->N, nun = R.nun;
    WS(hitcount, u32, WS_RA_CUR, N + 2); R.hitcount = hitcount;                    // (what the probe pass counted when it wrote the hits out; else zeroed below)
    const u32* order = d->idOf + 1;                                                // ids in locality order (positions 1..N)
    if (R.ranked || R.shareWorld > 1) {                                            // (several ranks cut the SAME list into shares: it must not depend on the order of atomics)
        // the unresolved reads listed in LOCALITY order (a stable compaction of `order`): their potential lists are then laid out in that
        // order too, so the lists the host's walk visits one after the other sit next to each other in memory (cache lines, TLB)
        WS(flg, u32, WS_RR_IN, N + 2); WS(fpos, u32, WS_RR_WIDX, N + 2);
        { int rc = ensure_status_by_id(d, err); if (rc) return rc; }
        hipLaunchKernelGGL(k_rr_unres_flag, dim3(grid_for(N, 256)), dim3(256), 0, d->stream, order, (u64)N, d->status, flg);
        u64 cnt2 = 0; { int rc = scan_u32(d, flg, N, fpos, &cnt2, err); if (rc) return rc; }
        if (cnt2 != nun) { err = "unresolved read count changed"; return SAGE2OV_ERR_INTERNAL; }
        hipLaunchKernelGGL(k_rr_unres_pick, dim3(grid_for(N, 256)), dim3(256), 0, d->stream, order, (u64)N, flg, fpos, R.ids);
    }
    WS(slow, u32, WS_SLOW, N + 1);
    const unsigned blocks = (unsigned)std::min<u64>((N + FAST_CHUNK - 1) / FAST_CHUNK, 256ull * 16);
    u64 cap = std::max<u64>(1 << 16, nun * 80) + (u64)blocks * FAST_WPB * HITS_CHUNK; bool ok = false;
    if (d->opt.get("SAGE2OV_TEST_SMALL_BUFFERS")) cap = 8192;                      // tests: start far too small, the sizing loop must recover
    // The initial pass may have written every read's hits out already (dev_probe, noisy data): drop the ones with a resolved end, in place, and
    // run the hit-list kernel only for the unresolved reads that pass did not cover (its sample, hand-overs).  Any shortage of room: the
    // ordinary way below, from scratch.
    if (d->pre.valid && !d->opt.get("SAGE2OV_TEST_SMALL_BUFFERS")) {
        d->pre.valid = false;                                                     // (consumed: the filter works in place)
        R.dh = d->pre.hits; const u64 pcap = d->pre.cap; u64 used = d->pre.used;
        WS(noneList, u32, WS_PRE_NONE, N + 2);
        HIPCHK(hipMemsetAsync(d->d_counters + CTR_FILTER, 0, 2 * sizeof(u64), d->stream));
        { int rc = ensure_status_by_id(d, err); if (rc) return rc; }
        hipLaunchKernelGGL(k_hits_filter, dim3((unsigned)std::min<u64>((N + 3) / 4, 256ull * 64)), dim3(256), 0, d->stream, R.dh, d->pre.base, d->status, d->statusP, d->idOf, d->posOf, (u64)N, hitcount, noneList, d->d_counters + CTR_FILTER);
        u64 fc[2] = {0, 0}; { int rc = read_counters(d, CTR_FILTER, 2, fc, err); if (rc) return rc; }
        HIPCHK(hipGetLastError());
        R.nh = fc[0]; ok = true;
        if (fc[1]) {                                                              // unresolved reads without written hits: the hit-list pass over their positions, appending
            u64 c3[3] = {used, 0, 0}; HIPCHK(hipMemcpyAsync(d->d_counters + CTR_HIT_CURSOR, c3, sizeof c3, hipMemcpyHostToDevice, d->stream));      // (cursor, CTR_HIT_REAL, CTR_HANDED[0])
            ProbeArgs A = base_args(d); A.ids = noneList; A.n_ids = fc[1]; A.hits = R.dh; A.hits_cap = pcap; A.hitcount = hitcount; A.slow = slow; A.slow_cap = N + 1;
            const unsigned nb = plan_fast_grid(d->opt, A, fc[1], true);
            u64 used2 = 0; { int rc = hit_list_pass(d, A, nb, c3, &used2, err); if (rc) return rc; }
            if (used2 > pcap) ok = false; else { R.nh += c3[1] + (used2 - std::max(c3[0], used)); used = used2; }
        }
        if (ok) R.nslots = used;
    }
    for (int attempt = 0; attempt < 4 && !ok; attempt++) {
        WS(hb, Hit, WS_HITS, cap); R.dh = hb;
        HIPCHK(hipMemsetAsync(d->d_counters + CTR_HIT_CURSOR, 0, 3 * sizeof(u64), d->stream));      // (cursor, CTR_HIT_REAL, CTR_HANDED[0])
        HIPCHK(hipMemsetAsync(hitcount, 0, (N + 2) * sizeof(u32), d->stream));
        ProbeArgs A = base_args(d); A.lo = 1; A.hi = N + 1; A.hits = R.dh; A.hits_cap = cap; A.hitcount = hitcount;
        A.slow = slow; A.slow_cap = N + 1;                                       // (all positions; the kernel skips what is not status 0)
        u64 c3[3] = {0, 0, 0}, used = 0;
        { int rc = hit_list_pass(d, A, blocks, c3, &used, err); if (rc) return rc; }
        if (used > cap) { cap = used + used / 8 + 1024; continue; }                  // some chunk or the appended hits did not fit: everything again
        R.nslots = used; R.nh = c3[1] + (used - c3[0]); ok = true;                       // real hits: fast kernel's count + what the sequential kernel appended
    }
    if (!ok) { err = "hit buffer sizing failed"; return SAGE2OV_ERR_INTERNAL; }
    return 0;
}
// Final lists, first half: their buffers, and the degrees that the candidates of the reciprocal pass contribute (the ranked order needs these alone)
static int reduce_cand_degrees(Device* d, ReduceRun& R, std::string& err) {
    const u64 N = d->N, nc = d->n_cand;
    WS(deg, u32, WS_RA_DEG, N + 2); WS(offs, u32, WS_RA_OFF, N + 2); WS(cur, u32, WS_CURSOR, N + 2); R.deg = deg; R.offs = offs; R.cur = cur;
    HIPCHK(hipMemsetAsync(deg, 0, (N + 2) * sizeof(u32), d->stream)); HIPCHK(hipMemsetAsync(cur, 0, (N + 2) * sizeof(u32), d->stream));
    { int rc = ensure_status_by_id(d, err); if (rc) return rc; }
    if (nc) hipLaunchKernelGGL(k_ra_degree_c, dim3(grid_for(nc, 256)), dim3(256), 0, d->stream, d->cand, (u64)nc, d->status, deg);
    HIPCHK(hipMemsetAsync(d->d_counters + CTR_RANKED, 0, 4 * sizeof(u64), d->stream));
    return 0;
}
// Ranked order.  plist[offp[w] .. offp[w+1]) = potential list of the w-th unresolved read (own hits + twins of incoming hits), sorted like the reference sorts
// a list when the read is explored (:853-871).  An own hit is in the read's list iff the target was still unexplored when the read was explored, a twin iff
// its source had been explored before; candidates of the reciprocal pass (hasCand) are always there but their far ends are never explorable.
struct RankLists {                                                                   // the potential lists as the host's walk reads them, and the device arrays the slices share
    std::vector<u32> hLen, hDegp, hLoc; std::vector<uint8_t> hasCand; std::vector<const u32*> listPtr;
    std::vector<std::vector<u32>> heavyLists;                                        // lists beyond the device sort (reads that thousands of others see): sorted and merged on the host
    u32 *degp = nullptr, *lenp = nullptr, *widx = nullptr, *pcur = nullptr;
};
// degrees of the potential lists, on the device and on the host, with the tables the walk and the host merge need (position of an id, reads with candidates)
static int rank_degrees(Device* d, ReduceRun& R, RankLists& L, std::string& err) {
    const u64 N = d->N, nun = R.nun;
    // (WS_RR_IN, WS_RR_WIDX: instead of the flags and positions of reduce_hit_lists' compaction, which are used up)
    WS(incount, u32, WS_RR_IN, N + 2); WS(widx, u32, WS_RR_WIDX, N + 2); WS(degp, u32, WS_RR_DEGP, nun + 2); WS(pcur, u32, WS_RR_CUR, N + 2);
    L.degp = degp; L.widx = widx; L.pcur = pcur;
    HIPCHK(hipMemsetAsync(incount, 0, (N + 2) * sizeof(u32), d->stream)); HIPCHK(hipMemsetAsync(pcur, 0, (N + 2) * sizeof(u32), d->stream)); HIPCHK(hipMemsetAsync(widx, 0, (N + 2) * sizeof(u32), d->stream));
    hipLaunchKernelGGL(k_rr_widx, dim3(grid_for(nun, 256)), dim3(256), 0, d->stream, R.ids, (u64)nun, widx);
    if (R.nslots) hipLaunchKernelGGL(k_rr_incount, dim3(grid_for(R.nslots, 256)), dim3(256), 0, d->stream, R.dh, (u64)R.nslots, incount);
    hipLaunchKernelGGL(k_rr_degp, dim3(grid_for(nun, 256)), dim3(256), 0, d->stream, R.ids, (u64)nun, R.hitcount, incount, degp);
    std::vector<u32> hIds(nun), hDeg(N + 2);
    L.hLen.assign(nun, 0); L.hDegp.resize(nun); L.hLoc.resize(N + 2); L.hasCand.assign(nun, 0); L.listPtr.assign(nun, nullptr);
    HIPCHK(hipMemcpyAsync(L.hLoc.data(), d->posOf, (N + 2) * sizeof(u32), hipMemcpyDeviceToHost, d->stream));      // read id -> 1-based position in the locality order
    HIPCHK(hipMemcpyAsync(L.hDegp.data(), degp, nun * sizeof(u32), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipMemcpyAsync(hIds.data(), R.ids, nun * sizeof(u32), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipMemcpyAsync(hDeg.data(), R.deg, (N + 2) * sizeof(u32), hipMemcpyDeviceToHost, d->stream)); HIPCHK(hipStreamSynchronize(d->stream));   // (deg so far: candidate entries only)
    for (u64 w = 0; w < nun; w++) L.hasCand[w] = hDeg[hIds[w]] != 0;
    if (R.timing) { u64 c512 = 0, c1k = 0, c4k = 0; u32 mx = 0; for (u32 v : L.hDegp) { c512 += v > 512; c1k += v > 1024; c4k += v > 4096; mx = std::max(mx, v); }
        fprintf(stderr, "[reduce/device] potential lists: %llu reads, > 512: %llu, > 1024: %llu, > 4096: %llu, longest %u\n", (unsigned long long)nun, (unsigned long long)c512, (unsigned long long)c1k, (unsigned long long)c4k, mx); }
    return 0;
}
// one slice of potential lists, those of the unresolved reads [w0, w1): scan, fill, sort and compact on the device, download into a staging buffer; the lists
// over RR_CAP (their device length is 0) are fetched unsorted and sorted and merged here
static int rank_slice(Device* d, ReduceRun& R, RankLists& L, RrStaging& staging, u64 w0, u64 w1, std::string& err) {
    const u64 nw = w1 - w0, nslots = R.nslots; u32* const degp = L.degp; u32* const lenp = L.lenp;
    WS(offp, u32, WS_RR_OFFP, nw + 2); WS(coff, u32, WS_RR_COFF, nw + 2);
    u64 totp = 0; { int rc = scan_u32(d, degp + w0, nw, offp, &totp, err); if (rc) return rc; }
    WS(entp, u64, WS_RR_ENTP, totp + 64); WS(outp, u32, WS_RR_OUTP, totp + 64);
    HIPCHK(hipMemsetAsync(entp, 0, (totp + 64) * sizeof(u64), d->stream));
    if (nslots) hipLaunchKernelGGL(k_rr_fillp, dim3(grid_for(nslots, 256)), dim3(256), 0, d->stream, R.dh, (u64)nslots, d->reads, d->S, d->uniL, L.widx, (u32)w0, (u32)w1, offp, R.hitcount, L.pcur, entp);
    hipLaunchKernelGGL(k_rr_sortp, dim3((unsigned)std::min<u64>((nw + 3) / 4, 256ull * 16)), dim3(256), 0, d->stream, (u64)nw, offp, degp + w0, entp, outp, lenp + w0, d->d_counters + CTR_RANKED + 3);
    u64 totc = 0; { int rc = scan_u32(d, lenp + w0, nw, coff, &totc, err); if (rc) return rc; }
    WS(outc, u32, WS_RR_OUTC, totc + 64);
    hipLaunchKernelGGL(k_rr_compact, dim3((unsigned)std::min<u64>((nw + 3) / 4, 256ull * 16)), dim3(256), 0, d->stream, (u64)nw, offp, lenp + w0, coff, outp, d->posOf, outc);
    R.lap(d, "  potential lists: kernels");
    u32* hbuf = staging.get(totc); if (!hbuf) { err = "host staging buffer allocation failed"; return SAGE2OV_ERR_NOMEM; }
    R.lap(d, "  potential lists: staging buffer (2 MB pages, touched, registered)");
    HIPCHK(hipMemcpyAsync(L.hLen.data() + w0, lenp + w0, nw * sizeof(u32), hipMemcpyDeviceToHost, d->stream));
    if (totc) HIPCHK(hipMemcpyAsync(hbuf, outc, totc * sizeof(u32), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    u64 at = 0, rel = 0; std::vector<u64> seg;
    for (u64 w = w0; w < w1; w++) {
        const u32 n = L.hDegp[w];
        if (n <= (u32)RR_CAP) { L.listPtr[w] = hbuf + at; at += L.hLen[w]; }
        else {
            seg.resize(n); HIPCHK(hipMemcpy(seg.data(), entp + rel, (size_t)n * sizeof(u64), hipMemcpyDeviceToHost));
            std::sort(seg.begin(), seg.end(), std::greater<u64>());
            L.heavyLists.emplace_back(); std::vector<u32>& hl = L.heavyLists.back(); hl.reserve(n);
            for (u32 x = 0; x < n; x++) {
                const u64 kx = seg[x]; if (kx == 0) break;
                const bool twin = kx & 1ull;
                if (!twin && x > 0 && (seg[x - 1] & 1ull) && (seg[x - 1] >> 1) == (kx >> 1)) continue;      // the own hit behind its twin: merged
                const bool sym = twin && x + 1 < n && seg[x + 1] != 0 && !(seg[x + 1] & 1ull) && (seg[x + 1] >> 1) == (kx >> 1);
                hl.push_back(L.hLoc[(u32)(kx >> 11) & 0x3FFFFFFFu] | ((sym ? 0u : (twin ? 2u : 1u)) << 30));
            }
            L.hLen[w] = (u32)hl.size();
        }
        rel += n;
    }
    return 0;
}
// the walk's set-up: positions of the unresolved reads in list order (posOf) and in ascending id order (startOrder, the walk's starts): two gathers and a
// compaction, on the device
static int rank_walk_setup(Device* d, ReduceRun& R, std::vector<u32>& posOf, std::vector<u32>& startOrder, std::string& err) {
    const u64 N = d->N, nun = R.nun;
    // (all four instead of what the slices used, which the host has by now: WS_RR_IN incount, WS_RR_WIDX widx, WS_RR_CUR the fill cursors, WS_RR_DEGP degp)
    WS(sflg, u32, WS_RR_IN, N + 2); WS(sfpos, u32, WS_RR_WIDX, N + 2); WS(sout, u32, WS_RR_CUR, N + 2); WS(pout, u32, WS_RR_DEGP, nun + 2);
    hipLaunchKernelGGL(k_ids_to_pos, dim3(grid_for(nun, 256)), dim3(256), 0, d->stream, R.ids, (u64)nun, d->posOf, pout);
    { int rc = ensure_status_by_id(d, err); if (rc) return rc; }
    hipLaunchKernelGGL(k_rr_start_flag, dim3(grid_for(N, 256)), dim3(256), 0, d->stream, (u64)N, d->status, sflg);
    u64 cnt3 = 0; { int rc = scan_u32(d, sflg, N, sfpos, &cnt3, err); if (rc) return rc; }
    if (cnt3 != nun) { err = "unresolved read count changed"; return SAGE2OV_ERR_INTERNAL; }
    hipLaunchKernelGGL(k_rr_start_pick, dim3(grid_for(N, 256)), dim3(256), 0, d->stream, (u64)N, sflg, sfpos, d->posOf, sout);
    posOf.resize(nun); startOrder.resize(nun);
    HIPCHK(hipMemcpyAsync(posOf.data(), pout, nun * sizeof(u32), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipMemcpyAsync(startOrder.data(), sout, nun * sizeof(u32), hipMemcpyDeviceToHost, d->stream)); HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}
// the ranks back on the device, by read id (R.rankDev): 1-based exploration order, 0: not an unresolved read
static int rank_upload(Device* d, ReduceRun& R, const std::vector<u32>& rankByPos, std::string& err) {
    const u64 N = d->N;
    { WS(rk, u32, WS_RR_RANK, N + 2); R.rankDev = rk; }
    WS(rl, u32, WS_RR_RANKL, N + 2);
    HIPCHK(hipMemcpyAsync(rl, rankByPos.data(), (N + 2) * sizeof(u32), hipMemcpyHostToDevice, d->stream));
    hipLaunchKernelGGL(k_rr_rank_by_id, dim3(grid_for(N + 2, 256)), dim3(256), 0, d->stream, rl, d->posOf, (u64)(N + 2), R.rankDev);
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}
// potential lists sorted and merged on the device, slice by slice (a slice stays below 2^30 entries); exploration order on the host; ranks back
static int reduce_ranked_order(Device* d, ReduceRun& R, std::string& err) {
    const u64 N = d->N, nun = R.nun; RankLists L;
    { int rc = rank_degrees(d, R, L, err); if (rc) return rc; }
    // gigabytes at 10 M reads: 2 MB pages for the host's walk, registered so that the download is a DMA; kept in the context from step to step (allocating, touching
    // and registering 1.7 GB took 100 ms of every call)
    if (!d->rrStaging) d->rrStaging = new RrStaging();
    RrStaging& staging = *(RrStaging*)d->rrStaging; staging.next = 0;
    u64 sliceEntries = 1ull << 30; if (const char* ev = d->opt.get("SAGE2OV_TEST_RANK_SLICE")) sliceEntries = std::max<u64>(1024, strtoull(ev, nullptr, 10));
    { WS(lenp, u32, WS_RR_LEN, nun + 2); L.lenp = lenp; }
    for (u64 w0 = 0; w0 < nun;) {
        u64 w1 = w0, tot0 = 0; while (w1 < nun && (w1 == w0 || tot0 + L.hDegp[w1] <= sliceEntries)) tot0 += L.hDegp[w1++];
        if (tot0 >= (1ull << 32) - 64) return REDUCE_REPLAY;                      // one read with 2^32 potential neighbours: not this path
        { int rc = rank_slice(d, R, L, staging, w0, w1, err); if (rc) return rc; }
        w0 = w1; R.slices++;
    }
    { size_t hx = 0; for (u64 w = 0; w < nun; w++) if (L.hDegp[w] > (u32)RR_CAP) L.listPtr[w] = L.heavyLists[hx++].data(); }      // (after the last push_back: the vectors no longer move)
    R.lap(d, "potential lists (build + sort + download)");
    std::vector<u32> rankByPos, posOf, startOrder;
    { int rc = rank_walk_setup(d, R, posOf, startOrder, err); if (rc) return rc; }
    R.lap(d, "walk set-up (device + download)");
    explore_order(d->opt, posOf, L.listPtr, L.hLen, L.hasCand, N, startOrder, rankByPos);
    if (rankByPos.size() != N + 2) { err = "exploration walk: table allocation failed"; return SAGE2OV_ERR_NOMEM; }
    R.lap(d, "exploration order (host)");
    return rank_upload(d, R, rankByPos, err);
}
// Final lists, second half: the degrees the hits contribute (ranked: those the exploration order keeps), offsets, and the entries of candidates and hits
static int reduce_final_lists(Device* d, ReduceRun& R, std::string& err) {
    const u64 N = d->N, nc = d->n_cand, nslots = R.nslots; u32* const deg = R.deg; u32* const offs = R.offs;
    if (R.ranked) { if (nslots) hipLaunchKernelGGL(k_rr_degree_h, dim3(grid_for(nslots, 256)), dim3(256), 0, d->stream, R.dh, (u64)nslots, R.rankDev, deg, d->d_counters + CTR_RANKED); }
    else hipLaunchKernelGGL(k_ra_degree_h, dim3(grid_for(N + 1, 256)), dim3(256), 0, d->stream, R.hitcount, (u64)N, deg);
    R.lap(d, "  ranks to the device, degrees of the final lists");
    u64 tot = 0; { int rc = scan_u32(d, deg, N + 2, offs, &tot, err); if (rc) return rc; }
    if (tot >= (1ull << 32) - 64) return REDUCE_REPLAY;
    WS(ent, u64, WS_RA_ENT, tot + 64); WS(rm, uint8_t, WS_RA_RM, tot + 64); WS(ent32, u32, WS_RA_ENT32, tot + 64); R.ent = ent; R.rm = rm; R.ent32 = ent32;
    if (nc) hipLaunchKernelGGL(k_ra_fill_c, dim3(grid_for(nc, 256)), dim3(256), 0, d->stream, d->cand, (u64)nc, d->reads, d->S, d->uniL, offs, R.cur, ent, ent32);
    if (R.ranked) { if (nslots) hipLaunchKernelGGL(k_rr_fill_h, dim3(grid_for(nslots, 256)), dim3(256), 0, d->stream, R.dh, (u64)nslots, R.rankDev, d->reads, d->S, d->uniL, offs, R.cur, ent, ent32); }
    else if (nslots) hipLaunchKernelGGL(k_ra_fill_h, dim3(grid_for(nslots, 256)), dim3(256), 0, d->stream, R.dh, (u64)nslots, offs, deg, R.hitcount, ent, ent32);
    if (R.ranked) { u64 c4[4]; int rc = read_counters(d, CTR_RANKED, 4, c4, err); if (rc) return rc; R.present = c4[2]; R.potBeyond = c4[3]; }
    return 0;
}
// the marks of lists beyond the LDS kernel (heavy[0, nhv), listed by k_ra_mark): same marking out of global scratch, one wavefront each; c = CTR_MARKS afterwards
static int reduce_marks_heavy(Device* d, ReduceRun& R, const u32* ids, u32* heavy, u32 nhv, u64 c[4], std::string& err) {
    WS(hsize, u32, WS_RA_HSIZE, nhv); WS(hscr, u64, WS_RA_HSCR, nhv);
    hipLaunchKernelGGL(k_ra_heavy_sizes, dim3(grid_for(nhv, 256)), dim3(256), 0, d->stream, heavy, nhv, ids, R.deg, hsize);
    std::vector<u32> hs(nhv); HIPCHK(hipMemcpyAsync(hs.data(), hsize, nhv * sizeof(u32), hipMemcpyDeviceToHost, d->stream)); HIPCHK(hipStreamSynchronize(d->stream));   // (the stream is non-blocking: the null stream does not wait for it)
    std::vector<u64> so(nhv); u64 words = 0;
    for (u32 b = 0; b < nhv; b++) { u64 P = 64; while (P < hs[b]) P <<= 1; so[b] = words; words += P + 2 * P + 2 * P; }      // key[P] u64 + ht[4P] u32 + mk[4P] u32
    HIPCHK(hipMemcpyAsync(hscr, so.data(), nhv * sizeof(u64), hipMemcpyHostToDevice, d->stream)); HIPCHK(hipStreamSynchronize(d->stream));
    DevTmp tmp; u64* scratch = tmp.get<u64>(words); if (!scratch) { err = "k_ra_mark_big: out of device memory"; return SAGE2OV_ERR_NOMEM; }
    hipLaunchKernelGGL(k_ra_mark_big, dim3(nhv), dim3(64), 0, d->stream, ids, heavy, hscr, scratch, R.offs, R.deg, R.ent, R.rm, R.svn, d->d_counters + CTR_MARKS);
    hipError_t e2 = hipStreamSynchronize(d->stream); tmp.release(scratch);
    if (e2 != hipSuccess) { err = std::string("k_ra_mark_big: ") + hipGetErrorString(e2); return SAGE2OV_ERR_DEVICE; }
    HIPCHK(hipMemcpy(c, d->d_counters + CTR_MARKS, 4 * sizeof(u64), hipMemcpyDeviceToHost));
    return 0;
}
// Marks (:643-707) of this rank's share: the transitive entries of every list, survivors counted per read (R.svn); d->ev[5] opens marks_ms
static int reduce_marks(Device* d, ReduceRun& R, std::string& err) {
    HIPCHK(hipMemsetAsync(d->d_counters + CTR_MARKS, 0, 5 * sizeof(u64), d->stream));      // (the words of CTR_RANKED, read by now)
    const u32* const ids = R.ids + R.wlo; const u64 nun = R.whi - R.wlo;
    WS(svn, u32, WS_NEED, nun + 2); WS(svoff, u32, WS_OWNER, nun + 2); R.svn = svn; R.svoff = svoff;
    const unsigned gb = R.share_grid();
    const u64 heavyCap = 1 << 16; WS(heavy, u32, WS_RA_HEAVY, heavyCap);
    R.lap(d, "  final lists filled");                                       // (closes reduce_final_lists: it stands behind the marks' buffers, in front of the event that opens marks_ms)
    HIPCHK(hipEventRecord(d->ev[5], d->stream));                          // (marks_ms: the sharded part of the phase -- marks, removals, re-emission)
    const u32 noShortcut = d->opt.get("SAGE2OV_RA_NO_SHORTCUT") ? 1u : 0u;      // (tests: the walk of every list, as until round 4)
    WS(mid, u32, WS_RA_SPLIT, nun + 2);                                          // the reads with more than 128 entries, listed by the first launch for the second
    if (nun) {
    hipLaunchKernelGGL((k_ra_mark<128, 8, 0, false>), dim3(gb), dim3(256), 0, d->stream, ids, (u64)nun, R.offs, R.deg, R.ent, R.ent32, R.rm, svn, d->d_counters + CTR_MARKS, heavy, heavyCap, noShortcut, mid);     // lists of <= 128 entries
    hipLaunchKernelGGL((k_ra_mark<RA_CAP, 10, 128, true>), dim3(gb), dim3(256), 0, d->stream, ids, (u64)nun, R.offs, R.deg, R.ent, R.ent32, R.rm, svn, d->d_counters + CTR_MARKS, heavy, heavyCap, noShortcut, mid);   // 129 .. RA_CAP (the reads the first launch listed); longer: k_ra_mark_big
    }
    u64 c[5];
    { int rc = read_counters(d, CTR_MARKS, 5, c, err); if (rc) return rc; }
    HIPCHK(hipGetLastError());
    R.nHeavy = c[0]; R.scLists = c[2]; R.scReads = c[3]; R.nMid = c[4];      // (before reduce_marks_heavy reads c again)
    if (R.timing) fprintf(stderr, "[reduce/device] marks of %llu of %llu reads by the short cut (k_ra_mark: ra_shortcut), %.2f lists read per read\n", (unsigned long long)c[3], (unsigned long long)nun, nun ? (double)c[2] / (double)nun : 0.0);
    if (c[0] > heavyCap) { if (R.shareWorld > 1) { err = "reduce: too many oversized lists in this rank's share"; return SAGE2OV_ERR_LIMIT; } return REDUCE_REPLAY; }   // (never seen) that many oversized lists: serial replay (a rank of many cannot decide that alone)
    if (c[0]) { int rc = reduce_marks_heavy(d, R, ids, heavy, (u32)c[0], c, err); if (rc) return rc; }
    R.removed = c[1];
    return 0;
}
// Emit: the survivors of this rank's share behind the candidates of the reciprocal pass (d->n_cand grows by them)
static int reduce_emit(Device* d, ReduceRun& R, std::string& err) {
    const u32* const ids = R.ids + R.wlo; const u64 nun = R.whi - R.wlo;
    u64 nsv = 0; if (nun) { int rc = scan_u32(d, R.svn, nun, R.svoff, &nsv, err); if (rc) return rc; }
    if (d->n_cand + nsv > d->cand_cap || d->opt.get("SAGE2OV_TEST_SMALL_BUFFERS")) {
        { int rc = cand_resize(d, d->n_cand + nsv + 1024, d->n_cand, err); if (rc) return rc; }
    }
    R.lap(d, "final lists + marks");                                           // (closes reduce_marks: printed here, once the candidate list has room)
    if (nun) hipLaunchKernelGGL(k_ra_emit, dim3(R.share_grid()), dim3(256), 0, d->stream, ids, (u64)nun, R.offs, R.deg, R.ent, R.rm, R.svoff, d->cand, (u64)d->n_cand, (u64)d->cand_cap);
    HIPCHK(hipGetLastError());
    d->n_cand += nsv;
    return 0;
}
int dev_reduce_device(Device* d, uint64_t min_unresolved, uint64_t* n_unresolved, uint64_t* n_hits, uint64_t* inserted, uint64_t* removed, int* done, std::string& err,
                      uint32_t shareRank, uint32_t shareWorld) {
    HIPCHK(hipSetDevice(d->ordinal));
    *done = 0; *inserted = 0; *removed = 0; *n_hits = 0;
    for (u64& v : d->reduceStats) v = 0;
    HIPCHK(hipEventRecord(d->ev[0], d->stream));
    ReduceRun R;
    if (const char* eb = d->opt.get("SAGE2OV_TEST_MARK_BLOCKS")) R.gridCap = (u64)std::max(1, atoi(eb));
    { int rc = collect_unresolved(d, &R.ids, &R.nun, err); if (rc) return rc; }
    const u64 nun = R.nun; *n_unresolved = nun;
    d->reduceStats[1] = nun;
    if (nun == 0) { *done = 1; return 0; }
    if (nun < min_unresolved) return 0;
    R.ranked = d->n_long != 0; R.shareWorld = shareWorld;
    R.wlo = shareWorld > 1 ? nun * shareRank / shareWorld : 0; R.whi = shareWorld > 1 ? nun * (shareRank + 1) / shareWorld : nun;
    R.timing = d->opt.get("SAGE2OV_TIMING") != nullptr; R.tp = std::chrono::steady_clock::now();
    int rc = reduce_hit_lists(d, R, err); if (rc) return rc;
    *n_hits = R.nh;
    R.lap(d, "hit lists");
    rc = reduce_cand_degrees(d, R, err);
    if (!rc && R.ranked) rc = reduce_ranked_order(d, R, err);
    if (!rc) rc = reduce_final_lists(d, R, err);
    if (!rc) rc = reduce_marks(d, R, err);
    if (!rc) rc = reduce_emit(d, R, err);
    if (rc) return rc == REDUCE_REPLAY ? 0 : rc;                          // (replay: *done stays 0)
    *inserted = R.ranked ? 2 * R.present : R.nh; *removed = R.removed; *done = 1;
    { const u64 st[SAGE2OV_REDUCE_STATS] = {R.ranked ? 2ull : 1ull, nun, R.nMid, R.nHeavy, R.scLists, R.scReads, R.removed, R.potBeyond, R.slices}; for (int x = 0; x < SAGE2OV_REDUCE_STATS; x++) d->reduceStats[x] = st[x]; }
    HIPCHK(hipEventRecord(d->ev[1], d->stream)); HIPCHK(hipStreamSynchronize(d->stream));
    float ms = 0; hipEventElapsedTime(&ms, d->ev[0], d->ev[1]); d->tm.hits_ms += ms;
    hipEventElapsedTime(&ms, d->ev[5], d->ev[1]); d->tm.marks_ms += ms;
    mem_sample(d);
    return 0;
}

// candidates that touch an unresolved read or one of its neighbours (their adjacency lists are what
// markTransitiveEdge reads, economyGraph.cpp:643-679); candidates owned by unresolved reads are flagged
// as dropped on the device: the replay re-emits the survivors.
int dev_collect_reduce_edges(Device* d, const std::vector<uint32_t>& unresolved, std::vector<EdgeCand>& out, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    out.clear(); const u64 n = d->n_cand; if (n == 0) return 0;
    EdgeCand* buf = nullptr; u64 cap = 1 << 16;
    const u32 nUn = (u32)std::min<size_t>(unresolved.size(), 1u << 30);
    if (nUn && nUn <= FEW_MAX / 3 && !d->opt.get("SAGE2OV_TEST_GENERAL_COLLECT")) {
        // a handful of unresolved reads (see k_red_collect_few): the short list = these reads + their two extension partners, found from their records
        d->unresGen = 0;                                                   // (WS_IDS is taken: it lists the short list from here on)
        WS(dIds, u32, WS_IDS, 4 * (u64)FEW_MAX); WS(dRec, u64, WS_NEED, 2 * (u64)nUn + 2);
        u32* dNeed = dIds + FEW_MAX;
        HIPCHK(hipMemcpyAsync(dIds, unresolved.data(), nUn * sizeof(u32), hipMemcpyHostToDevice, d->stream));
        hipLaunchKernelGGL(k_gather_records, dim3(grid_for(nUn, 256)), dim3(256), 0, d->stream, dIds, nUn, d->posOf, d->idOf, d->right, d->left, dRec);
        std::vector<u64> rec(2 * (size_t)nUn); HIPCHK(hipMemcpyAsync(rec.data(), dRec, rec.size() * sizeof(u64), hipMemcpyDeviceToHost, d->stream)); HIPCHK(hipStreamSynchronize(d->stream));
        std::vector<u32> need(unresolved.begin(), unresolved.begin() + nUn);
        for (u64 r : rec) { const u32 id = (u32)(r & ((1ull << 40) - 1)); if (id) need.push_back(id); }
        std::sort(need.begin(), need.end()); need.erase(std::unique(need.begin(), need.end()), need.end());
        HIPCHK(hipMemcpyAsync(dNeed, need.data(), need.size() * sizeof(u32), hipMemcpyHostToDevice, d->stream));
        const unsigned blocks = (unsigned)std::min<u64>(grid_for(n, 256), 256ull * 8);
        // (every candidate that touches a read of the short list was emitted by a read of the list or by a partner of one: at most 2 per read and partner)
        cap = 2 * (u64)need.size() * 3 + 64; { WS(nb_, EdgeCand, WS_NEAR, cap); buf = nb_; }
        HIPCHK(hipMemsetAsync(d->d_counters + CTR_LIST, 0, sizeof(u64), d->stream));
        hipLaunchKernelGGL(k_red_collect_few, dim3(blocks), dim3(256), 0, d->stream, d->cand, (u64)n, dNeed, (u32)need.size(), dIds, nUn, buf, cap, d->d_counters + CTR_LIST);
        HIPCHK(hipGetLastError());
        u64 cnt = 0; { int rc = read_counters(d, CTR_LIST, 1, &cnt, err); if (rc) return rc; }
        if (cnt <= cap) {                                                  // (else: the general form below -- the 0x80 flags are idempotent)
            out.resize(cnt); if (cnt) HIPCHK(hipMemcpy(out.data(), buf, cnt * sizeof(EdgeCand), hipMemcpyDeviceToHost));
            return 0;
        }
    }
    { int rc = ensure_status_by_id(d, err); if (rc) return rc; }
    WS(need, uint8_t, WS_NEED, d->N + 1); HIPCHK(hipMemsetAsync(need, 0, d->N + 1, d->stream));
    hipLaunchKernelGGL(k_red_mark, dim3(grid_for(n, 256)), dim3(256), 0, d->stream, d->cand, (u64)n, d->status, need);
    // first a dry count (cap 0 keeps the flagging idempotent), then the real collection
    HIPCHK(hipMemsetAsync(d->d_counters + CTR_LIST, 0, sizeof(u64), d->stream));
    hipLaunchKernelGGL(k_red_collect, dim3(grid_for(n, 256)), dim3(256), 0, d->stream, d->cand, (u64)n, d->status, need, (EdgeCand*)nullptr, (u64)0, d->d_counters + CTR_LIST);
    u64 cnt = 0; { int rc = read_counters(d, CTR_LIST, 1, &cnt, err); if (rc) return rc; }
    if (cnt) {
        cap = cnt; { WS(nb_, EdgeCand, WS_NEAR, cap); buf = nb_; }
        HIPCHK(hipMemsetAsync(d->d_counters + CTR_LIST, 0, sizeof(u64), d->stream));
        hipLaunchKernelGGL(k_red_collect, dim3(grid_for(n, 256)), dim3(256), 0, d->stream, d->cand, (u64)n, d->status, need, buf, cap, d->d_counters + CTR_LIST);
        HIPCHK(hipStreamSynchronize(d->stream));
        out.resize(cnt); HIPCHK(hipMemcpy(out.data(), buf, cnt * sizeof(EdgeCand), hipMemcpyDeviceToHost));
        for (auto& e : out) e.type &= 0x7Fu;
    }
    return 0;
}

// ReadLoader::getIdOfRead for a batch (kernels_find.inc).  Queries go through in chunks bounded in queries and in bytes, so a launch stays far below 2^32 threads
// and the staging is bounded (a chunk always takes one query at least: a single query larger than the bound is staged whole).  Every buffer but the directory is a
// transient allocation of this call; the steps' results, their phase blocks and the workspace arena are not touched.  Returns 1 when no read store is resident
// (the caller searches its host copy instead).
constexpr u64 FIND_CHUNK_BYTES = 256ull << 20;      // ASCII per chunk, and the chunk's packed image
struct FindRun {                                                                     // one call: which store, the chunk bound -- and the chunks' seven buffers (slots of tmp) and timers
    const u64* store = nullptr; bool byPos = false; int S = 0; u64 qcap = 0; u32 maxLen = 0;
    DevTmp tmp; StreamLap pack, search;
    explicit FindRun(hipStream_t s) : pack(s), search(s) {}
};
struct FindChunk { u64 q = 0; unsigned char* db = nullptr; u64* dof = nullptr; signed char* sign = nullptr; long long* dids = nullptr; u64* cnt = nullptr; };
// what every call does once: which store, the directory (once per read set), the chunk bound.  Returns 1 when no read store is resident.
static int find_begin(Device* d, FindRun& R, FindStats* st, std::string& err) {
    R.byPos = d->reads == nullptr;
    if (R.byPos && !(d->readsLoc && d->posOf)) return 1;
    R.store = R.byPos ? d->readsLoc : d->reads; R.S = d->S; const int S = d->S; const u64 N = d->N;
    if (S != 4 && S != 8 && S != 16 && S != 32) { err = "unsupported words-per-read"; return SAGE2OV_ERR_INTERNAL; }
    HIPCHK(R.pack.create()); HIPCHK(R.search.create());
    *st = FindStats(); st->byPos = R.byPos;
    if (!d->findDir) {                                                               // the directory: once per read set
        int B = 0; while ((1ull << B) < N) B++;                                      // ceil(log2 N)
        B = std::min(FIND_B_MAX, std::max(FIND_B_MIN, B - 1));
        u32* dir = nullptr; HIPCHK(hipMalloc(&dir, ((size_t)(1u << B) + 1) * sizeof(u32)));
        HIPCHK(R.pack.start());                                                      // (the pack timer is free until the first chunk)
        if (R.byPos) hipLaunchKernelGGL(k_find_dir<true>, dim3(grid_for((1u << B) + 1, 256)), dim3(256), 0, d->stream, R.store, d->posOf, (u32)N, S, B, dir);
        else hipLaunchKernelGGL(k_find_dir<false>, dim3(grid_for((1u << B) + 1, 256)), dim3(256), 0, d->stream, R.store, d->posOf, (u32)N, S, B, dir);
        hipError_t e = hipGetLastError(); if (e == hipSuccess) e = R.pack.stop(st->dir_ms);
        if (e != hipSuccess) { hipFree(dir); err = std::string("read-id directory: ") + hipGetErrorString(e); return SAGE2OV_ERR_DEVICE; }
        d->findDir = dir; d->findDirBits = B;
    }
    st->dirBits = (u32)d->findDirBits;
    const long long forced = d->opt.num("SAGE2OV_TEST_FIND_BATCH", 0);             // test-only: queries per chunk
    R.qcap = forced > 0 ? (u64)forced : std::min<u64>(1ull << 22, FIND_CHUNK_BYTES / ((u64)S * sizeof(u64)));
    const u32 lenCap = (u32)((64 * S - (S > 16 ? 11 : 9)) / 2);                    // bases a slot of this layout holds
    R.maxLen = std::min<u32>((u32)std::max(d->maxL, 0), lenCap);
    return 0;
}
// end of the chunk that starts at query r0: bounded in queries and in bytes, one query at least
static u64 find_chunk_end(const FindRun& R, const uint64_t* off, u64 n, u64 r0) {
    u64 r1 = r0 + 1; const u64 lastQ = std::min<u64>(n, r0 + R.qcap);
    while (r1 < lastQ && off[r1 + 1] - off[r0] <= FIND_CHUNK_BYTES) r1++;
    return r1;
}
// the body of one chunk, queries [r0, r1): upload, k_org_classify, k_find_pack, k_find_search.  The ids stay on the device (C.dids, with the sign bytes and
// the counters [0..5] k_org_classify, [6] found); R.pack and R.search bracket pack and search.  Nothing is synchronised here.
static int find_chunk(Device* d, FindRun& R, const char* bases, const uint64_t* off, u64 r0, u64 r1, std::vector<u64>& ho, FindChunk& C, std::string& err) {
    const int S = R.S; const bool byPos = R.byPos; const u64* store = R.store;
    const u64 q = r1 - r0, nbytes = off[r1] - off[r0];
    ho.resize(q + 1); for (u64 x = 0; x <= q; x++) ho[x] = off[r0 + x] - off[r0];
    DevTmp& T = R.tmp;
    unsigned char* db = T.slot<unsigned char>(0, nbytes + 64); u64* dof = T.slot<u64>(1, q + 1); u32* flag = T.slot<u32>(2, q);
    u64* img = T.slot<u64>(3, q * S); signed char* sign = T.slot<signed char>(4, q); long long* dids = T.slot<long long>(5, q);
    u64* cnt = T.slot<u64>(6, 8);
    if (!db || !dof || !flag || !img || !sign || !dids || !cnt) { err = "read-id lookup: out of device memory"; return SAGE2OV_ERR_NOMEM; }
    if (nbytes) HIPCHK(hipMemcpyAsync(db, bases + off[r0], nbytes, hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipMemcpyAsync(dof, ho.data(), (q + 1) * sizeof(u64), hipMemcpyHostToDevice, d->stream));
    const u64 init[8] = {0, 0, 0, 0, ~0ull, 0, 0, 0}; HIPCHK(hipMemcpyAsync(cnt, init, sizeof init, hipMemcpyHostToDevice, d->stream));      // [0..5] k_org_classify, [6] found
    HIPCHK(R.pack.start());
    hipLaunchKernelGGL(k_org_classify, dim3(grid_for(q, 256)), dim3(256), 0, d->stream, db, dof, (u64)q, (u32)d->k, R.maxLen, flag, cnt);
    hipLaunchKernelGGL(k_find_pack, dim3(grid_for(q, 256)), dim3(256), 0, d->stream, db, dof, (u64)q, flag, S, img, sign);
    HIPCHK(R.pack.end()); HIPCHK(R.search.start());
    const dim3 grid(grid_for(q * (u64)(S / 2), 256)), block(256); unsigned long long* fnd = (unsigned long long*)(cnt + 6);
#define S2_FIND(SS) do { if (byPos) hipLaunchKernelGGL((k_find_search<SS, true>), grid, block, 0, d->stream, store, d->posOf, d->findDir, d->findDirBits, img, sign, (u32)q, dids, fnd); \
                         else hipLaunchKernelGGL((k_find_search<SS, false>), grid, block, 0, d->stream, store, d->posOf, d->findDir, d->findDirBits, img, sign, (u32)q, dids, fnd); } while (0)
    if (S == 4) S2_FIND(4); else if (S == 8) S2_FIND(8); else if (S == 16) S2_FIND(16); else S2_FIND(32);
#undef S2_FIND
    HIPCHK(hipGetLastError());
    HIPCHK(R.search.end());
    C.q = q; C.db = db; C.dof = dof; C.sign = sign; C.dids = dids; C.cnt = cnt;
    return 0;
}
int dev_find_ids(Device* d, const char* bases, const uint64_t* off, uint64_t n, int64_t* ids, FindStats* st, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    FindRun R(d->stream);
    { const int rc = find_begin(d, R, st, err); if (rc) return rc; }
    std::vector<u64> ho;
    for (u64 r0 = 0; r0 < n;) {
        const u64 r1 = find_chunk_end(R, off, n, r0); FindChunk C;
        { const int rc = find_chunk(d, R, bases, off, r0, r1, ho, C, err); if (rc) return rc; }
        const u64 q = C.q; u64 hc[8];
        HIPCHK(hipMemcpyAsync(ids + r0, C.dids, q * sizeof(long long), hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipMemcpyAsync(hc, C.cnt, sizeof hc, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
        R.pack.add(st->pack_ms); R.search.add(st->search_ms); st->launches++;
        st->found += hc[6]; st->not_good += q - hc[1] - hc[5];                       // hc[1]: good and no longer than the store's longest; hc[5]: good but longer
        r0 = r1;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- the mate-pair table (kernels_mates.inc)
// MatePair::processMatePairs (matePair.cpp:161-239) on the device.  The table of a library (keys, counts, firsts: sorted by key, unique) and the pending
// records of the call in progress live in allocations of their own (Device::mates): not in the phase block, not in the workspace arena, so the steps and
// the table never see each other.  Everything else is a transient allocation of the call.
constexpr u64 MATE_FLUSH_RECORDS = 1ull << 25;      // pending records at which a flush runs: one sort stays far below 2^32 records (k_rs_scatter's positions are u32)
static Mates* mates_of(Device* d) { if (!d->mates) d->mates = new Mates(); return d->mates; }
static void mates_drop_pending(Mates* m) { hipFree(m->pkey); hipFree(m->pord); m->pkey = m->pord = nullptr; m->pn = m->pcap = 0; }
static void mates_release(Device* d) {
    if (!d->mates) return;
    for (auto& L : d->mates->lib) { hipFree(L.key); hipFree(L.cnt); hipFree(L.first); }
    mates_drop_pending(d->mates); delete d->mates; d->mates = nullptr;
}
void dev_mates_clear(Device* d) { hipSetDevice(d->ordinal); mates_release(d); }
void dev_mates_abort(Device* d) { if (d->mates) { hipSetDevice(d->ordinal); mates_drop_pending(d->mates); } }
uint64_t dev_mates_count(Device* d, int library) { return d->mates ? d->mates->lib[library].n : 0; }
// the 8-bit digits of a key (from:30 | to:30 | t_from:1 | t_to:1) that can be non-zero when no id exceeds N: `to` and the types end at bit 2 + b, `from` at 32 + b
static int mate_passes(u64 N, int* shifts) {
    int b = 0; while ((N >> b) != 0) b++;                                            // ceil(log2(N + 1))
    int np = 0;
    for (int p = 0; p < 8; p++) { const int lo = 8 * p; if (lo < 2 + b || (lo >= 32 && lo < 32 + b)) shifts[np++] = lo; }
    return np;
}
static int mate_nomem(std::string& err) { err = "mate table: out of device memory"; return SAGE2OV_ERR_NOMEM; }
// stable LSD sort of (key, index 0 .. n-1) by the passes of mate_passes; the sorted keys and indices come back in *ks / *vs (buffers of B)
static int mate_sort(Device* d, DevTmp& B, u64* k0, u32 n, const int* shifts, int np, u64** ks, u32** vs, MateStats* st, std::string& err) {
    const u64 nh = rs_hist_words(n);
    const RsBufs R = {{k0, B.get<u64>(n)}, {B.get<u32>(n), B.get<u32>(n)}, B.get<u32>(nh), B.get<u32>(nh), B.get<u64>(scan_partial_words(nh))};
    if (!R.k[1] || !R.v[0] || !R.v[1] || !R.hist || !R.hscan || !R.partial) return mate_nomem(err);
    hipLaunchKernelGGL(k_mate_iota, dim3(grid_for(n, 256)), dim3(256), 0, d->stream, R.v[0], n);
    int side = 0; { const int rc = radix_sort_pairs(d, R, n, shifts, np, &side, err); if (rc) return rc; }
    st->passes += np;
    B.release(R.hist); B.release(R.hscan); B.release(R.partial); B.release(R.v[side ^ 1]); if (R.k[side ^ 1] != k0) B.release(R.k[side ^ 1]);
    *ks = R.k[side]; *vs = R.v[side];
    return 0;
}
// heads of the sorted keys: hp[e] = position of the e-th distinct key, hp[E] = n
static int mate_heads(Device* d, DevTmp& B, const u64* keys, u32 n, u32** hp_out, u32* E_out, std::string& err) {
    u32* flag = B.get<u32>(n); u32* pos = B.get<u32>(n); u64* partial = B.get<u64>(scan_partial_words(n));
    if (!flag || !pos || !partial) return mate_nomem(err);
    hipLaunchKernelGGL(k_mate_heads, dim3(grid_for(n, 256)), dim3(256), 0, d->stream, keys, n, flag);
    u64 E = 0; { const int rc = scan_u32(d, flag, n, pos, partial, &E, err); if (rc) return rc; }
    u32* hp = B.get<u32>(E + 1); if (!hp) return mate_nomem(err);
    { const int rc = head_positions(d, flag, pos, n, hp, E, err); if (rc) return rc; }
    HIPCHK(hipStreamSynchronize(d->stream));
    B.release(flag); B.release(pos); B.release(partial);
    *hp_out = hp; *E_out = (u32)E;
    return 0;
}
// sort, reduce and merge the pending records into the library's table
int dev_mates_flush(Device* d, int library, MateStats* st, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    Mates* M = d->mates; if (!M || !M->pn) { if (M) mates_drop_pending(M); return 0; }
    MateLib& L = M->lib[library]; const u32 n = (u32)M->pn;
    int shifts[8]; const int np = mate_passes(d->N, shifts);
    DevTmp B; StreamLap lap(d->stream); HIPCHK(lap.create());
    u64 *ks = nullptr; u32 *vs = nullptr, *hp = nullptr; u32 E = 0;
    HIPCHK(lap.start());
    { const int rc = mate_sort(d, B, M->pkey, n, shifts, np, &ks, &vs, st, err); if (rc) return rc; }
    HIPCHK(lap.stop(st->sort_ms));
    HIPCHK(lap.start());
    { const int rc = mate_heads(d, B, ks, n, &hp, &E, err); if (rc) return rc; }
    u64* ek = B.get<u64>((u64)E + L.n); u64* ec = B.get<u64>((u64)E + L.n); u64* ef = B.get<u64>((u64)E + L.n);      // (room for the table behind the new entries: the merge's input)
    if (!ek || !ec || !ef) return mate_nomem(err);
    hipLaunchKernelGGL(k_mate_reduce, dim3(grid_for(E, 256)), dim3(256), 0, d->stream, ks, vs, M->pord, hp, E, ek, ec, ef);
    HIPCHK(hipGetLastError());
    HIPCHK(lap.stop(st->reduce_ms));
    if (ks != M->pkey) B.release(ks); B.release(vs); B.release(hp);
    mates_drop_pending(M);
    st->flushes++;
    if (!L.n) {                                                                      // a library's first entries: they are its table
        B.keep(ek); B.keep(ec); B.keep(ef); L.key = ek; L.cnt = ec; L.first = ef; L.n = E;
        return 0;
    }
    if ((u64)E + L.n >= (1ull << 32) - RS_TILE) { err = "mate table: more than 2^32 entries in one library"; return SAGE2OV_ERR_LIMIT; }
    HIPCHK(lap.start());
    const u32 m = E + (u32)L.n;
    HIPCHK(hipMemcpyAsync(ek + E, L.key, L.n * sizeof(u64), hipMemcpyDeviceToDevice, d->stream));
    HIPCHK(hipMemcpyAsync(ec + E, L.cnt, L.n * sizeof(u64), hipMemcpyDeviceToDevice, d->stream));
    HIPCHK(hipMemcpyAsync(ef + E, L.first, L.n * sizeof(u64), hipMemcpyDeviceToDevice, d->stream));
    { const int rc = mate_sort(d, B, ek, m, shifts, np, &ks, &vs, st, err); if (rc) return rc; }
    u32 E2 = 0; { const int rc = mate_heads(d, B, ks, m, &hp, &E2, err); if (rc) return rc; }
    u64* nk = B.get<u64>(E2); u64* nc = B.get<u64>(E2); u64* nf = B.get<u64>(E2);
    if (!nk || !nc || !nf) return mate_nomem(err);
    hipLaunchKernelGGL(k_mate_merge, dim3(grid_for(E2, 256)), dim3(256), 0, d->stream, ks, vs, ec, ef, hp, E2, nk, nc, nf);
    HIPCHK(hipGetLastError());
    HIPCHK(lap.stop(st->merge_ms));
    hipFree(L.key); hipFree(L.cnt); hipFree(L.first);
    B.keep(nk); B.keep(nc); B.keep(nf); L.key = nk; L.cnt = nc; L.first = nf; L.n = E2;
    return 0;
}
// room for nrec more records in the pending buffer (its records are kept)
static int mates_pending_reserve(Device* d, Mates* M, u64 nrec, u64 bound, std::string& err) {
    if (M->pn + nrec <= M->pcap) return 0;
    const u64 cap = std::max<u64>(M->pn + nrec, std::min<u64>(2 * M->pcap, bound + (1ull << 22)));
    u64 *nk = nullptr, *no = nullptr;
    if (hipMalloc(&nk, cap * sizeof(u64)) != hipSuccess || hipMalloc(&no, cap * sizeof(u64)) != hipSuccess) { (void)hipGetLastError(); hipFree(nk); err = "mate table: out of device memory"; return SAGE2OV_ERR_NOMEM; }
    if (M->pn) { hipMemcpyAsync(nk, M->pkey, M->pn * sizeof(u64), hipMemcpyDeviceToDevice, d->stream); hipMemcpyAsync(no, M->pord, M->pn * sizeof(u64), hipMemcpyDeviceToDevice, d->stream); }
    hipError_t e = hipStreamSynchronize(d->stream);
    hipFree(M->pkey); hipFree(M->pord); M->pkey = nk; M->pord = no; M->pcap = cap;
    if (e != hipSuccess) { err = std::string("mate table: ") + hipGetErrorString(e); return SAGE2OV_ERR_DEVICE; }
    return 0;
}
// One readsArray of processMatePairs: reads [0, n) of the call, n even (the caller drops a trailing odd read), pair0 = ordinal of the call's first pair in
// its library.  The chunks hold an even number of queries, so a pair is never cut from its ids.  Records collect in the pending buffer, which is flushed at
// MATE_FLUSH_RECORDS (SAGE2OV_TEST_MATE_FLUSH: a bound for tests); the caller ends its call with dev_mates_flush.  Returns 1 (and does nothing) when no
// read store is resident.
int dev_mates_add(Device* d, const char* bases, const uint64_t* off, uint64_t n, int library, uint64_t pair0, MateStats* st, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (d->N >= (1ull << 30)) { err = "mate table: read ids beyond 2^30 - 1"; return SAGE2OV_ERR_LIMIT; }
    FindRun R(d->stream); FindStats fs;
    { const int rc = find_begin(d, R, &fs, err); if (rc) return rc; }
    st->find_ms += fs.dir_ms;
    R.qcap = std::min<u64>((R.qcap + 1) & ~1ull, 1ull << 22);                      // an even number of queries per chunk (a forced odd value: the next even one)
    const long long forced = d->opt.num("SAGE2OV_TEST_MATE_FLUSH", 0);
    const u64 bound = forced > 0 ? (u64)forced : MATE_FLUSH_RECORDS;
    Mates* M = mates_of(d); StreamLap lap(d->stream); HIPCHK(lap.create());
    std::vector<u64> ho;
    for (u64 r0 = 0; r0 < n;) {
        u64 r1 = find_chunk_end(R, off, n, r0); if ((r1 - r0) & 1) r1++;            // (n is even: r1 <= n)
        FindChunk C;
        { const int rc = find_chunk(d, R, bases, off, r0, r1, ho, C, err); if (rc) return rc; }
        HIPCHK(hipStreamSynchronize(d->stream));
        R.pack.add(st->find_ms); R.search.add(st->find_ms);
        st->chunks++;
        const u32 np = (u32)(C.q / 2);
        HIPCHK(lap.start());
        DevTmp B; u32* keep = B.get<u32>(np); u32* pos = B.get<u32>(np); u64* partial = B.get<u64>(scan_partial_words(np));
        if (!keep || !pos || !partial) return mate_nomem(err);
        unsigned long long* kinds = (unsigned long long*)(C.cnt + 6); HIPCHK(hipMemsetAsync(kinds, 0, 2 * sizeof(u64), d->stream));      // ([6], [7] of the chunk's counters: read above, free now)
        hipLaunchKernelGGL(k_mate_keep, dim3(grid_for(np, 256)), dim3(256), 0, d->stream, C.dids, C.sign, C.db, C.dof, np, (u32)d->k, R.maxLen, keep, kinds);
        u64 nrec = 0; { const int rc = scan_u32(d, keep, np, pos, partial, &nrec, err); if (rc) return rc; }
        u64 hk[2]; HIPCHK(hipMemcpyAsync(hk, kinds, sizeof hk, hipMemcpyDeviceToHost, d->stream)); HIPCHK(hipStreamSynchronize(d->stream));
        st->seen += np; st->not_good += hk[0]; st->not_found += hk[1]; st->added += nrec / 2;
        { const int rc = mates_pending_reserve(d, M, nrec, bound, err); if (rc) return rc; }
        if (nrec) hipLaunchKernelGGL(k_mate_records, dim3(grid_for(np, 256)), dim3(256), 0, d->stream, C.dids, keep, pos, np, 2ull * (pair0 + r0 / 2), M->pkey + M->pn, M->pord + M->pn);
        HIPCHK(hipGetLastError());
        HIPCHK(lap.stop(st->records_ms));
        M->pn += nrec;
        if (M->pn >= bound) { const int rc = dev_mates_flush(d, library, st, err); if (rc) return rc; }
        r0 = r1;
    }
    return 0;
}
// One reads_add_* call as one mates call, from the ids dev_organize_reads kept (sage2ov_mates_from_reads; k_pair_slots, k_pair_keep): see
// sage2ov_internal.h.  Chunks of 2^22 pairs bound the transient ids; the records collect in the pending buffer exactly as dev_mates_add's do, flush bound included.
void dev_pairing_release(Device* d) { if (d->pairId) { hipSetDevice(d->ordinal); hipFree(d->pairId); } d->pairId = nullptr; d->pairN = 0; d->pairRaw = d->pairValid = false; }
int dev_mates_pair_call(Device* d, bool raw, const uint32_t* ord, uint64_t nStaged, uint64_t first, uint64_t records, int library, uint64_t pair0, MateStats* st, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (raw) ord = nullptr;
    if (!d->pairValid || d->pairRaw != raw || (!raw && nStaged && !ord)) { err = "pairing: the organiser kept no ids of this kind"; return SAGE2OV_ERR_ARG; }
    if (d->N >= (1ull << 30)) { err = "mate table: read ids beyond 2^30 - 1"; return SAGE2OV_ERR_LIMIT; }
    if (records >= (1ull << 32) - RS_TILE) { err = "pairing: too many input records in one call"; return SAGE2OV_ERR_LIMIT; }
    // every index the kernels form stays inside its array: the staged range (or the raw range) inside the ids, every ordinal inside the call's records
    if (!raw ? (first > d->pairN || nStaged > d->pairN - first) : (first > d->pairN || records > d->pairN - first)) { err = "pairing: a call outside the staged reads"; return SAGE2OV_ERR_INTERNAL; }
    if (!raw) for (u64 x = 0; x < nStaged; x++) if (ord[x] >= records) { err = "pairing: a record ordinal outside its call"; return SAGE2OV_ERR_INTERNAL; }
    const u64 npAll = records / 2; if (!npAll) return 0;
    const long long forced = d->opt.num("SAGE2OV_TEST_MATE_FLUSH", 0);
    const u64 bound = forced > 0 ? (u64)forced : MATE_FLUSH_RECORDS;
    Mates* M = mates_of(d); StreamLap lap(d->stream); HIPCHK(lap.create());
    DevTmp B; u32* slotOf = nullptr;
    HIPCHK(lap.start());
    if (!raw) {
        slotOf = B.get<u32>(records); u32* dord = B.get<u32>(nStaged); if (!slotOf || !dord) return mate_nomem(err);
        HIPCHK(hipMemsetAsync(slotOf, 0, records * sizeof(u32), d->stream));
        if (nStaged) {
            HIPCHK(hipMemcpyAsync(dord, ord, nStaged * sizeof(u32), hipMemcpyHostToDevice, d->stream));
            hipLaunchKernelGGL(k_pair_slots, dim3(grid_for(nStaged, 256)), dim3(256), 0, d->stream, dord, (u64)nStaged, (u32)first, slotOf);
        }
        HIPCHK(hipStreamSynchronize(d->stream)); B.release(dord);
    }
    const int* idOf = raw ? d->pairId + first : d->pairId;
    const long long fb = d->opt.num("SAGE2OV_TEST_FIND_BATCH", 0);                   // (tests: records per chunk, as the look-up chunks of dev_mates_add)
    const u64 CH = fb > 0 ? (u64)((fb + 1) / 2) : 1ull << 22, npc = std::min(CH, npAll);
    long long* ids = B.get<long long>(2 * npc); u32* keep = B.get<u32>(npc); u32* pos = B.get<u32>(npc); u64* partial = B.get<u64>(scan_partial_words(npc));
    unsigned long long* kinds = (unsigned long long*)B.get<u64>(1);
    if (!ids || !keep || !pos || !partial || !kinds) return mate_nomem(err);
    HIPCHK(lap.stop(st->find_ms));
    for (u64 p0 = 0; p0 < npAll; p0 += CH) {
        const u32 np = (u32)std::min(CH, npAll - p0);
        st->chunks++;
        HIPCHK(lap.start());
        HIPCHK(hipMemsetAsync(kinds, 0, sizeof(u64), d->stream));
        hipLaunchKernelGGL(k_pair_keep, dim3(grid_for(np, 256)), dim3(256), 0, d->stream, idOf, slotOf, 2 * p0, np, ids, keep, kinds);
        u64 nrec = 0; { const int rc = scan_u32(d, keep, np, pos, partial, &nrec, err); if (rc) return rc; }
        u64 hk = 0; HIPCHK(hipMemcpyAsync(&hk, kinds, sizeof hk, hipMemcpyDeviceToHost, d->stream)); HIPCHK(hipStreamSynchronize(d->stream));
        st->seen += np; st->not_good += hk; st->added += nrec / 2;
        { const int rc = mates_pending_reserve(d, M, nrec, bound, err); if (rc) return rc; }
        if (nrec) hipLaunchKernelGGL(k_mate_records, dim3(grid_for(np, 256)), dim3(256), 0, d->stream, ids, keep, pos, np, 2ull * (pair0 + p0), M->pkey + M->pn, M->pord + M->pn);
        HIPCHK(hipGetLastError());
        HIPCHK(lap.stop(st->records_ms));
        M->pn += nrec;
        if (M->pn >= bound) { const int rc = dev_mates_flush(d, library, st, err); if (rc) return rc; }
    }
    return 0;
}
// the table of a library as it lies on the device: n = dev_mates_count entries each; offsets: N + 2 values (k_mate_offsets), or null
int dev_mates_export(Device* d, int library, uint64_t* key, uint64_t* cnt, uint64_t* first, uint64_t* offsets, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    static const MateLib none; const MateLib& L = d->mates ? d->mates->lib[library] : none;
    if (L.n) {
        HIPCHK(hipMemcpyAsync(key, L.key, L.n * sizeof(u64), hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipMemcpyAsync(cnt, L.cnt, L.n * sizeof(u64), hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipMemcpyAsync(first, L.first, L.n * sizeof(u64), hipMemcpyDeviceToHost, d->stream));
    }
    if (offsets) {
        DevTmp B; u64* dofs = B.get<u64>(d->N + 2); if (!dofs) return mate_nomem(err);
        hipLaunchKernelGGL(k_mate_offsets, dim3(grid_for(d->N + 2, 256)), dim3(256), 0, d->stream, L.key, (u32)L.n, (u32)d->N, dofs);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(offsets, dofs, (d->N + 2) * sizeof(u64), hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
    }
    HIPCHK(hipStreamSynchronize(d->stream));
    return 0;
}
// a table built on the host moves to the device (a context whose device had no store resident when the table was begun)
int dev_mates_import(Device* d, int library, const uint64_t* key, const uint64_t* cnt, const uint64_t* first, uint64_t n, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    MateLib& L = mates_of(d)->lib[library];
    hipFree(L.key); hipFree(L.cnt); hipFree(L.first); L = MateLib();
    if (!n) return 0;
    HIPCHK(hipMalloc(&L.key, n * sizeof(u64))); HIPCHK(hipMalloc(&L.cnt, n * sizeof(u64))); HIPCHK(hipMalloc(&L.first, n * sizeof(u64)));
    HIPCHK(hipMemcpyAsync(L.key, key, n * sizeof(u64), hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipMemcpyAsync(L.cnt, cnt, n * sizeof(u64), hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipMemcpyAsync(L.first, first, n * sizeof(u64), hipMemcpyHostToDevice, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    L.n = n;
    return 0;
}

int dev_meminfo(Device* d, uint64_t* out4, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    size_t fr = 0, to = 0; HIPCHK(hipMemGetInfo(&fr, &to)); mem_sample(d);
    u64 arena = 0; for (auto& b : d->ws) if (!b.epoch) arena += b.cap;
    arena += d->ph.cap;                                                            // (diet mode: the phase block; what was carved out of it is not counted twice)
    if (d->opt.get("SAGE2OV_MEMINFO")) {                                         // diagnostic: the big buffers of the arena, by workspace id (enum order)
        fprintf(stderr, "[meminfo] free %.2f GB of %.2f, lowest %.2f, arena %.2f GB, N %llu, diet %d:", fr / 1e9, to / 1e9, d->memLow / 1e9, arena / 1e9, (unsigned long long)d->N, (int)d->diet);
        for (int x = 0; x < WS_COUNT; x++) if (d->ws[x].cap >= (64u << 20)) fprintf(stderr, " ws%d=%.2f", x, d->ws[x].cap / 1e9);
        fprintf(stderr, "\n");
    }
    out4[0] = fr; out4[1] = to; out4[2] = d->memLow; out4[3] = arena; return 0;
}
int dev_debug_table(Device* d, uint64_t* out5, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    u64* dk = nullptr; HIPCHK(hipMalloc(&dk, 8 * sizeof(u64))); HIPCHK(hipMemsetAsync(dk, 0, 8 * sizeof(u64), d->stream));
    hipLaunchKernelGGL(k_debug_table, dim3(grid_for_capped(d->T, 256)), dim3(256), 0, d->stream, d->slots, (u64)d->T, dk);
    HIPCHK(hipStreamSynchronize(d->stream));
    HIPCHK(hipMemcpy(out5, dk, 5 * sizeof(u64), hipMemcpyDeviceToHost)); hipFree(dk); return 0;
}
int dev_debug_keys(Device* d, uint64_t* out, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (!d->reads) { err = "the id-ordered read store has been released (memory-diet mode)"; return SAGE2OV_ERR_ARG; }
    u64* dk = nullptr; HIPCHK(hipMalloc(&dk, 8 * d->N * sizeof(u64)));
    hipLaunchKernelGGL(k_debug_keys, dim3(grid_for(4 * d->N, 256)), dim3(256), 0, d->stream, d->reads, (u64)d->N, d->S, d->h, dk);
    HIPCHK(hipStreamSynchronize(d->stream));
    HIPCHK(hipMemcpy(out, dk, 8 * d->N * sizeof(u64), hipMemcpyDeviceToHost));
    hipFree(dk); return 0;
}
// diagnostic: hit lists (economyGraph.cpp:591-633 semantics) of EVERY read, as if all were unresolved
int dev_debug_all_hits(Device* d, std::vector<Hit>& hits, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    const u64 N = d->N; DevTmp tmp;
    uint8_t* saved = tmp.get<uint8_t>(N + 1); if (!saved) { err = "debug hits: out of device memory"; return SAGE2OV_ERR_NOMEM; }
    HIPCHK(hipStreamSynchronize(d->stream));
    { int rc = ensure_status_by_id(d, err); if (rc) return rc; }           // (the by-id array is the one written here, statusP refreshed from it: both agree, before and after)
    d->statusGen++; d->unresGen = 0;
    HIPCHK(hipMemcpyAsync(saved, d->status, N + 1, hipMemcpyDeviceToDevice, d->stream));
    HIPCHK(hipMemsetAsync(d->status, 0, N + 1, d->stream));
    u64 cap = std::max<u64>(1 << 16, N * 128);
    Hit* dh = tmp.get<Hit>(cap); if (!dh) { err = "debug hits: out of device memory"; return SAGE2OV_ERR_NOMEM; }
    HIPCHK(hipMemsetAsync(d->d_counters + CTR_HIT_CURSOR, 0, sizeof(u64), d->stream));
    ProbeArgs A = base_args(d); A.lo = 1; A.hi = N + 1; A.hits = dh; A.hits_cap = cap;
    int rc = refresh_status_by_pos(d, err); if (!rc) rc = launch_probe<1>(d, A, err);
    u64 nh = 0;
    if (!rc) { int rcr = read_counters(d, CTR_HIT_CURSOR, 1, &nh, err); if (rcr) return rcr; }
    if (!rc && nh > cap) { err = "debug hit buffer too small"; rc = SAGE2OV_ERR_LIMIT; }
    if (!rc) { hits.resize(nh); if (nh) HIPCHK(hipMemcpy(hits.data(), dh, nh * sizeof(Hit), hipMemcpyDeviceToHost)); }
    HIPCHK(hipMemcpyAsync(d->status, saved, N + 1, hipMemcpyDeviceToDevice, d->stream));
    { int rc2 = refresh_status_by_pos(d, err); if (!rc) rc = rc2; }      // (statusP is what the reciprocal pass left again)
    HIPCHK(hipStreamSynchronize(d->stream));
    return rc;
}

int dev_append_edges(Device* d, const EdgeCand* e, uint64_t n, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (n == 0) return 0;
    if (d->n_cand + n > d->cand_cap) {
        { int rc = cand_resize(d, d->n_cand + n + 1024, d->n_cand, err); if (rc) return rc; }
    }
    HIPCHK(hipMemcpyAsync(d->cand + d->n_cand, e, n * sizeof(EdgeCand), hipMemcpyHostToDevice, d->stream)); HIPCHK(hipStreamSynchronize(d->stream));
    d->n_cand += n;
    return 0;
}

int dev_download_edges(Device* d, std::vector<FinalEdge>& out, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    out.resize(d->n_final);
    if (d->n_final) HIPCHK(hipMemcpy(out.data(), d->final_edges, d->n_final * sizeof(FinalEdge), hipMemcpyDeviceToHost));
    return 0;
}
int dev_upload_edges(Device* d, const std::vector<FinalEdge>& in, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    WS(fe, FinalEdge, WS_FINAL, std::max<size_t>(1, in.size()));
    if (!in.empty()) HIPCHK(hipMemcpy(fe, in.data(), in.size() * sizeof(FinalEdge), hipMemcpyHostToDevice));
    d->final_edges = fe; d->n_final = in.size();
    return 0;
}
int dev_convert(Device* d, uint64_t* n_final, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    const u64 N = d->N, n = d->n_cand;
    d->final_edges = nullptr; d->n_final = 0;
    HIPCHK(hipEventRecord(d->ev[0], d->stream));
    if (n) {
        if (n >= (1ull << 32) - PT_TILE) { err = "too many edge candidates"; return SAGE2OV_ERR_LIMIT; }
        // Round 3: the candidates arrive in POSITION order of their emitters (their `from` ids are random): a stable LSD radix sort by `from`
        // (kernels_partition.inc, <= 9 bits per pass; the candidate list itself is only read) makes every read's list contiguous without an atomic --
        // the counting form this replaces (two atomics per candidate on per-read counters) took 5.4 ms at BASELINE configs[2], 3.4 when the
        // candidates still came in id order.
        PtBufs B; B.W = 4; B.src0 = (const u32*)d->cand;
        { WS(a, u32, WS_PT_K0, 4 * (n + 4)); B.E[0] = a; } { WS(a, u32, WS_PT_K1, 4 * (n + 4)); B.E[1] = a; }
        const u32 ntiles = (u32)((n + PT_TILE - 1) / PT_TILE);
        WS(cnt, u32, WS_PT_CNT, (u64)PT_NB_MAX * std::max<u32>(ntiles, 1) + 2); WS(base, u32, WS_PT_BASE, (u64)PT_NB_MAX * std::max<u32>(ntiles, 1) + 2);
        WS(keys, u64, WS_KEYS, n); WS(keep, u32, WS_KEEP, n);
        int cur = 0; int rc = partition_by_window(d, B, 0, (u32)n, 0, N + 2, false, cnt, base, nullptr, &cur, err); if (rc) return rc;
        const EdgeCand* sorted = (const EdgeCand*)B.E[cur];
        hipLaunchKernelGGL(k_conv_group, dim3(grid_for(n, 256)), dim3(256), 0, d->stream, sorted, (u64)n, keys, keep);
        // the kept entries in front of every block of SCAN_BLOCK candidates; k_conv_emit ranks the entries within its block itself
        WS(partial, u64, WS_PARTIAL, scan_partial_words(n));      // (asked for after the sort's scans: they use the same buffer)
        const u64 nb = scan_block_sums(d, keep, n, partial);
        u64 nf = 0; HIPCHK(hipMemcpyAsync(&nf, partial + nb, sizeof(u64), hipMemcpyDeviceToHost, d->stream)); HIPCHK(hipStreamSynchronize(d->stream));
        { WS(fe, FinalEdge, WS_FINAL, std::max<u64>(1, nf)); d->final_edges = fe; }
        hipLaunchKernelGGL(k_conv_emit, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, d->stream, (u64)n, keys, keep, partial, sorted, d->reads, d->S, d->uniL, d->final_edges);
        HIPCHK(hipGetLastError());
        d->n_final = nf;
        HIPCHK(hipStreamSynchronize(d->stream));
    }
    HIPCHK(hipEventRecord(d->ev[1], d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    float ms = 0; hipEventElapsedTime(&ms, d->ev[0], d->ev[1]); d->tm.convert_ms += ms;
    mem_sample(d);
    if (d->diet) for (int id : {WS_PT_K0, WS_PT_K1, WS_PT_CNT, WS_PT_BASE, WS_KEYS, WS_KEEP, WS_PARTIAL}) ws_free(d, id);
    *n_final = d->n_final;
    return 0;
}

// =============================================================================================
// step 4: simplification of the overlap graph in HBM (main.cpp:139-172).  Input: the final edges of step 3 (device resident, .graph3 order).
// =============================================================================================
namespace {
struct S4Mem {                                   // released on every exit path -- into the device's cache of step-4 blocks (Device::s4cache), or freed in diet mode
    Device* d = nullptr;
    std::vector<std::pair<void*, size_t>> ptrs;
    void* take(size_t bytes) {
        for (auto& c : d->s4cache) if (c.second == bytes) { void* p = c.first; c = d->s4cache.back(); d->s4cache.pop_back(); return p; }
        void* p = nullptr;
        if (hipMalloc(&p, bytes) == hipSuccess) return p;
        (void)hipGetLastError();
        s4cache_release(d);                                                           // (blocks of other sizes are in the way)
        return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
    }
    template <class T> T* get(size_t n, std::string& err) { const size_t bytes = std::max<size_t>(n, 1) * sizeof(T); void* p = take(bytes); if (!p) { (void)hipGetLastError(); err = "step 4: device allocation failed"; return nullptr; } ptrs.push_back({p, bytes}); return (T*)p; }
    void give_back(void* p, size_t bytes) { if (d->diet) hipFree(p); else d->s4cache.push_back({p, bytes}); }
    void drop(void* p) { for (auto& q : ptrs) if (q.first == p) { give_back(q.first, q.second); q.first = nullptr; } }
    ~S4Mem() { for (auto& q : ptrs) if (q.first) give_back(q.first, q.second); }
};
}
#define S4GET(var, type, n) type* var = mem.get<type>((n), err); if (!var) return SAGE2OV_ERR_NOMEM;
struct S4Keep { S4Mem mem; S4Graph g; u32 nh = 0; u64 listUsed = 0; float* flow = nullptr;       // flow: one float per half-edge (null: every flow is 0, the state after step 4)
                u64 capH = 0, listCap = 0, flowCap = 0; };                                       // what the half-edge arrays, the list pool and flow[] hold (splice_pairs grows them)
void dev_simplify_release(Device* d) { dev_estflags_release(d); dev_readmap_release(d); dev_contigs_release(d); dev_copycount_release(d); if (d->s4keep) { hipSetDevice(d->ordinal); delete (S4Keep*)d->s4keep; d->s4keep = nullptr; } }

int dev_simplify(Device* d, SimplifiedGraph& out, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    const bool timing = d->opt.get("SAGE2OV_TIMING") != nullptr; auto tp = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) { if (!timing) return; auto t = std::chrono::steady_clock::now(); fprintf(stderr, "[step 4] %-40s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(t - tp).count()); tp = t; };
    dev_simplify_release(d);
    lap("release of the previous result");
    std::unique_ptr<S4Keep> keep(new S4Keep());
    S4Mem& mem = keep->mem; S4Graph& g = keep->g; mem.d = d;
    const u64 N64 = d->N, np = d->n_final;
    if (2 * np + 2 * (N64 + 1) >= (1ull << 32)) { err = "step 4: too many edges"; return SAGE2OV_ERR_LIMIT; }
    const u32 N = (u32)N64, capH = (u32)(2 * np + 2 * (N64 + 1));
    { S4GET(a, u32, capH) g.from = a; } { S4GET(a, u32, capH) g.to = a; } { S4GET(a, u32, capH) g.len = a; } { S4GET(a, u32, capH) g.cnt = a; } { S4GET(a, u32, capH) g.off = a; }
    { S4GET(a, uint8_t, capH) g.type = a; } { S4GET(a, uint8_t, capH) g.alive = a; }
    { S4GET(a, u32, N + 2) g.deg = a; } { S4GET(a, u32, N + 2) g.adjOff = a; } { S4GET(a, u32, capH) g.adj = a; }
    u64 listCap = std::max<u64>(4 * (N64 + 1), 1 << 16), listUsed = 0;
    { S4GET(a, u64, listCap) g.lists = a; }
    S4GET(cursor, u32, N + 2) S4GET(cont, uint8_t, N + 2) S4GET(forced, uint8_t, N + 2) S4GET(role, uint8_t, N + 2) S4GET(h0, u32, N + 2) S4GET(h1, u32, N + 2)
    S4GET(stA, S4State, 2 * (size_t)(N + 1)) S4GET(stB, S4State, 2 * (size_t)(N + 1)) S4GET(stC, S4State, 2 * (size_t)(N + 1))
    S4GET(spFlag, u32, 2 * (size_t)(N + 1) + 2) S4GET(spPos, u32, 2 * (size_t)(N + 1) + 2) S4GET(spList, u32, 2 * (size_t)(N + 1) + 2)
    S4GET(isNew, u32, N + 2) S4GET(newCnt, u32, N + 2) S4GET(rank, u32, N + 2) S4GET(cntScan, u32, N + 2)
    S4GET(chain, S4Chain, capH) S4GET(jobs, S4Job, 4 * (size_t)(N + 1)) S4GET(jobLen, u32, 4 * (size_t)(N + 1)) S4GET(jobStart, u32, 4 * (size_t)(N + 1))
    S4GET(decA, uint8_t, N + 2) S4GET(decB, uint8_t, N + 2) S4GET(othA, u32, N + 2) S4GET(othB, u32, N + 2) S4GET(remA, u32, capH) S4GET(remB, u32, capH)
    S4GET(dctr, u32, 8)
    u32 tabBits = 10; while ((1ull << tabBits) < 2ull * (N64 + 2)) tabBits++;
    const u32 tabMask = (u32)((1ull << tabBits) - 1);
    S4GET(tab, S4Pair, (size_t)1 << tabBits)
    u32 nh = (u32)(2 * np);
    hipStream_t st = d->stream;
    lap("allocations");
    HIPCHK(hipEventRecord(d->ev[0], st));
    if (np) hipLaunchKernelGGL(k_s4_init, dim3(grid_for(np, 256)), dim3(256), 0, st, d->final_edges, (u64)np, g);
    auto rd = [&](u32* v, int n) -> int { return hipMemcpyAsync(v, dctr, n * sizeof(u32), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess ? 0 : -1; };
    bool adjValid = false;                                                         // the lists only change when a sweep changes the graph
    auto adjacency = [&]() -> int {
        if (adjValid) return 0;
        adjValid = true;
        HIPCHK(hipMemsetAsync(g.deg, 0, (N + 2) * sizeof(u32), st)); HIPCHK(hipMemsetAsync(cursor, 0, (N + 2) * sizeof(u32), st));
        if (nh) hipLaunchKernelGGL(k_s4_degree, dim3(grid_for(nh, 256)), dim3(256), 0, st, g, nh);
        u64 tot = 0; int rc = scan_u32(d, g.deg, (u64)N + 1, g.adjOff, &tot, err); if (rc) return rc;
        if (nh) hipLaunchKernelGGL(k_s4_fill, dim3(grid_for(nh, 256)), dim3(256), 0, st, g, nh, cursor);
        hipLaunchKernelGGL(k_s4_sortadj, dim3(grid_for((u64)N + 1, 256)), dim3(256), 0, st, g, N);
        return 0;
    };
    const dim3 gN(grid_for((u64)N + 1, 256)), gS(grid_for(2 * ((u64)N + 1), 256)), b256(256);
    int jumpRounds = 1; while ((1ull << jumpRounds) < 2ull * (N64 + 2)) jumpRounds++;
    // ---- contractCompositePaths (simplification.cpp:14-53)
    auto contract = [&](u64* merged) -> int {
        int rc = adjacency(); if (rc) return rc;
        HIPCHK(hipMemsetAsync(forced, 0, N + 2, st));
        const S4State* fin = nullptr; bool plainJumping = d->opt.get("SAGE2OV_S4_PLAIN_JUMPING") != nullptr;
        for (int round = 0;; round++) {
            if (round > 64) { err = "step 4: chain promotion does not settle"; return SAGE2OV_ERR_INTERNAL; }
            hipLaunchKernelGGL(k_s4_contractible, gN, b256, 0, st, g, N, forced, cont, h0, h1);
            hipLaunchKernelGGL(k_s4_state_init, gS, b256, 0, st, g, N, cont, h0, h1, stA);
            bool ranked = false;
            if (!plainJumping) {                                                     // O(n): splitters, jumping over the splitter states only, hand-out
                hipLaunchKernelGGL(k_s4_split_flags, gS, b256, 0, st, N, cont, spFlag);
                u64 nS = 0; rc = scan_u32(d, spFlag, 2 * ((u64)N + 1), spPos, &nS, err); if (rc) return rc;
                HIPCHK(hipMemsetAsync(dctr, 0, 8 * sizeof(u32), st));
                if (nS) {
                    hipLaunchKernelGGL(k_s4_split_list, gS, b256, 0, st, N, spFlag, spPos, spList);
                    hipLaunchKernelGGL(k_s4_walk_a, dim3(grid_for(nS, 64)), dim3(64), 0, st, spList, (u32)nS, stA, stB, dctr + 2);
                }
                S4State* a = stB; S4State* b = stC;
                for (int r = 0; nS && r < jumpRounds; r++) {
                    HIPCHK(hipMemsetAsync(dctr, 0, sizeof(u32), st));
                    hipLaunchKernelGGL(k_s4_jump_list, dim3(grid_for(nS, 256)), b256, 0, st, spList, (u32)nS, a, b, dctr); std::swap(a, b);
                    u32 open = 0; if (rd(&open, 1)) { err = "step 4: counter read failed"; return SAGE2OV_ERR_DEVICE; }
                    if (!open) break;
                }
                HIPCHK(hipMemsetAsync(b, 0xFF, 2 * (size_t)(N + 1) * sizeof(S4State), st));
                hipLaunchKernelGGL(k_s4_walk_b, dim3(grid_for(2 * ((u64)N + 1), 64)), dim3(64), 0, st, N, cont, stA, a, b, dctr + 2);
                u32 cz[3] = {0, 0, 0}; if (rd(cz, 3)) { err = "step 4: counter read failed"; return SAGE2OV_ERR_DEVICE; }
                if (cz[2]) plainJumping = true; else { fin = b; ranked = true; }
            }
            if (!ranked) {
                S4State* a = stA; S4State* b = stB;
                for (int r = 0; r < jumpRounds; r++) {                               // stops as soon as every state has reached its chain end (cycles never do)
                    HIPCHK(hipMemsetAsync(dctr, 0, sizeof(u32), st));
                    hipLaunchKernelGGL(k_s4_jump, gS, b256, 0, st, N, cont, a, b, dctr); std::swap(a, b);
                    u32 open = 0; if (rd(&open, 1)) { err = "step 4: counter read failed"; return SAGE2OV_ERR_DEVICE; }
                    if (!open) break;
                }
                fin = a;
            }
            HIPCHK(hipMemsetAsync(tab, 0xFF, sizeof(S4Pair) << tabBits, st)); HIPCHK(hipMemsetAsync(dctr, 0, 8 * sizeof(u32), st));
            hipLaunchKernelGGL(k_s4_chain, gN, b256, 0, st, g, N, cont, fin, stA, role, tab, tabMask, dctr);
            hipLaunchKernelGGL(k_s4_parallel, gN, b256, 0, st, g, N, fin, role, tab, tabMask, dctr);
            u32 pz[2] = {0, 0}; if (rd(pz, 2)) { err = "step 4: counter read failed"; return SAGE2OV_ERR_DEVICE; }
            if (pz[1]) { if (plainJumping) { err = "step 4: chain states left unwritten"; return SAGE2OV_ERR_INTERNAL; } plainJumping = true; round--; continue; }   // a cycle without a splitter
            const u32 promoted = pz[0];
            if (!promoted) break;
            hipLaunchKernelGGL(k_s4_promote, gN, b256, 0, st, N, role, forced);
        }
        hipLaunchKernelGGL(k_s4_creator_counts, gN, b256, 0, st, N, role, fin, isNew, newCnt);
        u64 nNew = 0, nList = 0;
        rc = scan_u32(d, isNew, (u64)N + 1, rank, &nNew, err); if (rc) return rc;
        rc = scan_u32(d, newCnt, (u64)N + 1, cntScan, &nList, err); if (rc) return rc;
        if (!nNew) { *merged = 0; return 0; }
        if ((u64)nh + 2 * nNew > capH) { err = "step 4: half-edge pool exhausted"; return SAGE2OV_ERR_INTERNAL; }
        if (listUsed + 2 * nList >= (1ull << 32)) { err = "step 4: read lists exceed 2^32 entries"; return SAGE2OV_ERR_LIMIT; }
        if (listUsed + 2 * nList > listCap) {                                       // grow the list pool (old segments stay where they are)
            const u64 want = std::max<u64>(2 * listCap, listUsed + 2 * nList);
            u64* nl = mem.get<u64>(want, err); if (!nl) return SAGE2OV_ERR_NOMEM;
            if (listUsed) HIPCHK(hipMemcpyAsync(nl, g.lists, listUsed * sizeof(u64), hipMemcpyDeviceToDevice, st));
            HIPCHK(hipStreamSynchronize(st)); mem.drop(g.lists); g.lists = nl; listCap = want;
        }
        HIPCHK(hipMemsetAsync(dctr, 0, 8 * sizeof(u32), st));
        hipLaunchKernelGGL(k_s4_emit, gN, b256, 0, st, g, N, role, fin, h0, h1, rank, cntScan, nh, (u32)listUsed, chain);
        hipLaunchKernelGGL(k_s4_entries, gN, b256, 0, st, g, N, role, fin, h0, h1, chain, jobs, dctr);
        u32 nj = 0; if (rd(&nj, 1)) { err = "step 4: counter read failed"; return SAGE2OV_ERR_DEVICE; }
        if (nj) {
            hipLaunchKernelGGL(k_s4_job_len, dim3(grid_for(nj, 256)), b256, 0, st, jobs, nj, jobLen);
            u64 total = 0; rc = scan_u32(d, jobLen, nj, jobStart, &total, err); if (rc) return rc;
            if (total) hipLaunchKernelGGL(k_s4_copy, dim3(grid_for(total, 256)), b256, 0, st, jobs, nj, jobStart, (u64)total, g.lists);
        }
        nh += (u32)(2 * nNew); listUsed += 2 * nList; adjValid = false;
        *merged = nNew;                                                            // (non-zero: the caller counts the merged nodes)
        return 0;
    };
    // merged nodes of a sweep = nodes with role 1 or 2 (every one of them is one successful mergeEdges)
    auto count_roles = [&](u64* n) -> int {
        HIPCHK(hipMemsetAsync(dctr, 0, 8 * sizeof(u32), st));
        hipLaunchKernelGGL(k_s4_count, gN, b256, 0, st, N, role, dctr);
        u32 v = 0; if (rd(&v, 1)) { err = "step 4: counter read failed"; return SAGE2OV_ERR_DEVICE; }
        *n = v; return 0;
    };
    auto contract_counted = [&](u64* merged) -> int { u64 m = 0; int rc = contract(&m); if (rc) return rc; if (!m) { *merged = 0; return 0; } return count_roles(merged); };
    // ---- removeDeadEnds (simplification.cpp:58-113)
    auto dead_ends = [&](int threshold, u64* removed) -> int {
        int rc = adjacency(); if (rc) return rc;
        HIPCHK(hipMemsetAsync(decA, 0, N + 2, st)); HIPCHK(hipMemsetAsync(decB, 0, N + 2, st));
        uint8_t* in = decA; uint8_t* o = decB;
        for (int it = 0;; it++) {
            if (it > 100000) { err = "step 4: dead-end sweep does not settle"; return SAGE2OV_ERR_INTERNAL; }
            HIPCHK(hipMemsetAsync(dctr, 0, 8 * sizeof(u32), st));
            hipLaunchKernelGGL(k_s4_dead, gN, b256, 0, st, g, N, threshold, in, o, dctr);
            u32 ch = 0; if (rd(&ch, 1)) { err = "step 4: counter read failed"; return SAGE2OV_ERR_DEVICE; }
            std::swap(in, o);
            if (!ch) break;
        }
        HIPCHK(hipMemsetAsync(dctr, 0, 8 * sizeof(u32), st));
        hipLaunchKernelGGL(k_s4_count, gN, b256, 0, st, N, in, dctr);
        if (nh) hipLaunchKernelGGL(k_s4_dead_apply, dim3(grid_for(nh, 256)), b256, 0, st, g, nh, in);
        u32 v = 0; if (rd(&v, 1)) { err = "step 4: counter read failed"; return SAGE2OV_ERR_DEVICE; }
        *removed = v; if (v) hipLaunchKernelGGL(k_s4_filteradj, gN, b256, 0, st, g, N);     // deletions only: the lists are compacted, not rebuilt
        return 0;
    };
    // ---- removeBubbles (simplification.cpp:118-194)
    auto bubbles = [&](long long closeLength, u64* removed) -> int {
        int rc = adjacency(); if (rc) return rc;
        HIPCHK(hipMemsetAsync(decA, 0, N + 2, st)); HIPCHK(hipMemsetAsync(othA, 0, (N + 2) * sizeof(u32), st)); HIPCHK(hipMemsetAsync(remA, 0xFF, (size_t)capH * sizeof(u32), st));
        uint8_t* din = decA; uint8_t* dout = decB; u32* oin = othA; u32* oout = othB; u32* rin = remA; u32* rout = remB;
        for (int it = 0;; it++) {
            if (it > 100000) { err = "step 4: bubble sweep does not settle"; return SAGE2OV_ERR_INTERNAL; }
            HIPCHK(hipMemsetAsync(dctr, 0, 8 * sizeof(u32), st));
            hipLaunchKernelGGL(k_s4_bubble, gN, b256, 0, st, g, N, closeLength, rin, din, oin, dout, oout, dctr);
            u32 ch = 0; if (rd(&ch, 1)) { err = "step 4: counter read failed"; return SAGE2OV_ERR_DEVICE; }
            if (!ch) break;                                                        // rin is the removal map of exactly these decisions
            HIPCHK(hipMemsetAsync(rout, 0xFF, (size_t)capH * sizeof(u32), st));
            hipLaunchKernelGGL(k_s4_bubble_rem, gN, b256, 0, st, g, N, rin, dout, oout, rout);
            std::swap(din, dout); std::swap(oin, oout); std::swap(rin, rout);
        }
        HIPCHK(hipMemsetAsync(dctr, 0, 8 * sizeof(u32), st));
        hipLaunchKernelGGL(k_s4_count, gN, b256, 0, st, N, din, dctr);
        if (nh) hipLaunchKernelGGL(k_s4_bubble_apply, dim3(grid_for(nh, 256)), b256, 0, st, g, nh, rin);
        u32 v = 0; if (rd(&v, 1)) { err = "step 4: counter read failed"; return SAGE2OV_ERR_DEVICE; }
        *removed = v; if (v) hipLaunchKernelGGL(k_s4_filteradj, gN, b256, 0, st, g, N);
        return 0;
    };
    // ---- main.cpp:150-172
    int threshold = 0; long long closeValue = 10; u64 contracted = 0, removed = 0, iters = 0, x = 0;
    int rc;
    if ((rc = contract_counted(&x))) return rc; contracted += x;
    if ((rc = dead_ends(threshold, &x))) return rc; removed += x;
    if ((rc = bubbles(closeValue, &x))) return rc; removed += x;
    if ((rc = contract_counted(&x))) return rc; contracted += x;
    for (;;) {
        u64 a = 0, b = 0, c = 0;
        if ((rc = dead_ends(threshold, &a))) return rc;
        if ((rc = bubbles(closeValue, &b))) return rc;
        if ((rc = contract_counted(&c))) return rc;
        removed += a + b; contracted += c; iters++;
        if (a + b + c == 0) break;
        if (closeValue < 50) closeValue += 10;
        if (threshold < 3) threshold++;
    }
    HIPCHK(hipEventRecord(d->ev[1], st)); HIPCHK(hipStreamSynchronize(st));
    float ms = 0; hipEventElapsedTime(&ms, d->ev[0], d->ev[1]);
    lap("sweeps (host view)");
    S4GET(dstat, u64, 2)
    HIPCHK(hipMemsetAsync(dstat, 0, 2 * sizeof(u64), st));
    if (nh) hipLaunchKernelGGL(k_s4_stats, dim3(grid_for(nh / 2 + 1, 256)), b256, 0, st, g, nh, dstat);
    u64 hs[2] = {0, 0}; HIPCHK(hipMemcpyAsync(hs, dstat, sizeof hs, hipMemcpyDeviceToHost, st)); HIPCHK(hipStreamSynchronize(st));
    out = SimplifiedGraph();
    out.n_half_edges = nh; out.contracted = contracted; out.removed = removed; out.iterations = iters; out.device_ms = ms; out.N = N64; out.pairs_alive = hs[0]; out.reads_on_edges = hs[1];
    // the graph stays in HBM (downloaded only when it is written); the work buffers go
    for (void* p : {(void*)stA, (void*)stB, (void*)stC, (void*)spFlag, (void*)spPos, (void*)spList, (void*)tab, (void*)jobs, (void*)jobLen, (void*)jobStart, (void*)remA, (void*)remB, (void*)chain, (void*)g.adj, (void*)cursor, (void*)h0, (void*)h1,
                    (void*)isNew, (void*)newCnt, (void*)rank, (void*)cntScan, (void*)othA, (void*)othB}) mem.drop(p);
    g.adj = nullptr;
    lap("statistics + release of the work buffers");
    keep->nh = nh; keep->listUsed = listUsed; keep->capH = capH; keep->listCap = listCap;
    d->s4keep = keep.release();
    return 0;
}
int dev_simplify_download(Device* d, SimplifiedGraph& out, std::string& err, bool withLists) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (!d->s4keep) { err = "step 4: no simplified graph on the device"; return SAGE2OV_ERR_ARG; }
    if (out.downloaded || (out.fields && !withLists)) return 0;
    const S4Keep& k = *(S4Keep*)d->s4keep; const S4Graph& g = k.g; const u32 nh = k.nh;
    if (!out.fields) { out.from.resize(nh); out.to.resize(nh); out.len.resize(nh); out.cnt.resize(nh); out.off.resize(nh); out.type.resize(nh); out.alive.resize(nh); }
    if (nh && !out.fields) {
        HIPCHK(hipMemcpy(out.from.data(), g.from, nh * sizeof(u32), hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(out.to.data(), g.to, nh * sizeof(u32), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out.len.data(), g.len, nh * sizeof(u32), hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(out.cnt.data(), g.cnt, nh * sizeof(u32), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out.off.data(), g.off, nh * sizeof(u32), hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(out.type.data(), g.type, nh, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out.alive.data(), g.alive, nh, hipMemcpyDeviceToHost));
    }
    out.fields = true;
    if (!withLists) return 0;
    out.lists.resize(k.listUsed);
    if (k.listUsed) HIPCHK(hipMemcpy(out.lists.data(), g.lists, k.listUsed * sizeof(u64), hipMemcpyDeviceToHost));
    out.downloaded = true;
    return 0;
}

// a graph that was parsed from a file (sage2ov_graph_load_composite) takes the place of step 4's result: the half-edge arrays and the list pool, nothing else
int dev_simplify_upload(Device* d, const SimplifiedGraph& in, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    dev_simplify_release(d);
    const u64 nh64 = in.n_half_edges, nl = in.lists.size();
    if (nh64 >= (1ull << 32) - RS_TILE || nl >= (1ull << 32) - RS_TILE) { err = "graph load: too many edges or list entries"; return SAGE2OV_ERR_LIMIT; }
    std::unique_ptr<S4Keep> keep(new S4Keep());
    S4Mem& mem = keep->mem; S4Graph& g = keep->g; mem.d = d; g = S4Graph();
    const u32 nh = (u32)nh64;
    { S4GET(a, u32, nh) g.from = a; } { S4GET(a, u32, nh) g.to = a; } { S4GET(a, u32, nh) g.len = a; } { S4GET(a, u32, nh) g.cnt = a; } { S4GET(a, u32, nh) g.off = a; }
    { S4GET(a, uint8_t, nh) g.type = a; } { S4GET(a, uint8_t, nh) g.alive = a; } { S4GET(a, u64, nl) g.lists = a; }
    if (nh) {
        HIPCHK(hipMemcpy(g.from, in.from.data(), nh * sizeof(u32), hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(g.to, in.to.data(), nh * sizeof(u32), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(g.len, in.len.data(), nh * sizeof(u32), hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(g.cnt, in.cnt.data(), nh * sizeof(u32), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(g.off, in.off.data(), nh * sizeof(u32), hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(g.type, in.type.data(), nh, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(g.alive, in.alive.data(), nh, hipMemcpyHostToDevice));
    }
    if (nl) HIPCHK(hipMemcpy(g.lists, in.lists.data(), nl * sizeof(u64), hipMemcpyHostToDevice));
    keep->nh = nh; keep->listUsed = nl; keep->capH = std::max<u64>(nh, 1); keep->listCap = std::max<u64>(nl, 1);
    d->s4keep = keep.release();
    return in.flow.empty() ? 0 : dev_flow_set(d, in.flow.data(), in.flow.size(), err);
}
// the flows of the resident graph, one per half-edge (null: all 0 again).  The supports go: they were made from the flows
int dev_flow_set(Device* d, const float* flow, uint64_t n, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (!d->s4keep) { err = "flows: no step-4 graph on the device"; return SAGE2OV_ERR_ARG; }
    S4Keep& K = *(S4Keep*)d->s4keep; S4Mem& mem = K.mem;
    dev_support_release(d); dev_paths_release(d);
    if (!flow) { if (K.flow) { mem.drop(K.flow); K.flow = nullptr; K.flowCap = 0; } return 0; }
    if (n != K.nh) { err = "flows: one value per half-edge"; return SAGE2OV_ERR_INTERNAL; }
    if (!K.flow) { S4GET(a, float, K.nh) K.flow = a; K.flowCap = std::max<u64>(K.nh, 1); }
    if (n) HIPCHK(hipMemcpy(K.flow, flow, n * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// room for `created` new pairs and `total` new list entries.  The pools grow as step 4's list pool does: a new block, the old content copied
static int s4_pools_grow(Device* d, S4Keep& K, u64 created, u64 total, std::string& err) {
    S4Mem& mem = K.mem; S4Graph& g = K.g; hipStream_t sm = d->stream;
    const u64 needH = (u64)K.nh + 2 * created;
    if (needH > K.capH) {
        const u64 want = std::min<u64>(std::max<u64>(needH, K.capH + K.capH / 2), (1ull << 32) - RS_TILE);
        auto grow = [&](auto*& arr) -> int {
            using T = std::remove_reference_t<decltype(*arr)>;
            T* nw = mem.get<T>(want, err); if (!nw) return SAGE2OV_ERR_NOMEM;
            if (K.nh && hipMemcpyAsync(nw, arr, (size_t)K.nh * sizeof(T), hipMemcpyDeviceToDevice, sm) != hipSuccess) { err = "graph pools: device copy failed"; return SAGE2OV_ERR_DEVICE; }
            if (hipStreamSynchronize(sm) != hipSuccess) { err = "graph pools: device copy failed"; return SAGE2OV_ERR_DEVICE; }
            mem.drop(arr); arr = nw; return 0;
        };
        int rc;
        if ((rc = grow(g.from)) || (rc = grow(g.to)) || (rc = grow(g.len)) || (rc = grow(g.cnt)) || (rc = grow(g.off)) || (rc = grow(g.type)) || (rc = grow(g.alive))) return rc;
        K.capH = want;
    }
    if (K.flow && needH > K.flowCap) {
        float* nw = mem.get<float>(K.capH, err); if (!nw) return SAGE2OV_ERR_NOMEM;
        if (K.nh) HIPCHK(hipMemcpyAsync(nw, K.flow, (size_t)K.nh * sizeof(float), hipMemcpyDeviceToDevice, sm));
        HIPCHK(hipStreamSynchronize(sm)); mem.drop(K.flow); K.flow = nw; K.flowCap = K.capH;
    }
    if (K.listUsed + total > K.listCap) {
        const u64 want = std::max<u64>(K.listUsed + total, K.listCap + K.listCap / 2);
        u64* nl = mem.get<u64>(want, err); if (!nl) return SAGE2OV_ERR_NOMEM;
        if (K.listUsed) HIPCHK(hipMemcpyAsync(nl, g.lists, K.listUsed * sizeof(u64), hipMemcpyDeviceToDevice, sm));
        HIPCHK(hipStreamSynchronize(sm)); mem.drop(g.lists); g.lists = nl; K.listCap = want;
    }
    return 0;
}
// ---- a batch of splices (kernels_splice.inc): the sequence that merges and joins share.  a[i], b[i]: the operand half-edges of splice i,
// below K.nh, no pair named twice -- the caller has checked it.  planStage(da, db, plan, lens, partial, rank, created) runs its plan kernel on the uploaded
// operands, between lap.start and the scan of lens (its time is plan_ms, less what it laps apart itself), and sets rank and created where it can refuse; left
// alone, splice i makes pair K.nh / 2 + i.  makesFlow: flows that were all 0 (no array) become an array.  out[i]: the plan of splice i.  Everything made from the
// graph goes (as in dev_simplify_release), the graph itself stays.
template <class PlanStage>
static int splice_pairs(Device* d, DevTmp& B, StreamLap& lap, const std::string& who, const u32* a, const u32* b, u64 n, u64 maxN, bool makesFlow, SplicePlan* out,
                        SpliceStats* st, std::string& err, PlanStage&& planStage) {
    S4Keep& K = *(S4Keep*)d->s4keep; S4Mem& mem = K.mem; S4Graph& g = K.g; hipStream_t sm = d->stream;
    if (n >= maxN || (u64)K.nh + 2 * n >= (1ull << 32) - RS_TILE) { err = who + ": more than 2^32 half-edges"; return SAGE2OV_ERR_LIMIT; }
    const u32 m = (u32)n;
    u32* da = B.get<u32>(n); u32* db = B.get<u32>(n); SplicePlan* plan = B.get<SplicePlan>(n); u32* lens = B.get<u32>(2 * n); u32* lo = B.get<u32>(2 * n);
    u64* partial = B.get<u64>(scan_partial_words(2 * n));
    if (!da || !db || !plan || !lens || !lo || !partial) { err = who + ": out of device memory"; return SAGE2OV_ERR_NOMEM; }
    HIPCHK(lap.start());
    HIPCHK(hipMemcpyAsync(da, a, n * sizeof(u32), hipMemcpyHostToDevice, sm)); HIPCHK(hipMemcpyAsync(db, b, n * sizeof(u32), hipMemcpyHostToDevice, sm));
    u32* rank = nullptr; u64 total = 0, created = n;
    { const int rc = planStage(da, db, plan, lens, partial, rank, created); if (rc) return rc; }
    HIPCHK(hipGetLastError());
    { const int rc = scan_u32(d, lens, 2 * n, lo, partial, &total, err); if (rc) return rc; }
    HIPCHK(lap.stop(st->plan_ms));
    if (K.listUsed + total >= (1ull << 32) - RS_TILE) { err = who + ": read lists exceed 2^32 entries"; return SAGE2OV_ERR_LIMIT; }
    if (created) {
        if (makesFlow && !K.flow) {                                                    // (every flow was 0: the plan read them as 0; the new edges have 1.0)
            float* f = mem.get<float>(std::max<u64>(K.capH, 1), err); if (!f) return SAGE2OV_ERR_NOMEM;
            HIPCHK(hipMemsetAsync(f, 0, std::max<u64>(K.capH, 1) * sizeof(float), sm)); K.flow = f; K.flowCap = std::max<u64>(K.capH, 1);
        }
        { const int rc = s4_pools_grow(d, K, created, total, err); if (rc) return rc; }
        dev_readmap_release(d); dev_contigs_release(d); dev_copycount_release(d);
        HIPCHK(lap.start());
        hipLaunchKernelGGL(k_sp_lists, dim3(grid_for(total, 256)), dim3(256), 0, sm, g, plan, lo, 2 * m, (u64)total, (u32)K.listUsed);
        HIPCHK(hipGetLastError());
        HIPCHK(lap.stop(st->lists_ms));
        HIPCHK(lap.start());
        hipLaunchKernelGGL(k_sp_commit, dim3(grid_for(n, 256)), dim3(256), 0, sm, g, K.flow, plan, lo, rank, m, K.nh, (u32)K.listUsed);
        HIPCHK(hipGetLastError());
        HIPCHK(lap.stop(st->commit_ms));
    }
    HIPCHK(hipMemcpy(out, plan, n * sizeof(SplicePlan), hipMemcpyDeviceToHost));
    for (u64 i = 0; i < n; i++) {
        const SplicePlan& p = out[i];
        st->pairs_deleted += (u64)p.del1 + p.del2;
        for (int dI = 0; dI < 2; dI++) { st->overlaps += p.how[dI] == SC_OVERLAP; st->concatenated += p.how[dI] == SC_CONCAT; st->gapped += p.how[dI] == SC_GAPPED; }
    }
    K.nh += (u32)(2 * created); K.listUsed += total;
    st->made = created; st->entries_copied = total; st->half_edges = K.nh; st->list_entries = K.listUsed;
    return 0;
}
// mergeEdgesAndUpdate for a batch: to[a] == from[b], and a simple operand's length within 11 bits -- the caller has checked it.  A merge can be refused (made 0)
int dev_merge_pairs(Device* d, const u32* a, const u32* b, uint64_t n, int typeOfMerge, SplicePlan* out, SpliceStats* st, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (!d->s4keep) { err = "merge: no step-4 graph on the device"; return SAGE2OV_ERR_ARG; }
    *st = SpliceStats();
    if (!n) return 0;
    DevTmp B; StreamLap lap(d->stream); HIPCHK(lap.create());
    return splice_pairs(d, B, lap, "merge", a, b, n, 1ull << 31, false, out, st, err, [&](const u32* da, const u32* db, SplicePlan* plan, u32* lens, u64* partial, u32*& rank, u64& created) -> int {
        const S4Keep& K = *(const S4Keep*)d->s4keep;
        u32* isNew = B.get<u32>(n); rank = B.get<u32>(n);
        if (!isNew || !rank) { err = "merge: out of device memory"; return SAGE2OV_ERR_NOMEM; }
        hipLaunchKernelGGL(k_mg_plan, dim3(grid_for(n, 256)), dim3(256), 0, d->stream, K.g, (const float*)K.flow, da, db, (u32)n, typeOfMerge, plan, lens, isNew);
        return scan_u32(d, isNew, n, rank, partial, &created, err);
    });
}
// mergeDisconnectedEdges for a batch: gap[i] the gap of join i; both operands alive, with a list, lengths within 32 bits -- the caller has checked it.  Nothing is
// refused.  overlap (may be null): 2 n values.  Flows that were all 0 (no array) become an array: the new edges have flow 1.0
static bool contig_reads(Device* d, CtReads& R);
int dev_join_pairs(Device* d, const u32* a, const u32* b, const int32_t* gap, uint64_t n, SplicePlan* out, int32_t* overlap, SpliceStats* st, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (!d->s4keep) { err = "join: no step-4 graph on the device"; return SAGE2OV_ERR_ARG; }
    CtReads Rd; if (!contig_reads(d, Rd)) { err = "join: no read store on the device"; return SAGE2OV_ERR_ARG; }
    *st = SpliceStats();
    if (!n) return 0;
    DevTmp B; StreamLap lap(d->stream); HIPCHK(lap.create());
    int* ov = nullptr;
    const int rc = splice_pairs(d, B, lap, "join", a, b, n, 1ull << 30, true, out, st, err, [&](const u32* da, const u32* db, SplicePlan* plan, u32* lens, u64*, u32*&, u64&) -> int {
        const S4Keep& K = *(const S4Keep*)d->s4keep; hipStream_t sm = d->stream; const u32 m = (u32)n;
        int* dgap = B.get<int>(n); ov = B.get<int>(2 * n);
        if (!dgap || !ov) { err = "join: out of device memory"; return SAGE2OV_ERR_NOMEM; }
        HIPCHK(hipMemcpyAsync(dgap, gap, n * sizeof(int), hipMemcpyHostToDevice, sm));
        hipLaunchKernelGGL(k_sc_overlap, dim3(2 * m), dim3(64), 0, sm, K.g, Rd, da, db, 2 * m, ov);
        HIPCHK(hipGetLastError());
        HIPCHK(lap.stop(st->overlap_ms));
        HIPCHK(lap.start());
        hipLaunchKernelGGL(k_sc_plan, dim3(grid_for(n, 256)), dim3(256), 0, sm, K.g, Rd, (const float*)K.flow, da, db, dgap, ov, m, plan, lens);
        return 0;
    });
    if (rc) return rc;
    if (overlap) HIPCHK(hipMemcpy(overlap, ov, 2 * n * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

// =============================================================================================
// the read-to-edge table, the mate flags, the distances and the rounds (kernels_readmap.inc; MatePair::meanSdEstimation, matePair.cpp:244-569)
// =============================================================================================
struct ReadMapLib { unsigned char* flag = nullptr; u32 *dist = nullptr, *dEntry = nullptr, *dPair = nullptr; u64 nflag = 0, nd = 0; bool joined = false; };
static void readmap_drop_join(ReadMapLib& L) { hipFree(L.flag); hipFree(L.dist); hipFree(L.dEntry); hipFree(L.dPair); L = ReadMapLib(); }
struct ReadMap {
    u32 *eRead = nullptr, *ePair = nullptr, *eNf = nullptr, *eNr = nullptr, *eLoc = nullptr, *readOff = nullptr; int* locs = nullptr; u64 E = 0, R = 0; ReadMapLib lib[128];
    ~ReadMap() { for (auto& L : lib) readmap_drop_join(L); hipFree(eRead); hipFree(ePair); hipFree(eNf); hipFree(eNr); hipFree(eLoc); hipFree(readOff); hipFree(locs); }
};
void dev_readmap_drop_joins(Device* d) { dev_support_release(d); dev_paths_release(d); dev_links_release(d); if (!d->readmap) return; hipSetDevice(d->ordinal); for (auto& L : ((ReadMap*)d->readmap)->lib) readmap_drop_join(L); }
void dev_readmap_release(Device* d) { dev_support_release(d); dev_paths_release(d); dev_links_release(d); if (d->readmap) { hipSetDevice(d->ordinal); delete (ReadMap*)d->readmap; d->readmap = nullptr; } }
static int readmap_nomem(std::string& err) { err = "read-to-edge table: out of device memory"; return SAGE2OV_ERR_NOMEM; }
template <class T> static T* readmap_alloc(u64 n) { return (T*)DevTmp::alloc(std::max<u64>(n, 1) * sizeof(T)); }
// the 8-bit digits of a record key (read:30 | pair:31 | side:1) that can be non-zero: side and pair end at bit 1 + bits(pairs), the read at 32 + bits(N)
static int readmap_passes(u64 N, u64 pairs, int* shifts) {
    int b = 0; while ((N >> b) != 0) b++;
    int bp = 0; while ((pairs >> bp) != 0) bp++;
    int np = 0;
    for (int p = 0; p < 8; p++) { const int lo = 8 * p; if (lo < 1 + bp || (lo >= 32 && lo < 32 + b)) shifts[np++] = lo; }
    return np;
}
// ---- the stages that the sort-and-reduce sweeps over the resident graph share (the read-to-edge table, the supports, the links)
// sums[i] = the distPrevious of the pool entries in front of i, dead lists included (k_rm_dprev, one scan); nobody keeps them: every sweep makes them again
static int pool_running_sums(Device* d, DevTmp& B, const u64* lists, u64 nl, u64* partial, u32*& sums, int (*nomem)(std::string&), std::string& err) {
    u32* dprev = B.get<u32>(nl); sums = B.get<u32>(nl);
    if (!dprev || !sums) return nomem(err);
    if (nl) hipLaunchKernelGGL(k_rm_dprev, dim3(grid_for_capped(nl, 256)), dim3(256), 0, d->stream, lists, nl, dprev);
    { const int rc = scan_u32(d, dprev, nl, sums, partial, nullptr, err); if (rc) return rc; }
    B.release(dprev);
    return 0;
}
// uniq[r] = pair + 1 when read r has exactly one read-to-edge entry and no alive half-edge leaves node r, else 0 (k_ms_nodes, k_ms_unique); nodeFlag: N + 2 bytes of scratch
static int unique_reads(Device* d, const S4Graph& g, u32 nh, const MsTable& T, uint8_t* nodeFlag, u32* uniq, std::string& err) {
    HIPCHK(hipMemsetAsync(nodeFlag, 0, (u64)T.N + 2, d->stream));
    hipLaunchKernelGGL(k_ms_nodes, dim3(grid_for(nh, 256)), dim3(256), 0, d->stream, g, nh, nodeFlag);
    hipLaunchKernelGGL(k_ms_unique, dim3(grid_for((u64)T.N + 1, 256)), dim3(256), 0, d->stream, T, nodeFlag, uniq);
    return 0;
}
// the 8-bit digits of a (half:32 | half:32) key that can be non-zero: those below the number of half-edges, in both words
static int half_pair_passes(u32 nh, int* shifts) {
    int b = 0; while (((u64)nh >> b) != 0) b++;
    int np = 0;
    for (int p = 0; p < 8; p++) { const int lo = 8 * p; if ((lo & 31) < b) shifts[np++] = lo; }
    return np;
}
int dev_readmap_build(Device* d, ReadMapStats* st, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (!d->s4keep) { err = "read-to-edge table: no step-4 graph on the device"; return SAGE2OV_ERR_ARG; }
    if (d->N >= (1ull << 30)) { err = "read-to-edge table: read ids beyond 2^30 - 1"; return SAGE2OV_ERR_LIMIT; }
    dev_readmap_release(d);
    const S4Keep& K = *(S4Keep*)d->s4keep; const S4Graph& g = K.g; const u32 nh = K.nh; const u64 nl = K.listUsed;
    if (nl >= (1ull << 32) - RS_TILE) { err = "read-to-edge table: more than 2^32 list entries"; return SAGE2OV_ERR_LIMIT; }
    std::unique_ptr<ReadMap> M(new ReadMap());
    DevTmp B; StreamLap lap(d->stream); HIPCHK(lap.create());
    M->readOff = readmap_alloc<u32>(d->N + 2); if (!M->readOff) return readmap_nomem(err);
    // ---- locations: one scan of distPrevious over the whole pool
    HIPCHK(lap.start());
    u32* scan = nullptr; u64* partial = B.get<u64>(scan_partial_words(std::max<u64>(nl, nh)));
    u32* cnt = B.get<u32>(nh); u32* recOff = B.get<u32>(nh);
    if (!partial || !cnt || !recOff) return readmap_nomem(err);
    { const int rc = pool_running_sums(d, B, g.lists, nl, partial, scan, readmap_nomem, err); if (rc) return rc; }
    HIPCHK(lap.stop(st->scan_ms));
    // ---- records
    HIPCHK(lap.start());
    if (nh) hipLaunchKernelGGL(k_rm_count, dim3(grid_for(nh, 256)), dim3(256), 0, d->stream, g, nh, cnt);
    u64 R = 0; { const int rc = scan_u32(d, cnt, nh, recOff, partial, &R, err); if (rc) return rc; }
    if (R >= (1ull << 32) - RS_TILE) { err = "read-to-edge table: more than 2^32 records"; return SAGE2OV_ERR_LIMIT; }
    st->records = st->locations = R;
    if (!R) {                                                                        // a graph of simple edges maps nothing
        HIPCHK(hipMemsetAsync(M->readOff, 0, (d->N + 2) * sizeof(u32), d->stream)); HIPCHK(hipStreamSynchronize(d->stream));
        d->readmap = M.release(); return 0;
    }
    u64* key = B.get<u64>(R); u32* loc = B.get<u32>(R);
    if (!key || !loc) return readmap_nomem(err);
    hipLaunchKernelGGL(k_rm_records, dim3(grid_for(R, 256)), dim3(256), 0, d->stream, g, nh, recOff, (u32)R, scan, nl, key, loc);
    HIPCHK(hipGetLastError());
    HIPCHK(lap.stop(st->records_ms));
    B.release(scan); B.release(cnt); B.release(recOff); B.release(partial);
    // ---- sort by (read, pair, side)
    HIPCHK(lap.start());
    int shifts[8]; const int np = readmap_passes(d->N, nh / 2, shifts);
    u64* ks = nullptr; u32* vs = nullptr; MateStats ms;
    { const int rc = mate_sort(d, B, key, (u32)R, shifts, np, &ks, &vs, &ms, err); if (rc) return rc; }
    st->passes = ms.passes;
    HIPCHK(lap.stop(st->sort_ms));
    // ---- reduce: heads over (read, pair), entries, locations in sorted order, per-read offsets
    HIPCHK(lap.start());
    u32* flag = B.get<u32>(R); u32* pos = B.get<u32>(R); u64* partial2 = B.get<u64>(scan_partial_words(R));
    if (!flag || !pos || !partial2) return readmap_nomem(err);
    hipLaunchKernelGGL(k_rm_heads, dim3(grid_for(R, 256)), dim3(256), 0, d->stream, ks, (u32)R, flag);
    u64 E = 0; { const int rc = scan_u32(d, flag, R, pos, partial2, &E, err); if (rc) return rc; }
    u32* hp = B.get<u32>(E + 1); if (!hp) return readmap_nomem(err);
    { const int rc = head_positions(d, flag, pos, R, hp, E, err); if (rc) return rc; }
    M->eRead = readmap_alloc<u32>(E); M->ePair = readmap_alloc<u32>(E); M->eNf = readmap_alloc<u32>(E); M->eNr = readmap_alloc<u32>(E); M->eLoc = readmap_alloc<u32>(E); M->locs = readmap_alloc<int>(R);
    if (!M->eRead || !M->ePair || !M->eNf || !M->eNr || !M->eLoc || !M->locs) return readmap_nomem(err);
    hipLaunchKernelGGL(k_rm_entries, dim3(grid_for(E, 256)), dim3(256), 0, d->stream, ks, hp, (u32)E, M->eRead, M->ePair, M->eNf, M->eNr, M->eLoc);
    hipLaunchKernelGGL(k_rm_gather, dim3(grid_for(R, 256)), dim3(256), 0, d->stream, vs, loc, (u32)R, M->locs);
    hipLaunchKernelGGL(k_rm_offsets, dim3(grid_for(d->N + 2, 256)), dim3(256), 0, d->stream, M->eRead, (u32)E, (u32)d->N, M->readOff);
    HIPCHK(hipGetLastError());
    HIPCHK(lap.stop(st->reduce_ms));
    M->E = E; M->R = R; st->entries = E;
    d->readmap = M.release();
    return 0;
}
// flags of the library's mate entries, and its distances (left in HBM for the rounds)
int dev_readmap_join(Device* d, int library, ReadMapStats* st, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (!d->readmap) { err = "read-to-edge table: not built"; return SAGE2OV_ERR_INTERNAL; }
    ReadMap* M = (ReadMap*)d->readmap; ReadMapLib& J = M->lib[library];
    if (J.joined) return 0;
    readmap_drop_join(J);
    static const MateLib none; const MateLib& L = d->mates ? d->mates->lib[library] : none;
    if (!L.n) { J.joined = true; return 0; }
    if (L.n >= (1ull << 32) / RM_GROUP) { err = "read-to-edge table: too many mate entries in one library"; return SAGE2OV_ERR_LIMIT; }
    const u32 n = (u32)L.n;
    DevTmp B; StreamLap lap(d->stream); HIPCHK(lap.create());
    HIPCHK(lap.start());
    u32* dcount = B.get<u32>(n); u32* dpos = B.get<u32>(n); u64* partial = B.get<u64>(scan_partial_words(n));
    J.flag = readmap_alloc<unsigned char>(n);
    if (!dcount || !dpos || !partial || !J.flag) { readmap_drop_join(J); return readmap_nomem(err); }
    const RmTable T = {M->readOff, M->ePair, M->eNf, M->eLoc, M->locs, (u32)d->N};
    const dim3 grid(grid_for((u64)n * RM_GROUP, 256)), block(256);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rm_join<false>), grid, block, 0, d->stream, L.key, n, T, J.flag, dcount, (const u32*)nullptr, (u32*)nullptr, (u32*)nullptr, (u32*)nullptr);
    u64 nd = 0; { const int rc = scan_u32(d, dcount, n, dpos, partial, &nd, err); if (rc) { readmap_drop_join(J); return rc; } }
    if (nd) {
        J.dist = readmap_alloc<u32>(nd); J.dEntry = readmap_alloc<u32>(nd); J.dPair = readmap_alloc<u32>(nd);
        if (!J.dist || !J.dEntry || !J.dPair) { readmap_drop_join(J); return readmap_nomem(err); }
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_rm_join<true>), grid, block, 0, d->stream, L.key, n, T, (unsigned char*)nullptr, (u32*)nullptr, (const u32*)dpos, J.dist, J.dEntry, J.dPair);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(lap.stop(st->join_ms));
    J.nflag = n; J.nd = nd; J.joined = true;
    return 0;
}
// one round of computeMeanSD over the library's distances: out = {count, sum, sq low, sq high} of the d < thr
int dev_readmap_round(Device* d, int library, long long mu, uint64_t thr, uint64_t out[4], ReadMapStats* st, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!d->readmap) { err = "read-to-edge table: not built"; return SAGE2OV_ERR_INTERNAL; }
    const ReadMapLib& J = ((ReadMap*)d->readmap)->lib[library];
    if (!J.nd) return 0;
    const unsigned blocks = (unsigned)std::min<u64>(grid_for(J.nd, 256), 1024);
    DevTmp B; u64* partial = B.get<u64>(4ull * blocks); if (!partial) return readmap_nomem(err);
    StreamLap lap(d->stream); HIPCHK(lap.create()); HIPCHK(lap.start());
    hipLaunchKernelGGL(k_rm_round, dim3(blocks), dim3(256), 0, d->stream, J.dist, J.nd, (u64)thr, mu, partial);
    HIPCHK(hipGetLastError());
    std::vector<u64> h(4ull * blocks);
    HIPCHK(hipMemcpyAsync(h.data(), partial, h.size() * sizeof(u64), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(lap.stop(st->round_ms));
    unsigned __int128 sq = 0;
    for (unsigned b = 0; b < blocks; b++) { out[0] += h[4 * b]; out[1] += h[4 * b + 1]; sq += ((unsigned __int128)h[4 * b + 3] << 64) | h[4 * b + 2]; }
    out[2] = (u64)sq; out[3] = (u64)(sq >> 64);
    st->rounds++;
    return 0;
}
void dev_readmap_counts(Device* d, uint64_t* entries, uint64_t* locations) { const ReadMap* M = (const ReadMap*)d->readmap; *entries = M ? M->E : 0; *locations = M ? M->R : 0; }
// the table as it lies on the device: entries arrays of E values, locations of R, offsets of N + 2
int dev_readmap_export(Device* d, uint32_t* read, uint32_t* pair, uint32_t* nf, uint32_t* nr, uint32_t* loc, int32_t* locs, uint32_t* offsets, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    const ReadMap* M = (const ReadMap*)d->readmap; if (!M) { err = "read-to-edge table: not built"; return SAGE2OV_ERR_INTERNAL; }
    if (M->E) {
        HIPCHK(hipMemcpy(read, M->eRead, M->E * sizeof(u32), hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(pair, M->ePair, M->E * sizeof(u32), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(nf, M->eNf, M->E * sizeof(u32), hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(nr, M->eNr, M->E * sizeof(u32), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(loc, M->eLoc, M->E * sizeof(u32), hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(locs, M->locs, M->R * sizeof(int), hipMemcpyDeviceToHost));
    }
    HIPCHK(hipMemcpy(offsets, M->readOff, (d->N + 2) * sizeof(u32), hipMemcpyDeviceToHost));
    return 0;
}
uint64_t dev_readmap_flag_count(Device* d, int library) { const ReadMap* M = (const ReadMap*)d->readmap; return M ? M->lib[library].nflag : 0; }
uint64_t dev_readmap_distance_count(Device* d, int library) { const ReadMap* M = (const ReadMap*)d->readmap; return M ? M->lib[library].nd : 0; }
int dev_readmap_flags(Device* d, int library, uint8_t* out, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    const ReadMap* M = (const ReadMap*)d->readmap; if (!M) { err = "read-to-edge table: not built"; return SAGE2OV_ERR_INTERNAL; }
    const ReadMapLib& J = M->lib[library];
    if (J.nflag) HIPCHK(hipMemcpy(out, J.flag, J.nflag, hipMemcpyDeviceToHost));
    return 0;
}
int dev_readmap_distances(Device* d, int library, uint32_t* dist, uint32_t* entry, uint32_t* pair, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    const ReadMap* M = (const ReadMap*)d->readmap; if (!M) { err = "read-to-edge table: not built"; return SAGE2OV_ERR_INTERNAL; }
    const ReadMapLib& J = M->lib[library];
    if (J.nd) {
        HIPCHK(hipMemcpy(dist, J.dist, J.nd * sizeof(u32), hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(entry, J.dEntry, J.nd * sizeof(u32), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(pair, J.dPair, J.nd * sizeof(u32), hipMemcpyDeviceToHost));
    }
    return 0;
}

// =============================================================================================
// the mate-pair supports of (in-half, out-half) pairs at a node (kernels_support.inc; the sweep of ContigExtender::findMatepairSupports, mergeContigs.cpp:959-1110)
// =============================================================================================
struct Support { u64* key = nullptr; u32* sup = nullptr; u64 E = 0; ~Support() { hipFree(key); hipFree(sup); } };
void dev_support_release(Device* d) { if (d->support) { hipSetDevice(d->ordinal); delete (Support*)d->support; d->support = nullptr; } }
uint64_t dev_support_count(Device* d) { const Support* S = (const Support*)d->support; return S ? S->E : 0; }
static int support_nomem(std::string& err) { err = "mate-pair supports: out of device memory"; return SAGE2OV_ERR_NOMEM; }
int dev_support_build(Device* d, const SupportParams& P, SupportStats* st, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (!d->s4keep) { err = "mate-pair supports: no step-4 graph on the device"; return SAGE2OV_ERR_ARG; }
    if (!d->readmap) { err = "mate-pair supports: the read-to-edge table is not built"; return SAGE2OV_ERR_INTERNAL; }
    dev_support_release(d);
    const S4Keep& K = *(S4Keep*)d->s4keep; const S4Graph& g = K.g; const u32 nh = K.nh; const u64 nl = K.listUsed; const ReadMap* M = (const ReadMap*)d->readmap;
    std::unique_ptr<Support> S(new Support());
    *st = SupportStats();
    if (!K.flow || !nh || !nl) { d->support = S.release(); return 0; }                 // every flow is 0 (the graph as step 4 leaves it), or no list: no candidate
    const u32 N = (u32)d->N; hipStream_t sm = d->stream;
    DevTmp B; StreamLap lap(sm); HIPCHK(lap.create());
    // ---- unique reads, the role of every half-edge, candidates per node
    HIPCHK(lap.start());
    uint8_t* nodeFlag = B.get<uint8_t>((u64)N + 2); u32* uniq = B.get<u32>((u64)N + 2); uint8_t* role = B.get<uint8_t>(nh); u32* inCnt = B.get<u32>(nh); u32* inOff = B.get<u32>(nh);
    u32* nIn = B.get<u32>((u64)N + 2); u32* nOut = B.get<u32>((u64)N + 2); u32* prod = B.get<u32>((u64)N + 2); u32* prodScan = B.get<u32>((u64)N + 2);
    unsigned long long* ctr = B.get<unsigned long long>(4); u64* partial = B.get<u64>(scan_partial_words(std::max<u64>(std::max<u64>(nl, nh), (u64)N + 2)));
    MsLib* libs = B.get<MsLib>(128);
    if (!nodeFlag || !uniq || !role || !inCnt || !inOff || !nIn || !nOut || !prod || !prodScan || !ctr || !partial || !libs) return support_nomem(err);
    HIPCHK(hipMemsetAsync(nIn, 0, ((u64)N + 2) * sizeof(u32), sm)); HIPCHK(hipMemsetAsync(nOut, 0, ((u64)N + 2) * sizeof(u32), sm));
    HIPCHK(hipMemsetAsync(ctr, 0, 4 * sizeof(unsigned long long), sm));
    const MsTable T = {M->readOff, M->ePair, M->eNf, M->eNr, M->eLoc, M->locs, N};
    const dim3 b256(256);
    { const int rc = unique_reads(d, g, nh, T, nodeFlag, uniq, err); if (rc) return rc; }
    hipLaunchKernelGGL(k_ms_roles, dim3(grid_for(nh, 256)), b256, 0, sm, g, nh, K.flow, role, inCnt, nIn, nOut, ctr);
    hipLaunchKernelGGL(k_ms_cand, dim3(grid_for((u64)N + 1, 256)), b256, 0, sm, nIn, nOut, N, prod);
    { u64 cand = 0; const int rc = scan_u32(d, prod, (u64)N + 1, prodScan, partial, &cand, err); if (rc) return rc; st->candidates = cand; }
    u64 W = 0; { const int rc = scan_u32(d, inCnt, nh, inOff, partial, &W, err); if (rc) return rc; }
    HIPCHK(lap.stop(st->roles_ms));
    unsigned long long hc[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpy(hc, ctr, sizeof hc, hipMemcpyDeviceToHost));
    st->in_halves = hc[0]; st->out_halves = hc[1];
    B.release(nodeFlag); B.release(nIn); B.release(nOut); B.release(prod); B.release(prodScan); B.release(inCnt);
    if (!W || !st->out_halves) { d->support = S.release(); return 0; }
    // ---- the running sums of the whole pool
    HIPCHK(lap.start());
    u32* scan = nullptr; { const int rc = pool_running_sums(d, B, g.lists, nl, partial, scan, support_nomem, err); if (rc) return rc; }
    HIPCHK(lap.stop(st->scan_ms));
    // ---- records: count, scan, write
    HIPCHK(lap.start());
    MsLib hl[128]; for (auto& x : hl) x = MsLib{nullptr, 0, 0, 0, 0};
    const u32 nlib = std::min<u32>(P.libraries, 127);
    for (u32 L = 1; L <= nlib; L++) if (d->mates && d->mates->lib[L].n && P.thr[L] > 0) hl[L] = MsLib{d->mates->lib[L].key, d->mates->lib[L].n, (long long)P.thr[L], 0, 0};
    HIPCHK(hipMemcpyAsync(libs, hl, sizeof hl, hipMemcpyHostToDevice, sm));
    u32* cnt = B.get<u32>(W); u32* pos = B.get<u32>(W);
    if (!cnt || !pos) return support_nomem(err);
    const dim3 gW(grid_for(W, 256));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ms_records<false>), gW, b256, 0, sm, g, nh, inOff, (u32)W, scan, nl, (u64)P.bound, role, uniq, T, libs, nlib, cnt, (const u32*)nullptr, (u64*)nullptr, ctr + 3);
    u64 R = 0; { const int rc = scan_u32(d, cnt, W, pos, partial, &R, err); if (rc) return rc; }      // (synchronises: hl may go out of scope after it)
    HIPCHK(hipMemcpy(hc, ctr, sizeof hc, hipMemcpyDeviceToHost));
    st->entries_within = hc[3]; st->records = R;
    if (R >= (1ull << 32) - RS_TILE) { err = "mate-pair supports: more than 2^32 records"; return SAGE2OV_ERR_LIMIT; }
    if (!R) { HIPCHK(lap.stop(st->records_ms)); d->support = S.release(); return 0; }
    u64* key = B.get<u64>(R); if (!key) return support_nomem(err);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ms_records<true>), gW, b256, 0, sm, g, nh, inOff, (u32)W, scan, nl, (u64)P.bound, role, uniq, T, libs, nlib, (u32*)nullptr, (const u32*)pos, key, ctr + 3);
    HIPCHK(hipGetLastError());
    HIPCHK(lap.stop(st->records_ms));
    B.release(cnt); B.release(pos); B.release(scan); B.release(uniq); B.release(role); B.release(inOff); B.release(partial);
    // ---- sort by (in-half, out-half): the digits below the number of half-edges, in both words
    HIPCHK(lap.start());
    int shifts[8]; const int np = half_pair_passes(nh, shifts);
    u64* ks = nullptr; u32* vs = nullptr; MateStats ms;
    { const int rc = mate_sort(d, B, key, (u32)R, shifts, np, &ks, &vs, &ms, err); if (rc) return rc; }
    st->passes = ms.passes;
    HIPCHK(lap.stop(st->sort_ms));
    B.release(vs);
    // ---- reduce: one entry per distinct key, its support the length of the run
    HIPCHK(lap.start());
    u32* hp = nullptr; u32 E = 0;
    { const int rc = mate_heads(d, B, ks, (u32)R, &hp, &E, err); if (rc) return rc; }
    S->key = (u64*)DevTmp::alloc((u64)E * sizeof(u64)); S->sup = (u32*)DevTmp::alloc((u64)E * sizeof(u32));
    if (!S->key || !S->sup) return support_nomem(err);
    hipLaunchKernelGGL(k_ms_reduce, dim3(grid_for(E, 256)), b256, 0, sm, ks, hp, E, S->key, S->sup, ctr);
    HIPCHK(hipGetLastError());
    HIPCHK(lap.stop(st->reduce_ms));
    HIPCHK(hipMemcpy(hc, ctr, sizeof hc, hipMemcpyDeviceToHost));
    S->E = E; st->keys = E; st->keys2 = hc[2];
    d->support = S.release();
    return 0;
}
int dev_support_export(Device* d, uint64_t* key, uint32_t* support, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    const Support* S = (const Support*)d->support; if (!S) { err = "mate-pair supports: not built"; return SAGE2OV_ERR_INTERNAL; }
    if (S->E) { HIPCHK(hipMemcpy(key, S->key, S->E * sizeof(u64), hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(support, S->sup, S->E * sizeof(u32), hipMemcpyDeviceToHost)); }
    return 0;
}

// =============================================================================================
// the scaffold links of ordered half-edge pairs (kernels_links.inc; the sweep that opens ScaffoldMaker::mergeFinal / mergeFinalSmall, scaffolding.cpp:786-935, :981-1130)
// =============================================================================================
struct Links { u64* key = nullptr; u32* sup = nullptr; int* gap = nullptr; int* sum = nullptr; u64 E = 0; ~Links() { hipFree(key); hipFree(sup); hipFree(gap); hipFree(sum); } };
void dev_links_release(Device* d) { if (d->links) { hipSetDevice(d->ordinal); delete (Links*)d->links; d->links = nullptr; } }
uint64_t dev_links_count(Device* d) { const Links* S = (const Links*)d->links; return S ? S->E : 0; }
static int links_nomem(std::string& err) { err = "scaffold links: out of device memory"; return SAGE2OV_ERR_NOMEM; }
int dev_links_build(Device* d, const LinkParams& P, LinkStats* st, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (!d->s4keep) { err = "scaffold links: no step-4 graph on the device"; return SAGE2OV_ERR_ARG; }
    if (!d->readmap) { err = "scaffold links: the read-to-edge table is not built"; return SAGE2OV_ERR_INTERNAL; }
    dev_links_release(d);
    const S4Keep& K = *(S4Keep*)d->s4keep; const S4Graph& g = K.g; const u32 nh = K.nh; const u64 nl = K.listUsed; const ReadMap* M = (const ReadMap*)d->readmap;
    std::unique_ptr<Links> S(new Links());
    *st = LinkStats();
    if (!nh || !nl) { d->links = S.release(); return 0; }
    const u32 N = (u32)d->N; hipStream_t sm = d->stream;
    DevTmp B; StreamLap lap(sm); HIPCHK(lap.create());
    // ---- unique reads, the list length of every alive half-edge
    HIPCHK(lap.start());
    uint8_t* nodeFlag = B.get<uint8_t>((u64)N + 2); u32* uniq = B.get<u32>((u64)N + 2); u32* hCnt = B.get<u32>(nh); u32* hOff = B.get<u32>(nh);
    unsigned long long* ctr = B.get<unsigned long long>(4); u64* partial = B.get<u64>(scan_partial_words(std::max<u64>(nl, nh) + 1));
    MsLib* libs = B.get<MsLib>(128);
    if (!nodeFlag || !uniq || !hCnt || !hOff || !ctr || !partial || !libs) return links_nomem(err);
    HIPCHK(hipMemsetAsync(ctr, 0, 4 * sizeof(unsigned long long), sm));
    const MsTable T = {M->readOff, M->ePair, M->eNf, M->eNr, M->eLoc, M->locs, N};
    const dim3 b256(256);
    { const int rc = unique_reads(d, g, nh, T, nodeFlag, uniq, err); if (rc) return rc; }
    hipLaunchKernelGGL(k_sl_halves, dim3(grid_for(nh, 256)), b256, 0, sm, g, nh, hCnt, ctr);
    u64 W = 0; { const int rc = scan_u32(d, hCnt, nh, hOff, partial, &W, err); if (rc) return rc; }
    HIPCHK(lap.stop(st->halves_ms));
    B.release(nodeFlag); B.release(hCnt);
    if (!W) { d->links = S.release(); return 0; }
    if (W >= (1ull << 32) - RS_TILE) { err = "scaffold links: more than 2^32 list entries"; return SAGE2OV_ERR_LIMIT; }
    // ---- the running sums of the whole pool
    HIPCHK(lap.start());
    u32* scan = nullptr; { const int rc = pool_running_sums(d, B, g.lists, nl, partial, scan, links_nomem, err); if (rc) return rc; }
    HIPCHK(lap.stop(st->scan_ms));
    // ---- records: count, scan, write
    HIPCHK(lap.start());
    MsLib hl[128]; for (auto& x : hl) x = MsLib{nullptr, 0, 0, 0, 0};
    const u32 nlib = std::min<u32>(P.libraries, 127);
    for (u32 L = 1; L <= nlib; L++) if (d->mates && d->mates->lib[L].n && P.thr[L] > 0) hl[L] = MsLib{d->mates->lib[L].key, d->mates->lib[L].n, (long long)P.thr[L], P.gbase[L], 0};
    HIPCHK(hipMemcpyAsync(libs, hl, sizeof hl, hipMemcpyHostToDevice, sm));
    u32* cnt = B.get<u32>(W); u32* pos = B.get<u32>(W);
    if (!cnt || !pos) return links_nomem(err);
    const dim3 gW(grid_for(W, 256));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sl_records<false>), gW, b256, 0, sm, g, nh, hOff, (u32)W, scan, nl, (u64)P.bound, uniq, T, libs, nlib, cnt, (const u32*)nullptr, (u64*)nullptr, (u32*)nullptr, ctr);
    u64 R = 0; { const int rc = scan_u32(d, cnt, W, pos, partial, &R, err); if (rc) return rc; }      // (synchronises: hl may go out of scope after it)
    unsigned long long hc[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpy(hc, ctr, sizeof hc, hipMemcpyDeviceToHost));
    st->halves = hc[0]; st->entries_within = hc[1]; st->unique_entries = hc[2]; st->mate_entries = hc[3]; st->records = R;
    if (R >= (1ull << 32) - RS_TILE) { err = "scaffold links: more than 2^32 records"; return SAGE2OV_ERR_LIMIT; }
    if (!R) { HIPCHK(lap.stop(st->records_ms)); d->links = S.release(); return 0; }
    u64* key = B.get<u64>(R); u32* val = B.get<u32>(R); if (!key || !val) return links_nomem(err);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sl_records<true>), gW, b256, 0, sm, g, nh, hOff, (u32)W, scan, nl, (u64)P.bound, uniq, T, libs, nlib, (u32*)nullptr, (const u32*)pos, key, val, ctr);
    HIPCHK(hipGetLastError());
    HIPCHK(lap.stop(st->records_ms));
    B.release(cnt); B.release(pos); B.release(scan); B.release(uniq); B.release(hOff);
    // ---- sort by (a, b): the digits below the number of half-edges, in both words; then the values in sorted order and their running sum
    HIPCHK(lap.start());
    int shifts[8]; const int np = half_pair_passes(nh, shifts);
    u64* ks = nullptr; u32* vs = nullptr; MateStats ms;
    { const int rc = mate_sort(d, B, key, (u32)R, shifts, np, &ks, &vs, &ms, err); if (rc) return rc; }
    st->passes = ms.passes;
    HIPCHK(lap.stop(st->sort_ms));
    HIPCHK(lap.start());
    B.release(partial);                                                            // (sized for the pool; the records may be more)
    u32* sv = B.get<u32>(R + 1); u32* sc = B.get<u32>(R + 1); u64* partialR = B.get<u64>(scan_partial_words(R + 1)); if (!sv || !sc || !partialR) return links_nomem(err);
    hipLaunchKernelGGL(k_sl_gather, dim3(grid_for(R + 1, 256)), b256, 0, sm, vs, val, (u32)R, sv);
    { const int rc = scan_u32(d, sv, R + 1, sc, partialR, nullptr, err); if (rc) return rc; }
    HIPCHK(hipStreamSynchronize(sm));
    B.release(vs); B.release(val); B.release(sv); B.release(partialR);
    // ---- reduce: one row per distinct key
    u32* hp = nullptr; u32 E = 0;
    { const int rc = mate_heads(d, B, ks, (u32)R, &hp, &E, err); if (rc) return rc; }
    S->key = (u64*)DevTmp::alloc((u64)E * sizeof(u64)); S->sup = (u32*)DevTmp::alloc((u64)E * sizeof(u32)); S->gap = (int*)DevTmp::alloc((u64)E * sizeof(int)); S->sum = (int*)DevTmp::alloc((u64)E * sizeof(int));
    if (!S->key || !S->sup || !S->gap || !S->sum) return links_nomem(err);
    hipLaunchKernelGGL(k_sl_reduce, dim3(grid_for(E, 256)), b256, 0, sm, ks, hp, sc, E, S->key, S->sup, S->gap, S->sum);
    HIPCHK(hipGetLastError());
    HIPCHK(lap.stop(st->reduce_ms));
    S->E = E; st->keys = E;
    d->links = S.release();
    return 0;
}
int dev_links_export(Device* d, uint64_t* key, uint32_t* support, int32_t* gap, int32_t* gapSum, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    const Links* S = (const Links*)d->links; if (!S) { err = "scaffold links: not built"; return SAGE2OV_ERR_INTERNAL; }
    if (S->E) {
        HIPCHK(hipMemcpy(key, S->key, S->E * sizeof(u64), hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(support, S->sup, S->E * sizeof(u32), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(gap, S->gap, S->E * sizeof(int), hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(gapSum, S->sum, S->E * sizeof(int), hipMemcpyDeviceToHost));
    }
    return 0;
}

// =============================================================================================
// the path supports of consecutive half-edge pairs (kernels_paths.inc; the sweep of ContigExtender::findPathSupports / findPathSupportsNew, mergeContigs.cpp:118-353, :359-743)
// =============================================================================================
struct EstFlags { unsigned char* f[128] = {}; u64 n[128] = {}; ~EstFlags() { for (unsigned char* p : f) hipFree(p); } };
void dev_estflags_release(Device* d) { if (d->estflags) { hipSetDevice(d->ordinal); delete (EstFlags*)d->estflags; d->estflags = nullptr; } }
int dev_estflags_keep(Device* d, int library, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (!d->readmap) { err = "estimate flags: the read-to-edge table is not built"; return SAGE2OV_ERR_INTERNAL; }
    if (!d->estflags) d->estflags = new EstFlags();
    EstFlags& F = *(EstFlags*)d->estflags; const ReadMapLib& J = ((const ReadMap*)d->readmap)->lib[library];
    hipFree(F.f[library]); F.f[library] = nullptr; F.n[library] = 0;
    if (!J.nflag) return 0;
    F.f[library] = (unsigned char*)DevTmp::alloc(J.nflag);
    if (!F.f[library]) { err = "estimate flags: out of device memory"; return SAGE2OV_ERR_NOMEM; }
    HIPCHK(hipMemcpyAsync(F.f[library], J.flag, J.nflag, hipMemcpyDeviceToDevice, d->stream)); HIPCHK(hipStreamSynchronize(d->stream));
    F.n[library] = J.nflag;
    return 0;
}
struct PathTable { u64* key = nullptr; u32* sup = nullptr; u64 E = 0; ~PathTable() { hipFree(key); hipFree(sup); } };
void dev_paths_release(Device* d) { if (d->paths) { hipSetDevice(d->ordinal); delete (PathTable*)d->paths; d->paths = nullptr; } }
uint64_t dev_paths_count(Device* d) { const PathTable* S = (const PathTable*)d->paths; return S ? S->E : 0; }
static int paths_nomem(std::string& err) { err = "path supports: out of device memory"; return SAGE2OV_ERR_NOMEM; }
static int paths_limit(const char* what, std::string& err) { err = std::string("path supports: more than 2^32 ") + what; return SAGE2OV_ERR_LIMIT; }
int dev_paths_build(Device* d, const PathParams& P, PathStats* st, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (!d->s4keep) { err = "path supports: no step-4 graph on the device"; return SAGE2OV_ERR_ARG; }
    if (!d->readmap) { err = "path supports: the read-to-edge table is not built"; return SAGE2OV_ERR_INTERNAL; }
    dev_paths_release(d);
    const S4Keep& K = *(S4Keep*)d->s4keep; const S4Graph& g = K.g; const u32 nh = K.nh; const u64 nl = K.listUsed; const ReadMap* M = (const ReadMap*)d->readmap;
    std::unique_ptr<PathTable> S(new PathTable());
    *st = PathStats();
    if (!K.flow || !nh || !nl) { d->paths = S.release(); return 0; }                   // every flow is 0 (the graph as step 4 leaves it): no path has a first edge
    if (P.bound >= (1ull << 31)) { err = "path supports: maximumUpperBoundOfInsert beyond 2^31 (a path's length is a 32-bit value)"; return SAGE2OV_ERR_LIMIT; }
    const u32 N = (u32)d->N; hipStream_t sm = d->stream; const u64 lim = (1ull << 32) - RS_TILE;
    DevTmp B; StreamLap lap(sm); HIPCHK(lap.create());
    const dim3 b256(256);
    // ---- the claim: unique reads, the list entries of the alive halves, the running sums, the minimum per read
    HIPCHK(lap.start());
    uint8_t* nodeFlag = B.get<uint8_t>((u64)N + 2); u32* uniq = B.get<u32>((u64)N + 2); u32* claim = B.get<u32>((u64)N + 2); u32* hCnt = B.get<u32>(nh); u32* hOff = B.get<u32>(nh);
    unsigned long long* ctr = B.get<unsigned long long>(12); u64* partial = B.get<u64>(scan_partial_words(std::max<u64>(std::max<u64>(nl, nh), (u64)N + 2) + 1));
    if (!nodeFlag || !uniq || !claim || !hCnt || !hOff || !ctr || !partial) return paths_nomem(err);
    HIPCHK(hipMemsetAsync(ctr, 0, 12 * sizeof(unsigned long long), sm)); HIPCHK(hipMemsetAsync(claim, 0xFF, ((u64)N + 2) * sizeof(u32), sm));
    const MsTable T = {M->readOff, M->ePair, M->eNf, M->eNr, M->eLoc, M->locs, N};
    { const int rc = unique_reads(d, g, nh, T, nodeFlag, uniq, err); if (rc) return rc; }
    hipLaunchKernelGGL(k_sl_halves, dim3(grid_for(nh, 256)), b256, 0, sm, g, nh, hCnt, ctr + 11);
    u64 W = 0; { const int rc = scan_u32(d, hCnt, nh, hOff, partial, &W, err); if (rc) return rc; }
    if (W >= lim) return paths_limit("list entries", err);
    if (!W) { d->paths = S.release(); return 0; }
    u32* scan = nullptr; { const int rc = pool_running_sums(d, B, g.lists, nl, partial, scan, paths_nomem, err); if (rc) return rc; }
    hipLaunchKernelGGL(k_pt_claim, dim3(grid_for(W, 256)), b256, 0, sm, g, nh, hOff, (u32)W, scan, nl, (u64)P.bound, N, claim);
    HIPCHK(hipGetLastError());
    HIPCHK(lap.stop(st->claim_ms));
    B.release(scan); B.release(hCnt); B.release(hOff); B.release(nodeFlag);
    // ---- the start nodes: (claiming node, end node) records of the claimed reads, distinct and ascending
    HIPCHK(lap.start());
    u32* rcnt = B.get<u32>((u64)N + 2); u32* rpos = B.get<u32>((u64)N + 2); if (!rcnt || !rpos) return paths_nomem(err);
    const dim3 gN(grid_for((u64)N + 1, 256));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pt_starts<false>), gN, b256, 0, sm, g, T, claim, rcnt, (const u32*)nullptr, (u64*)nullptr, ctr);
    u64 R0 = 0; { const int rc = scan_u32(d, rcnt, (u64)N + 1, rpos, partial, &R0, err); if (rc) return rc; }
    unsigned long long hc[12] = {};
    HIPCHK(hipMemcpy(hc, ctr, sizeof hc, hipMemcpyDeviceToHost));
    st->claimed_reads = hc[0];
    if (R0 >= lim) return paths_limit("start records", err);
    if (!R0) { HIPCHK(lap.stop(st->starts_ms)); d->paths = S.release(); return 0; }
    u64* skey = B.get<u64>(R0); if (!skey) return paths_nomem(err);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pt_starts<true>), gN, b256, 0, sm, g, T, claim, (u32*)nullptr, (const u32*)rpos, skey, ctr);
    HIPCHK(hipGetLastError());
    int shifts[8]; int np = half_pair_passes(N + 1u, shifts);
    u64* ks = nullptr; u32* vs = nullptr; MateStats ms;
    { const int rc = mate_sort(d, B, skey, (u32)R0, shifts, np, &ks, &vs, &ms, err); if (rc) return rc; }
    B.release(vs); B.release(rcnt); B.release(rpos);
    u32* hp = nullptr; u32 nS = 0;
    { const int rc = mate_heads(d, B, ks, (u32)R0, &hp, &nS, err); if (rc) return rc; }
    u32* startNode = B.get<u32>(nS); u32* sflag = B.get<u32>(nS); u32* spos = B.get<u32>(nS); u64* partialS = B.get<u64>(scan_partial_words((u64)nS + 1));
    if (!startNode || !sflag || !spos || !partialS) return paths_nomem(err);
    hipLaunchKernelGGL(k_pt_take, dim3(grid_for(nS, 256)), b256, 0, sm, ks, hp, nS, startNode, sflag);
    u64 C64 = 0; { const int rc = scan_u32(d, sflag, nS, spos, partialS, &C64, err); if (rc) return rc; }
    const u32 C = (u32)C64;
    u32* segOff = B.get<u32>((u64)C + 1); u32* segNode = B.get<u32>(C); if (!segOff || !segNode) return paths_nomem(err);
    { const int rc = head_positions(d, sflag, spos, nS, segOff, C, err); if (rc) return rc; }
    hipLaunchKernelGGL(k_pt_seg_nodes, dim3(grid_for(C, 256)), b256, 0, sm, ks, hp, segOff, C, segNode);
    HIPCHK(hipGetLastError());
    HIPCHK(lap.stop(st->starts_ms));
    B.release(ks); B.release(hp); B.release(sflag); B.release(spos);
    st->start_nodes = nS; st->claiming_nodes = C; st->passes = ms.passes;
    // ---- the walk: adjacency (alive halves of every node, oldest first), count, scan, fill
    HIPCHK(lap.start());
    S4Graph ga = g; u32* cursor = B.get<u32>((u64)N + 2);
    ga.deg = B.get<u32>((u64)N + 2); ga.adjOff = B.get<u32>((u64)N + 2); ga.adj = B.get<u32>(nh);
    u32* pcnt = B.get<u32>((u64)nS + 1); u32* pathOff = B.get<u32>((u64)nS + 1);
    if (!cursor || !ga.deg || !ga.adjOff || !ga.adj || !pcnt || !pathOff) return paths_nomem(err);
    HIPCHK(hipMemsetAsync(ga.deg, 0, ((u64)N + 2) * sizeof(u32), sm)); HIPCHK(hipMemsetAsync(cursor, 0, ((u64)N + 2) * sizeof(u32), sm));
    HIPCHK(hipMemsetAsync(pcnt, 0, ((u64)nS + 1) * sizeof(u32), sm));
    hipLaunchKernelGGL(k_s4_degree, dim3(grid_for(nh, 256)), b256, 0, sm, ga, nh);
    { const int rc = scan_u32(d, ga.deg, (u64)N + 1, ga.adjOff, partial, nullptr, err); if (rc) return rc; }
    hipLaunchKernelGGL(k_s4_fill, dim3(grid_for(nh, 256)), b256, 0, sm, ga, nh, cursor);
    hipLaunchKernelGGL(k_s4_sortadj, gN, b256, 0, sm, ga, N);
    const dim3 gC(grid_for(C, PT_BLOCK)), bW(PT_BLOCK);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pt_walk<false>), gC, bW, 0, sm, ga, (const float*)K.flow, C, (const u32*)segOff, (const u32*)startNode, (u64)P.bound, pcnt, (const u32*)nullptr, (PtPath*)nullptr, (u64)0, ctr);
    u64 PT = 0; { const int rc = scan_u32(d, pcnt, (u64)nS + 1, pathOff, partialS, &PT, err); if (rc) return rc; }
    HIPCHK(hipMemcpy(hc, ctr, sizeof hc, hipMemcpyDeviceToHost));
    st->paths = hc[1]; st->capped_nodes = hc[2];
    if (PT >= lim) return paths_limit("paths", err);
    if (PT != hc[1]) { err = "path supports: the count pass and its scan disagree"; return SAGE2OV_ERR_INTERNAL; }
    if (!PT) { HIPCHK(lap.stop(st->walk_ms)); d->paths = S.release(); return 0; }
    PtPath* paths = B.get<PtPath>(PT); if (!paths) return paths_nomem(err);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pt_walk<true>), gC, bW, 0, sm, ga, (const float*)K.flow, C, (const u32*)segOff, (const u32*)startNode, (u64)P.bound, (u32*)nullptr, (const u32*)pathOff, paths, (u64)PT, ctr);
    HIPCHK(hipGetLastError());
    HIPCHK(lap.stop(st->walk_ms));
    B.release(cursor); B.release(ga.deg); B.release(ga.adjOff); B.release(ga.adj); B.release(pcnt);
    // ---- the votes: one lane per mate entry of every valid library, then the survivors as records
    HIPCHK(lap.start());
    const EstFlags* F = (const EstFlags*)d->estflags; const u32 nlib = std::min<u32>(P.libraries, 127);
    u64 Mall = 0;
    for (u32 L = 1; L <= nlib; L++) {
        const u64 n = d->mates ? d->mates->lib[L].n : 0; if (!n || !P.valid[L]) continue;
        if (!F || F->n[L] != n) { err = "path supports: no estimate flags for a library's mate entries"; return SAGE2OV_ERR_INTERNAL; }
        Mall += n;
    }
    if (Mall >= lim) return paths_limit("mate entries", err);
    if (!Mall) { HIPCHK(lap.stop(st->vote_ms)); d->paths = S.release(); return 0; }
    u32* first = B.get<u32>(Mall); u32* fe1 = B.get<u32>(Mall); u32* mask = B.get<u32>(Mall); u32* vcnt = B.get<u32>(Mall); u32* vpos = B.get<u32>(Mall);
    u64* partialM = B.get<u64>(scan_partial_words(Mall));
    if (!first || !fe1 || !mask || !vcnt || !vpos || !partialM) return paths_nomem(err);
    const PtIndex X = {segNode, segOff, C, startNode, pathOff, paths};
    { u64 base = 0;
      for (u32 L = 1; L <= nlib; L++) {
          const u64 n = d->mates ? d->mates->lib[L].n : 0; if (!n || !P.valid[L]) continue;
          const PtLib lib = {d->mates->lib[L].key, F->f[L], n, (long long)P.lower[L], (long long)P.upper[L]};
          hipLaunchKernelGGL(k_pt_vote, dim3(grid_for(n, 256)), b256, 0, sm, g, nh, T, (const u32*)uniq, (const u32*)claim, lib, X, first + base, fe1 + base, mask + base, vcnt + base, ctr);
          base += n;
      } }
    u64 R = 0; { const int rc = scan_u32(d, vcnt, Mall, vpos, partialM, &R, err); if (rc) return rc; }
    HIPCHK(hipMemcpy(hc, ctr, sizeof hc, hipMemcpyDeviceToHost));
    st->eligible = hc[3]; st->voting = hc[4]; st->mirrored = hc[5]; st->records = R;
    if (R >= lim) return paths_limit("records", err);
    if (!R) { HIPCHK(lap.stop(st->vote_ms)); d->paths = S.release(); return 0; }
    u64* key = B.get<u64>(R); if (!key) return paths_nomem(err);
    hipLaunchKernelGGL(k_pt_emit, dim3(grid_for(Mall, 256)), b256, 0, sm, (const u32*)first, (const u32*)fe1, (const u32*)mask, (const u32*)vpos, (u32)Mall, (const PtPath*)paths, (u64)R, key);
    HIPCHK(hipGetLastError());
    HIPCHK(lap.stop(st->vote_ms));
    B.release(first); B.release(fe1); B.release(mask); B.release(vcnt); B.release(vpos); B.release(partialM); B.release(paths); B.release(pathOff); B.release(startNode);
    B.release(segOff); B.release(segNode); B.release(uniq); B.release(claim); B.release(partial); B.release(partialS);
    // ---- sort by (a, b) and reduce: one row per distinct key, its support the length of the run
    HIPCHK(lap.start());
    np = half_pair_passes(nh, shifts);
    MateStats ms2;
    { const int rc = mate_sort(d, B, key, (u32)R, shifts, np, &ks, &vs, &ms2, err); if (rc) return rc; }
    st->passes += ms2.passes;
    HIPCHK(lap.stop(st->sort_ms));
    B.release(vs);
    HIPCHK(lap.start());
    u32 E = 0;
    { const int rc = mate_heads(d, B, ks, (u32)R, &hp, &E, err); if (rc) return rc; }
    S->key = (u64*)DevTmp::alloc((u64)E * sizeof(u64)); S->sup = (u32*)DevTmp::alloc((u64)E * sizeof(u32));
    if (!S->key || !S->sup) return paths_nomem(err);
    hipLaunchKernelGGL(k_ms_reduce, dim3(grid_for(E, 256)), b256, 0, sm, ks, hp, E, S->key, S->sup, ctr + 8);
    HIPCHK(hipGetLastError());
    HIPCHK(lap.stop(st->reduce_ms));
    S->E = E; st->rows = E;
    d->paths = S.release();
    return 0;
}
int dev_paths_export(Device* d, uint64_t* key, uint32_t* support, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    const PathTable* S = (const PathTable*)d->paths; if (!S) { err = "path supports: not built"; return SAGE2OV_ERR_INTERNAL; }
    if (S->E) { HIPCHK(hipMemcpy(key, S->key, S->E * sizeof(u64), hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(support, S->sup, S->E * sizeof(u32), hipMemcpyDeviceToHost)); }
    return 0;
}

// =============================================================================================
// the contig table and the contig strings (kernels_contig.inc; OverlapGraph::printGraph / saveContigsToFile, overlapGraph.cpp:507-784)
// =============================================================================================
struct Contigs {
    CtRow* rows = nullptr; u32* chunkOff = nullptr; u32* dScan = nullptr; u64 R = 0, chunks = 0;
    struct Buf { uint4* dev = nullptr; char* host = nullptr; u64 cap = 0; hipEvent_t a = nullptr, b = nullptr, done = nullptr; } buf[2];      // a range is spelled into one while the caller formats the other
    ~Contigs() { hipFree(rows); hipFree(chunkOff); hipFree(dScan);
                 for (auto& B : buf) { hipFree(B.dev); if (B.host) hipHostFree(B.host); if (B.a) hipEventDestroy(B.a); if (B.b) hipEventDestroy(B.b); if (B.done) hipEventDestroy(B.done); } }
};
void dev_contigs_release(Device* d) { if (d->contigs) { hipSetDevice(d->ordinal); hipStreamSynchronize(d->stream); delete (Contigs*)d->contigs; d->contigs = nullptr; } }
static int contigs_nomem(std::string& err) { err = "contigs: out of device memory"; return SAGE2OV_ERR_NOMEM; }
// whichever read store is resident: the id-ordered one, or (memory-diet mode) the locality-ordered one through posOf
static bool contig_reads(Device* d, CtReads& R) {
    const bool byPos = d->reads == nullptr;
    if (byPos && !(d->readsLoc && d->posOf)) return false;
    R = CtReads{byPos ? d->readsLoc : d->reads, d->posOf, byPos ? 1 : 0, d->S, (u32)d->uniL, (u32)d->N, slot_len_mask(d->S)};
    return true;
}
int dev_contigs_build(Device* d, uint32_t threshold, std::vector<ContigRow>& out, ContigBuildStats* st, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (!d->s4keep) { err = "contigs: no step-4 graph on the device"; return SAGE2OV_ERR_ARG; }
    dev_contigs_release(d);
    CtReads Rd; if (!contig_reads(d, Rd)) { err = "contigs: no read store on the device"; return SAGE2OV_ERR_ARG; }
    const S4Keep& K = *(S4Keep*)d->s4keep; const S4Graph& g = K.g; const u32 nh = K.nh; const u64 nl = K.listUsed; const u32 N = (u32)d->N; hipStream_t sm = d->stream;
    std::unique_ptr<Contigs> C(new Contigs());
    *st = ContigBuildStats(); out.clear();
    DevTmp B; StreamLap lap(sm); HIPCHK(lap.create());
    const dim3 b256(256);
    // ---- select and compact
    HIPCHK(lap.start());
    u32* sel = B.get<u32>(nh); u32* pos = B.get<u32>(nh); unsigned long long* ctr = B.get<unsigned long long>(2);
    u64* partial = B.get<u64>(scan_partial_words(std::max<u64>(nl + 1, nh)));
    if (!sel || !pos || !ctr || !partial) return contigs_nomem(err);
    HIPCHK(hipMemsetAsync(ctr, 0, 2 * sizeof(unsigned long long), sm));
    if (nh) hipLaunchKernelGGL(k_ct_select, dim3(grid_for(nh, 256)), b256, 0, sm, g, nh, (u32)threshold, sel, ctr);
    u64 R = 0; { const int rc = scan_u32(d, sel, nh, pos, partial, &R, err); if (rc) return rc; }
    HIPCHK(lap.stop(st->select_ms));
    if (!R) { d->contigs = C.release(); return 0; }
    unsigned long long hc[2] = {0, 0}; HIPCHK(hipMemcpy(hc, ctr, sizeof hc, hipMemcpyDeviceToHost));
    const u32 longest = (u32)hc[0];
    // ---- order: (len descending, from ascending, index descending) by stable passes over the digits of (longest - len, from) that can be non-zero
    HIPCHK(lap.start());
    u64* key = B.get<u64>(R); u32* hs = B.get<u32>(R); u32* rowH = B.get<u32>(R);
    if (!key || !hs || !rowH) return contigs_nomem(err);
    hipLaunchKernelGGL(k_ct_keys, dim3(grid_for(nh, 256)), b256, 0, sm, g, nh, sel, pos, (u32)R, longest, key, hs);
    int shifts[8], np = 0; { int bn = 0, bl = 0; while (((u64)N >> bn) != 0) bn++; while (((u64)longest >> bl) != 0) bl++;
                             for (int p = 0; p < 8; p++) { const int lo = 8 * p; if (lo < 32 ? lo < bn : lo - 32 < bl) shifts[np++] = lo; } }
    u64* ks = nullptr; u32* vs = nullptr; MateStats ms;
    { const int rc = mate_sort(d, B, key, (u32)R, shifts, np, &ks, &vs, &ms, err); if (rc) return rc; }
    hipLaunchKernelGGL(k_ct_gather, dim3(grid_for(R, 256)), b256, 0, sm, vs, hs, (u32)R, rowH);
    HIPCHK(hipGetLastError());
    HIPCHK(lap.stop(st->sort_ms));
    st->passes = ms.passes;
    B.release(sel); B.release(pos); B.release(vs); B.release(hs); if (ks != key) B.release(ks); B.release(key);
    // ---- layout: the running distPrevious (kept for the spelling), the gap and N counts, the rows, where their chunks begin
    HIPCHK(lap.start());
    u32* tmp = B.get<u32>(nl + 1); u32* gap = B.get<u32>(nl + 1); u32* ns = B.get<u32>(nl + 1); u32* gScan = B.get<u32>(nl + 1); u32* nScan = B.get<u32>(nl + 1); u32* deg = B.get<u32>((u64)N + 2);
    u32* chunks = B.get<u32>(R + 1);
    C->dScan = (u32*)DevTmp::alloc((nl + 1) * sizeof(u32)); C->rows = (CtRow*)DevTmp::alloc(R * sizeof(CtRow)); C->chunkOff = (u32*)DevTmp::alloc((R + 1) * sizeof(u32));
    if (!tmp || !gap || !ns || !gScan || !nScan || !deg || !chunks || !C->dScan || !C->rows || !C->chunkOff) return contigs_nomem(err);
    HIPCHK(hipMemsetAsync(deg, 0, ((u64)N + 2) * sizeof(u32), sm));
    HIPCHK(hipMemsetAsync(tmp + nl, 0, sizeof(u32), sm)); HIPCHK(hipMemsetAsync(gap + nl, 0, sizeof(u32), sm)); HIPCHK(hipMemsetAsync(ns + nl, 0, sizeof(u32), sm));
    hipLaunchKernelGGL(k_ct_degree, dim3(grid_for(nh, 256)), b256, 0, sm, g, nh, deg);
    if (nl) {
        hipLaunchKernelGGL(k_rm_dprev, dim3(grid_for_capped(nl, 256)), b256, 0, sm, g.lists, nl, tmp);
        hipLaunchKernelGGL(k_ct_gaps, dim3(grid_for_capped(nl, 256)), b256, 0, sm, g.lists, nl, Rd, gap, ns);
    }
    { const int rc = scan_u32(d, tmp, nl + 1, C->dScan, partial, nullptr, err); if (rc) return rc; }
    { const int rc = scan_u32(d, gap, nl + 1, gScan, partial, nullptr, err); if (rc) return rc; }
    { const int rc = scan_u32(d, ns, nl + 1, nScan, partial, nullptr, err); if (rc) return rc; }
    hipLaunchKernelGGL(k_ct_layout, dim3(grid_for(R + 1, 256)), b256, 0, sm, g, rowH, (u32)R, Rd, deg, C->dScan, gScan, nScan, nl, C->rows, chunks);
    u64 total = 0; { const int rc = scan_u32(d, chunks, R + 1, C->chunkOff, partial, &total, err); if (rc) return rc; }
    HIPCHK(lap.stop(st->layout_ms));
    static_assert(sizeof(CtRow) == sizeof(ContigRow), "the row as the host takes it");
    out.resize(R); HIPCHK(hipMemcpy(out.data(), C->rows, R * sizeof(CtRow), hipMemcpyDeviceToHost));
    u64 sum = 0;
    for (const ContigRow& r : out) { if (r.flags & CT_LIMIT) { err = "contigs: a contig string of 2^32 characters or more"; return SAGE2OV_ERR_LIMIT; } sum += ((u64)r.string_length + 15) >> 4; }
    if (sum != total || total >= (1ull << 32) - RS_TILE) { err = "contigs: 2^36 characters or more in all"; return SAGE2OV_ERR_LIMIT; }
    C->R = R; C->chunks = total;
    d->contigs = C.release();
    return 0;
}
// rows [first, first + count), whose chunks are [chunk0, chunk0 + nChunks) of the table, into buffer `which` (0 or 1) and on to its pinned host image; nothing is waited for
int dev_contigs_spell_begin(Device* d, int which, uint64_t first, uint64_t count, uint64_t chunk0, uint64_t nChunks, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    Contigs* C = (Contigs*)d->contigs; if (!C || !d->s4keep) { err = "contigs: not built"; return SAGE2OV_ERR_INTERNAL; }
    if (which < 0 || which > 1 || first + count > C->R || chunk0 + nChunks > C->chunks) { err = "contigs: range outside the table"; return SAGE2OV_ERR_INTERNAL; }
    CtReads Rd; if (!contig_reads(d, Rd)) { err = "contigs: no read store on the device"; return SAGE2OV_ERR_ARG; }
    Contigs::Buf& B = C->buf[which];
    if (!B.a) { HIPCHK(hipEventCreate(&B.a)); HIPCHK(hipEventCreate(&B.b)); HIPCHK(hipEventCreate(&B.done)); }
    if (B.cap < nChunks) {
        HIPCHK(hipStreamSynchronize(d->stream));
        hipFree(B.dev); if (B.host) hipHostFree(B.host); B.dev = nullptr; B.host = nullptr; B.cap = 0;
        B.dev = (uint4*)DevTmp::alloc(nChunks * 16); if (!B.dev) return contigs_nomem(err);
        if (hipHostMalloc((void**)&B.host, nChunks * 16, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); B.host = nullptr; err = "contigs: out of pinned host memory"; return SAGE2OV_ERR_NOMEM; }
        B.cap = nChunks;
    }
    const S4Keep& K = *(S4Keep*)d->s4keep;
    HIPCHK(hipEventRecord(B.a, d->stream));
    if (nChunks) hipLaunchKernelGGL(k_ct_spell, dim3(grid_for(nChunks, 256)), dim3(256), 0, d->stream, K.g, Rd, C->rows, C->chunkOff, (u32)first, (u32)count, C->dScan, K.listUsed, B.dev, (u32)nChunks);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(B.b, d->stream));
    if (nChunks) HIPCHK(hipMemcpyAsync(B.host, B.dev, nChunks * 16, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipEventRecord(B.done, d->stream));
    return 0;
}
// the host image of buffer `which`, once its copy has arrived: a row begins 16 * (its first chunk - chunk0) bytes in; ms += the kernel's time
int dev_contigs_spell_wait(Device* d, int which, const char** image, double* ms, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    Contigs* C = (Contigs*)d->contigs; if (!C || which < 0 || which > 1 || !C->buf[which].done) { err = "contigs: nothing was spelled"; return SAGE2OV_ERR_INTERNAL; }
    Contigs::Buf& B = C->buf[which];
    HIPCHK(hipEventSynchronize(B.done));
    float t = 0; if (hipEventElapsedTime(&t, B.a, B.b) == hipSuccess) *ms += t; else (void)hipGetLastError();
    *image = B.host;
    return 0;
}

// =============================================================================================
// step 5 around its solver (kernels_copycount.inc; CopyCountEstimator, copycountEstimator.cpp:29-417)
// =============================================================================================
struct CopyCount {
    unsigned short* freq = nullptr; unsigned long long* kPair = nullptr; u64 present = 0;      // of dev_copycount_prepare
    u32 *adj = nullptr, *hp = nullptr, *nodeOf = nullptr; CcArc* arcs = nullptr; u64 F = 0, E = 0, nArcs = 0; bool net = false;      // of dev_flownet_build
    long long* solFlow = nullptr; void* solPrice = nullptr; u32 solWords = 0; u64 solScale = 0; bool solved = false;      // of dev_flow_solve: a flow per arc, a price of solWords 64-bit words per network node (nodes 1..n of n + 2)
    void drop_solution() { hipFree(solFlow); hipFree(solPrice); solFlow = nullptr; solPrice = nullptr; solWords = 0; solScale = 0; solved = false; }
    void drop_net() { drop_solution(); hipFree(adj); hipFree(hp); hipFree(nodeOf); hipFree(arcs); adj = hp = nodeOf = nullptr; arcs = nullptr; F = E = nArcs = 0; net = false; }
    ~CopyCount() { drop_net(); hipFree(freq); hipFree(kPair); }
};
static_assert(sizeof(CcArc) == sizeof(FlowArc) && sizeof(CcArc) == 20, "an arc record is five 32-bit words");
void dev_copycount_release(Device* d) { if (d->copycount) { hipSetDevice(d->ordinal); delete (CopyCount*)d->copycount; d->copycount = nullptr; } }
static int copycount_nomem(std::string& err) { err = "copy counts: out of device memory"; return SAGE2OV_ERR_NOMEM; }
// the 8-bit digits of a node id that can be non-zero
static int copycount_passes(u64 N, int* shifts) { int b = 0; while ((N >> b) != 0) b++; int np = 0; for (int p = 0; p < 4; p++) if (8 * p < b) shifts[np++] = 8 * p; return np; }

int dev_copycount_prepare(Device* d, const uint16_t* freq, CopyCountStats* st, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (!d->s4keep) { err = "copy counts: no step-4 graph on the device"; return SAGE2OV_ERR_ARG; }
    if (d->N >= (1ull << 32) - 2) { err = "copy counts: read ids beyond 2^32 - 3"; return SAGE2OV_ERR_LIMIT; }
    dev_copycount_release(d);
    const S4Keep& K = *(S4Keep*)d->s4keep; const S4Graph& g = K.g; const u32 nh = K.nh; const u64 nl = K.listUsed; const u32 N = (u32)d->N; hipStream_t sm = d->stream;
    std::unique_ptr<CopyCount> S(new CopyCount());
    DevTmp B; StreamLap lap(sm); HIPCHK(lap.create());
    HIPCHK(lap.start());
    const u64 np = (u64)nh / 2 + 1;
    S->freq = (unsigned short*)DevTmp::alloc(((u64)N + 2) * sizeof(unsigned short)); S->kPair = (unsigned long long*)DevTmp::alloc(np * sizeof(unsigned long long));
    uint8_t* present = B.get<uint8_t>((u64)N + 2); u32* hCnt = B.get<u32>(nh); u32* hOff = B.get<u32>(nh); unsigned long long* ctr = B.get<unsigned long long>(2);
    u64* partial = B.get<u64>(scan_partial_words((u64)nh + 1));
    if (!S->freq || !S->kPair || !present || !hCnt || !hOff || !ctr || !partial) return copycount_nomem(err);
    HIPCHK(hipMemcpyAsync(S->freq, freq, ((u64)N + 1) * sizeof(unsigned short), hipMemcpyHostToDevice, sm));
    HIPCHK(hipMemsetAsync(S->kPair, 0, np * sizeof(unsigned long long), sm)); HIPCHK(hipMemsetAsync(present, 0, (u64)N + 2, sm)); HIPCHK(hipMemsetAsync(ctr, 0, 2 * sizeof(unsigned long long), sm));
    const dim3 b256(256);
    u64 W = 0;
    if (nh) {
        hipLaunchKernelGGL(k_cc_nodes, dim3(grid_for(nh, 256)), b256, 0, sm, g, nh, present, N);
        hipLaunchKernelGGL(k_sl_halves, dim3(grid_for(nh, 256)), b256, 0, sm, g, nh, hCnt, ctr + 1);
        { const int rc = scan_u32(d, hCnt, nh, hOff, partial, &W, err); if (rc) return rc; }
        if (W >= (1ull << 32) - RS_TILE) { err = "copy counts: more than 2^32 list entries"; return SAGE2OV_ERR_LIMIT; }
        if (W) hipLaunchKernelGGL(k_cc_entries, dim3(grid_for(W, 256)), b256, 0, sm, g, nh, hOff, (u32)W, nl, S->freq, N, present, S->kPair);
    }
    hipLaunchKernelGGL(k_cc_present, dim3((unsigned)std::min<u64>(grid_for((u64)N + 1, 256), 4096)), b256, 0, sm, present, S->freq, N, ctr);
    HIPCHK(hipGetLastError());
    unsigned long long hc[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, sm));
    HIPCHK(lap.stop(st->k_ms));
    S->present = hc[0]; st->present = hc[0];
    d->copycount = S.release();
    return 0;
}
int dev_copycount_round(Device* d, int first, float ratio, float l2, uint64_t out[2], CopyCountStats* st, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    CopyCount* S = (CopyCount*)d->copycount;
    if (!d->s4keep || !S) { err = "copy counts: not prepared"; return SAGE2OV_ERR_INTERNAL; }
    const S4Keep& K = *(S4Keep*)d->s4keep; const u32 nh = K.nh; hipStream_t sm = d->stream;
    DevTmp B; StreamLap lap(sm); HIPCHK(lap.create());
    unsigned long long* ctr = B.get<unsigned long long>(2); if (!ctr) return copycount_nomem(err);
    HIPCHK(lap.start());
    HIPCHK(hipMemsetAsync(ctr, 0, 2 * sizeof(unsigned long long), sm));
    if (nh) hipLaunchKernelGGL(k_cc_round, dim3(grid_for(nh, 256)), dim3(256), 0, sm, K.g, nh, S->kPair, first, ratio, l2, ctr);
    HIPCHK(hipGetLastError());
    unsigned long long hc[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, sm));
    HIPCHK(lap.stop(st->round_ms));
    out[0] = hc[0]; out[1] = hc[1];
    return 0;
}
int dev_flownet_build(Device* d, const CopyCountConst& P, CopyCountStats* st, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    CopyCount* S = (CopyCount*)d->copycount;
    if (!d->s4keep || !S) { err = "flow network: the copy counts are not prepared"; return SAGE2OV_ERR_INTERNAL; }
    S->drop_net();
    const S4Keep& K = *(S4Keep*)d->s4keep; const S4Graph& g = K.g; const u32 nh = K.nh; const u64 nl = K.listUsed; const u32 N = (u32)d->N; hipStream_t sm = d->stream;
    CcConst C; C.ratio = P.ratio; for (int j = 0; j < 21; j++) C.lj[j] = P.lj[j];
    C.l1 = P.l1; C.l3 = P.l3; C.l5 = P.l5; C.l1000 = P.l1000; C.fN1 = P.fN1; C.fN3 = P.fN3; C.fN5 = P.fN5; C.dN3 = P.dN3; C.dN1000 = P.dN1000; C.n = P.n;
    DevTmp B; StreamLap lap(sm); HIPCHK(lap.create());
    const dim3 b256(256);
    // ---- the save order: the halves the writer visits, per node by ascending index
    HIPCHK(lap.start());
    u64 nOrd = 0;
    u32* sel = B.get<u32>(nh); u32* pos = B.get<u32>(nh); u64* partial = B.get<u64>(scan_partial_words((u64)nh + 1));
    if (!sel || !pos || !partial) return copycount_nomem(err);
    if (nh) {
        hipLaunchKernelGGL(k_cc_select, dim3(grid_for(nh, 256)), b256, 0, sm, g, nh, sel);
        const int rc = scan_u32(d, sel, nh, pos, partial, &nOrd, err); if (rc) return rc;
    }
    const u64 F = 2 * nOrd;
    if (F >= (1ull << 32) - RS_TILE) { err = "flow network: more than 2^32 records"; return SAGE2OV_ERR_LIMIT; }
    S->arcs = nullptr;
    if (!F) {                                                                          // no edge: the header arc alone
        S->arcs = (CcArc*)DevTmp::alloc(sizeof(CcArc)); if (!S->arcs) return copycount_nomem(err);
        hipLaunchKernelGGL(k_cc_node_arcs, dim3(1), b256, 0, sm, 0u, S->arcs);
        HIPCHK(hipGetLastError()); HIPCHK(lap.stop(st->order_ms));
        S->nArcs = 1; S->net = true; st->nodes = st->edges = st->simple = st->once = st->many = 0; st->arcs = 1;
        return 0;
    }
    int shifts[4]; const int np = copycount_passes(N, shifts);
    u64* key1 = B.get<u64>(nOrd); u32* half = B.get<u32>(nOrd); if (!key1 || !half) return copycount_nomem(err);
    hipLaunchKernelGGL(k_cc_compact, dim3(grid_for(nh, 256)), b256, 0, sm, g, nh, sel, pos, key1, half);
    u64* ks1 = nullptr; u32* idx1 = nullptr; MateStats ms;
    { const int rc = mate_sort(d, B, key1, (u32)nOrd, shifts, np, &ks1, &idx1, &ms, err); if (rc) return rc; }
    // ---- the records in descending file position, sorted by their start node: the loaded lists
    u64* key2 = B.get<u64>(F); u32* rec = B.get<u32>(F); if (!key2 || !rec) return copycount_nomem(err);
    hipLaunchKernelGGL(k_cc_filekeys, dim3(grid_for(F, 256)), b256, 0, sm, g, half, idx1, (u32)F, key2, rec);
    u64* ks2 = nullptr; u32* idx2 = nullptr;
    { const int rc = mate_sort(d, B, key2, (u32)F, shifts, np, &ks2, &idx2, &ms, err); if (rc) return rc; }
    st->passes = ms.passes;
    S->adj = (u32*)DevTmp::alloc(F * sizeof(u32)); if (!S->adj) return copycount_nomem(err);
    hipLaunchKernelGGL(k_cc_gather, dim3(grid_for(F, 256)), b256, 0, sm, idx2, rec, (u32)F, S->adj);
    u32* hp = nullptr; u32 E = 0;
    { const int rc = mate_heads(d, B, ks2, (u32)F, &hp, &E, err); if (rc) return rc; }
    S->hp = (u32*)DevTmp::alloc(((u64)E + 1) * sizeof(u32)); S->nodeOf = (u32*)DevTmp::alloc(std::max<u64>(E, 1) * sizeof(u32));
    u32* rankOf = B.get<u32>((u64)N + 2);
    if (!S->hp || !S->nodeOf || !rankOf) return copycount_nomem(err);
    HIPCHK(hipMemcpyAsync(S->hp, hp, ((u64)E + 1) * sizeof(u32), hipMemcpyDeviceToDevice, sm));
    hipLaunchKernelGGL(k_cc_ranks, dim3(grid_for(E, 256)), b256, 0, sm, ks2, hp, E, S->nodeOf);
    HIPCHK(hipMemsetAsync(rankOf, 0, ((u64)N + 2) * sizeof(u32), sm));
    hipLaunchKernelGGL(k_cc_rank_of, dim3(grid_for(E, 256)), b256, 0, sm, S->nodeOf, E, rankOf, N);
    HIPCHK(hipGetLastError());
    HIPCHK(lap.stop(st->order_ms));
    S->F = F; S->E = E;
    // ---- classes, arc counts, positions
    HIPCHK(lap.start());
    uint8_t* cls = B.get<uint8_t>(F); uint8_t* lb = B.get<uint8_t>(F); u32* arcs = B.get<u32>(F); u32* apos = B.get<u32>(F); unsigned long long* ctr = B.get<unsigned long long>(4);
    u64* partialF = B.get<u64>(scan_partial_words(F + 1));
    if (!cls || !lb || !arcs || !apos || !ctr || !partialF) return copycount_nomem(err);
    HIPCHK(hipMemsetAsync(ctr, 0, 4 * sizeof(unsigned long long), sm));
    hipLaunchKernelGGL(k_cc_classes, dim3(grid_for(F, 256)), b256, 0, sm, g, S->adj, (u32)F, S->kPair, C, cls, lb, arcs, ctr);
    u64 A = 0; { const int rc = scan_u32(d, arcs, F, apos, partialF, &A, err); if (rc) return rc; }
    unsigned long long hc[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpy(hc, ctr, sizeof hc, hipMemcpyDeviceToHost));
    HIPCHK(lap.stop(st->classes_ms));
    st->nodes = E; st->edges = hc[0]; st->simple = hc[1]; st->once = hc[2]; st->many = hc[3];
    const u64 base = 1 + 6ull * E, total = base + A;
    if (total >= (1ull << 32) - RS_TILE) { err = "flow network: 2^32 - 2048 arcs or more"; S->drop_net(); return SAGE2OV_ERR_LIMIT; }
    // ---- the arc records
    HIPCHK(lap.start());
    S->arcs = (CcArc*)DevTmp::alloc(total * sizeof(CcArc)); if (!S->arcs) { S->drop_net(); return copycount_nomem(err); }
    hipLaunchKernelGGL(k_cc_node_arcs, dim3(grid_for(std::max<u64>(E, 1), 256)), b256, 0, sm, E, S->arcs);
    hipLaunchKernelGGL(k_cc_edge_arcs, dim3((unsigned)std::min<u64>(grid_for(F, 4), CC_ARC_BLOCKS)), b256, 0, sm, g, S->adj, (u32)F, cls, lb, apos, base, rankOf, S->freq, N, nl, C, S->arcs);
    HIPCHK(hipGetLastError());
    HIPCHK(lap.stop(st->arcs_ms));
    S->nArcs = total; S->net = true; st->arcs = total;
    return 0;
}
uint64_t dev_flownet_arcs(Device* d) { const CopyCount* S = (const CopyCount*)d->copycount; return S && S->net ? S->nArcs : 0; }
int dev_flownet_export(Device* d, FlowArc* out, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    const CopyCount* S = (const CopyCount*)d->copycount; if (!S || !S->net) { err = "flow network: not built"; return SAGE2OV_ERR_INTERNAL; }
    HIPCHK(hipMemcpy(out, S->arcs, S->nArcs * sizeof(CcArc), hipMemcpyDeviceToHost));
    return 0;
}
// the lines of a solution onto the flows of the resident graph (the caller has checked every node number against the network); the supports go, as in dev_flow_set.
// dfr, dto, dfl: the lines in device memory
static int flow_apply_lines(Device* d, const u64* dfr, const u64* dto, const u64* dfl, uint64_t n, CopyCountStats* st, std::string& err) {
    const CopyCount* S = (const CopyCount*)d->copycount;
    S4Keep& K = *(S4Keep*)d->s4keep; S4Mem& mem = K.mem; const u32 nh = K.nh; hipStream_t sm = d->stream;
    DevTmp B; StreamLap lap(sm); HIPCHK(lap.create());
    unsigned long long* acc = B.get<unsigned long long>(nh); unsigned long long* ctr = B.get<unsigned long long>(2);
    if (!acc || !ctr) return copycount_nomem(err);
    const bool fresh = !K.flow;
    if (fresh) { S4GET(a, float, nh) K.flow = a; K.flowCap = std::max<u64>(nh, 1); }
    dev_support_release(d); dev_paths_release(d);
    HIPCHK(lap.start());
    if (fresh && nh) HIPCHK(hipMemsetAsync(K.flow, 0, (u64)nh * sizeof(float), sm));
    if (nh) HIPCHK(hipMemsetAsync(acc, 0, (u64)nh * sizeof(unsigned long long), sm));
    HIPCHK(hipMemsetAsync(ctr, 0, 2 * sizeof(unsigned long long), sm));
    if (n && S->F) hipLaunchKernelGGL(k_cc_apply, dim3(grid_for(n, 256)), dim3(256), 0, sm, K.g, S->adj, S->hp, S->nodeOf, (u32)S->E, dfr, dto, dfl, (u64)n, acc, ctr);
    if (nh) hipLaunchKernelGGL(k_cc_average, dim3(grid_for((u64)nh / 2 + 1, 256)), dim3(256), 0, sm, K.g, nh, acc, K.flow, ctr);
    HIPCHK(hipGetLastError());
    unsigned long long hc[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, sm));
    HIPCHK(lap.stop(st->apply_ms));
    st->applied = hc[0]; st->different = hc[1];
    return 0;
}
int dev_flow_apply(Device* d, const uint64_t* from, const uint64_t* to, const uint64_t* flow, uint64_t n, CopyCountStats* st, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    const CopyCount* S = (const CopyCount*)d->copycount;
    if (!d->s4keep || !S || !S->net) { err = "flow solution: no flow network"; return SAGE2OV_ERR_INTERNAL; }
    DevTmp B; hipStream_t sm = d->stream;
    u64* dfr = B.get<u64>(n); u64* dto = B.get<u64>(n); u64* dfl = B.get<u64>(n);
    if (!dfr || !dto || !dfl) return copycount_nomem(err);
    if (n) {
        HIPCHK(hipMemcpyAsync(dfr, from, n * sizeof(u64), hipMemcpyHostToDevice, sm)); HIPCHK(hipMemcpyAsync(dto, to, n * sizeof(u64), hipMemcpyHostToDevice, sm));
        HIPCHK(hipMemcpyAsync(dfl, flow, n * sizeof(u64), hipMemcpyHostToDevice, sm));
    }
    return flow_apply_lines(d, dfr, dto, dfl, n, st, err);
}
int dev_flow_get(Device* d, float* flow, uint64_t n, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    if (!d->s4keep) { err = "flows: no step-4 graph on the device"; return SAGE2OV_ERR_ARG; }
    const S4Keep& K = *(S4Keep*)d->s4keep;
    if (n != K.nh) { err = "flows: one value per half-edge"; return SAGE2OV_ERR_INTERNAL; }
    if (!K.flow) { std::fill(flow, flow + n, 0.f); return 0; }
    if (n) HIPCHK(hipMemcpy(flow, K.flow, n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// =============================================================================================
// step 5's solver (kernels_flow.inc; main_cs2, copycountEstimator.cpp:359)
// =============================================================================================
static int mcf_nomem(std::string& err) { err = "min-cost flow: out of device memory"; return SAGE2OV_ERR_NOMEM; }
// the epsilon of every phase, and whether the lowest price the phases can reach -- with room for one reduced cost -- stays inside +-2^62 (P = long long) or
// +-2^126 (P = __int128).  Nothing here wraps in 128 unsigned bits: scale < 2^32 and maxc <= 2^63, so cmax < 2^95; cmax is then held against lim / ((1 + alpha) *
// scale) before the first product, so that every term (1 + alpha) * scale * e, e <= cmax, is at most lim <= 2^126; the sum is below lim before a term is added, so
// below 2^127 after it; and floor + 2 cmax + 1 < 2^126 + 2^96 + 1.
template <class P> static bool mcf_phases(u64 scale, u64 maxc, P* cmaxOut, std::vector<P>& eps) {
    const unsigned __int128 lim = (unsigned __int128)mf_inf<P>(), step = (unsigned __int128)(1 + MF_ALPHA) * scale;
    unsigned __int128 cmax = (unsigned __int128)scale * maxc; if (cmax < 1) cmax = 1;
    if (cmax >= lim || cmax > lim / step) return false;                                // (beyond lim / step the first term alone passes lim)
    unsigned __int128 floor = 0;
    for (P e = (P)cmax;;) { eps.push_back(e); floor += step * (unsigned __int128)e; if (floor >= lim) return false; if (e == 1) break; e = std::max<P>(1, e / MF_ALPHA); }
    if (floor + 2 * cmax + 1 >= lim) return false;
    *cmaxOut = (P)cmax;
    return true;
}
bool mcf_wide_guard(uint64_t n, uint64_t maxc) { i128 c; std::vector<i128> e; return mcf_phases<i128>(n + 1, maxc, &c, e); }
static int mcf_flag_error(unsigned long long flags, std::string& err) {
    if (flags & MF_F_NAN) { err = "min-cost flow: a cost that is no number"; return SAGE2OV_ERR_ARG; }
    if (flags & MF_F_BADARC) { err = "min-cost flow: a bad arc (from == to, a node number outside 1..n, lower > upper or a negative bound)"; return SAGE2OV_ERR_ARG; }
    if (flags & MF_F_RANGE) { err = "min-cost flow: costs and prices beyond the range of the method's integers"; return SAGE2OV_ERR_LIMIT; }
    if (flags & MF_F_INFEASIBLE) { err = "min-cost flow: the network is infeasible (excess that no residual path can carry to a deficit)"; return SAGE2OV_ERR_ARG; }
    if (flags & MF_F_LIMIT) { err = "min-cost flow: the round budget is spent"; return SAGE2OV_ERR_LIMIT; }
    return 0;
}
// dArcs: m records in device memory.  On success *flowOut (m words) and *priceOut (n + 2 words, node v at word v) are allocations the caller frees; on any
// error nothing is handed out.  st is filled as far as the solve got.  P: the price type (kernels_flow.inc); *range: the failure was P's range -- the guard before
// the layout or the one before a price update -- and nothing else.
template <class P> static int mcf_solve_device(Device* d, const McfArc* dArcs, u64 m, u32 n, u64 maxRounds, long long** flowOut, P** priceOut, McfStats* st, bool* range, std::string& err) {
    constexpr bool wide = sizeof(P) == 16;
    *flowOut = nullptr; *priceOut = nullptr; *range = false; *st = McfStats(); st->priceWords = wide ? 2 : 1;
    if (m >= (1ull << 31) - RS_TILE) { err = "min-cost flow: 2^31 - 2048 arcs or more"; return SAGE2OV_ERR_LIMIT; }
    if (n >= 0xFFFFFFF0u) { err = "min-cost flow: too many nodes"; return SAGE2OV_ERR_LIMIT; }
    if (!maxRounds) maxRounds = SAGE2OV_MCF_DEFAULT_ROUNDS;
    hipStream_t sm = d->stream; const dim3 b256(256); const u32 M = (u32)(2 * m); const u64 scale = (u64)n + 1;
    st->nodes = n; st->arcs = m; st->scale = scale;
    DevTmp B; StreamLap lap(sm); HIPCHK(lap.create());
    unsigned long long* ctr = B.get<unsigned long long>(MF_CTRS); if (!ctr) return mcf_nomem(err);
    unsigned long long hc[MF_CTRS];
    HIPCHK(lap.start());
    HIPCHK(hipMemsetAsync(ctr, 0, MF_CTRS * sizeof(unsigned long long), sm));
    if (m) hipLaunchKernelGGL(k_mf_check, dim3(grid_for(m, 256)), b256, 0, sm, dArcs, m, n, ctr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, sm)); HIPCHK(hipStreamSynchronize(sm));
    { const int rc = mcf_flag_error(hc[MF_FLAGS], err); if (rc) return rc; }
    P cmax = 1; std::vector<P> epsList;
    if (!mcf_phases<P>(scale, hc[MF_MAXC], &cmax, epsList)) {
        *range = true; err = wide ? "min-cost flow: (n + 1) * max |cost| and the price range of the method do not fit 128 bits" : "min-cost flow: (n + 1) * max |cost| and the price range of the method do not fit 64 bits";
        return SAGE2OV_ERR_LIMIT;
    }
    // ---- the layout
    long long* excess = B.get<long long>((u64)n + 2); long long* delta = B.get<long long>((u64)n + 2); long long* dist = B.get<long long>((u64)n + 2);
    P* price[2] = {(P*)DevTmp::alloc(((u64)n + 2) * sizeof(P)), B.get<P>((u64)n + 2)};                      // (device allocations are aligned to 256 bytes: a 128-bit price is one load)
    struct Free { void* p; ~Free() { hipFree(p); } } fp0{price[0]};                   // handed out on success only
    long long* flow = (long long*)DevTmp::alloc(std::max<u64>(m, 1) * sizeof(long long)); Free ff{flow};
    u32* head = B.get<u32>(M); u32* sis = B.get<u32>(M); u32* tail = B.get<u32>(M); u32* start = B.get<u32>((u64)n + 3); u32* pos = B.get<u32>(M);
    long long* cost = B.get<long long>(M); int* rcap = B.get<int>(M); u64* key = B.get<u64>(M);
    if (!excess || !delta || !dist || !price[0] || !price[1] || !flow || !head || !sis || !tail || !start || !pos || !cost || !rcap || !key) return mcf_nomem(err);
    HIPCHK(hipMemsetAsync(excess, 0, ((u64)n + 2) * sizeof(long long), sm)); HIPCHK(hipMemsetAsync(delta, 0, ((u64)n + 2) * sizeof(long long), sm));
    HIPCHK(hipMemsetAsync(price[0], 0, ((u64)n + 2) * sizeof(P), sm)); HIPCHK(hipMemsetAsync(price[1], 0, ((u64)n + 2) * sizeof(P), sm));
    if (m) {
        hipLaunchKernelGGL(k_mf_keys, dim3(grid_for(m, 256)), b256, 0, sm, dArcs, m, key, excess);
        int shifts[4]; const int np = copycount_passes(n, shifts);
        u64* ks = nullptr; u32* idx = nullptr; MateStats ms;
        { const int rc = mate_sort(d, B, key, M, shifts, np, &ks, &idx, &ms, err); if (rc) return rc; }
        hipLaunchKernelGGL(k_mf_pos, dim3(grid_for(M, 256)), b256, 0, sm, idx, M, pos);
        hipLaunchKernelGGL(k_mf_entries, dim3(grid_for(M, 256)), b256, 0, sm, dArcs, idx, pos, ks, M, wide ? 1ll : (long long)scale, head, sis, tail, cost, rcap);      // (128-bit prices: the entries keep the unscaled cost)
        hipLaunchKernelGGL(k_mf_starts, dim3(grid_for((u64)n + 2, 256)), b256, 0, sm, ks, M, n, start);
    } else HIPCHK(hipMemsetAsync(start, 0, ((u64)n + 3) * sizeof(u32), sm));
    // (SAGE2OV_TEST_MCF_LDS=0: tests only -- a network that fits the single-workgroup form takes the launches all the same)
    bool lds = false;
    if constexpr (!wide) lds = m && n <= MF_LDS_NODES && M <= MF_LDS_ENTRIES && d->opt.num("SAGE2OV_TEST_MCF_LDS", 1) != 0;
    st->form = lds ? SAGE2OV_MCF_FORM_LDS : SAGE2OV_MCF_FORM_LAUNCHES;
    // the hub form (the launches only): lists longer than hubDeg.  SAGE2OV_TEST_MCF_HUB_DEG (tests only): 0 off, d >= 64 the threshold (below 64 a lane walks the list)
    u32 hubDeg = 0;
    if (!lds && m) { const long long v = d->opt.num("SAGE2OV_TEST_MCF_HUB_DEG", SAGE2OV_MCF_HUB_DEG); hubDeg = v <= 0 ? 0 : (u32)std::min<long long>(std::max<long long>(v, MF_LANE_DEG), MF_NO_HUBS - 1); }
    st->hub[0] = hubDeg; st->hub[1] = MF_HUB_TILE;
    unsigned long long hubCounts[2] = {0, 0};
    if (hubDeg) {                                                                       // the two counts come back with the layout's own synchronisation
        hipLaunchKernelGGL(k_mf_hub_count, dim3(grid_for(n, 256)), b256, 0, sm, (const u32*)start, n, hubDeg, ctr);
        HIPCHK(hipMemcpyAsync(hubCounts, ctr + MF_HUBS, sizeof hubCounts, hipMemcpyDeviceToHost, sm));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(lap.stop(st->build_ms));
    const MfNet N = {head, sis, tail, start, cost, rcap, excess, delta, n, M, (long long)scale};
    const u32 nodeGrid = grid_for(n, MF_BLOCK), entryGrid = grid_for(M, 256);
    // the tables of the hubs, when there are any: ranks by the project's scan, so ascending node number and the same tables on every run
    MfHubs Hb = {}; P* tbest = nullptr; u32* tadm = nullptr;
    if (hubCounts[0]) {
        const u32 H = (u32)hubCounts[0], T = (u32)hubCounts[1];
        HIPCHK(lap.start());
        u32* isHub = B.get<u32>(n); u32* nTiles = B.get<u32>(n); u32* rank = B.get<u32>(n); u32* tileRank = B.get<u32>(n); u64* partial = B.get<u64>(scan_partial_words(n));
        u32* hnode = B.get<u32>(H); u32* tile0 = B.get<u32>((u64)H + 1); u32* tileHub = B.get<u32>(T); u32* tileBeg = B.get<u32>(T);
        long long* snap = B.get<long long>(H); long long* tsum = B.get<long long>(T); tbest = B.get<P>(T); tadm = B.get<u32>(T);
        if (!isHub || !nTiles || !rank || !tileRank || !partial || !hnode || !tile0 || !tileHub || !tileBeg || !snap || !tsum || !tbest || !tadm) return mcf_nomem(err);
        hipLaunchKernelGGL(k_mf_hub_mark, dim3(grid_for(n, 256)), b256, 0, sm, (const u32*)start, n, hubDeg, isHub, nTiles);
        { const int rc = scan_u32(d, isHub, n, rank, partial, nullptr, err); if (rc) return rc; }
        { const int rc = scan_u32(d, nTiles, n, tileRank, partial, nullptr, err); if (rc) return rc; }
        hipLaunchKernelGGL(k_mf_hub_tables, dim3(grid_for(n, 256)), b256, 0, sm, (const u32*)start, n, hubDeg, (const u32*)rank, (const u32*)tileRank, H, T, hnode, tile0, tileHub, tileBeg);
        HIPCHK(hipGetLastError());
        HIPCHK(lap.stop(st->build_ms));
        Hb = MfHubs{hnode, tile0, tileHub, tileBeg, snap, tsum, H, T};
        st->hub[2] = H; st->hub[3] = T;
    }
    const u32 roundHubDeg = hubDeg ? hubDeg : MF_NO_HUBS;
    u32 cur = 0; unsigned long long flags = 0;
    HIPCHK(lap.start());
    if constexpr (!wide) if (lds) {
        const MfLdsArgs A = {cmax, (long long)scale, maxRounds, MF_PERIOD};
        hipLaunchKernelGGL(k_mf_lds, dim3(1), dim3(MF_BLOCK), 0, sm, N, price[0], A, ctr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, sm)); HIPCHK(hipStreamSynchronize(sm));
        st->phases = hc[MF_PHASES]; st->rounds = hc[MF_ROUNDS]; st->pushes = hc[MF_PUSHES]; st->relabels = hc[MF_RELABELS]; st->updates = hc[MF_UPDATES]; flags = hc[MF_FLAGS];
    }
    if (!lds && m) {
        const long long cap = (long long)(1 + MF_ALPHA) * (long long)scale;
        P floor = 0; u64 rounds = 0, updates = 0;
        hipEvent_t e0 = nullptr, e1 = nullptr; HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
        struct Ev { hipEvent_t a, b; ~Ev() { hipEventDestroy(a); hipEventDestroy(b); } } evs{e0, e1};
        for (size_t ph = 0; ph < epsList.size() && !flags; ph++) {
            const P eps = epsList[ph], capEps = (P)cap * eps;                           // (below the bound: mcf_phases)
            floor -= capEps; st->phases++;
            const u64 r0 = rounds;
            HIPCHK(hipEventRecord(e0, sm));
            hipLaunchKernelGGL(k_mf_saturate<P>, dim3(entryGrid), b256, 0, sm, N, (const P*)price[cur]);
            u64 since = MF_PERIOD;
            for (bool done = false; !done && !flags;) {
                const u64 left = maxRounds - rounds;
                if (!left) { flags |= MF_F_LIMIT; break; }
                if (since >= MF_PERIOD) {                                               // the price update: relax until a launch improves nothing
                    since = 0; floor -= capEps;                                         // (the floor was above -bound, capEps is below bound: no wrap)
                    if (floor < -(mf_inf<P>() - 2 * cmax - 1)) { flags |= MF_F_RANGE; *range = true; break; }
                    hipLaunchKernelGGL(k_mf_pu_init, dim3(grid_for((u64)n + 2, 256)), b256, 0, sm, excess, n, dist);
                    bool settled = false;
                    for (u64 it = 0; it <= (u64)n + MF_BATCH && !settled; it += MF_BATCH) {      // (a shortest path has at most n - 1 entries)
                        HIPCHK(hipMemsetAsync(ctr + MF_ACT, 0, MF_BATCH * sizeof(unsigned long long), sm));
                        for (u32 k = 0; k < MF_BATCH; k++) hipLaunchKernelGGL(k_mf_pu_relax<P>, dim3(entryGrid), b256, 0, sm, N, (const P*)price[cur], eps, capEps, cap, dist, ctr + MF_ACT + k);
                        HIPCHK(hipGetLastError());
                        HIPCHK(hipMemcpyAsync(hc, ctr, MF_BATCH * sizeof(unsigned long long), hipMemcpyDeviceToHost, sm)); HIPCHK(hipStreamSynchronize(sm));
                        for (u32 k = 0; k < MF_BATCH; k++) if (!hc[MF_ACT + k]) settled = true;
                    }
                    if (!settled) { err = "min-cost flow: the price update did not settle"; return SAGE2OV_ERR_INTERNAL; }
                    hipLaunchKernelGGL(k_mf_pu_apply<P>, dim3(grid_for((u64)n + 1, 256)), b256, 0, sm, (const long long*)excess, (const long long*)dist, n, eps, cap, price[cur], ctr);
                    updates++;
                }
                const u32 K = (u32)std::min<u64>(MF_BATCH, left);
                HIPCHK(hipMemsetAsync(ctr + MF_ACT, 0, MF_BATCH * sizeof(unsigned long long), sm));
                for (u32 k = 0; k < K; k++) {
                    hipLaunchKernelGGL(k_mf_push<P>, dim3(nodeGrid), dim3(MF_BLOCK), 0, sm, N, (const P*)price[cur], roundHubDeg, ctr);
                    if (Hb.H) {
                        hipLaunchKernelGGL(k_mf_hub_sum<P>, dim3(Hb.T), dim3(MF_BLOCK), 0, sm, N, Hb, (const P*)price[cur]);
                        hipLaunchKernelGGL(k_mf_hub_push<P>, dim3(Hb.T), dim3(MF_BLOCK), 0, sm, N, Hb, (const P*)price[cur], ctr);
                    }
                    hipLaunchKernelGGL(k_mf_relabel<P>, dim3(nodeGrid), dim3(MF_BLOCK), 0, sm, N, (const P*)price[cur], price[cur ^ 1u], eps, floor, roundHubDeg, ctr + MF_ACT + k, ctr);
                    if (Hb.H) {
                        hipLaunchKernelGGL(k_mf_hub_rel<P>, dim3(Hb.T), dim3(MF_BLOCK), 0, sm, N, Hb, (const P*)price[cur], eps, tbest, tadm);
                        hipLaunchKernelGGL(k_mf_hub_rel_fin<P>, dim3(Hb.H), dim3(MF_BLOCK), 0, sm, N, Hb, (const P*)tbest, (const u32*)tadm, floor, price[cur ^ 1u], ctr);
                    }
                    cur ^= 1u;
                }
                HIPCHK(hipGetLastError());
                HIPCHK(hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, sm)); HIPCHK(hipStreamSynchronize(sm));
                flags |= hc[MF_FLAGS];
                u32 used = K;
                for (u32 k = 0; k < K; k++) if (!hc[MF_ACT + k]) { used = k + 1; done = true; break; }      // (the rounds behind it found nothing to do)
                rounds += used; since += used;
            }
            HIPCHK(hipEventRecord(e1, sm)); HIPCHK(hipEventSynchronize(e1));
            if (ph < SAGE2OV_MCF_PHASES) { float t = 0; hipEventElapsedTime(&t, e0, e1); st->refine_ms[ph] = t; st->refine_rounds[ph] = rounds - r0; }
            st->rounds = rounds; st->updates = updates; st->pushes = hc[MF_PUSHES]; st->relabels = hc[MF_RELABELS];
            st->hub[4] = hc[MF_HUB_PUSHES]; st->hub[5] = hc[MF_HUB_RELABELS];
        }
    }
    HIPCHK(lap.stop(st->solve_ms));
    { const int rc = mcf_flag_error(flags, err); if (rc) return rc; }
    if (m) hipLaunchKernelGGL(k_mf_flows, dim3(grid_for(m, 256)), b256, 0, sm, dArcs, pos, rcap, m, flow);
    HIPCHK(hipGetLastError());
    if (cur == 1) HIPCHK(hipMemcpyAsync(price[0], price[1], ((u64)n + 2) * sizeof(P), hipMemcpyDeviceToDevice, sm));
    HIPCHK(hipStreamSynchronize(sm));
    *flowOut = flow; *priceOut = price[0]; ff.p = nullptr; fp0.p = nullptr;
    return 0;
}
// price: n words, or 2 n with wide (a node's low word first), or null
int dev_mcf_solve(Device* d, const void* arcs, uint64_t m, uint32_t n, uint64_t maxRounds, bool wide, int64_t* flow, void* price, McfStats* st, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    static_assert(sizeof(McfArc) == 24, "an arc is 24 bytes");
    DevTmp B; McfArc* dA = B.get<McfArc>(m); if (!dA) return mcf_nomem(err);
    if (m) HIPCHK(hipMemcpyAsync(dA, arcs, m * sizeof(McfArc), hipMemcpyHostToDevice, d->stream));
    long long* dF = nullptr; void* dP = nullptr; bool range = false; const size_t w = wide ? sizeof(i128) : sizeof(long long);
    if (wide) { i128* q = nullptr; const int rc = mcf_solve_device<i128>(d, dA, m, n, maxRounds, &dF, &q, st, &range, err); if (rc) return rc; dP = q; }
    else { long long* q = nullptr; const int rc = mcf_solve_device<long long>(d, dA, m, n, maxRounds, &dF, &q, st, &range, err); if (rc) return rc; dP = q; }
    hipError_t e = hipSuccess;
    if (m) e = hipMemcpy(flow, dF, m * sizeof(long long), hipMemcpyDeviceToHost);
    if (e == hipSuccess && price && n) e = hipMemcpy(price, (const char*)dP + w, (u64)n * w, hipMemcpyDeviceToHost);
    hipFree(dF); hipFree(dP);
    HIPCHK(e);
    return 0;
}
// the resident network of dev_flownet_build; the earlier solution stays unless this one succeeds.  64-bit prices where their guard admits the network, 128-bit ones
// where it does not, and from the start again where a 64-bit solve met the guard on the way (nothing was applied; the statistics are the second solve's).
// SAGE2OV_TEST_MCF_WIDE (tests only): 0 never wide, 1 always
int dev_flow_solve(Device* d, uint64_t maxRounds, McfStats* st, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    CopyCount* S = (CopyCount*)d->copycount;
    if (!d->s4keep || !S || !S->net) { err = "flow solve: no flow network"; return SAGE2OV_ERR_ARG; }
    const u64 m = S->nArcs; const u64 nn = 4 * S->E + 2;
    DevTmp B; McfArc* dA = B.get<McfArc>(m); unsigned long long* ctr = B.get<unsigned long long>(MF_CTRS); if (!dA || !ctr) return mcf_nomem(err);
    HIPCHK(hipMemsetAsync(ctr, 0, MF_CTRS * sizeof(unsigned long long), d->stream));
    hipLaunchKernelGGL(k_mf_from_cc, dim3(grid_for(m, 256)), dim3(256), 0, d->stream, S->arcs, m, dA, ctr);
    HIPCHK(hipGetLastError());
    unsigned long long fl = 0; HIPCHK(hipMemcpyAsync(&fl, ctr + MF_FLAGS, sizeof fl, hipMemcpyDeviceToHost, d->stream)); HIPCHK(hipStreamSynchronize(d->stream));
    { const int rc = mcf_flag_error(fl, err); if (rc) return rc; }
    const long long mode = d->opt.num("SAGE2OV_TEST_MCF_WIDE", -1);
    long long* dF = nullptr; void* dP = nullptr; u32 words = 1; bool range = false; int rc = 0;
    if (mode != 1) { long long* q = nullptr; rc = mcf_solve_device<long long>(d, dA, m, (u32)nn, maxRounds, &dF, &q, st, &range, err); dP = q; }
    if (mode == 1 || (rc && range && mode != 0)) { i128* q = nullptr; words = 2; rc = mcf_solve_device<i128>(d, dA, m, (u32)nn, maxRounds, &dF, &q, st, &range, err); dP = q; }
    if (rc) return rc;
    S->drop_solution(); S->solFlow = dF; S->solPrice = dP; S->solWords = words; S->solScale = nn + 1; S->solved = true;
    return 0;
}
bool dev_flow_solved(Device* d) { const CopyCount* S = (const CopyCount*)d->copycount; return S && S->net && S->solved; }
uint32_t dev_flow_price_words(Device* d) { const CopyCount* S = (const CopyCount*)d->copycount; return S && S->net && S->solved ? S->solWords : 0; }
// flow: one word per arc; price: dev_flow_price_words() words per network node (either may be null)
int dev_flow_solution_get(Device* d, int64_t* flow, void* price, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    const CopyCount* S = (const CopyCount*)d->copycount; if (!S || !S->net || !S->solved) { err = "flow solution: none"; return SAGE2OV_ERR_ARG; }
    if (flow) HIPCHK(hipMemcpy(flow, S->solFlow, S->nArcs * sizeof(long long), hipMemcpyDeviceToHost));
    const size_t w = S->solWords * sizeof(long long);
    if (price) HIPCHK(hipMemcpy(price, (const char*)S->solPrice + w, (4 * S->E + 2) * w, hipMemcpyDeviceToHost));
    return 0;
}
// the resident flows through k_cc_apply / k_cc_average: the lines are made on the device and never leave it.  *tts: the flow of the `2 1` arc
int dev_flow_commit(Device* d, CopyCountStats* st, uint64_t* tts, uint64_t* lines, std::string& err) {
    HIPCHK(hipSetDevice(d->ordinal));
    const CopyCount* S = (const CopyCount*)d->copycount;
    if (!d->s4keep || !S || !S->net || !S->solved) { err = "flow commit: no solution of the present network"; return SAGE2OV_ERR_ARG; }
    const u64 m = S->nArcs; hipStream_t sm = d->stream;
    DevTmp B; McfArc* dA = B.get<McfArc>(m); u64* dfr = B.get<u64>(m); u64* dto = B.get<u64>(m); u64* dfl = B.get<u64>(m); unsigned long long* ctr = B.get<unsigned long long>(MF_CTRS);
    if (!dA || !dfr || !dto || !dfl || !ctr) return mcf_nomem(err);
    HIPCHK(hipMemsetAsync(ctr, 0, MF_CTRS * sizeof(unsigned long long), sm));
    hipLaunchKernelGGL(k_mf_from_cc, dim3(grid_for(m, 256)), dim3(256), 0, sm, S->arcs, m, dA, ctr);
    hipLaunchKernelGGL(k_mf_triples, dim3(grid_for(m, 256)), dim3(256), 0, sm, dA, S->solFlow, m, dfr, dto, dfl, ctr);
    HIPCHK(hipGetLastError());
    unsigned long long t = 0; HIPCHK(hipMemcpyAsync(&t, ctr + MF_TTS, sizeof t, hipMemcpyDeviceToHost, sm)); HIPCHK(hipStreamSynchronize(sm));
    *tts = t; *lines = m;
    return flow_apply_lines(d, dfr, dto, dfl, m, st, err);
}

}  // namespace s2
