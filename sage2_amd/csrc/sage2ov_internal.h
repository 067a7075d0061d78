// sage2_amd/csrc/sage2ov_internal.h -- interface between the host side (sage2ov_host.cpp, g++)
// and the device side (sage2ov_device.hip, hipcc).  Plain C++ structs, no HIP types leak out.
#pragma once
#include <cstdint>
#include "sage2ov.h"
#include <sys/mman.h>
#include <algorithm>
#include <cstdlib>
#include <new>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace s2 {

// ----------------------------------------------------------------------------------------------
// HBM layout of the read store
//   reads: (N+1) slots of S u64 words (S = 4, 8, 16 or 32: a power of two so a read never straddles a
//   64-byte sector boundary more than its size requires).  Base p of a read lives in word p/32 at
//   bits 63-2(p%32)..62-2(p%32) (A0 C1 G2 T3): the byte-swapped image of the reference's MSB-first
//   byte packing (utils.cpp:96), so unsigned word compare == the reference's byte compare.
//   The read length sits in the low 9 bits of the slot's last word (SLOT_LEN_MASK 0x1FF; bases never reach
//   there: S is chosen with 2*maxL + 9 <= 64*S; the 32-word layout, 505..1018 bases, keeps 11 bits: slot_len_mask(S)).
//   Slot 0 is all zero (ids are 1-based).
// Index slot (8 bytes):  tag:24 | cnt:7 | payload:33
//   0 = empty; cnt 1 -> payload is the single entry id*4+type; 2..99 -> payload = offset into csr[];
//   127 -> long bucket (>= 100 entries, hashTable.cpp:111-123): never matches a lookup.
// ----------------------------------------------------------------------------------------------
constexpr uint64_t SLOT_TAG_SHIFT = 40;
constexpr uint64_t SLOT_CNT_SHIFT = 33;
constexpr uint64_t SLOT_PAY_MASK = (1ull << 33) - 1;
constexpr uint32_t SLOT_CNT_LONG = 127;
constexpr uint32_t HASH_THRESHOLD = 100;   // hashTable.cpp:76
constexpr uint32_t CONN_LIMIT = 300;       // economyGraph.cpp:43

struct EdgeCand { uint32_t from, to; uint32_t len; uint32_t type; };   // from < to, len already 20-bit masked
// a verified directional hit of an unresolved read (economyGraph.cpp:591-633).  16 bytes, one aligned 16-byte access (20 with a byte-sized type until round 4: the hit
// lists of noisy data are 450 M entries that the probe kernel writes and two kernels of the reduce phase stream); seq: the hit's number among its read's hits
struct alignas(16) Hit { uint32_t from; uint32_t to; int32_t len; uint32_t seq : 30; uint32_t type : 2; };
static_assert(sizeof(Hit) == 16, "Hit: 16 bytes");
struct FinalEdge { uint32_t from, to, len, len_twin; uint32_t type; };

struct DevTimings { double index_ms = 0, probe_ms = 0, reciprocal_ms = 0, hits_ms = 0, convert_ms = 0, probe_kernel_ms = 0, organize_ms = 0, recip_cond_ms = 0, marks_ms = 0; uint64_t probe_launches = 0, slow_reads = 0, probe_fast_launches = 0; };

// ----------------------------------------------------------------------------------------------
// Every switch the library takes from the environment (SAGE2OV_*; INTEGRATION.md lists them with their class: T = test-only override of a decision the library
// otherwise makes by itself -- every route is exact, the tests force each --, G = grid / tuning sweep, D = diagnostic), read ONCE when a context is created:
// Options::from_env snapshots the SAGE2OV_* variables that are set, the context and its device carry the snapshot, and nothing on the timed path calls getenv
// (round 3 had ~60 getenv calls, several per step).  sage2ov_options_reload(ctx) takes a new snapshot (tests that change a switch between two steps of one context).
struct Options {
    std::vector<std::pair<std::string, std::string>> kv;                 // the variables that are set, sorted by name (a handful at most)
    static Options from_env();
    const char* get(const char* name) const {                            // like getenv: the value, or nullptr
        for (const auto& e : kv) if (e.first == name) return e.second.c_str();
        return nullptr;
    }
    bool flag(const char* name) const { return get(name) != nullptr; }
    long long num(const char* name, long long dflt) const { const char* v = get(name); return v ? strtoll(v, nullptr, 10) : dflt; }
};
// the exploration order of the ranked reduce (sage2ov_walk.cpp, host code): rank[position] for the unresolved reads whose potential lists are `lists` / `lenp`
void explore_order(const Options& O, const std::vector<uint32_t>& pos, const std::vector<const uint32_t*>& lists, const std::vector<uint32_t>& lenp, const std::vector<uint8_t>& hasCand,
                   unsigned long long N, const std::vector<uint32_t>& startOrder, std::vector<uint32_t>& rank);


struct Device;   // opaque, lives in sage2ov_device.hip

// every function returns 0 on success, else a negative SAGE2OV_ERR_* and fills err
Device* dev_create(int device_ordinal, const Options& opt, std::string& err);
void dev_set_options(Device* d, const Options& opt);
void dev_destroy(Device* d);
void* dev_stream(Device* d);

int dev_upload_reads(Device* d, const uint64_t* words, uint64_t N, int S, int minL, int maxL, int k, std::string& err);
int dev_build_index(Device* d, uint64_t* slots, uint64_t* keys, uint64_t* csr, uint64_t* nlong, uint32_t* rebuilds, std::string& err);
int dev_lookup(Device* d, uint64_t hi, uint64_t lo, uint64_t* entries, uint32_t cap, uint32_t* count, std::string& err);
// probe+verify+extension kernel over ids [lo, hi)
int dev_probe(Device* d, uint64_t lo, uint64_t hi, std::string& err);
// run mode of the last dev_probe: {reads answered off the ring, steps, of those reads: records with a lane per read, such steps}
int dev_probe_run_stats(Device* d, uint64_t out[4], std::string& err);
// multi-GPU record exchange: 24 bytes per read {right u64, left u64, conn u32, cflag u32}
int dev_export_records(Device* d, void* dev_dst, uint64_t lo, uint64_t hi, std::string& err);
int dev_import_records(Device* d, const void* dev_src, uint64_t first, uint64_t n, std::string& err);
// reciprocal pass (economyGraph.cpp:455-480) over all reads -> status[], edge candidates on device
// cond() for every read; edge candidates are emitted only for reads in [emit_lo, emit_hi)
int dev_reciprocal(Device* d, uint64_t emit_lo, uint64_t emit_hi, uint64_t* n_ov, uint64_t* contained, uint64_t* contained_size, std::string& err);
int dev_export_flags(Device* d, void* dev_dst, std::string& err);      // 2*(N+1) bytes
int dev_import_flags(Device* d, const void* dev_src, std::string& err);
uint64_t dev_cand_count(Device* d);
int dev_export_cands(Device* d, void* dev_dst, uint64_t cap, std::string& err);   // 16 bytes per candidate
int dev_set_cands(Device* d, const void* dev_src, uint64_t n, std::string& err);
bool dev_has_minimiser_groups(Device* d);
void dev_set_probe_share(Device* d, double share);    // share of the reads this context probes (1 / world): decides whether the minimiser groups pay
int dev_download_initial(Device* d, uint64_t* right, uint64_t* left, uint8_t* status, uint32_t* conn, std::string& err);
// directional hit lists of status-0 reads (economyGraph.cpp:591-633), sorted by (from, seq)
int dev_unresolved_hits(Device* d, std::vector<Hit>& hits, uint64_t* n_unresolved, std::string& err, std::vector<uint32_t>* ids_out = nullptr);   // ids_out: the unresolved ids, ascending
int dev_download_status(Device* d, std::vector<uint8_t>& status, std::string& err);
int dev_unresolved_ids(Device* d, std::vector<uint32_t>& ids, std::string& err);          // ascending
int dev_collect_reduce_edges(Device* d, const std::vector<uint32_t>& unresolved, std::vector<EdgeCand>& out, std::string& err);
// host arrays of hundreds of MB that are overwritten right after they are sized: resize() must not write zeros through them on one thread
// -- and from 32 MB on they ask for 2 MB pages (transparent huge pages in `madvise` mode): 512 times fewer page faults on first touch and on release
template <class T> struct NoInitAlloc : std::allocator<T> {
    template <class U> struct rebind { using other = NoInitAlloc<U>; };
    NoInitAlloc() = default; template <class U> NoInitAlloc(const NoInitAlloc<U>&) {}
    T* allocate(size_t n) {
        const size_t bytes = n * sizeof(T);
        if (bytes < (32u << 20)) { void* p = malloc(bytes ? bytes : 1); if (!p) throw std::bad_alloc(); return (T*)p; }
        void* p = nullptr; if (posix_memalign(&p, 2u << 20, (bytes + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1)) != 0) throw std::bad_alloc();
        madvise(p, bytes, MADV_HUGEPAGE);
        return (T*)p;
    }
    void deallocate(T* p, size_t) { free(p); }
    template <class U, class... A> void construct(U* p, A&&... a) { if constexpr (sizeof...(A) == 0) ::new ((void*)p) U; else ::new ((void*)p) U(std::forward<A>(a)...); }
};
using RawU64 = std::vector<uint64_t, NoInitAlloc<uint64_t>>;
using RawU16 = std::vector<uint16_t, NoInitAlloc<uint16_t>>;
// first touch of a freshly sized array by `nt` threads (a copy into it on one thread would take its page faults one by one); the content is about to be overwritten
inline void touch_pages(void* p, size_t bytes, int nt) {
    if (bytes < (64u << 20) || nt < 2) return;
    std::vector<std::thread> th; const size_t per = (bytes / nt + 4095) & ~(size_t)4095;
    for (int t = 0; t < nt; t++) th.emplace_back([=] { char* b = (char*)p; const size_t a = per * t, e = std::min(bytes, a + per); for (size_t x = a; x < e; x += 4096) b[x] = 0; });
    for (auto& x : th) x.join();
}
// ASCII input of step 1 (sage2ov_reads_add_ascii): raw bases + offsets in, filter / pack / canonical orientation on the device; the counters come back
struct OrgAscii { const char* bases; uint64_t nbytes; const uint64_t* off; uint64_t n_in; uint64_t good = 0, total_bp = 0, small = 0; int maxL = 0, minL = 0, S = 0; };
int dev_organize_reads(Device* d, const uint64_t* pool, uint64_t pool_words, const uint64_t* off, const uint16_t* len, uint64_t n, int S, int minL, int maxL, int k,
                       uint64_t* N_out, RawU64& words_out, RawU16& freq_out, std::string& err, OrgAscii* ascii = nullptr, bool pairing = false);
// pairing (sage2ov_reads_pair_library): dev_organize_reads(..., pairing) also leaves +-id of every staged read on the device (of every raw record on
// the ASCII route, 0 for one that was not staged), 4 bytes each, until dev_pairing_release or the read set goes.  dev_mates_pair_call: one reads_add_* call as one
// mates call -- `records` input records; ord: the call's staged reads are entries [first, first + nStaged) of the staging and ord[x] < records is the ordinal of the
// x-th; raw: the call's records are raw records [first, first + records).  Its records go to the pending buffer as dev_mates_add's do; dev_mates_flush ends the call.
struct MateStats;
int dev_mates_pair_call(Device* d, bool raw, const uint32_t* ord, uint64_t nStaged, uint64_t first, uint64_t records, int library, uint64_t pair0, MateStats* st, std::string& err);
void dev_pairing_release(Device* d);
// which way the last dev_reduce_device went (the words of sage2ov_reduce_stats_get)
void dev_reduce_stats(Device* d, uint64_t out[SAGE2OV_REDUCE_STATS]);
int dev_reduce_device(Device* d, uint64_t min_unresolved, uint64_t* n_unresolved, uint64_t* n_hits, uint64_t* inserted, uint64_t* removed, int* done, std::string& err,
                      uint32_t shareRank = 0, uint32_t shareWorld = 1);
int dev_export_cand_range(Device* d, void* dev_dst, uint64_t first, uint64_t n, std::string& err);
int dev_replace_cand_tail(Device* d, uint64_t keep, const void* dev_src, uint64_t n, std::string& err);
// append host-computed edge candidates (from the reduce replay) to the device candidate list
int dev_debug_table(Device* d, uint64_t* out5, std::string& err);
int dev_meminfo(Device* d, uint64_t* out4, std::string& err);
// ReadLoader::getIdOfRead, batched (sage2ov_reads_find_ids): query r = bases[off[r], off[r + 1]) -> ids[r] = +-id or 0.  Returns 1 (and does nothing) when neither
// read store is resident: the caller then searches the host copy
struct FindStats { uint64_t found = 0, not_good = 0; uint32_t dirBits = 0, launches = 0; double pack_ms = 0, dir_ms = 0, search_ms = 0; bool byPos = false; };
int dev_find_ids(Device* d, const char* bases, const uint64_t* off, uint64_t n, int64_t* ids, FindStats* st, std::string& err);
// MatePair::processMatePairs on the device (sage2ov_mates_*): dev_mates_add takes one batch of an even number of reads (pair0: ordinal of its first pair in the
// library) into the pending records and flushes them at a bound; dev_mates_flush ends the call.  dev_mates_add returns 1 (and does nothing) when no read store
// is resident.  The table of a library is exported as parallel arrays (key = from:30 | to:30 | t_from:1 | t_to:1, count, first) in key order.
struct MateStats { uint64_t seen = 0, added = 0, not_good = 0, not_found = 0; uint32_t chunks = 0, passes = 0, flushes = 0; double find_ms = 0, records_ms = 0, sort_ms = 0, reduce_ms = 0, merge_ms = 0; };
int dev_mates_add(Device* d, const char* bases, const uint64_t* off, uint64_t n, int library, uint64_t pair0, MateStats* st, std::string& err);
int dev_mates_flush(Device* d, int library, MateStats* st, std::string& err);
void dev_mates_abort(Device* d);                 // drops the pending records of a call that failed
uint64_t dev_mates_count(Device* d, int library);
int dev_mates_export(Device* d, int library, uint64_t* key, uint64_t* cnt, uint64_t* first, uint64_t* offsets, std::string& err);
int dev_mates_import(Device* d, int library, const uint64_t* key, const uint64_t* cnt, const uint64_t* first, uint64_t n, std::string& err);
void dev_mates_clear(Device* d);
int dev_debug_keys(Device* d, uint64_t* out, std::string& err);
int dev_debug_all_hits(Device* d, std::vector<Hit>& hits, std::string& err);
int dev_append_edges(Device* d, const EdgeCand* e, uint64_t n, std::string& err);
// sortEconomyGraph + convertGraph: canonical list
int dev_convert(Device* d, uint64_t* n_final, std::string& err);     // result stays in HBM
int dev_download_edges(Device* d, std::vector<FinalEdge>& out, std::string& err);
int dev_upload_edges(Device* d, const std::vector<FinalEdge>& in, std::string& err);
// step 4 (graph simplification) on the device: the surviving half-edges (pair p = 2p, 2p+1; index = age) and their read lists
struct SimplifiedGraph {
    std::vector<float> flow;          // one per half-edge as loadOverlapGraphFromFile parses it (overlapGraph.cpp:393, :409, :433); empty: every flow is 0
    uint64_t N = 0, n_half_edges = 0, contracted = 0, removed = 0, iterations = 0, pairs_alive = 0, reads_on_edges = 0; double device_ms = 0; bool downloaded = false;
    bool fields = false;              // from .. alive are filled (downloaded: the lists too)
    std::vector<uint32_t> from, to, len, cnt, off; std::vector<uint8_t> type, alive; std::vector<uint64_t> lists;
};
int dev_simplify(Device* d, SimplifiedGraph& out, std::string& err);             // result stays in HBM
int dev_simplify_download(Device* d, SimplifiedGraph& out, std::string& err, bool withLists = true);    // fills the arrays (once); withLists false: the half-edge fields only
// A batch of edge-disjoint splices over the resident graph (kernels_splice.inc): a splice makes a new pair of half-edges from the operand
// half-edges a and b and retires them.  SplicePlan is what the plan kernel of either kind writes for one splice and what the device hands back.
//   made: 0 for a refused merge, always 1 for a join;  type, del1, del2: the new pair's type, whether a's and b's pair were deleted (else they lost `flow`);
//   flow: the flow of the new edge;  lenF, lenT: the lengths of the new forward half and its twin;  extra: the entries between the operands' lists (1: a merge, a join
//   with equal end nodes; 2: a join);  dNext1, dPrev2, how: per direction (forward, twin), the distances between a join's two middle entries and how it was made
//   (0 equal end nodes, 1 overlap, 2 concatenated, 3 gapped)
struct SplicePlan { uint32_t a, b; float flow; uint32_t lenF, lenT, dNext1[2], dPrev2[2]; uint8_t type, made, del1, del2, extra, how[2], pad; };
static_assert(sizeof(SplicePlan) == 44, "the splice record as the device writes it");
struct SpliceStats { uint64_t made = 0, entries_copied = 0, pairs_deleted = 0, half_edges = 0, list_entries = 0, overlaps = 0, concatenated = 0, gapped = 0;
                     double overlap_ms = 0, plan_ms = 0, lists_ms = 0, commit_ms = 0; };
// ContigExtender::mergeEdgesAndUpdate for a batch of merges (sage2ov_graph_merge_pairs; k_mg_plan)
int dev_merge_pairs(Device* d, const uint32_t* a, const uint32_t* b, uint64_t n, int typeOfMerge, SplicePlan* out, SpliceStats* st, std::string& err);
// ScaffoldMaker::mergeDisconnectedEdges for a batch of joins over the graph and the read store (sage2ov_graph_join_pairs; kernels_scaffold.inc).  overlap (may be
// null): 2 n values, what stringOverlapSize returned for the forward and the twin list (-2: equal end nodes, no search)
int dev_join_pairs(Device* d, const uint32_t* a, const uint32_t* b, const int32_t* gap, uint64_t n, SplicePlan* out, int32_t* overlap, SpliceStats* st, std::string& err);
void dev_simplify_release(Device* d);
int dev_simplify_upload(Device* d, const SimplifiedGraph& in, std::string& err);  // a parsed graph (from .. lists filled) takes the place of step 4's result in HBM
// MatePair::mapReadsToEdges / mapReadLocations / computeMeanSD on the device (sage2ov_mates_map_reads, _estimate): dev_readmap_build makes the
// read-to-edge table from the resident step-4 graph; dev_readmap_join the flags and distances of one library's mate table (kept until dev_readmap_drop_joins);
// dev_readmap_round one round's {count, sum, sq low, sq high}.  The table goes with the graph (dev_simplify_release) and the read set.
struct ReadMapStats { uint64_t entries = 0, locations = 0, records = 0; uint32_t passes = 0, rounds = 0; double scan_ms = 0, records_ms = 0, sort_ms = 0, reduce_ms = 0, join_ms = 0, round_ms = 0; };
int dev_readmap_build(Device* d, ReadMapStats* st, std::string& err);
int dev_readmap_join(Device* d, int library, ReadMapStats* st, std::string& err);
int dev_readmap_round(Device* d, int library, long long mu, uint64_t thr, uint64_t out[4], ReadMapStats* st, std::string& err);
void dev_readmap_counts(Device* d, uint64_t* entries, uint64_t* locations);
int dev_readmap_export(Device* d, uint32_t* read, uint32_t* pair, uint32_t* nf, uint32_t* nr, uint32_t* loc, int32_t* locs, uint32_t* offsets, std::string& err);
uint64_t dev_readmap_flag_count(Device* d, int library);
uint64_t dev_readmap_distance_count(Device* d, int library);
int dev_readmap_flags(Device* d, int library, uint8_t* out, std::string& err);
int dev_readmap_distances(Device* d, int library, uint32_t* dist, uint32_t* entry, uint32_t* pair, std::string& err);
void dev_readmap_drop_joins(Device* d);
void dev_readmap_release(Device* d);
int dev_flow_set(Device* d, const float* flow, uint64_t n, std::string& err);      // one float per half-edge of the resident graph; null: every flow is 0
// the sweep of ContigExtender::findMatepairSupports on the device (sage2ov_mates_supports): needs the read-to-edge table, the mate tables and the
// insert bounds.  The table (key = in-half:32 | out-half:32, support) stays in HBM until the read-to-edge table, the mate flags or the flows go.
struct SupportParams { uint64_t bound = 0; int64_t thr[128] = {}; uint32_t libraries = 0; };      // bound: maximumUpperBoundOfInsert; thr[L]: upper[L] + minOverlap - 2 * averageReadLength, 0 when L is not valid
struct SupportStats { uint64_t in_halves = 0, out_halves = 0, candidates = 0, entries_within = 0, records = 0, keys = 0, keys2 = 0; uint32_t passes = 0;
                      double roles_ms = 0, scan_ms = 0, records_ms = 0, sort_ms = 0, reduce_ms = 0; };
int dev_support_build(Device* d, const SupportParams& P, SupportStats* st, std::string& err);
uint64_t dev_support_count(Device* d);
int dev_support_export(Device* d, uint64_t* key, uint32_t* support, std::string& err);
void dev_support_release(Device* d);
// the sweep that opens ScaffoldMaker::mergeFinal / mergeFinalSmall on the device (sage2ov_links): needs the read-to-edge table, the mate tables and
// the insert estimates.  The table (key = half a:32 | half b:32, support, gap) stays in HBM until the read-to-edge table or the mate flags go; flows are not read.
struct LinkParams { uint64_t bound = 0; int64_t thr[128] = {}; uint32_t gbase[128] = {}; uint32_t libraries = 0; };      // bound: maximumUpperBoundOfInsert; thr[L]: upper[L] + minOverlap -
                                                                                                                         // 2 * averageReadLength, 0 when L is not valid; gbase[L]: Mean[L] - 2 * averageReadLength mod 2^32
struct LinkStats { uint64_t halves = 0, entries_within = 0, unique_entries = 0, mate_entries = 0, records = 0, keys = 0; uint32_t passes = 0;
                   double halves_ms = 0, scan_ms = 0, records_ms = 0, sort_ms = 0, reduce_ms = 0; };
int dev_links_build(Device* d, const LinkParams& P, LinkStats* st, std::string& err);
uint64_t dev_links_count(Device* d);
int dev_links_export(Device* d, uint64_t* key, uint32_t* support, int32_t* gap, int32_t* gapSum, std::string& err);
void dev_links_release(Device* d);
// the sweep of ContigExtender::findPathSupports / findPathSupportsNew on the device (sage2ov_path_supports; kernels_paths.inc): needs the read-to-edge
// table, the mate tables, the insert bounds and the mate flags as of the estimate (dev_estflags_keep: a copy per library that outlives the read-to-edge table of the
// graph it was made on).  The table (key = half a:32 | half b:32, a entering the node b leaves; support) stays in HBM as long as the mate-pair supports would.
struct PathParams { uint64_t bound = 0; int64_t lower[128] = {}, upper[128] = {}; uint8_t valid[128] = {}; uint32_t libraries = 0; };      // bound: maximumUpperBoundOfInsert
struct PathStats { uint64_t claimed_reads = 0, claiming_nodes = 0, start_nodes = 0, paths = 0, capped_nodes = 0, eligible = 0, voting = 0, records = 0, rows = 0, mirrored = 0;
                   uint32_t passes = 0; double claim_ms = 0, starts_ms = 0, walk_ms = 0, vote_ms = 0, sort_ms = 0, reduce_ms = 0; };
int dev_estflags_keep(Device* d, int library, std::string& err);      // after dev_readmap_join of the library
void dev_estflags_release(Device* d);
int dev_paths_build(Device* d, const PathParams& P, PathStats* st, std::string& err);
uint64_t dev_paths_count(Device* d);
int dev_paths_export(Device* d, uint64_t* key, uint32_t* support, std::string& err);
void dev_paths_release(Device* d);
// OverlapGraph::printGraph / saveContigsToFile on the device (sage2ov_contigs_*).  dev_contigs_build selects, orders and lays out the rows: they stay
// in HBM with the running distPrevious of the list pool and come back in table order.  dev_contigs_spell_begin spells the strings of a range of rows into one of two
// buffers -- 16-byte chunks, every row from a chunk boundary -- and copies them to a pinned host image; dev_contigs_spell_wait hands that image out.  The table goes
// with the graph (dev_simplify_release) and the read set.
struct ContigRow { uint32_t h, string_length, contig_length, start, gap_count, n_count, flags, pad; };      // h: the half-edge; flags: 1 inconsistent, 2 wrapped, 4 beyond the limit
struct ContigBuildStats { uint32_t passes = 0; double select_ms = 0, sort_ms = 0, layout_ms = 0; };
int dev_contigs_build(Device* d, uint32_t threshold, std::vector<ContigRow>& rows, ContigBuildStats* st, std::string& err);
int dev_contigs_spell_begin(Device* d, int which, uint64_t first, uint64_t count, uint64_t chunk0, uint64_t nChunks, std::string& err);
int dev_contigs_spell_wait(Device* d, int which, const char** image, double* ms, std::string& err);
void dev_contigs_release(Device* d);
// step 5 around its solver on the device (sage2ov_genome_size_estimate, sage2ov_flow_*; kernels_copycount.inc).  dev_copycount_prepare uploads the
// frequencies (freq[0 .. N]) and makes k of every pair and the number of present reads; dev_copycount_round returns one round's {deltaSum, kSum} (previous 0: the
// first round); dev_flownet_build the arc records and what dev_flow_apply needs, in allocations of their own that go with the graph and the read set.
struct CopyCountStats { uint64_t present = 0, nodes = 0, edges = 0, simple = 0, once = 0, many = 0, arcs = 0, applied = 0, different = 0; uint32_t passes = 0;
                        double k_ms = 0, round_ms = 0, order_ms = 0, classes_ms = 0, arcs_ms = 0, apply_ms = 0; };
struct CopyCountConst { float ratio, lj[21], l1, l3, l5, l1000, fN1, fN3, fN5; double dN3, dN1000; uint64_t n; };
struct FlowArc { uint32_t from, to; int32_t lower, upper; float cost; };
int dev_copycount_prepare(Device* d, const uint16_t* freq, CopyCountStats* st, std::string& err);
int dev_copycount_round(Device* d, int first, float ratio, float l2, uint64_t out[2], CopyCountStats* st, std::string& err);
int dev_flownet_build(Device* d, const CopyCountConst& C, CopyCountStats* st, std::string& err);
uint64_t dev_flownet_arcs(Device* d);
int dev_flownet_export(Device* d, FlowArc* out, std::string& err);
int dev_flow_apply(Device* d, const uint64_t* from, const uint64_t* to, const uint64_t* flow, uint64_t n, CopyCountStats* st, std::string& err);
int dev_flow_get(Device* d, float* flow, uint64_t n, std::string& err);
void dev_copycount_release(Device* d);
// step 5's solver on the device (sage2ov_mcf_solve, sage2ov_flow_solve, sage2ov_flow_solution_*; kernels_flow.inc).  dev_mcf_solve: any network, host
// arrays in and out (arcs: sage2ov_mcf_arc records; price may be null).  dev_flow_solve: the resident network; its solution stays on the device with the network.
struct McfStats { uint64_t nodes = 0, arcs = 0, scale = 0, phases = 0, rounds = 0, pushes = 0, relabels = 0, updates = 0; uint32_t form = 0, priceWords = 0; double build_ms = 0, solve_ms = 0;
                  uint64_t refine_rounds[SAGE2OV_MCF_PHASES] = {}; double refine_ms[SAGE2OV_MCF_PHASES] = {};
                  uint64_t hub[6] = {}; };             // sage2ov_mcf_hub_stats_get: threshold in force, MF_HUB_TILE, hubs, tiles, entries pushed along and relabels by the hub form
// wide: 128-bit prices (price: two words per node, the low one first).  dev_flow_solve chooses the width itself; dev_flow_price_words: 1 or 2, of the resident solution
// (0: none).  mcf_wide_guard: whether n nodes with that largest |cost| stay inside +-2^126 (host arithmetic only).
int dev_mcf_solve(Device* d, const void* arcs, uint64_t m, uint32_t n, uint64_t maxRounds, bool wide, int64_t* flow, void* price, McfStats* st, std::string& err);
bool mcf_wide_guard(uint64_t n, uint64_t maxc);
uint32_t dev_flow_price_words(Device* d);
int dev_flow_solve(Device* d, uint64_t maxRounds, McfStats* st, std::string& err);
bool dev_flow_solved(Device* d);
int dev_flow_solution_get(Device* d, int64_t* flow, void* price, std::string& err);
int dev_flow_commit(Device* d, CopyCountStats* st, uint64_t* tts, uint64_t* lines, std::string& err);
void dev_timings(Device* d, DevTimings* t);
void dev_reset_timings(Device* d);
int dev_sync(Device* d, std::string& err);

}  // namespace s2
