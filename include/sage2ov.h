/* ============================================================================
 * sage2ov.h -- C ABI of the MI355X-native SAGE2 read-overlap path (CLI steps 1-3; step 4 at the end of the file).
 *
 * SAGE2 has no plugin/FFI interface; its replaceable seam is (a) the step/prefix file
 * API (<outdir>/<prefix>.reads + <prefix>.graph3, consumed by `SAGE2 -m 4 -i <prefix>`,
 * main.cpp:141-148) and (b) in process, the four classes main.cpp:44-131 drives:
 * ReadLoader -> HashTable -> EconomyGraph -> OverlapGraph.  Each entry point below
 * replaces the member function cited next to it (paths relative to the reference tree).
 *
 * Conventions: opaque context, plain pointers and sizes, no exceptions across the ABI,
 * `int` status (0 ok, <0 error; text via sage2ov_last_error), caller-owned output
 * buffers, one host thread per context (distinct contexts may live on distinct threads).
 * All device work is hand-written HIP for gfx950 on the context's own stream; there is no
 * CPU fallback: every compute call fails with SAGE2OV_ERR_DEVICE when no GPU is usable.
 * ========================================================================== */
#ifndef SAGE2OV_H_
#define SAGE2OV_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAGE2OV_OK            0
#define SAGE2OV_ERR_ARG      -1   /* bad argument / call order */
#define SAGE2OV_ERR_IO       -2   /* file could not be opened / parsed */
#define SAGE2OV_ERR_DEVICE   -3   /* HIP error or no GPU */
#define SAGE2OV_ERR_NOMEM    -4
#define SAGE2OV_ERR_LIMIT    -5   /* input exceeds a documented limit */
/* The documented limits of a context (SAGE2OV_ERR_LIMIT; the reference's widths next to them):
 *   - read length <= 1018 bases (32 words of 2-bit bases with the 11-bit length field in the last one; inputReader/readLoader.h:28 holds any uint16_t length:
 *     reads of 1019 .. 65535 bases are refused by the reads_add_* / reads_organize calls, not truncated);
 *   - fewer than 2^30 unique reads per context (position * 4 + type is a 32-bit entry; economyGraph/hashTable.h:13-18 carries 40-bit ids);
 *   - at most 2^32 slot pairs of the table (8 slots per read: never reached below the previous limit). */
#define SAGE2OV_ERR_INTERNAL -6

typedef struct sage2ov_ctx sage2ov_ctx;

#define SAGE2OV_DEVICE_CURRENT (-1)
#define SAGE2OV_DEVICE_NONE    (-2)  /* step-1-only context (what `-M 1` needs): parsing, canonical order, P.reads.
                                        Every step 2/3 call on it fails with SAGE2OV_ERR_DEVICE. */

typedef struct sage2ov_config {
    uint32_t min_overlap;   /* -k (main.cpp:424); hash string length h = min(k,64) (hashTable.cpp:78-81) */
    int32_t  device;        /* HIP device ordinal; SAGE2OV_DEVICE_CURRENT; SAGE2OV_DEVICE_NONE */
    uint32_t rank;          /* multi-GPU: this context's rank ...            */
    uint32_t world;         /* ... of `world` ranks (0 or 1 = single GPU)    */
    uint32_t host_threads;  /* OpenMP threads for host-side step 1 (0 = default) */
    uint32_t flags;         /* SAGE2OV_FLAG_* */
} sage2ov_config;

#define SAGE2OV_FLAG_HOST_REDUCE 1u  /* force the exact serial BFS replay (economyGraph.cpp:513-564) on the host
                                        even when the order-independent device form would be exact */
#define SAGE2OV_FLAG_ASYNC_DEVICE 2u /* open the device on a helper thread: sage2ov_ctx_create returns at once and the caller parses its
                                        input files meanwhile (the HIP runtime takes ~0.2 s to start).  The first call that needs the
                                        device waits for it; a device that cannot be opened is reported there (SAGE2OV_ERR_DEVICE) */

/* ---- lifetime: replaces new/delete of the four classes (main.cpp:44,76,108,116) ---- */
int  sage2ov_ctx_create(const sage2ov_config* cfg, sage2ov_ctx** out);
void sage2ov_ctx_destroy(sage2ov_ctx* ctx);
const char* sage2ov_last_error(const sage2ov_ctx* ctx);   /* ctx may be NULL: error of the last failed create */
/* The library's SAGE2OV_* environment switches (test-only route overrides, grid sweeps, diagnostics -- the reference has none,
 * main.cpp:384-521 takes flags only) are read ONCE, when the context is created; no step reads the environment.  This call takes a new snapshot: for tests
 * and diagnostics that change a switch between two steps of one context. */
int sage2ov_options_reload(sage2ov_ctx* ctx);
const char* sage2ov_version(void);

/* ---- STEP 1: ReadLoader (inputReader/readLoader.h:44-55) ---- */
typedef struct sage2ov_read_stats {
    uint64_t total_reads;        /* ReadLoader::totalReads                      */
    uint64_t good_reads;         /* ReadLoader::numberOfReads (incl. duplicates) */
    uint64_t unique_reads;       /* ReadLoader::numberOfUniqueReads = N          */
    uint64_t total_bp;           /* ReadLoader::totalBP                          */
    uint64_t average_read_length;/* global averageReadLength = totalBP/numberOfReads (readLoader.cpp:161) */
    uint32_t max_read_length;
    uint32_t words_per_read;     /* u64 words per read slot in HBM */
} sage2ov_read_stats;

/* readDatasetInBytes' loop body (readLoader.cpp:145-158): filter (len<=k, non-ACGT; utils.cpp:144),
 * canonical orientation (readLoader.cpp:179-213), 2-bit pack (utils.cpp:96).  Read r is
 * bases[offsets[r] .. offsets[r+1]). */
int sage2ov_reads_add_ascii(sage2ov_ctx* ctx, const char* bases, const uint64_t* offsets, uint64_t n);
/* ReadLoader::readDatasetInBytes(mateFile1, mateFile2) (readLoader.cpp:133): FASTA/FASTQ, optionally
 * gzip; with two files reads alternate file1/file2 (inputReader.cpp:26-49). path2 may be NULL. */
int sage2ov_reads_add_file(sage2ov_ctx* ctx, const char* path1, const char* path2);
/* ReadLoader::loadFromList (readLoader.cpp:73): list grammar f1=/f2=/f=, '#' comments. */
int sage2ov_reads_add_list(sage2ov_ctx* ctx, const char* list_path);
/* ReadLoader::organizeReads (readLoader.cpp:215) + the orientation choice of insertReadIntoList (readLoader.cpp:195):
 * canonical orientation, sort by stringCompareInBytes order (utils.cpp:224), unique with frequency (u16 wrap), ids 1..N.
 * With a GPU context all of it runs on the device (the staged forward reads are uploaded once) and the read store stays
 * resident in HBM; a device-less context (SAGE2OV_DEVICE_NONE) uses the host organiser. */
int sage2ov_reads_organize(sage2ov_ctx* ctx);
int sage2ov_reads_stats(const sage2ov_ctx* ctx, sage2ov_read_stats* out);
/* class Read fields (readLoader.h:21-30) for ids 1..N, arrays indexed [0..N] (entry 0 unused):
 * packed = MSB-first 2-bit bytes (utils.cpp:96) of the forward strand, `stride` bytes apart. */
int sage2ov_reads_export(const sage2ov_ctx* ctx, uint8_t* packed, uint64_t stride, uint16_t* length, uint16_t* frequency);
int sage2ov_reads_save(sage2ov_ctx* ctx, const char* path);   /* saveReadsInFile  (readLoader.cpp:270) -> P.reads */
int sage2ov_reads_load(sage2ov_ctx* ctx, const char* path);   /* loadReadsFromFile (readLoader.cpp:289) + upload  */
/* graph3 header fields when reads came from P.reads (good_reads / average length are not in that file;
 * main.cpp:141-148 likewise takes them from the graph file) */
int sage2ov_reads_set_totals(sage2ov_ctx* ctx, uint64_t good_reads, uint64_t total_bp);
/* The organised read store in its HBM word layout ((N+1) x words_per_read u64): one rank
 * organises, the others import the image (multi-GPU: every rank needs all reads). */
int sage2ov_reads_export_words(const sage2ov_ctx* ctx, uint64_t* words, uint64_t cap_words, uint16_t* frequency);
int sage2ov_reads_import_words(sage2ov_ctx* ctx, const uint64_t* words, uint64_t n_unique, uint32_t words_per_read,
                               uint32_t max_read_length, const uint16_t* frequency, uint64_t good_reads, uint64_t total_bp);

/* ReadLoader::getIdOfRead (readLoader.cpp:319-353), batched: query r is bases[offsets[r] .. offsets[r+1]).
 * ids[r] = +id  the read as given is its own canonical form (read < reverse complement, strictly: :325)
 *          -id  its reverse complement is (a read equal to its reverse complement gets -id, as :325-334 do)
 *           0   not in the store, or not a good read (utils.cpp:144-166: length <= minOverlap, a character outside ACGTacgt)
 * Needs organised reads (reads_organize / reads_load / reads_import_words); usable at any later point and
 * changes nothing the steps read or write.  A query longer than the store's longest read is simply not found.  With a GPU context
 * the queries are classified, packed and searched on the device against the resident read store; a device-less
 * context searches its host copy (the reference's method). */
int sage2ov_reads_find_ids(sage2ov_ctx* ctx, const char* bases, const uint64_t* offsets, uint64_t n, int64_t* ids);
typedef struct sage2ov_find_stats {
    uint64_t queries, found, not_good, not_found;
    uint32_t directory_bits, launches;     /* bits of the first-word directory; chunks the batch went through (0, 0 on the host route) */
    double device_ms, directory_ms;        /* HIP events: classify + pack + search of all chunks; the directory build (0 when it was cached) */
    double pack_ms, search_ms;             /* the two parts of device_ms */
    uint32_t route;                        /* SAGE2OV_FIND_ROUTE_*: which copy of the reads the search read */
    uint32_t reserved;
} sage2ov_find_stats;
#define SAGE2OV_FIND_ROUTE_HOST     0u   /* host copy (device-less context, or no store resident on the device) */
#define SAGE2OV_FIND_ROUTE_ID_STORE 1u   /* the id-ordered store in HBM */
#define SAGE2OV_FIND_ROUTE_LOCALITY 2u   /* the locality-ordered store through posOf[] (memory-diet mode after an index build: the id-ordered store is released) */
int sage2ov_reads_find_stats_get(const sage2ov_ctx* ctx, sage2ov_find_stats* out);   /* of the last find call */

/* MatePair::mapMatePairs / processMatePairs (matePair.cpp:125-239), as run with one thread: the table of mate links between read ids.
 * A call hands over reads 0 .. n-1 (layout of sage2ov_reads_add_ascii) and a library number 1 .. 127; its pairs are (2j, 2j+1) for 2j+1 < n, a trailing
 * odd read is dropped (:172), pairs never span two calls.  A pair is skipped when either mate is not a good read (:176), and -- a DELIBERATE DIFFERENCE
 * from the reference -- when either mate is a good read that is not in the store (id 0): the reference files such a pair under read 0 with type 0, which
 * its own log line at readLoader.cpp:350 calls an accident.  With id1 = |ids[2j]|, type1 = ids[2j] > 0, id2 = |ids[2j+1]|, type2 = ids[2j+1] > 0 a
 * surviving pair adds two directed records: (from id1, to id2, type1, type2) with side 0 and its twin (from id2, to id1, type2, type1) with side 1.
 * The table of a library holds one entry per distinct (from, to, type1, type2) among all records given to that library so far:
 *   count  records with that key;  freq = count & 255 (the reference's uint8_t freq starts at 1 and wraps: 256 records give 0)
 *   first  the smallest record ordinal 2 * p + side with that key, p = ordinal of the pair among ALL pairs given to this library so far (skipped
 *          ones included, counted across calls).  matePairList[a] of the reference is the entries of from == a in DESCENDING first (head insertion).
 * Entries of different libraries never merge.  The `flag` field of MatePairInfo (set later by mapReadsToEdges) is not part of this.
 * All calls need organised reads; the table is dropped with the read set and by sage2ov_mates_clear, and changes nothing steps 2-4 read or write.
 * With a GPU context the ids are found, the records written, sorted and reduced and the table merged on the device; a device-less
 * context builds the same table on the host. */
typedef struct sage2ov_mate { uint32_t from, to; uint64_t count, first; uint8_t freq, type1, type2, library; uint8_t pad[4]; } sage2ov_mate;   /* 32 bytes */
int sage2ov_mates_add_ascii(sage2ov_ctx* ctx, const char* bases, const uint64_t* offsets, uint64_t n, int library);   /* processMatePairs for one readsArray */
int sage2ov_mates_add_file(sage2ov_ctx* ctx, const char* path1, const char* path2 /* may be NULL */, int library);    /* mapMatePairs (matePair.cpp:125): one interleaved file, or two files read in turn */
int sage2ov_mates_add_list(sage2ov_ctx* ctx, const char* list_path);   /* mapMatePairsFromList (:70-120): `f=` or `f1=` then `f2=` per dataset; dataset i is library i */
int sage2ov_mates_count(sage2ov_ctx* ctx, int library, uint64_t* n);
/* entries of one library in ascending (from, to, type1, type2); offsets (N + 2 values, may be NULL): the entries of read a are [offsets[a], offsets[a+1]),
 * offsets[N+1] is the entry count.  cap < count: SAGE2OV_ERR_ARG, nothing written */
int sage2ov_mates_export(sage2ov_ctx* ctx, int library, sage2ov_mate* out, uint64_t cap, uint64_t* offsets);
int sage2ov_mates_clear(sage2ov_ctx* ctx);
typedef struct sage2ov_mate_stats {
    uint64_t pairs_seen, pairs_added, pairs_not_good, pairs_not_found;   /* seen = added + not_good + not_found */
    uint64_t records;                        /* 2 * pairs_added */
    uint64_t entries_before, entries_after;  /* of the call's library (add_list: of its last dataset) */
    uint32_t library, libraries;             /* the call's library; the highest library in use (numberOfLibrary) */
    uint32_t chunks, sort_passes;            /* id look-up chunks; 8-bit radix passes run (record sorts and merges); 0, 0 on the host route */
    uint32_t flushes, route;                 /* sort + reduce + merge rounds; SAGE2OV_MATE_ROUTE_* */
    double find_ms, records_ms, sort_ms, reduce_ms, merge_ms;   /* HIP events (0 on the host route) */
} sage2ov_mate_stats;
#define SAGE2OV_MATE_ROUTE_HOST   0u
#define SAGE2OV_MATE_ROUTE_DEVICE 1u
int sage2ov_mates_stats_get(const sage2ov_ctx* ctx, sage2ov_mate_stats* out);   /* of the last add call */
/* The mate table of the reads a context organised, without a second pass over the input: step 1 already knows the id and the orientation of
 * every read it staged, and with pairing on the context also remembers which input record each staged read was.
 * sage2ov_reads_pair_library: 0 switches pairing off (the default: step 1 then does exactly what it does without this call); 1 .. 127 makes every later
 *   sage2ov_reads_add_ascii / sage2ov_reads_add_file call ALSO one mates call for that library, by the rules above: the call's records are numbered 0 .. n-1 in
 *   input order (two files: alternating, file 1 first), its pairs are (2j, 2j+1), a trailing odd record is dropped, pairs never span two calls.  With pairing on
 *   sage2ov_reads_add_list numbers its datasets itself, dataset i is library i as in sage2ov_mates_add_list (the value given here only has to be non-zero; more
 *   than 127 datasets: SAGE2OV_ERR_ARG).  A call of 2^32 - 2048 input records or more with pairing on: SAGE2OV_ERR_LIMIT.  After sage2ov_reads_organize, or a
 *   library outside 0 .. 127: SAGE2OV_ERR_ARG.  sage2ov_reads_add_synth is never a mates call.
 * sage2ov_mates_from_reads: adds to the mate tables exactly what the matching sequence of sage2ov_mates_add_* calls would add at that moment -- every entry of
 *   every library field for field, `first` continuing from whatever earlier add calls left, sage2ov_mate_stats as after the last of those calls with
 *   pairs_not_found 0 by construction (a good read is always in the store it was organised into).  Needs organised reads that were staged with pairing on, else
 *   SAGE2OV_ERR_ARG and nothing changes; once per organised read set (a second call: SAGE2OV_ERR_ARG).  It reads neither the input nor the read store, so it works
 *   at any point after sage2ov_reads_organize, memory-diet mode after an index build included.  What pairing remembers (4 bytes per staged read on the host until
 *   the organiser has run, 4 bytes per staged read -- per input record on the ASCII route of a GPU context -- on the device after it) is released by this call, by
 *   sage2ov_mates_clear and with the read set. */
int sage2ov_reads_pair_library(sage2ov_ctx* ctx, int library);
int sage2ov_mates_from_reads(sage2ov_ctx* ctx);

/* ---- STEP 2: HashTable (economyGraph/hashTable.h:20-43) ---- */
typedef struct sage2ov_index_stats {
    uint64_t slots;          /* open-addressed 8-byte slots in HBM           */
    uint64_t keys;           /* occupied slots (distinct prefix/suffix keys, up to tag merges) */
    uint64_t csr_entries;    /* bucket entries stored out of line            */
    uint64_t long_buckets;   /* buckets with >= 100 entries (hashTable.cpp:111-123): never found */
    uint32_t hash_string_length;
    uint32_t rebuilds;       /* reseeds after an impure long bucket */
    uint32_t minimiser_groups; /* 1: the fast probe kernel's second access path (keys grouped by minimiser) was built and is used; the library decides
                                * by the share of reads without a predecessor in the locality order */
    uint32_t reserved;
} sage2ov_index_stats;
int sage2ov_index_build(sage2ov_ctx* ctx);                      /* hashPrefixesAndSuffix (hashTable.cpp:70) */
int sage2ov_index_stats_get(const sage2ov_ctx* ctx, sage2ov_index_stats* out);
/* hashTableSearch (hashTable.cpp:193) + the bucket walk of economyGraph.cpp:89-93 for one key
 * (key[0]=v0 leading bases, key[1]=v1 last 32 bases, utils.cpp:171-187).  Entries are id*4+type in
 * bucket order; *count = 0 for "not found" (absent or long).  Test/diagnostic entry point. */
int sage2ov_index_lookup(sage2ov_ctx* ctx, const uint64_t key[2], uint64_t* entries, uint32_t cap, uint32_t* count);
/* saveHashTableInFile (hashTable.cpp:256-273, :12-20) -> P.hashTable: the slot-by-slot text dump of the REFERENCE's double-hashed table (what
 * `SAGE2 -m 3` loads).  Our index has another shape, so the reference's serial insertion (hashTable.cpp:94-109, :133-187: table size, start
 * slot, probe step, 101-entry cap, long-bucket flag) is replayed on the host for this file alone.  Needs organised reads only (no GPU). */
int sage2ov_hashtable_save(sage2ov_ctx* ctx, const char* path);

/* ---- STEP 3: EconomyGraph + OverlapGraph::convertGraph ---- */
typedef struct sage2ov_overlap_stats {
    uint64_t verified_overlaps;   /* sum of `connections` (economyGraph.cpp:96,189,281,361) = N_ov */
    uint64_t contained_extension; /* "Total contained by extension" (economyGraph.cpp:485) */
    uint64_t contained_size;      /* "Total contained by size"      (economyGraph.cpp:486) */
    uint64_t left_to_explore;     /* economyGraph.cpp:487 */
    uint64_t edges_inserted;      /* "Total edges inserted"   (economyGraph.cpp:569), twins counted */
    uint64_t transitive_removed;  /* "Transitive edge removed"(economyGraph.cpp:571) */
    uint64_t edges;               /* undirected edges in the canonical list (= record pairs in P.graph3) */
    uint64_t unresolved_hits;     /* directional hits of status-0 reads fed to the reduce phase */
} sage2ov_overlap_stats;
/* buildInitialOverlapGraph (economyGraph.cpp:37): probe+verify+extension kernel over this rank's read
 * range, then the reciprocal pass (economyGraph.cpp:455-480). */
int sage2ov_overlap_initial(sage2ov_ctx* ctx);
/* buildOverlapGraphEconomy (economyGraph.cpp:495): all-edges + transitive reduction of unresolved reads.
 * On the device; when the index hides keys (>= 100 entries, hashTable.cpp:111-123) the order in which the serial BFS explores
 * the reads decides which edges exist (:605) and is walked on the host over device-built lists. */
int sage2ov_overlap_reduce(sage2ov_ctx* ctx);
/* sortEconomyGraph (economyGraph.cpp:896) + OverlapGraph::convertGraph (overlapGraph.cpp:84):
 * canonical edge list, ascending (from,to,type,length), from<to, one per (from,to,type). */
int sage2ov_overlap_convert(sage2ov_ctx* ctx);
int sage2ov_overlap_stats_get(const sage2ov_ctx* ctx, sage2ov_overlap_stats* out);
/* per-read results of the initial pass, arrays [0..N]: ExtensionTable records packed exactly like
 * economyGraph.h:24-30 (readId:40 | type:2 | length:22), exploredReads value (0/4/5/6), connections. */
int sage2ov_overlap_export_initial(sage2ov_ctx* ctx, uint64_t* right_ext, uint64_t* left_ext, uint8_t* status, uint32_t* connections);

typedef struct sage2ov_edge {      /* one record pair of P.graph3 (overlapGraph.cpp:12-20,136-163) */
    uint64_t from, to;             /* from < to */
    uint32_t length;               /* Edge::lengthOfEdge of from->to  */
    uint32_t length_twin;          /* lengthOfEdge of the twin to->from */
    uint8_t  type;                 /* typeOfEdge of from->to; twin = reverseEdgeType (utils.cpp:212) */
    uint8_t  pad[7];
} sage2ov_edge;
int sage2ov_edges_count(const sage2ov_ctx* ctx, uint64_t* n);
int sage2ov_edges_export(sage2ov_ctx* ctx, sage2ov_edge* out, uint64_t cap);
int sage2ov_graph_save(sage2ov_ctx* ctx, const char* path);     /* saveOverlapGraphInFile (overlapGraph.cpp:338) -> P.graph3 */
/* loadOverlapGraphFromFile's role for a graph of simple edges (overlapGraph.cpp:371): take this edge list (the layout edges_export
 * writes; pairs are pushed in the order given) instead of computing it -- the entry for step 4 on an existing graph. */
int sage2ov_edges_import(sage2ov_ctx* ctx, const sage2ov_edge* edges, uint64_t n);
int sage2ov_graph_load(sage2ov_ctx* ctx, const char* path);     /* loadOverlapGraphFromFile (overlapGraph.cpp:371) <- P.graph3 (simple edges) */

/* ---- step 4: simplification of the overlap graph on the device, main.cpp:139-172 over overlapGraph/simplification.cpp:
 * contractCompositePaths (:14), removeDeadEnds (:58), removeBubbles (:118) in the reference's loop, with its growing thresholds.
 * Needs sage2ov_overlap_convert.  The result is the graph the reference holds in memory after its step 4; sage2ov_graph4_save writes
 * it with saveOverlapGraphInFile's format (overlapGraph.cpp:338-369, :12-20) as `P.graph4`, the file the reference's step 5 reads
 * (main.cpp:196) but none of its steps writes. */
typedef struct sage2ov_simplify_stats {
    uint64_t nodes_contracted;     /* sum of contractCompositePaths' "Nodes removed" */
    uint64_t removed;              /* sum of removeDeadEnds' and removeBubbles' return values */
    uint64_t loop_iterations;      /* passes of the while(1) loop, main.cpp:158 */
    uint64_t edges;                /* surviving edge pairs */
    uint64_t reads_on_edges;       /* entries of the surviving forward read lists */
    double   device_ms;
} sage2ov_simplify_stats;
int sage2ov_graph_simplify(sage2ov_ctx* ctx);
int sage2ov_simplify_stats_get(const sage2ov_ctx* ctx, sage2ov_simplify_stats* out);
int sage2ov_graph4_save(sage2ov_ctx* ctx, const char* path);

/* loadOverlapGraphFromFile's role for a graph with composite edges (overlapGraph.cpp:371-443): any P.graph4 / P.graph5 / P.graph6.  The file is parsed on the
 * host and uploaded into step 4's half-edge and read-list pools, record pairs in file order (pair p = half-edges 2p, 2p+1: the record and its twin).  The
 * header is handled as sage2ov_graph_load handles it.  `flow` is parsed and kept, one float per half-edge, the record's and the twin's each their own (overlapGraph.cpp:393, :409, :433): sage2ov_mates_supports
 * reads it (step 5 assigns it and changes no edge, copycountEstimator.cpp:401-402, :710-711); sage2ov_graph4_save writes 0 as it always does.  Needs organised reads and a GPU context.
 * Refused with SAGE2OV_ERR_ARG: a twin that does not mirror its record (end nodes, list length, or a twin list that is not the forward list's read ids in
 * reverse order); node or read ids above N or 0; a truncated record.  SAGE2OV_ERR_LIMIT: a distPrevious / distNext above the 11-bit field of a list entry.
 * Afterwards sage2ov_graph4_save and the sage2ov_mates_* calls below work on the loaded graph; sage2ov_graph_simplify is refused (SAGE2OV_ERR_ARG) until
 * sage2ov_overlap_convert has run again.
 * A DELIBERATE DIFFERENCE: saveOverlapGraphInFile writes the record pair of a loop edge (from == to) twice -- both halves hang on the one node and pass
 * `i <= u->ID` (overlapGraph.cpp:354-364) -- as (A, B) and then (B, A).  The reference's loader makes two edges of the two pairs (and its next save four).
 * Here a loop's record pair that is directly followed by its mirror image is taken for what the writer made of ONE edge: it becomes one pair, so that the
 * loaded graph is the graph that was saved and load-then-save reproduces the file.  A loop pair without its mirror image is loaded as it stands. */
int sage2ov_graph_load_composite(sage2ov_ctx* ctx, const char* path);

/* ---- MatePair::meanSdEstimation (matePair.cpp:244-313) over mapReadsToEdges (:387-484), mapReadLocations (:490-569), computeMeanSD (:318-381), as the
 * reference runs them with ONE thread (its loops insert into shared lists without a lock).  On the device; all quantities are integers.
 * The graph is the one step 4 left in HBM (sage2ov_graph_simplify) or a loaded one (sage2ov_graph_load_composite).
 *   A pair p is two half-edges.  E(p) is the half mapReadsToEdges visits first: the one leaving the smaller node id; for a loop the one that comes first in
 *   the node's newest-first list = the half with the higher index = the second record of the pair as sage2ov_graph4_save writes it the first time.
 *   READ-TO-EDGE TABLE: one entry per distinct (read, pair) with the read on the pair's lists (end nodes are not on lists): `forward` = the read's locations
 *   on E's list, `reverse` = on the twin's list, both in list order.  A location is the running sum of distPrevious from the start of the list up to and
 *   including the read's entry (uint32_t arithmetic), negated when orientation == 0 (:521-524), read as int32_t (:575-609).
 *   FLAG of a mate entry (from a, to b): 1 (:206), 0 when a and b have an entry for the same pair (:461-481).
 *   DISTANCES of library L: per mate entry with from < to (once per entry, whatever its count) and per pair both reads have an entry for, when both reads
 *   have exactly one forward location there (:352): d = | |loc(a)| - |loc(b)| |.
 *   ESTIMATION (sage2ov_insert_estimate): mu = sd = 5000; up to 10 rounds; a round considers the d < 4 * mu: count, sum = SUM d, sq = SUM (mu - d)^2,
 *   rmu = sum / count (integer division), rsd = (int)sqrtl((long double)sq / (count - 1)); it is final when |mu - rmu| <= rmu / 100 and |sd - rsd| <= rsd / 100;
 *   then mu, sd = rmu, rsd.  mean = rmu + average read length, sd = rsd, lower = max(0, mean - 3 sd), upper = mean + 3 sd.
 * DELIBERATE DIFFERENCES: (1) a round with count < 2 makes the reference divide by zero; here the library gets valid = 0, rounds = the rounds completed before
 * it, zero mean / sd / bounds, and is left out of the minimum and maximum upper bound.  (2) sq is accumulated exactly (128 bits); the reference's long double
 * sum is exact only below 2^64, equality with it is claimed below that.  (3) 4 * mu is taken in 64 bits (the reference's int product wraps from mu = 2^29 on).
 * The pair of a loop edge: see sage2ov_graph_load_composite. */
typedef struct sage2ov_read_edge {     /* one entry of the read-to-edge table (ReadToEdgeMap, matePair.h) -- 32 bytes */
    uint32_t read, pair;               /* pair: ordinal of the record pair in the order sage2ov_graph4_save writes (a loop, written twice: the first time) */
    uint32_t from, to;                 /* of E */
    uint32_t n_forward, n_reverse;
    uint32_t location;                 /* the entry's locations start here in the location array: n_forward forward ones, then n_reverse reverse ones */
    uint8_t  type, pad[3];             /* typeOfEdge of E */
} sage2ov_read_edge;
#define SAGE2OV_INSERT_ROUNDS 10
typedef struct sage2ov_insert {
    uint32_t valid, rounds, final_round, library;       /* rounds: rounds completed (<= 10); final_round: 1 when the last one met the 1 % rule */
    uint64_t considered[SAGE2OV_INSERT_ROUNDS];         /* "Mate-pairs considered" per round; with valid = 0, considered[rounds] is the count (0 or 1) that ended it */
    int64_t  mu[SAGE2OV_INSERT_ROUNDS], sd[SAGE2OV_INSERT_ROUNDS];   /* rmu, rsd per completed round */
    int64_t  mean, deviation, lower, upper;             /* Mean[L], standardDeviation[L], lowerBoundOfInsert[L], upperBoundOfInsert[L] */
} sage2ov_insert;
typedef struct sage2ov_readmap_stats {                  /* of the last sage2ov_mates_map_reads / sage2ov_mates_estimate */
    uint64_t entries, locations, records;               /* table entries; locations = records = list entries of the alive half-edges */
    uint64_t mate_entries;                              /* mate entries whose flag was computed, all libraries */
    uint64_t distances[128];                            /* per library */
    uint32_t sort_passes, route;                        /* 8-bit radix passes run; SAGE2OV_MATE_ROUTE_DEVICE */
    uint32_t rounds, reserved;                          /* round launches of the last estimate, all libraries */
    double scan_ms, records_ms, sort_ms, reduce_ms, join_ms, round_ms;   /* HIP events */
} sage2ov_readmap_stats;
/* mapReadsToEdges + mapReadLocations: builds the table from the resident graph and sets the flag of every mate entry present.  SAGE2OV_ERR_ARG without a
 * step-4 graph, SAGE2OV_ERR_DEVICE on a device-less context.  The table is dropped whenever the graph or the read set changes (reads_*, overlap_convert,
 * edges_import, graph_simplify, graph_load_composite); after sage2ov_mates_add_* / _clear the flags and distances are recomputed by the next call that needs them. */
int sage2ov_mates_map_reads(sage2ov_ctx* ctx);
/* the table in ascending (read, pair): offsets (N + 2 values, may be NULL) as in sage2ov_mates_export; locations: n_locations int32_t.  A buffer that is too
 * small: SAGE2OV_ERR_ARG, nothing written.  Maps first when the table is stale. */
int sage2ov_mates_read_edges_count(sage2ov_ctx* ctx, uint64_t* n_entries, uint64_t* n_locations);
int sage2ov_mates_read_edges_export(sage2ov_ctx* ctx, sage2ov_read_edge* out, uint64_t cap, int32_t* locations, uint64_t cap_locations, uint64_t* offsets);
/* MatePairInfo::flag of the library's entries, parallel to sage2ov_mates_export's order (sage2ov_mates_count values) */
int sage2ov_mates_flags_export(sage2ov_ctx* ctx, int library, uint8_t* flags);
/* the library's distances in mate-entry order, then ascending pair; d may be NULL to size.  *n = their number; cap < *n with d given: SAGE2OV_ERR_ARG */
int sage2ov_mates_distances_export(sage2ov_ctx* ctx, int library, uint32_t* d, uint64_t cap, uint64_t* n);
/* meanSdEstimation: maps when the table is stale, then distances and rounds for every library 1 .. the highest in use.  The distances stay in HBM; a round is
 * one launch that returns count, sum and sq, and the arithmetic is sage2ov_insert_estimate's. */
int sage2ov_mates_estimate(sage2ov_ctx* ctx);
int sage2ov_mates_insert_get(const sage2ov_ctx* ctx, int library, sage2ov_insert* out);                       /* after sage2ov_mates_estimate */
int sage2ov_mates_bounds_get(const sage2ov_ctx* ctx, uint64_t* minimum_upper, uint64_t* maximum_upper);      /* minimumUpperBoundOfInsert, maximumUpperBoundOfInsert (:292-308) */
int sage2ov_readmap_stats_get(const sage2ov_ctx* ctx, sage2ov_readmap_stats* out);
/* the round arithmetic alone, on the host: needs no context and no GPU.  out->library is left 0. */
int sage2ov_insert_estimate(const uint32_t* d, uint64_t n, uint64_t average_read_length, sage2ov_insert* out);

/* ---- the flows of the resident step-4 graph: one float per half-edge.  sage2ov_graph_load_composite fills them from the file; after sage2ov_graph_simplify they are 0
 * (what the reference holds before its step 5).  Both calls use two values per record pair (record, twin) in the order sage2ov_graph4_save writes the pairs; a
 * loop, written twice, counts at its first writing.  This is the in-process route for a caller that ran its own step 5.  export: cap below twice the pair count:
 * SAGE2OV_ERR_ARG, nothing written.  import: n must be twice the pair count, else SAGE2OV_ERR_ARG; the supports below are recomputed by the next call that needs
 * them.  SAGE2OV_ERR_ARG without a step-4 graph, SAGE2OV_ERR_DEVICE on a device-less context. */
int sage2ov_graph_flow_export(sage2ov_ctx* ctx, float* flow, uint64_t cap);
int sage2ov_graph_flow_import(sage2ov_ctx* ctx, const float* flow, uint64_t n);

/* ---- step 5 around its solver (CopyCountEstimator, overlapGraph/copycountEstimator.cpp): the genome-size estimate (:29-100), the flow network as
 * input.cs2 (computeMinCostFlow, :105-355) and a solver's output.cs2 back onto the flows (:362-403), over the resident step-4 graph.  The solver (CS2, :359) has its
 * own section below (sage2ov_flow_solve); a caller may still run any min-cost-flow solver on the file or the arc records.  computeMinCostFlow_new (:422-) is never called by main.cpp.
 *
 * State restated: the reference's after `-m 5` loads the files this library writes -- loadOverlapGraphFromFile (overlapGraph.cpp:371-443) of what
 * sage2ov_graph4_save would write.  insertIntoList puts the newest edge first, so a node's edge list is the reverse of file order over the records that start at the
 * node; a loop's record pair is in the file twice and is two edges, four records at its node.  checkIfAllReadsPresent (overlapGraph.cpp:445-493, main.cpp:199)
 * runs first and replaces numberOfReads: n = the sum of Read::frequency over the reads that are a node with an edge or stand on a read list (reads_present).
 *   k of a record     sum of frequency (uint16_t) over its read list (:73-79, :137-143, :250-254); forward and twin lists hold the same reads; 0 for a simple edge.
 *                     delta = lengthOfEdge - 1.
 *   genome size       previous = 0; up to 10 rounds (:36-49).  A round (:59-100) sums delta and k over the records with from < to (:69: each non-loop pair once, a
 *                     loop never) that qualify: lengthOfEdge > 500 in the round with previous == 0 (:90), else a >= 3 && delta >= 1000 with
 *                     a = (float)delta * ((float)n / (float)previous) - (float)k * log((float)2), every operation in float (:83-84).
 *                     current = (uint64_t)((float)n / (float)kSum * (float)deltaSum) (:98); the rounds end when current == previous (:39).
 *                     NAMED DIFFERENCE FROM ISO C++ (not from the reference): a float that does not fit uint64_t -- NaN when nothing qualifies, an infinity, 2^64 or
 *                     more -- gives 2^63 = 9223372036854775808, as the reference's x86-64 build does for the NaN, and `degenerate` is 1.
 *   classes           of a record with from >= to (:130, :229): simple (no list); once: a_1 >= 3 && delta >= 1000 (:146, :294); many: every other one.
 *                     a_j = (float)delta * ((float)n / (float)G) - (float)k * log((float)((float)(j + 1) / (float)j)), j = 1..20 (:145, :256), G the genome size.
 *                     many: flow_lb = the first j + 1, j = 1..19, with a_j < -3 && a_{j+1} > 3 when delta > 1000 (:305-315), else 1 when the list has more than 35
 *                     entries (:318), else 0.
 *   arcs              header, `n 1 0`, `n 2 0`, `a 2 1 1 <100 * network nodes> 0` (:190-193); network nodes = 4 * nodes + 2 (:160).  Six arcs per node that has an
 *                     edge, nodes ascending, node_index = 3 + 4 * rank (:195-224).  Then for every node i ascending the records of its list, in list order, with
 *                     i >= ID (:225-229): two arcs (simple: 0 100 cost 10000; once: 1 1 cost 1) or six (many: bounds :333-338); end points by typeOfEdge :258-285.
 *   costs of a many   three float accumulators folded over the list entries in list order (:325-332), divided by 2, 2 and 995 (:340-342), printed as cost * 10 with
 *                     std::fixed.  With <cmath> and `using namespace std`, log((float)x) is the float overload and log(N - first_UB), log(N - third_UB) -- integer
 *                     arguments -- the double one: the terms of cost_1 and cost_3 are double, added to the float accumulator in double and rounded back; cost_2 is
 *                     float throughout.  (n - xi) is uint64_t and goes to float or double as its partner demands.  The goldens confirm the overloads.
 *   apply             a line `from to flow` (:365-366), in the solver's order.  Lines on node 1 or 2 are skipped (a `2 1` or `1 2` line is the T-to-S flow, the last such line when there are several, :372-373), as are
 *                     lines whose ends are the same graph node (:378).  Else the flow is added to the first record of from_node's list whose ID is to_node
 *                     (:380-387): with parallel edges the record written last in the file, whatever arc carried the flow.  Then both halves of every pair get
 *                     (f + f_twin) / 2, and flow_different counts the pairs whose halves differed (:391-403).  The additions are small integers, exact in any
 *                     order: integer atomics and one averaging pass equal the reference.
 *   P.graph5          saveOverlapGraphInFile (overlapGraph.cpp:338-369): sage2ov_graph4_save's text with the genome size in line 1, reads_present in line 2 and
 *                     the flows as `ostream << float` prints them.  A loop's pair is written twice (the reference, holding it as two edges, writes four).
 * Every call: SAGE2OV_ERR_ARG without a step-4 graph, SAGE2OV_ERR_DEVICE on a device-less context.  Estimate and network go when the graph or the read set
 * changes; build estimates first when the estimate is stale, count / export / save build first when the network is stale. */
#define SAGE2OV_GENOME_ROUNDS 10
typedef struct sage2ov_genome_estimate {
    uint64_t genome_size;                              /* the estimate of the last round */
    uint64_t estimate[SAGE2OV_GENOME_ROUNDS];          /* of every round run */
    uint64_t delta_sum[SAGE2OV_GENOME_ROUNDS], k_sum[SAGE2OV_GENOME_ROUNDS];
    uint32_t rounds;                                   /* rounds run, 1..10 */
    uint32_t degenerate;                               /* the last round's float did not fit uint64_t */
    uint32_t agreed;                                   /* the last round repeated the one before ("Final estimation"); 0 after ten rounds without */
    uint32_t reserved;
} sage2ov_genome_estimate;
typedef struct sage2ov_flow_arc { uint32_t from, to; int32_t lower, upper; float cost; } sage2ov_flow_arc;      /* cost: as printed (already * 10).  Arc 0 is `2 1`:
                                                                                                                 * its upper bound saturates at 2^31 - 1 here, the file has the exact number */
typedef struct sage2ov_copycount_stats {
    uint64_t genome_size, estimate[SAGE2OV_GENOME_ROUNDS];
    uint32_t rounds, degenerate, agreed, reserved;
    uint64_t reads_present;                            /* n: numberOfReads after checkIfAllReadsPresent */
    uint64_t nodes, edges, simple, once, many;         /* as computeMinCostFlow logs them (:154-158); a loop counts four times */
    uint64_t network_nodes, network_arcs;              /* the `p min` line */
    uint64_t t_to_s_flow, flow_different;              /* of the last solution applied */
    uint64_t solution_lines, lines_applied;            /* lines given, lines that found their record */
    double prepare_ms, rounds_ms, order_ms, classes_ms, arcs_ms, apply_ms;      /* HIP-event times of the stages */
} sage2ov_copycount_stats;
/* the rounds alone, on the host: needs no context and no GPU.  length[i], k[i]: lengthOfEdge and k of the i-th non-loop pair (its record with from < to); reads: n */
int sage2ov_genome_size_rounds(const uint32_t* length, const uint64_t* k, uint64_t pairs, uint64_t reads, sage2ov_genome_estimate* out);
int sage2ov_genome_size_estimate(sage2ov_ctx* ctx, uint64_t* genome_size);
int sage2ov_flow_network_build(sage2ov_ctx* ctx);                                       /* SAGE2OV_ERR_LIMIT from 2^32 - 2048 arcs on */
int sage2ov_flow_network_count(sage2ov_ctx* ctx, uint64_t* network_nodes, uint64_t* arcs);
int sage2ov_flow_network_export(sage2ov_ctx* ctx, sage2ov_flow_arc* out, uint64_t cap);  /* the arcs in input.cs2's order; cap below their number: SAGE2OV_ERR_ARG, nothing written */
int sage2ov_flow_network_save(sage2ov_ctx* ctx, const char* path);                      /* input.cs2, byte for byte */
/* n lines (from[i], to[i], flow[i]).  A node number that is 0 or above the network's nodes, or a null array: SAGE2OV_ERR_ARG, nothing changes (any other error: the
 * supports and contigs are stale and the flows may be partly updated, as after a failed sage2ov_graph_flow_import).  The flows add onto those present; the
 * supports and contigs are recomputed by the next call that needs them, as after sage2ov_graph_flow_import.  Needs the network (built when stale). */
int sage2ov_flow_solution_apply(sage2ov_ctx* ctx, const uint64_t* from, const uint64_t* to, const uint64_t* flow, uint64_t n);
int sage2ov_flow_solution_load(sage2ov_ctx* ctx, const char* path);                     /* output.cs2: whitespace-separated triples; anything else: SAGE2OV_ERR_IO */
int sage2ov_graph5_save(sage2ov_ctx* ctx, const char* path);
int sage2ov_copycount_stats_get(const sage2ov_ctx* ctx, sage2ov_copycount_stats* out);

/* ---- step 5's solver (main_cs2, copycountEstimator.cpp:359; cs2/cs2.cpp, cs2/parser_cs2.h): min-cost flow on the device, by Goldberg-Tarjan cost
 * scaling with round-synchronous push-relabel.  The contract is OPTIMAL, NOT IDENTICAL: the total cost is the optimum any exact solver finds; the flows are the
 * reference's only where the optimum is unique.  Integers only; solving the same network twice gives the same flows and prices, bit for bit.
 *   the problem       a circulation: nodes 1..n without supplies (the `n` lines of input.cs2 say 0), arcs with lower <= flow <= upper, sum of flow * cost minimal.
 *                     parser_cs2.h:257 reads a cost with %lld: the integer prefix of the printed text, truncation towards zero (`-691.348000` is -691, `-0.7` is 0).
 *   scale             costs are multiplied by n + 1: a flow that is 1-optimal in scaled units is optimal.  Prices are in scaled units.
 *   the certificate   lower <= flow <= upper; every node conserved; cost * scale + price[from] - price[to] >= -1 wherever flow < upper, <= 1 wherever flow > lower.
 *   price width       prices, scaled and reduced costs, epsilon and the price floor are 64-bit integers (sage2ov_mcf_solve) or 128-bit ones (sage2ov_mcf_solve_wide);
 *                     the method, and on a network both admit every flow, price and counter, are the same.  The lowest price the method can reach, with room for one
 *                     reduced cost -- about 10.3 * (n + 1)^2 * max |cost| -- must stay inside +-2^62 or +-2^126: 64 bits carry some 211 000 nodes with step 5's costs
 *                     of 10^7, 128 bits any network whose nodes are 32-bit numbers and whose costs stay below about 2^58 -- every resident network.  The calls on the
 *                     resident network (sage2ov_flow_solve, sage2ov_copy_counts) take 64 bits where that guard admits the network and 128 bits where it does not.
 *                     A 128-bit price is two uint64_t words, the low one first, two's complement.
 *   limits            SAGE2OV_ERR_LIMIT, nothing solved: the guard of the width refuses (checked before any launch of the solve, and again before every price
 *                     update); 2^31 - 2048 arcs or more; the round budget spent (max_rounds; 0: SAGE2OV_MCF_DEFAULT_ROUNDS) -- then
 *                     the statistics are filled in, nothing is applied and the graph, the network and any earlier solution stay as they were.
 *   SAGE2OV_ERR_ARG   from == to, a node number outside 1..n, lower > upper, a negative bound; an infeasible network ("infeasible" in sage2ov_last_error): excess
 *                     that no residual path carries to a deficit, or a price below the bound of the method.
 * SAGE2OV_ERR_DEVICE on a device-less context. */
#define SAGE2OV_MCF_DEFAULT_ROUNDS (1ull << 22)
#define SAGE2OV_MCF_PHASES 24               /* epsilon phases whose rounds and times the statistics keep (2^62 needs 21; 128-bit prices can need more: the first 24 are kept) */
#define SAGE2OV_MCF_FORM_LDS 1              /* one workgroup, the network in LDS: at most 512 nodes and 1024 arcs */
#define SAGE2OV_MCF_FORM_LAUNCHES 2         /* two launches per round (six where the network has hub nodes), the rounds counted on the host */
#define SAGE2OV_MCF_HUB_DEG 65536           /* the launches form: a node whose list (arcs out and in) is longer is a hub -- its list is walked by a workgroup per tile of its entries, not by the node's own */
typedef struct sage2ov_mcf_arc { uint32_t from, to; int32_t lower, upper; int64_t cost; } sage2ov_mcf_arc;      /* cs2/parser_cs2.h:232-262: `a from to lower upper cost` */
typedef struct sage2ov_mcf_stats {
    uint64_t nodes, arcs, scale;                       /* scale = nodes + 1 */
    uint64_t phases, rounds, pushes, relabels, price_updates;
    int64_t  total_cost;                               /* sum of flow * cost, unscaled */
    uint32_t form, price_words;                        /* SAGE2OV_MCF_FORM_*; 64-bit words of a price: 1 or 2 */
    double   build_ms, solve_ms;                       /* HIP-event times: layout, rounds */
    uint64_t refine_rounds[SAGE2OV_MCF_PHASES];        /* the launches form: per epsilon phase */
    double   refine_ms[SAGE2OV_MCF_PHASES];
} sage2ov_mcf_stats;
/* any network; needs a device context and no reads.  flow_out: m words, the full flow (lower bound included, cs2.cpp:1872) in input order; price_out: n words or NULL */
int sage2ov_mcf_solve(sage2ov_ctx* ctx, uint64_t n_nodes, const sage2ov_mcf_arc* arcs, uint64_t m, uint64_t max_rounds, int64_t* flow_out, int64_t* price_out, sage2ov_mcf_stats* stats);
/* the same with 128-bit prices, whatever the network (statistics: price_words 2, form SAGE2OV_MCF_FORM_LAUNCHES); price_out: 2 n words or NULL, node v's low word at
 * 2 (v - 1).  The guard against +-2^126 is held on the arcs given before anything is allocated on the device */
int sage2ov_mcf_solve_wide(sage2ov_ctx* ctx, uint64_t n_nodes, const sage2ov_mcf_arc* arcs, uint64_t m, uint64_t max_rounds, int64_t* flow_out, uint64_t* price_out, sage2ov_mcf_stats* stats);
/* the resident network of sage2ov_flow_network_build (before it: SAGE2OV_ERR_ARG); an arc's cost is the truncation towards zero of the float in its record, a NaN or
 * an infinity there SAGE2OV_ERR_ARG (the reference's parser would refuse the line).  The solution stays resident and goes with the network.  stats may be NULL */
int sage2ov_flow_solve(sage2ov_ctx* ctx, uint64_t max_rounds, sage2ov_mcf_stats* stats);
/* flow: one word per arc of sage2ov_flow_network_export, price: one per network node; a cap below the count with the array given: SAGE2OV_ERR_ARG, nothing written;
 * a NULL array is skipped.  Without a solution: SAGE2OV_ERR_ARG */
int sage2ov_flow_solution_export(sage2ov_ctx* ctx, int64_t* flow, uint64_t cap_flow, int64_t* price, uint64_t cap_price, uint64_t* scale);
/* the same for a solution of either width (sage2ov_mcf_stats.price_words of the solve): price has two words per network node (cap_price counts nodes), 64-bit prices
 * sign-extended.  sage2ov_flow_solution_export with a price array on a solution of 128-bit prices: SAGE2OV_ERR_LIMIT, nothing written; without one it serves both */
int sage2ov_flow_solution_export_wide(sage2ov_ctx* ctx, int64_t* flow, uint64_t cap_flow, uint64_t* price, uint64_t cap_price, uint64_t* scale);
/* `from to flow` for the arcs with upper > 0 (cs2.cpp prints no other).  The ORDER IS OURS, not the reference's: by tail, then input order.  sage2ov_flow_solution_load
 * of the file gives the flows sage2ov_flow_solution_commit gives */
int sage2ov_flow_solution_save(sage2ov_ctx* ctx, const char* path);
/* the resident flows onto the graph by the apply path of sage2ov_flow_solution_apply (:365-403), no file and no host copy of the lines; what that call says about
 * adding onto the flows present and about the supports and contigs holds here */
int sage2ov_flow_solution_commit(sage2ov_ctx* ctx);
/* the whole of step 5 (main.cpp -m 5; computeMinCostFlow, :105-417): estimate, build, solve, commit */
int sage2ov_copy_counts(sage2ov_ctx* ctx, uint64_t* genome_size);
int sage2ov_mcf_stats_get(const sage2ov_ctx* ctx, sage2ov_mcf_stats* out);              /* of the last solve */
/* the hub form in the last solve: out[0] the threshold in force (0: off -- the single-workgroup form, or no solve yet), out[1] the entries of a tile, out[2] hub nodes,
 * out[3] tiles, out[4] entries the hub form pushed along (they are among sage2ov_mcf_stats.pushes), out[5] relabels it made (among .relabels).  The flows, prices
 * and counters of a solve do not depend on the threshold.  SAGE2OV_ERR_DEVICE on a device-less context */
int sage2ov_mcf_hub_stats_get(const sage2ov_ctx* ctx, uint64_t out[6]);

/* ---- the sweep of ContigExtender::findMatepairSupports (matePair/mergeContigs.cpp:959-1030): getSupportOfEdges (:1032-1097) over isUniqueInEdge (:1102-1110) for every
 * incoming x outgoing pair of composite edges of every node, on the device; all quantities are integers.  The merge that follows it in the
 * reference (mergeByMatepairSupports / mergeEdgesAndUpdate: order-dependent, changes the graph) is sage2ov_extend_round, below.
 * The graph is the resident step-4 graph; mates, read-to-edge table, locations and insert bounds are those of the calls above.
 *   CANDIDATE HALVES of node i: the alive half-edges leaving i with flow >= 1 (the half's own float), a non-empty read list and from != to (:979).  Such a half is an
 *   IN-HALF when its type is 0 or 1 (the reference's edge1 is its twin, which enters i, :981-983) and an OUT-HALF when its type is 2 or 3 (:984-986).
 *   CANDIDATES: every (in-half a, out-half b) of one node (:987-989).
 *   support(a, b) = getSupportOfEdges(a, b, minOverlap): walk a's list from the node outward with run = the running sum of distPrevious; stop at the first entry with
 *   run > maximumUpperBoundOfInsert (:1043; sage2ov_mates_bounds_get's second value).  For every entry walked (per list entry: a read that stands twice within the
 *   bound counts twice) whose read m1 is UNIQUE ON a, and every mate entry (m1 -> m2, type1, type2) of every library L, whatever its flag or count, once per entry,
 *   with m2 UNIQUE ON b: let d1 be the locations of m1 on half a -- the `forward` ones of its read-to-edge entry if a is E of its pair, else the `reverse` ones
 *   (findDistanceOnEdge, matePair.cpp:575-609) -- and d2 likewise for m2 on b.  The entry counts 1 when some x in d1, y in d2 have s1 * x < 0, s2 * y < 0 (s = +1 for
 *   type 1, -1 for type 0) and |x| + |y| + 2 * averageReadLength < upper[L] + minOverlap (strict, :1073-1076).  A library with valid = 0 never counts.
 *   UNIQUE ON h (:1102-1110): the read has exactly one read-to-edge entry, that entry is for h's pair, and the read is not itself a node with an alive edge.
 * THE TABLE has one entry per candidate with support >= 1.  findMatepairSupports takes those with support > 1 (:992): min_support = 2 gives its list.
 * Equal to the reference while list totals stay below 2^32 and |x| + |y| below 2^31 (its int32_t distance_all).  The pair of a loop edge (sage2ov_graph_load_composite)
 * does not matter here: loops are never candidates and a read on a loop is never unique on a candidate.
 * After sage2ov_graph_simplify every flow is 0: the table is empty, which is no error. */
typedef struct sage2ov_support {       /* 24 bytes */
    uint32_t node;                     /* the node both halves leave */
    uint32_t pair_in, pair_out;        /* ordinals of the record pairs in sage2ov_graph4_save's order, as in sage2ov_read_edge */
    uint32_t to_in, to_out;            /* the other end of the in-half and of the out-half */
    uint32_t support;
} sage2ov_support;
typedef struct sage2ov_support_stats { /* of the last sage2ov_mates_supports */
    uint64_t in_halves, out_halves, candidates;      /* candidates = SUM over the nodes of ins x outs, zero supports included */
    uint64_t entries_within;                         /* list entries of in-halves whose running sum is within the bound */
    uint64_t records;                                /* mate entries that counted (the sum of all supports) */
    uint64_t keys, keys2;                            /* candidates with support >= 1 and >= 2 */
    uint32_t sort_passes, reserved;                  /* 8-bit radix passes run */
    double roles_ms, scan_ms, records_ms, sort_ms, reduce_ms;   /* HIP events */
} sage2ov_support_stats;
/* builds the table.  Estimates first when the estimate is stale (as sage2ov_mates_estimate maps first).  SAGE2OV_ERR_ARG without a step-4 graph, SAGE2OV_ERR_DEVICE on
 * a device-less context, SAGE2OV_ERR_LIMIT from 2^32 - 2048 records on.  The table goes with the graph and the read set, and when the mate table, the flows or the
 * estimate change; sage2ov_mates_supports_count / _export build it when it is stale.  Not sharded: a context with world > 1 behaves as a single one. */
int sage2ov_mates_supports(sage2ov_ctx* ctx);
int sage2ov_mates_supports_count(sage2ov_ctx* ctx, uint32_t min_support, uint64_t* n);
/* the entries with support >= min_support in ascending (node, pair_in, pair_out); cap below their number: SAGE2OV_ERR_ARG, nothing written */
int sage2ov_mates_supports_export(sage2ov_ctx* ctx, uint32_t min_support, sage2ov_support* out, uint64_t cap);
int sage2ov_support_stats_get(const sage2ov_ctx* ctx, sage2ov_support_stats* out);

/* ---- the sweep that opens every round of ScaffoldMaker::mergeFinal (matePair/scaffolding.cpp:786-935) and mergeFinalSmall (:981-1130): for every composite edge and every
 * edge its mates reach, connected through a node or not, the number of mate pairs that link the two and the mean gap those pairs imply, on the device;
 * all quantities are integers.  The merges that follow it in the reference (mergeAccordingToSupport / mergeAccordingToSupport2 / mergeDisconnectedEdges: serial, they change
 * the graph) and its ordering of the rows (quicksortListOfLongEdges, :252-275: ties are open there) are sage2ov_scaffold_round, below.
 * The graph is the resident step-4 graph; mates, read-to-edge table, locations and insert estimates are those of the calls above; minOverlap is the context's k.
 *   LINK(a, b) is defined for an ordered pair of alive half-edges with pair(a) != pair(b) and a non-empty list on a.  Loops take part like any other pair (unlike
 *   sage2ov_mates_supports).  Walk a's list from its start with run = the running sum of distPrevious; stop at the first entry with run > maximumUpperBoundOfInsert
 *   (:833-835).  For every entry walked (per list entry: a read that stands twice within the bound counts twice) whose read m1 is UNIQUE ON a (:837), and every mate
 *   entry (m1 -> m2, type1, type2) of every valid library L, once per entry whatever its count or flag, with m2 UNIQUE ON b (:839-843): let d1 be the locations of m1 on
 *   half a -- the `forward` ones of its read-to-edge entry if a is E of its pair, else the `reverse` ones (findDistanceOnEdge, matePair.cpp:575-609) -- and d2 those of
 *   m2 on half b, both in list order.  Scan x over d1 outside and y over d2 inside: dist = |x| + |y| when s1 * x < 0 and s2 * y < 0 (s = +1 for type 1, -1 for type 0),
 *   otherwise dist = 10 000 000 (:854-865).  The FIRST (x, y) with dist + 2 * averageReadLength < upper[L] + minOverlap (strict, :866) ends the scan: the entry counts 1
 *   towards support and adds Mean[L] - (dist + 2 * averageReadLength) to gapSum, in 32-bit wrapping arithmetic (the reference's int32_t gapSum takes a uint64_t
 *   expression, :878).  It is the first hit in list order that fixes the gap, not the nearest.  gap = gapSum / support as an int32_t division, truncating towards zero (:892).
 *   UNIQUE ON h (:239-247): as for sage2ov_mates_supports.
 * THE TABLE has one row per ordered (a, b) with support >= 1.  No feasibility filter is needed: support >= 1 implies that b's pair is in getListOfFeasibleEdges of a's
 * pair (:148-234), and given that the reference evaluates each ordered pair at most once, from a's side.  Its row (edge_1, edge_2) = (twin of a, b) (:889-890).
 * DELIBERATE DIFFERENCES: (1) the reference skips (a, b) when `edge1 > edge2` compares the ADDRESSES of the two Edge objects (:828), so of (a, b) and (b, a) it keeps
 * whichever malloc placed lower; the table here holds both directions and leaves that choice to the caller.  (2) A library with valid = 0 never counts, as for
 * sage2ov_mates_supports.  (3) A loop that a graph file holds twice is one pair here (sage2ov_graph_load_composite); the reference's loader makes two edges of it.
 * Equal to the reference while list totals stay below 2^32 and |x| + |y| below 2^31 (its int32_t distance_all).
 * FILTERS are applied at export, on the host.  They read lengthOfEdge and flow of E(pair(a)) and E(pair(b)): the halves getListOfCompositeEdges (:104-143) and
 * readToEdgeList[..]->edge hand to the reference.  SAGE2OV_LINKS_ALL: none.  SAGE2OV_LINKS_FINAL (:801): len1 > 200 && len2 > 200, or both flows > 0 and both lengths >
 * contigLengthThreshold = (int)ceilf(100 * (averageReadLength / 100.0)) (:20).  SAGE2OV_LINKS_SMALL (:996): len1 < 500 && len2 < 500.  The flows are those of the host
 * copy at export (as sage2ov_contigs_* take them): sage2ov_graph_flow_import does not make the table stale. */
#define SAGE2OV_LINKS_ALL 0
#define SAGE2OV_LINKS_FINAL 1
#define SAGE2OV_LINKS_SMALL 2
typedef struct sage2ov_link {          /* 44 bytes */
    uint32_t pair_a, pair_b;           /* ordinals of the record pairs in sage2ov_graph4_save's order, as in sage2ov_read_edge */
    uint32_t from_a, to_a, from_b, to_b;   /* the end nodes of the halves a and b themselves */
    uint32_t len_a, len_b;             /* lengthOfEdge of E(pair(a)) and E(pair(b)): the values the filters read */
    uint32_t support;
    int32_t  gap;
    uint8_t  second_a, second_b;       /* 0: the half is the record sage2ov_graph4_save writes first of its pair (the first time, for a loop); 1: it is that record's twin */
    uint8_t  type_a, type_b;           /* typeOfEdge of the halves a and b */
} sage2ov_link;
typedef struct sage2ov_link_stats {    /* of the last sage2ov_links */
    uint64_t halves;                   /* alive half-edges with a list: the halves walked */
    uint64_t entries_within;           /* their list entries whose running sum is within the bound */
    uint64_t unique_entries;           /* of those, the entries whose read is unique on the half */
    uint64_t mate_entries;             /* mate entries of valid libraries probed from them */
    uint64_t records;                  /* (entry, mate entry, half of the mate's pair) that counted: the sum of all supports */
    uint64_t keys;                     /* rows */
    uint32_t sort_passes, reserved;    /* 8-bit radix passes run */
    double halves_ms, scan_ms, records_ms, sort_ms, reduce_ms;   /* HIP events */
} sage2ov_link_stats;
/* builds the table.  Estimates (and maps) first when those are stale.  SAGE2OV_ERR_ARG without a step-4 graph, SAGE2OV_ERR_DEVICE on a device-less context,
 * SAGE2OV_ERR_LIMIT from 2^32 - 2048 records on.  The table goes with the graph and the read set, and when the mate table or the estimate change;
 * sage2ov_links_count / _export build it when it is stale.  Not sharded: a context with world > 1 behaves as a single one. */
int sage2ov_links(sage2ov_ctx* ctx);
/* mode: SAGE2OV_LINKS_*, anything else: SAGE2OV_ERR_ARG */
int sage2ov_links_count(sage2ov_ctx* ctx, uint32_t mode, uint32_t min_support, uint64_t* n);
/* the rows that pass the filter with support >= min_support in ascending (pair_a, second_a, pair_b, second_b); cap below their number: SAGE2OV_ERR_ARG, nothing written */
int sage2ov_links_export(sage2ov_ctx* ctx, uint32_t mode, uint32_t min_support, sage2ov_link* out, uint64_t cap);
int sage2ov_link_stats_get(const sage2ov_ctx* ctx, sage2ov_link_stats* out);

/* ---- OverlapGraph::printGraph (overlapGraph.cpp:507-593) and saveContigsToFile (:607-784): the contigs of the resident step-4 graph, selected, ordered, laid out and
 * spelled on the device; all quantities are integers.  L(i) is the length of read i; a node's DEGREE is the number of alive half-edges leaving it
 * (getDegree, :595-602).
 *   SELECTION (:529-585): a half-edge h is a row when it is alive, from[h] >= to[h] and len[h] >= threshold.  Of a loop (from == to) only the half met first in the
 *   node's newest-first list is a row (:535-547): the half with the higher index of its pair.
 *   threshold = 0 asks for contigLengthThreshold = (int)ceilf(100 * (averageReadLength / 100.0)) (:32) from the context's read totals.
 *   ORDER: lengthOfEdge descending.  The reference's std::sort (:496-501, :588) leaves the order of equal lengths open; HERE ties keep the enumeration order of
 *   :529-531, `from` ascending, then half-edge index descending (a deliberate difference: the order is defined).
 *   STRING (:635-697): len[h] + L(from) characters, all 'N' at first.  The `from` read, reverse-complemented for types 0 and 1; then per list entry its read (forward
 *   when orientation is 1, else reverse-complemented): its last distPrevious bases when distPrevious <= L, else (a GAP) distPrevious - L times 'N' and the whole read --
 *   1 to gap_count, distPrevious - L to n_count --; then the last nextDistance bases of the `to` read, forward for types 1 and 3, else reverse-complemented, where
 *   nextDistance is the last entry's distNext, or len[h] without a list.  Kept quirks: nextDistance > L(to) copies nothing (the reference's unsigned loop start wraps,
 *   :696) and those positions stay 'N'; when distPrevious's sum + nextDistance != len[h] the edge counts as `inconsistent`, characters beyond the string are dropped
 *   and positions not reached stay 'N' (the reference writes out of bounds there).
 *   TRIM (:699-724): both degrees 1: the whole string; only from's: start 0, contig_length = L(from) + (len - L(to) / 2); only to's: start = L(from) - L(from) / 2,
 *   contig_length = start + len; neither: start likewise, contig_length = start + (len - L(to) / 2).  Where len < L(to) / 2 the reference's unsigned subtraction wraps:
 *   HERE contig_length = 0, the row is left out of the file and counts as `wrapped` (a deliberate difference).
 *   FILE (:726-742): a record for every row with contig_length >= threshold: the header of :730, then string[start, start + contig_length) in lines of 60 -- cut at
 *   the string's end as substr cuts it (start + contig_length passes it by one when L(from) is odd).  The ordinal is the row's position in the table, from 1; gapCount
 *   and nCount in the header are the reference's running totals over all rows so far, written or not (:668-669 never resets them); flow= as an ostream writes a float.
 *   STATISTICS (:745-783) from genome_size: N_X adds contig_length row by row; N50 / N90 are the contig_length and ordinal of the first row with N_X >= genome_size / 2
 *   resp. genome_size * 9 / 10 (genome_size = 0: the first row, as in the reference); covered = base_pair_covered, the sum of len over the rows; longest =
 *   contig_length of row 1.
 * A loop that a graph file holds twice is one edge here (sage2ov_graph_load_composite) and one row; the reference's loader makes two edges of it, and two rows. */
typedef struct sage2ov_contig {        /* 48 bytes */
    uint32_t from, to;
    uint32_t pair;                     /* ordinal of the record pair in sage2ov_graph4_save's order, as in sage2ov_read_edge */
    uint32_t edge_length, string_length, contig_length, start;
    uint32_t gap_count, n_count;       /* of this row (the file's header carries running totals) */
    float    flow;
    uint8_t  type;
    uint8_t  pad[7];
} sage2ov_contig;
typedef struct sage2ov_contig_stats {  /* of the last sage2ov_contigs_build; spell_ms grows with every string spelled since */
    uint64_t contigs, written, bases, longest;      /* rows; rows with contig_length >= threshold; their summed contig_length; contig_length of row 1 */
    uint64_t n50, n50_ordinal, n90, n90_ordinal;
    uint64_t covered, gaps, n_bases, inconsistent, wrapped;
    double   select_ms, sort_ms, layout_ms, spell_ms;          /* HIP events; spell_ms: the spelling kernel alone */
} sage2ov_contig_stats;
/* builds the table and where every string begins, in HBM; spells nothing.  SAGE2OV_ERR_ARG without a step-4 graph, SAGE2OV_ERR_DEVICE on a device-less context,
 * SAGE2OV_ERR_LIMIT for a string of 2^32 characters or 2^36 in all.  The table goes with the graph and the read set and when the flows change; the calls below build it
 * when it is stale, with the threshold and genome size of the last build (0, 0 before any).  Not sharded: a context with world > 1 behaves as a single one. */
int sage2ov_contigs_build(sage2ov_ctx* ctx, uint32_t threshold, uint64_t genome_size);
int sage2ov_contigs_count(sage2ov_ctx* ctx, uint64_t* n, uint64_t* total_string_bases);
/* the rows in table order; cap below their number: SAGE2OV_ERR_ARG, nothing written */
int sage2ov_contigs_export(sage2ov_ctx* ctx, sage2ov_contig* out, uint64_t cap);
/* the whole strings of rows [first, first + count), one after the other, and count + 1 offsets into `out`.  cap below their summed length, or a range outside the table:
 * SAGE2OV_ERR_ARG, nothing written.  The device buffer has the size of the range (every row rounded up to 16 bytes): the caller bounds the memory by the range. */
int sage2ov_contigs_sequences(sage2ov_ctx* ctx, uint64_t first, uint64_t count, char* out, uint64_t cap, uint64_t* offsets);
/* P_contig.fasta (is_scaffold 0) or P_scaffold.fasta's text (1: ">scaffold_"), spelled in ranges of at most SAGE2OV_CONTIG_RANGE_BYTES (a longer string is a range
 * of its own); a range is formatted while the next one is spelled */
#define SAGE2OV_CONTIG_RANGE_BYTES (64u << 20)
int sage2ov_contigs_save(sage2ov_ctx* ctx, const char* path, int is_scaffold);
int sage2ov_contig_stats_get(const sage2ov_ctx* ctx, sage2ov_contig_stats* out);

/* ---- the first loop of ContigExtender::extendContigs (matePair/mergeContigs.cpp:47-60): findMatepairSupports as a whole (:959-1030) -- the sweep above, the selection
 * of mergeByMatepairSupports (:1112-1255) and mergeEdgesAndUpdate (:1260-1469) applied on the device to the resident step-4 graph -- run until a round
 * merges nothing.  findPathSupports and findPathSupportsNew (:62-99) are PATH SUPPORTS, below; mergeShortOverlaps (:101-110) is SHORT OVERLAPS, after step 7's block, whose selection it shares.
 *   MERGE (e1, e2), e1 entering a node and e2 leaving it (mergeEdgesAndUpdate, overlapGraph.cpp:165-186, :259-266, :299-336): refused (no error, nothing changes) when
 *   e1 == e2, e1 == e2's twin, either is dead, or combinedEdgeType is -1 -- the valid rows are (e1 type, e2 type) -> (0,0) 0, (1,2) 0, (0,1) 1, (1,3) 1, (2,0) 2, (3,2) 2,
 *   (2,1) 3, (3,3) 3.  isReducible is 1 on every edge the loader, step 4 and a merge make (insertEdge sets it, nothing here clears it): no field is carried.
 *   flow = 0 when both operands' flows are 0, else 1.0 for type_of_merge 1, else min(e1.flow, e2.flow) (type 2), read from e1's and e2's own floats.  The new edge
 *   e1.from -> e2.to has type combinedEdgeType, length e1.len + e2.len (twin: e1.twin.len + e2.twin.len), `flow` on both halves, and the list getListOfReads(e1, e2):
 *   e1's entries, one entry for the shared node {read = e1.to, orientation = 1 iff e1's type is 1 or 3, flag 0, distPrevious = distNext of e1's last entry (e1.len
 *   when e1 has no list), distNext = distPrevious of e2's first entry (e2.len without a list)}, e2's entries; the twin's list is getListOfReads(e2.twin, e1.twin).
 *   Then for e1 and for e2: own flow <= `flow`: both halves are deleted; else both halves lose `flow`, each its own float.
 *   The new halves are the newest of their nodes (insertIntoList): they go to the end of the half-edge pool, forward half first, dead halves stay dead in place, and
 *   sage2ov_graph4_save's order (node ascending, then pool order) is the reference's file order: a new pair comes after every older pair written at min(from, to).
 *   A ROUND (findMatepairSupports(minOverlap = the context's k, high_threshold)): LIST = the supports table's entries with support > 1 as {edge1 = the twin of the
 *   in-half, edge2 = the out-half, support}, built node ascending, in-half newest first (descending pool index), out-half likewise.  SEARCH maps the key
 *   (edge1.from ^ edge1.to, edge2.from ^ edge2.to) -- an XOR: distinct pairs can share a key -- to the support of the first entry with the largest support (:1005-1012).
 *   Every entry is filed under its four end nodes (deleteList).  The list is ordered by support descending.  For each entry in order (:1125-1248): skip when its key
 *   is not in SEARCH; skip when node = edge1.to is BLOCKED (nodeSearch); stop at the first support < high_threshold.  Over the node's alive halves v, newest first,
 *   with flow >= 1, a list and from != to, as the graph is now: ins = the twins v' != edge1 that match edge2, outs = the v != edge2 that edge1 matches (match(x, y):
 *   combinedEdgeType(x, y) != -1, matchEdgeType :392).  inSupp = SEARCH[key(in), key(edge2)], else SEARCH[key(edge2), key(in)] (the mirrored pair of twins has
 *   the same XOR values, swapped), else 0; outSupp likewise for (edge1, out).  Any of them > low_threshold: no merge.  Otherwise the `to` of every alive non-loop half
 *   of the node is BLOCKED and MERGE(edge1, edge2, 1) runs; when it is not refused, every entry filed under the node leaves SEARCH.
 *   Within a round no selection reads what an earlier merge of the round changed (both ends of a merged edge and all other neighbours of its node are blocked), so the
 *   selection is a serial pass on the host over the table and the half-edge fields (from, to, type, flow, list length, alive -- never a read list), and the merges
 *   of a round are edge-disjoint and go to the device as one batch.  (Should a selection name an edge an earlier merge of the round made or used, the batch so far is
 *   applied first.)
 *   THE INSERT BOUNDS are those of the last sage2ov_mates_estimate: a merge drops the read-to-edge table, supports, links, contigs and step 5's network -- the next call
 *   that needs one rebuilds it from the merged graph -- but mean, deviation, bounds and maximumUpperBoundOfInsert stay until the caller estimates again (or the mates,
 *   the read set or the graph are replaced).  Without an estimate, a round estimates once before its sweep.
 * DELIBERATE DIFFERENCES: (1) std::sort leaves the order of equal supports open; HERE ties keep the order the list is built in (node ascending, in-half newest first,
 * out-half newest first).  Equality with findMatepairSupports is claimed when no round holds two entries of equal support >= high_threshold; with ties, with the
 * reference's mergeByMatepairSupports handed the list in this order.  (2) :1233 reads edge1->ID after mergeEdgesAndUpdate may have freed edge1; HERE the erase key is
 * always the node.  Equality is claimed for rounds in which no merge deletes its in-edge while another entry at the same node is still listed.  (3) An entry whose key
 * is listed through an XOR collision but whose edges are dead is skipped (the reference reads freed memory).  (4) The mate flags describe the merged graph after
 * the table is rebuilt; the reference keeps those of meanSdEstimation.  The first loop does not read them; PATH SUPPORTS, below, reads the copy kept with the estimate. */
typedef struct sage2ov_merge {         /* one merge of the last round, 40 bytes */
    uint32_t node, from, to;           /* the shared node; the new edge's ends (edge1.from, edge2.to) */
    uint32_t support;
    uint32_t pair_in, pair_out;        /* ordinals of edge1's and edge2's record pairs in sage2ov_graph4_save's order BEFORE the round (0xFFFFFFFF: made within it) */
    uint32_t pair_new;                 /* ordinal of the new pair AFTER the round (0xFFFFFFFF: a later merge of the round used it up) */
    float    flow;                     /* of the new edge */
    uint8_t  type, in_deleted, out_deleted, pad[5];
} sage2ov_merge;
typedef struct sage2ov_extend_counts {
    uint64_t entries;                  /* list entries (support > 1) */
    uint64_t at_threshold;             /* of those, support >= high_threshold */
    uint64_t refused;                  /* entries reached whose inSupp or outSupp exceeded low_threshold */
    uint64_t blocked;                  /* entries skipped because their node was blocked */
    uint64_t merges;
    uint64_t entries_copied;           /* entries written to new lists (both lists of every merge) */
    uint64_t pairs_deleted;            /* operand pairs deleted */
    uint64_t batches;                  /* device batches (1 per round with a merge unless a selection named an edge of the round) */
    double   sweep_ms, select_ms, lists_ms, commit_ms;      /* HIP events; select_ms: host wall time */
} sage2ov_extend_counts;               /* 96 bytes */
typedef struct sage2ov_extend_stats { uint64_t rounds, reserved; sage2ov_extend_counts last, total; } sage2ov_extend_stats;      /* 208 bytes; total: since the graph was made or loaded */
/* the primitive: MERGE for a batch.  Operand i is e1 = the record (first_reversed[i] == 0) or the twin (1) of record pair pair_first[i] in sage2ov_graph4_save's order
 * (the ordinals of sage2ov_read_edge and sage2ov_support; a loop is written twice and either ordinal names it, the record being the half written first there), e2 likewise from pair_second / second_reversed; type_of_merge 1 or 2.  merged[i] (may be NULL) = 1, or 0 for a refused merge.
 * New pairs are created in batch order.  SAGE2OV_ERR_ARG, nothing changed: an ordinal out of range, a pair named twice in the batch, e1.to != e2.from, a null array,
 * another type_of_merge, no step-4 graph.  SAGE2OV_ERR_LIMIT, nothing changed: a simple operand (no list) whose length or twin length is above 2047, the 11-bit field
 * of a list entry; half-edges or list entries beyond the pools' 32-bit limits.  SAGE2OV_ERR_DEVICE on a device-less context.  Before the first merge on a graph the
 * genome size is estimated if it is not (sage2ov_graph6_save writes that header).  Not sharded: a context with world > 1 behaves as a single one. */
int sage2ov_graph_merge_pairs(sage2ov_ctx* ctx, const uint32_t* pair_first, const uint8_t* first_reversed, const uint32_t* pair_second, const uint8_t* second_reversed,
                              uint64_t n, int type_of_merge, uint8_t* merged);
/* :43-54, float for float: coverage = (float)((reads * average_read_length) / genome_size) (integer division), high = (int)ceilf((0.20 * coverage) * (100.0 /
 * average_read_length)); with genome_size > 10^9 the factor is 0.10 in iterations 4-6 and 0.05 from 7 on.  Host only.  genome_size or average_read_length 0,
 * iteration 0: SAGE2OV_ERR_ARG (the reference divides by zero). */
int sage2ov_extend_threshold(uint64_t reads, uint64_t average_read_length, uint64_t genome_size, uint32_t iteration, int* high_threshold);
/* one round; *merged (may be NULL) = its merges */
int sage2ov_extend_round(sage2ov_ctx* ctx, int high_threshold, int low_threshold, uint64_t* merged);
/* the loop of :47-60 with low_threshold 1 (main.cpp:357): rounds until one merges nothing; *rounds counts that one too.  genome_size 0: the value sage2ov_graph5_save
 * would write (estimated when it is not); reads and average read length are that file's other two header values.  A genome size or average read length of 0:
 * SAGE2OV_ERR_ARG.  After 10 000 rounds: SAGE2OV_ERR_INTERNAL. */
int sage2ov_extend_by_supports(sage2ov_ctx* ctx, uint64_t genome_size, uint64_t* rounds, uint64_t* merged);
/* the merges of the last round in selection order; cap below their number: SAGE2OV_ERR_ARG, nothing written */
int sage2ov_extend_merges_count(const sage2ov_ctx* ctx, uint64_t* n);
int sage2ov_extend_merges_export(const sage2ov_ctx* ctx, sage2ov_merge* out, uint64_t cap);
int sage2ov_extend_stats_get(const sage2ov_ctx* ctx, sage2ov_extend_stats* out);
/* P.graph6: saveOverlapGraphInFile of the graph as it now is.  sage2ov_graph5_save's text, except that after a merge line 1 and line 2 stay what sage2ov_graph5_save
 * would have written before the first merge (the reference's genomeSize and numberOfReads do not change in step 6); on a graph without a merge it is an alias.
 * It serves after sage2ov_graph_join_pairs and the scaffold rounds too: the resident graph with the same two header lines (the reference has no file for that state). */
int sage2ov_graph6_save(sage2ov_ctx* ctx, const char* path);

/* ---- PATH SUPPORTS: the second and third loop of ContigExtender::extendContigs (matePair/mergeContigs.cpp:62-99): findPathSupports (:118-353) with mergeByPathSupports
 * (:794-952) and findPathSupportsNew (:2148-) with mergeByPathSupportsNew (:2388-2546), on the device.  They extend contigs past forks whose branches
 * are too short to carry their own mates: a mate pair votes for the consecutive edge pairs that every feasible path between its two reads has in common.  All citations
 * are matePair/mergeContigs.cpp; all quantities are integers except flows.  Equality is with the reference at ONE thread (its flag[] array is raced with more).
 *   ESTIMATE FLAGS.  MatePairInfo::flag is cleared by mapReadsToEdges when both mates have an entry for one edge (matePair.cpp:461-481) and never set again: after merges it
 *   still describes the graph of meanSdEstimation.  HERE a copy of every library's flags as of the last sage2ov_mates_estimate is kept with the estimate (it survives
 *   merges and goes when the estimate goes); sage2ov_mates_flags_export keeps describing the graph as it now is.
 *   CLAIM (:190-216).  For every alive half-edge h with a list, walk the list with the running sum of distPrevious and stop at the first entry whose sum is above
 *   maximumUpperBoundOfInsert.  Every entry walked offers its read the node min(from[h], to[h]); claim[r] is the smallest node offered, or none.  No uniqueness test, no flow.
 *   START NODES of node i (:220-239): both end nodes of every record pair for which a read claimed by i has a read-to-edge entry, each once, HERE in ascending order.
 *   PATHS of node i (exploreGraph :359-387, checkFlow :403-415, savePath :420-429): a depth-first walk from each start node s.  Level 1 takes the alive halves v leaving s
 *   that have a list and flow > 0 and saves [v] with length 0.  Level L <= 7 appends an alive v leaving the previous edge's end when matchEdgeType(prev, v) holds, checkFlow
 *   holds -- with uses = the number of times v or its twin already stands in the path: uses <= flow[v] for a v without a list, uses < flow[v] for one with a list, the flow
 *   being v's own float -- and len_before(prev) + len[prev] < maximumUpperBoundOfInsert (strict).  Every extension is saved with path length = the summed lengths of all
 *   its edges but the last.  Adjacency is newest first.  A call at any level returns at once when the node's saved paths so far exceed 1000 (:362); the count is shared by
 *   all start nodes of i, and a call that has begun still saves one path per remaining sibling.
 *   PAIR VOTES (:254-300, findPathsBetweenMatepairs :539-670, insertPath :699-743).  A mate entry (m1 -> m2, type1, type2, library L) votes at node i = claim[m1] when its
 *   estimate flag is 1, L is valid, claim[m2] is none or greater than i (equal claims do not vote; the mirrored entry votes from its side only when claim[m2] < claim[m1]),
 *   and m1 is UNIQUE ON its pair p1 and m2 on p2 (:1102-1110, as for sage2ov_mates_supports: that includes that neither read is a node with an alive edge).  The four
 *   combinations are taken in the order of :565-586, edge1 in {E(p1), its twin}, edge2 in {E(p2), its twin}.  For each: d1 = the locations of m1 on the twin of edge1, d2 =
 *   those of m2 on edge2 (findDistanceOnEdge), both non-empty.  The QUALIFYING PATHS are the saved paths of node i that start at node to[edge1], have a first edge that
 *   matchEdgeType(edge1, .) accepts and end in the half edge2 itself, and for which some x in d1, y in d2 have lower[L] < D < upper[L] (both strict), D = |x| + |y| + path
 *   length when s1 * x < 0 and s2 * y < 0, else D = 100 000 (the reference's initial value, :614: it matters only for a library with upper[L] > 100 000).  Each qualifying
 *   path is read as the edge sequence edge1, path[1..n].  The entry's SURVIVORS are the consecutive pairs (a, b) of the first qualifying path that occur in every other
 *   qualifying path, over all four combinations, as (a, b) or as (twin of b, twin of a).  No qualifying path, or no survivor: no vote.  Each survivor gets +1, once per
 *   mate entry whatever its count.
 *   THE TABLE: one row per ordered pair of halves (a enters a node, b leaves it) with votes >= 1, in ascending (node, a newest first, b newest first).
 *   A ROUND (variant 0: mergeByPathSupports, 1: mergeByPathSupportsNew).  SEARCH maps the XOR key of :283-284 to the summed support of the rows that share it; every row is
 *   filed under its four end nodes.  For each row in ORDER: skip when its key has left SEARCH; skip when node = to[a] is BLOCKED; skip (no stop) when support < high;
 *   otherwise over the node's alive halves v with flow >= 1 and from != to (no list is required, :837): ins = the twins v' != a that match b, outs = the v != b that a
 *   matches, inSupp / outSupp from SEARCH with the mirrored fall-back of :859-871, uniqueIn / uniqueOut = none above low.  Variant 0 merges when both are unique,
 *   variant 1 when at least one is (:2504).  A merge blocks the `to` of every alive non-loop half of the node and runs MERGE(a, b, 1) of the first loop; when it is not
 *   refused, every row filed under the node leaves SEARCH.  The merges of a round go to the device as one batch, as for sage2ov_extend_round; the estimate and its
 *   flags stand.
 *   LOOPS (:62-99): rounds with the thresholds of sage2ov_extend_threshold by iteration, low 1, until a round merges <= stop; stop = 10 when genome_size > 10^9, else 0.
 * DELIBERATE DIFFERENCES, each with a counter that is 0 where equality is claimed: (1) ORDER (order_dependent): the reference walks an unordered_map in bucket order; HERE
 * rows go by support descending, ties in table order.  Equality is claimed for rounds in which the rows with support >= high sit at pairwise different nodes and none of
 * those nodes is an end of another such row's halves.  (2) XOR keys (key_collisions = rows - distinct keys): the reference's map holds one entry per key with the edges
 * of the last writer; HERE rows are exact.  (3) Cap (capped_nodes): the reference explores start nodes in the order of its linked lists, HERE ascending; it matters only
 * for a node that saves more than 1000 paths (the reference's path array has 2000 rows and no check; HERE the pool is sized by a counting pass).  (4) Mirror (mirrored):
 * which path comes first follows an unstable quicksort (:434-478) in the reference, HERE enumeration order; the survivors are the same set, their orientation can differ
 * only when a survivor was matched through its mirrored form: mirrored counts the survivors that some qualifying path held in the mirrored form only. */
typedef struct sage2ov_path_support {  /* 28 bytes */
    uint32_t node;                     /* a enters it, b leaves it */
    uint32_t pair_a, pair_b;           /* ordinals of the record pairs in sage2ov_graph4_save's order, as in sage2ov_read_edge */
    uint32_t from_a, to_b;             /* the far ends */
    uint32_t support;
    uint8_t  second_a, second_b;       /* 0: the half is the record sage2ov_graph4_save writes first of its pair (the first time, for a loop); 1: it is that record's twin */
    uint8_t  pad[2];
} sage2ov_path_support;
typedef struct sage2ov_path_stats {    /* of the last sage2ov_path_supports: they stand until the next sweep, through the merges that drop its table; order_dependent: of the
                                          last sage2ov_extend_paths_round since that sweep */
    uint64_t claimed_reads, claiming_nodes, start_nodes;      /* start_nodes: (claiming node, start node) pairs */
    uint64_t paths, capped_nodes;
    uint64_t eligible_entries, voting_entries;                /* mate entries that pass the five conditions; of those, the ones with a survivor */
    uint64_t records, rows;                                   /* survivors (the sum of all supports); distinct (a, b) */
    uint64_t key_collisions, mirrored, order_dependent;
    uint32_t sort_passes, reserved;                           /* 8-bit radix passes run */
    double claim_ms, starts_ms, walk_ms, vote_ms, sort_ms, reduce_ms;      /* HIP events */
} sage2ov_path_stats;                  /* 152 bytes */
/* builds the table.  Estimates first when there is no estimate (a rebuilt read-to-edge table after a merge leaves the estimate alone).  SAGE2OV_ERR_ARG without a step-4
 * graph, SAGE2OV_ERR_DEVICE on a device-less context, SAGE2OV_ERR_LIMIT from 2^32 - 2048 records, paths or start records on, or a maximumUpperBoundOfInsert of 2^31.  The
 * table goes when the supports table of sage2ov_mates_supports would; _count / _export build it when it is stale.  After sage2ov_graph_simplify every flow is 0: no path
 * has a first edge, the table is empty, which is no error.  Not sharded: a context with world > 1 behaves as a single one. */
int sage2ov_path_supports(sage2ov_ctx* ctx);
int sage2ov_path_supports_count(sage2ov_ctx* ctx, uint32_t min_support, uint64_t* n);
/* the rows with support >= min_support in table order; cap below their number: SAGE2OV_ERR_ARG, nothing written */
int sage2ov_path_supports_export(sage2ov_ctx* ctx, uint32_t min_support, sage2ov_path_support* out, uint64_t cap);
int sage2ov_path_stats_get(const sage2ov_ctx* ctx, sage2ov_path_stats* out);
/* one round; variant 0 or 1 (else SAGE2OV_ERR_ARG); *merged (may be NULL) = its merges.  It fills the "last round" of sage2ov_extend_merges_count / _export and
 * sage2ov_extend_stats_get: entries = rows, at_threshold = rows with support >= high, refused, blocked, merges and the batch figures as for sage2ov_extend_round. */
int sage2ov_extend_paths_round(sage2ov_ctx* ctx, int high_threshold, int low_threshold, int variant, uint64_t* merged);
/* one of the two loops; *rounds counts the round that ends it too.  genome_size 0, reads and average read length: as for sage2ov_extend_by_supports.  After 10 000
 * rounds: SAGE2OV_ERR_INTERNAL. */
int sage2ov_extend_by_paths(sage2ov_ctx* ctx, uint64_t genome_size, int variant, uint64_t* rounds, uint64_t* merged);

/* ---- step 7, ScaffoldMaker::makeScaffolds (matePair/scaffolding.cpp:31-98): the rounds of mergeFinal (:774-967) and mergeFinalSmall (:969-) -- the sweep of
 * sage2ov_links above, the selection of mergeAccordingToSupport (:488-626) / mergeAccordingToSupport2 (:631-769) and mergeDisconnectedEdges (:281-482) applied on the
 * device to the resident step-4 graph.  All citations without a file are matePair/scaffolding.cpp.
 *   OVERLAP(s1, s2, L1, L2) (stringOverlapSize, overlapGraph.cpp:884-907): the smallest i in [0, L1 - 10) with L2 - i >= 0 for which the number of j in [0, L2 - i) with
 *   s1[i + j] != s2[j] is at most (L2 - i) / 10 + 1 (the early break of :895 does not change that); -1 when there is none.  A position i + j >= L1 is a mismatch: the
 *   reference reads past its string there, so equality with it is claimed for L2 <= L1 only.
 *   JOIN(e1, e2, gap), e1 and e2 alive halves of different pairs, both with a list, sharing a node or not (mergeDisconnectedEdges; nothing is refused, the type is
 *   never -1): type = 0 / 1 / 2 / 3 for (e1's type in {0, 1}, e2's in {0, 2}) / ({0, 1}, {1, 3}) / ({2, 3}, {0, 2}) / ({2, 3}, {1, 3}) (:290-297).  The new edge e1.from ->
 *   e2.to has flow 1.0 on both halves and two lists made each on its own, LIST(e1, e2, gap) for the forward half and LIST(e2.twin, e1.twin, gap) for the twin, each with
 *   its own length (getListOfReadsInDisconnectedEdges, overlapGraph.cpp:789-882).  LIST(x, y, gap): node1 = x.to spelled forward iff x's type is 1 or 3, node2 = y.from
 *   spelled forward iff y's type is 2 or 3 (else the reverse complement), L1 and L2 their read lengths, P = distNext of x's last entry, Q = distPrevious of y's first.
 *     node1 == node2: x's entries, {node1, orientation = spelled forward, flag 0, distPrevious P, distNext Q}, y's entries; length x.len + y.len.  (The reference
 *     leaves the flag of the entries it inserts uninitialised; HERE it is 0.)
 *     otherwise: x's entries, {node1, .., P, D1}, {node2, .., D2, Q}, y's entries; length x.len + y.len + D1, with o = OVERLAP(spelling of node1, spelling of node2, L1, L2):
 *       o > 0: D1 = D2 = o.   o == 0 and o == -1 alike (:837 tests len > 0): gap < 0: D1 = L1, D2 = L2 (concatenated); gap >= 0: D1 = gap + L1, D2 = gap + L2 (N's).
 *     The entry's distances are 11-bit fields (overlapGraph.h:20-21): D1, D2 above 2047 wrap in the entry, in the reference and here alike; the length takes D1 whole.
 *   Then for e1 and for e2: own flow <= 1.0 (0 included): both halves are deleted; else both halves lose 1.0, each its own float (:301-386).
 *   The new halves go to the end of the half-edge pool, forward half first, in batch order.
 *   A ROUND (high, flag 1 or 2, small): ROWS = for every LINK(a, b) of the table above that passes SAGE2OV_LINKS_FINAL (small: SAGE2OV_LINKS_SMALL) and has a < b as
 *   half-edge pool indices: {edge_1 = a's twin, edge_2 = b, support, gap}, in the table's export order.  SEARCH maps (edge_1.from ^ edge_1.to, edge_2.from ^ edge_2.to) to
 *   the support of the first row with the largest support of that key (:904-911); every row is filed under its four end nodes (:913-916).  The rows are ordered by
 *   support descending, then edge_1.len + edge_2.len descending (:252-275).  For each row in order: SKIPPED when its key is not in SEARCH (:504-506); BELOW when its
 *   support < high (no break, :508); else with FEASIBLE(p) = the pairs that share a row of the unfiltered table (either direction, any halves) with pair p at the
 *   start of the round, less the SPENT pairs, and nothing at all when p is spent: count2 = the q in FEASIBLE(pair(edge_1)) with SEARCH[x(edge_1), x(q)], else SEARCH[x(q),
 *   x(edge_1)], else 0, >= high -- leaving out q == pair(edge_2) when edge_2 is E of its pair (the reference compares the pointer the read-to-edge table holds, :565);
 *   count1 likewise over FEASIBLE(pair(edge_2)) with SEARCH[x(q), x(edge_2)], else SEARCH[x(edge_2), x(q)], leaving out pair(edge_1) when edge_1 is E; CYCLE when one q
 *   counts on both sides (:580-600).  count1, count2 <= 1 (flag 2: <= 2) and no cycle: JOIN(edge_1, edge_2, gap), both pairs become SPENT, and every row filed under
 *   edge_1.to leaves SEARCH (:607-614); otherwise the row is a CYCLE or BLOCKED.
 *   THE LOOPS (:31-98) with coverage = (float)((reads * averageReadLength) / genomeSize) (an integer quotient), T(f) = (int)ceilf((f * coverage) * (100.0 /
 *   averageReadLength)): loop 1: rounds of flag 1 at T(0.10), from iteration 6 on at T(0.05), until a round merges nothing at high == T(0.05); loop 2: the same with
 *   flag 2; loop 3: flag 1 at high 2 until a round merges nothing; loop 4: flag 1 at high 1; loop 5: flag 2, small, at high 1.
 * WHAT THE CONTRACT SETTLES: (a) the reference evaluates (a, b) only when a's Edge object lies at or below b's in memory (:828, :1023); LINK(a, b) and LINK(b, a) propose the
 * same join (b.twin . a is the twin of a.twin . b) with possibly different support and gap.  HERE the row of {a, b} is LINK(a, b) with a < b as pool indices and no row
 * comes from the other direction, even when only that one has support; on a freshly loaded graph this is what malloc order gives the reference.  (b) Ties of the sort
 * (open in the reference's quicksort) keep the table's export order.  (c) The reference takes getListOfFeasibleEdges (:148-234) from the read-to-edge table as the
 * merges of the round have changed it.  After a join the reads of both operands lie on the new edge alone (operand deleted) or on two edges (operand kept): unique
 * on no operand.  HERE an operand pair of an earlier join of the round is SPENT; a new edge is feasible but has no SEARCH entry of its own and is left out (an XOR
 * collision could give it one in the reference).  Feasible pairs without any row of the unfiltered table cannot reach SEARCH except through such a collision and
 * are left out too.  (d) A row that names a half an earlier join of the round deleted is skipped (the reference reads the freed Edge, :502); the erase key is the node
 * edge_1.to as read before the join (:607 reads it after, from an Edge the join may have freed: a join that deletes edge_1 while other rows filed under that node are
 * still in SEARCH is outside the reference too); the round is marked outside_reference from such a row or join on.  (e) A kept operand (flow above 1) may be named
 * again by a later row: the batch so far is applied first (`batches`).
 * The selection is a serial pass on the host over the exported table and the half-edge fields; the joins of a round go to the device as a batch and no read list
 * is downloaded.  A join drops the read-to-edge table, supports, links, contigs and step 5's network; the insert estimate stands, as for sage2ov_extend_round. */
typedef struct sage2ov_join {          /* one join of the last scaffold round, 48 bytes */
    uint32_t from, to;                 /* the new edge's ends (edge_1.from, edge_2.to) */
    uint32_t support; int32_t gap;
    uint32_t pair_first, pair_second;  /* ordinals of edge_1's and edge_2's record pairs in sage2ov_graph4_save's order BEFORE the round (the rows are older than the edges a round makes) */
    uint32_t pair_new;                 /* ordinal of the new pair AFTER the round */
    int32_t  overlap_forward, overlap_twin;      /* OVERLAP of the forward and of the twin list; -2: equal end nodes, no search */
    uint8_t  type, first_deleted, second_deleted;
    uint8_t  how_forward, how_twin;    /* SAGE2OV_JOIN_* */
    uint8_t  pad[7];
} sage2ov_join;
#define SAGE2OV_JOIN_EQUAL 0           /* node1 == node2: one entry */
#define SAGE2OV_JOIN_OVERLAP 1         /* OVERLAP > 0 */
#define SAGE2OV_JOIN_CONCAT 2          /* no overlap, gap < 0 */
#define SAGE2OV_JOIN_GAPPED 3          /* no overlap, gap >= 0 */
typedef struct sage2ov_scaffold_counts {
    uint64_t rows, below_threshold, skipped, blocked, cycles, merged, batches;
    uint64_t overlaps, concatenated, gapped;       /* lists (two per join) by SAGE2OV_JOIN_*; the rest have equal end nodes */
    uint64_t outside_reference;        /* last: 1 when (d) applied -- a row named a deleted half, or a join deleted edge_1 while other rows filed under its node were in
                                          SEARCH --, else 0; total: the number of such rounds */
    uint64_t entries_copied, pairs_deleted;
    double   sweep_ms, select_ms, overlap_ms, lists_ms, commit_ms;      /* HIP events; select_ms: host wall time */
} sage2ov_scaffold_counts;             /* 144 bytes */
typedef struct sage2ov_scaffold_stats { uint64_t rounds, reserved; sage2ov_scaffold_counts last, total; } sage2ov_scaffold_stats;      /* 304 bytes; total: since the graph was made or loaded */
/* the primitive: JOIN for a batch.  Operands as for sage2ov_graph_merge_pairs ((pair ordinal, reversed) in sage2ov_graph4_save's order); gap[i] as a row carries it.
 * overlap (may be NULL): 2 n values, OVERLAP of the forward list and of the twin list of join i (-2: equal end nodes); how (may be NULL): 2 n values SAGE2OV_JOIN_*.
 * New pairs are created in batch order.  SAGE2OV_ERR_ARG, nothing changed: an ordinal out of range, a pair named twice in the batch (e1 and e2 of one pair included),
 * an operand without a list, a null array, no step-4 graph, no read store.  SAGE2OV_ERR_LIMIT, nothing changed: a length beyond 32 bits, half-edges or list entries
 * beyond the pools' limits.  SAGE2OV_ERR_DEVICE on a device-less context.  The P.graph6 header is held as for sage2ov_graph_merge_pairs.  Not sharded. */
int sage2ov_graph_join_pairs(sage2ov_ctx* ctx, const uint32_t* pair_first, const uint8_t* first_reversed, const uint32_t* pair_second, const uint8_t* second_reversed,
                             const int32_t* gap, uint64_t n, int32_t* overlap, uint8_t* how);
/* high of THE LOOPS: loop 1..5, iteration from 1.  Host only.  genome_size or average_read_length 0, iteration 0, another loop: SAGE2OV_ERR_ARG. */
int sage2ov_scaffold_threshold(uint64_t reads, uint64_t average_read_length, uint64_t genome_size, uint32_t loop, uint32_t iteration, int* high);
/* one round; flag 1 or 2 (else SAGE2OV_ERR_ARG); small != 0: mergeFinalSmall's filter; *merged (may be NULL) = its joins */
int sage2ov_scaffold_round(sage2ov_ctx* ctx, int high, int flag, int small, uint64_t* merged);
/* the five loops; *rounds counts every round, the empty ones that end a loop too.  genome_size 0, reads and average read length: as for sage2ov_extend_by_supports.
 * After 10 000 rounds: SAGE2OV_ERR_INTERNAL. */
int sage2ov_scaffold(sage2ov_ctx* ctx, uint64_t genome_size, uint64_t* rounds, uint64_t* merged);
/* the joins of the last round in selection order; cap below their number: SAGE2OV_ERR_ARG, nothing written */
int sage2ov_scaffold_merges_count(const sage2ov_ctx* ctx, uint64_t* n);
int sage2ov_scaffold_merges_export(const sage2ov_ctx* ctx, sage2ov_join* out, uint64_t cap);
int sage2ov_scaffold_stats_get(const sage2ov_ctx* ctx, sage2ov_scaffold_stats* out);

/* ---- SHORT OVERLAPS: the fourth loop of ContigExtender::extendContigs (matePair/mergeContigs.cpp:101-110): mergeShortOverlaps (:1474-1648) with mergeShortOverlap
 * (:1788-1908) and mergeDisconnectedEdges1 (:1913-2114), on the device.  It joins contigs whose mates say that they overlap (a summed gap of at
 * most 0) but whose overlap the graph does not hold.  All citations without a file are matePair/mergeContigs.cpp.  Its sweep (:1494-1635) is the sweep of
 * sage2ov_links, its merge is JOIN of step 7, its selection is step 7's with the three changes below; only the raw gap sum is new.
 *   GAPSUM.  The sweep adds Mean[lib] - (distance + 2 averageReadLength) per supporting mate into an int32_t (:1577) that wraps like the reference's; LINK.gap is
 *   gapSum / support truncated towards zero (:1592), so a gapSum of +1 over support 2 has gap 0 and yet fails :1587.  The table keeps both.
 *   A ROUND (high): ROWS = for every LINK(a, b) of the unfiltered table with a < b as half-edge pool indices (rule (a) of step 7, for :1527), flow of E(pair(a)) and
 *   of E(pair(b)) both > 0 (from the host copy, as SAGE2OV_LINKS_FINAL reads them; a graph without flows has no rows), both lengths strictly above
 *   contigLengthThreshold = (int)ceilf(100 * (averageReadLength / 100.0)) (:21, :1500: there is no "> 200" alternative here) and gapSum <= 0 (:1587):
 *   {edge_1 = a's twin, edge_2 = b, support, gap = gapSum / support}, in the table's export order.  SEARCH, the filing under four end nodes, the sort (:2119-2142),
 *   SKIPPED, BELOW, FEASIBLE from the unfiltered table, SPENT, count1, count2 and rules (b)-(e) are those of step 7's ROUND.  A row joins iff count1 == 0 and
 *   count2 == 0 (:1858-1878: any rival at or above high on either side); there is no cycle test, a rival on both sides is BLOCKED like any other and `cycles` stays 0.
 *   JOIN(edge_1, edge_2, gap) then runs as a batch on the device.  gapSum <= 0 gives gap <= 0: without an overlap a negative gap concatenates and a gap of 0
 *   takes the `gap >= 0` branch of getListOfReadsInDisconnectedEdges: SAGE2OV_JOIN_GAPPED with D1 = L1, D2 = L2, no N.
 *   Equality with the reference is claimed for high >= 1, under the conditions of step 7's contract (outside_reference 0, no ties of the sort).  For high <= 0
 *   the round does what sage2ov_scaffold_round does with such a value: no row is BELOW, and a missing SEARCH entry counts as a rival of support 0 on edge_1's side
 *   (count2) while it is no rival on edge_2's side; the reference's own loop passes no negative value, and 0 only when the coverage quotient is 0.
 *   THE LOOP (:101-110): rounds at high = (int)ceilf((0.05 * coverage) * (100.0 / averageReadLength)), coverage as in sage2ov_extend_threshold, whatever the genome
 *   size, until a round joins nothing.
 * The records and totals of these rounds are kept apart from step 7's: sage2ov_scaffold_merges_* and sage2ov_scaffold_stats_get do not see them. */
/* gapSum of exactly the rows sage2ov_links_export(mode, min_support) returns, in the same order.  Errors as for that call; builds the table when it is stale. */
int sage2ov_links_gap_sums(sage2ov_ctx* ctx, uint32_t mode, uint32_t min_support, int32_t* out, uint64_t cap);
/* high of THE LOOP.  Host only.  genome_size or average_read_length 0: SAGE2OV_ERR_ARG. */
int sage2ov_extend_short_threshold(uint64_t reads, uint64_t average_read_length, uint64_t genome_size, int* high);
/* one round, mergeShortOverlaps(k, high); *merged (may be NULL) = its joins.  Errors as for sage2ov_scaffold_round. */
int sage2ov_extend_short_round(sage2ov_ctx* ctx, int high, uint64_t* merged);
/* THE LOOP; *rounds counts the empty round that ends it too.  genome_size 0, reads and average read length: as for sage2ov_extend_by_supports.  After 10 000
 * rounds: SAGE2OV_ERR_INTERNAL. */
int sage2ov_extend_by_short_overlaps(sage2ov_ctx* ctx, uint64_t genome_size, uint64_t* rounds, uint64_t* merged);
/* ContigExtender::extendContigs as a whole (:37-113): sage2ov_extend_by_supports, sage2ov_extend_by_paths variant 0, then variant 1, then
 * sage2ov_extend_by_short_overlaps; rounds[i] and merged[i] (either may be NULL) are those of loop i, 0 for a loop an error kept from running. */
int sage2ov_extend_contigs(sage2ov_ctx* ctx, uint64_t genome_size, uint64_t rounds[4], uint64_t merged[4]);
/* the joins of the last short-overlap round in selection order, and the counters of these rounds (cycles is always 0) */
int sage2ov_extend_short_merges_count(const sage2ov_ctx* ctx, uint64_t* n);
int sage2ov_extend_short_merges_export(const sage2ov_ctx* ctx, sage2ov_join* out, uint64_t cap);
int sage2ov_extend_short_stats_get(const sage2ov_ctx* ctx, sage2ov_scaffold_stats* out);

/* diagnostic: table census {occupied, inline, claimed-but-unfilled, zero-tag, entries in short CSR buckets} */
int sage2ov_debug_table(sage2ov_ctx* ctx, uint64_t* out5);
/* diagnostic: device memory {free now, total, LOWEST free seen at the library's sampling points since the context was created (end of step 1, the index
 * build's peak, end of the probe pass, reduce, convert), bytes held by the context's grow-only workspace arena}: the high-water mark of a run is
 * total - out[2] when the context is the only user of the GPU */
int sage2ov_debug_meminfo(sage2ov_ctx* ctx, uint64_t* out4);
/* diagnostic: the four index keys (hashTable.cpp:96-104) of every read as the device computes them: 8N u64 (hi,lo per entry) */
int sage2ov_debug_keys(sage2ov_ctx* ctx, uint64_t* out);
/* diagnostic: the directional hit list (economyGraph.cpp:591-633: to, edge type, length) of EVERY read, rows of
 * 5 x u32 {from, to, type, length, sequence-number}, sorted by (from, sequence).  out may be NULL to size. */
int sage2ov_debug_all_hits(sage2ov_ctx* ctx, uint32_t* out, uint64_t cap_rows, uint64_t* n_rows);

/* whole timed region of SURVEY 8(d): index build + initial + reduce + convert, reads already in HBM */
int sage2ov_run_steps23(sage2ov_ctx* ctx);

/* ---- multi-GPU exchange points (one process per GPU; the caller owns the communicator and the
 * collective -- RCCL through torch.distributed or directly -- and hands device buffers in and out).
 * Rank r probes read ids [lo_r, hi_r); the reciprocal test reads the neighbours' records
 * (economyGraph.cpp:460), hence the all-gather of fixed-size per-read records, then of edge buckets. */
int sage2ov_shard_range(const sage2ov_ctx* ctx, uint64_t* lo, uint64_t* hi);          /* ids, hi exclusive */
int sage2ov_shard_record_bytes(const sage2ov_ctx* ctx, uint64_t* bytes_per_read);     /* 16: right and left extension (position:30, type:2, length:22 each), connection count:18, containment flags:2 */
int sage2ov_overlap_probe_shard(sage2ov_ctx* ctx);                                    /* kernel only, own range */
int sage2ov_shard_export_records(sage2ov_ctx* ctx, void* dev_dst, uint64_t max_reads);/* own range -> device buffer */
int sage2ov_shard_import_records(sage2ov_ctx* ctx, const void* dev_src, uint64_t first_id, uint64_t n_reads);
/* containment marks (economyGraph.cpp:735) land on reads of ANY rank: 2*(N+1) bytes (two bit planes) that the
 * caller MAX-all-reduces (= bitwise OR) between export and import */
int sage2ov_shard_flags_bytes(const sage2ov_ctx* ctx, uint64_t* bytes);
int sage2ov_shard_export_flags(sage2ov_ctx* ctx, void* dev_dst);
int sage2ov_shard_import_flags(sage2ov_ctx* ctx, const void* dev_src);
/* reciprocal test for every read (cheap, replicated), edge buckets only for this rank's reads */
int sage2ov_overlap_reciprocal(sage2ov_ctx* ctx);
/* per-rank edge buckets (16-byte records {from,to,len,type}): all-gather counts, then the padded buckets,
 * then hand every rank the concatenation */
int sage2ov_shard_edges_count(const sage2ov_ctx* ctx, uint64_t* n);
int sage2ov_shard_edges_export(sage2ov_ctx* ctx, void* dev_dst, uint64_t cap_edges);
int sage2ov_shard_edges_set(sage2ov_ctx* ctx, const void* dev_src, uint64_t n_edges);

/* Sharded reduce phase (round 3).  On a context with world > 1, sage2ov_overlap_reduce (buildOverlapGraphEconomy, economyGraph.cpp:495-574) builds the hit
 * lists and the adjacency of ALL unresolved reads -- every rank's marks read them -- but runs markTransitiveEdge / removeTransitiveEdges (:643-707) and the
 * re-emission of the surviving edges only for THIS RANK'S SHARE of the unresolved reads (a contiguous part of their list; any cut is exact: a read's marks
 * are a function of the lists).  The survivors of the share are this rank's survivor bucket (16-byte records like the edge buckets): all-gather the buckets,
 * sum `removed_partial` over the ranks, and hand every rank the concatenation before sage2ov_overlap_convert (which refuses to run without it).
 * Where the phase runs replicated (the serial replay for a handful of reads), rank 0's bucket carries everything and the others are empty. */
int sage2ov_shard_survivors_count(const sage2ov_ctx* ctx, uint64_t* n, uint64_t* removed_partial);
int sage2ov_shard_survivors_export(sage2ov_ctx* ctx, void* dev_dst, uint64_t cap_edges);
int sage2ov_shard_survivors_set(sage2ov_ctx* ctx, const void* dev_src, uint64_t n_total, uint64_t removed_total);

/* ---- profiling hooks: HIP-event timings of the last run, milliseconds ---- */
typedef struct sage2ov_timings {
    double index_ms, probe_ms, reciprocal_ms, reduce_ms, convert_ms, total_ms;
    double probe_kernel_ms;      /* the dominant kernel alone (HIP events on the context stream), summed over its launches */
    uint64_t probe_kernel_launches;   /* probe PASSES timed (one per initial pass): probe_kernel_ms / this = kernel time per pass */
    uint64_t sequential_reads;   /* reads the fast kernel handed to the sequential state-machine kernel */
    double organize_ms;          /* step 1 on the device: upload of the staged reads .. organised read store resident (HIP events) */
    uint64_t probe_fast_launches;     /* launches of the fast kernel behind probe_kernel_ms: a pass is a sample launch, the rest of the range
                                         and, if reads were listed, one launch over the list */
    /* what a multi-rank run keeps replicated / shards inside the two phases above (bench.py's scaling model): */
    double reciprocal_cond_ms;        /* the part of reciprocal_ms every rank spends on ALL reads (cond(i), economyGraph.cpp:460); the rest is the emit half, sharded */
    double reduce_marks_ms;           /* the part of reduce_ms spent in the marks + removals + re-emission (economyGraph.cpp:643-707): sharded over the ranks */
} sage2ov_timings;
int sage2ov_timings_get(const sage2ov_ctx* ctx, sage2ov_timings* out);
int sage2ov_timings_reset(sage2ov_ctx* ctx);
/* Run mode of the last probe pass (the launches of one sage2ov_overlap_probe_shard / sage2ov_overlap_initial), counted on the device and copied on this call only:
 * out[0] reads answered off the slot ring, out[1] steps that answered them (a step answers up to 16 consecutive reads), out[2] of those reads: records computed
 * with a lane per read, out[3] such steps.  Zero where the resident reads have no run mode (several lengths, k > 64, noisy data's forms). */
int sage2ov_probe_run_stats_get(sage2ov_ctx* ctx, uint64_t out[4]);
/* Which way the reduce phase went in the last sage2ov_overlap_reduce / sage2ov_run_steps23 (a multi-rank context: this rank's share of the marks).  Every word
 * is a counter the phase keeps anyway, copied on its read-backs:
 * out[0] form: 0 nothing unresolved, 1 symmetric form on the device, 2 ranked form on the device, 3 serial replay on the host; out[1] unresolved reads;
 * out[2] lists of more than 128 entries (handed to the second size class of the marks' kernel); out[3] lists beyond its 512 entries (marked out of global scratch);
 * out[4] neighbour lists the marks' short cut read; out[5] reads whose marks it settled; out[6] removed entries; out[7] potential lists of more than 1024 entries
 * (ranked form: sorted on the host); out[8] slices the potential lists were built in.  out[2..5], [7], [8] are zero in form 3. */
#define SAGE2OV_REDUCE_STATS 9
int sage2ov_reduce_stats_get(sage2ov_ctx* ctx, uint64_t out[SAGE2OV_REDUCE_STATS]);
void* sage2ov_stream(sage2ov_ctx* ctx);   /* hipStream_t the context launches on */

/* ---- deterministic synthetic reads (repo-owned, not part of the reference) ---- */
typedef struct sage2ov_synth_params {
    uint64_t seed;
    uint64_t genome_len;
    uint64_t n_reads;            /* reads, i.e. 2 x pairs; interleaved mate1, mate2 */
    uint32_t read_len;           /* L (max) */
    uint32_t read_len_min;       /* 0 or >= read_len: fixed length; else uniform in [min, L] */
    uint32_t err_ppm;            /* substitution rate, parts per million */
    uint32_t n_repeat_families;  /* planted repeats: families x copies x length */
    uint32_t repeat_copies;
    uint32_t repeat_len;
} sage2ov_synth_params;
int      sage2ov_synth_genome(const sage2ov_synth_params* p, uint8_t* genome /* genome_len codes 0..3 */);
uint32_t sage2ov_synth_read_len(const sage2ov_synth_params* p, uint64_t read_index);
int      sage2ov_synth_reads_ascii(const sage2ov_synth_params* p, const uint8_t* genome, uint64_t first, uint64_t n,
                                   char* bases, uint64_t* offsets /* n+1 */);
int      sage2ov_synth_write_fasta(const sage2ov_synth_params* p, const char* path);
/* generate reads [first, first+n) and feed them through the same filter/canonical/pack path as
 * sage2ov_reads_add_ascii, in parallel on the host, without materialising ASCII */
int      sage2ov_reads_add_synth(sage2ov_ctx* ctx, const sage2ov_synth_params* p, const uint8_t* genome, uint64_t first, uint64_t n);

#ifdef __cplusplus
}
#endif
#endif /* SAGE2OV_H_ */
