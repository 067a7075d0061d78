// sage2_amd/csrc/sage2ov_host.cpp -- host side of the C ABI (include/sage2ov.h).
//
// Step 1 (FASTA/FASTQ parsing, filter, canonical orientation, 2-bit packing, sort, dedupe) runs on the
// host for now and hands the packed unique reads to HBM; steps 2-3 are HIP kernels
// (sage2ov_device.hip).  The exact serial BFS of the reduce phase (economyGraph.cpp:513-564) is
// replayed here from device-computed hit lists.  There is no CPU fallback for the device work.
#include <zlib.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <parallel/algorithm>
#include <string>
#include <thread>
#include <memory>
#include <mutex>
#include <condition_variable>
#include <unordered_map>
#include <unordered_set>
#include <vector>
#include <omp.h>
#include <sched.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include "sage2ov.h"
#include "sage2ov_internal.h"

using namespace s2;

namespace {

thread_local std::string g_create_error;

inline uint64_t rev2_host(uint64_t x) {
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(x);
}
inline uint64_t bits64_host(const uint64_t* w, int nw, int bitpos) {
    int q = bitpos >> 6, r = bitpos & 63;
    uint64_t a = q < nw ? w[q] : 0;
    if (r == 0) return a;
    uint64_t b = q + 1 < nw ? w[q + 1] : 0;
    return (a << r) | (b >> (64 - r));
}
inline uint64_t mask_top_host(int nb) { return nb >= 32 ? ~0ull : (nb <= 0 ? 0ull : (~0ull << (64 - 2 * nb))); }
// reverse complement of an L-base word-packed read (left aligned), nw words in and out
inline void revcomp_words(const uint64_t* in, int nw, int L, uint64_t* out) {
    for (int c = 0; c < nw; c++) {
        int rem = L - 32 * c; uint64_t r;
        if (rem <= 0) r = 0;
        else if (rem >= 32) r = ~rev2_host(bits64_host(in, nw, 2 * (rem - 32)));
        else r = (~rev2_host(in[0] >> (64 - 2 * rem))) & mask_top_host(rem);
        out[c] = r;
    }
}
inline int flip_type_host(int t) { return t == 0 ? 3 : (t == 3 ? 0 : t); }   // utils.cpp:212

struct AdjEdge { uint32_t to; uint8_t type; uint8_t mark; uint32_t len; };

// SAGE2OV_TIMING: wall-clock laps of the host-side stages (file input, step 1, the writers) on stderr
struct HostLap {
    const bool on; const char* stage; std::chrono::steady_clock::time_point tp = std::chrono::steady_clock::now();
    HostLap(const sage2ov_ctx* c, const char* s);
    void operator()(const char* what) { if (!on) return; auto t = std::chrono::steady_clock::now(); fprintf(stderr, "[%s] %-36s %8.1f ms\n", stage, what, std::chrono::duration<double, std::milli>(t - tp).count()); tp = t; }
};

}  // namespace

extern char** environ;
namespace s2 {
Options Options::from_env() {
    Options o;
    for (char** e = environ; e && *e; e++) {
        const char* v = *e;
        if (strncmp(v, "SAGE2OV_", 8) != 0 && strncmp(v, "LOCAL_WORLD_SIZE=", 17) != 0) continue;
        const char* eq = strchr(v, '='); if (!eq) continue;
        o.kv.emplace_back(std::string(v, eq - v), std::string(eq + 1));
    }
    std::sort(o.kv.begin(), o.kv.end());
    return o;
}
}  // namespace s2

struct sage2ov_ctx {
    sage2ov_config cfg{};
    std::string err;
    s2::Options opt = s2::Options::from_env();         // the SAGE2OV_* switches as they were when the context was created (sage2ov_options_reload re-reads them)
    // the device: opened by sage2ov_ctx_create, or (SAGE2OV_FLAG_ASYNC_DEVICE) on a helper thread that the first device() call joins
    mutable Device* dev_ = nullptr; mutable std::thread devOpen; mutable std::string devErr;
    bool gpu() const { return cfg.device != SAGE2OV_DEVICE_NONE; }
    Device* device() const { if (devOpen.joinable()) devOpen.join(); return dev_; }
    // ---- step 1 staging: variable-length word-packed canonical reads
    RawU64 pool, poolOff; RawU16 poolLen;
    // ... or, for ASCII handed over through sage2ov_reads_add_ascii on a GPU context, the raw bases: filter, 2-bit pack and canonical orientation
    // then run on the device (utils.cpp:144-166, :96-119; readLoader.cpp:195) when the reads are organised
    std::vector<char> ascii; std::vector<uint64_t> asciiOff;
    uint64_t totalReads = 0, goodReads = 0, totalBP = 0, smallReads = 0;
    std::vector<uint32_t> replayDense;                 // scratch of the host replay (read id -> dense index), all zero between calls
    // ---- organised reads (host copy, ids 1..N)
    uint64_t N = 0; int S = 0, maxL = 0; bool organized = false;
    RawU64 words; std::vector<uint16_t> len; RawU16 freq;
    // ---- step 2/3 state
    bool indexBuilt = false, probed = false, reciprocalDone = false, reduced = false, converted = false;
    sage2ov_index_stats istats{};
    sage2ov_find_stats fstats{};                       // of the last sage2ov_reads_find_ids
    // ---- the mate-pair table (sage2ov_mates_*): per library either on the device (mateOnDevice) or here, sorted by key and unique
    struct MateLib { std::vector<uint64_t> key, cnt, first; };
    std::vector<MateLib> mates = std::vector<MateLib>(128); bool mateOnDevice[128] = {};
    uint64_t matePairs[128] = {};                      // pairs given to each library so far, skipped ones included: the base of the record ordinals
    uint32_t mateLibraries = 0;                        // highest library in use (numberOfLibrary)
    sage2ov_mate_stats mstats{};                       // of the last add call
    // ---- the read-to-edge table, flags, distances and insert sizes (sage2ov_mates_map_reads / _estimate): the data live on the device
    bool rmValid = false, estimated = false;           // the table describes the resident graph; inserts / bounds are of the present table and mates
    sage2ov_readmap_stats rmstats{};
    std::vector<sage2ov_insert> inserts = std::vector<sage2ov_insert>(128); uint64_t minUpper = 0, maxUpper = 0;
    std::vector<uint32_t> pairOrdinal;                 // internal pair -> ordinal of its record pair in sage2ov_graph4_save's order (filled by the exports)
    uint64_t readsGen = 0, g4Gen = 0;                  // stamps of the read set and of the read set the step-4 graph was made from: the table is built only when they agree
    // ---- the mate-pair supports (sage2ov_mates_supports): built on the device, kept here in export order once a call has asked for them
    bool supValid = false;                             // the table is of the present graph, flows, mates and estimate (it also needs `estimated`)
    sage2ov_support_stats sstats{}; std::vector<sage2ov_support> supports; bool supOnHost = false;
    void supports_forget() { supValid = supOnHost = false; supports.clear(); sstats = sage2ov_support_stats{}; }
    // ---- the path supports (sage2ov_path_supports): built on the device, kept here in table order with the internal halves (a : 32 | b : 32) of every row; stale
    // whenever the supports above would be
    bool pathValid = false; sage2ov_path_stats pstats{}; std::vector<sage2ov_path_support> prows; std::vector<uint64_t> pkeys;
    void paths_forget() { pathValid = false; prows.clear(); pkeys.clear(); }         // (pstats stays: the figures of the last sweep, until the next one)
    // ---- the scaffold links (sage2ov_links): built on the device, kept here in export order, unfiltered, once a call has asked for them; the flows are read at export
    bool linkValid = false, linkOnHost = false;        // the table is of the present graph, mates and estimate (it also needs `estimated`)
    sage2ov_link_stats lstats{}; std::vector<sage2ov_link> links; std::vector<uint32_t> linkHalves;      // linkHalves: E(pair(a)), E(pair(b)) of every row, internal half-edges
    std::vector<int32_t> linkSums;                     // the raw int32_t gapSum of every row (mergeContigs.cpp:1587 reads it; links[e].gap is its quotient)
    void links_forget() { linkValid = linkOnHost = false; links.clear(); linkHalves.clear(); linkSums.clear(); lstats = sage2ov_link_stats{}; }
    // ---- the contigs (sage2ov_contigs_*): rows and layout are built on the device and kept here in table order; threshold and genome size as the last build was asked
    bool ctgValid = false; uint32_t ctgThreshold = 0, ctgThresholdUsed = 0; uint64_t ctgGenome = 0; sage2ov_contig_stats cstats{};
    std::vector<ContigRow> ctgRows; std::vector<uint64_t> ctgChunk;      // ctgChunk[r]: 16-byte chunks of the device buffer in front of row r (every row begins at a chunk); R + 1 values
    void contigs_forget() { ctgValid = false; ctgRows.clear(); ctgChunk.clear(); cstats = sage2ov_contig_stats{}; }
    // ---- step 5 around its solver (sage2ov_genome_size_estimate, sage2ov_flow_*): the estimate and the network are of the present graph and read set; the data live on the device
    bool gsValid = false, netValid = false; sage2ov_copycount_stats ccstats{};
    sage2ov_mcf_stats mcfstats{};                                                      // of the last solve (sage2ov_mcf_solve, sage2ov_flow_solve)
    uint64_t mcfhub[6] = {};                                                           // sage2ov_mcf_hub_stats_get, of the same solve
    void copycount_forget() { gsValid = netValid = false; ccstats = sage2ov_copycount_stats{}; }
    // ---- the merge rounds (sage2ov_graph_merge_pairs, sage2ov_extend_*): the estimate outlives a merge (estimateHeld: a rebuilt table leaves it alone); the header
    // values of P.graph6 are those from before the first merge
    bool estimateHeld = false, hdrHeld = false; uint64_t hdrGenome = 0, hdrReads = 0;
    sage2ov_extend_stats xstats{}; std::vector<sage2ov_merge> xmerges;
    sage2ov_scaffold_stats scstats{}; std::vector<sage2ov_join> scjoins;      // the scaffold rounds (sage2ov_scaffold_*)
    sage2ov_scaffold_stats sostats{}; std::vector<sage2ov_join> sojoins;      // the short-overlap rounds of step 6 (sage2ov_extend_short_*), kept apart from step 7's
    void extend_forget() { estimateHeld = hdrHeld = false; hdrGenome = hdrReads = 0; xstats = sage2ov_extend_stats{}; xmerges.clear(); scstats = sage2ov_scaffold_stats{}; scjoins.clear(); sostats = sage2ov_scaffold_stats{}; sojoins.clear(); }
    void readmap_forget() { rmValid = estimated = false; extend_forget(); pairOrdinal.clear(); rmstats = sage2ov_readmap_stats{}; supports_forget(); paths_forget(); links_forget(); contigs_forget(); copycount_forget(); }      // the graph or the read set goes
    // ---- pairing (sage2ov_reads_pair_library / sage2ov_mates_from_reads): which input record every staged read was.  A call of reads_add_* made
    // with pairing on is one PairCall: `records` input records, numbered in input order.  raw: the call's records are entries [first, first + records) of the raw ASCII
    // staging (their ordinal is their index); else its staged reads are entries [first, first + count) of the pool and pairOrd[ordAt + x] is the ordinal of the x-th.
    // After the organiser: pairIds (host organiser: +-id of every staged read) or the device's copy (pairOnDevice).  Nothing of this is touched with pairing off.
    struct PairCall { int lib; bool raw; uint64_t records, first, count, ordAt; };
    int pairLib = 0; std::vector<PairCall> pairCalls; std::vector<uint32_t> pairOrd; std::vector<int32_t> pairIds; bool pairReady = false, pairOnDevice = false;
    void pairing_forget() { pairLib = 0; pairReady = pairOnDevice = false; std::vector<PairCall>().swap(pairCalls); std::vector<uint32_t>().swap(pairOrd); std::vector<int32_t>().swap(pairIds); }
    void mates_forget(bool readSetGoes = true) {       // the read set goes: its ids mean nothing any more (the device drops its part in free_reads) -- or sage2ov_mates_clear
        if (pairReady) pairing_forget();               // (the pairing of an organised set goes with it; what is staged for the next organiser stays)
        if (readSetGoes) { readmap_forget(); readsGen++; } else estimated = estimateHeld = false;
        for (auto& L : mates) L = MateLib();
        for (int i = 0; i < 128; i++) { mateOnDevice[i] = false; matePairs[i] = 0; }
        mateLibraries = 0; mstats = sage2ov_mate_stats{};
    }
    sage2ov_overlap_stats ostats{};
    std::vector<FinalEdge> edges; bool edgesOnHost = false;
    SimplifiedGraph g4; bool g4Valid = false;
    double reduce_ms = 0, total_ms = 0;
    // multi-rank contexts: the survivors this rank's share of the reduce phase re-emitted = candidates [survBase, survBase + survCount) of the device list
    uint64_t survBase = 0, survCount = 0, removedPartial = 0; bool survivorsExchanged = true;
    uint64_t rstats[SAGE2OV_REDUCE_STATS] = {0};   // which way the last reduce phase went (sage2ov_reduce_stats_get)

    int fail(int code, const std::string& m) { err = m; return code; }
};
namespace { HostLap::HostLap(const sage2ov_ctx* c, const char* s) : on(c->opt.flag("SAGE2OV_TIMING")), stage(s) {} }

namespace {

// ------------------------------------------------------------------------------------------ step 1
// filter + canonical + pack one read (readLoader.cpp:145-158, utils.cpp:144, readLoader.cpp:179-213)
// codes: 0..3 per base or 255 for anything that is not ACGTacgt
template <class VP, class VL>
inline void stage_codes(sage2ov_ctx* c, const uint8_t* codes, int L, VP& pool, VP& off, VL& lens, uint64_t& good, uint64_t& bp, uint64_t& small) {
    if (L <= (int)c->cfg.min_overlap) { small++; return; }
    const int nw = (L + 31) / 32;
    uint64_t f[34], r[34];
    if (nw > 32) { lens.push_back(0xFFFF); off.push_back(pool.size()); good++; bp += L; return; }   // too long: organise reports the limit
    for (int w = 0; w < nw; w++) f[w] = 0;
    for (int i = 0; i < L; i++) { if (codes[i] > 3) return; f[i >> 5] |= (uint64_t)codes[i] << (62 - 2 * (i & 31)); }
    // the forward strand is staged; the canonical orientation (readLoader.cpp:195) is chosen by the organiser (device or host)
    (void)r;
    off.push_back(pool.size()); lens.push_back((uint16_t)L);
    pool.insert(pool.end(), f, f + nw);
    good++; bp += L;
}
static uint8_t g_code[256];
struct CodeInit { CodeInit() { memset(g_code, 255, 256); g_code['A'] = g_code['a'] = 0; g_code['C'] = g_code['c'] = 1; g_code['G'] = g_code['g'] = 2; g_code['T'] = g_code['t'] = 3; } } g_code_init;
// 2-bit codes of 8 ASCII bases (first base in the lowest byte of x) as 16 bits, first base highest; false when a byte is not one of ACGTacgt
inline bool pack8(uint64_t x, uint64_t& out) {
    const uint64_t K1 = 0x0101010101010101ull;
    const uint64_t y = x & 0xDFDFDFDFDFDFDFDFull;                              // upper case
    const uint64_t cd = ((y >> 1) ^ (y >> 2)) & (3 * K1);                      // A 0, C 1, G 2, T 3 (bits 1 and 2 of the letters)
    const uint64_t b0 = cd & K1, b1 = (cd >> 1) & K1, both = b0 & b1;
    const uint64_t letter = (0x40 * K1) | (both << 4) | (b1 << 2) | ((b0 ^ b1) << 1) | (both ^ K1);      // the letter each code stands for: 41 43 47 54
    uint64_t t = __builtin_bswap64(cd);
    t = (t | (t >> 6)) & 0x000F000F000F000Full; t = (t | (t >> 12)) & 0x000000FF000000FFull; t = (t | (t >> 24)) & 0xFFFFull;
    out = t; return letter == y;
}
// stage_codes straight from the text of a sequence line; -1: the line holds white space (the general reader drops it: utils of fastAQReader.cpp:16-45), nothing staged
template <class VP, class VL>
inline int stage_ascii(sage2ov_ctx* c, const char* b, size_t Ls, VP& pool, VP& off, VL& lens, uint64_t& good, uint64_t& bp, uint64_t& small) {
    if (Ls > 1024) return -1;                                                    // (beyond the 32-word layout: the general reader's business)
    bool valid = true; uint64_t f[34]; const int L = (int)Ls, nw = (L + 31) / 32;
    for (int w = 0; w < nw; w++) f[w] = 0;
    int i = 0;
    for (; i + 8 <= L; i += 8) { uint64_t x, o; memcpy(&x, b + i, 8); valid &= pack8(x, o); f[i >> 5] |= o << (48 - 2 * (i & 31)); }
    for (; i < L; i++) { const uint8_t cd = g_code[(unsigned char)b[i]]; valid &= cd <= 3; f[i >> 5] |= (uint64_t)(cd & 3) << (62 - 2 * (i & 31)); }
    if (!valid) { for (size_t q = 0; q < Ls; q++) if ((unsigned char)b[q] <= ' ') return -1; }
    if (L <= (int)c->cfg.min_overlap) { small++; return 0; }
    if (!valid) return 0;
    off.push_back(pool.size()); lens.push_back((uint16_t)L);
    pool.insert(pool.end(), f, f + nw);
    good++; bp += L;
    return 0;
}
inline bool canonicalise_words(uint64_t* f, int L) {        // readLoader.cpp:195: read < revcomp ? read : revcomp (tie: revcomp, same bytes); true: the read as given stays
    const int nw = (L + 31) / 32; uint64_t r[34];
    revcomp_words(f, nw, L, r);
    bool useF = false;
    for (int w = 0; w < nw; w++) { if (f[w] != r[w]) { useF = f[w] < r[w]; break; } }
    if (!useF) for (int w = 0; w < nw; w++) f[w] = r[w];
    return useF;
}
// pairing: a call's record ordinals are kept in 32 bits and its dense slot table has one word per record
constexpr uint64_t PAIR_CALL_RECORDS_MAX = (1ull << 32) - 2048;
static int pair_call_limit(sage2ov_ctx* c) { return c->fail(SAGE2OV_ERR_LIMIT, "pairing: 2^32 - 2048 input records or more in one call"); }
// worker threads of the host-side I/O helpers: the configured number, else what OpenMP and the CPU affinity allow, at most 16
// (many short parallel regions on an oversubscribed CPU share cost more than they give)
static int io_threads(const sage2ov_ctx* c) {
    if (c->cfg.host_threads) return (int)c->cfg.host_threads;
    int nt = omp_get_max_threads();
    cpu_set_t set; CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof set, &set) == 0) nt = std::min(nt, CPU_COUNT(&set));
    return std::max(1, std::min(nt, 16));
}

// minimal FASTA/FASTQ(.gz) record reader with kseq-like rules (fastAQReader.cpp:16-45)
struct SeqFile {
    gzFile fp = nullptr; std::vector<char> buf; size_t pos = 0, end = 0; bool eof = false, ioError = false; const char* win = nullptr;   // win: the current window (buf, or a mapped range)
    // gzip inflates at a few hundred MB/s on one thread: a reader thread fills the next 8 MB window while the caller splits the current one
    std::vector<char> nextBuf; std::thread reader; std::mutex mu; std::condition_variable cv; int nextN = 0; bool nextReady = false, wantNext = false, quit = false;
    void reader_loop() {
        for (;;) {
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return wantNext || quit; }); if (quit) return; wantNext = false; }
            const int n = gzread(fp, nextBuf.data(), (unsigned)nextBuf.size());
            { std::lock_guard<std::mutex> lk(mu); nextN = n; nextReady = true; }
            cv.notify_all();
            if (n <= 0) return;
        }
    }
    bool open(const char* p) {
        fp = gzopen(p, "r"); if (!fp) return false;
        gzbuffer(fp, 1 << 20); buf.resize(8 << 20); nextBuf.resize(8 << 20); win = buf.data();
        wantNext = true; reader = std::thread([this] { reader_loop(); });
        return true;
    }
    void open_range(const char* b, size_t n) { win = b; pos = 0; end = n; eof = true; }        // parse a range of a mapped file: one window, never refilled
    ~SeqFile() {
        if (reader.joinable()) { { std::lock_guard<std::mutex> lk(mu); quit = true; } cv.notify_all(); reader.join(); }
        if (fp) gzclose(fp);
    }
    bool refill() {
        if (eof) return false;
        int n;
        { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return nextReady; }); n = nextN; nextReady = false; if (n > 0) { buf.swap(nextBuf); wantNext = true; } }
        if (n <= 0) { eof = true; if (n < 0) ioError = true; return false; }      // n < 0: corrupt or truncated gzip stream (gzerror), not an end of file
        cv.notify_all();
        win = buf.data(); end = (size_t)n; pos = 0; return true;
    }
    // next line (without the line end) appended to `s`; lines are found with memchr on the 8 MB window
    bool line(std::string& s) {
        s.clear(); bool any = false;
        for (;;) {
            if (pos >= end && !refill()) break;
            any = true;
            const char* b = win + pos; const char* nl = (const char*)memchr(b, '\n', end - pos);
            if (nl) { s.append(b, (size_t)(nl - b)); pos = (size_t)(nl - win) + 1; break; }
            s.append(b, end - pos); pos = end;
        }
        if (!s.empty() && s.back() == '\r') s.pop_back();
        return any;
    }
    std::string held, l; bool haveHeld = false;
    // The common shapes -- a FASTA record with one sequence line, a four-line FASTQ record -- when the whole record and the first
    // character behind it lie inside the current window: found with memchr, the sequence copied once, no per-line strings.
    // Anything else (multi-line sequences, white space inside a line, a record that crosses the window) is left to the general path.
    bool fast_next(std::string& out, size_t& len) {
        if (haveHeld || pos >= end) return false;
        const char* const b = win + pos; const char* const e = win + end;
        const char kind = *b; if (kind != '>' && kind != '@') return false;
        const char* nl1 = (const char*)memchr(b, '\n', (size_t)(e - b)); if (!nl1) return false;
        const char* sq = nl1 + 1; const char* nl2 = (const char*)memchr(sq, '\n', (size_t)(e - sq)); if (!nl2 || nl2 + 1 >= e) return false;
        size_t n = (size_t)(nl2 - sq); if (n && sq[n - 1] == '\r') n--;
        if (n == 0) return false;
        for (size_t i = 0; i < n; i++) if ((unsigned char)sq[i] <= ' ') return false;
        const char* after = nl2 + 1;
        if (kind == '>') { if (*after != '>') return false; }
        else {
            if (*after != '+') return false;
            const char* nl3 = (const char*)memchr(after, '\n', (size_t)(e - after)); if (!nl3) return false;
            const char* q = nl3 + 1; const char* nl4 = (const char*)memchr(q, '\n', (size_t)(e - q)); if (!nl4 || nl4 + 1 >= e) return false;
            size_t nq = (size_t)(nl4 - q); if (nq && q[nq - 1] == '\r') nq--;
            if (nq != n || nl4[1] != '@') return false;
            after = nl4 + 1;
        }
        out.append(sq, n); len = n; pos = (size_t)(after - win);
        return true;
    }
    // bases of the next record appended to `out` (white space dropped); false at end of file
    bool next(std::string& out, size_t& len) {
        if (fast_next(out, len)) return true;
        const size_t start = out.size();
        for (;;) { if (haveHeld) { l.swap(held); haveHeld = false; } else if (!line(l)) return false; if (!l.empty() && (l[0] == '>' || l[0] == '@')) break; }
        for (;;) {
            if (!line(l)) { len = out.size() - start; return true; }
            if (!l.empty() && (l[0] == '>' || l[0] == '@')) { held.swap(l); haveHeld = true; len = out.size() - start; return true; }
            if (!l.empty() && l[0] == '+') break;
            const size_t at = out.size(); out.append(l);                      // (white space inside a sequence line is rare: compact only then)
            bool ws = false; for (size_t x = at; x < out.size(); x++) ws |= (unsigned char)out[x] <= ' ';
            if (ws) { size_t w = at; for (size_t x = at; x < out.size(); x++) if ((unsigned char)out[x] > ' ') out[w++] = out[x]; out.resize(w); }
        }
        len = out.size() - start;
        size_t q = 0; while (q < len) { if (!line(l)) break; q += l.size(); }          // quality: as many characters as bases
        return true;
    }
};

// A plain (uncompressed) single file is mapped and cut at record starts into chunks that the threads parse, filter and pack
// independently -- the read ids do not depend on the input order (they are ranks after the sort).  FASTA: a '>' at a line start is
// always a header.  FASTQ: a quality line may start with '@' as well; in the four-line form a line starting with '@' is a header iff
// the line two below starts with '+', and every chunk is parsed strictly as four-line records (equal sequence and quality lengths).
// Anything else -- multi-line FASTQ, a file that is neither, a chunk that does not parse -- returns false and the sequential reader
// below takes the whole file.
struct StagePart { RawU64 pool, off; RawU16 lens; uint64_t good = 0, bp = 0, small = 0, records = 0; std::vector<uint32_t> ord; };      // what one thread staged (ord: with pairing, the file ordinal of every staged read)
// track (pairing): the chunks are handed out dynamically, so every thread notes per chunk where its staged reads begin and their ordinals inside the
// chunk, every chunk its record count; a prefix sum over the chunks then makes file ordinals of them
static bool parse_plain_file_parallel(sage2ov_ctx* c, const char* path, std::vector<StagePart>& parts, bool track = false) {
    const int fd = ::open(path, O_RDONLY); if (fd < 0) return false;
    struct stat sb; if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size < (1 << 20)) { ::close(fd); return false; }
    const size_t size = (size_t)sb.st_size;
    const char* m = (const char*)mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0); ::close(fd);
    if (m == MAP_FAILED) return false;
    struct Unmap { const char* p; size_t n; ~Unmap() { munmap((void*)p, n); } } um{m, size};
    madvise((void*)m, size, MADV_SEQUENTIAL);
    if ((unsigned char)m[0] == 0x1f && (unsigned char)m[1] == 0x8b) return false;                          // gzip
    const char kind = m[0]; if (kind != '>' && kind != '@') return false;
    auto line_start_after = [&](size_t p) -> size_t { const char* nl = (const char*)memchr(m + p, '\n', size - p); return nl ? (size_t)(nl - m) + 1 : size; };
    auto boundary = [&](size_t from) -> size_t {                                                        // first record start at or after `from` (a line start)
        size_t p = from == 0 ? 0 : line_start_after(from - 1);
        while (p < size) {
            if (m[p] == kind) {
                if (kind == '>') return p;
                const size_t l1 = line_start_after(p), l2 = l1 < size ? line_start_after(l1) : size;
                if (l2 < size && m[l2] == '+') return p;
            }
            p = line_start_after(p);
        }
        return size;
    };
    const int nt = io_threads(c); HostLap lap(c, "input");
    const size_t nchunks = std::max<size_t>((size_t)nt, std::min<size_t>(4096, size >> 24));
    std::vector<size_t> cut(nchunks + 1); cut[0] = 0; cut[nchunks] = size;
    for (size_t x = 1; x < nchunks; x++) cut[x] = std::max(cut[x - 1], boundary((size * x) / nchunks));
    using Part = StagePart;
    parts.clear(); parts.resize(nt); bool bad = false;
    std::vector<uint64_t> chunkRec(track ? nchunks + 1 : 0, 0); std::vector<std::vector<std::pair<size_t, size_t>>> segs(track ? nt : 0);      // segs: (chunk, index into the thread's ord)
    #pragma omp parallel num_threads(nt)
    {
        Part& P = parts[omp_get_thread_num()]; std::string seq; std::vector<uint8_t> codes;
        #pragma omp for schedule(dynamic, 1)
        for (int64_t x = 0; x < (int64_t)nchunks; x++) {
            if (cut[x] >= cut[x + 1]) continue;
            const uint64_t rec0 = P.records; if (track) segs[omp_get_thread_num()].emplace_back((size_t)x, P.ord.size());
            auto note = [&](size_t before) { if (track && P.lens.size() > before) P.ord.push_back((uint32_t)(P.records - rec0)); };      // (before the record is counted)
            auto stage = [&](const char* b, size_t L) { codes.resize(L); for (size_t i = 0; i < L; i++) codes[i] = g_code[(unsigned char)b[i]]; const size_t at = P.lens.size(); stage_codes(c, codes.data(), (int)L, P.pool, P.off, P.lens, P.good, P.bp, P.small); note(at); P.records++; };
            if (kind == '>') {
                // records of one header line + one sequence line, packed straight from the mapping (eight bases per step); the first record that
                // is anything else -- a second sequence line, white space inside the line, the last record of the chunk -- hands the rest of the chunk to the general reader
                size_t p = cut[x]; const size_t e = cut[x + 1];
                while (p < e) {
                    const char* nl1 = (const char*)memchr(m + p, '\n', e - p); if (!nl1) break;
                    const char* sq = nl1 + 1; const char* nl2 = (const char*)memchr(sq, '\n', (size_t)(m + e - sq)); if (!nl2 || nl2 + 1 >= m + e || nl2[1] != '>') break;
                    size_t n = (size_t)(nl2 - sq); if (n && sq[n - 1] == '\r') n--;
                    if (n == 0) break;
                    const size_t at = P.lens.size();
                    const int st = stage_ascii(c, sq, n, P.pool, P.off, P.lens, P.good, P.bp, P.small);
                    if (st < 0) break;                                                                   // white space inside the line
                    note(at); P.records++; p = (size_t)(nl2 + 1 - m);
                }
                if (p < e) {
                    SeqFile f; f.open_range(m + p, e - p); size_t len = 0;
                    for (;;) { seq.clear(); if (!f.next(seq, len)) break; stage(seq.data(), len); }
                }
            } else {                                                                                    // strict four-line FASTQ
                size_t p = cut[x]; const size_t e = cut[x + 1];
                auto trimmed = [&](size_t a, size_t b) { size_t n = b - a; if (n && m[b - 1] == '\n') n--; if (n && m[a + n - 1] == '\r') n--; return n; };
                while (p < e) {
                    const size_t l1 = line_start_after(p), l2 = l1 < e ? line_start_after(l1) : e, l3 = l2 < e ? line_start_after(l2) : e, l4 = l3 < e ? line_start_after(l3) : e;
                    const size_t ns = trimmed(l1, l2), nq = trimmed(l3, l4);
                    bool ws = false; for (size_t i = 0; i < ns; i++) ws |= (unsigned char)m[l1 + i] <= ' ';
                    if (m[p] != '@' || l2 >= e || m[l2] != '+' || ns != nq || ns == 0 || ws) {
                        #pragma omp atomic write
                        bad = true;
                        break;
                    }
                    const size_t at = P.lens.size();
                    if (stage_ascii(c, m + l1, ns, P.pool, P.off, P.lens, P.good, P.bp, P.small) < 0) stage(m + l1, ns); else { note(at); P.records++; }     // (eight bases per step; longer than the 32-word layout: the table form)
                    p = l4;
                }
            }
            if (track) chunkRec[x] = P.records - rec0;
        }
    }
    if (bad) return false;
    if (track) {
        uint64_t run = 0; for (size_t x = 0; x <= nchunks; x++) { const uint64_t r = chunkRec[x]; chunkRec[x] = run; run += r; }      // records in front of every chunk
        if (run < PAIR_CALL_RECORDS_MAX) for (int t = 0; t < nt; t++) for (size_t g = 0; g < segs[t].size(); g++) {
            const size_t e = g + 1 < segs[t].size() ? segs[t][g + 1].second : parts[t].ord.size(); const uint32_t base = (uint32_t)chunkRec[segs[t][g].first];
            for (size_t i = segs[t][g].second; i < e; i++) parts[t].ord[i] += base;
        }
    }
    lap("split + filter + pack (threads)");
    return true;
}
// the threads' pools, one behind the other at the end of the context's staging arrays (each thread copies its own: the arrays are sized without being written)
// track: the parts' file ordinals o go behind the context's as o * mul + add (two mate files: 2 j and 2 j + 1)
static void commit_parts(sage2ov_ctx* c, std::vector<StagePart>& parts, bool track = false, uint32_t mul = 1, uint32_t add = 0) {
    using Part = StagePart; const int nt = (int)parts.size(); HostLap lap(c, "input");
    if (track) for (Part& P : parts) { for (uint32_t o : P.ord) c->pairOrd.push_back(o * mul + add); std::vector<uint32_t>().swap(P.ord); }      // (in the order the pools are laid down below)
    std::vector<uint64_t> wordBase(nt + 1), readBase(nt + 1); wordBase[0] = c->pool.size(); readBase[0] = c->poolOff.size();
    for (int t = 0; t < nt; t++) { wordBase[t + 1] = wordBase[t] + parts[t].pool.size(); readBase[t + 1] = readBase[t] + parts[t].off.size(); }
    c->pool.resize(wordBase[nt]); c->poolOff.resize(readBase[nt]); c->poolLen.resize(readBase[nt]);
    #pragma omp parallel for num_threads(nt) schedule(static, 1)
    for (int t = 0; t < nt; t++) {
        Part& P = parts[t];
        if (!P.pool.empty()) memcpy(c->pool.data() + wordBase[t], P.pool.data(), P.pool.size() * sizeof(uint64_t));
        uint64_t* po = c->poolOff.data() + readBase[t]; const uint64_t base = wordBase[t];
        for (size_t i = 0; i < P.off.size(); i++) po[i] = base + P.off[i];
        if (!P.lens.empty()) memcpy(c->poolLen.data() + readBase[t], P.lens.data(), P.lens.size() * sizeof(uint16_t));
        RawU64().swap(P.pool); RawU64().swap(P.off); RawU16().swap(P.lens);
    }
    for (Part& P : parts) { c->goodReads += P.good; c->totalBP += P.bp; c->smallReads += P.small; c->totalReads += P.records; }
    lap("concatenation of the threads' pools");
}
static bool add_plain_file_parallel(sage2ov_ctx* c, const char* path, bool track, uint64_t* records) {
    std::vector<StagePart> parts; if (!parse_plain_file_parallel(c, path, parts, track)) return false;
    *records = 0; for (auto& P : parts) *records += P.records;
    commit_parts(c, parts, track && *records < PAIR_CALL_RECORDS_MAX); return true;
}
// Two mate files are read alternately, file 1 first, until the file whose turn it is has no record left (inputReader.cpp:26-49): with n1 = n2 or n1 = n2 + 1 records
// that is every record of both files, and since the ids are ranks after the sort the order they are staged in is free -- both files then go through the parallel
// reader one after the other.  Any other pair of counts (or a file the parallel reader does not take) is the sequential reader's business.
static bool add_mate_files_parallel(sage2ov_ctx* c, const char* p1, const char* p2, bool track, uint64_t* records) {
    std::vector<StagePart> a, b; if (!parse_plain_file_parallel(c, p1, a, track) || !parse_plain_file_parallel(c, p2, b, track)) return false;
    uint64_t n1 = 0, n2 = 0; for (auto& P : a) n1 += P.records; for (auto& P : b) n2 += P.records;
    if (n1 != n2 && n1 != n2 + 1) return false;
    *records = n1 + n2; track = track && *records < PAIR_CALL_RECORDS_MAX;
    commit_parts(c, a, track, 2, 0); commit_parts(c, b, track, 2, 1); return true;      // (record j of file 1 is record 2 j of the alternating stream, record j of file 2 is 2 j + 1)
}

// records are split sequentially (cheap: memchr), filtered and packed by all threads in batches
// pairLib != 0 (pairing): the call is also one mates call of that library -- the ordinal of every staged read is noted
int add_files(sage2ov_ctx* c, const char* p1, const char* p2, int pairLib = 0) {
    const bool track = pairLib != 0; const uint64_t first0 = c->poolLen.size(), ordAt0 = c->pairOrd.size(); uint64_t records = 0;
    auto pair_done = [&]() -> int {                                   // the call as sage2ov_mates_from_reads will see it
        if (!track) return SAGE2OV_OK;
        if (records >= PAIR_CALL_RECORDS_MAX) return pair_call_limit(c);
        c->pairCalls.push_back({pairLib, false, records, first0, c->poolLen.size() - first0, ordAt0}); return SAGE2OV_OK;
    };
    if (!c->opt.get("SAGE2OV_SEQUENTIAL_READER") && ((p2 && *p2) ? add_mate_files_parallel(c, p1, p2, track, &records) : add_plain_file_parallel(c, p1, track, &records))) return pair_done();
    SeqFile f1, f2; if (!f1.open(p1)) return c->fail(SAGE2OV_ERR_IO, std::string("cannot open ") + p1);
    const bool two = p2 && *p2; if (two && !f2.open(p2)) return c->fail(SAGE2OV_ERR_IO, std::string("cannot open ") + p2);
    const int nt = io_threads(c);
    const size_t BATCH = 1 << 19;
    std::string flat; std::vector<uint64_t> boff; uint64_t inFile = 0; bool more = true;
    std::vector<std::vector<uint64_t>> pools(nt), offs(nt); std::vector<std::vector<uint16_t>> lens(nt); std::vector<std::vector<uint32_t>> ords(track ? nt : 0);
    while (more) {
        flat.clear(); boff.clear(); boff.push_back(0);
        while (boff.size() <= BATCH) {                             // inputReader.cpp:26-49: alternate by parity
            SeqFile& f = (two && (inFile & 1)) ? f2 : f1;
            size_t len = 0;
            if (!f.next(flat, len)) { more = false; break; }
            boff.push_back(flat.size()); inFile++;
        }
        const int64_t nb = (int64_t)boff.size() - 1; if (nb == 0) break;
        std::vector<uint64_t> good(nt, 0), bp(nt, 0), small(nt, 0);
        for (int t = 0; t < nt; t++) { pools[t].clear(); offs[t].clear(); lens[t].clear(); if (track) ords[t].clear(); }
        const uint64_t batch0 = inFile - (uint64_t)nb;                // records in front of this batch: the reader stages in input order and only has to count
        #pragma omp parallel num_threads(nt)
        {
            const int t = omp_get_thread_num(); const int64_t chunk = (nb + nt - 1) / nt, a = t * chunk, b = std::min<int64_t>(nb, a + chunk);
            std::vector<uint8_t> codes;
            for (int64_t r = a; r < b; r++) {
                const size_t L = boff[r + 1] - boff[r]; codes.resize(L);
                const unsigned char* sq = (const unsigned char*)flat.data() + boff[r];
                for (size_t i = 0; i < L; i++) codes[i] = g_code[sq[i]];
                const size_t at = lens[t].size();
                stage_codes(c, codes.data(), (int)L, pools[t], offs[t], lens[t], good[t], bp[t], small[t]);
                if (track && lens[t].size() > at) ords[t].push_back((uint32_t)(batch0 + (uint64_t)r));
            }
        }
        for (int t = 0; t < nt; t++) {                              // concatenate in file order (thread t holds a contiguous slice)
            const uint64_t base = c->pool.size();
            c->pool.insert(c->pool.end(), pools[t].begin(), pools[t].end());
            for (uint64_t o : offs[t]) c->poolOff.push_back(base + o);
            c->poolLen.insert(c->poolLen.end(), lens[t].begin(), lens[t].end());
            if (track) c->pairOrd.insert(c->pairOrd.end(), ords[t].begin(), ords[t].end());
            c->goodReads += good[t]; c->totalBP += bp[t]; c->smallReads += small[t];
        }
        c->totalReads += (uint64_t)nb;
    }
    records = inFile;
    for (SeqFile* f : {&f1, &f2}) if (f->ioError) {
        int en = 0; const char* m = f->fp ? gzerror(f->fp, &en) : nullptr;
        return c->fail(SAGE2OV_ERR_IO, std::string("read error in ") + (f == &f1 ? p1 : p2) + ": " + (m && *m ? m : "corrupt or truncated input"));
    }
    return pair_done();
}
std::string trim(const std::string& s) { size_t a = s.find_first_not_of(" \t\r\n"), b = s.find_last_not_of(" \t\r\n"); return a == std::string::npos ? "" : s.substr(a, b - a + 1); }

// ------------------------------------------------------------------------------------------ reduce replay
// exact restatement of economyGraph.cpp:495-574 over device-computed hit lists
// Serial replay of the reduce phase (economyGraph.cpp:513-707).  All state is in flat arrays over a dense numbering of the reads
// it can touch (unresolved reads and the ends of the candidates near them): no hashing on the hot path.
struct Replay {
    sage2ov_ctx* c;
    std::vector<uint32_t>& dense;                      // read id -> dense index + 1 (0: not part of the replay); lives in the context, all zero between replays
    explicit Replay(std::vector<uint32_t>& d) : dense(d) {}
    ~Replay() { for (uint32_t id : idOf) dense[id] = 0; }
    std::vector<uint32_t> idOf;                        // dense index -> read id
    std::vector<std::vector<AdjEdge>> adj;             // per dense index
    std::vector<uint8_t> st;                           // per dense index: 0 unexplored, 1 explored, 2 marked, 4 not an unresolved read
    std::vector<std::pair<uint64_t, uint64_t>> hitRange;
    const std::vector<Hit>* hits = nullptr;
    uint64_t inserted = 0, removed = 0;
    uint32_t add(uint32_t id) { uint32_t& d = dense[id]; if (!d) { idOf.push_back(id); d = (uint32_t)idOf.size(); } return d - 1; }
    void finish_setup() { adj.resize(idOf.size()); st.assign(idOf.size(), 4); hitRange.assign(idOf.size(), {0, 0}); }
    uint8_t status_id(uint32_t id) const { const uint32_t d = dense[id]; return d ? st[d - 1] : 4; }
    int insert_edge(uint32_t u, uint32_t v, uint32_t delta, int type) {              // economyGraph.cpp:813-849 (u, v: read ids)
        if (u == v) return 0;
        int d2 = (int)c->len[u] - ((int)c->len[v] - (int)delta);
        adj[dense[u] - 1].push_back(AdjEdge{v, (uint8_t)type, 0, delta & 0xFFFFFu});
        adj[dense[v] - 1].push_back(AdjEdge{u, (uint8_t)flip_type_host(type), 0, (uint32_t)d2 & 0xFFFFFu});
        return 1;
    }
    uint64_t explore(uint32_t r1) {                                                  // economyGraph.cpp:580-638
        const uint32_t d1 = dense[r1]; if (!d1 || st[d1 - 1] != 0) return 0;
        st[d1 - 1] = 1; uint64_t ins = 0;
        for (uint64_t x = hitRange[d1 - 1].first; x < hitRange[d1 - 1].second; x++) {
            const Hit& h = (*hits)[x];
            if (status_id(h.to) != 0) continue;                                      // :605 current status
            if (h.len == -1) continue;                                               // :627 sentinel quirk
            ins += insert_edge(r1, h.to, (uint32_t)h.len, h.type);
        }
        auto& a = adj[d1 - 1];
        if (a.size() > 1) std::sort(a.begin(), a.end(), [](const AdjEdge& x, const AdjEdge& y) {   // :853-871
            if (x.len != y.len) return x.len > y.len; if (x.to != y.to) return x.to > y.to; return x.type > y.type; });
        return ins * 2;
    }
    // markTransitiveEdge (economyGraph.cpp:643-679).  When it runs in the serial BFS the lists of `from` and of all its neighbours are
    // complete and nothing has been removed from them yet (every neighbour is explored by then, nobody appends to the list of an
    // explored read, and a read's removal waits until all its neighbours are marked): the marks are a function of the final lists, so
    // the BFS below only keeps the statuses that steer the traversal and the marks are computed afterwards, reads in parallel.
    void mark_edges(uint32_t from, std::vector<uint8_t>& mkb) {
        auto& a = adj[dense[from] - 1];
        for (auto& e : a) mkb[dense[e.to] - 1] = 1;
        for (auto& e : a) {
            if (mkb[dense[e.to] - 1] != 1) continue;
            for (auto& f : adj[dense[e.to] - 1]) {
                const uint32_t df = dense[f.to]; if (!df || mkb[df - 1] != 1) continue;
                int t1 = e.type, t2 = f.type;
                if ((t1 == 0 || t1 == 2) && (t2 == 0 || t2 == 1)) mkb[df - 1] = 2;
                else if ((t1 == 1 || t1 == 3) && (t2 == 2 || t2 == 3)) mkb[df - 1] = 2;
            }
        }
        for (auto& e : a) if (mkb[dense[e.to] - 1] == 2) e.mark = 1;
        for (auto& e : a) mkb[dense[e.to] - 1] = 0;
    }
    void mark(uint32_t from) { st[dense[from] - 1] = 2; }                            // traversal only: status 1 -> 2 (:679)
    uint64_t remove_marked(uint32_t r) {                                             // economyGraph.cpp:681-707
        auto& a = adj[dense[r] - 1]; size_t before = a.size();
        a.erase(std::remove_if(a.begin(), a.end(), [](const AdjEdge& e) { return e.mark != 0; }), a.end());
        return before - a.size();
    }
    bool timing = false;
    void run(const std::vector<uint32_t>& ids) {
        auto tp = std::chrono::steady_clock::now();
        auto lap = [&](const char* what) { if (!timing) return; auto t = std::chrono::steady_clock::now(); fprintf(stderr, "[reduce/host]   %-26s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(t - tp).count()); tp = t; };
        std::vector<uint32_t> queue;
        for (uint32_t i : ids) {                                                     // the serial part: exploration order (:513-564)
            if (status_id(i) != 0) continue;
            queue.clear(); size_t start = 0; queue.push_back(i);
            while (start < queue.size()) {
                uint32_t r1 = queue[start++];
                if (status_id(r1) == 0) inserted += explore(r1);
                const uint32_t d1 = dense[r1] - 1;
                if (adj[d1].empty()) continue;
                if (st[d1] == 1) {
                    for (size_t x = 0; x < adj[d1].size(); x++) { uint32_t r2 = adj[d1][x].to; if (status_id(r2) == 0) { queue.push_back(r2); inserted += explore(r2); } }
                    mark(r1);
                }
                if (st[d1] == 2) {
                    for (size_t x = 0; x < adj[d1].size(); x++) {
                        uint32_t r2 = adj[d1][x].to; if (status_id(r2) != 1) continue;
                        const uint32_t d2 = dense[r2] - 1;
                        for (size_t y = 0; y < adj[d2].size(); y++) { uint32_t r3 = adj[d2][y].to; if (status_id(r3) == 0) { queue.push_back(r3); inserted += explore(r3); } }
                        mark(r2);
                    }
                }
            }
        }
        lap("serial exploration");
        // marks on the final lists (all reads first: they read their neighbours' unreduced lists), then the removals (:681-707)
        const int64_t n = (int64_t)ids.size();
        const int nthr = io_threads(c);
        #pragma omp parallel num_threads(nthr) if (n > 4096)
        {
            std::vector<uint8_t> mkb(idOf.size(), 0);
            #pragma omp for schedule(dynamic, 1024)
            for (int64_t x = 0; x < n; x++) { const uint32_t d = dense[ids[x]] - 1; if (st[d] == 2 && !adj[d].empty()) mark_edges(ids[x], mkb); }
        }
        lap("marks (parallel)");
        uint64_t rem = 0;
        #pragma omp parallel for num_threads(nthr) schedule(dynamic, 1024) reduction(+ : rem) if (n > 4096)
        for (int64_t x = 0; x < n; x++) { const uint32_t d = dense[ids[x]] - 1; if (st[d] == 2) rem += remove_marked(ids[x]); }
        removed += rem;
        lap("removals (parallel)");
    }
};

}  // namespace

static inline char* put_u(char* p, unsigned long long v) {          // decimal, no sign, no padding (what %u / %llu print)
    char t[24]; int n = 0; do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v); while (n) *p++ = t[--n]; return p;
}
// text of items [0, n) produced by `fmt(i, out)` (appends to a std::string): chunks of about 4 MB of text, formatted by whichever thread is free into its own
// (cache-resident, reused) buffer and copied into the page cache at the chunk's offset.  The offset of chunk j + 1 is published as soon as chunk j is
// FORMATTED, so nobody waits for somebody else's write: formatting and the copies into the page cache overlap (in the batch form this replaces --
// all format, barrier, all write -- thread 0 spent 0.26 of 0.46 s working on the 2.8 GB .reads file of 10 M reads).
template <class F>
static int write_formatted(sage2ov_ctx* c, FILE* f, uint64_t n, size_t bytes_per_item, F fmt) {
    const int nt = io_threads(c); HostLap lap(c, "writer");
    if (fflush(f) != 0) return c->fail(SAGE2OV_ERR_IO, "write failed");
    const off_t pos0 = ftello(f); const int fd = fileno(f);
    // (items of very uneven size -- the edges of P.graph4 carry read lists -- still give every thread several chunks)
    const uint64_t per = std::max<uint64_t>(64, std::min<uint64_t>((4u << 20) / std::max<size_t>(bytes_per_item, 1), (n + (uint64_t)nt * 8 - 1) / ((uint64_t)nt * 8))), nchunks = (n + per - 1) / per;
    std::unique_ptr<std::atomic<int64_t>[]> at(new std::atomic<int64_t>[nchunks + 1]);
    for (uint64_t j = 0; j <= nchunks; j++) at[j].store(-1, std::memory_order_relaxed);
    at[0].store((int64_t)pos0);
    std::atomic<uint64_t> next{0}; std::atomic<bool> failed{false};
    #pragma omp parallel num_threads(nt)
    {
        std::string out; out.reserve((size_t)per * bytes_per_item + 4096);
        for (;;) {
            const uint64_t j = next.fetch_add(1); if (j >= nchunks || failed.load()) break;
            out.clear(); const uint64_t a = j * per, e = std::min(n, a + per);
            for (uint64_t i = a; i < e; i++) fmt(i, out);
            int64_t o; while ((o = at[j].load(std::memory_order_acquire)) < 0 && !failed.load()) sched_yield();
            if (o < 0) break;
            at[j + 1].store(o + (int64_t)out.size(), std::memory_order_release);
            const char* p = out.data(); size_t left = out.size();
            while (left) { const ssize_t w = pwrite(fd, p, left, (off_t)o); if (w <= 0) { failed.store(true); break; } p += w; left -= (size_t)w; o += w; }
        }
    }
    lap("format + pwrite (threads)");
    if (failed.load() || fseeko(f, (off_t)at[nchunks].load(), SEEK_SET) != 0) return c->fail(SAGE2OV_ERR_IO, "write failed");
    return SAGE2OV_OK;
}

// ============================================================================================ C ABI
extern "C" {

const char* sage2ov_version(void) { return "sage2ov 0.1 (gfx950)"; }
const char* sage2ov_last_error(const sage2ov_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }
void* sage2ov_stream(sage2ov_ctx* c) { return c && c->device() ? dev_stream(c->device()) : nullptr; }

int sage2ov_ctx_create(const sage2ov_config* cfg, sage2ov_ctx** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return SAGE2OV_ERR_ARG; }
    if (cfg->min_overlap == 0) { g_create_error = "min_overlap (-k) is required"; return SAGE2OV_ERR_ARG; }   // main.cpp:506-510
    if (cfg->rank >= std::max<uint32_t>(1, cfg->world)) { g_create_error = "rank >= world"; return SAGE2OV_ERR_ARG; }
    auto* c = new sage2ov_ctx(); c->cfg = *cfg;
    if (c->cfg.world == 0) c->cfg.world = 1;
    if (cfg->device != SAGE2OV_DEVICE_NONE) {
        const int ordinal = cfg->device; const double share = 1.0 / (double)c->cfg.world;
        auto open = [c, ordinal, share] { c->dev_ = dev_create(ordinal, c->opt, c->devErr); if (c->dev_) dev_set_probe_share(c->dev_, share); };
        if (cfg->flags & SAGE2OV_FLAG_ASYNC_DEVICE) c->devOpen = std::thread(open);      // the caller stages its input meanwhile; device() joins
        else { open(); if (!c->dev_) { g_create_error = c->devErr; delete c; return SAGE2OV_ERR_DEVICE; } }
    }
    *out = c; return SAGE2OV_OK;
}
void sage2ov_ctx_destroy(sage2ov_ctx* c) { if (!c) return; if (Device* d = c->device()) dev_destroy(d); delete c; }
int sage2ov_options_reload(sage2ov_ctx* c) { if (!c) return SAGE2OV_ERR_ARG; c->opt = s2::Options::from_env(); if (Device* d = c->device()) dev_set_options(d, c->opt); return SAGE2OV_OK; }

int sage2ov_reads_add_ascii(sage2ov_ctx* c, const char* bases, const uint64_t* off, uint64_t n) {
    if (!c || !bases || !off) return SAGE2OV_ERR_ARG;
    if (c->organized) return c->fail(SAGE2OV_ERR_ARG, "reads already organised");
    if (c->pairLib && n >= PAIR_CALL_RECORDS_MAX) return pair_call_limit(c);
    if (c->gpu() && !c->opt.get("SAGE2OV_HOST_PACK") && !c->opt.get("SAGE2OV_HOST_ORGANIZE")) {        // staged as they come: the device filters and packs them
        if (c->asciiOff.empty()) c->asciiOff.push_back(0);
        const uint64_t base = c->ascii.size(), first = off[0], bytes = off[n] - first;
        c->ascii.insert(c->ascii.end(), bases + first, bases + first + bytes);
        if (c->pairLib) c->pairCalls.push_back({c->pairLib, true, n, (uint64_t)c->asciiOff.size() - 1, 0, 0});      // (raw input: a record's ordinal is its index)
        for (uint64_t r = 1; r <= n; r++) c->asciiOff.push_back(base + (off[r] - first));
        c->totalReads += n;
        return SAGE2OV_OK;
    }
    std::vector<uint8_t> codes; const uint64_t first0 = c->poolLen.size(), ordAt0 = c->pairOrd.size();
    for (uint64_t r = 0; r < n; r++) {
        const int L = (int)(off[r + 1] - off[r]); codes.resize(L);
        for (int i = 0; i < L; i++) codes[i] = g_code[(unsigned char)bases[off[r] + i]];
        const size_t at = c->poolLen.size();
        stage_codes(c, codes.data(), L, c->pool, c->poolOff, c->poolLen, c->goodReads, c->totalBP, c->smallReads);
        if (c->pairLib && c->poolLen.size() > at) c->pairOrd.push_back((uint32_t)r);
        c->totalReads++;
    }
    if (c->pairLib) c->pairCalls.push_back({c->pairLib, false, n, first0, c->poolLen.size() - first0, ordAt0});
    return SAGE2OV_OK;
}
int sage2ov_reads_add_file(sage2ov_ctx* c, const char* p1, const char* p2) {
    if (!c || !p1) return SAGE2OV_ERR_ARG;
    if (c->organized) return c->fail(SAGE2OV_ERR_ARG, "reads already organised");
    return add_files(c, p1, p2, c->pairLib);
}
int sage2ov_reads_pair_library(sage2ov_ctx* c, int library) {
    if (!c) return SAGE2OV_ERR_ARG;
    if (c->organized) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_reads_pair_library: reads already organised");
    if (library < 0 || library > 127) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_reads_pair_library: the library must be 0 (off) or 1 .. 127");
    c->pairLib = library; return SAGE2OV_OK;
}
int sage2ov_reads_add_list(sage2ov_ctx* c, const char* lp) {                         // readLoader.cpp:73-131
    if (!c || !lp) return SAGE2OV_ERR_ARG;
    FILE* f = fopen(lp, "r"); if (!f) return c->fail(SAGE2OV_ERR_IO, std::string("cannot open ") + lp);
    char buf[8192]; std::string val1; unsigned mate = 0; int rc = SAGE2OV_OK;
    while (fgets(buf, sizeof buf, f)) {
        std::string line = buf; while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        size_t p = line.find('=');
        if (p == std::string::npos) { rc = c->fail(SAGE2OV_ERR_IO, "list of input files in a wrong format"); break; }
        std::string var = trim(line.substr(0, p)), val = trim(line.substr(p + 1));
        const int lib = c->pairLib ? (int)(mate / 2) + 1 : 0;                            // with pairing: dataset i is library i (matePair.cpp:102, :107)
        if (lib > 127 && (var == "f" || var == "f2")) { rc = c->fail(SAGE2OV_ERR_ARG, "sage2ov_reads_add_list: more than 127 datasets with pairing on"); break; }
        if (mate % 2 == 0 && var == "f1") val1 = val;
        else if (mate % 2 == 0 && var == "f") { rc = add_files(c, val.c_str(), nullptr, lib); mate++; }
        else if (mate % 2 == 1 && var == "f2") rc = add_files(c, val1.c_str(), val.c_str(), lib);
        else { rc = c->fail(SAGE2OV_ERR_IO, "list of input files in a wrong format"); }
        if (rc) break;
        mate++;
    }
    fclose(f); return rc;
}

int sage2ov_reads_add_synth(sage2ov_ctx* c, const sage2ov_synth_params* p, const uint8_t* genome, uint64_t first, uint64_t n) {
    if (!c || !p || !genome) return SAGE2OV_ERR_ARG;
    if (c->organized) return c->fail(SAGE2OV_ERR_ARG, "reads already organised");
    const int nt = io_threads(c);
    std::vector<std::vector<uint64_t>> pools(nt), offs(nt); std::vector<std::vector<uint16_t>> lens(nt);
    std::vector<uint64_t> good(nt, 0), bp(nt, 0), small(nt, 0);
    int rcAll = 0;
    #pragma omp parallel num_threads(nt)
    {
        const int t = omp_get_thread_num(); const uint64_t chunk = (n + nt - 1) / nt, a = first + t * chunk, b = std::min(first + n, a + chunk);
        std::vector<char> bases(p->read_len + 1); std::vector<uint8_t> codes(p->read_len + 1); uint64_t o[2];
        for (uint64_t r = a; r < b; r++) {
            int rc = sage2ov_synth_reads_ascii(p, genome, r, 1, bases.data(), o);
            if (rc) { rcAll = rc; break; }
            const int L = (int)o[1];
            for (int i = 0; i < L; i++) codes[i] = g_code[(unsigned char)bases[i]];
            stage_codes(c, codes.data(), L, pools[t], offs[t], lens[t], good[t], bp[t], small[t]);
        }
    }
    if (rcAll) return c->fail(rcAll, "synthetic generator failed");
    for (int t = 0; t < nt; t++) {                                  // concatenate in read order (thread t holds a contiguous slice)
        const uint64_t base = c->pool.size();
        c->pool.insert(c->pool.end(), pools[t].begin(), pools[t].end());
        for (uint64_t o : offs[t]) c->poolOff.push_back(base + o);
        c->poolLen.insert(c->poolLen.end(), lens[t].begin(), lens[t].end());
        c->goodReads += good[t]; c->totalBP += bp[t]; c->smallReads += small[t];
    }
    c->totalReads += n;
    return SAGE2OV_OK;
}

static int upload(sage2ov_ctx* c) {
    if (c->gpu() && !c->device()) return c->fail(SAGE2OV_ERR_DEVICE, c->devErr);
    if (!c->device()) { c->organized = true; c->mates_forget(); return SAGE2OV_OK; }      // step-1-only context (SAGE2OV_DEVICE_NONE)
    int minL = c->N ? 0xFFFF : 0; for (uint64_t i = 1; i <= c->N; i++) minL = std::min<int>(minL, c->len[i]);
    int rc = dev_upload_reads(c->device(), c->words.data(), c->N, c->S, minL, c->maxL, (int)c->cfg.min_overlap, c->err);
    if (rc) return rc;
    c->organized = true; c->mates_forget(); c->indexBuilt = c->probed = c->reciprocalDone = c->reduced = c->converted = false;
    return SAGE2OV_OK;
}
// a slot of S words holds the bases and, in the low 9 bits of its last word, the length: 123 / 251 / 507 bases for S = 4 / 8 / 16
static constexpr uint64_t slot_len_mask(int S) { return S > 16 ? 0x7FFull : 0x1FFull; }     // (kernels_common.inc: the 32-word layout keeps 11 bits)
#define SLOT_LEN_MASK slot_len_mask(c->S)
// words per slot: 2 bits per base + the length field (9 bits up to 16 words = 504 bases, 11 bits in the 32-word layout = 1018 bases)
static int choose_S(int maxL) { int need = (2 * maxL + 9 + 63) / 64; int S = 4; while (S < need) S *= 2; if (S > 16) { need = (2 * maxL + 11 + 63) / 64; S = need <= 32 ? 32 : 64; } return S; }

int sage2ov_reads_organize(sage2ov_ctx* c) {                                          // readLoader.cpp:215-260
    if (!c) return SAGE2OV_ERR_ARG;
    if (c->organized) return c->fail(SAGE2OV_ERR_ARG, "reads already organised");
    if (c->gpu() && !c->device()) return c->fail(SAGE2OV_ERR_DEVICE, c->devErr);      // (a device opened in the background: this is where a failure surfaces)
    const int nthr = io_threads(c);                                                   // (clauses, not omp_set_num_threads: a library call must not change the host's OpenMP state)
    if (!c->asciiOff.empty() && !c->poolLen.empty()) {                                // both kinds of input staged: pack the ASCII here and organise one pool
        std::vector<uint8_t> codes; const uint64_t na = c->asciiOff.size() - 1;
        auto stage_raw = [&](uint64_t r) { const int L = (int)(c->asciiOff[r + 1] - c->asciiOff[r]); codes.resize(L); for (int i = 0; i < L; i++) codes[i] = g_code[(unsigned char)c->ascii[c->asciiOff[r] + i]];
            stage_codes(c, codes.data(), L, c->pool, c->poolOff, c->poolLen, c->goodReads, c->totalBP, c->smallReads); };
        uint64_t r = 0;
        for (auto& P : c->pairCalls) if (P.raw) {                                      // (pairing: a raw call becomes a pool call; the raw calls are disjoint and ascend, and the staging order is free)
            for (; r < P.first; r++) stage_raw(r);
            const uint64_t first0 = c->poolLen.size(), ordAt0 = c->pairOrd.size();
            for (; r < P.first + P.records; r++) { const size_t at = c->poolLen.size(); stage_raw(r); if (c->poolLen.size() > at) c->pairOrd.push_back((uint32_t)(r - P.first)); }
            P.raw = false; P.first = first0; P.count = c->poolLen.size() - first0; P.ordAt = ordAt0;
        }
        for (; r < na; r++) stage_raw(r);
        std::vector<char>().swap(c->ascii); std::vector<uint64_t>().swap(c->asciiOff);
    }
    if (!c->asciiOff.empty()) {                                                       // ASCII only: step 1 entirely on the device
        OrgAscii A{c->ascii.data(), c->ascii.size(), c->asciiOff.data(), c->asciiOff.size() - 1};
        uint64_t N = 0;
        int rc = dev_organize_reads(c->device(), nullptr, 0, nullptr, nullptr, 0, 0, 0, 0, (int)c->cfg.min_overlap, &N, c->words, c->freq, c->err, &A, !c->pairCalls.empty());
        if (rc) return rc;
        c->goodReads += A.good; c->totalBP += A.total_bp; c->smallReads += A.small; c->maxL = A.maxL; c->S = A.S;
        c->N = N; c->len.assign(N + 1, 0);
        #pragma omp parallel for num_threads(nthr)
        for (uint64_t i = 1; i <= N; i++) c->len[i] = (uint16_t)(c->words[i * c->S + c->S - 1] & SLOT_LEN_MASK);
        std::vector<char>().swap(c->ascii); std::vector<uint64_t>().swap(c->asciiOff);
        c->organized = true; c->mates_forget(); c->indexBuilt = c->probed = c->reciprocalDone = c->reduced = c->converted = false;
        c->pairReady = c->pairOnDevice = !c->pairCalls.empty();
        return SAGE2OV_OK;
    }
    const uint64_t n = c->poolLen.size(); HostLap lap(c, "step 1");
    int maxL = 0; for (uint64_t i = 0; i < n; i++) maxL = std::max<int>(maxL, c->poolLen[i]);
    c->maxL = maxL; c->S = choose_S(std::max(maxL, 1));
    if (c->S > 32 || maxL > 1018) return c->fail(SAGE2OV_ERR_LIMIT, "reads longer than 1018 bases are not supported");
    if (n >= (1ull << 32)) return c->fail(SAGE2OV_ERR_LIMIT, "too many reads for the host organiser");
    for (uint64_t i = 0; i < n; i++) if (c->poolLen[i] == 0xFFFF) return c->fail(SAGE2OV_ERR_LIMIT, "reads longer than 1018 bases are not supported");
    if (c->device() && !c->opt.get("SAGE2OV_HOST_ORGANIZE")) {                                 // step 1 on the device: canonical orientation, sort, unique, ids
        uint64_t N = 0;
        int minL = n ? 0xFFFF : 0; for (uint64_t i = 0; i < n; i++) minL = std::min<int>(minL, c->poolLen[i]);
        lap("length scans");
        int rc = dev_organize_reads(c->device(), c->pool.data(), c->pool.size(), c->poolOff.data(), c->poolLen.data(), n, c->S, minL, c->maxL, (int)c->cfg.min_overlap,
                                    &N, c->words, c->freq, c->err, nullptr, !c->pairCalls.empty());
        if (rc) return rc;
        lap("device organiser (incl. transfers)");
        c->N = N; c->len.assign(N + 1, 0);
        #pragma omp parallel for num_threads(nthr)
        for (uint64_t i = 1; i <= N; i++) c->len[i] = (uint16_t)(c->words[i * c->S + c->S - 1] & SLOT_LEN_MASK);
        RawU64().swap(c->pool); RawU64().swap(c->poolOff); RawU16().swap(c->poolLen);
        lap("lengths + release of the staging");
        c->organized = true; c->mates_forget(); c->indexBuilt = c->probed = c->reciprocalDone = c->reduced = c->converted = false;
        c->pairReady = c->pairOnDevice = !c->pairCalls.empty();
        return SAGE2OV_OK;
    }
    const bool pairing = !c->pairCalls.empty(); std::vector<uint8_t> fwd(pairing ? n : 0);      // pairing: whether every staged read stayed as given (the sign of its id)
    #pragma omp parallel for num_threads(nthr)
    for (uint64_t i = 0; i < n; i++) { const bool f = canonicalise_words(&c->pool[c->poolOff[i]], c->poolLen[i]); if (pairing) fwd[i] = f; }
    std::vector<uint32_t> ord(n);
    #pragma omp parallel for num_threads(nthr)
    for (uint64_t i = 0; i < n; i++) ord[i] = (uint32_t)i;
    const uint64_t* pool = c->pool.data(); const uint64_t* off = c->poolOff.data(); const uint16_t* pl = c->poolLen.data();
    auto cmp = [&](uint32_t a, uint32_t b) -> int {                                   // utils.cpp:224-242 on big-endian words
        const int la = pl[a], lb = pl[b], wa = (la + 31) / 32, wb = (lb + 31) / 32, wm = std::min(wa, wb);
        const uint64_t *pa = pool + off[a], *pb = pool + off[b];
        for (int w = 0; w < wm; w++) { if (pa[w] != pb[w]) return pa[w] < pb[w] ? -1 : 1; }
        // bytes beyond the shorter read's last WORD may still be inside its last byte range: the reference compares
        // ceil(len/4) bytes, all of which lie in the first wm words except when the longer read has more words;
        // those extra bytes only matter while they are within min(bytes): they are not (min bytes <= 8*wm).
        if (la != lb) {
            // the shorter read is zero padded inside its last word, so a difference within min(bytes) was caught above
            return la < lb ? -1 : 1;
        }
        return 0;
    };
    __gnu_parallel::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return cmp(a, b) < 0; }, __gnu_parallel::default_parallel_tag(nthr));   // readLoader.cpp:221
    // unique + frequency (readLoader.cpp:225-235)
    std::vector<uint32_t> firstOf; firstOf.reserve(n); std::vector<uint16_t> fr; fr.reserve(n);
    if (pairing) c->pairIds.assign(n, 0);
    for (uint64_t x = 0; x < n; x++) {
        if (x == 0 || cmp(ord[x - 1], ord[x]) != 0) { firstOf.push_back(ord[x]); fr.push_back(0); }
        fr.back()++;                                                                  // u16 wrap like the reference
        if (pairing) { const int32_t id = (int32_t)firstOf.size(); c->pairIds[ord[x]] = fwd[ord[x]] ? id : -id; }      // the sign of sage2ov_reads_find_ids
    }
    const uint64_t N = firstOf.size(); const int S = c->S;
    c->N = N; c->words.assign((N + 1) * S, 0); c->len.assign(N + 1, 0); c->freq.assign(N + 1, 0);
    #pragma omp parallel for num_threads(nthr)
    for (uint64_t i = 1; i <= N; i++) {
        const uint32_t a = firstOf[i - 1]; const int L = pl[a], nw = (L + 31) / 32;
        uint64_t* w = &c->words[i * S];
        for (int q = 0; q < nw; q++) w[q] = pool[off[a] + q];
        w[S - 1] |= (uint64_t)L;                                                       // length in the low 9 bits of the last word
        c->len[i] = (uint16_t)L; c->freq[i] = fr[i - 1];
    }
    RawU64().swap(c->pool); RawU64().swap(c->poolOff); RawU16().swap(c->poolLen);
    const int rc = upload(c);
    if (rc == SAGE2OV_OK) c->pairReady = pairing; else std::vector<int32_t>().swap(c->pairIds);
    return rc;
}

int sage2ov_reads_stats(const sage2ov_ctx* c, sage2ov_read_stats* o) {
    if (!c || !o) return SAGE2OV_ERR_ARG;
    o->total_reads = c->totalReads; o->good_reads = c->goodReads; o->unique_reads = c->N; o->total_bp = c->totalBP;
    o->average_read_length = c->goodReads ? c->totalBP / c->goodReads : 0; o->max_read_length = (uint32_t)c->maxL; o->words_per_read = (uint32_t)c->S;
    return SAGE2OV_OK;
}
static void unpack_bytes(const uint64_t* w, int L, uint8_t* out, uint64_t stride) {    // word image -> utils.cpp:96 byte image
    const int nb = (L + 3) / 4; for (uint64_t b = 0; b < stride; b++) out[b] = 0;
    for (int b = 0; b < nb && (uint64_t)b < stride; b++) out[b] = (uint8_t)(w[b >> 3] >> (56 - 8 * (b & 7)));
    if (L & 3) out[nb - 1] &= (uint8_t)(0xFF << (8 - 2 * (L & 3)));
}
int sage2ov_reads_export(const sage2ov_ctx* c, uint8_t* packed, uint64_t stride, uint16_t* length, uint16_t* frequency) {
    if (!c || !c->organized) return SAGE2OV_ERR_ARG;
    for (uint64_t i = 0; i <= c->N; i++) {
        if (packed) { if (i == 0) memset(packed, 0, stride); else unpack_bytes(&c->words[i * c->S], c->len[i], packed + i * stride, stride); }
        if (length) length[i] = c->len[i];
        if (frequency) frequency[i] = c->freq[i];
    }
    return SAGE2OV_OK;
}
static void words_to_ascii(const uint64_t* w, int L, char* out) { static const char B[4] = {'A', 'C', 'G', 'T'}; for (int i = 0; i < L; i++) out[i] = B[(w[i >> 5] >> (62 - 2 * (i & 31))) & 3]; }
int sage2ov_reads_save(sage2ov_ctx* c, const char* path) {                            // readLoader.cpp:270-287, :29-36
    if (!c || !path || !c->organized) return SAGE2OV_ERR_ARG;
    FILE* f = fopen(path, "w"); if (!f) return c->fail(SAGE2OV_ERR_IO, std::string("cannot open ") + path);
    std::vector<char> io(1 << 22); setvbuf(f, io.data(), _IOFBF, io.size());
    fprintf(f, "%llu\n", (unsigned long long)c->N);
    const int S = c->S;
    int rc = write_formatted(c, f, c->N, (size_t)(2 * c->maxL + 24), [&](uint64_t x, std::string& o) {
        const uint64_t i = x + 1; const int L = c->len[i]; const uint64_t* w = &c->words[i * S];
        uint64_t tmp[34], r[34]; const int nw = (L + 31) / 32; for (int q = 0; q < nw; q++) tmp[q] = w[q]; if (nw == S) tmp[nw - 1] &= ~SLOT_LEN_MASK;
        revcomp_words(tmp, nw, L, r);
        char hd[48]; char* p = put_u(hd, c->freq[i]); *p++ = '\t'; p = put_u(p, (unsigned)L); *p++ = '\t';
        const size_t at = o.size(); o.resize(at + (size_t)(p - hd) + 2 * (size_t)L + 2);
        char* d = &o[at]; memcpy(d, hd, (size_t)(p - hd)); d += p - hd;
        words_to_ascii(tmp, L, d); d += L; *d++ = '\t'; words_to_ascii(r, L, d); d += L; *d++ = '\n';
    });
    fclose(f); return rc;
}
// P.reads as the writers produce it (readLoader.cpp:29-36: "frequency TAB length TAB read TAB reverse complement NL" per read, N on the first line), mapped and
// parsed by all I/O threads: a first pass over line-aligned chunks counts the lines and finds the longest read, a second packs every read straight into its slot
// (eight bases per step, pack8).  1: loaded.  0: the file is not strictly of that shape (other separators, CRLF, a sequence whose length differs from its length
// field, a wrong line count, ...) -- the fscanf reader below then takes it, with the reference's token semantics.  < 0: error.
static int reads_load_parallel(sage2ov_ctx* c, const char* path) {
    const int fd = ::open(path, O_RDONLY); if (fd < 0) return 0;
    struct stat sb; if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size < 4) { ::close(fd); return 0; }
    const size_t size = (size_t)sb.st_size;
    const char* m = (const char*)mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0); ::close(fd);
    if (m == MAP_FAILED) return 0;
    struct Unmap { const char* p; size_t n; ~Unmap() { munmap((void*)p, n); } } um{m, size};
    madvise((void*)m, size, MADV_SEQUENTIAL);
    size_t h = 0; uint64_t N = 0; while (h < size && m[h] >= '0' && m[h] <= '9' && h < 19) N = N * 10 + (uint64_t)(m[h++] - '0');
    if (h == 0 || h >= size || m[h] != '\n') return 0;
    h++;
    if (N >= (1ull << 32) || m[size - 1] != '\n') return 0;
    const int nt = io_threads(c); const size_t nchunks = (size_t)nt * 4;
    std::vector<size_t> cut(nchunks + 1); cut[0] = h; cut[nchunks] = size;
    for (size_t x = 1; x < nchunks; x++) { size_t p = h + (size - h) / nchunks * x; if (p < cut[x - 1]) p = cut[x - 1]; const char* nl = (const char*)memchr(m + p, '\n', size - p); cut[x] = nl ? (size_t)(nl - m) + 1 : size; }
    // one line: digits TAB digits TAB <len> characters TAB ... NL; returns the position behind the line, 0 when the line is not of that shape
    auto line = [&](size_t p, size_t e, uint64_t& fr, uint64_t& L, size_t& sq) -> size_t {
        size_t q = p; fr = 0; while (q < e && m[q] >= '0' && m[q] <= '9' && q - p < 10) fr = fr * 10 + (uint64_t)(m[q++] - '0');
        if (q == p || q >= e || m[q] != '\t') return 0;
        const size_t p2 = ++q; L = 0; while (q < e && m[q] >= '0' && m[q] <= '9' && q - p2 < 7) L = L * 10 + (uint64_t)(m[q++] - '0');
        if (q == p2 || q >= e || m[q] != '\t') return 0;
        sq = ++q; if (sq + L >= e || m[sq + L] != '\t') return 0;
        const char* nl = (const char*)memchr(m + sq + L + 1, '\n', e - (sq + L + 1)); if (!nl) return 0;
        return (size_t)(nl - m) + 1;
    };
    std::vector<uint64_t> cnt(nchunks + 1, 0); std::vector<int> mx(nchunks, 0); bool bad = false;
    #pragma omp parallel for num_threads(nt) schedule(dynamic, 1)
    for (int64_t x = 0; x < (int64_t)nchunks; x++) {
        size_t p = cut[x]; const size_t e = cut[x + 1]; uint64_t n = 0, fr, L; size_t sq; int ml = 0;
        while (p < e) {
            const size_t nx = line(p, e, fr, L, sq);
            bool ws = false; if (nx) for (size_t i = 0; i < L; i++) ws |= (unsigned char)m[sq + i] <= ' ';
            if (!nx || ws || L > 1018) {
                #pragma omp atomic write
                bad = true;
                break;
            }
            ml = std::max(ml, (int)L); n++; p = nx;
        }
        cnt[x + 1] = n; mx[x] = ml;
    }
    if (bad) return 0;
    int maxL = 0; for (size_t x = 0; x < nchunks; x++) { cnt[x + 1] += cnt[x]; maxL = std::max(maxL, mx[x]); }
    if (cnt[nchunks] != N) return 0;
    c->maxL = maxL; c->S = choose_S(std::max(maxL, 1)); const int S = c->S;
    c->N = N; c->words.resize((N + 1) * S); c->len.resize(N + 1); c->freq.resize(N + 1);
    for (int q = 0; q < S; q++) c->words[q] = 0;
    c->len[0] = 0; c->freq[0] = 0;
    #pragma omp parallel for num_threads(nt) schedule(dynamic, 1)
    for (int64_t x = 0; x < (int64_t)nchunks; x++) {
        size_t p = cut[x]; const size_t e = cut[x + 1]; uint64_t i = cnt[x] + 1, fr, L; size_t sq;
        while (p < e) {
            p = line(p, e, fr, L, sq);
            uint64_t* w = &c->words[i * S]; for (int q = 0; q < S; q++) w[q] = 0;
            const char* b = m + sq; int y = 0;
            for (; y + 8 <= (int)L; y += 8) {
                uint64_t v, o; memcpy(&v, b + y, 8);
                if (!pack8(v, o)) { o = 0; for (int z = 0; z < 8; z++) { uint8_t cd = g_code[(unsigned char)b[y + z]]; if (cd > 3) cd = 0; o |= (uint64_t)cd << (14 - 2 * z); } }   // (anything but ACGT reads as A, like the loop below)
                w[y >> 5] |= o << (48 - 2 * (y & 31));
            }
            for (; y < (int)L; y++) { uint8_t cd = g_code[(unsigned char)b[y]]; if (cd > 3) cd = 0; w[y >> 5] |= (uint64_t)cd << (62 - 2 * (y & 31)); }
            w[S - 1] |= L; c->len[i] = (uint16_t)L; c->freq[i] = (uint16_t)(unsigned)fr;
            i++;
        }
    }
    return 1;
}
int sage2ov_reads_load(sage2ov_ctx* c, const char* path) {                            // readLoader.cpp:289-307, :38-48
    if (!c || !path) return SAGE2OV_ERR_ARG;
    if (!c->opt.get("SAGE2OV_SEQUENTIAL_READER")) { const int pr = reads_load_parallel(c, path); if (pr < 0) return pr; if (pr == 1) { c->organized = false; return upload(c); } }
    FILE* f = fopen(path, "r"); if (!f) return c->fail(SAGE2OV_ERR_IO, std::string("cannot open ") + path);
    unsigned long long N = 0; if (fscanf(f, "%llu", &N) != 1) { fclose(f); return c->fail(SAGE2OV_ERR_IO, "bad .reads header"); }
    std::vector<std::string> seqs(N + 1); std::vector<unsigned> fr(N + 1), ln(N + 1); int maxL = 0;
    std::vector<char> a(70000), b(70000);
    for (unsigned long long i = 1; i <= N; i++) {
        if (fscanf(f, "%u %u %69999s %69999s", &fr[i], &ln[i], a.data(), b.data()) != 4) { fclose(f); return c->fail(SAGE2OV_ERR_IO, "bad .reads record"); }
        seqs[i] = a.data(); maxL = std::max<int>(maxL, (int)ln[i]);
    }
    fclose(f);
    c->maxL = maxL; c->S = choose_S(std::max(maxL, 1)); if (c->S > 32) return c->fail(SAGE2OV_ERR_LIMIT, "reads longer than 1018 bases are not supported");
    c->N = N; const int S = c->S; c->words.assign((N + 1) * S, 0); c->len.assign(N + 1, 0); c->freq.assign(N + 1, 0);
    for (unsigned long long i = 1; i <= N; i++) {
        const int L = (int)ln[i]; uint64_t* w = &c->words[i * S];
        for (int p = 0; p < L && p < (int)seqs[i].size(); p++) { uint8_t x = g_code[(unsigned char)seqs[i][p]]; if (x > 3) x = 0; w[p >> 5] |= (uint64_t)x << (62 - 2 * (p & 31)); }
        w[S - 1] |= (uint64_t)L; c->len[i] = (uint16_t)L; c->freq[i] = (uint16_t)fr[i];
    }
    c->organized = false;
    return upload(c);
}
// word-layout image of the organised reads (what lives in HBM): lets one rank organise and the others import
int sage2ov_reads_export_words(const sage2ov_ctx* c, uint64_t* words, uint64_t cap_words, uint16_t* frequency) {
    if (!c || !c->organized || !words) return SAGE2OV_ERR_ARG;
    if (cap_words < c->words.size()) return SAGE2OV_ERR_ARG;
    memcpy(words, c->words.data(), c->words.size() * sizeof(uint64_t));
    if (frequency) memcpy(frequency, c->freq.data(), (c->N + 1) * sizeof(uint16_t));
    return SAGE2OV_OK;
}
int sage2ov_reads_import_words(sage2ov_ctx* c, const uint64_t* words, uint64_t n_unique, uint32_t words_per_read, uint32_t max_read_length,
                               const uint16_t* frequency, uint64_t good_reads, uint64_t total_bp) {
    if (!c || !words) return SAGE2OV_ERR_ARG;
    if (words_per_read != 4 && words_per_read != 8 && words_per_read != 16 && words_per_read != 32) return c->fail(SAGE2OV_ERR_ARG, "words_per_read must be 4, 8, 16 or 32");
    c->N = n_unique; c->S = (int)words_per_read; c->maxL = (int)max_read_length;
    c->words.assign(words, words + (n_unique + 1) * words_per_read);
    c->len.assign(n_unique + 1, 0); c->freq.assign(n_unique + 1, 0);
    for (uint64_t i = 1; i <= n_unique; i++) { c->len[i] = (uint16_t)(c->words[i * c->S + c->S - 1] & SLOT_LEN_MASK); c->freq[i] = frequency ? frequency[i] : 1; }
    c->goodReads = good_reads; c->totalBP = total_bp; c->totalReads = good_reads; c->organized = false;
    return upload(c);
}
// ReadLoader::getIdOfRead (readLoader.cpp:319-353) on the host copy of the store: isGoodRead, canonical orientation, pack, binary search with the slot compare
// (words in order, the last one carrying the length = stringCompareInBytes, utils.cpp:224).  The route of a device-less context, and of a GPU context
// whose device holds no read store.
static void find_ids_host(const sage2ov_ctx* c, const char* bases, const uint64_t* off, uint64_t n, int64_t* ids, sage2ov_find_stats& st) {
    const int S = c->S; const uint64_t N = c->N; const uint64_t* words = c->words.data();
    const uint64_t k = c->cfg.min_overlap, maxL = std::min<uint64_t>((uint64_t)std::max(c->maxL, 0), (64 * (uint64_t)S - (S > 16 ? 11 : 9)) / 2);
    uint64_t found = 0, notGood = 0;
    #pragma omp parallel for num_threads(io_threads(c)) schedule(dynamic, 1024) reduction(+ : found, notGood)
    for (uint64_t r = 0; r < n; r++) {
        const unsigned char* b = (const unsigned char*)bases + off[r]; const uint64_t Ls = off[r + 1] - off[r];
        ids[r] = 0;
        if (Ls <= k) { notGood++; continue; }
        bool valid = true; for (uint64_t i = 0; i < Ls && valid; i++) valid = g_code[b[i]] <= 3;
        if (!valid) { notGood++; continue; }
        if (Ls > maxL) continue;                                                       // longer than every read of the store: not found
        const int L = (int)Ls, nw = (L + 31) / 32; uint64_t f[34], rc[34], q[32];
        for (int w = 0; w < nw; w++) f[w] = 0;
        for (int i = 0; i < L; i++) f[i >> 5] |= (uint64_t)g_code[b[i]] << (62 - 2 * (i & 31));
        revcomp_words(f, nw, L, rc);
        bool useF = false;                                                             // :325: strictly smaller, else the reverse complement (a tie too)
        for (int w = 0; w < nw; w++) if (f[w] != rc[w]) { useF = f[w] < rc[w]; break; }
        for (int w = 0; w < S; w++) q[w] = w < nw ? (useF ? f[w] : rc[w]) : 0;
        q[S - 1] |= (uint64_t)L;
        uint64_t lb = 1, ub = N;                                                       // :335-348
        while (lb <= ub) {
            const uint64_t mid = (lb + ub) >> 1; const uint64_t* s = words + mid * S; int cmp = 0;
            for (int w = 0; w < S; w++) if (q[w] != s[w]) { cmp = q[w] < s[w] ? -1 : 1; break; }
            if (cmp == 0) { ids[r] = useF ? (int64_t)mid : -(int64_t)mid; found++; break; }
            if (cmp > 0) lb = mid + 1; else ub = mid - 1;
        }
    }
    st.found = found; st.not_good = notGood; st.route = SAGE2OV_FIND_ROUTE_HOST;
}
int sage2ov_reads_find_ids(sage2ov_ctx* c, const char* bases, const uint64_t* off, uint64_t n, int64_t* ids) {
    if (!c) return SAGE2OV_ERR_ARG;
    if (!c->organized) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_reads_find_ids: organise (or load) the reads first");
    c->fstats = sage2ov_find_stats{}; c->fstats.queries = n;
    if (n == 0) return SAGE2OV_OK;
    if (!bases || !off || !ids) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_reads_find_ids: null argument");
    for (uint64_t r = 0; r < n; r++) if (off[r + 1] < off[r]) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_reads_find_ids: offsets must not decrease");
    if (c->gpu() && !c->device()) return c->fail(SAGE2OV_ERR_DEVICE, c->devErr);
    int route = 1;                                                                     // 1: nothing resident on a device (or no device): search the host copy
    if (Device* d = c->device()) {
        FindStats fs; route = dev_find_ids(d, bases, off, n, ids, &fs, c->err);
        if (route < 0) return route;
        if (route == 0) {
            c->fstats.found = fs.found; c->fstats.not_good = fs.not_good; c->fstats.directory_bits = fs.dirBits; c->fstats.launches = fs.launches;
            c->fstats.pack_ms = fs.pack_ms; c->fstats.search_ms = fs.search_ms; c->fstats.device_ms = fs.pack_ms + fs.search_ms; c->fstats.directory_ms = fs.dir_ms;
            c->fstats.route = fs.byPos ? SAGE2OV_FIND_ROUTE_LOCALITY : SAGE2OV_FIND_ROUTE_ID_STORE;
        }
    }
    if (route == 1) find_ids_host(c, bases, off, n, ids, c->fstats);
    c->fstats.not_found = n - c->fstats.found - c->fstats.not_good;
    return SAGE2OV_OK;
}
int sage2ov_reads_find_stats_get(const sage2ov_ctx* c, sage2ov_find_stats* o) { if (!c || !o) return SAGE2OV_ERR_ARG; *o = c->fstats; return SAGE2OV_OK; }
// ------------------------------------------------------------------------------------------ the mate-pair table
// MatePair::processMatePairs (matePair.cpp:161-239) as run with one thread; the semantics are stated in sage2ov.h.  A GPU context with a resident read store
// builds the table on the device (dev_mates_add); a device-less context, or a GPU context with no store resident, here: find_ids_host, the
// records (key = from:30 | to:30 | t_from:1 | t_to:1, ordinal) sorted, runs of equal keys reduced, the result merged into the library's sorted table.
namespace {
struct MateCall {                                      // one add call (one dataset of a list)
    int lib = 0; bool onDevice = false, routeKnown = false; MateStats ds; uint64_t before = 0;
    std::vector<std::pair<uint64_t, uint64_t>> rec;    // host route: (key, ordinal) of the call's records
    std::vector<int64_t> ids;
};
uint64_t mates_entries(sage2ov_ctx* c, int lib) { return c->mateOnDevice[lib] ? dev_mates_count(c->device(), lib) : c->mates[lib].key.size(); }
// the library's table goes where this call runs (only a context whose device lost or gained its read store between two calls ever moves one)
int mates_place(sage2ov_ctx* c, int lib, bool onDevice) {
    if (c->mateOnDevice[lib] == onDevice) return SAGE2OV_OK;
    auto& L = c->mates[lib]; Device* d = c->device();
    if (onDevice) {
        if (!L.key.empty()) { const int rc = dev_mates_import(d, lib, L.key.data(), L.cnt.data(), L.first.data(), L.key.size(), c->err); if (rc) return rc; }
        L = sage2ov_ctx::MateLib();
    } else {
        const uint64_t n = dev_mates_count(d, lib); L.key.resize(n); L.cnt.resize(n); L.first.resize(n);
        int rc = dev_mates_export(d, lib, L.key.data(), L.cnt.data(), L.first.data(), nullptr, c->err); if (rc) return rc;
        rc = dev_mates_import(d, lib, nullptr, nullptr, nullptr, 0, c->err); if (rc) return rc;
    }
    c->mateOnDevice[lib] = onDevice;
    return SAGE2OV_OK;
}
int mates_begin(sage2ov_ctx* c, int lib, MateCall& M) {
    M.lib = lib; M.before = mates_entries(c, lib);
    c->mstats = sage2ov_mate_stats{}; c->mstats.library = (uint32_t)lib; c->mstats.libraries = c->mateLibraries;
    c->mstats.entries_before = c->mstats.entries_after = M.before;
    return SAGE2OV_OK;
}
// one readsArray: reads [0, n) with n even
int mates_batch(sage2ov_ctx* c, MateCall& M, const char* bases, const uint64_t* off, uint64_t n) {
    if (n == 0) return SAGE2OV_OK;
    const int lib = M.lib; const uint64_t pair0 = c->matePairs[lib];
    if (!M.routeKnown) {                                                               // the first batch decides the route of the call
        int route = 1;
        if (Device* d = c->device()) {
            if (!c->mateOnDevice[lib]) { const int rc = mates_place(c, lib, true); if (rc) return rc; }
            route = dev_mates_add(d, bases, off, n, lib, pair0, &M.ds, c->err);
            if (route < 0) return route;
            if (route == 1) { const int rc = mates_place(c, lib, false); if (rc) return rc; }
        }
        M.routeKnown = true; M.onDevice = route == 0;
        if (M.onDevice) { c->matePairs[lib] += n / 2; return SAGE2OV_OK; }
    } else if (M.onDevice) {
        const int rc = dev_mates_add(c->device(), bases, off, n, lib, pair0, &M.ds, c->err);
        if (rc) return rc < 0 ? rc : c->fail(SAGE2OV_ERR_DEVICE, "mate table: the read store left the device during a call");
        c->matePairs[lib] += n / 2; return SAGE2OV_OK;
    }
    M.ids.resize(n); sage2ov_find_stats fs{};
    find_ids_host(c, bases, off, n, M.ids.data(), fs);
    const uint64_t k = c->cfg.min_overlap;
    for (uint64_t j = 0; j < n / 2; j++) {
        const int64_t a = M.ids[2 * j], b = M.ids[2 * j + 1];
        M.ds.seen++;
        if (!a || !b) {                                                                // not a good read (matePair.cpp:176), or a good read that is not in the store
            bool bad = false;
            for (uint64_t m = 2 * j; m < 2 * j + 2 && !bad; m++) {
                if (M.ids[m]) continue;
                const unsigned char* s = (const unsigned char*)bases + off[m]; const uint64_t Ls = off[m + 1] - off[m];
                bad = Ls <= k; for (uint64_t i = 0; i < Ls && !bad; i++) bad = g_code[s[i]] > 3;
            }
            if (bad) M.ds.not_good++; else M.ds.not_found++;
            continue;
        }
        const uint64_t id1 = (uint64_t)llabs(a), id2 = (uint64_t)llabs(b), t1 = a > 0, t2 = b > 0, o = 2 * (pair0 + j);      // :180-189
        M.rec.emplace_back((id1 << 32) | (id2 << 2) | (t1 << 1) | t2, o);
        M.rec.emplace_back((id2 << 32) | (id1 << 2) | (t2 << 1) | t1, o + 1);
        M.ds.added++;
    }
    c->matePairs[lib] += n / 2;
    return SAGE2OV_OK;
}
int mates_end(sage2ov_ctx* c, MateCall& M, int rc) {
    const int lib = M.lib;
    c->estimated = false; if (Device* d = c->device()) dev_readmap_drop_joins(d);      // flags and distances are recomputed by the next call that needs them
    if (M.onDevice) { if (rc == SAGE2OV_OK) rc = dev_mates_flush(c->device(), lib, &M.ds, c->err); if (rc != SAGE2OV_OK) dev_mates_abort(c->device()); }
    else if (rc == SAGE2OV_OK && !M.rec.empty()) {
        __gnu_parallel::sort(M.rec.begin(), M.rec.end(), std::less<std::pair<uint64_t, uint64_t>>(), __gnu_parallel::default_parallel_tag(io_threads(c)));
        auto& L = c->mates[lib]; sage2ov_ctx::MateLib out; size_t t = 0; const size_t nr = M.rec.size(), nt = L.key.size();
        for (size_t i = 0; i < nr;) {                                                  // a run of equal keys = one entry; the table's entries below it first
            size_t e = i + 1; while (e < nr && M.rec[e].first == M.rec[i].first) e++;
            const uint64_t key = M.rec[i].first;
            for (; t < nt && L.key[t] < key; t++) { out.key.push_back(L.key[t]); out.cnt.push_back(L.cnt[t]); out.first.push_back(L.first[t]); }
            uint64_t cnt = e - i, first = M.rec[i].second;
            if (t < nt && L.key[t] == key) { cnt += L.cnt[t]; first = std::min(first, L.first[t]); t++; }
            out.key.push_back(key); out.cnt.push_back(cnt); out.first.push_back(first);
            i = e;
        }
        for (; t < nt; t++) { out.key.push_back(L.key[t]); out.cnt.push_back(L.cnt[t]); out.first.push_back(L.first[t]); }
        L = std::move(out);
    }
    if (M.ds.seen) c->mateLibraries = std::max<uint32_t>(c->mateLibraries, (uint32_t)lib);
    sage2ov_mate_stats& s = c->mstats;
    s.pairs_seen = M.ds.seen; s.pairs_added = M.ds.added; s.pairs_not_good = M.ds.not_good; s.pairs_not_found = M.ds.not_found; s.records = 2 * M.ds.added;
    s.entries_after = mates_entries(c, lib); s.libraries = c->mateLibraries;
    s.chunks = M.ds.chunks; s.sort_passes = M.ds.passes; s.flushes = M.ds.flushes; s.route = M.onDevice ? SAGE2OV_MATE_ROUTE_DEVICE : SAGE2OV_MATE_ROUTE_HOST;
    s.find_ms = M.ds.find_ms; s.records_ms = M.ds.records_ms; s.sort_ms = M.ds.sort_ms; s.reduce_ms = M.ds.reduce_ms; s.merge_ms = M.ds.merge_ms;
    return rc;
}
int mates_check(sage2ov_ctx* c, const char* who, int lib) {
    if (!c->organized) return c->fail(SAGE2OV_ERR_ARG, std::string(who) + ": organise (or load) the reads first");
    if (lib < 1 || lib > 127) return c->fail(SAGE2OV_ERR_ARG, std::string(who) + ": the library must be 1 .. 127");
    if (c->gpu() && !c->device()) return c->fail(SAGE2OV_ERR_DEVICE, c->devErr);
    return SAGE2OV_OK;
}
// mapMatePairs (matePair.cpp:125-159): the file(s) through the sequential reader, two files in turn by parity (inputReader.cpp:26-49), in batches of an even
// number of reads so that the pairing is that of one continuous stream; the file is never staged whole
int mates_add_files(sage2ov_ctx* c, const char* p1, const char* p2, int lib) {
    SeqFile f1, f2; if (!f1.open(p1)) return c->fail(SAGE2OV_ERR_IO, std::string("cannot open ") + p1);
    const bool two = p2 && *p2; if (two && !f2.open(p2)) return c->fail(SAGE2OV_ERR_IO, std::string("cannot open ") + p2);
    const long long forced = c->opt.num("SAGE2OV_TEST_MATE_FILE_BATCH", 0);           // test-only: reads per batch (made even)
    const size_t BATCH = forced > 0 ? (size_t)((forced + 1) & ~1ll) : (size_t)1 << 20;
    MateCall M; int rc = mates_begin(c, lib, M);
    std::string flat; std::vector<uint64_t> boff; uint64_t inFile = 0; bool more = true;
    while (more && rc == SAGE2OV_OK) {
        flat.clear(); boff.clear(); boff.push_back(0);
        while (boff.size() <= BATCH) {
            SeqFile& f = (two && (inFile & 1)) ? f2 : f1;
            size_t len = 0;
            if (!f.next(flat, len)) { more = false; break; }
            boff.push_back(flat.size()); inFile++;
        }
        const uint64_t nb = (boff.size() - 1) & ~1ull;                                 // (only the last batch can be odd: its last read has no mate, :172)
        rc = mates_batch(c, M, flat.data(), boff.data(), nb);
    }
    for (SeqFile* f : {&f1, &f2}) if (rc == SAGE2OV_OK && f->ioError) {
        int en = 0; const char* m = f->fp ? gzerror(f->fp, &en) : nullptr;
        rc = c->fail(SAGE2OV_ERR_IO, std::string("read error in ") + (f == &f1 ? p1 : p2) + ": " + (m && *m ? m : "corrupt or truncated input"));
    }
    return mates_end(c, M, rc);
}
}  // namespace
int sage2ov_mates_add_ascii(sage2ov_ctx* c, const char* bases, const uint64_t* off, uint64_t n, int library) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = mates_check(c, "sage2ov_mates_add_ascii", library); if (rc) return rc; }
    if (n > 0 && (!bases || !off)) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_mates_add_ascii: null argument");
    for (uint64_t r = 0; r < n; r++) if (off[r + 1] < off[r]) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_mates_add_ascii: offsets must not decrease");
    MateCall M; int rc = mates_begin(c, library, M);
    if (rc == SAGE2OV_OK) rc = mates_batch(c, M, bases, off, n & ~1ull);               // a trailing odd read is dropped (matePair.cpp:172)
    return mates_end(c, M, rc);
}
int sage2ov_mates_add_file(sage2ov_ctx* c, const char* p1, const char* p2, int library) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = mates_check(c, "sage2ov_mates_add_file", library); if (rc) return rc; }
    if (!p1) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_mates_add_file: null argument");
    return mates_add_files(c, p1, p2, library);
}
int sage2ov_mates_add_list(sage2ov_ctx* c, const char* lp) {                          // matePair.cpp:70-120
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = mates_check(c, "sage2ov_mates_add_list", 1); if (rc) return rc; }
    if (!lp) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_mates_add_list: null argument");
    FILE* f = fopen(lp, "r"); if (!f) return c->fail(SAGE2OV_ERR_IO, std::string("cannot open ") + lp);
    char buf[8192]; std::string val1; unsigned mate = 0; int rc = SAGE2OV_OK;
    while (fgets(buf, sizeof buf, f)) {
        std::string line = buf; while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        size_t p = line.find('=');
        if (p == std::string::npos) { rc = c->fail(SAGE2OV_ERR_IO, "list of input files in a wrong format"); break; }
        std::string var = trim(line.substr(0, p)), val = trim(line.substr(p + 1));
        const int lib = (int)(mate / 2) + 1;                                           // :102, :107
        if (lib > 127 && (var == "f" || var == "f2")) { rc = c->fail(SAGE2OV_ERR_ARG, "sage2ov_mates_add_list: more than 127 datasets"); break; }
        if (mate % 2 == 0 && var == "f1") val1 = val;
        else if (mate % 2 == 0 && var == "f") { rc = mates_add_files(c, val.c_str(), nullptr, lib); mate++; }
        else if (mate % 2 == 1 && var == "f2") rc = mates_add_files(c, val1.c_str(), val.c_str(), lib);
        else { rc = c->fail(SAGE2OV_ERR_IO, "list of input files in a wrong format"); }
        if (rc) break;
        mate++;
    }
    fclose(f);
    if (rc == SAGE2OV_OK && mate % 2 == 1) rc = c->fail(SAGE2OV_ERR_IO, "list of input files in a wrong format");      // an f1 without its f2
    return rc;
}
int sage2ov_mates_count(sage2ov_ctx* c, int library, uint64_t* n) {
    if (!c || !n) return SAGE2OV_ERR_ARG;
    { const int rc = mates_check(c, "sage2ov_mates_count", library); if (rc) return rc; }
    *n = mates_entries(c, library); return SAGE2OV_OK;
}
int sage2ov_mates_export(sage2ov_ctx* c, int library, sage2ov_mate* out, uint64_t cap, uint64_t* offsets) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = mates_check(c, "sage2ov_mates_export", library); if (rc) return rc; }
    const uint64_t n = mates_entries(c, library);
    if (cap < n) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_mates_export: the buffer holds fewer entries than the table (sage2ov_mates_count)");
    if (n && !out) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_mates_export: null argument");
    const sage2ov_ctx::MateLib* L = &c->mates[library]; sage2ov_ctx::MateLib tmp;
    if (c->mateOnDevice[library]) {
        tmp.key.resize(n); tmp.cnt.resize(n); tmp.first.resize(n); L = &tmp;
        const int rc = dev_mates_export(c->device(), library, tmp.key.data(), tmp.cnt.data(), tmp.first.data(), offsets, c->err); if (rc) return rc;
    } else if (offsets) {
        uint64_t t = 0;
        for (uint64_t a = 0; a <= c->N + 1; a++) { while (t < n && (L->key[t] >> 32) < a) t++; offsets[a] = a == c->N + 1 ? n : t; }
    }
    #pragma omp parallel for num_threads(io_threads(c))
    for (uint64_t e = 0; e < n; e++) {
        const uint64_t k = L->key[e]; sage2ov_mate m{};
        m.from = (uint32_t)(k >> 32); m.to = (uint32_t)((k >> 2) & 0x3FFFFFFFu); m.type1 = (uint8_t)((k >> 1) & 1); m.type2 = (uint8_t)(k & 1);
        m.count = L->cnt[e]; m.first = L->first[e]; m.freq = (uint8_t)(m.count & 255); m.library = (uint8_t)library;
        out[e] = m;
    }
    return SAGE2OV_OK;
}
int sage2ov_mates_clear(sage2ov_ctx* c) {
    if (!c) return SAGE2OV_ERR_ARG;
    if (Device* d = c->device()) { dev_mates_clear(d); dev_readmap_drop_joins(d); dev_pairing_release(d); }    // (the read-to-edge table describes the graph, not the mates: it stays)
    c->mates_forget(false); return SAGE2OV_OK;
}
// The mate table of the reads this context organised, from step 1's own by-products: every reads_add_* call made with pairing on is one mates
// call.  Per call a dense slotOf[ordinal] = staging index + 1 (0: the record was not staged), then per pair both ids or a skip; the records and everything behind
// them are those of the mates_add_* route (mates_end / dev_mates_flush).
int sage2ov_mates_from_reads(sage2ov_ctx* c) {
    if (!c) return SAGE2OV_ERR_ARG;
    if (!c->organized) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_mates_from_reads: organise the reads first");
    if (!c->pairReady) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_mates_from_reads: the reads were not staged with pairing on (sage2ov_reads_pair_library), or their pairing was used or cleared");
    if (c->gpu() && !c->device()) return c->fail(SAGE2OV_ERR_DEVICE, c->devErr);
    int rc = SAGE2OV_OK;
    for (const auto& P : c->pairCalls) {
        const int lib = P.lib; MateCall M; rc = mates_begin(c, lib, M);
        const uint64_t pair0 = c->matePairs[lib], np = P.records / 2;                   // (a trailing odd record has no mate, matePair.cpp:172)
        if (rc == SAGE2OV_OK && c->pairOnDevice) {
            rc = mates_place(c, lib, true); M.routeKnown = M.onDevice = rc == SAGE2OV_OK;
            if (rc == SAGE2OV_OK) rc = dev_mates_pair_call(c->device(), P.raw, P.raw ? nullptr : c->pairOrd.data() + P.ordAt, P.count, P.first, P.records, lib, pair0, &M.ds, c->err);
        } else if (rc == SAGE2OV_OK && P.raw) rc = c->fail(SAGE2OV_ERR_INTERNAL, "pairing: a raw call without the device's ids");
        else if (rc == SAGE2OV_OK) {
            if (c->device() && c->mateOnDevice[lib]) rc = mates_place(c, lib, false);
            M.routeKnown = true;
            std::vector<uint32_t> slotOf(P.records, 0);
            for (uint64_t x = 0; x < P.count; x++) slotOf[c->pairOrd[P.ordAt + x]] = (uint32_t)(P.first + x + 1);
            for (uint64_t j = 0; rc == SAGE2OV_OK && j < np; j++) {
                const uint32_t sa = slotOf[2 * j], sb = slotOf[2 * j + 1];
                M.ds.seen++;
                if (!sa || !sb) { M.ds.not_good++; continue; }                         // only a read that is not good is not staged: "not in the store" cannot happen
                const int64_t a = c->pairIds[sa - 1], b = c->pairIds[sb - 1];
                const uint64_t id1 = (uint64_t)llabs(a), id2 = (uint64_t)llabs(b), t1 = a > 0, t2 = b > 0, o = 2 * (pair0 + j);
                M.rec.emplace_back((id1 << 32) | (id2 << 2) | (t1 << 1) | t2, o);
                M.rec.emplace_back((id2 << 32) | (id1 << 2) | (t2 << 1) | t1, o + 1);
                M.ds.added++;
            }
        }
        if (rc == SAGE2OV_OK) c->matePairs[lib] += np;
        rc = mates_end(c, M, rc);
        if (rc) break;
    }
    if (Device* d = c->device()) dev_pairing_release(d);
    c->pairing_forget();
    return rc;
}
int sage2ov_mates_stats_get(const sage2ov_ctx* c, sage2ov_mate_stats* o) { if (!c || !o) return SAGE2OV_ERR_ARG; *o = c->mstats; return SAGE2OV_OK; }
int sage2ov_reads_set_totals(sage2ov_ctx* c, uint64_t good, uint64_t bp) { if (!c) return SAGE2OV_ERR_ARG; c->goodReads = good; c->totalBP = bp; return SAGE2OV_OK; }

// ------------------------------------------------------------------------------------------ step 2
int sage2ov_index_build(sage2ov_ctx* c) {
    if (!c) return SAGE2OV_ERR_ARG;
    if (!c->device()) return c->fail(SAGE2OV_ERR_DEVICE, "this context has no GPU (SAGE2OV_DEVICE_NONE): steps 2-3 are device-only");
    if (!c->organized) return c->fail(SAGE2OV_ERR_ARG, "organise (or load) the reads first");
    uint64_t slots, keys, csr, nlong; uint32_t reb;
    int rc = dev_build_index(c->device(), &slots, &keys, &csr, &nlong, &reb, c->err); if (rc) return rc;
    c->istats.slots = slots; c->istats.keys = keys; c->istats.csr_entries = csr; c->istats.long_buckets = nlong;
    c->istats.hash_string_length = c->cfg.min_overlap > 64 ? 64 : c->cfg.min_overlap; c->istats.rebuilds = reb; c->istats.minimiser_groups = dev_has_minimiser_groups(c->device()) ? 1u : 0u; c->istats.reserved = 0;
    c->indexBuilt = true; c->probed = c->reciprocalDone = c->reduced = c->converted = false;
    return SAGE2OV_OK;
}
int sage2ov_index_stats_get(const sage2ov_ctx* c, sage2ov_index_stats* o) { if (!c || !o) return SAGE2OV_ERR_ARG; *o = c->istats; return SAGE2OV_OK; }
int sage2ov_index_lookup(sage2ov_ctx* c, const uint64_t key[2], uint64_t* entries, uint32_t cap, uint32_t* count) {
    if (!c || !key || !count) return SAGE2OV_ERR_ARG;
    if (!c->indexBuilt) return c->fail(SAGE2OV_ERR_ARG, "index not built");
    return dev_lookup(c->device(), key[0], key[1], entries, cap, count, c->err);
}

// P.hashTable (hashTable.cpp:256-273, :12-20): the text dump of the REFERENCE's own table -- one line per slot of its double-hashed table, in
// slot order -- which SAGE2 writes with -s or -M 2 and reads back with -m 3.  Our index has another shape, so the file
// is produced by replaying the reference's serial insertion (hashTable.cpp:94-109, :133-187) on the host: same table size (:243-254), same
// start slot (:233), same probe step (:140), same cap of 101 entries per bucket (:178), same flag for buckets of >= 100 entries (:111-123).
// Only the file needs this; look-ups never do (the placement is invisible in P.graph3).
namespace {
// The reference picks its table size from a literal list of 450 primes (hashTable.cpp:246).  The list follows a rule, which is what is
// implemented here instead of the list: k * 100000 < p prime, smallest, for k = 1..10; then the smallest SAFE prime (p and (p-1)/2 prime)
// above m * 65536 for m = mant * 2^e, mant = 17..31, e = 0, 1, 2, ... starting at m = 27.  (Checked against the reference's numbers when the
// golden fixtures were made: oracle/make_golden.py records the table size the reference printed; tests/test_hashtable_file.py.)
inline uint64_t mulmod64(uint64_t a, uint64_t b, uint64_t m) { return (uint64_t)((unsigned __int128)a * b % m); }
inline uint64_t powmod64(uint64_t a, uint64_t e, uint64_t m) { uint64_t r = 1; a %= m; while (e) { if (e & 1) r = mulmod64(r, a, m); a = mulmod64(a, a, m); e >>= 1; } return r; }
bool is_prime64(uint64_t n) {
    if (n < 2) return false;
    for (uint64_t p : {2ull, 3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull}) { if (n % p == 0) return n == p; }
    uint64_t d = n - 1; int r = 0; while ((d & 1) == 0) { d >>= 1; r++; }
    for (uint64_t a : {2ull, 3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull}) {          // deterministic for 64-bit n
        uint64_t x = powmod64(a, d, n); if (x == 1 || x == n - 1) continue;
        bool comp = true; for (int i = 1; i < r; i++) { x = mulmod64(x, x, n); if (x == n - 1) { comp = false; break; } }
        if (comp) return false;
    }
    return true;
}
// n-th table size of the reference (0-based), 0 beyond the list's 450 entries
uint64_t ref_table_size(int n) {
    if (n < 0 || n >= 450) return 0;
    if (n < 10) { uint64_t p = (uint64_t)(n + 1) * 100000; do p++; while (!is_prime64(p)); return p; }
    const int x = n - 10 + 10;                                       // position counted from mantissa 17 of exponent 0: the list starts at mantissa 27
    const int e = x / 15, mant = 17 + x % 15;
    uint64_t p = ((uint64_t)mant << e) * 65536ull;
    for (;;) { p++; if ((p & 3) == 3 && is_prime64(p) && is_prime64((p - 1) / 2)) return p; }
}
void ref_table_sizes(uint64_t value, uint64_t* next, uint64_t* prev) {      // findNextPrime / findPreviousPrime (hashTable.cpp:243-254, :303-314)
    uint64_t last = 0, before = 0;
    for (int n = 0; n < 450; n++) { before = last; last = ref_table_size(n); if (last > value || n == 449) break; }
    *next = last; *prev = before;                                    // (value <= 100003: the reference indexes [-1]; the caller refuses)
}
}  // namespace
int sage2ov_hashtable_save(sage2ov_ctx* c, const char* path) {
    if (!c || !path) return SAGE2OV_ERR_ARG;
    if (!c->organized) return c->fail(SAGE2OV_ERR_ARG, "organise (or load) the reads first");
    const uint64_t N = c->N; const int S = c->S; const int h = c->cfg.min_overlap > 64 ? 64 : (int)c->cfg.min_overlap;
    if (8 * N <= 100003) return c->fail(SAGE2OV_ERR_LIMIT, "P.hashTable: fewer than 12501 unique reads (the reference's own table-size look-up is undefined there, hashTable.cpp:309-313)");
    uint64_t M, Mprev; ref_table_sizes(8 * N, &M, &Mprev);
    if (M <= 8 * N) return c->fail(SAGE2OV_ERR_LIMIT, "P.hashTable: more reads than the reference's largest table holds");
    const uint64_t pre = ((0xFFFFFFFFFFFFFFFFull) % M + 1) % M;                        // hashTable.cpp:85
    // the four keys of a read (hashTable.cpp:96-104) as (v0, v1) of utils.cpp:171-187
    auto take = [](const uint64_t* w, int nw, int a, int n) -> uint64_t { return n <= 0 ? 0ull : (bits64_host(w, nw, 2 * a) >> (64 - 2 * n)); };
    auto key_of = [&](const uint64_t* w, int nw, int a, uint64_t& v0, uint64_t& v1) { if (h <= 32) { v0 = 0; v1 = take(w, nw, a, h); } else { v0 = take(w, nw, a, h - 32); v1 = take(w, nw, a + h - 32, 32); } };
    struct Slot { uint64_t v0, v1; int64_t head, tail; uint32_t count; };
    std::vector<Slot> slot(M + 1, Slot{0, 0, -1, -1, 0});                              // (index M is reachable: `while (p > M)`, hashTable.cpp:163)
    std::vector<uint64_t> entVal; std::vector<int64_t> entNext; entVal.reserve(4 * N); entNext.reserve(4 * N);
    for (uint64_t i = 1; i <= N; i++) {                                                // hashTable.cpp:94-109: serial, ids ascending, types 0..3
        const int L = c->len[i], nw = (L + 31) / 32; uint64_t f[34], r[34];
        for (int q = 0; q < nw; q++) f[q] = c->words[i * S + q];
        if (nw == S) f[nw - 1] &= ~SLOT_LEN_MASK;
        f[nw] = 0; revcomp_words(f, nw, L, r); r[nw] = 0;
        uint64_t kv[4][2];
        key_of(f, nw + 1, 0, kv[0][0], kv[0][1]); key_of(f, nw + 1, L - h, kv[1][0], kv[1][1]);
        key_of(r, nw + 1, 0, kv[2][0], kv[2][1]); key_of(r, nw + 1, L - h, kv[3][0], kv[3][1]);
        for (int t = 0; t < 4; t++) {
            const uint64_t v0 = kv[t][0], v1 = kv[t][1];
            const uint64_t probe = ((v1 % M) + (v0 % M) * pre) % M, inc = 1 + ((v0 + v1) % Mprev);   // :233, :140
            uint64_t pp = probe, miss = 0;
            while (slot[pp].head >= 0 && !(slot[pp].v1 == v1 && slot[pp].v0 == v0)) { miss++; pp = probe + miss * inc; while (pp > M) pp -= M; }
            Slot& sl = slot[pp];
            if (sl.head < 0 || sl.count <= HASH_THRESHOLD) {                           // :168-186: at most 101 entries
                const int64_t e = (int64_t)entVal.size(); entVal.push_back(i * 4 + (uint64_t)t); entNext.push_back(-1);
                if (sl.head < 0) { sl.head = e; sl.v0 = v0; sl.v1 = v1; } else entNext[sl.tail] = e;
                sl.tail = e; sl.count++;
            }
        }
    }
    FILE* fo = fopen(path, "w"); if (!fo) return c->fail(SAGE2OV_ERR_IO, std::string("cannot open ") + path);
    std::vector<char> io(1 << 22); setvbuf(fo, io.data(), _IOFBF, io.size());
    fprintf(fo, "%llu\n", (unsigned long long)M);
    const uint64_t longHash = N + 100;                                                 // :77, :111-123
    int rc = write_formatted(c, fo, M, 24, [&](uint64_t x, std::string& o) {            // hashTable.cpp:12-20 per slot + the "\n" of :268
        const Slot& sl = slot[x];
        if (sl.head < 0) { o.append("0\n"); return; }
        char buf[64]; char* q = put_u(buf, sl.count); *q++ = '\n'; o.append(buf, (size_t)(q - buf));
        bool first = true;
        for (int64_t e = sl.head; e >= 0; e = entNext[e]) {
            const uint64_t id = (first && sl.count >= HASH_THRESHOLD) ? longHash : (entVal[e] >> 2); first = false;
            q = put_u(buf, id); *q++ = '\t'; q = put_u(q, entVal[e] & 3); *q++ = '\t'; o.append(buf, (size_t)(q - buf));
        }
        o.push_back('\n');
    });
    fclose(fo); return rc;
}

// ------------------------------------------------------------------------------------------ step 3
int sage2ov_shard_range(const sage2ov_ctx* c, uint64_t* lo, uint64_t* hi) {
    if (!c || !lo || !hi) return SAGE2OV_ERR_ARG;
    const uint64_t N = c->N, w = c->cfg.world, r = c->cfg.rank;
    *lo = 1 + (N * r) / w; *hi = 1 + (N * (r + 1)) / w; return SAGE2OV_OK;
}
int sage2ov_shard_record_bytes(const sage2ov_ctx* c, uint64_t* b) { if (!c || !b) return SAGE2OV_ERR_ARG; *b = 16; return SAGE2OV_OK; }
int sage2ov_overlap_probe_shard(sage2ov_ctx* c) {
    if (!c) return SAGE2OV_ERR_ARG;
    if (!c->indexBuilt) return c->fail(SAGE2OV_ERR_ARG, "build the index first");
    uint64_t lo, hi; sage2ov_shard_range(c, &lo, &hi);
    int rc = dev_probe(c->device(), lo, hi, c->err); if (rc) return rc;
    c->probed = true; c->reciprocalDone = c->reduced = c->converted = false; return SAGE2OV_OK;
}
int sage2ov_shard_export_records(sage2ov_ctx* c, void* dst, uint64_t max_reads) {
    if (!c || !dst) return SAGE2OV_ERR_ARG; if (!c->probed) return c->fail(SAGE2OV_ERR_ARG, "probe first");
    uint64_t lo, hi; sage2ov_shard_range(c, &lo, &hi); if (hi - lo > max_reads) return c->fail(SAGE2OV_ERR_ARG, "destination too small");
    return dev_export_records(c->device(), dst, lo, hi, c->err);
}
int sage2ov_shard_import_records(sage2ov_ctx* c, const void* src, uint64_t first, uint64_t n) {
    if (!c || !src) return SAGE2OV_ERR_ARG; if (first < 1 || first + n > c->N + 1) return c->fail(SAGE2OV_ERR_ARG, "id range out of bounds");
    return dev_import_records(c->device(), src, first, n, c->err);
}
int sage2ov_overlap_reciprocal(sage2ov_ctx* c) {
    if (!c) return SAGE2OV_ERR_ARG; if (!c->probed) return c->fail(SAGE2OV_ERR_ARG, "probe first");
    uint64_t lo, hi; sage2ov_shard_range(c, &lo, &hi);
    uint64_t nov, cont, csize; int rc = dev_reciprocal(c->device(), lo, hi, &nov, &cont, &csize, c->err); if (rc) return rc;
    c->ostats = sage2ov_overlap_stats{}; c->ostats.verified_overlaps = nov; c->ostats.contained_extension = cont; c->ostats.contained_size = csize;
    c->ostats.left_to_explore = c->N - cont - csize;
    c->reciprocalDone = true; c->reduced = c->converted = false; return SAGE2OV_OK;
}
int sage2ov_shard_flags_bytes(const sage2ov_ctx* c, uint64_t* b) { if (!c || !b) return SAGE2OV_ERR_ARG; *b = 2 * (c->N + 1); return SAGE2OV_OK; }
int sage2ov_shard_export_flags(sage2ov_ctx* c, void* dst) { if (!c || !dst) return SAGE2OV_ERR_ARG; if (!c->probed) return c->fail(SAGE2OV_ERR_ARG, "probe first"); return dev_export_flags(c->device(), dst, c->err); }
int sage2ov_shard_import_flags(sage2ov_ctx* c, const void* src) { if (!c || !src) return SAGE2OV_ERR_ARG; if (!c->probed) return c->fail(SAGE2OV_ERR_ARG, "probe first"); return dev_import_flags(c->device(), src, c->err); }
int sage2ov_shard_edges_count(const sage2ov_ctx* c, uint64_t* n) { if (!c || !n || !c->reciprocalDone) return SAGE2OV_ERR_ARG; *n = dev_cand_count(c->device()); return SAGE2OV_OK; }
int sage2ov_shard_edges_export(sage2ov_ctx* c, void* dst, uint64_t cap) { if (!c || !dst) return SAGE2OV_ERR_ARG; if (!c->reciprocalDone) return c->fail(SAGE2OV_ERR_ARG, "reciprocal pass first"); return dev_export_cands(c->device(), dst, cap, c->err); }
int sage2ov_shard_edges_set(sage2ov_ctx* c, const void* src, uint64_t n) { if (!c || (!src && n)) return SAGE2OV_ERR_ARG; if (!c->reciprocalDone) return c->fail(SAGE2OV_ERR_ARG, "reciprocal pass first"); return dev_set_cands(c->device(), src, n, c->err); }
int sage2ov_overlap_initial(sage2ov_ctx* c) {
    if (!c) return SAGE2OV_ERR_ARG;
    if (c->cfg.world > 1) return c->fail(SAGE2OV_ERR_ARG, "multi-GPU contexts use probe_shard / export / import / reciprocal");
    int rc = sage2ov_overlap_probe_shard(c); if (rc) return rc;
    return sage2ov_overlap_reciprocal(c);
}

int sage2ov_overlap_reduce(sage2ov_ctx* c) {
    if (!c) return SAGE2OV_ERR_ARG; if (!c->reciprocalDone) return c->fail(SAGE2OV_ERR_ARG, "run the initial pass first");
    auto t0 = std::chrono::steady_clock::now();
    // Many unresolved reads and no long bucket: the order-independent form runs on the device; the serial
    // replay below stays the path for long-bucket indexes (A.7) and for a handful of reads.  Both are exact.
    {
        const char* ev = c->opt.get("SAGE2OV_DEVICE_REDUCE_MIN");
        const uint64_t minUn = ev ? strtoull(ev, nullptr, 10) : 4096;
        uint64_t nun0 = 0, nh0 = 0, ins = 0, rem = 0; int done = 0;
        const bool multi = c->cfg.world > 1;
        c->survBase = dev_cand_count(c->device()); c->survCount = 0; c->removedPartial = 0; c->survivorsExchanged = !multi;
        if (!c->opt.get("SAGE2OV_HOST_REDUCE")) {
            int rc0 = dev_reduce_device(c->device(), minUn, &nun0, &nh0, &ins, &rem, &done, c->err, c->cfg.rank, multi ? c->cfg.world : 1); if (rc0) return rc0;
        }
        for (uint64_t& v : c->rstats) v = 0;
        if (done) {
            dev_reduce_stats(c->device(), c->rstats);
            c->survCount = dev_cand_count(c->device()) - c->survBase; c->removedPartial = rem;
            c->ostats.unresolved_hits = nh0; c->ostats.edges_inserted = ins; c->ostats.transitive_removed = rem;
            c->reduce_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            c->reduced = true; c->converted = false; return SAGE2OV_OK;
        }
    }
    std::vector<Hit> hits; uint64_t nun = 0;
    const bool timing = c->opt.get("SAGE2OV_TIMING") != nullptr; auto tp = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) { if (!timing) return; auto t = std::chrono::steady_clock::now(); fprintf(stderr, "[reduce/host] %-28s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(t - tp).count()); tp = t; };
    std::vector<uint32_t> ids;
    int rc = dev_unresolved_hits(c->device(), hits, &nun, c->err, &ids); if (rc) return rc;
    lap("hit lists (device + download)");
    c->ostats.unresolved_hits = hits.size(); c->ostats.edges_inserted = 0; c->ostats.transitive_removed = 0;
    c->rstats[0] = nun ? 3 : 0; c->rstats[1] = nun;
    if (nun) {
        std::vector<EdgeCand> near; rc = dev_collect_reduce_edges(c->device(), ids, near, c->err); if (rc) return rc;
        lap("ids + nearby candidates");
        __gnu_parallel::sort(hits.begin(), hits.end(), [](const Hit& a, const Hit& b) { return a.from != b.from ? a.from < b.from : a.seq < b.seq; }, __gnu_parallel::default_parallel_tag(io_threads(c)));
        lap("sort hits");
        if (c->replayDense.size() != c->N + 2) c->replayDense.assign(c->N + 2, 0);
        Replay R(c->replayDense); R.c = c; R.hits = &hits;
        for (uint32_t i : ids) R.add(i);
        for (auto& e : near) { R.add(e.from); R.add(e.to); }
        for (auto& h : hits) R.add(h.to);                                              // (status-0 reads: already in, kept for safety)
        R.finish_setup();
        for (uint32_t i : ids) R.st[R.dense[i] - 1] = 0;
        for (uint64_t x = 0; x < hits.size();) { uint64_t y = x; while (y < hits.size() && hits[y].from == hits[x].from) y++; R.hitRange[R.dense[hits[x].from] - 1] = {x, y}; x = y; }
        for (auto& e : near) {                                                        // both directed entries of every stored edge
            R.adj[R.dense[e.from] - 1].push_back(AdjEdge{e.to, (uint8_t)e.type, 0, e.len});
            // e is the entry of list[from]; it was created either directly (u=from) or as the twin of (u=to): either way
            // list[to] holds the involutive twin, length L_from - (L_to - len)  (economyGraph.cpp:821)
            const int d2 = (int)c->len[e.from] - ((int)c->len[e.to] - (int)e.len);
            R.adj[R.dense[e.to] - 1].push_back(AdjEdge{e.from, (uint8_t)flip_type_host(e.type), 0, (uint32_t)d2 & 0xFFFFFu});
        }
        lap("replay set-up");
        R.timing = timing; R.run(ids);
        lap("replay (total)");
        c->ostats.edges_inserted = R.inserted; c->ostats.transitive_removed = R.removed; c->rstats[6] = R.removed;
        // surviving list entries of unresolved reads with to > from replace what the device dropped
        std::vector<EdgeCand> survivors;
        for (uint32_t i : ids) for (auto& e : R.adj[R.dense[i] - 1]) if (e.to > i) survivors.push_back(EdgeCand{i, e.to, e.len, e.type});
        // (multi-rank contexts: the replay is replicated -- every rank computes the same survivors; rank 0's are the ones that are exchanged)
        if (c->cfg.world > 1 && c->cfg.rank != 0) { survivors.clear(); c->removedPartial = 0; } else c->removedPartial = R.removed;
        rc = dev_append_edges(c->device(), survivors.data(), survivors.size(), c->err); if (rc) return rc;
        c->survCount = survivors.size();
        lap("survivors -> device");
    }
    c->reduce_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->reduced = true; c->converted = false; return SAGE2OV_OK;
}

int sage2ov_debug_table(sage2ov_ctx* c, uint64_t* out5) { if (!c || !out5 || !c->device() || !c->indexBuilt) return SAGE2OV_ERR_ARG; return dev_debug_table(c->device(), out5, c->err); }
int sage2ov_debug_meminfo(sage2ov_ctx* c, uint64_t* out4) { if (!c || !out4 || !c->device()) return SAGE2OV_ERR_ARG; return dev_meminfo(c->device(), out4, c->err); }
int sage2ov_debug_keys(sage2ov_ctx* c, uint64_t* out) { if (!c || !out || !c->device() || !c->organized) return SAGE2OV_ERR_ARG; return dev_debug_keys(c->device(), out, c->err); }
// diagnostic (tests/tools): every read's verified hits as 5 x u32 rows {from, to, type, len, seq}, sorted by (from, seq)
int sage2ov_debug_all_hits(sage2ov_ctx* c, uint32_t* out, uint64_t cap_rows, uint64_t* n_rows) {
    if (!c || !n_rows) return SAGE2OV_ERR_ARG; if (!c->reciprocalDone) return c->fail(SAGE2OV_ERR_ARG, "run the initial pass first");
    std::vector<Hit> hits; int rc = dev_debug_all_hits(c->device(), hits, c->err); if (rc) return rc;
    std::sort(hits.begin(), hits.end(), [](const Hit& a, const Hit& b) { return a.from != b.from ? a.from < b.from : a.seq < b.seq; });
    *n_rows = hits.size();
    if (out) { if (cap_rows < hits.size()) return c->fail(SAGE2OV_ERR_ARG, "buffer too small");
        for (size_t x = 0; x < hits.size(); x++) { out[5 * x] = hits[x].from; out[5 * x + 1] = hits[x].to; out[5 * x + 2] = hits[x].type; out[5 * x + 3] = (uint32_t)hits[x].len; out[5 * x + 4] = hits[x].seq; } }
    return SAGE2OV_OK;
}
// ---- sharded reduce phase: survivor buckets (multi-rank contexts)
int sage2ov_shard_survivors_count(const sage2ov_ctx* c, uint64_t* n, uint64_t* removed_partial) {
    if (!c || !n || !c->reduced) return SAGE2OV_ERR_ARG;
    *n = c->survCount; if (removed_partial) *removed_partial = c->removedPartial; return SAGE2OV_OK;
}
int sage2ov_shard_survivors_export(sage2ov_ctx* c, void* dst, uint64_t cap) {
    if (!c || (!dst && c->survCount)) return SAGE2OV_ERR_ARG; if (!c->reduced) return c->fail(SAGE2OV_ERR_ARG, "run the reduce phase first");
    if (c->survCount > cap) return c->fail(SAGE2OV_ERR_ARG, "destination too small");
    return dev_export_cand_range(c->device(), dst, c->survBase, c->survCount, c->err);
}
int sage2ov_shard_survivors_set(sage2ov_ctx* c, const void* src, uint64_t n_total, uint64_t removed_total) {
    if (!c || (!src && n_total)) return SAGE2OV_ERR_ARG; if (!c->reduced) return c->fail(SAGE2OV_ERR_ARG, "run the reduce phase first");
    int rc = dev_replace_cand_tail(c->device(), c->survBase, src, n_total, c->err); if (rc) return rc;
    c->survCount = n_total; c->removedPartial = removed_total; c->ostats.transitive_removed = removed_total; c->survivorsExchanged = true; c->converted = false;
    return SAGE2OV_OK;
}
int sage2ov_overlap_convert(sage2ov_ctx* c) {
    if (!c) return SAGE2OV_ERR_ARG; if (!c->reduced) return c->fail(SAGE2OV_ERR_ARG, "run the reduce phase first");
    if (!c->survivorsExchanged) return c->fail(SAGE2OV_ERR_ARG, "multi-rank context: exchange the survivor buckets of the reduce phase first (sage2ov_shard_survivors_*)");
    uint64_t nf = 0; int rc = dev_convert(c->device(), &nf, c->err); if (rc) return rc;
    c->ostats.edges = nf; c->edgesOnHost = false; c->converted = true;
    c->readmap_forget(); dev_readmap_release(c->device());                             // (the graph the table described is being replaced)
    return SAGE2OV_OK;
}
int sage2ov_overlap_stats_get(const sage2ov_ctx* c, sage2ov_overlap_stats* o) { if (!c || !o) return SAGE2OV_ERR_ARG; *o = c->ostats; return SAGE2OV_OK; }
int sage2ov_overlap_export_initial(sage2ov_ctx* c, uint64_t* r, uint64_t* l, uint8_t* st, uint32_t* cn) {
    if (!c) return SAGE2OV_ERR_ARG; if (!c->reciprocalDone) return c->fail(SAGE2OV_ERR_ARG, "run the initial pass first");
    return dev_download_initial(c->device(), r, l, st, cn, c->err);
}
static int fetch_edges(sage2ov_ctx* c) {
    if (!c->converted) return c->fail(SAGE2OV_ERR_ARG, "run convert first");
    if (c->edgesOnHost) return SAGE2OV_OK;
    int rc = dev_download_edges(c->device(), c->edges, c->err); if (rc) return rc;
    c->edgesOnHost = true; return SAGE2OV_OK;
}
int sage2ov_edges_count(const sage2ov_ctx* c, uint64_t* n) { if (!c || !n || !c->converted) return SAGE2OV_ERR_ARG; *n = c->ostats.edges; return SAGE2OV_OK; }
int sage2ov_edges_export(sage2ov_ctx* c, sage2ov_edge* out, uint64_t cap) {
    if (!c || !out) return SAGE2OV_ERR_ARG; int rc = fetch_edges(c); if (rc) return rc;
    if (cap < c->edges.size()) return c->fail(SAGE2OV_ERR_ARG, "edge buffer too small");
    for (size_t x = 0; x < c->edges.size(); x++) { const FinalEdge& e = c->edges[x]; sage2ov_edge o{}; o.from = e.from; o.to = e.to; o.length = e.len; o.length_twin = e.len_twin; o.type = (uint8_t)e.type; out[x] = o; }
    return SAGE2OV_OK;
}
// the counterpart of loadOverlapGraphFromFile for a graph of simple edges (overlapGraph.cpp:371-442): take the canonical edge list instead
// of computing it (`-m 4` on existing files; synthetic graphs in the step-4 tests).  Pairs keep the order given = the order they are pushed.
int sage2ov_edges_import(sage2ov_ctx* c, const sage2ov_edge* e, uint64_t n) {
    if (!c || (!e && n)) return SAGE2OV_ERR_ARG;
    if (!c->device()) return c->fail(SAGE2OV_ERR_DEVICE, "no GPU context");
    if (!c->organized) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_edges_import: the read set comes first (reads_organize / reads_load)");
    c->edges.resize(n);
    for (uint64_t x = 0; x < n; x++) {
        if (e[x].from == 0 || e[x].to == 0 || e[x].from > c->N || e[x].to > c->N || e[x].type > 3) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_edges_import: read id or edge type out of range");
        c->edges[x] = FinalEdge{(uint32_t)e[x].from, (uint32_t)e[x].to, e[x].length, e[x].length_twin, e[x].type};
    }
    int rc = dev_upload_edges(c->device(), c->edges, c->err); if (rc) return rc;
    c->ostats.edges = n; c->edgesOnHost = true; c->converted = true; c->g4Valid = false; c->readmap_forget(); if (Device* dd = c->device()) dev_readmap_release(dd);
    return SAGE2OV_OK;
}
// loadOverlapGraphFromFile (overlapGraph.cpp:371-442) for the graph step 3 writes: simple edges only (list size 0)
// P.graph3 as the writers produce it (overlapGraph.cpp:338-369, :12-20: three header lines, then per edge the record "from TAB to TAB type TAB 1 TAB length TAB 0 TAB 0",
// an empty line, the twin's record, an empty line), mapped and parsed by all I/O threads: a first pass over line-aligned chunks counts the record lines, which tells
// every chunk whether it starts at an edge or at a twin; the second parses edge + twin pairs (the owner of an edge reads its twin past the chunk's end).
// 1: edges filled.  0: not strictly that shape (the parser below then takes the file, with its own diagnostics).
static int graph_load_parallel(sage2ov_ctx* c, const char* path, std::vector<sage2ov_edge>& edges, unsigned long long& nr, unsigned long long& avg) {
    const int fd = ::open(path, O_RDONLY); if (fd < 0) return 0;
    struct stat sb; if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size < 8) { ::close(fd); return 0; }
    const size_t size = (size_t)sb.st_size;
    const char* m = (const char*)mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0); ::close(fd);
    if (m == MAP_FAILED) return 0;
    struct Unmap { const char* p; size_t n; ~Unmap() { munmap((void*)p, n); } } um{m, size};
    if (m[size - 1] != '\n') return 0;
    auto num = [&](size_t& p, size_t e, unsigned long long& v) -> bool { const size_t p0 = p; v = 0; while (p < e && m[p] >= '0' && m[p] <= '9' && p - p0 < 19) v = v * 10 + (unsigned long long)(m[p++] - '0'); return p > p0; };
    size_t h = 0; unsigned long long hd[3];
    for (int x = 0; x < 3; x++) { if (!num(h, size, hd[x]) || h >= size || m[h] != '\n') return 0; h++; }
    nr = hd[1]; avg = hd[2];
    // a record line + its empty line; v: from, to, type, 1, length, flow, list size.  Returns the position behind the empty line, 0 when the lines are not of that shape
    auto record = [&](size_t p, size_t e, unsigned long long* v) -> size_t {
        for (int x = 0; x < 7; x++) { if (!num(p, e, v[x]) || p >= e || m[p] != (x < 6 ? '\t' : '\n')) return 0; p++; }
        if (p >= e || m[p] != '\n') return 0;
        return p + 1;
    };
    const int nt = io_threads(c); const size_t nchunks = (size_t)nt * 4;
    std::vector<size_t> cut(nchunks + 1); cut[0] = h; cut[nchunks] = size;
    for (size_t x = 1; x < nchunks; x++) {            // cut behind an empty line (i.e. at the start of a record line)
        size_t p = std::max(cut[x - 1], h + (size - h) / nchunks * x);
        for (;;) { const char* nl = p < size ? (const char*)memchr(m + p, '\n', size - p) : nullptr; if (!nl || (size_t)(nl - m) + 1 >= size) { p = size; break; } p = (size_t)(nl - m) + 1; if (m[p] == '\n') { p++; break; } }
        cut[x] = std::max(p, cut[x - 1]);
    }
    std::vector<uint64_t> cnt(nchunks + 1, 0); bool bad = false;
    #pragma omp parallel for num_threads(nt) schedule(dynamic, 1)
    for (int64_t x = 0; x < (int64_t)nchunks; x++) {
        size_t p = cut[x]; const size_t e = cut[x + 1]; uint64_t n = 0; unsigned long long v[7];
        while (p < e) { p = record(p, e, v); if (!p || v[6] != 0) { bad = true; break; } n++; }      // (benign race: only ever set)
        cnt[x + 1] = n;
    }
    if (bad) return 0;
    for (size_t x = 0; x < nchunks; x++) cnt[x + 1] += cnt[x];
    if (cnt[nchunks] & 1) return 0;
    edges.resize(cnt[nchunks] / 2);
    #pragma omp parallel for num_threads(nt) schedule(dynamic, 1)
    for (int64_t x = 0; x < (int64_t)nchunks; x++) {
        size_t p = cut[x]; const size_t e = cut[x + 1]; uint64_t r = cnt[x]; unsigned long long a[7], b[7];
        if (p < e && (r & 1)) { p = record(p, size, a); r++; }                                       // a twin: its edge belongs to the chunk before
        while (p < e) {
            p = record(p, size, a); const size_t q = record(p, size, b);
            if (!q || a[0] != b[1] || a[1] != b[0]) { bad = true; break; }
            sage2ov_edge o{}; o.from = a[0]; o.to = a[1]; o.type = (uint8_t)a[2]; o.length = (uint32_t)a[4]; o.length_twin = (uint32_t)b[4];
            edges[r / 2] = o; r += 2; p = q;
        }
    }
    return bad ? 0 : 1;
}
int sage2ov_graph_load(sage2ov_ctx* c, const char* path) {
    if (!c || !path) return SAGE2OV_ERR_ARG;
    if (!c->opt.get("SAGE2OV_SEQUENTIAL_READER")) {
        std::vector<sage2ov_edge> pe; unsigned long long pnr = 0, pavg = 0;
        if (graph_load_parallel(c, path, pe, pnr, pavg) == 1) { c->goodReads = pnr; c->totalBP = pavg * pnr; return sage2ov_edges_import(c, pe.data(), pe.size()); }
    }
    FILE* f = fopen(path, "rb"); if (!f) return c->fail(SAGE2OV_ERR_IO, std::string("cannot open ") + path);
    std::string txt; { char buf[1 << 16]; size_t n; while ((n = fread(buf, 1, sizeof buf, f)) > 0) txt.append(buf, n); } fclose(f);
    const char* p = txt.c_str(); const char* end = p + txt.size();
    auto num = [&](unsigned long long& v) -> bool {
        while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) p++;
        if (p >= end || *p < '0' || *p > '9') return false;
        v = 0; while (p < end && *p >= '0' && *p <= '9') v = v * 10 + (unsigned long long)(*p++ - '0');
        if (p < end && *p == '.') { p++; while (p < end && *p >= '0' && *p <= '9') p++; }          // the flow column is a float ("0")
        return true;
    };
    unsigned long long gs, nr, avg;
    if (!num(gs) || !num(nr) || !num(avg)) return c->fail(SAGE2OV_ERR_IO, "bad .graph3 header");
    std::vector<sage2ov_edge> e;
    for (;;) {
        unsigned long long a[7], b[7];
        if (!num(a[0])) break;
        for (int x = 1; x < 7; x++) if (!num(a[x])) return c->fail(SAGE2OV_ERR_IO, "bad .graph3 record");
        for (int x = 0; x < 7; x++) if (!num(b[x])) return c->fail(SAGE2OV_ERR_IO, "bad .graph3 record (twin)");
        if (a[6] != 0 || b[6] != 0) return c->fail(SAGE2OV_ERR_LIMIT, "sage2ov_graph_load: composite edges (a graph already simplified) are not supported");
        if (a[0] != b[1] || a[1] != b[0]) return c->fail(SAGE2OV_ERR_IO, "bad .graph3: a record is not followed by its twin");
        sage2ov_edge o{}; o.from = a[0]; o.to = a[1]; o.type = (uint8_t)a[2]; o.length = (uint32_t)a[4]; o.length_twin = (uint32_t)b[4];
        e.push_back(o);
    }
    c->goodReads = nr; c->totalBP = avg * nr;
    return sage2ov_edges_import(c, e.data(), e.size());
}
int sage2ov_graph_save(sage2ov_ctx* c, const char* path) {                            // overlapGraph.cpp:338-369, :12-20
    if (!c || !path) return SAGE2OV_ERR_ARG; int rc = fetch_edges(c); if (rc) return rc;
    FILE* f = fopen(path, "w"); if (!f) return c->fail(SAGE2OV_ERR_IO, std::string("cannot open ") + path);
    std::vector<char> io(1 << 22); setvbuf(f, io.data(), _IOFBF, io.size());
    fprintf(f, "0\n%llu\n%llu\n", (unsigned long long)c->goodReads, (unsigned long long)(c->goodReads ? c->totalBP / c->goodReads : 0));
    auto rec = [](char* p, unsigned a, unsigned b, unsigned t, unsigned len) {           // "%u\t%u\t%u\t1\t%u\t0\t0\n\n"
        p = put_u(p, a); *p++ = '\t'; p = put_u(p, b); *p++ = '\t'; p = put_u(p, t); memcpy(p, "\t1\t", 3); p += 3; p = put_u(p, len); memcpy(p, "\t0\t0\n\n", 6); return p + 6;
    };
    rc = write_formatted(c, f, c->edges.size(), 96, [&](uint64_t x, std::string& o) {
        const FinalEdge& e = c->edges[x]; char buf[128];
        char* p = rec(buf, e.from, e.to, e.type, e.len);
        p = rec(p, e.to, e.from, (unsigned)flip_type_host((int)e.type), e.len_twin);
        o.append(buf, (size_t)(p - buf));
    });
    fclose(f); return rc;
}

// ---- step 4
namespace {
// the half-edges sage2ov_graph4_save writes a record pair for, in its order: per node, the alive half-edges with from <= to by ascending index (the writer
// walks each list from its tail, overlapGraph.cpp:356-358).  Both halves of a loop are among them: its pair is written twice
void g4_save_order(const SimplifiedGraph& g, std::vector<uint32_t>& order) {
    const uint64_t N = g.N, nh = g.n_half_edges;
    std::vector<uint32_t> offs(N + 2, 0);
    for (uint64_t h = 0; h < nh; h++) if (g.alive[h] && g.from[h] <= g.to[h]) offs[g.from[h] + 1]++;
    for (uint64_t i = 0; i <= N; i++) offs[i + 1] += offs[i];
    order.resize(offs[N + 1]);
    std::vector<uint32_t> cur(offs.begin(), offs.end() - 1); for (uint64_t h = 0; h < nh; h++) if (g.alive[h] && g.from[h] <= g.to[h]) order[cur[g.from[h]]++] = (uint32_t)h;
}
}  // namespace
int sage2ov_graph_simplify(sage2ov_ctx* c) {                                          // main.cpp:139-172
    if (!c) return SAGE2OV_ERR_ARG;
    if (!c->device()) return c->fail(SAGE2OV_ERR_DEVICE, "no GPU context: step 4 runs on the device only");
    if (!c->converted) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_graph_simplify: call sage2ov_overlap_convert first");
    c->g4Valid = false; c->g4 = SimplifiedGraph(); c->readmap_forget();
    int rc = dev_simplify(c->device(), c->g4, c->err); if (rc) return rc;
    c->g4Valid = true; c->g4Gen = c->readsGen; return SAGE2OV_OK;
}
int sage2ov_simplify_stats_get(const sage2ov_ctx* c, sage2ov_simplify_stats* o) {
    if (!c || !o || !c->g4Valid) return SAGE2OV_ERR_ARG;
    const SimplifiedGraph& g = c->g4; const uint64_t e = g.pairs_alive, r = g.reads_on_edges;
    o->nodes_contracted = g.contracted; o->removed = g.removed; o->loop_iterations = g.iterations; o->edges = e; o->reads_on_edges = r; o->device_ms = g.device_ms;
    return SAGE2OV_OK;
}
// saveOverlapGraphInFile of the resident graph: P.graph4 (line 1 and the flow column 0, line 2 the good reads) or, withFlows, P.graph5 (line 1 the genome size,
// line 2 `reads`, the flows as `ostream << float` prints them)
static int save_composite(sage2ov_ctx* c, const char* path, bool withFlows, unsigned long long genomeSize, unsigned long long reads) {
    HostLap lap(c, withFlows ? "graph5" : "graph4");
    { int rc = dev_simplify_download(c->device(), c->g4, c->err); if (rc) return rc; }
    lap("download of the simplified graph");
    const SimplifiedGraph& g = c->g4;
    std::vector<uint32_t> order; g4_save_order(g, order);
    FILE* f = fopen(path, "w"); if (!f) return c->fail(SAGE2OV_ERR_IO, std::string("cannot open ") + path);
    std::vector<char> io(1 << 22); setvbuf(f, io.data(), _IOFBF, io.size());
    fprintf(f, "%llu\n%llu\n%llu\n", genomeSize, reads, (unsigned long long)(c->goodReads ? c->totalBP / c->goodReads : 0));
    const float* flows = withFlows && !g.flow.empty() ? g.flow.data() : nullptr;
    // items: a header line, a block of up to 4096 list entries, or the blank line that ends a record -- a contracted chromosome is ONE
    // edge with millions of entries, so the unit of parallel formatting cannot be the edge
    struct Item { uint32_t h, first, count; };                                          // count == 0: header; first == ~0u: blank line
    std::vector<Item> items; items.reserve(order.size() * 4);
    for (uint32_t h0 : order)
        for (uint32_t h : {h0, h0 ^ 1u}) {
            items.push_back(Item{h, 0, 0});
            for (uint32_t x = 0; x < g.cnt[h]; x += 4096) items.push_back(Item{h, x, std::min<uint32_t>(4096, g.cnt[h] - x)});
            items.push_back(Item{h, ~0u, 1});
        }
    lap("edge order + items");
    int rc = write_formatted(c, f, items.size(), 64, [&](uint64_t x, std::string& o) {
        const Item it = items[x]; const uint32_t h = it.h; char buf[96]; char* p;
        if (it.first == ~0u) { o.push_back('\n'); return; }
        if (it.count == 0) {
            p = put_u(buf, g.from[h]); *p++ = '\t'; p = put_u(p, g.to[h]); *p++ = '\t'; p = put_u(p, g.type[h]); memcpy(p, "\t1\t", 3); p += 3;
            p = put_u(p, g.len[h]); *p++ = '\t';
            if (flows) p += snprintf(p, 32, "%g", (double)flows[h]); else *p++ = '0';
            *p++ = '\t'; p = put_u(p, g.cnt[h]); *p++ = '\n'; o.append(buf, (size_t)(p - buf));
            return;
        }
        for (uint32_t y = it.first; y < it.first + it.count; y++) {
            const uint64_t e = g.lists[(uint64_t)g.off[h] + y];
            p = put_u(buf, (unsigned long long)(e & ((1ull << 40) - 1))); *p++ = '\t'; *p++ = (char)('0' + ((e >> 40) & 1)); *p++ = '\t'; *p++ = (char)('0' + ((e >> 41) & 1)); *p++ = '\t';
            p = put_u(p, (unsigned)((e >> 42) & 0x7FF)); *p++ = '\t'; p = put_u(p, (unsigned)((e >> 53) & 0x7FF)); *p++ = '\n'; o.append(buf, (size_t)(p - buf));
        }
    });
    fclose(f); return rc;
}
int sage2ov_graph4_save(sage2ov_ctx* c, const char* path) {                           // overlapGraph.cpp:338-369, :12-20
    if (!c || !path) return SAGE2OV_ERR_ARG;
    if (!c->g4Valid) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_graph4_save: call sage2ov_graph_simplify first");
    return save_composite(c, path, false, 0, (unsigned long long)c->goodReads);
}

// ---- a graph with composite edges from a file (loadOverlapGraphFromFile, overlapGraph.cpp:371-443); the semantics are stated in sage2ov.h
int sage2ov_graph_load_composite(sage2ov_ctx* c, const char* path) {
    if (!c || !path) return SAGE2OV_ERR_ARG;
    if (!c->device()) return c->fail(SAGE2OV_ERR_DEVICE, c->gpu() && !c->devErr.empty() ? c->devErr : "no GPU context: the loaded graph lives on the device");
    if (!c->organized) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_graph_load_composite: organise (or load) the reads first");
    FILE* f = fopen(path, "rb"); if (!f) return c->fail(SAGE2OV_ERR_IO, std::string("cannot open ") + path);
    std::string txt; { char buf[1 << 16]; size_t n; while ((n = fread(buf, 1, sizeof buf, f)) > 0) txt.append(buf, n); } fclose(f);
    const char* p = txt.c_str(); const char* end = p + txt.size();
    auto skip = [&]() { while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) p++; };
    auto num = [&](unsigned long long& v) -> bool {
        skip(); if (p >= end || *p < '0' || *p > '9') return false;
        v = 0; while (p < end && *p >= '0' && *p <= '9') v = v * 10 + (unsigned long long)(*p++ - '0');
        return p >= end || *p == ' ' || *p == '\t' || *p == '\n' || *p == '\r';
    };
    float flowRead = 0;
    auto real = [&]() -> bool {                                                        // the flow column (a float: "0", "2", "1.5", "1e+06"), kept as the reference keeps it: a float
        skip(); if (p >= end) return false;
        char* e = nullptr; const double v = strtod(p, &e); if (e == p) return false; p = e; flowRead = (float)v; return true;
    };
    unsigned long long gs, nr, avg;
    if (!num(gs) || !num(nr) || !num(avg)) return c->fail(SAGE2OV_ERR_IO, "sage2ov_graph_load_composite: bad header");
    const uint64_t N = c->N;
    SimplifiedGraph g; g.N = N;
    // one record into the pools; 0 ok, 1 clean end of file (only where a record may start), else an error code
    auto record = [&](bool mayEnd) -> int {
        unsigned long long v[7];
        skip(); if (p >= end) return mayEnd ? 1 : c->fail(SAGE2OV_ERR_ARG, "sage2ov_graph_load_composite: a record without its twin (truncated file)");
        for (int x = 0; x < 7; x++) if (x == 5 ? !real() : !num(v[x])) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_graph_load_composite: truncated or malformed record");
        if (v[0] < 1 || v[0] > N || v[1] < 1 || v[1] > N) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_graph_load_composite: a node id is 0 or above the number of reads");
        if (v[2] > 3 || v[4] > 0xFFFFFFFFull || v[6] >= (1ull << 32)) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_graph_load_composite: edge type, length or list size out of range");
        if (g.lists.size() + v[6] >= (1ull << 32)) return c->fail(SAGE2OV_ERR_LIMIT, "sage2ov_graph_load_composite: more than 2^32 list entries");
        g.from.push_back((uint32_t)v[0]); g.to.push_back((uint32_t)v[1]); g.type.push_back((uint8_t)v[2]); g.len.push_back((uint32_t)v[4]);
        g.cnt.push_back((uint32_t)v[6]); g.off.push_back((uint32_t)g.lists.size()); g.alive.push_back(1); g.flow.push_back(flowRead);
        for (unsigned long long j = 0; j < v[6]; j++) {
            unsigned long long e[5];
            for (int x = 0; x < 5; x++) if (!num(e[x])) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_graph_load_composite: truncated or malformed read list");
            if (e[0] < 1 || e[0] > N) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_graph_load_composite: a read id on a list is 0 or above the number of reads");
            if (e[1] > 1 || e[2] > 1) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_graph_load_composite: orientation and flag are 0 or 1");
            if (e[3] > 0x7FF || e[4] > 0x7FF) return c->fail(SAGE2OV_ERR_LIMIT, "sage2ov_graph_load_composite: distPrevious / distNext above 2047 (the 11-bit field of a list entry)");
            g.lists.push_back(e[0] | (e[1] << 40) | (e[2] << 41) | (e[3] << 42) | (e[4] << 53));
        }
        return 0;
    };
    auto same = [&](size_t a, size_t b) {                                              // two half-edges with equal fields and equal lists
        return g.from[a] == g.from[b] && g.to[a] == g.to[b] && g.type[a] == g.type[b] && g.len[a] == g.len[b] && g.cnt[a] == g.cnt[b] &&
               std::equal(g.lists.begin() + g.off[a], g.lists.begin() + g.off[a] + g.cnt[a], g.lists.begin() + g.off[b]);
    };
    auto pop = [&]() { g.lists.resize(g.off.back()); g.from.pop_back(); g.to.pop_back(); g.type.pop_back(); g.len.pop_back(); g.cnt.pop_back(); g.off.pop_back(); g.alive.pop_back(); g.flow.pop_back(); };
    uint64_t reads = 0;
    for (;;) {
        int rc = record(true); if (rc == 1) break; if (rc) return rc;
        rc = record(false); if (rc) return rc;
        const size_t a = g.from.size() - 2, b = a + 1;
        if (g.from[a] != g.to[b] || g.to[a] != g.from[b]) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_graph_load_composite: a record is not followed by its twin");
        if (g.cnt[a] != g.cnt[b]) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_graph_load_composite: the twin's list has another length");
        for (uint32_t x = 0; x < g.cnt[a]; x++)
            if (((g.lists[(uint64_t)g.off[a] + x] ^ g.lists[(uint64_t)g.off[b] + g.cnt[a] - 1 - x]) & ((1ull << 40) - 1)) != 0)
                return c->fail(SAGE2OV_ERR_ARG, "sage2ov_graph_load_composite: the twin's list is not the forward list's read ids in reverse order");
        // a loop's pair directly after its mirror image: the second writing of one edge (see sage2ov.h)
        if (a >= 2 && g.from[a] == g.to[a] && g.from[a - 2] == g.to[a - 2] && g.alive[a - 2] == 1 && same(a, a - 1) && same(b, a - 2)) { pop(); pop(); g.alive[a - 2] = g.alive[a - 1] = 2; continue; }
        reads += g.cnt[a];
    }
    for (auto& x : g.alive) x = 1;                                                     // (2 marked a loop pair that has taken its mirror image: a third copy is a pair of its own)
    g.n_half_edges = g.from.size(); g.pairs_alive = g.n_half_edges / 2; g.reads_on_edges = reads; g.downloaded = g.fields = true;
    c->g4Valid = false; c->readmap_forget();
    { const int rc = dev_simplify_upload(c->device(), g, c->err); if (rc) return rc; }
    c->g4 = std::move(g); c->g4Valid = true; c->g4Gen = c->readsGen; c->converted = false;                     // (no edge list of step 3 stands behind this graph: graph_simplify is refused)
    c->goodReads = nr; c->totalBP = avg * nr;
    return SAGE2OV_OK;
}

// ---- MatePair::meanSdEstimation (matePair.cpp:244-569); the semantics are stated in sage2ov.h
namespace {
typedef unsigned __int128 u128;
// the rounds of meanSdEstimation (:265-291) over round(mu, count, sum, sq) = computeMeanSD's sums (:318-381) of the d < 4 * mu
extern "C++" { template <class F>
int estimate_rounds(F&& round, uint64_t averageReadLength, sage2ov_insert* o) {
    *o = sage2ov_insert{};
    int64_t mu = 5000, sd = 5000, rmu = 0, rsd = 0;
    for (int i = 0; i < SAGE2OV_INSERT_ROUNDS; i++) {
        uint64_t count = 0, sum = 0; u128 sq = 0;
        { const int rc = round(mu, count, sum, sq); if (rc) return rc; }
        o->considered[i] = count;
        if (count < 2) { o->valid = 0; o->final_round = 0; return SAGE2OV_OK; }        // (the reference divides by zero here)
        rmu = (int64_t)(sum / count);
        rsd = (int64_t)sqrtl((long double)sq / (long double)(count - 1));
        const bool fin = llabs(mu - rmu) <= rmu / 100 && llabs(sd - rsd) <= rsd / 100;
        mu = rmu; sd = rsd; o->mu[i] = rmu; o->sd[i] = rsd; o->rounds = (uint32_t)(i + 1);
        if (fin) { o->final_round = 1; break; }
    }
    o->valid = 1; o->mean = rmu + (int64_t)averageReadLength; o->deviation = rsd;
    o->lower = std::max<int64_t>(0, o->mean - 3 * o->deviation); o->upper = o->mean + 3 * o->deviation;
    return SAGE2OV_OK;
} }
uint64_t average_read_length(const sage2ov_ctx* c) { return c->goodReads ? c->totalBP / c->goodReads : 0; }
int readmap_check(sage2ov_ctx* c, const char* who) {
    if (!c->device()) return c->fail(SAGE2OV_ERR_DEVICE, c->gpu() && !c->devErr.empty() ? c->devErr : std::string(who) + ": no GPU context: the read-to-edge table is built on the device only");
    if (!c->g4Valid || c->g4Gen != c->readsGen) return c->fail(SAGE2OV_ERR_ARG, std::string(who) + ": call sage2ov_graph_simplify or sage2ov_graph_load_composite first (on the present read set)");
    return SAGE2OV_OK;
}
void readmap_stats_take(sage2ov_ctx* c, const ReadMapStats& s) {
    sage2ov_readmap_stats& o = c->rmstats;
    o.entries = s.entries; o.locations = s.locations; o.records = s.records; o.sort_passes = s.passes; o.route = SAGE2OV_MATE_ROUTE_DEVICE;
    o.scan_ms = s.scan_ms; o.records_ms = s.records_ms; o.sort_ms = s.sort_ms; o.reduce_ms = s.reduce_ms;
}
int readmap_build(sage2ov_ctx* c) {
    c->rmValid = false; if (!c->estimateHeld) c->estimated = false;
    c->rmstats = sage2ov_readmap_stats{}; c->supports_forget(); c->paths_forget(); c->links_forget();
    ReadMapStats s; const int rc = dev_readmap_build(c->device(), &s, c->err); if (rc) return rc;
    readmap_stats_take(c, s); c->rmValid = true; return SAGE2OV_OK;
}
// flags and distances of one library (kept on the device until the mate table changes)
int readmap_join(sage2ov_ctx* c, int lib) {
    if (!c->mateOnDevice[lib] && !c->mates[lib].key.empty()) { const int rc = mates_place(c, lib, true); if (rc) return rc; }
    ReadMapStats s; const int rc = dev_readmap_join(c->device(), lib, &s, c->err); if (rc) return rc;
    c->rmstats.join_ms += s.join_ms; c->rmstats.distances[lib] = dev_readmap_distance_count(c->device(), lib);
    return SAGE2OV_OK;
}
int readmap_ensure(sage2ov_ctx* c, const char* who) {
    { const int rc = readmap_check(c, who); if (rc) return rc; }
    return c->rmValid ? SAGE2OV_OK : readmap_build(c);
}
// the estimate for a sweep: made when there is none; after a merge (estimateHeld) it stands and only the table is rebuilt from the merged graph, with the mates
// placed as an estimate would place them
int estimate_ensure(sage2ov_ctx* c) {
    if (!c->estimated) return sage2ov_mates_estimate(c);
    if (c->rmValid) return SAGE2OV_OK;
    { const int rc = readmap_build(c); if (rc) return rc; }
    dev_readmap_drop_joins(c->device());
    for (int lib = 1; lib <= (int)c->mateLibraries && lib < 128; lib++) { const int rc = readmap_join(c, lib); if (rc) return rc; }
    return SAGE2OV_OK;
}
// internal pair -> ordinal of its record pair in sage2ov_graph4_save's order (a loop, written twice: the first time)
int pair_ordinals(sage2ov_ctx* c) {
    if (!c->pairOrdinal.empty()) return SAGE2OV_OK;
    { const int rc = dev_simplify_download(c->device(), c->g4, c->err, false); if (rc) return rc; }
    std::vector<uint32_t> order; g4_save_order(c->g4, order);
    c->pairOrdinal.assign(c->g4.n_half_edges / 2 + 1, ~0u);
    for (size_t x = 0; x < order.size(); x++) { uint32_t& o = c->pairOrdinal[order[x] >> 1]; if (o == ~0u) o = (uint32_t)x; }
    return SAGE2OV_OK;
}
}  // namespace
int sage2ov_insert_estimate(const uint32_t* d, uint64_t n, uint64_t averageReadLength, sage2ov_insert* out) {
    if (!out || (n && !d)) return SAGE2OV_ERR_ARG;
    return estimate_rounds([&](int64_t mu, uint64_t& count, uint64_t& sum, u128& sq) {
        const uint64_t thr = 4 * (uint64_t)mu;
        for (uint64_t i = 0; i < n; i++) if (d[i] < thr) { const int64_t df = mu - (int64_t)d[i]; sq += (u128)((__int128)df * df); count++; sum += d[i]; }
        return 0;
    }, averageReadLength, out);
}
int sage2ov_mates_map_reads(sage2ov_ctx* c) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = readmap_check(c, "sage2ov_mates_map_reads"); if (rc) return rc; }
    { const int rc = readmap_build(c); if (rc) return rc; }
    dev_readmap_drop_joins(c->device());
    for (int lib = 1; lib < 128; lib++) {
        if (!mates_entries(c, lib)) continue;
        const int rc = readmap_join(c, lib); if (rc) return rc;
        c->rmstats.mate_entries += dev_readmap_flag_count(c->device(), lib);
    }
    return SAGE2OV_OK;
}
int sage2ov_mates_read_edges_count(sage2ov_ctx* c, uint64_t* ne, uint64_t* nl) {
    if (!c || !ne || !nl) return SAGE2OV_ERR_ARG;
    { const int rc = readmap_ensure(c, "sage2ov_mates_read_edges_count"); if (rc) return rc; }
    dev_readmap_counts(c->device(), ne, nl); return SAGE2OV_OK;
}
int sage2ov_mates_read_edges_export(sage2ov_ctx* c, sage2ov_read_edge* out, uint64_t cap, int32_t* locations, uint64_t capLoc, uint64_t* offsets) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = readmap_ensure(c, "sage2ov_mates_read_edges_export"); if (rc) return rc; }
    uint64_t E = 0, R = 0; dev_readmap_counts(c->device(), &E, &R);
    if (cap < E || capLoc < R) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_mates_read_edges_export: a buffer holds fewer values than the table (sage2ov_mates_read_edges_count)");
    if ((E && !out) || (R && !locations)) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_mates_read_edges_export: null argument");
    { const int rc = pair_ordinals(c); if (rc) return rc; }
    std::vector<uint32_t> rd(E), pr(E), nf(E), nr(E), lo(E), off(c->N + 2); std::vector<int32_t> ls(R);
    { const int rc = dev_readmap_export(c->device(), rd.data(), pr.data(), nf.data(), nr.data(), lo.data(), ls.data(), off.data(), c->err); if (rc) return rc; }
    const SimplifiedGraph& g = c->g4; const std::vector<uint32_t>& ord = c->pairOrdinal;
    // per read: its entries by the ordinal of the pair (the device orders them by the pair's index in the pool); the read's locations keep their stretch
    #pragma omp parallel for num_threads(io_threads(c)) schedule(dynamic, 4096)
    for (uint64_t a = 0; a <= c->N; a++) {
        const uint32_t e0 = off[a], e1 = off[a + 1]; if (e0 == e1) continue;
        uint32_t idx[8]; std::vector<uint32_t> big; uint32_t* ix = idx;
        if (e1 - e0 > 8) { big.resize(e1 - e0); ix = big.data(); }
        for (uint32_t x = 0; x < e1 - e0; x++) ix[x] = e0 + x;
        std::sort(ix, ix + (e1 - e0), [&](uint32_t x, uint32_t y) { return ord[pr[x]] < ord[pr[y]]; });
        uint32_t at = lo[e0];
        for (uint32_t x = 0; x < e1 - e0; x++) {
            const uint32_t e = ix[x], p = pr[e], h0 = 2 * p, h1 = 2 * p + 1;
            const uint32_t hE = g.from[h0] < g.to[h0] ? h0 : (g.from[h0] > g.to[h0] ? h1 : h1);
            sage2ov_read_edge r{}; r.read = rd[e]; r.pair = ord[p]; r.from = g.from[hE]; r.to = g.to[hE]; r.type = g.type[hE]; r.n_forward = nf[e]; r.n_reverse = nr[e]; r.location = at;
            out[e0 + x] = r;
            memcpy(locations + at, ls.data() + lo[e], (size_t)(nf[e] + nr[e]) * sizeof(int32_t)); at += nf[e] + nr[e];
        }
    }
    if (offsets) for (uint64_t a = 0; a <= c->N + 1; a++) offsets[a] = off[a];
    return SAGE2OV_OK;
}
int sage2ov_mates_flags_export(sage2ov_ctx* c, int library, uint8_t* flags) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = mates_check(c, "sage2ov_mates_flags_export", library); if (rc) return rc; }
    { const int rc = readmap_ensure(c, "sage2ov_mates_flags_export"); if (rc) return rc; }
    { const int rc = readmap_join(c, library); if (rc) return rc; }
    if (dev_readmap_flag_count(c->device(), library) && !flags) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_mates_flags_export: null argument");
    return dev_readmap_flags(c->device(), library, flags, c->err);
}
int sage2ov_mates_distances_export(sage2ov_ctx* c, int library, uint32_t* d, uint64_t cap, uint64_t* n) {
    if (!c || !n) return SAGE2OV_ERR_ARG;
    { const int rc = mates_check(c, "sage2ov_mates_distances_export", library); if (rc) return rc; }
    { const int rc = readmap_ensure(c, "sage2ov_mates_distances_export"); if (rc) return rc; }
    { const int rc = readmap_join(c, library); if (rc) return rc; }
    const uint64_t nd = dev_readmap_distance_count(c->device(), library); *n = nd;
    if (!d) return SAGE2OV_OK;
    if (cap < nd) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_mates_distances_export: the buffer holds fewer values than there are distances");
    { const int rc = pair_ordinals(c); if (rc) return rc; }
    std::vector<uint32_t> dist(nd), ent(nd), pr(nd);
    { const int rc = dev_readmap_distances(c->device(), library, dist.data(), ent.data(), pr.data(), c->err); if (rc) return rc; }
    const std::vector<uint32_t>& ord = c->pairOrdinal;
    for (uint64_t i = 0; i < nd;) {                                                    // a mate entry with several distances (rare): by the pair's ordinal
        uint64_t e = i + 1; while (e < nd && ent[e] == ent[i]) e++;
        if (e - i > 1) {
            std::vector<std::pair<uint32_t, uint32_t>> run; for (uint64_t x = i; x < e; x++) run.emplace_back(ord[pr[x]], dist[x]);
            std::sort(run.begin(), run.end()); for (uint64_t x = i; x < e; x++) dist[x] = run[x - i].second;
        }
        i = e;
    }
    if (nd) memcpy(d, dist.data(), nd * sizeof(uint32_t));
    return SAGE2OV_OK;
}
int sage2ov_mates_estimate(sage2ov_ctx* c) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = readmap_ensure(c, "sage2ov_mates_estimate"); if (rc) return rc; }
    c->estimated = c->estimateHeld = false; c->rmstats.rounds = 0; c->rmstats.round_ms = 0; c->supports_forget(); c->paths_forget(); c->links_forget();
    const uint64_t arl = average_read_length(c); Device* d = c->device();
    c->minUpper = 1000000; c->maxUpper = 0;                                            // matePair.cpp:292-293
    for (auto& I : c->inserts) I = sage2ov_insert{};
    for (int lib = 1; lib <= (int)c->mateLibraries; lib++) {
        { const int rc = readmap_join(c, lib); if (rc) return rc; }
        { const int rc = dev_estflags_keep(d, lib, c->err); if (rc) return rc; }         // the flags of this graph: what the path supports read after merges (sage2ov.h, ESTIMATE FLAGS)
        ReadMapStats s; sage2ov_insert& I = c->inserts[lib];
        const int rc = estimate_rounds([&](int64_t mu, uint64_t& count, uint64_t& sum, u128& sq) {
            uint64_t o[4]; const int r = dev_readmap_round(d, lib, mu, 4 * (uint64_t)mu, o, &s, c->err);
            count = o[0]; sum = o[1]; sq = ((u128)o[3] << 64) | o[2]; return r;
        }, arl, &I);
        if (rc) return rc;
        I.library = (uint32_t)lib; c->rmstats.rounds += s.rounds; c->rmstats.round_ms += s.round_ms;
        if (!I.valid) continue;                                                        // (left out of the bounds: see sage2ov.h)
        if (c->minUpper >= (uint64_t)I.upper) c->minUpper = (uint64_t)I.upper;
        if (c->maxUpper <= (uint64_t)I.upper) c->maxUpper = (uint64_t)I.upper;
    }
    c->maxUpper *= 3 * ((arl + 99) / 100);                                             // 3 * ceil(averageReadLength / 100.0), :308
    c->estimated = true;
    return SAGE2OV_OK;
}
int sage2ov_mates_insert_get(const sage2ov_ctx* c, int library, sage2ov_insert* out) {
    if (!c || !out || library < 1 || library > 127 || !c->estimated) return SAGE2OV_ERR_ARG;
    *out = c->inserts[library]; return SAGE2OV_OK;
}
int sage2ov_mates_bounds_get(const sage2ov_ctx* c, uint64_t* mn, uint64_t* mx) {
    if (!c || !mn || !mx || !c->estimated) return SAGE2OV_ERR_ARG;
    *mn = c->minUpper; *mx = c->maxUpper; return SAGE2OV_OK;
}
int sage2ov_readmap_stats_get(const sage2ov_ctx* c, sage2ov_readmap_stats* o) { if (!c || !o) return SAGE2OV_ERR_ARG; *o = c->rmstats; return SAGE2OV_OK; }

// ---- the flows of the resident graph and the sweep of ContigExtender::findMatepairSupports (mergeContigs.cpp:959-1110); the semantics are stated in sage2ov.h
namespace {
static_assert(sizeof(sage2ov_support) == 24, "sage2ov_support is six uint32_t");
// the half-edges that open a record pair in sage2ov_graph4_save's order, a loop at its first writing only
int flow_order(sage2ov_ctx* c, std::vector<uint32_t>& first) {
    { const int rc = dev_simplify_download(c->device(), c->g4, c->err, false); if (rc) return rc; }
    std::vector<uint32_t> order; g4_save_order(c->g4, order);
    std::vector<uint8_t> seen(c->g4.n_half_edges / 2 + 1, 0); first.clear();
    for (uint32_t h : order) if (!seen[h >> 1]) { seen[h >> 1] = 1; first.push_back(h); }
    return SAGE2OV_OK;
}
int supports_ensure(sage2ov_ctx* c, const char* who) {
    { const int rc = readmap_check(c, who); if (rc) return rc; }
    if (c->supValid && c->estimated && c->rmValid) return SAGE2OV_OK;
    return sage2ov_mates_supports(c);
}
// the table in export order, on the host (once per table)
int supports_fetch(sage2ov_ctx* c) {
    if (c->supOnHost) return SAGE2OV_OK;
    Device* d = c->device(); const uint64_t E = dev_support_count(d);
    std::vector<uint64_t> key(E); std::vector<uint32_t> sup(E);
    { const int rc = dev_support_export(d, key.data(), sup.data(), c->err); if (rc) return rc; }
    { const int rc = pair_ordinals(c); if (rc) return rc; }
    const SimplifiedGraph& g = c->g4; const std::vector<uint32_t>& ord = c->pairOrdinal;
    c->supports.resize(E);
    for (uint64_t e = 0; e < E; e++) {
        const uint32_t a = (uint32_t)(key[e] >> 32), b = (uint32_t)key[e];
        sage2ov_support o{}; o.node = g.from[a]; o.pair_in = ord[a >> 1]; o.pair_out = ord[b >> 1]; o.to_in = g.to[a]; o.to_out = g.to[b]; o.support = sup[e];
        c->supports[e] = o;
    }
    std::sort(c->supports.begin(), c->supports.end(), [](const sage2ov_support& x, const sage2ov_support& y) {
        return x.node != y.node ? x.node < y.node : (x.pair_in != y.pair_in ? x.pair_in < y.pair_in : x.pair_out < y.pair_out); });
    c->supOnHost = true;
    return SAGE2OV_OK;
}
}  // namespace
int sage2ov_graph_flow_export(sage2ov_ctx* c, float* flow, uint64_t cap) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = readmap_check(c, "sage2ov_graph_flow_export"); if (rc) return rc; }
    std::vector<uint32_t> first; { const int rc = flow_order(c, first); if (rc) return rc; }
    if (cap < 2 * first.size()) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_graph_flow_export: the buffer holds fewer than two values per record pair");
    if (!first.empty() && !flow) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_graph_flow_export: null argument");
    const std::vector<float>& f = c->g4.flow;
    for (size_t x = 0; x < first.size(); x++) { flow[2 * x] = f.empty() ? 0.f : f[first[x]]; flow[2 * x + 1] = f.empty() ? 0.f : f[first[x] ^ 1u]; }
    return SAGE2OV_OK;
}
int sage2ov_graph_flow_import(sage2ov_ctx* c, const float* flow, uint64_t n) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = readmap_check(c, "sage2ov_graph_flow_import"); if (rc) return rc; }
    std::vector<uint32_t> first; { const int rc = flow_order(c, first); if (rc) return rc; }
    if (n != 2 * first.size()) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_graph_flow_import: two values per record pair, in sage2ov_graph4_save's order");
    if (n && !flow) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_graph_flow_import: null argument");
    std::vector<float> f(c->g4.n_half_edges, 0.f);
    for (size_t x = 0; x < first.size(); x++) { f[first[x]] = flow[2 * x]; f[first[x] ^ 1u] = flow[2 * x + 1]; }
    c->supports_forget(); c->paths_forget(); c->contigs_forget();
    { const int rc = dev_flow_set(c->device(), f.data(), f.size(), c->err); if (rc) return rc; }
    c->g4.flow = std::move(f);
    return SAGE2OV_OK;
}
// ---- step 5 around its solver (copycountEstimator.cpp:29-417); the semantics are stated in sage2ov.h
namespace {
static_assert(sizeof(sage2ov_flow_arc) == 20 && sizeof(sage2ov_flow_arc) == sizeof(FlowArc), "sage2ov_flow_arc is five 32-bit words");
// (uint64_t)x as the reference's build leaves it, with the named rule for a float that does not fit
inline uint64_t float_to_u64(float x, uint32_t* degenerate) {
    if (!(x >= 0.0f) || !(x < 18446744073709551616.0f)) { *degenerate = 1; return 1ull << 63; }
    *degenerate = 0; return (uint64_t)x;
}
// :83, :145: every operation in float
inline float a_statistic(uint64_t delta, uint64_t k, float ratio, float lg) {
    const float t1 = (float)delta * ratio;
    const float t2 = (float)k * lg;
    return t1 - t2;
}
// genomeSizeEstimation (:29-54) over sums(first, ratio, l2, out) = findGenomeSize's deltaSum and kSum (:59-97)
extern "C++" { template <class F>
int genome_rounds(F&& sums, uint64_t n, sage2ov_genome_estimate* o) {
    *o = sage2ov_genome_estimate{};
    const float l2 = std::log((float)2);
    uint64_t previous = 0, current = 0;
    for (int i = 0; i < SAGE2OV_GENOME_ROUNDS; i++) {
        uint64_t ds[2] = {0, 0};
        const float ratio = previous ? (float)n / (float)previous : 0.0f;
        { const int rc = sums(previous == 0, ratio, l2, ds); if (rc) return rc; }
        const float q = (float)n / (float)ds[1];
        const float x = q * (float)ds[0];                                              // :98
        current = float_to_u64(x, &o->degenerate);
        o->estimate[i] = current; o->delta_sum[i] = ds[0]; o->k_sum[i] = ds[1]; o->rounds = (uint32_t)(i + 1);
        if (current == previous) { o->agreed = 1; break; }
        previous = current;
    }
    o->genome_size = current;
    return SAGE2OV_OK;
} }
int copycount_check(sage2ov_ctx* c, const char* who) { return readmap_check(c, who); }
void copycount_times(sage2ov_ctx* c, const CopyCountStats& s) {
    sage2ov_copycount_stats& o = c->ccstats;
    o.prepare_ms += s.k_ms; o.rounds_ms += s.round_ms; o.order_ms += s.order_ms; o.classes_ms += s.classes_ms; o.arcs_ms += s.arcs_ms; o.apply_ms += s.apply_ms;
}
int genome_estimate(sage2ov_ctx* c) {
    c->copycount_forget();
    CopyCountStats s;
    { const int rc = dev_copycount_prepare(c->device(), c->freq.data(), &s, c->err); if (rc) return rc; }
    sage2ov_genome_estimate e;
    const int rc = genome_rounds([&](bool first, float ratio, float l2, uint64_t* out) { return dev_copycount_round(c->device(), first ? 1 : 0, ratio, l2, out, &s, c->err); }, s.present, &e);
    if (rc) return rc;
    sage2ov_copycount_stats& o = c->ccstats;
    o.genome_size = e.genome_size; for (int i = 0; i < SAGE2OV_GENOME_ROUNDS; i++) o.estimate[i] = e.estimate[i];
    o.rounds = e.rounds; o.degenerate = e.degenerate; o.agreed = e.agreed; o.reads_present = s.present;
    copycount_times(c, s);
    c->gsValid = true;
    return SAGE2OV_OK;
}
int network_ensure(sage2ov_ctx* c, const char* who) {
    { const int rc = copycount_check(c, who); if (rc) return rc; }
    return c->netValid ? SAGE2OV_OK : sage2ov_flow_network_build(c);
}
}  // namespace
int sage2ov_genome_size_rounds(const uint32_t* length, const uint64_t* k, uint64_t pairs, uint64_t reads, sage2ov_genome_estimate* out) {
    if (!out || (pairs && (!length || !k))) return SAGE2OV_ERR_ARG;
    return genome_rounds([&](bool first, float ratio, float l2, uint64_t* o) {
        uint64_t ds = 0, ks = 0;
        for (uint64_t i = 0; i < pairs; i++) {
            const uint64_t delta = (uint32_t)(length[i] - 1u);
            const bool ok = first ? length[i] > 500 : (a_statistic(delta, k[i], ratio, l2) >= 3.0f && delta >= 1000);
            if (ok) { ds += delta; ks += k[i]; }
        }
        o[0] = ds; o[1] = ks; return 0;
    }, reads, out);
}
int sage2ov_genome_size_estimate(sage2ov_ctx* c, uint64_t* genome_size) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = copycount_check(c, "sage2ov_genome_size_estimate"); if (rc) return rc; }
    if (!c->gsValid) { const int rc = genome_estimate(c); if (rc) return rc; }
    if (genome_size) *genome_size = c->ccstats.genome_size;
    return SAGE2OV_OK;
}
int sage2ov_flow_network_build(sage2ov_ctx* c) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = copycount_check(c, "sage2ov_flow_network_build"); if (rc) return rc; }
    if (!c->gsValid) { const int rc = genome_estimate(c); if (rc) return rc; }
    c->netValid = false;
    const uint64_t n = c->ccstats.reads_present, N = c->ccstats.genome_size;
    CopyCountConst P;                                                                  // every log as the reference spells it (:145, :329-331)
    P.ratio = (float)n / (float)N;
    P.lj[0] = 0; for (int j = 1; j <= 20; j++) P.lj[j] = std::log((float)((float)(j + 1) / (float)j));
    const int first_UB = 3, second_UB = 5, third_UB = 1000;
    P.l1 = std::log((float)(1)); P.l3 = std::log((float)(first_UB)); P.l5 = std::log((float)(second_UB)); P.l1000 = std::log((float)(third_UB));
    P.fN1 = std::log((float)(N - 1)); P.fN3 = std::log((float)(N - first_UB)); P.fN5 = std::log((float)(N - second_UB));
    P.dN3 = std::log(N - first_UB); P.dN1000 = std::log(N - third_UB);
    P.n = n;
    CopyCountStats s;
    { const int rc = dev_flownet_build(c->device(), P, &s, c->err); if (rc) return rc; }
    sage2ov_copycount_stats& o = c->ccstats;
    o.nodes = s.nodes; o.edges = s.edges; o.simple = s.simple; o.once = s.once; o.many = s.many; o.network_nodes = 4 * s.nodes + 2; o.network_arcs = s.arcs;
    copycount_times(c, s);
    c->netValid = true;
    return SAGE2OV_OK;
}
int sage2ov_flow_network_count(sage2ov_ctx* c, uint64_t* nodes, uint64_t* arcs) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = network_ensure(c, "sage2ov_flow_network_count"); if (rc) return rc; }
    if (nodes) *nodes = c->ccstats.network_nodes;
    if (arcs) *arcs = c->ccstats.network_arcs;
    return SAGE2OV_OK;
}
int sage2ov_flow_network_export(sage2ov_ctx* c, sage2ov_flow_arc* out, uint64_t cap) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = network_ensure(c, "sage2ov_flow_network_export"); if (rc) return rc; }
    if (cap < c->ccstats.network_arcs) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_flow_network_export: the buffer holds fewer arcs than the network has");
    if (!out) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_flow_network_export: null argument");
    return dev_flownet_export(c->device(), (FlowArc*)out, c->err);
}
int sage2ov_flow_network_save(sage2ov_ctx* c, const char* path) {                      // :185-356
    if (!c || !path) return SAGE2OV_ERR_ARG;
    { const int rc = network_ensure(c, "sage2ov_flow_network_save"); if (rc) return rc; }
    std::vector<FlowArc> arcs(c->ccstats.network_arcs);
    { const int rc = dev_flownet_export(c->device(), arcs.data(), c->err); if (rc) return rc; }
    FILE* f = fopen(path, "w"); if (!f) return c->fail(SAGE2OV_ERR_IO, std::string("cannot open ") + path);
    std::vector<char> io(1 << 22); setvbuf(f, io.data(), _IOFBF, io.size());
    const unsigned long long nn = c->ccstats.network_nodes;
    fprintf(f, "p min %llu %llu\nn 1 0\nn 2 0\na 2 1 1 %llu 0\n", nn, (unsigned long long)arcs.size(), nn * 100ull);
    const int rc = write_formatted(c, f, arcs.size() - 1, 40, [&](uint64_t x, std::string& o) {
        const FlowArc& a = arcs[x + 1]; char buf[128]; char* p = buf;
        *p++ = 'a'; *p++ = ' '; p = put_u(p, a.from); *p++ = ' '; p = put_u(p, a.to); *p++ = ' ';
        p += snprintf(p, 64, "%d %d %f\n", a.lower, a.upper, (double)a.cost);          // (`ostream << std::fixed << float`: six decimals of the float's value)
        o.append(buf, (size_t)(p - buf));
    });
    fclose(f); return rc;
}
int sage2ov_flow_solution_apply(sage2ov_ctx* c, const uint64_t* from, const uint64_t* to, const uint64_t* flow, uint64_t n) {      // :365-403
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = network_ensure(c, "sage2ov_flow_solution_apply"); if (rc) return rc; }
    if (n && (!from || !to || !flow)) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_flow_solution_apply: null argument");
    if (n >= (1ull << 32) - 2048) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_flow_solution_apply: more lines than a network can have arcs");
    const uint64_t nn = c->ccstats.network_nodes; uint64_t tts = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (from[i] < 1 || from[i] > nn || to[i] < 1 || to[i] > nn) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_flow_solution_apply: a node number outside the network");
        if ((from[i] == 1 && to[i] == 2) || (from[i] == 2 && to[i] == 1)) tts = flow[i];
    }
    CopyCountStats s;
    c->supports_forget(); c->paths_forget(); c->contigs_forget();
    { const int rc = dev_flow_apply(c->device(), from, to, flow, n, &s, c->err); if (rc) return rc; }
    std::vector<float> f(c->g4.n_half_edges, 0.f);
    { const int rc = dev_flow_get(c->device(), f.data(), f.size(), c->err); if (rc) return rc; }
    c->g4.flow = std::move(f);
    sage2ov_copycount_stats& o = c->ccstats;
    o.t_to_s_flow = tts; o.flow_different = s.different; o.solution_lines = n; o.lines_applied = s.applied;
    copycount_times(c, s);
    return SAGE2OV_OK;
}
int sage2ov_flow_solution_load(sage2ov_ctx* c, const char* path) {
    if (!c || !path) return SAGE2OV_ERR_ARG;
    { const int rc = network_ensure(c, "sage2ov_flow_solution_load"); if (rc) return rc; }
    FILE* f = fopen(path, "rb"); if (!f) return c->fail(SAGE2OV_ERR_IO, std::string("cannot open ") + path);
    std::string txt; { char buf[1 << 16]; size_t n; while ((n = fread(buf, 1, sizeof buf, f)) > 0) txt.append(buf, n); } fclose(f);
    std::vector<uint64_t> v[3]; const char* p = txt.c_str(); const char* end = p + txt.size(); int col = 0;
    for (;;) {
        while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) p++;
        if (p >= end) break;
        if (*p < '0' || *p > '9') return c->fail(SAGE2OV_ERR_IO, "sage2ov_flow_solution_load: not a number");
        uint64_t x = 0; while (p < end && *p >= '0' && *p <= '9') x = x * 10 + (uint64_t)(*p++ - '0');
        v[col].push_back(x); col = (col + 1) % 3;
    }
    if (col != 0) return c->fail(SAGE2OV_ERR_IO, "sage2ov_flow_solution_load: a line is not `from to flow`");
    return sage2ov_flow_solution_apply(c, v[0].data(), v[1].data(), v[2].data(), v[0].size());
}
int sage2ov_graph5_save(sage2ov_ctx* c, const char* path) {                            // overlapGraph.cpp:338-369
    if (!c || !path) return SAGE2OV_ERR_ARG;
    { const int rc = copycount_check(c, "sage2ov_graph5_save"); if (rc) return rc; }
    if (!c->gsValid) { const int rc = genome_estimate(c); if (rc) return rc; }
    return save_composite(c, path, true, (unsigned long long)c->ccstats.genome_size, (unsigned long long)c->ccstats.reads_present);
}
int sage2ov_copycount_stats_get(const sage2ov_ctx* c, sage2ov_copycount_stats* o) { if (!c || !o) return SAGE2OV_ERR_ARG; *o = c->ccstats; return SAGE2OV_OK; }
// ---- step 5's solver (main_cs2, :359)
namespace {
void mcf_stats_set(sage2ov_ctx* c, const McfStats& s) {
    sage2ov_mcf_stats o{};
    o.nodes = s.nodes; o.arcs = s.arcs; o.scale = s.scale; o.phases = s.phases; o.rounds = s.rounds; o.pushes = s.pushes; o.relabels = s.relabels; o.price_updates = s.updates;
    o.form = s.form; o.price_words = s.priceWords; o.build_ms = s.build_ms; o.solve_ms = s.solve_ms;
    for (int i = 0; i < SAGE2OV_MCF_PHASES; i++) { o.refine_rounds[i] = s.refine_rounds[i]; o.refine_ms[i] = s.refine_ms[i]; }
    c->mcfstats = o;
    for (int i = 0; i < 6; i++) c->mcfhub[i] = s.hub[i];
}
// sum of flow * cost; false when it leaves int64
extern "C++" { template <class Cost>
bool mcf_total_cost(const int64_t* flow, uint64_t m, Cost&& cost, int64_t* out) {
    __int128 t = 0;
    for (uint64_t i = 0; i < m; i++) t += (__int128)flow[i] * (__int128)cost(i);
    if (t > (__int128)INT64_MAX || t < (__int128)INT64_MIN) return false;
    *out = (int64_t)t; return true;
} }
// the cost the solver sees of a record's float: truncation towards zero (k_mf_from_cc)
int64_t mcf_trunc(float c) { return (int64_t)c; }
}  // namespace
int sage2ov_mcf_solve(sage2ov_ctx* c, uint64_t n, const sage2ov_mcf_arc* arcs, uint64_t m, uint64_t max_rounds, int64_t* flow, int64_t* price, sage2ov_mcf_stats* stats) {
    if (!c) return SAGE2OV_ERR_ARG;
    if (m && (!arcs || !flow)) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_mcf_solve: null argument");
    if (!c->device()) return c->fail(SAGE2OV_ERR_DEVICE, c->gpu() ? c->devErr : "sage2ov_mcf_solve: this context has no GPU");
    if (n >= 0xFFFFFFF0ull) return c->fail(SAGE2OV_ERR_LIMIT, "sage2ov_mcf_solve: too many nodes");
    McfStats s;
    const int rc = dev_mcf_solve(c->device(), arcs, m, (uint32_t)n, max_rounds, false, flow, price, &s, c->err);
    mcf_stats_set(c, s);
    int out = rc;
    if (!rc && !mcf_total_cost(flow, m, [&](uint64_t i) { return arcs[i].cost; }, &c->mcfstats.total_cost)) out = c->fail(SAGE2OV_ERR_LIMIT, "sage2ov_mcf_solve: the total cost does not fit 64 bits");
    if (stats) *stats = c->mcfstats;
    return out;
}
int sage2ov_mcf_solve_wide(sage2ov_ctx* c, uint64_t n, const sage2ov_mcf_arc* arcs, uint64_t m, uint64_t max_rounds, int64_t* flow, uint64_t* price, sage2ov_mcf_stats* stats) {
    if (!c) return SAGE2OV_ERR_ARG;
    if (m && (!arcs || !flow)) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_mcf_solve_wide: null argument");
    if (n >= 0xFFFFFFF0ull) return c->fail(SAGE2OV_ERR_LIMIT, "sage2ov_mcf_solve_wide: too many nodes");
    // the guard on the host's copy of the costs, before the device is touched (the solve holds the device's maximum against it again)
    uint64_t maxc = 0;
    for (uint64_t i = 0; i < m; i++) maxc = std::max<uint64_t>(maxc, arcs[i].cost < 0 ? 0ull - (uint64_t)arcs[i].cost : (uint64_t)arcs[i].cost);
    McfStats s; s.nodes = n; s.arcs = m; s.scale = n + 1; s.priceWords = 2;
    int rc = 0;
    if (!mcf_wide_guard(n, maxc)) rc = c->fail(SAGE2OV_ERR_LIMIT, "min-cost flow: (n + 1) * max |cost| and the price range of the method do not fit 128 bits");
    else if (!c->device()) rc = c->fail(SAGE2OV_ERR_DEVICE, c->gpu() ? c->devErr : "sage2ov_mcf_solve_wide: this context has no GPU");
    else rc = dev_mcf_solve(c->device(), arcs, m, (uint32_t)n, max_rounds, true, flow, price, &s, c->err);
    mcf_stats_set(c, s);
    int out = rc;
    if (!rc && !mcf_total_cost(flow, m, [&](uint64_t i) { return arcs[i].cost; }, &c->mcfstats.total_cost)) out = c->fail(SAGE2OV_ERR_LIMIT, "sage2ov_mcf_solve_wide: the total cost does not fit 64 bits");
    if (stats) *stats = c->mcfstats;
    return out;
}
int sage2ov_flow_solve(sage2ov_ctx* c, uint64_t max_rounds, sage2ov_mcf_stats* stats) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = copycount_check(c, "sage2ov_flow_solve"); if (rc) return rc; }
    if (!c->netValid) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_flow_solve: build the flow network first (sage2ov_flow_network_build)");
    McfStats s;
    const int rc = dev_flow_solve(c->device(), max_rounds, &s, c->err);
    mcf_stats_set(c, s);
    int out = rc;
    if (!rc) {
        std::vector<FlowArc> arcs(c->ccstats.network_arcs); std::vector<int64_t> flow(arcs.size());
        out = dev_flownet_export(c->device(), arcs.data(), c->err);
        if (!out) out = dev_flow_solution_get(c->device(), flow.data(), nullptr, c->err);
        if (!out && !mcf_total_cost(flow.data(), flow.size(), [&](uint64_t i) { return mcf_trunc(arcs[i].cost); }, &c->mcfstats.total_cost))
            out = c->fail(SAGE2OV_ERR_LIMIT, "sage2ov_flow_solve: the total cost does not fit 64 bits");
    }
    if (stats) *stats = c->mcfstats;
    return out;
}
int sage2ov_flow_solution_export(sage2ov_ctx* c, int64_t* flow, uint64_t cap_flow, int64_t* price, uint64_t cap_price, uint64_t* scale) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = copycount_check(c, "sage2ov_flow_solution_export"); if (rc) return rc; }
    if (!c->netValid || !dev_flow_solved(c->device())) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_flow_solution_export: no solution of the present network (sage2ov_flow_solve)");
    if ((flow && cap_flow < c->ccstats.network_arcs) || (price && cap_price < c->ccstats.network_nodes)) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_flow_solution_export: a buffer is too small");
    if (price && dev_flow_price_words(c->device()) != 1) return c->fail(SAGE2OV_ERR_LIMIT, "sage2ov_flow_solution_export: the solution has 128-bit prices (sage2ov_flow_solution_export_wide)");
    if (scale) *scale = c->ccstats.network_nodes + 1;
    return dev_flow_solution_get(c->device(), flow, price, c->err);
}
int sage2ov_flow_solution_export_wide(sage2ov_ctx* c, int64_t* flow, uint64_t cap_flow, uint64_t* price, uint64_t cap_price, uint64_t* scale) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = copycount_check(c, "sage2ov_flow_solution_export_wide"); if (rc) return rc; }
    if (!c->netValid || !dev_flow_solved(c->device())) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_flow_solution_export_wide: no solution of the present network (sage2ov_flow_solve)");
    const uint64_t nn = c->ccstats.network_nodes;
    if ((flow && cap_flow < c->ccstats.network_arcs) || (price && cap_price < nn)) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_flow_solution_export_wide: a buffer is too small");
    if (scale) *scale = nn + 1;
    if (!price || dev_flow_price_words(c->device()) == 2) return dev_flow_solution_get(c->device(), flow, price, c->err);
    std::vector<int64_t> p(nn);                                                        // 64-bit prices: sign-extended
    { const int rc = dev_flow_solution_get(c->device(), flow, p.data(), c->err); if (rc) return rc; }
    for (uint64_t v = 0; v < nn; v++) { price[2 * v] = (uint64_t)p[v]; price[2 * v + 1] = p[v] < 0 ? ~0ull : 0ull; }
    return SAGE2OV_OK;
}
int sage2ov_flow_solution_save(sage2ov_ctx* c, const char* path) {
    if (!c || !path) return SAGE2OV_ERR_ARG;
    { const int rc = copycount_check(c, "sage2ov_flow_solution_save"); if (rc) return rc; }
    if (!c->netValid || !dev_flow_solved(c->device())) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_flow_solution_save: no solution of the present network (sage2ov_flow_solve)");
    std::vector<FlowArc> arcs(c->ccstats.network_arcs); std::vector<int64_t> flow(arcs.size());
    { const int rc = dev_flownet_export(c->device(), arcs.data(), c->err); if (rc) return rc; }
    { const int rc = dev_flow_solution_get(c->device(), flow.data(), nullptr, c->err); if (rc) return rc; }
    std::vector<uint32_t> order; order.reserve(arcs.size());
    for (uint64_t i = 0; i < arcs.size(); i++) if (arcs[i].upper > 0) order.push_back((uint32_t)i);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return arcs[a].from < arcs[b].from; });      // by tail, then input order
    FILE* f = fopen(path, "w"); if (!f) return c->fail(SAGE2OV_ERR_IO, std::string("cannot open ") + path);
    std::vector<char> io(1 << 22); setvbuf(f, io.data(), _IOFBF, io.size());
    for (uint32_t i : order) fprintf(f, "%u %u %lld\n", arcs[i].from, arcs[i].to, (long long)flow[i]);
    const bool bad = ferror(f) != 0;
    if (fclose(f) != 0 || bad) return c->fail(SAGE2OV_ERR_IO, std::string("cannot write ") + path);
    return SAGE2OV_OK;
}
int sage2ov_flow_solution_commit(sage2ov_ctx* c) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = copycount_check(c, "sage2ov_flow_solution_commit"); if (rc) return rc; }
    if (!c->netValid || !dev_flow_solved(c->device())) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_flow_solution_commit: no solution of the present network (sage2ov_flow_solve)");
    CopyCountStats s; uint64_t tts = 0, lines = 0;
    c->supports_forget(); c->paths_forget(); c->contigs_forget();
    { const int rc = dev_flow_commit(c->device(), &s, &tts, &lines, c->err); if (rc) return rc; }
    std::vector<float> f(c->g4.n_half_edges, 0.f);
    { const int rc = dev_flow_get(c->device(), f.data(), f.size(), c->err); if (rc) return rc; }
    c->g4.flow = std::move(f);
    sage2ov_copycount_stats& o = c->ccstats;
    o.t_to_s_flow = tts; o.flow_different = s.different; o.solution_lines = lines; o.lines_applied = s.applied;
    copycount_times(c, s);
    return SAGE2OV_OK;
}
int sage2ov_copy_counts(sage2ov_ctx* c, uint64_t* genome_size) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = sage2ov_genome_size_estimate(c, genome_size); if (rc) return rc; }
    { const int rc = sage2ov_flow_network_build(c); if (rc) return rc; }
    { const int rc = sage2ov_flow_solve(c, 0, nullptr); if (rc) return rc; }
    return sage2ov_flow_solution_commit(c);
}
int sage2ov_mcf_stats_get(const sage2ov_ctx* c, sage2ov_mcf_stats* o) { if (!c || !o) return SAGE2OV_ERR_ARG; *o = c->mcfstats; return SAGE2OV_OK; }
int sage2ov_mcf_hub_stats_get(const sage2ov_ctx* c, uint64_t out[6]) {
    if (!c || !out) return SAGE2OV_ERR_ARG;
    if (!c->device()) return SAGE2OV_ERR_DEVICE;
    for (int i = 0; i < 6; i++) out[i] = c->mcfhub[i];
    return SAGE2OV_OK;
}
int sage2ov_mates_supports(sage2ov_ctx* c) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = readmap_check(c, "sage2ov_mates_supports"); if (rc) return rc; }
    { const int rc = estimate_ensure(c); if (rc) return rc; }
    c->supports_forget();
    const int64_t arl = (int64_t)average_read_length(c), k = (int64_t)c->cfg.min_overlap;
    SupportParams P; P.bound = c->maxUpper; P.libraries = c->mateLibraries;
    for (int lib = 1; lib <= (int)c->mateLibraries && lib < 128; lib++) P.thr[lib] = c->inserts[lib].valid ? c->inserts[lib].upper + k - 2 * arl : 0;
    SupportStats s; const int rc = dev_support_build(c->device(), P, &s, c->err); if (rc) return rc;
    sage2ov_support_stats& o = c->sstats;
    o.in_halves = s.in_halves; o.out_halves = s.out_halves; o.candidates = s.candidates; o.entries_within = s.entries_within; o.records = s.records; o.keys = s.keys; o.keys2 = s.keys2;
    o.sort_passes = s.passes; o.roles_ms = s.roles_ms; o.scan_ms = s.scan_ms; o.records_ms = s.records_ms; o.sort_ms = s.sort_ms; o.reduce_ms = s.reduce_ms;
    c->supValid = true;
    return SAGE2OV_OK;
}
int sage2ov_mates_supports_count(sage2ov_ctx* c, uint32_t min_support, uint64_t* n) {
    if (!c || !n) return SAGE2OV_ERR_ARG;
    { const int rc = supports_ensure(c, "sage2ov_mates_supports_count"); if (rc) return rc; }
    { const int rc = supports_fetch(c); if (rc) return rc; }
    uint64_t m = 0; for (const sage2ov_support& e : c->supports) m += e.support >= min_support;
    *n = m; return SAGE2OV_OK;
}
int sage2ov_mates_supports_export(sage2ov_ctx* c, uint32_t min_support, sage2ov_support* out, uint64_t cap) {
    if (!c) return SAGE2OV_ERR_ARG;
    uint64_t m = 0; { const int rc = sage2ov_mates_supports_count(c, min_support, &m); if (rc) return rc; }
    if (cap < m) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_mates_supports_export: the buffer holds fewer entries than the table (sage2ov_mates_supports_count)");
    if (m && !out) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_mates_supports_export: null argument");
    uint64_t at = 0; for (const sage2ov_support& e : c->supports) if (e.support >= min_support) out[at++] = e;
    return SAGE2OV_OK;
}
int sage2ov_support_stats_get(const sage2ov_ctx* c, sage2ov_support_stats* o) { if (!c || !o) return SAGE2OV_ERR_ARG; *o = c->sstats; return SAGE2OV_OK; }

// ---- the first loop of ContigExtender::extendContigs (mergeContigs.cpp:47-60, :959-1030, :1112-1469); the semantics are stated in sage2ov.h
namespace {
static_assert(sizeof(sage2ov_merge) == 40 && sizeof(sage2ov_extend_counts) == 96 && sizeof(sage2ov_extend_stats) == 208, "the records of the merge rounds");
inline int combined_type(unsigned t1, unsigned t2) {                                   // overlapGraph.cpp:259-266
    if ((t1 == 0 && t2 == 0) || (t1 == 1 && t2 == 2)) return 0;
    if ((t1 == 0 && t2 == 1) || (t1 == 1 && t2 == 3)) return 1;
    if ((t1 == 2 && t2 == 0) || (t1 == 3 && t2 == 2)) return 2;
    if ((t1 == 2 && t2 == 1) || (t1 == 3 && t2 == 3)) return 3;
    return -1;
}
// lines 1 and 2 of P.graph6: what sage2ov_graph5_save would write before the first merge
int header_hold(sage2ov_ctx* c) {
    if (c->hdrHeld) return SAGE2OV_OK;
    if (!c->gsValid) { const int rc = genome_estimate(c); if (rc) return rc; }
    c->hdrGenome = c->ccstats.genome_size; c->hdrReads = c->ccstats.reads_present; c->hdrHeld = true;
    return SAGE2OV_OK;
}
int link_length_threshold(const sage2ov_ctx* c) { return (int)ceilf((float)(100 * ((double)average_read_length(c) / 100.0))); }      // scaffolding.cpp:20
// a batch of splices on internal half-edges: merges (mergeEdgesAndUpdate) or joins (mergeDisconnectedEdges; gap, and ov comes back), with what the device planned
struct SpliceBatch {
    std::vector<uint32_t> a, b; std::vector<int32_t> gap; std::vector<SplicePlan> plan; std::vector<int32_t> ov; SpliceStats s;
    void clear() { a.clear(); b.clear(); gap.clear(); }
};
// the batch through the device (typeOfMerge 0: joins); afterwards everything made from the graph is stale, the estimate stands and the host copy of the fields is gone.
// The flows come back when the host had them, and after joins always (flows that were all 0 are an array now: the new edges have 1.0)
int splice_apply(sage2ov_ctx* c, SpliceBatch& B, int typeOfMerge) {
    { const int rc = header_hold(c); if (rc) return rc; }
    const bool join = typeOfMerge == 0; const uint64_t n = B.a.size();
    B.plan.assign(n, SplicePlan{}); B.ov.assign(join ? 2 * n : 0, 0); SpliceStats& s = B.s;
    { const int rc = join ? dev_join_pairs(c->device(), B.a.data(), B.b.data(), B.gap.data(), n, B.plan.data(), B.ov.data(), &s, c->err)
                          : dev_merge_pairs(c->device(), B.a.data(), B.b.data(), n, typeOfMerge, B.plan.data(), &s, c->err); if (rc) return rc; }
    if (!s.made) return SAGE2OV_OK;
    const bool est = c->estimated;
    c->rmValid = false; c->pairOrdinal.clear(); c->rmstats = sage2ov_readmap_stats{}; c->supports_forget(); c->paths_forget(); c->links_forget(); c->contigs_forget(); c->copycount_forget();
    c->estimateHeld = est;
    SimplifiedGraph& g = c->g4;
    g.downloaded = g.fields = false; g.lists.clear(); g.lists.shrink_to_fit();
    g.n_half_edges = s.half_edges; g.pairs_alive += s.made; g.pairs_alive -= std::min<uint64_t>(g.pairs_alive, s.pairs_deleted);
    if (!join && g.flow.empty()) return SAGE2OV_OK;
    g.flow.assign(g.n_half_edges, 0.f);
    return dev_flow_get(c->device(), g.flow.data(), g.flow.size(), c->err);
}
// (pair ordinal, reversed) of the two batch entry points -> the half-edges B.a, B.b, with the checks on what a batch may name.  A join also rejects a == b's pair; a
// merge lets that through, so that the device refuses it without an error
int splice_operands(sage2ov_ctx* c, const std::string& who, const uint32_t* pf, const uint8_t* fr, const uint32_t* ps, const uint8_t* sr, uint64_t n, bool join, SpliceBatch& B) {
    { const int rc = dev_simplify_download(c->device(), c->g4, c->err, false); if (rc) return rc; }
    const SimplifiedGraph& g = c->g4;
    std::vector<uint32_t> first; g4_save_order(g, first);                              // ordinal -> the half that opens the record pair (a loop has two ordinals, one per half)
    B.a.resize(n); B.b.resize(n); std::vector<uint8_t> used(g.n_half_edges / 2 + 1, 0);
    for (uint64_t i = 0; i < n; i++) {
        if (pf[i] >= first.size() || ps[i] >= first.size()) return c->fail(SAGE2OV_ERR_ARG, who + ": a pair ordinal beyond the record pairs of the graph");
        const uint32_t a = B.a[i] = first[pf[i]] ^ (fr[i] ? 1u : 0u), b = B.b[i] = first[ps[i]] ^ (sr[i] ? 1u : 0u);
        if ((join && (a >> 1) == (b >> 1)) || used[a >> 1] || used[b >> 1])
            return c->fail(SAGE2OV_ERR_ARG, who + (join ? ": a record pair is named twice in the batch" : ": a record pair is named by two merges of the batch"));
        used[a >> 1] = used[b >> 1] = 1;
        if (join && (!g.cnt[a] || !g.cnt[b])) return c->fail(SAGE2OV_ERR_ARG, who + ": an operand without a read list (the reference joins composite edges only)");
        if (!join && g.to[a] != g.from[b]) return c->fail(SAGE2OV_ERR_ARG, who + ": the first edge does not end where the second begins");
    }
    return SAGE2OV_OK;
}
// what a round of merges or of joins (typeOfMerge 0) keeps around its selection rule: the working copy of the half-edge fields, SEARCH with its keys filed under their
// end nodes, the batch on its way to the device, and the accounting
extern "C++" { struct SpliceRound {
    sage2ov_ctx* c; std::string who; int typeOfMerge;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> ordBefore, from, to, len, cnt; std::vector<uint8_t> type, alive; std::vector<float> flow;
    uint32_t nh, devNh;                                                                // the half-edges of the working copy, and of the device's graph (behind by the batch)
    std::unordered_map<uint64_t, uint32_t> search; std::unordered_multimap<uint32_t, uint64_t> filed;
    SpliceBatch batch; std::unordered_set<uint32_t> usedPair;
    std::vector<uint32_t> newHalf; std::vector<SplicePlan> want, plans; std::vector<int32_t> ov;      // of the whole round, in selection order: want as selected, plans and ov as the device made them
    SpliceStats sum; uint64_t batches = 0; double deviceMs = 0;                        // deviceMs: time spent in the device batches, not selection

    SpliceRound(sage2ov_ctx* ctx, const char* name, int merge) : c(ctx), who(name), typeOfMerge(merge), ordBefore(ctx->pairOrdinal), from(ctx->g4.from), to(ctx->g4.to), len(ctx->g4.len),
        cnt(ctx->g4.cnt), type(ctx->g4.type), alive(ctx->g4.alive), flow(ctx->g4.flow) { flow.resize(from.size(), 0.f); nh = devNh = (uint32_t)from.size(); }
    static uint64_t k2(uint64_t x, uint64_t y) { return (x << 32) | y; }
    uint64_t xk(uint32_t h) const { return (uint64_t)(from[h] ^ to[h]); }
    uint64_t key(uint32_t h1, uint32_t h2) const { return k2(xk(h1), xk(h2)); }
    void insert(uint32_t e1, uint32_t e2, uint32_t sup) {                             // the highest support of a key; the key under the four end nodes
        const uint64_t kk = key(e1, e2);
        auto it = search.find(kk);
        if (it == search.end()) search[kk] = sup; else if (sup > it->second) it->second = sup;
        for (uint32_t nd : {to[e1], from[e1], to[e2], from[e2]}) filed.insert({nd, kk});
    }
    int64_t find(uint64_t kk) const { auto it = search.find(kk); return it == search.end() ? -1 : (int64_t)it->second; }
    bool erase_at(uint32_t node, uint64_t own) {                                       // every key filed under the node goes; true: one that was still there and is not `own`
        bool others = false;
        auto its = filed.equal_range(node);
        for (auto it = its.first; it != its.second; ++it) if (search.erase(it->second) && it->second != own) others = true;
        return others;
    }
    int flush() {
        if (batch.a.empty()) return SAGE2OV_OK;
        const auto f0 = std::chrono::steady_clock::now();
        { const int rc = splice_apply(c, batch, typeOfMerge); if (rc) return rc; }
        const SpliceStats& s = batch.s;
        for (const SplicePlan& p : batch.plan) if (!p.made) return c->fail(SAGE2OV_ERR_INTERNAL, who + ": the device refused a merge the selection made");
        if (s.half_edges != nh) return c->fail(SAGE2OV_ERR_INTERNAL, who + ": the device and the selection disagree on the half-edges");
        for (size_t i = 0; i < batch.plan.size(); i++) {
            const SplicePlan &p = batch.plan[i], &w = want[plans.size() + i];
            if (p.type != w.type || p.del1 != w.del1 || p.del2 != w.del2) return c->fail(SAGE2OV_ERR_INTERNAL, who + ": the device and the selection disagree on a " + (typeOfMerge ? "merge" : "join"));
        }
        plans.insert(plans.end(), batch.plan.begin(), batch.plan.end()); ov.insert(ov.end(), batch.ov.begin(), batch.ov.end());
        sum.entries_copied += s.entries_copied; sum.pairs_deleted += s.pairs_deleted; sum.overlaps += s.overlaps; sum.concatenated += s.concatenated; sum.gapped += s.gapped;
        sum.overlap_ms += s.overlap_ms; sum.plan_ms += s.plan_ms; sum.lists_ms += s.lists_ms; sum.commit_ms += s.commit_ms; batches++;
        batch.clear(); usedPair.clear(); devNh = nh;
        deviceMs += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - f0).count();
        return SAGE2OV_OK;
    }
    // before (e1, e2) is taken: the batch goes first when it names an operand's pair or made one of the operands; the half-edge limit
    int make_room(uint32_t e1, uint32_t e2) {
        if (e1 >= devNh || e2 >= devNh || usedPair.count(e1 >> 1) || usedPair.count(e2 >> 1)) { const int rc = flush(); if (rc) return rc; }
        if ((uint64_t)nh + 2 >= (1ull << 32) - 4096) return c->fail(SAGE2OV_ERR_LIMIT, who + ": more than 2^32 half-edges");
        return SAGE2OV_OK;
    }
    uint32_t push_pair(uint32_t e1, uint32_t e2, uint8_t t, float f) {                 // insertEdge; the lengths of a round's own edges are not read (a join's are the device's to find)
        const uint32_t h = nh, n = cnt[e1] + cnt[e2] + (to[e1] == from[e2] ? 1u : 2u);
        from.push_back(from[e1]); to.push_back(to[e2]); type.push_back(t); len.push_back(0); cnt.push_back(n); alive.push_back(1); flow.push_back(f);
        from.push_back(to[e2]); to.push_back(from[e1]); type.push_back((uint8_t)flip_type_host(t)); len.push_back(0); cnt.push_back(n); alive.push_back(1); flow.push_back(f);
        nh += 2; return h;
    }
    void retire(uint32_t e, bool deleted, float f) { if (deleted) alive[e] = alive[e ^ 1u] = 0; else { flow[e] -= f; flow[e ^ 1u] -= f; } }
    // the selected splice on the working copy and into the batch; the new forward half
    uint32_t splice(uint32_t e1, uint32_t e2, uint8_t t, float f, bool del1, bool del2, int32_t gap) {
        const uint32_t h = push_pair(e1, e2, t, f);
        retire(e1, del1, f); retire(e2, del2, f);
        batch.a.push_back(e1); batch.b.push_back(e2); if (!typeOfMerge) batch.gap.push_back(gap);
        usedPair.insert(e1 >> 1); usedPair.insert(e2 >> 1);
        SplicePlan w{}; w.type = t; w.del1 = del1; w.del2 = del2; want.push_back(w); newHalf.push_back(h);
        return h;
    }
    // the end of a round: the last batch, the ordinals of the new pairs in the graph as it is now, the counters both kinds of round have
    template <class Rec, class Counts> int finish(std::vector<Rec>& recs, Counts& R) {
        { const int rc = flush(); if (rc) return rc; }
        R.entries_copied = sum.entries_copied; R.pairs_deleted = sum.pairs_deleted; R.batches = batches; R.lists_ms = sum.lists_ms; R.commit_ms = sum.plan_ms + sum.commit_ms;
        R.select_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - deviceMs;
        if (recs.empty()) return SAGE2OV_OK;
        { const int rc = pair_ordinals(c); if (rc) return rc; }
        for (size_t i = 0; i < recs.size(); i++) recs[i].pair_new = (newHalf[i] >> 1) < c->pairOrdinal.size() ? c->pairOrdinal[newHalf[i] >> 1] : ~0u;
        return SAGE2OV_OK;
    }
}; }
// the node lists as a merge round finds them (alive halves by ascending index; walked backwards: newest first) and the halves the round adds
extern "C++" { struct NodeLists {
    const SpliceRound& S; std::vector<uint32_t> offs, adj; std::unordered_map<uint32_t, std::vector<uint32_t>> added;
    NodeLists(const SpliceRound& round, uint64_t N) : S(round), offs(N + 2, 0) {
        for (uint32_t h = 0; h < S.nh; h++) if (S.alive[h]) offs[S.from[h] + 1]++;
        for (uint64_t i = 0; i <= N; i++) offs[i + 1] += offs[i];
        adj.resize(offs[N + 1]);
        std::vector<uint32_t> cur(offs.begin(), offs.end() - 1); for (uint32_t h = 0; h < S.nh; h++) if (S.alive[h]) adj[cur[S.from[h]]++] = h;
    }
    template <class F> void walk(uint32_t node, F&& fn) const {
        auto it = added.find(node);
        if (it != added.end()) for (size_t x = it->second.size(); x-- > 0;) if (S.alive[it->second[x]]) fn(it->second[x]);
        for (uint32_t x = offs[node + 1]; x-- > offs[node];) if (S.alive[adj[x]]) fn(adj[x]);
    }
}; }
void counts_add(sage2ov_extend_counts& t, const sage2ov_extend_counts& r) {
    t.entries += r.entries; t.at_threshold += r.at_threshold; t.refused += r.refused; t.blocked += r.blocked; t.merges += r.merges; t.entries_copied += r.entries_copied;
    t.pairs_deleted += r.pairs_deleted; t.batches += r.batches; t.sweep_ms += r.sweep_ms; t.select_ms += r.select_ms; t.lists_ms += r.lists_ms; t.commit_ms += r.commit_ms;
}
}  // namespace
int sage2ov_graph_merge_pairs(sage2ov_ctx* c, const uint32_t* pf, const uint8_t* fr, const uint32_t* ps, const uint8_t* sr, uint64_t n, int type, uint8_t* merged) {
    if (!c) return SAGE2OV_ERR_ARG;
    if (type != 1 && type != 2) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_graph_merge_pairs: type_of_merge is 1 or 2");
    if (n && (!pf || !fr || !ps || !sr)) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_graph_merge_pairs: null argument");
    { const int rc = readmap_check(c, "sage2ov_graph_merge_pairs"); if (rc) return rc; }
    if (n >= (1ull << 31)) return c->fail(SAGE2OV_ERR_LIMIT, "sage2ov_graph_merge_pairs: more merges than there can be pairs");
    SpliceBatch B;
    { const int rc = splice_operands(c, "sage2ov_graph_merge_pairs", pf, fr, ps, sr, n, false, B); if (rc) return rc; }
    const SimplifiedGraph& g = c->g4;
    for (uint64_t i = 0; i < n; i++)
        for (uint32_t h : {B.a[i], B.b[i]})
            if (g.cnt[h] == 0 && (g.len[h] > 0x7FF || g.len[h ^ 1u] > 0x7FF))
                return c->fail(SAGE2OV_ERR_LIMIT, "sage2ov_graph_merge_pairs: a simple edge longer than 2047 (the 11-bit field of a list entry)");
    { const int rc = splice_apply(c, B, type); if (rc) return rc; }
    if (merged) for (uint64_t i = 0; i < n; i++) merged[i] = B.plan[i].made;
    return SAGE2OV_OK;
}
int sage2ov_extend_threshold(uint64_t reads, uint64_t arl, uint64_t genomeSize, uint32_t iteration, int* high) {     // mergeContigs.cpp:43-54
    if (!high || !arl || !genomeSize || !iteration) return SAGE2OV_ERR_ARG;
    const float coverage = (reads * arl) / genomeSize;
    double factor = 0.20;
    if (genomeSize > 1000000000) { if (iteration >= 4 && iteration <= 6) factor = 0.10; else if (iteration > 6) factor = 0.05; }
    *high = (int)ceilf((factor * coverage) * (100.0 / arl));
    return SAGE2OV_OK;
}
int sage2ov_extend_round(sage2ov_ctx* c, int highTh, int lowTh, uint64_t* merged) {                                   // :959-1030, :1112-1255
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = readmap_check(c, "sage2ov_extend_round"); if (rc) return rc; }
    sage2ov_extend_counts R{};
    const bool swept = !(c->supValid && c->estimated && c->rmValid);
    { const int rc = supports_ensure(c, "sage2ov_extend_round"); if (rc) return rc; }
    if (swept) R.sweep_ms = c->sstats.roles_ms + c->sstats.scan_ms + c->sstats.records_ms + c->sstats.sort_ms + c->sstats.reduce_ms;
    Device* d = c->device();
    const uint64_t E = dev_support_count(d);
    std::vector<uint64_t> key(E); std::vector<uint32_t> sup(E);
    { const int rc = dev_support_export(d, key.data(), sup.data(), c->err); if (rc) return rc; }
    { const int rc = pair_ordinals(c); if (rc) return rc; }                           // (the half-edge fields come with it; no read list)
    SpliceRound S(c, "sage2ov_extend_round", 1);
    const std::vector<uint32_t>&ordBefore = S.ordBefore, &from = S.from, &to = S.to, &cnt = S.cnt; const std::vector<uint8_t>&type = S.type, &alive = S.alive; const std::vector<float>& flow = S.flow;
    NodeLists lists(S, c->g4.N); std::unordered_map<uint32_t, std::vector<uint32_t>>& added = lists.added;
    auto walk = [&](uint32_t node, auto&& fn) { lists.walk(node, fn); };
    // the list in building order (node ascending, in-half newest first, out-half newest first), SEARCH and the entries filed under their end nodes
    struct Ent { uint32_t e1, e2, sup, node; };
    std::vector<Ent> list;
    for (uint64_t e = 0; e < E; e++) if (sup[e] > 1) { const uint32_t ia = (uint32_t)(key[e] >> 32), ob = (uint32_t)key[e]; list.push_back(Ent{ia ^ 1u, ob, sup[e], from[ia]}); }
    std::sort(list.begin(), list.end(), [](const Ent& x, const Ent& y) { return x.node != y.node ? x.node < y.node : (x.e1 != y.e1 ? x.e1 > y.e1 : x.e2 > y.e2); });
    auto k2 = [&](uint32_t h1, uint32_t h2) -> uint64_t { return S.key(h1, h2); };
    for (const Ent& en : list) S.insert(en.e1, en.e2, en.sup);
    std::stable_sort(list.begin(), list.end(), [](const Ent& x, const Ent& y) { return x.sup > y.sup; });
    R.entries = list.size(); for (const Ent& en : list) R.at_threshold += (int64_t)en.sup >= (int64_t)highTh;
    auto lookup = [&](uint64_t kk) -> int64_t { return S.find(kk); };
    std::unordered_set<uint32_t> blocked; std::vector<sage2ov_merge> merges;
    for (const Ent& en : list) {
        const uint32_t e1 = en.e1, e2 = en.e2;
        if (!alive[e1] || !alive[e2]) continue;                                        // (difference 3)
        if (lookup(k2(e1, e2)) < 0) continue;
        const uint32_t node = to[e1];
        if (blocked.count(node)) { R.blocked++; continue; }
        if ((int64_t)en.sup < (int64_t)highTh) break;
        bool unique = true;
        walk(node, [&](uint32_t v) {
            if (!(flow[v] >= 1.f) || cnt[v] == 0 || to[v] == from[v]) return;
            if ((v ^ 1u) != e1 && combined_type(type[v ^ 1u], type[e2]) >= 0) {
                int64_t s = lookup(k2(v ^ 1u, e2)); if (s < 0) s = lookup(k2(e2 ^ 1u, v)); if (s > lowTh) unique = false;
            }
            if (v != e2 && combined_type(type[e1], type[v]) >= 0) {
                int64_t s = lookup(k2(e1, v)); if (s < 0) s = lookup(k2(v ^ 1u, e1 ^ 1u)); if (s > lowTh) unique = false;
            }
        });
        if (!unique) { R.refused++; continue; }
        walk(node, [&](uint32_t v) { if (to[v] != from[v]) blocked.insert(to[v]); });
        const int t = combined_type(type[e1], type[e2]);
        if (e1 == e2 || e1 == (e2 ^ 1u) || t < 0) continue;                            // mergeEdgesAndUpdate returns NULL
        { const int rc = S.make_room(e1, e2); if (rc) return rc; }
        const float f1 = flow[e1], f2 = flow[e2], f = (f1 == 0.f && f2 == 0.f) ? 0.f : 1.f;
        sage2ov_merge m{}; m.node = node; m.from = from[e1]; m.to = to[e2]; m.support = en.sup; m.flow = f; m.type = (uint8_t)t;
        m.pair_in = (e1 >> 1) < ordBefore.size() ? ordBefore[e1 >> 1] : ~0u; m.pair_out = (e2 >> 1) < ordBefore.size() ? ordBefore[e2 >> 1] : ~0u; m.pair_new = ~0u;
        m.in_deleted = f1 <= f; m.out_deleted = f2 <= f;
        const uint32_t h = S.splice(e1, e2, (uint8_t)t, f, m.in_deleted, m.out_deleted, 0);
        added[from[h]].push_back(h); added[from[h + 1]].push_back(h + 1);
        merges.push_back(m);
        S.erase_at(node, 0);                                                           // (difference 2: the key is the node)
    }
    { const int rc = S.finish(merges, R); if (rc) return rc; }
    R.merges = merges.size();
    c->xmerges = std::move(merges);
    c->xstats.rounds++; c->xstats.last = R; counts_add(c->xstats.total, R);
    if (merged) *merged = R.merges;
    return SAGE2OV_OK;
}
int sage2ov_extend_by_supports(sage2ov_ctx* c, uint64_t genomeSize, uint64_t* rounds, uint64_t* merged) {             // :47-60
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = readmap_check(c, "sage2ov_extend_by_supports"); if (rc) return rc; }
    { const int rc = header_hold(c); if (rc) return rc; }
    const uint64_t gs = genomeSize ? genomeSize : c->hdrGenome, reads = c->hdrReads, arl = average_read_length(c);
    if (!gs || !arl) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_extend_by_supports: a genome size or an average read length of 0");
    uint64_t r = 0, total = 0;
    for (uint32_t it = 1; it <= 10000; it++) {
        int high = 0; sage2ov_extend_threshold(reads, arl, gs, it, &high);
        uint64_t m = 0; { const int rc = sage2ov_extend_round(c, high, 1, &m); if (rc) return rc; }
        r++; total += m;
        if (rounds) *rounds = r; if (merged) *merged = total;
        if (!m) return SAGE2OV_OK;
    }
    return c->fail(SAGE2OV_ERR_INTERNAL, "sage2ov_extend_by_supports: 10 000 rounds without a fixed point");
}
int sage2ov_extend_merges_count(const sage2ov_ctx* c, uint64_t* n) { if (!c || !n) return SAGE2OV_ERR_ARG; *n = c->xmerges.size(); return SAGE2OV_OK; }
int sage2ov_extend_merges_export(const sage2ov_ctx* c, sage2ov_merge* out, uint64_t cap) {
    if (!c || cap < c->xmerges.size() || (!out && !c->xmerges.empty())) return SAGE2OV_ERR_ARG;
    if (!c->xmerges.empty()) memcpy(out, c->xmerges.data(), c->xmerges.size() * sizeof(sage2ov_merge));
    return SAGE2OV_OK;
}
int sage2ov_extend_stats_get(const sage2ov_ctx* c, sage2ov_extend_stats* o) { if (!c || !o) return SAGE2OV_ERR_ARG; *o = c->xstats; return SAGE2OV_OK; }
int sage2ov_graph6_save(sage2ov_ctx* c, const char* path) {                            // overlapGraph.cpp:338-369
    if (!c || !path) return SAGE2OV_ERR_ARG;
    if (!c->hdrHeld) return sage2ov_graph5_save(c, path);
    { const int rc = copycount_check(c, "sage2ov_graph6_save"); if (rc) return rc; }
    return save_composite(c, path, true, (unsigned long long)c->hdrGenome, (unsigned long long)c->hdrReads);
}

// ---- PATH SUPPORTS: the second and third loop of ContigExtender::extendContigs (mergeContigs.cpp:62-99, :118-353, :794-952, :2148-2546); the semantics are stated in sage2ov.h
namespace {
static_assert(sizeof(sage2ov_path_support) == 28 && sizeof(sage2ov_path_stats) == 152, "the records of the path supports");
int paths_ensure(sage2ov_ctx* c, const char* who) {
    { const int rc = readmap_check(c, who); if (rc) return rc; }
    if (c->pathValid && c->estimated && c->rmValid) return SAGE2OV_OK;
    return sage2ov_path_supports(c);
}
// the table in table order (node ascending, a newest first, b newest first), on the host, with the number of rows that share their XOR key with an earlier one
int paths_fetch(sage2ov_ctx* c) {
    Device* d = c->device(); const uint64_t E = dev_paths_count(d);
    std::vector<uint64_t> key(E); std::vector<uint32_t> sup(E);
    { const int rc = dev_paths_export(d, key.data(), sup.data(), c->err); if (rc) return rc; }
    { const int rc = pair_ordinals(c); if (rc) return rc; }
    const SimplifiedGraph& g = c->g4; const std::vector<uint32_t>& ord = c->pairOrdinal;
    std::vector<uint32_t> order, first(g.n_half_edges / 2 + 1, ~0u); g4_save_order(g, order);
    for (uint32_t h : order) if (first[h >> 1] == ~0u) first[h >> 1] = h;
    std::vector<uint64_t> at(E); for (uint64_t e = 0; e < E; e++) at[e] = e;
    std::sort(at.begin(), at.end(), [&](uint64_t x, uint64_t y) {
        const uint32_t ax = (uint32_t)(key[x] >> 32), bx = (uint32_t)key[x], ay = (uint32_t)(key[y] >> 32), by = (uint32_t)key[y];
        return g.to[ax] != g.to[ay] ? g.to[ax] < g.to[ay] : (ax != ay ? ax > ay : bx > by); });
    c->prows.resize(E); c->pkeys.resize(E);
    std::unordered_set<uint64_t> xors;
    for (uint64_t e = 0; e < E; e++) {
        const uint64_t k = key[at[e]]; const uint32_t a = (uint32_t)(k >> 32), b = (uint32_t)k;
        sage2ov_path_support o{}; o.node = g.to[a]; o.pair_a = ord[a >> 1]; o.pair_b = ord[b >> 1]; o.from_a = g.from[a]; o.to_b = g.to[b]; o.support = sup[at[e]];
        o.second_a = first[a >> 1] == a ? 0 : 1; o.second_b = first[b >> 1] == b ? 0 : 1;
        c->prows[e] = o; c->pkeys[e] = k;
        xors.insert(((uint64_t)(g.from[a] ^ g.to[a]) << 32) | (uint64_t)(g.from[b] ^ g.to[b]));
    }
    c->pstats.key_collisions = E - xors.size();
    return SAGE2OV_OK;
}
}  // namespace
int sage2ov_path_supports(sage2ov_ctx* c) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = readmap_check(c, "sage2ov_path_supports"); if (rc) return rc; }
    { const int rc = estimate_ensure(c); if (rc) return rc; }
    c->paths_forget(); c->pstats = sage2ov_path_stats{};
    PathParams P; P.bound = c->maxUpper; P.libraries = c->mateLibraries;
    for (int lib = 1; lib <= (int)c->mateLibraries && lib < 128; lib++) { const sage2ov_insert& I = c->inserts[lib]; P.valid[lib] = I.valid ? 1 : 0; P.lower[lib] = I.lower; P.upper[lib] = I.upper; }
    PathStats s; const int rc = dev_paths_build(c->device(), P, &s, c->err); if (rc) return rc;
    sage2ov_path_stats& o = c->pstats;
    o.claimed_reads = s.claimed_reads; o.claiming_nodes = s.claiming_nodes; o.start_nodes = s.start_nodes; o.paths = s.paths; o.capped_nodes = s.capped_nodes;
    o.eligible_entries = s.eligible; o.voting_entries = s.voting; o.records = s.records; o.rows = s.rows; o.mirrored = s.mirrored; o.sort_passes = s.passes;
    o.claim_ms = s.claim_ms; o.starts_ms = s.starts_ms; o.walk_ms = s.walk_ms; o.vote_ms = s.vote_ms; o.sort_ms = s.sort_ms; o.reduce_ms = s.reduce_ms;
    { const int rc2 = paths_fetch(c); if (rc2) return rc2; }
    c->pathValid = true;
    return SAGE2OV_OK;
}
int sage2ov_path_supports_count(sage2ov_ctx* c, uint32_t min_support, uint64_t* n) {
    if (!c || !n) return SAGE2OV_ERR_ARG;
    { const int rc = paths_ensure(c, "sage2ov_path_supports_count"); if (rc) return rc; }
    uint64_t m = 0; for (const sage2ov_path_support& e : c->prows) m += e.support >= min_support;
    *n = m; return SAGE2OV_OK;
}
int sage2ov_path_supports_export(sage2ov_ctx* c, uint32_t min_support, sage2ov_path_support* out, uint64_t cap) {
    if (!c) return SAGE2OV_ERR_ARG;
    uint64_t m = 0; { const int rc = sage2ov_path_supports_count(c, min_support, &m); if (rc) return rc; }
    if (cap < m) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_path_supports_export: the buffer holds fewer rows than the table (sage2ov_path_supports_count)");
    if (m && !out) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_path_supports_export: null argument");
    uint64_t at = 0; for (const sage2ov_path_support& e : c->prows) if (e.support >= min_support) out[at++] = e;
    return SAGE2OV_OK;
}
int sage2ov_path_stats_get(const sage2ov_ctx* c, sage2ov_path_stats* o) { if (!c || !o) return SAGE2OV_ERR_ARG; *o = c->pstats; return SAGE2OV_OK; }
int sage2ov_extend_paths_round(sage2ov_ctx* c, int highTh, int lowTh, int variant, uint64_t* merged) {              // :794-952, :2388-2546
    if (!c) return SAGE2OV_ERR_ARG;
    if (variant != 0 && variant != 1) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_extend_paths_round: variant is 0 (mergeByPathSupports) or 1 (mergeByPathSupportsNew)");
    { const int rc = readmap_check(c, "sage2ov_extend_paths_round"); if (rc) return rc; }
    sage2ov_extend_counts R{};
    const bool swept = !(c->pathValid && c->estimated && c->rmValid);
    { const int rc = paths_ensure(c, "sage2ov_extend_paths_round"); if (rc) return rc; }
    if (swept) R.sweep_ms = c->pstats.claim_ms + c->pstats.starts_ms + c->pstats.walk_ms + c->pstats.vote_ms + c->pstats.sort_ms + c->pstats.reduce_ms;
    { const int rc = pair_ordinals(c); if (rc) return rc; }                           // (the half-edge fields come with it; no read list)
    const std::vector<uint64_t> keys = c->pkeys; std::vector<uint32_t> sup(keys.size());
    for (size_t e = 0; e < keys.size(); e++) sup[e] = c->prows[e].support;
    SpliceRound S(c, "sage2ov_extend_paths_round", 1);
    const std::vector<uint32_t>&ordBefore = S.ordBefore, &from = S.from, &to = S.to; const std::vector<uint8_t>&type = S.type, &alive = S.alive; const std::vector<float>& flow = S.flow;
    NodeLists lists(S, c->g4.N);
    // SEARCH holds the summed support of the rows that share a key; every row is filed under its four end nodes.  ORDER: support descending, ties in table order
    struct Row { uint32_t a, b, sup; };
    std::vector<Row> rows(keys.size());
    for (size_t e = 0; e < keys.size(); e++) {
        rows[e] = Row{(uint32_t)(keys[e] >> 32), (uint32_t)keys[e], sup[e]};
        const uint64_t kk = S.key(rows[e].a, rows[e].b);
        S.search[kk] += sup[e];
        for (uint32_t nd : {to[rows[e].a], from[rows[e].a], to[rows[e].b], from[rows[e].b]}) S.filed.insert({nd, kk});
    }
    std::stable_sort(rows.begin(), rows.end(), [](const Row& x, const Row& y) { return x.sup > y.sup; });
    R.entries = rows.size(); bool dependent = false;
    {   // difference 1: no decision depends on the order when the rows at the threshold sit at pairwise different nodes, none of them an end of another such row's halves
        std::unordered_map<uint32_t, uint32_t> at; std::vector<const Row*> top;
        for (const Row& r : rows) if ((int64_t)r.sup >= (int64_t)highTh) { R.at_threshold++; top.push_back(&r); at[to[r.a]]++; }
        for (const Row* r : top) {
            if (at[to[r->a]] > 1) dependent = true;
            for (uint32_t nd : {from[r->a], to[r->b]}) if (nd != to[r->a] && at.count(nd)) dependent = true;
        }
    }
    std::unordered_set<uint32_t> blocked; std::vector<sage2ov_merge> merges;
    for (const Row& r : rows) {
        const uint32_t e1 = r.a, e2 = r.b;
        if (!alive[e1] || !alive[e2]) continue;
        if (S.find(S.key(e1, e2)) < 0) continue;
        const uint32_t node = to[e1];
        if (blocked.count(node)) { R.blocked++; continue; }
        if ((int64_t)r.sup < (int64_t)highTh) continue;                                // (:831: no stop)
        bool uniqueIn = true, uniqueOut = true;
        lists.walk(node, [&](uint32_t v) {
            if (!(flow[v] >= 1.f) || to[v] == from[v]) return;                         // :837 (no list is asked for)
            if ((v ^ 1u) != e1 && combined_type(type[v ^ 1u], type[e2]) >= 0) {
                int64_t s = S.find(S.key(v ^ 1u, e2)); if (s < 0) s = S.find(S.key(e2 ^ 1u, v)); if (s > lowTh) uniqueIn = false;
            }
            if (v != e2 && combined_type(type[e1], type[v]) >= 0) {
                int64_t s = S.find(S.key(e1, v)); if (s < 0) s = S.find(S.key(v ^ 1u, e1 ^ 1u)); if (s > lowTh) uniqueOut = false;
            }
        });
        if (variant == 0 ? !(uniqueIn && uniqueOut) : !(uniqueIn || uniqueOut)) { R.refused++; continue; }
        lists.walk(node, [&](uint32_t v) { if (to[v] != from[v]) blocked.insert(to[v]); });
        const int t = combined_type(type[e1], type[e2]);
        if (e1 == e2 || e1 == (e2 ^ 1u) || t < 0) continue;                            // mergeEdgesAndUpdate returns NULL
        { const int rc = S.make_room(e1, e2); if (rc) return rc; }
        const float f1 = flow[e1], f2 = flow[e2], f = (f1 == 0.f && f2 == 0.f) ? 0.f : 1.f;
        sage2ov_merge m{}; m.node = node; m.from = from[e1]; m.to = to[e2]; m.support = r.sup; m.flow = f; m.type = (uint8_t)t;
        m.pair_in = (e1 >> 1) < ordBefore.size() ? ordBefore[e1 >> 1] : ~0u; m.pair_out = (e2 >> 1) < ordBefore.size() ? ordBefore[e2 >> 1] : ~0u; m.pair_new = ~0u;
        m.in_deleted = f1 <= f; m.out_deleted = f2 <= f;
        const uint32_t h = S.splice(e1, e2, (uint8_t)t, f, m.in_deleted, m.out_deleted, 0);
        lists.added[from[h]].push_back(h); lists.added[from[h + 1]].push_back(h + 1);
        merges.push_back(m);
        S.erase_at(node, 0);
    }
    { const int rc = S.finish(merges, R); if (rc) return rc; }
    R.merges = merges.size();
    c->xmerges = std::move(merges);
    c->xstats.rounds++; c->xstats.last = R; counts_add(c->xstats.total, R);
    c->pstats.order_dependent = dependent ? 1 : 0;
    if (merged) *merged = R.merges;
    return SAGE2OV_OK;
}
int sage2ov_extend_by_paths(sage2ov_ctx* c, uint64_t genomeSize, int variant, uint64_t* rounds, uint64_t* merged) {   // :62-99
    if (!c) return SAGE2OV_ERR_ARG;
    if (variant != 0 && variant != 1) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_extend_by_paths: variant is 0 (findPathSupports) or 1 (findPathSupportsNew)");
    { const int rc = readmap_check(c, "sage2ov_extend_by_paths"); if (rc) return rc; }
    { const int rc = header_hold(c); if (rc) return rc; }
    const uint64_t gs = genomeSize ? genomeSize : c->hdrGenome, reads = c->hdrReads, arl = average_read_length(c);
    if (!gs || !arl) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_extend_by_paths: a genome size or an average read length of 0");
    const uint64_t stop = gs > 1000000000 ? 10 : 0;
    uint64_t r = 0, total = 0;
    for (uint32_t it = 1; it <= 10000; it++) {
        int high = 0; sage2ov_extend_threshold(reads, arl, gs, it, &high);
        uint64_t m = 0; { const int rc = sage2ov_extend_paths_round(c, high, 1, variant, &m); if (rc) return rc; }
        r++; total += m;
        if (rounds) *rounds = r; if (merged) *merged = total;
        if (m <= stop) return SAGE2OV_OK;
    }
    return c->fail(SAGE2OV_ERR_INTERNAL, "sage2ov_extend_by_paths: 10 000 rounds without a fixed point");
}

// ---- the sweep that opens ScaffoldMaker::mergeFinal / mergeFinalSmall (scaffolding.cpp:786-935, :981-1130); the semantics are stated in sage2ov.h
namespace {
static_assert(sizeof(sage2ov_link) == 44, "sage2ov_link is ten 32-bit words and four bytes");
int links_ensure(sage2ov_ctx* c, const char* who) {
    { const int rc = readmap_check(c, who); if (rc) return rc; }
    if (c->linkValid && c->estimated && c->rmValid) return SAGE2OV_OK;
    return sage2ov_links(c);
}
// the table in export order, on the host (once per table)
int links_fetch(sage2ov_ctx* c) {
    if (c->linkOnHost) return SAGE2OV_OK;
    Device* d = c->device(); const uint64_t E = dev_links_count(d);
    std::vector<uint64_t> key(E); std::vector<uint32_t> sup(E); std::vector<int32_t> gap(E), sum(E);
    { const int rc = dev_links_export(d, key.data(), sup.data(), gap.data(), sum.data(), c->err); if (rc) return rc; }
    { const int rc = pair_ordinals(c); if (rc) return rc; }
    const SimplifiedGraph& g = c->g4; const std::vector<uint32_t>& ord = c->pairOrdinal;
    std::vector<uint32_t> order, first(g.n_half_edges / 2 + 1, ~0u); g4_save_order(g, order);      // first[pair]: the half that opens the pair's record in the save (a loop: the first time)
    for (uint32_t h : order) if (first[h >> 1] == ~0u) first[h >> 1] = h;
    auto E_of = [&](uint32_t h) -> uint32_t { const uint32_t t = h ^ 1u; return g.from[h] < g.to[h] ? h : (g.from[h] > g.to[h] ? t : (h | 1u)); };      // a loop: the half with the higher index
    std::vector<uint64_t> at(E); for (uint64_t e = 0; e < E; e++) at[e] = e;
    std::vector<sage2ov_link> rows(E); std::vector<uint32_t> halves(2 * E);
    for (uint64_t e = 0; e < E; e++) {
        const uint32_t a = (uint32_t)(key[e] >> 32), b = (uint32_t)key[e], ea = E_of(a), eb = E_of(b);
        sage2ov_link o{}; o.pair_a = ord[a >> 1]; o.pair_b = ord[b >> 1]; o.from_a = g.from[a]; o.to_a = g.to[a]; o.from_b = g.from[b]; o.to_b = g.to[b];
        o.len_a = g.len[ea]; o.len_b = g.len[eb]; o.support = sup[e]; o.gap = gap[e];
        o.second_a = first[a >> 1] == a ? 0 : 1; o.second_b = first[b >> 1] == b ? 0 : 1; o.type_a = g.type[a]; o.type_b = g.type[b];
        rows[e] = o; halves[2 * e] = ea; halves[2 * e + 1] = eb;
    }
    std::sort(at.begin(), at.end(), [&](uint64_t x, uint64_t y) {
        const sage2ov_link &p = rows[x], &q = rows[y];
        if (p.pair_a != q.pair_a) return p.pair_a < q.pair_a;
        if (p.second_a != q.second_a) return p.second_a < q.second_a;
        if (p.pair_b != q.pair_b) return p.pair_b < q.pair_b;
        return p.second_b < q.second_b; });
    c->links.resize(E); c->linkHalves.resize(2 * E); c->linkSums.resize(E);
    for (uint64_t e = 0; e < E; e++) { c->links[e] = rows[at[e]]; c->linkHalves[2 * e] = halves[2 * at[e]]; c->linkHalves[2 * e + 1] = halves[2 * at[e] + 1]; c->linkSums[e] = sum[at[e]]; }
    c->linkOnHost = true;
    return SAGE2OV_OK;
}
// scaffolding.cpp:801 and :996 on row e, with the flows of the host copy as they are now
bool link_passes(const sage2ov_ctx* c, uint64_t e, uint32_t mode, int threshold) {
    if (mode == SAGE2OV_LINKS_ALL) return true;
    const sage2ov_link& r = c->links[e]; const int64_t len1 = r.len_a, len2 = r.len_b;
    if (mode == SAGE2OV_LINKS_SMALL) return len1 < 500 && len2 < 500;
    const std::vector<float>& f = c->g4.flow;
    const float f1 = f.empty() ? 0.f : f[c->linkHalves[2 * e]], f2 = f.empty() ? 0.f : f[c->linkHalves[2 * e + 1]];
    return (len1 > 200 && len2 > 200) || ((f1 > 0 && len1 > threshold) && (f2 > 0 && len2 > threshold));
}
// mergeContigs.cpp:1500 and :1587 on row e: both flows and lengths, no "> 200" alternative, and the raw gap sum
bool short_passes(const sage2ov_ctx* c, uint64_t e, int threshold) {
    const sage2ov_link& r = c->links[e]; const int64_t len1 = r.len_a, len2 = r.len_b;
    const std::vector<float>& f = c->g4.flow; if (f.empty()) return false;
    const float f1 = f[c->linkHalves[2 * e]], f2 = f[c->linkHalves[2 * e + 1]];
    return (f1 > 0 && len1 > threshold) && (f2 > 0 && len2 > threshold) && c->linkSums[e] <= 0;
}
}  // namespace
int sage2ov_links(sage2ov_ctx* c) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = readmap_check(c, "sage2ov_links"); if (rc) return rc; }
    { const int rc = estimate_ensure(c); if (rc) return rc; }
    c->links_forget();
    const int64_t arl = (int64_t)average_read_length(c), k = (int64_t)c->cfg.min_overlap;
    LinkParams P; P.bound = c->maxUpper; P.libraries = c->mateLibraries;
    for (int lib = 1; lib <= (int)c->mateLibraries && lib < 128; lib++) {
        P.thr[lib] = c->inserts[lib].valid ? c->inserts[lib].upper + k - 2 * arl : 0;
        P.gbase[lib] = (uint32_t)(uint64_t)(c->inserts[lib].mean - 2 * arl);
    }
    LinkStats s; const int rc = dev_links_build(c->device(), P, &s, c->err); if (rc) return rc;
    sage2ov_link_stats& o = c->lstats;
    o.halves = s.halves; o.entries_within = s.entries_within; o.unique_entries = s.unique_entries; o.mate_entries = s.mate_entries; o.records = s.records; o.keys = s.keys;
    o.sort_passes = s.passes; o.halves_ms = s.halves_ms; o.scan_ms = s.scan_ms; o.records_ms = s.records_ms; o.sort_ms = s.sort_ms; o.reduce_ms = s.reduce_ms;
    c->linkValid = true;
    return SAGE2OV_OK;
}
int sage2ov_links_count(sage2ov_ctx* c, uint32_t mode, uint32_t min_support, uint64_t* n) {
    if (!c || !n) return SAGE2OV_ERR_ARG;
    if (mode > SAGE2OV_LINKS_SMALL) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_links_count: mode is one of SAGE2OV_LINKS_ALL, _FINAL, _SMALL");
    { const int rc = links_ensure(c, "sage2ov_links_count"); if (rc) return rc; }
    { const int rc = links_fetch(c); if (rc) return rc; }
    const int thr = link_length_threshold(c);
    uint64_t m = 0; for (uint64_t e = 0; e < c->links.size(); e++) m += c->links[e].support >= min_support && link_passes(c, e, mode, thr);
    *n = m; return SAGE2OV_OK;
}
int sage2ov_links_export(sage2ov_ctx* c, uint32_t mode, uint32_t min_support, sage2ov_link* out, uint64_t cap) {
    if (!c) return SAGE2OV_ERR_ARG;
    uint64_t m = 0; { const int rc = sage2ov_links_count(c, mode, min_support, &m); if (rc) return rc; }
    if (cap < m) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_links_export: the buffer holds fewer rows than the table (sage2ov_links_count)");
    if (m && !out) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_links_export: null argument");
    const int thr = link_length_threshold(c);
    uint64_t at = 0; for (uint64_t e = 0; e < c->links.size(); e++) if (c->links[e].support >= min_support && link_passes(c, e, mode, thr)) out[at++] = c->links[e];
    return SAGE2OV_OK;
}
int sage2ov_links_gap_sums(sage2ov_ctx* c, uint32_t mode, uint32_t min_support, int32_t* out, uint64_t cap) {
    if (!c) return SAGE2OV_ERR_ARG;
    uint64_t m = 0; { const int rc = sage2ov_links_count(c, mode, min_support, &m); if (rc) return rc; }
    if (cap < m) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_links_gap_sums: the buffer holds fewer rows than the table (sage2ov_links_count)");
    if (m && !out) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_links_gap_sums: null argument");
    const int thr = link_length_threshold(c);
    uint64_t at = 0; for (uint64_t e = 0; e < c->links.size(); e++) if (c->links[e].support >= min_support && link_passes(c, e, mode, thr)) out[at++] = c->linkSums[e];
    return SAGE2OV_OK;
}
int sage2ov_link_stats_get(const sage2ov_ctx* c, sage2ov_link_stats* o) { if (!c || !o) return SAGE2OV_ERR_ARG; *o = c->lstats; return SAGE2OV_OK; }

// ---- step 7: ScaffoldMaker::makeScaffolds (scaffolding.cpp:31-98, :281-482, :488-769); the semantics are stated in sage2ov.h
namespace {
static_assert(sizeof(sage2ov_join) == 48 && sizeof(sage2ov_scaffold_counts) == 144 && sizeof(sage2ov_scaffold_stats) == 304, "the records of the scaffold rounds");
void sc_counts_add(sage2ov_scaffold_counts& t, const sage2ov_scaffold_counts& r) {
    t.rows += r.rows; t.below_threshold += r.below_threshold; t.skipped += r.skipped; t.blocked += r.blocked; t.cycles += r.cycles; t.merged += r.merged; t.batches += r.batches;
    t.overlaps += r.overlaps; t.concatenated += r.concatenated; t.gapped += r.gapped; t.outside_reference += r.outside_reference; t.entries_copied += r.entries_copied;
    t.pairs_deleted += r.pairs_deleted; t.sweep_ms += r.sweep_ms; t.select_ms += r.select_ms; t.overlap_ms += r.overlap_ms; t.lists_ms += r.lists_ms; t.commit_ms += r.commit_ms;
}
// the checks of the two join entry points on internal half-edges: lengths within 32 bits (the longest read has 1018 bases)
bool join_length_fits(uint32_t lenA, uint32_t lenATwin, uint32_t lenB, uint32_t lenBTwin, int32_t gap) {
    const uint64_t add = (uint64_t)std::max<int32_t>(gap, 0) + 2048;
    return (uint64_t)lenA + lenB + add < (1ull << 32) && (uint64_t)lenATwin + lenBTwin + add < (1ull << 32);
}
}  // namespace
int sage2ov_graph_join_pairs(sage2ov_ctx* c, const uint32_t* pf, const uint8_t* fr, const uint32_t* ps, const uint8_t* sr, const int32_t* gap, uint64_t n, int32_t* overlap, uint8_t* how) {
    if (!c) return SAGE2OV_ERR_ARG;
    if (n && (!pf || !fr || !ps || !sr || !gap)) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_graph_join_pairs: null argument");
    { const int rc = readmap_check(c, "sage2ov_graph_join_pairs"); if (rc) return rc; }
    if (n >= (1ull << 30)) return c->fail(SAGE2OV_ERR_LIMIT, "sage2ov_graph_join_pairs: more joins than there can be pairs");
    SpliceBatch B;
    { const int rc = splice_operands(c, "sage2ov_graph_join_pairs", pf, fr, ps, sr, n, true, B); if (rc) return rc; }
    const SimplifiedGraph& g = c->g4; B.gap.assign(gap, gap + n);
    for (uint64_t i = 0; i < n; i++) { const uint32_t a = B.a[i], b = B.b[i];
        if (!join_length_fits(g.len[a], g.len[a ^ 1u], g.len[b], g.len[b ^ 1u], gap[i])) return c->fail(SAGE2OV_ERR_LIMIT, "sage2ov_graph_join_pairs: an edge length beyond 32 bits"); }
    { const int rc = splice_apply(c, B, 0); if (rc) return rc; }
    for (uint64_t i = 0; i < n; i++) {
        if (overlap) { overlap[2 * i] = B.ov[2 * i]; overlap[2 * i + 1] = B.ov[2 * i + 1]; }
        if (how) { how[2 * i] = B.plan[i].how[0]; how[2 * i + 1] = B.plan[i].how[1]; }
    }
    return SAGE2OV_OK;
}
int sage2ov_scaffold_threshold(uint64_t reads, uint64_t arl, uint64_t genomeSize, uint32_t loop, uint32_t iteration, int* high) {      // scaffolding.cpp:38-94
    if (!high || !arl || !genomeSize || !iteration || loop < 1 || loop > 5) return SAGE2OV_ERR_ARG;
    const float coverage = (reads * arl) / genomeSize;
    if (loop <= 2) *high = (int)ceilf(((iteration > 5 ? 0.05 : 0.10) * coverage) * (100.0 / arl));
    else *high = loop == 3 ? 2 : 1;
    return SAGE2OV_OK;
}
namespace {
// one round of joins on the link table: the selection of mergeAccordingToSupport / mergeAccordingToSupport2 (scaffolding.cpp:488-769) and of mergeShortOverlap
// (mergeContigs.cpp:1788-1908) differ in three things: which rows of the table are ROWS (filter: the row's index in export order), how many rivals at or above
// highTh each side may have (limit), and whether a rival counted on both sides makes the row a CYCLE (cycleTest).  The round's records go to `stats` and `out`.
int join_round(sage2ov_ctx* c, const char* who, int highTh, const std::function<bool(uint64_t)>& filter, uint64_t limit, bool cycleTest, sage2ov_scaffold_stats& stats, std::vector<sage2ov_join>& out, uint64_t* merged) {
    { const int rc = readmap_check(c, who); if (rc) return rc; }
    sage2ov_scaffold_counts R{};
    const bool swept = !(c->linkValid && c->estimated && c->rmValid);
    { const int rc = links_ensure(c, who); if (rc) return rc; }
    { const int rc = links_fetch(c); if (rc) return rc; }                             // (pair_ordinals and the half-edge fields come with it; no read list)
    if (swept) R.sweep_ms = c->lstats.halves_ms + c->lstats.scan_ms + c->lstats.records_ms + c->lstats.sort_ms + c->lstats.reduce_ms;
    SpliceRound S(c, who, 0);
    const std::vector<uint32_t>&ordBefore = S.ordBefore, &from = S.from, &to = S.to, &len = S.len; const std::vector<uint8_t>&type = S.type, &alive = S.alive; const std::vector<float>& flow = S.flow;
    std::vector<uint32_t> firstOf; g4_save_order(c->g4, firstOf);                      // ordinal -> the half that opens the record pair
    auto isE = [&](uint32_t h) -> bool { return from[h] < to[h] || (from[h] == to[h] && (h & 1u)); };      // the half the read-to-edge table names; a loop: the higher index
    // the rows by rule (a) in export order, FEASIBLE from the unfiltered table, SEARCH and the rows filed under their end nodes
    struct Row { uint32_t e1, e2, sup; int32_t gap; uint64_t lenSum; };
    std::vector<Row> rows; std::unordered_map<uint32_t, std::vector<uint32_t>> feasible;
    for (uint64_t e = 0; e < c->links.size(); e++) {
        const sage2ov_link& L = c->links[e]; if (!L.support) continue;
        const uint32_t a = firstOf[L.pair_a] ^ L.second_a, b = firstOf[L.pair_b] ^ L.second_b;
        auto& fa = feasible[a >> 1]; if (std::find(fa.begin(), fa.end(), b >> 1) == fa.end()) fa.push_back(b >> 1);
        auto& fb = feasible[b >> 1]; if (std::find(fb.begin(), fb.end(), a >> 1) == fb.end()) fb.push_back(a >> 1);
        if (a < b && filter(e)) rows.push_back(Row{a ^ 1u, b, L.support, L.gap, (uint64_t)len[a ^ 1u] + len[b]});
    }
    auto xk = [&](uint32_t h) -> uint64_t { return S.xk(h); };
    auto k2 = [&](uint64_t x, uint64_t y) -> uint64_t { return SpliceRound::k2(x, y); };
    for (const Row& r : rows) S.insert(r.e1, r.e2, r.sup);
    std::stable_sort(rows.begin(), rows.end(), [](const Row& x, const Row& y) { return x.sup != y.sup ? x.sup > y.sup : x.lenSum > y.lenSum; });
    R.rows = rows.size();
    auto present = [&](uint64_t x, uint64_t y) -> int64_t { const int64_t s = S.find(k2(x, y)); return s < 0 ? S.find(k2(y, x)) : s; };      // in either order; -1: in neither
    auto lookup = [&](uint64_t x, uint64_t y) -> int64_t { return std::max<int64_t>(present(x, y), 0); };
    std::unordered_set<uint32_t> spent; std::vector<sage2ov_join> joins;
    static const std::vector<uint32_t> none;
    for (const Row& r : rows) {
        const uint32_t e1 = r.e1, e2 = r.e2;
        if (!alive[e1] || !alive[e2]) { R.outside_reference = 1; R.skipped++; continue; }      // (d)
        if (S.find(k2(xk(e1), xk(e2))) < 0) { R.skipped++; continue; }
        if ((int64_t)r.sup < (int64_t)highTh) { R.below_threshold++; continue; }
        const uint32_t p1 = e1 >> 1, p2 = e2 >> 1;
        auto feas = [&](uint32_t p) -> const std::vector<uint32_t>& { if (spent.count(p)) return none; auto it = feasible.find(p); return it == feasible.end() ? none : it->second; };
        uint64_t count1 = 0, count2 = 0; bool cycle = false; std::vector<uint32_t> side2;
        for (uint32_t q : feas(p1)) {
            if (spent.count(q) || (q == p2 && isE(e2))) continue;
            if (lookup(xk(e1), xk(2 * q)) >= (int64_t)highTh) { count2++; side2.push_back(q); }
        }
        for (uint32_t q : feas(p2)) {
            if (spent.count(q) || (q == p1 && isE(e1))) continue;
            const int64_t s = present(xk(2 * q), xk(e2));
            if (s >= 0 && s >= (int64_t)highTh) { count1++; if (std::find(side2.begin(), side2.end(), q) != side2.end()) cycle = true; }
        }
        if (cycle && cycleTest) { R.cycles++; continue; }
        if (count1 > limit || count2 > limit) { R.blocked++; continue; }
        { const int rc = S.make_room(e1, e2); if (rc) return rc; }                     // (e): only a kept operand can be named again, the rows are older than the round's edges
        if (!join_length_fits(len[e1], len[e1 ^ 1u], len[e2], len[e2 ^ 1u], r.gap)) return c->fail(SAGE2OV_ERR_LIMIT, std::string(who) + ": an edge length beyond 32 bits");
        const uint32_t t1 = type[e1], t2 = type[e2], t = ((t1 == 2 || t1 == 3) ? 2u : 0u) | ((t2 == 1 || t2 == 3) ? 1u : 0u), node = to[e1];
        sage2ov_join m{}; m.from = from[e1]; m.to = to[e2]; m.support = r.sup; m.gap = r.gap; m.type = (uint8_t)t;
        m.pair_first = ordBefore[p1]; m.pair_second = ordBefore[p2]; m.pair_new = ~0u;
        m.first_deleted = flow[e1] <= 1.0f; m.second_deleted = flow[e2] <= 1.0f;
        const uint64_t own = k2(xk(e1), xk(e2));
        S.splice(e1, e2, (uint8_t)t, 1.0f, m.first_deleted, m.second_deleted, r.gap);
        spent.insert(p1); spent.insert(p2);
        joins.push_back(m);
        if (S.erase_at(node, own) && m.first_deleted) R.outside_reference = 1;        // (d): the reference reads the erase key from the freed edge_1 (:607)
    }
    { const int rc = S.finish(joins, R); if (rc) return rc; }
    for (size_t i = 0; i < joins.size(); i++) {
        sage2ov_join& j = joins[i]; const SplicePlan& p = S.plans[i];
        j.overlap_forward = S.ov[2 * i]; j.overlap_twin = S.ov[2 * i + 1]; j.how_forward = p.how[0]; j.how_twin = p.how[1];
    }
    R.merged = joins.size(); R.overlaps = S.sum.overlaps; R.concatenated = S.sum.concatenated; R.gapped = S.sum.gapped; R.overlap_ms = S.sum.overlap_ms;
    out = std::move(joins);
    stats.rounds++; stats.last = R; sc_counts_add(stats.total, R);
    if (merged) *merged = R.merged;
    return SAGE2OV_OK;
}
}  // namespace
int sage2ov_scaffold_round(sage2ov_ctx* c, int highTh, int flag, int small, uint64_t* merged) {                        // :774-967, :488-769
    if (!c) return SAGE2OV_ERR_ARG;
    if (flag != 1 && flag != 2) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_scaffold_round: flag is 1 or 2");
    const int thr = link_length_threshold(c);
    const uint32_t mode = small ? SAGE2OV_LINKS_SMALL : SAGE2OV_LINKS_FINAL;
    return join_round(c, "sage2ov_scaffold_round", highTh, [&](uint64_t e) { return link_passes(c, e, mode, thr); }, flag == 1 ? 1 : 2, true, c->scstats, c->scjoins, merged);
}
int sage2ov_scaffold(sage2ov_ctx* c, uint64_t genomeSize, uint64_t* rounds, uint64_t* merged) {                       // :31-98
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = readmap_check(c, "sage2ov_scaffold"); if (rc) return rc; }
    { const int rc = header_hold(c); if (rc) return rc; }
    const uint64_t gs = genomeSize ? genomeSize : c->hdrGenome, reads = c->hdrReads, arl = average_read_length(c);
    if (!gs || !arl) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_scaffold: a genome size or an average read length of 0");
    uint64_t r = 0, total = 0;
    int low = 0; sage2ov_scaffold_threshold(reads, arl, gs, 1, 6, &low);
    for (uint32_t loop = 1; loop <= 5; loop++)
        for (uint32_t it = 1;; it++) {
            if (r >= 10000) return c->fail(SAGE2OV_ERR_INTERNAL, "sage2ov_scaffold: 10 000 rounds without a fixed point");
            int high = 0; sage2ov_scaffold_threshold(reads, arl, gs, loop, it, &high);
            uint64_t m = 0; { const int rc = sage2ov_scaffold_round(c, high, (loop == 2 || loop == 5) ? 2 : 1, loop == 5, &m); if (rc) return rc; }
            r++; total += m;
            if (rounds) *rounds = r; if (merged) *merged = total;
            if (!m && (loop > 2 || high == low)) break;
        }
    return SAGE2OV_OK;
}
int sage2ov_scaffold_merges_count(const sage2ov_ctx* c, uint64_t* n) { if (!c || !n) return SAGE2OV_ERR_ARG; *n = c->scjoins.size(); return SAGE2OV_OK; }
int sage2ov_scaffold_merges_export(const sage2ov_ctx* c, sage2ov_join* out, uint64_t cap) {
    if (!c || cap < c->scjoins.size() || (!out && !c->scjoins.empty())) return SAGE2OV_ERR_ARG;
    if (!c->scjoins.empty()) memcpy(out, c->scjoins.data(), c->scjoins.size() * sizeof(sage2ov_join));
    return SAGE2OV_OK;
}
int sage2ov_scaffold_stats_get(const sage2ov_ctx* c, sage2ov_scaffold_stats* o) { if (!c || !o) return SAGE2OV_ERR_ARG; *o = c->scstats; return SAGE2OV_OK; }

// ---- the fourth loop of ContigExtender::extendContigs: mergeShortOverlaps (mergeContigs.cpp:101-110, :1474-1648, :1788-1908); the semantics are stated in sage2ov.h
int sage2ov_extend_short_threshold(uint64_t reads, uint64_t arl, uint64_t genomeSize, int* high) {                     // :43, :102
    if (!high || !arl || !genomeSize) return SAGE2OV_ERR_ARG;
    const float coverage = (reads * arl) / genomeSize;
    *high = (int)ceilf((0.05 * coverage) * (100.0 / arl));
    return SAGE2OV_OK;
}
int sage2ov_extend_short_round(sage2ov_ctx* c, int highTh, uint64_t* merged) {                                         // :1474-1648, :1788-1908
    if (!c) return SAGE2OV_ERR_ARG;
    const int thr = link_length_threshold(c);                                          // (mergeContigs.cpp:21 is scaffolding.cpp:20)
    return join_round(c, "sage2ov_extend_short_round", highTh, [&](uint64_t e) { return short_passes(c, e, thr); }, 0, false, c->sostats, c->sojoins, merged);
}
int sage2ov_extend_by_short_overlaps(sage2ov_ctx* c, uint64_t genomeSize, uint64_t* rounds, uint64_t* merged) {        // :101-110
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = readmap_check(c, "sage2ov_extend_by_short_overlaps"); if (rc) return rc; }
    { const int rc = header_hold(c); if (rc) return rc; }
    const uint64_t gs = genomeSize ? genomeSize : c->hdrGenome, reads = c->hdrReads, arl = average_read_length(c);
    if (!gs || !arl) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_extend_by_short_overlaps: a genome size or an average read length of 0");
    int high = 0; sage2ov_extend_short_threshold(reads, arl, gs, &high);
    uint64_t r = 0, total = 0;
    for (uint32_t it = 1; it <= 10000; it++) {
        uint64_t m = 0; { const int rc = sage2ov_extend_short_round(c, high, &m); if (rc) return rc; }
        r++; total += m;
        if (rounds) *rounds = r; if (merged) *merged = total;
        if (!m) return SAGE2OV_OK;
    }
    return c->fail(SAGE2OV_ERR_INTERNAL, "sage2ov_extend_by_short_overlaps: 10 000 rounds without a fixed point");
}
int sage2ov_extend_contigs(sage2ov_ctx* c, uint64_t genomeSize, uint64_t rounds[4], uint64_t merged[4]) {              // :37-113
    if (!c) return SAGE2OV_ERR_ARG;
    uint64_t r[4] = {0, 0, 0, 0}, m[4] = {0, 0, 0, 0};
    int rc = sage2ov_extend_by_supports(c, genomeSize, &r[0], &m[0]);
    if (!rc) rc = sage2ov_extend_by_paths(c, genomeSize, 0, &r[1], &m[1]);
    if (!rc) rc = sage2ov_extend_by_paths(c, genomeSize, 1, &r[2], &m[2]);
    if (!rc) rc = sage2ov_extend_by_short_overlaps(c, genomeSize, &r[3], &m[3]);
    for (int i = 0; i < 4; i++) { if (rounds) rounds[i] = r[i]; if (merged) merged[i] = m[i]; }
    return rc;
}
int sage2ov_extend_short_merges_count(const sage2ov_ctx* c, uint64_t* n) { if (!c || !n) return SAGE2OV_ERR_ARG; *n = c->sojoins.size(); return SAGE2OV_OK; }
int sage2ov_extend_short_merges_export(const sage2ov_ctx* c, sage2ov_join* out, uint64_t cap) {
    if (!c || cap < c->sojoins.size() || (!out && !c->sojoins.empty())) return SAGE2OV_ERR_ARG;
    if (!c->sojoins.empty()) memcpy(out, c->sojoins.data(), c->sojoins.size() * sizeof(sage2ov_join));
    return SAGE2OV_OK;
}
int sage2ov_extend_short_stats_get(const sage2ov_ctx* c, sage2ov_scaffold_stats* o) { if (!c || !o) return SAGE2OV_ERR_ARG; *o = c->sostats; return SAGE2OV_OK; }

// ---- OverlapGraph::printGraph / saveContigsToFile (overlapGraph.cpp:507-784); the semantics are stated in sage2ov.h
namespace {
static_assert(sizeof(sage2ov_contig) == 48, "sage2ov_contig is 48 bytes");
constexpr uint32_t CONTIG_WRAPPED = 2;                                                // ContigRow::flags
int contigs_ensure(sage2ov_ctx* c, const char* who) {
    { const int rc = readmap_check(c, who); if (rc) return rc; }
    return c->ctgValid ? SAGE2OV_OK : sage2ov_contigs_build(c, c->ctgThreshold, c->ctgGenome);
}
bool contig_written(const sage2ov_ctx* c, const ContigRow& r) { return !(r.flags & CONTIG_WRAPPED) && r.contig_length >= c->ctgThresholdUsed; }
// the bound of one range of sage2ov_contigs_save in 16-byte chunks (SAGE2OV_TEST_CONTIG_RANGE=<bytes>: lowered, so that the tests' few kilobases make many ranges)
uint64_t contig_range_chunks(const sage2ov_ctx* c) {
    const long long v = c->opt.num("SAGE2OV_TEST_CONTIG_RANGE", (long long)SAGE2OV_CONTIG_RANGE_BYTES);
    return std::max<uint64_t>(1, (uint64_t)std::max<long long>(16, std::min<long long>(v, (long long)SAGE2OV_CONTIG_RANGE_BYTES)) / 16);
}
// one FASTA record (overlapGraph.cpp:730-741): ordinal from 1, the running counters as they stand after this row
void contig_record(const sage2ov_ctx* c, uint64_t ordinal, const ContigRow& r, const char* str, bool scaffold, uint64_t gaps, uint64_t ns, std::string& o) {
    const SimplifiedGraph& g = c->g4; char buf[256];
    const float flow = g.flow.empty() ? 0.f : g.flow[r.h];
    const int n = snprintf(buf, sizeof buf, ">%s_%llu flow=%g Edge length=%u String length: %u e(%u, %u) gapCount=%llu nCount=%llu\n", scaffold ? "scaffold" : "contig", (unsigned long long)ordinal,
                           (double)flow, r.contig_length, r.string_length, g.from[r.h], g.to[r.h], (unsigned long long)gaps, (unsigned long long)ns);
    o.append(buf, (size_t)n);
    for (uint64_t at = r.start, left = r.contig_length; left > 0;) {                   // substr(startIndex, 60) cuts at the string's end
        const uint64_t want = std::min<uint64_t>(60, left), have = at < r.string_length ? std::min<uint64_t>(want, r.string_length - at) : 0;
        o.append(str + at, (size_t)have); o.push_back('\n'); at += want; left -= want;
    }
}
}  // namespace
int sage2ov_contigs_build(sage2ov_ctx* c, uint32_t threshold, uint64_t genome_size) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = readmap_check(c, "sage2ov_contigs_build"); if (rc) return rc; }
    c->contigs_forget(); c->ctgThreshold = threshold; c->ctgGenome = genome_size;
    const uint32_t thr = threshold ? threshold : (uint32_t)(int)ceilf((float)(100 * ((double)average_read_length(c) / 100.0)));      // overlapGraph.cpp:32
    c->ctgThresholdUsed = thr;
    ContigBuildStats bs; { const int rc = dev_contigs_build(c->device(), thr, c->ctgRows, &bs, c->err); if (rc) { c->ctgRows.clear(); return rc; } }
    { const int rc = pair_ordinals(c); if (rc) return rc; }                            // (the graph on the host: ends, lengths, types and flows of the rows)
    const SimplifiedGraph& g = c->g4; const std::vector<ContigRow>& rows = c->ctgRows;
    c->ctgChunk.assign(rows.size() + 1, 0);
    sage2ov_contig_stats& s = c->cstats; s = sage2ov_contig_stats{};
    s.select_ms = bs.select_ms; s.sort_ms = bs.sort_ms; s.layout_ms = bs.layout_ms;
    uint64_t nx = 0;
    for (size_t i = 0; i < rows.size(); i++) {
        const ContigRow& r = rows[i];
        c->ctgChunk[i + 1] = c->ctgChunk[i] + (((uint64_t)r.string_length + 15) >> 4);
        s.covered += g.len[r.h]; s.gaps += r.gap_count; s.n_bases += r.n_count; s.inconsistent += r.flags & 1u; s.wrapped += (r.flags & CONTIG_WRAPPED) ? 1 : 0;
        if (contig_written(c, r)) { s.written++; s.bases += r.contig_length; }
        if (i == 0) s.longest = r.contig_length;
        nx += r.contig_length;                                                         // overlapGraph.cpp:745-755
        if (!s.n50_ordinal && nx >= genome_size / 2) { s.n50 = r.contig_length; s.n50_ordinal = i + 1; }
        if (!s.n90_ordinal && nx >= genome_size * 9 / 10) { s.n90 = r.contig_length; s.n90_ordinal = i + 1; }
    }
    s.contigs = rows.size();
    c->ctgValid = true;
    return SAGE2OV_OK;
}
int sage2ov_contigs_count(sage2ov_ctx* c, uint64_t* n, uint64_t* total) {
    if (!c || !n) return SAGE2OV_ERR_ARG;
    { const int rc = contigs_ensure(c, "sage2ov_contigs_count"); if (rc) return rc; }
    *n = c->ctgRows.size();
    if (total) { uint64_t t = 0; for (const ContigRow& r : c->ctgRows) t += r.string_length; *total = t; }
    return SAGE2OV_OK;
}
int sage2ov_contigs_export(sage2ov_ctx* c, sage2ov_contig* out, uint64_t cap) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = contigs_ensure(c, "sage2ov_contigs_export"); if (rc) return rc; }
    if (cap < c->ctgRows.size()) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_contigs_export: the buffer holds fewer rows than the table (sage2ov_contigs_count)");
    if (!c->ctgRows.empty() && !out) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_contigs_export: null argument");
    const SimplifiedGraph& g = c->g4;
    for (size_t i = 0; i < c->ctgRows.size(); i++) {
        const ContigRow& r = c->ctgRows[i]; sage2ov_contig o{};
        o.from = g.from[r.h]; o.to = g.to[r.h]; o.pair = c->pairOrdinal[r.h >> 1]; o.edge_length = g.len[r.h]; o.string_length = r.string_length; o.contig_length = r.contig_length;
        o.start = r.start; o.gap_count = r.gap_count; o.n_count = r.n_count; o.flow = g.flow.empty() ? 0.f : g.flow[r.h]; o.type = g.type[r.h];
        out[i] = o;
    }
    return SAGE2OV_OK;
}
int sage2ov_contigs_sequences(sage2ov_ctx* c, uint64_t first, uint64_t count, char* out, uint64_t cap, uint64_t* offsets) {
    if (!c) return SAGE2OV_ERR_ARG;
    { const int rc = contigs_ensure(c, "sage2ov_contigs_sequences"); if (rc) return rc; }
    const std::vector<ContigRow>& rows = c->ctgRows;
    if (first > rows.size() || count > rows.size() - first) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_contigs_sequences: the range lies outside the table (sage2ov_contigs_count)");
    uint64_t need = 0; for (uint64_t i = first; i < first + count; i++) need += rows[i].string_length;
    if (cap < need) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_contigs_sequences: the buffer is shorter than the strings of the range");
    if (!offsets || (need && !out)) return c->fail(SAGE2OV_ERR_ARG, "sage2ov_contigs_sequences: null argument");
    const uint64_t chunk0 = c->ctgChunk[first], nChunks = c->ctgChunk[first + count] - chunk0;
    const char* img = nullptr;
    if (count) {
        { const int rc = dev_contigs_spell_begin(c->device(), 0, first, count, chunk0, nChunks, c->err); if (rc) return rc; }
        { const int rc = dev_contigs_spell_wait(c->device(), 0, &img, &c->cstats.spell_ms, c->err); if (rc) return rc; }
    }
    uint64_t at = 0;
    for (uint64_t i = first; i < first + count; i++) {                                 // compact on the way out: in the device buffer every row begins at a 16-byte chunk
        offsets[i - first] = at; memcpy(out + at, img + 16 * (c->ctgChunk[i] - chunk0), rows[i].string_length); at += rows[i].string_length;
    }
    offsets[count] = at;
    return SAGE2OV_OK;
}
int sage2ov_contigs_save(sage2ov_ctx* c, const char* path, int is_scaffold) {
    if (!c || !path) return SAGE2OV_ERR_ARG;
    { const int rc = contigs_ensure(c, "sage2ov_contigs_save"); if (rc) return rc; }
    const std::vector<ContigRow>& rows = c->ctgRows; const std::vector<uint64_t>& ch = c->ctgChunk; const uint64_t R = rows.size(), bound = contig_range_chunks(c);
    FILE* f = fopen(path, "w"); if (!f) return c->fail(SAGE2OV_ERR_IO, std::string("cannot open ") + path);
    std::vector<char> io(1 << 22); setvbuf(f, io.data(), _IOFBF, io.size());
    // a range: rows [a, b) with at most `bound` chunks, at least one row
    auto range_end = [&](uint64_t a) { uint64_t b = a + 1; while (b < R && ch[b + 1] - ch[a] <= bound) b++; return std::min(b, R); };
    auto begin = [&](int which, uint64_t a, uint64_t b) { return dev_contigs_spell_begin(c->device(), which, a, b - a, ch[a], ch[b] - ch[a], c->err); };
    int rc = SAGE2OV_OK, which = 0; uint64_t a = 0, b = R ? range_end(0) : 0, gaps = 0, ns = 0; std::string text;
    if (R) rc = begin(0, a, b);
    while (!rc && a < R) {
        const uint64_t a2 = b, b2 = a2 < R ? range_end(a2) : a2;
        if (a2 < R) rc = begin(which ^ 1, a2, b2);                                      // the next range is spelled while this one is formatted
        const char* img = nullptr;
        if (!rc) rc = dev_contigs_spell_wait(c->device(), which, &img, &c->cstats.spell_ms, c->err);
        if (rc) break;
        text.clear();
        for (uint64_t i = a; i < b; i++) {
            gaps += rows[i].gap_count; ns += rows[i].n_count;                           // running totals over all rows, written or not (:668-669)
            if (contig_written(c, rows[i])) contig_record(c, i + 1, rows[i], img + 16 * (ch[i] - ch[a]), is_scaffold != 0, gaps, ns, text);
        }
        if (fwrite(text.data(), 1, text.size(), f) != text.size()) { rc = c->fail(SAGE2OV_ERR_IO, std::string("cannot write ") + path); break; }
        a = a2; b = b2; which ^= 1;
    }
    if (rc) { std::string e; dev_sync(c->device(), e); }                               // (a range may still be in flight)
    if (fclose(f) != 0 && !rc) rc = c->fail(SAGE2OV_ERR_IO, std::string("cannot write ") + path);
    return rc;
}
int sage2ov_contig_stats_get(const sage2ov_ctx* c, sage2ov_contig_stats* o) { if (!c || !o) return SAGE2OV_ERR_ARG; *o = c->cstats; return SAGE2OV_OK; }

int sage2ov_run_steps23(sage2ov_ctx* c) {
    if (!c) return SAGE2OV_ERR_ARG;
    auto t0 = std::chrono::steady_clock::now();
    if (c->device()) dev_reset_timings(c->device());
    int rc = sage2ov_index_build(c); if (rc) return rc;
    rc = sage2ov_overlap_initial(c); if (rc) return rc;
    rc = sage2ov_overlap_reduce(c); if (rc) return rc;
    rc = sage2ov_overlap_convert(c); if (rc) return rc;
    c->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SAGE2OV_OK;
}
int sage2ov_probe_run_stats_get(sage2ov_ctx* c, uint64_t out[4]) {
    if (!c || !out) return SAGE2OV_ERR_ARG;
    if (!c->device()) return c->fail(SAGE2OV_ERR_DEVICE, "no GPU context: the probe pass runs on the device only");
    return dev_probe_run_stats(c->device(), out, c->err);
}
int sage2ov_reduce_stats_get(sage2ov_ctx* c, uint64_t out[SAGE2OV_REDUCE_STATS]) {
    if (!c || !out) return SAGE2OV_ERR_ARG; if (!c->reduced) return c->fail(SAGE2OV_ERR_ARG, "run the reduce phase first");
    for (int x = 0; x < SAGE2OV_REDUCE_STATS; x++) out[x] = c->rstats[x];
    return SAGE2OV_OK;
}
int sage2ov_timings_reset(sage2ov_ctx* c) { if (!c) return SAGE2OV_ERR_ARG; if (c->device()) dev_reset_timings(c->device()); c->reduce_ms = 0; c->total_ms = 0; return SAGE2OV_OK; }
int sage2ov_timings_get(const sage2ov_ctx* c, sage2ov_timings* o) {
    if (!c || !o) return SAGE2OV_ERR_ARG;
    DevTimings t; if (c->device()) dev_timings(c->device(), &t);
    o->index_ms = t.index_ms; o->probe_ms = t.probe_ms; o->reciprocal_ms = t.reciprocal_ms; o->reduce_ms = c->reduce_ms; o->convert_ms = t.convert_ms;
    o->total_ms = c->total_ms; o->probe_kernel_ms = t.probe_kernel_ms; o->probe_kernel_launches = t.probe_launches; o->sequential_reads = t.slow_reads; o->organize_ms = t.organize_ms; o->probe_fast_launches = t.probe_fast_launches;
    o->reciprocal_cond_ms = t.recip_cond_ms; o->reduce_marks_ms = t.marks_ms;
    return SAGE2OV_OK;
}

}  // extern "C"
