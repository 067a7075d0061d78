// sage2_amd/csrc/sage2ov.hpp -- host-side C++ mirror of the four reference classes main.cpp:44-131 drives for
// steps 1-3, as thin wrappers over the C ABI (include/sage2ov.h).  Same names, argument meaning and call order as
// the reference (inputReader/readLoader.h:44-55, economyGraph/hashTable.h:34-43, economyGraph/economyGraph.h:43-53,
// overlapGraph/overlapGraph.h:54-67); errors become exceptions instead of exit() (utils.cpp:36).
#pragma once
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>
#include "sage2ov.h"

namespace sage2ov {

struct Error : std::runtime_error { int code; Error(int c, const std::string& m) : std::runtime_error(m), code(c) {} };

class Context {
public:
    explicit Context(uint16_t minOvlp, int device = SAGE2OV_DEVICE_CURRENT, unsigned hostThreads = 0, unsigned rank = 0, unsigned world = 1, unsigned flags = 0) {
        sage2ov_config cfg{}; cfg.min_overlap = minOvlp; cfg.device = device; cfg.rank = rank; cfg.world = world; cfg.host_threads = hostThreads; cfg.flags = flags;
        int rc = sage2ov_ctx_create(&cfg, &c_); if (rc) throw Error(rc, sage2ov_last_error(nullptr));
    }
    ~Context() { sage2ov_ctx_destroy(c_); }
    Context(const Context&) = delete; Context& operator=(const Context&) = delete;
    sage2ov_ctx* get() const { return c_; }
    void check(int rc) const { if (rc) throw Error(rc, sage2ov_last_error(c_)); }
private:
    sage2ov_ctx* c_ = nullptr;
};

// ReadLoader (readLoader.h:44-55)
class ReadLoader {
public:
    uint64_t numberOfUniqueReads = 0, numberOfReads = 0, totalBP = 0, averageReadLength = 0;
    explicit ReadLoader(Context& ctx) : ctx_(ctx) {}
    void loadFromList(const std::string& listPath) { ctx_.check(sage2ov_reads_add_list(ctx_.get(), listPath.c_str())); }
    void readDatasetInBytes(const std::string& mateFile1, const std::string& mateFile2 = "") {
        ctx_.check(sage2ov_reads_add_file(ctx_.get(), mateFile1.c_str(), mateFile2.empty() ? nullptr : mateFile2.c_str()));
    }
    void organizeReads() { ctx_.check(sage2ov_reads_organize(ctx_.get())); refresh(); }
    void saveReadsInFile(const std::string& path) { ctx_.check(sage2ov_reads_save(ctx_.get(), path.c_str())); }
    void loadReadsFromFile(const std::string& path) { ctx_.check(sage2ov_reads_load(ctx_.get(), path.c_str())); refresh(); }
    // readLoader.cpp:319-353: +id the read as given is the stored form, -id its reverse complement is, 0 not in the list
    int64_t getIdOfRead(const std::string& read) {
        const uint64_t off[2] = {0, read.size()}; int64_t id = 0;
        ctx_.check(sage2ov_reads_find_ids(ctx_.get(), read.data(), off, 1, &id)); return id;
    }
    // the same for many reads in one call (one search pass on the device instead of one per read)
    std::vector<int64_t> getIdOfRead(const std::vector<std::string>& reads) {
        std::string bases; std::vector<uint64_t> off(reads.size() + 1, 0); std::vector<int64_t> ids(reads.size(), 0);
        for (size_t r = 0; r < reads.size(); r++) { bases += reads[r]; off[r + 1] = bases.size(); }
        ctx_.check(sage2ov_reads_find_ids(ctx_.get(), bases.data(), off.data(), reads.size(), ids.data())); return ids;
    }
    sage2ov_read_stats stats() const { sage2ov_read_stats s{}; ctx_.check(sage2ov_reads_stats(ctx_.get(), &s)); return s; }
    Context& context() { return ctx_; }
private:
    void refresh() { auto s = stats(); numberOfUniqueReads = s.unique_reads; numberOfReads = s.good_reads; totalBP = s.total_bp; averageReadLength = s.average_read_length; }
    Context& ctx_;
};

// MatePair (matePair/matePair.h): the part that builds the lists, mapMatePairs / processMatePairs (matePair.cpp:70-239).  The table lives in the
// context (on the device when it has one); list() fetches a library once and caches it until the next add call.
class MatePair {
public:
    explicit MatePair(ReadLoader* loader1) : loaderObj(loader1) {}
    void mapMatePairs(const std::string& mateFile1, const std::string& mateFile2, int library) {
        ctx().check(sage2ov_mates_add_file(ctx().get(), mateFile1.c_str(), mateFile2.empty() ? nullptr : mateFile2.c_str(), library)); cachedLibrary_ = 0;
    }
    void mapMatePairsFromList(const std::string& listPath) { ctx().check(sage2ov_mates_add_list(ctx().get(), listPath.c_str())); cachedLibrary_ = 0; }
    // the same table from step 1's own pass (no second pass over the input): pairLibrary before the loader reads its input, mapMatePairsFromReads after organizeReads
    void pairLibrary(int library) { ctx().check(sage2ov_reads_pair_library(ctx().get(), library)); }
    void mapMatePairsFromReads() { ctx().check(sage2ov_mates_from_reads(ctx().get())); cachedLibrary_ = 0; }
    void processMatePairs(const std::vector<std::string>& readsArray, int library) {
        std::string bases; std::vector<uint64_t> off(readsArray.size() + 1, 0);
        for (size_t r = 0; r < readsArray.size(); r++) { bases += readsArray[r]; off[r + 1] = bases.size(); }
        ctx().check(sage2ov_mates_add_ascii(ctx().get(), bases.data(), off.data(), readsArray.size(), library)); cachedLibrary_ = 0;
    }
    int numberOfLibrary() const { return (int)stats().libraries; }
    // matePairList[readId] of the reference, entries of `library` only, in the reference's serial list order: head insertion (matePair.cpp:210-211,
    // :233-234) = descending `first`
    std::vector<sage2ov_mate> list(uint64_t readId, int library) {
        if (cachedLibrary_ != library) {
            uint64_t n = 0; ctx().check(sage2ov_mates_count(ctx().get(), library, &n));
            sage2ov_read_stats rs{}; ctx().check(sage2ov_reads_stats(ctx().get(), &rs));
            entries_.assign(n, sage2ov_mate{}); offsets_.assign(rs.unique_reads + 2, 0);
            ctx().check(sage2ov_mates_export(ctx().get(), library, entries_.data(), n, offsets_.data())); cachedLibrary_ = library;
        }
        if (readId + 1 >= offsets_.size()) return {};
        std::vector<sage2ov_mate> out(entries_.begin() + offsets_[readId], entries_.begin() + offsets_[readId + 1]);
        std::sort(out.begin(), out.end(), [](const sage2ov_mate& a, const sage2ov_mate& b) { return a.first > b.first; });
        return out;
    }
    sage2ov_mate_stats stats() const { sage2ov_mate_stats s{}; ctx().check(sage2ov_mates_stats_get(ctx().get(), &s)); return s; }
    // ---- matePair.cpp:244-609: reads on edges, locations, insert sizes.  The graph is the one the context holds after step 4 (OverlapGraph::simplify) or
    // after OverlapGraph::loadCompositeGraphFromFile.  The members below carry the reference's names; index = library, 0 unused.
    std::vector<unsigned> Mean, standardDeviation; std::vector<int> upperBoundOfInsert, lowerBoundOfInsert;
    uint64_t minimumUpperBoundOfInsert = 0, maximumUpperBoundOfInsert = 0;
    void mapReadsToEdges() { ctx().check(sage2ov_mates_map_reads(ctx().get())); table_ = false; }      // (mapReadLocations' work is done with it)
    void mapReadLocations() { fetch(); }
    void meanSdEstimation() {
        ctx().check(sage2ov_mates_estimate(ctx().get())); table_ = false;
        const int nl = numberOfLibrary();
        Mean.assign(nl + 1, 0); standardDeviation.assign(nl + 1, 0); upperBoundOfInsert.assign(nl + 1, 0); lowerBoundOfInsert.assign(nl + 1, 0);
        for (int l = 1; l <= nl; l++) {
            const sage2ov_insert i = insert(l);
            Mean[l] = (unsigned)i.mean; standardDeviation[l] = (unsigned)i.deviation; upperBoundOfInsert[l] = (int)i.upper; lowerBoundOfInsert[l] = (int)i.lower;
        }
        ctx().check(sage2ov_mates_bounds_get(ctx().get(), &minimumUpperBoundOfInsert, &maximumUpperBoundOfInsert));
    }
    sage2ov_insert insert(int library) const { sage2ov_insert i{}; ctx().check(sage2ov_mates_insert_get(ctx().get(), library, &i)); return i; }
    // readToEdgeList[readId]: the read's entries in ascending pair; locations(e): forward ones, then reverse ones
    std::vector<sage2ov_read_edge> readToEdgeList(uint64_t readId) {
        fetch(); if (readId + 1 >= edgeOffsets_.size()) return {};
        return std::vector<sage2ov_read_edge>(edges_.begin() + edgeOffsets_[readId], edges_.begin() + edgeOffsets_[readId + 1]);
    }
    std::vector<int32_t> locations(const sage2ov_read_edge& e, bool forward) {
        fetch(); const size_t a = e.location + (forward ? 0 : e.n_forward);
        return std::vector<int32_t>(locations_.begin() + a, locations_.begin() + a + (forward ? e.n_forward : e.n_reverse));
    }
    // findDistanceOnEdge (:575-609) for the edge a table entry stands for (pair = sage2ov_read_edge::pair): {count, locations...} of `read` on E, {0} when it
    // is not there -- the reference's array with its length in front
    std::vector<int32_t> findDistanceOnEdge(uint32_t pair, uint64_t read) {
        for (const sage2ov_read_edge& e : readToEdgeList(read)) if (e.pair == pair) {
            std::vector<int32_t> out = locations(e, true); out.insert(out.begin(), (int32_t)e.n_forward); return out;
        }
        return {0};
    }
    // the sweep of ContigExtender::findMatepairSupports (mergeContigs.cpp:959-1022): every (in, out) pair of a node with support >= minSupport; 2 gives the list the
    // reference merges from (:992).  The merges themselves stay with the caller
    std::vector<sage2ov_support> matepairSupports(uint32_t minSupport = 2) {
        uint64_t n = 0; ctx().check(sage2ov_mates_supports_count(ctx().get(), minSupport, &n));
        std::vector<sage2ov_support> out(n); ctx().check(sage2ov_mates_supports_export(ctx().get(), minSupport, out.data(), n));
        return out;
    }
    // the sweep of ContigExtender::findPathSupports / findPathSupportsNew (mergeContigs.cpp:118-353): every (a enters a node, b leaves it) pair that mate pairs voted for
    // through the paths between them; one round of either (variant 0 / 1), and the loops of :62-99
    std::vector<sage2ov_path_support> pathSupports(uint32_t minSupport = 1) {
        uint64_t n = 0; ctx().check(sage2ov_path_supports_count(ctx().get(), minSupport, &n));
        std::vector<sage2ov_path_support> out(n); ctx().check(sage2ov_path_supports_export(ctx().get(), minSupport, out.data(), n));
        return out;
    }
    sage2ov_path_stats pathStats() const { sage2ov_path_stats s{}; ctx().check(sage2ov_path_stats_get(ctx().get(), &s)); return s; }
    uint64_t findPathSupports(int highTh, int variant = 0, int lowTh = 1) { uint64_t m = 0; ctx().check(sage2ov_extend_paths_round(ctx().get(), highTh, lowTh, variant, &m)); table_ = false; return m; }
    std::pair<uint64_t, uint64_t> extendByPaths(int variant, uint64_t genomeSize = 0) { uint64_t r = 0, m = 0; ctx().check(sage2ov_extend_by_paths(ctx().get(), genomeSize, variant, &r, &m)); table_ = false; return {r, m}; }
    // the sweep that opens ScaffoldMaker::mergeFinal (mode SAGE2OV_LINKS_FINAL) / mergeFinalSmall (SAGE2OV_LINKS_SMALL), scaffolding.cpp:786-935, :981-1130: support and
    // gap of every ordered pair of half-edges linked by mates, both directions.  The merges stay with the caller
    std::vector<sage2ov_link> scaffoldLinks(uint32_t mode = SAGE2OV_LINKS_ALL, uint32_t minSupport = 1) {
        uint64_t n = 0; ctx().check(sage2ov_links_count(ctx().get(), mode, minSupport, &n));
        std::vector<sage2ov_link> out(n); ctx().check(sage2ov_links_export(ctx().get(), mode, minSupport, out.data(), n));
        return out;
    }
    // ScaffoldMaker::makeScaffolds (scaffolding.cpp:31-98) on the resident graph: the five loops, or one mergeFinal / mergeFinalSmall round; the joins of the last round
    std::pair<uint64_t, uint64_t> makeScaffolds(uint64_t genomeSize = 0) { uint64_t r = 0, m = 0; ctx().check(sage2ov_scaffold(ctx().get(), genomeSize, &r, &m)); table_ = false; return {r, m}; }
    uint64_t mergeFinal(int highTh, int flag, bool small = false) { uint64_t m = 0; ctx().check(sage2ov_scaffold_round(ctx().get(), highTh, flag, small ? 1 : 0, &m)); table_ = false; return m; }
    std::vector<sage2ov_join> scaffoldJoins() {
        uint64_t n = 0; ctx().check(sage2ov_scaffold_merges_count(ctx().get(), &n));
        std::vector<sage2ov_join> out(n); ctx().check(sage2ov_scaffold_merges_export(ctx().get(), out.data(), n));
        return out;
    }
    // the raw int32_t gapSum of the rows scaffoldLinks(mode, minSupport) returns, in the same order (mergeContigs.cpp:1587 reads it; a row's gap is its quotient)
    std::vector<int32_t> scaffoldLinkGapSums(uint32_t mode = SAGE2OV_LINKS_ALL, uint32_t minSupport = 1) {
        uint64_t n = 0; ctx().check(sage2ov_links_count(ctx().get(), mode, minSupport, &n));
        std::vector<int32_t> out(n); ctx().check(sage2ov_links_gap_sums(ctx().get(), mode, minSupport, out.data(), n));
        return out;
    }
    void graphChanged() { table_ = false; }              // a merge or join made outside this object: the cached read-to-edge table is stale
    ReadLoader* loaderObj;
private:
    Context& ctx() const { return loaderObj->context(); }
    void fetch() {
        if (table_) return;
        uint64_t ne = 0, nl = 0; ctx().check(sage2ov_mates_read_edges_count(ctx().get(), &ne, &nl));
        sage2ov_read_stats rs{}; ctx().check(sage2ov_reads_stats(ctx().get(), &rs));
        edges_.assign(ne, sage2ov_read_edge{}); locations_.assign(nl, 0); edgeOffsets_.assign(rs.unique_reads + 2, 0);
        ctx().check(sage2ov_mates_read_edges_export(ctx().get(), edges_.data(), ne, locations_.data(), nl, edgeOffsets_.data())); table_ = true;
    }
    std::vector<sage2ov_mate> entries_; std::vector<uint64_t> offsets_; int cachedLibrary_ = 0;
    std::vector<sage2ov_read_edge> edges_; std::vector<int32_t> locations_; std::vector<uint64_t> edgeOffsets_; bool table_ = false;
};

// ContigExtender (mergeContigs.h): the fourth loop of extendContigs and the whole function, on the resident graph (the first three loops are also MatePair's
// findMatepairSupports sweep with sage2ov_extend_round, findPathSupports and extendByPaths above)
class ContigExtender {
public:
    explicit ContigExtender(MatePair* mate1) : mateObj(mate1) {}
    // mergeShortOverlaps (mergeContigs.cpp:1474-1648): one round.  The sweep uses the context's k, as every sweep here does: minOverlap is not read
    uint64_t mergeShortOverlaps(uint16_t /*minOverlap*/, int highTh) {
        uint64_t m = 0; ctx().check(sage2ov_extend_short_round(ctx().get(), highTh, &m)); mateObj->graphChanged(); return m;
    }
    std::vector<sage2ov_join> shortOverlapJoins() {
        uint64_t n = 0; ctx().check(sage2ov_extend_short_merges_count(ctx().get(), &n));
        std::vector<sage2ov_join> out(n); ctx().check(sage2ov_extend_short_merges_export(ctx().get(), out.data(), n));
        return out;
    }
    sage2ov_scaffold_stats shortOverlapStats() const { sage2ov_scaffold_stats s{}; ctx().check(sage2ov_extend_short_stats_get(ctx().get(), &s)); return s; }
    // extendContigs (:37-113): the four loops; returns the total number of merges (sum_node_resolved); rounds / merged (may be null): four values each
    uint64_t extendContigs(uint16_t /*minOverlap*/, uint64_t genomeSize = 0, uint64_t* rounds = nullptr, uint64_t* merged = nullptr) {
        uint64_t r[4] = {0, 0, 0, 0}, m[4] = {0, 0, 0, 0};
        const int rc = sage2ov_extend_contigs(ctx().get(), genomeSize, r, m); mateObj->graphChanged();
        for (int i = 0; i < 4; i++) { if (rounds) rounds[i] = r[i]; if (merged) merged[i] = m[i]; }
        ctx().check(rc); return m[0] + m[1] + m[2] + m[3];
    }
    MatePair* mateObj;
private:
    Context& ctx() const { return mateObj->loaderObj->context(); }
};

// HashTable (hashTable.h:20-43)
class HashTable {
public:
    explicit HashTable(ReadLoader* loader1) : loaderObj(loader1) {}
    void hashPrefixesAndSuffix() { loaderObj->context().check(sage2ov_index_build(loaderObj->context().get())); }
    void saveHashTableInFile(const std::string& path) { loaderObj->context().check(sage2ov_hashtable_save(loaderObj->context().get(), path.c_str())); }   // hashTable.cpp:256
    sage2ov_index_stats stats() const { sage2ov_index_stats s{}; loaderObj->context().check(sage2ov_index_stats_get(loaderObj->context().get(), &s)); return s; }
    ReadLoader* loaderObj;
};

// EconomyGraph (economyGraph.h:32-54)
class EconomyGraph {
public:
    explicit EconomyGraph(HashTable* hash1) : hashObj(hash1) {}
    void buildInitialOverlapGraph() { ctx().check(sage2ov_overlap_initial(ctx().get())); }
    void buildOverlapGraphEconomy() { ctx().check(sage2ov_overlap_reduce(ctx().get())); }
    void sortEconomyGraph() {}   // folded into OverlapGraph::convertGraph (one device pass does both, economyGraph.cpp:896 + overlapGraph.cpp:84)
    sage2ov_overlap_stats stats() const { sage2ov_overlap_stats s{}; ctx().check(sage2ov_overlap_stats_get(ctx().get(), &s)); return s; }
    HashTable* hashObj;
    Context& ctx() const { return hashObj->loaderObj->context(); }
};

// OverlapGraph, steps-1-3 part (overlapGraph.h:54-67: convertGraph, saveOverlapGraphInFile)
class OverlapGraph {
public:
    OverlapGraph(EconomyGraph* economy1, ReadLoader* loader1) : economyObj(economy1), ctx_(&loader1->context()) {}
    explicit OverlapGraph(ReadLoader* loader1) : economyObj(nullptr), ctx_(&loader1->context()) {}          // overlapGraph.cpp:47 (graph from a file)
    void convertGraph() { ctx_->check(sage2ov_overlap_convert(ctx_->get())); }
    void saveOverlapGraphInFile(const std::string& path) { ctx_->check(sage2ov_graph_save(ctx_->get(), path.c_str())); }
    void loadOverlapGraphFromFile(const std::string& path) { ctx_->check(sage2ov_graph_load(ctx_->get(), path.c_str())); }
    // step 4: the loop of main.cpp:150-172 over contractCompositePaths / removeDeadEnds / removeBubbles (simplification.cpp), on the device
    sage2ov_simplify_stats simplify() { ctx_->check(sage2ov_graph_simplify(ctx_->get())); sage2ov_simplify_stats s{}; ctx_->check(sage2ov_simplify_stats_get(ctx_->get(), &s)); return s; }
    void loadCompositeGraphFromFile(const std::string& path) { ctx_->check(sage2ov_graph_load_composite(ctx_->get(), path.c_str())); }   // overlapGraph.cpp:371 for P.graph4 / 5 / 6
    void saveSimplifiedGraphInFile(const std::string& path) { ctx_->check(sage2ov_graph4_save(ctx_->get(), path.c_str())); }   // what step 5 loads (main.cpp:196)
    // printGraph (overlapGraph.cpp:507-593) without the .gdl: writes fileName + ".fasta" over the graph the context holds; the statistics the reference logs come back.
    // contigLengthThreshold 0: the reference's own (:32)
    sage2ov_contig_stats printGraph(const std::string& fileName, bool isScaff = false, uint64_t genomeSize = 0, uint32_t contigLengthThreshold = 0) {
        ctx_->check(sage2ov_contigs_build(ctx_->get(), contigLengthThreshold, genomeSize));
        ctx_->check(sage2ov_contigs_save(ctx_->get(), (fileName + ".fasta").c_str(), isScaff ? 1 : 0));
        sage2ov_contig_stats s{}; ctx_->check(sage2ov_contig_stats_get(ctx_->get(), &s)); return s;
    }
    std::vector<sage2ov_contig> contigs() {
        uint64_t n = 0; ctx_->check(sage2ov_contigs_count(ctx_->get(), &n, nullptr));
        std::vector<sage2ov_contig> out(n); ctx_->check(sage2ov_contigs_export(ctx_->get(), out.data(), n)); return out;
    }
    // the whole strings of rows [first, first + count) of contigs(), one after the other; offsets: count + 1 values
    std::string contigSequences(uint64_t first, uint64_t count, std::vector<uint64_t>& offsets) {
        const std::vector<sage2ov_contig> rows = contigs(); uint64_t need = 0;
        for (uint64_t i = first; i < first + count && i < rows.size(); i++) need += rows[i].string_length;
        std::string out(need, 'N'); offsets.assign(count + 1, 0);
        ctx_->check(sage2ov_contigs_sequences(ctx_->get(), first, count, &out[0], need, offsets.data())); return out;
    }
    EconomyGraph* economyObj;
    Context& context() const { return *ctx_; }
private:
    Context* ctx_;
};

// CopyCountEstimator (copycountEstimator.h): step 5 over the graph the context holds
class CopyCountEstimator {
public:
    explicit CopyCountEstimator(OverlapGraph* graph1) : graphObj(graph1) {}
    // genomeSizeEstimation (copycountEstimator.cpp:29-54)
    uint64_t genomeSizeEstimation() { uint64_t g = 0; ctx().check(sage2ov_genome_size_estimate(ctx().get(), &g)); return g; }
    // computeMinCostFlow (:105-417): the network, the solve (main_cs2, :359 -- here on the device) and the flows onto the graph; returns the genome size
    uint64_t computeMinCostFlow() { uint64_t g = 0; ctx().check(sage2ov_copy_counts(ctx().get(), &g)); return g; }
    sage2ov_mcf_stats solverStats() const { sage2ov_mcf_stats s{}; ctx().check(sage2ov_mcf_stats_get(ctx().get(), &s)); return s; }
    OverlapGraph* graphObj;
private:
    Context& ctx() const { return graphObj->context(); }
};

}  // namespace sage2ov
