"""The restatement of tests/path_model.py against the reference itself, by the reference's objects with one thread on a P.reads a device-less context saved and a
graph file its own loader reads (every record pair is an edge: parse_graph(fold=False)).
Mode `paths`: the model names every claiming node's start nodes and its eligible mate entries; the driver calls the reference's own exploreGraph, quicksortPaths,
indexPaths and findPathsBetweenMatepairs (matePair/mergeContigs.cpp:359-743) and prints the path count and the supported pairs of every entry.
Mode `whole`: ContigExtender::findPathSupports / findPathSupportsNew (:118-353, :2148-) round after round, each round at its own threshold (the loops of :62-99 lower
it by iteration); the graph file after every round against the model's text.
Every case is one where the model reports zero for capped_nodes, mirrored and key_collisions and, in mode `whole`, an order-free round (include/sage2ov.h, DELIBERATE
DIFFERENCES): a case that does not meet the condition fails.  Runs only where the reference tree and the objects built from it (oracle/_ref/) are present.  The driver
below is our own text; it includes the reference's headers and links oracle/_ref/libsage2ref_driver.so."""
import gzip
import os
import subprocess

import pytest

import fixtures as fx
import compgen as CG
import extend_model as X
import path_model as PM
import test_compgen_host as GH
import test_mate_estimate_host as H
import test_mate_support_host as MS
from test_extend_reference import REF, REF_DIR, REF_LIB, body, hand_store, host_store

pytestmark = pytest.mark.skipif(not (os.path.isdir(REF) and os.path.exists(REF_LIB)), reason="the reference tree or oracle/_ref/libsage2ref_driver.so is absent")

DRIVER_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>
#include "matePair/mergeContigs.h"
extern ofstream logStream;
extern int lowThreshold;
static void name(Edge* e) { printf(" %llu %llu %d %llu", (unsigned long long)e->fromID, (unsigned long long)e->ID, (int)e->typeOfEdge, (unsigned long long)e->lengthOfEdge); }
int main(int argc, char** argv) {      // <whole|paths> <variant> <k> <P.reads> <graph file> <log file> <out prefix> <work file> <mates.fa of library 1> ...
    omp_set_num_threads(1);
    const bool whole = strcmp(argv[1], "whole") == 0;
    const int variant = atoi(argv[2]); const uint16_t k = (uint16_t)atoi(argv[3]);
    logStream.open(argv[6]);
    lowThreshold = 1;                                                   // main.cpp:357
    ReadLoader* loader = new ReadLoader(k);
    loader->loadReadsFromFile(argv[4]);
    OverlapGraph* graph = new OverlapGraph(loader);
    graph->loadOverlapGraphFromFile(argv[5]);
    MatePair* mates = new MatePair(graph, loader);
    for (int lib = 1; 8 + lib < argc; lib++) mates->mapMatePairs(argv[8 + lib], "", lib);
    mates->meanSdEstimation();
    ContigExtender* ext = new ContigExtender(graph, mates, loader);
    printf("x %llu\n", (unsigned long long)mates->maximumUpperBoundOfInsert);
    std::ifstream in(argv[8]);
    if (whole) {                                                        // work file: the threshold of every round
        int high, round = 0;
        while (in >> high) {
            round++;
            const uint64_t n = variant ? ext->findPathSupportsNew(high) : ext->findPathSupports(high);
            printf("r %d %llu\n", round, (unsigned long long)n);
            graph->saveOverlapGraphInFile(std::string(argv[7]) + "." + std::to_string(round));
        }
        logStream.close();
        return 0;
    }
    // paths: per node "node ns s1 .. ns ne" and ne lines "m1 m2 type1 type2 library"; the arrays as findPathSupports makes them (:148-162), with rows to spare
    const int ROWS = 4000;
    uint64_t* pathLengths = (uint64_t*)malloc(20 * sizeof(uint64_t)); Edge** pathEdges = (Edge**)malloc(20 * sizeof(Edge*));
    Edge*** all = (Edge***)malloc(ROWS * sizeof(Edge**)); uint64_t* allLen = (uint64_t*)malloc(ROWS * sizeof(uint64_t));
    for (int j = 0; j < ROWS; j++) all[j] = (Edge**)malloc(10 * sizeof(Edge*));
    PairSupported* sup = (PairSupported*)malloc(20000 * sizeof(PairSupported));
    long long node, ns, ne;
    while (in >> node >> ns) {
        for (int j = 0; j < 20; j++) { pathLengths[j] = 0; pathEdges[j] = NULL; }
        for (int j = 0; j < ROWS; j++) { allLen[j] = 0; for (int l = 0; l < 10; l++) all[j][l] = NULL; }
        uint64_t total = 0;
        for (long long s = 0; s < ns; s++) { long long st; in >> st; ext->exploreGraph((uint64_t)st, 1, total, pathEdges, pathLengths, all, allLen); }
        in >> ne;
        printf("p %lld %llu\n", node, (unsigned long long)total);
        Indexes** indx = NULL;
        if (total > 0) {
            ext->quicksortPaths(0, (int64_t)total - 1, all, allLen);
            indx = (Indexes**)malloc((ns + 2) * sizeof(Indexes*));
            ext->indexPaths((uint64_t)ns, indx, total, all);
        }
        for (long long e = 0; e < ne; e++) {
            long long m1, m2, t1, t2, lib; in >> m1 >> m2 >> t1 >> t2 >> lib;
            const int n = total ? ext->findPathsBetweenMatepairs((uint64_t)m1, (uint64_t)m2, t1 != 0, t2 != 0, (int)lib, indx, total, all, allLen, sup) : 0;
            printf("e %lld %lld %lld %lld %lld %d", m1, m2, t1, t2, lib, n);
            for (int j = 0; j < n; j++) { name(sup[j].edge1); name(sup[j].edge2); }
            printf("\n");
        }
        if (indx) { ext->freeIndexedPaths(indx); free(indx); }
    }
    logStream.close();
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("refpaths")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(DRIVER_CPP)
    subprocess.run(["g++", "-fopenmp", "-std=c++0x", "-O1", "-w", "-include", os.path.join(fx.ROOT, "oracle", "ref_prelude.h"), "-I", REF, src, "-o", exe,
                    "-L", REF_DIR, "-lsage2ref_driver", "-Wl,-rpath," + REF_DIR, "-lz"], check=True)
    return exe


def call(driver, tmp_path, mode, ctx, k, variant, text, pairs, work):
    seqs = H.stored_reads(ctx)
    rp, gp, lp, op, wp = (str(tmp_path / n) for n in ("P.reads", "P.graph", "log.txt", "out.graph", "work.txt"))
    ctx.reads_save(rp); open(gp, "w").write(text); open(wp, "w").write(work)
    mfs = []
    for L in sorted(pairs):
        bs, o = H.mates_ascii(pairs[L], seqs); mf = str(tmp_path / ("m%d.fa" % L)); mfs.append(mf)
        open(mf, "w").write("".join(">m%d\n%s\n" % (i, bs[int(o[i]):int(o[i + 1])].tobytes().decode()) for i in range(len(o) - 1)))
    out = subprocess.run([driver, mode, str(variant), str(k), rp, gp, lp, op, wp] + mfs, check=True, stdout=subprocess.PIPE, text=True, timeout=300,
                         env=dict(os.environ, OMP_NUM_THREADS="1")).stdout.splitlines()
    return out, op


def same_paths(driver, tmp_path, ctx, k, text, pairs, uncapped_only=False):
    """mode `paths` on every claiming node -> (nodes compared, their paths, entries compared, entries that vote, the most pairs one entry supports).  uncapped_only: the
    nodes that save more than 1000 paths are left out (the contract claims nothing for them) instead of failing the case"""
    g = X.Graph(H.parse_graph(text, fold=False)); est = PM.Estimate(g, pairs)
    sw = PM.sweep(g, pairs, est)
    assert (sw["stats"]["mirrored"], sw["stats"]["key_collisions"]) == (0, 0) and (uncapped_only or sw["stats"]["capped_nodes"] == 0)
    nodes = [i for i in sorted(sw["starts"]) if len(sw["paths"][i]) <= PM.CAP]
    sw["entries"] = [e for e in sw["entries"] if e["node"] in set(nodes)]
    by_node = {}
    for e in sw["entries"]:
        by_node.setdefault(e["node"], []).append(e)
    work = "".join("%d %d %s %d\n%s" % (i, len(sw["starts"][i]), " ".join(map(str, sw["starts"][i])), len(by_node.get(i, [])),
                                        "".join("%d %d %d %d %d\n" % (e["m1"], e["m2"], e["type1"], e["type2"], e["library"]) for e in by_node.get(i, []))) for i in nodes)
    out, _ = call(driver, tmp_path, "paths", ctx, k, 0, text, pairs, work)
    assert "x %d" % est.max_upper in out
    assert [x for x in out if x.startswith("p ")] == ["p %d %d" % (i, len(sw["paths"][i])) for i in nodes]
    named = lambda x: (g.h[x]["frm"], g.h[x]["to"], g.h[x]["type"], g.h[x]["len"])
    got = {}
    for x in out:
        if x.startswith("e "):
            f = [int(v) for v in x.split()[1:]]
            got[tuple(f[:5])] = (f[5], {(tuple(f[6 + 8 * j:10 + 8 * j]), tuple(f[10 + 8 * j:14 + 8 * j])) for j in range(f[5])})
    want = {(e["m1"], e["m2"], e["type1"], e["type2"], e["library"]): (len(e["survivors"]), {(named(a), named(b)) for a, b in e["survivors"]}) for e in sw["entries"]}
    assert got == want
    return len(nodes), sum(len(sw["paths"][i]) for i in nodes), len(want), sum(1 for n, _ in want.values() if n), max([n for n, _ in want.values()] + [0])


def same_rounds(driver, tmp_path, ctx, k, variant, text, pairs, highs):
    """mode `whole` with the threshold of every round -> merges per round; every round must lie inside the domain of the claimed equality"""
    g = X.Graph(H.parse_graph(text, fold=False)); est = PM.Estimate(g, pairs)
    out, op = call(driver, tmp_path, "whole", ctx, k, variant, text, pairs, " ".join(map(str, highs)))
    assert "x %d" % est.max_upper in out
    ref_rounds = [int(x.split()[2]) for x in out if x.startswith("r ")]
    assert len(ref_rounds) == len(highs)
    got = []
    for rd, (n, high) in enumerate(zip(ref_rounds, highs), 1):
        r = PM.round_(g, pairs, est, high, 1, variant)
        assert (r["order_dependent"], r["stats"]["key_collisions"], r["stats"]["capped_nodes"], r["stats"]["mirrored"]) == (0, 0, 0, 0), rd
        assert n == len(r["merges"]), rd
        assert body(open("%s.%d" % (op, rd)).read()) == body(g.text()), rd
        got.append(n)
    return got


# ------------------------------------------------------------------------------------------ mode `paths`
CHAIN_NODES = (1, 2, 4, 8, 16, 32, 64, 3, 5, 6)            # no two consecutive edge pairs share their XOR key
HAND = dict(PM.CASES, chain=lambda: PM.chain_graph(CHAIN_NODES))
del HAND["ladder"]                                          # (a capped node: the contract claims nothing for it)


@pytest.mark.parametrize("case", sorted(HAND))
def test_paths_and_supported_pairs_on_the_hand_built_graphs(case, driver, tmp_path):
    """the walk over loops with and without a list at uses == flow, the bound, seven levels, every distance edge; the chain's entry supports seven pairs"""
    N, header, recs, pairs = HAND[case]()
    ctx = hand_store(N)
    nodes, paths, entries, voting, most = same_paths(driver, tmp_path, ctx, MS.HAND_K, H.graph_text(header, recs), pairs)
    assert paths > 0 and (most == 7 if case == "chain" else True) and (paths == 122 if case == "flow" else True) and ((voting, most) == (3, 1) if case == "bubble" else True)
    ctx.close()


def generated(seed):
    """about 200 pairs with a hub, loops written once and twice, simple edges, reads on many pairs and twice on an edge, flows >= 1 on two pairs in three; the mates of
    compgen (same edge, through a node, ...) and 200 pairs placed across forks of the graph.  The seeds were chosen so that the three counters are 0"""
    case = CG.composite_graph(3000 + seed, 200, n_reads=2000, hubs=1, loops_once=2, loops_twice=2, dense_edges=2, read_copies=(2, 2, 3, 5), twice_on_edge=0.08,
                              flows=(1.0, 1.0, 2.0, 0.5, 1.0, 0.0))
    N, header, recs = case
    pairs = CG.mates_e(GH.parsed(case), seed, for_reference=True)
    g = X.Graph(H.parse_graph(H.graph_text(header, recs), fold=False)); est = PM.Estimate(g, pairs)
    pairs[1] = pairs[1] + PM.fork_mates(g, PM.sweep(g, pairs, est), seed)
    assert PM.Estimate(g, pairs).ests == est.ests                                    # (mates on different edges do not move the estimate)
    return N, header, recs, pairs


@pytest.mark.parametrize("seed", [0, 1, 3, 6])
def test_paths_and_supported_pairs_on_generated_graphs(seed, driver, tmp_path):
    N, header, recs, pairs = generated(seed)
    ctx = GH.host_store(N, 100 + seed)
    nodes, paths, entries, voting, most = same_paths(driver, tmp_path, ctx, CG.K, H.graph_text(header, recs), pairs)
    assert nodes > 64 and paths > 3000 and entries > 500 and voting > 100 and most >= 2
    ctx.close()


def golden(name):
    """the golden graph with flow 1 on every even record pair and 0 on the odd ones, and the golden cases' mates"""
    m = fx.golden(name); ctx = host_store(fx.make_reads(m["synth"]), m["k"])
    g = MS.with_flows(H.parse_graph(gzip.open(os.path.join(fx.GOLDEN, name + ".graph4.gz")).read(), fold=False), lambda q, a=None: (0.0, 0.0) if q % 2 else (1.0, 1.0))
    text = H.graph_text(g["header"], [r for _, a, b in g["pairs"] for r in (a, b)])
    return m, ctx, text, MS.golden_mates(g, ctx.reads_stats().unique_reads)


def test_paths_and_supported_pairs_on_g9_with_flows(driver, tmp_path):
    m, ctx, text, pairs = golden("g9_repeats160k_k40")
    nodes, paths, entries, voting, most = same_paths(driver, tmp_path, ctx, m["k"], text, pairs)
    assert nodes > 3000 and paths > 50000 and entries > 1000 and voting > 30
    ctx.close()


def test_paths_and_supported_pairs_on_the_uncapped_nodes_of_g4(driver, tmp_path):
    """g4 is a high-copy graph: whatever its flows, simple edges pass checkFlow once and hundreds of its nodes save more than 1000 paths.  Those are outside the claimed
    equality (difference 3) and are left out; every other claiming node and its entries are compared"""
    m, ctx, text, pairs = golden("g4_highcopy_k21")
    nodes, paths, entries, voting, most = same_paths(driver, tmp_path, ctx, m["k"], text, pairs, uncapped_only=True)
    assert nodes > 300 and paths > 20000 and entries > 50
    ctx.close()


# ------------------------------------------------------------------------------------------ mode `whole`
def lone_row(**kw):
    """the fork with a C of 120 bases whose read 61 is the mate of 41 and 42: (A, C) has the five votes of 41, 42, 43 -> E and 41, 42 -> 61, (C, E) the three of A's
    pairs and 61 -> 53's; at high 5 one row stands at the threshold"""
    extra = [(41, 1, 61, 0), (42, 1, 61, 0), (61, 1, 53, 1)] + list(kw.pop("more", []))
    return PM.fork_graph(lenC=120, extra=extra, **kw)


@pytest.mark.parametrize("variant", [0, 1])
def test_the_fork_with_one_row_at_the_threshold(variant, driver, tmp_path):
    N, header, recs, pairs = lone_row()
    g = X.Graph(H.parse_graph(H.graph_text(header, recs))); est = PM.Estimate(g, pairs)
    assert PM.sweep(g, pairs, est)["rows"] == [(10, 2, 6, 3), (10, 0, 4, 5), (11, 4, 8, 4), (12, 6, 10, 3)]
    ctx = hand_store(N)
    assert same_rounds(driver, tmp_path, ctx, MS.HAND_K, variant, H.graph_text(header, recs), pairs, [5, 5]) == [1, 0]
    ctx.close()


@pytest.mark.parametrize("variant", [0, 1])
def test_a_third_in_edge_at_the_threshold(variant, driver, tmp_path):
    """G's reads 47 and 48 have their mates on C: (G, C) has support 2 > low among the ins of (A, C).  Variant 0 refuses, variant 1 merges (:2504)"""
    N, header, recs, pairs = lone_row(third=True)
    pairs = {1: [p for p in pairs[1] if p[0] not in (48, 49)] + [(47, 1, 61, 0), (48, 1, 61, 0)]}
    g = X.Graph(H.parse_graph(H.graph_text(header, recs))); est = PM.Estimate(g, pairs)
    assert PM.sweep(g, pairs, est)["rows"] == [(10, 14, 4, 2), (10, 2, 6, 3), (10, 0, 4, 5), (11, 4, 8, 4), (12, 6, 10, 3)]
    ctx = hand_store(N)
    assert same_rounds(driver, tmp_path, ctx, MS.HAND_K, variant, H.graph_text(header, recs), pairs, [5, 5]) == ([0, 0] if variant == 0 else [1, 0])
    ctx.close()


@pytest.mark.parametrize("variant", [0, 1])
def test_four_rounds_at_falling_thresholds(variant, driver, tmp_path):
    """the thresholds of the loop fall with the iteration (:69-74).  At 5 the row (A, C) stands alone; at 4 (A.C, E) and (B, D) -- B's read 44 has its mate on D --
    stand at nodes that share no edge; at 3 (B.D, F) is left; then nothing"""
    N, header, recs, pairs = lone_row(more=[(44, 1, 62, 0)])
    ctx = hand_store(N)
    assert same_rounds(driver, tmp_path, ctx, MS.HAND_K, variant, H.graph_text(header, recs), pairs, [5, 4, 3, 3]) == [1, 2, 1, 0]
    ctx.close()


@pytest.mark.parametrize("seed,variant,merges", [(4, 0, [3, 0]), (4, 1, [4, 0]), (10, 0, [3, 0]), (10, 1, [5, 0])])
def test_rounds_on_generated_graphs(seed, variant, merges, driver, tmp_path):
    """compgen's case_e at the highest support of its table, 3: seeds where the rows at the threshold share no node and no edge end, in every round"""
    case = CG.case_e(seed); N, header, recs = case
    pairs = CG.mates_e(GH.parsed(case), seed, for_reference=True)
    ctx = GH.host_store(N, 100 + seed)
    assert same_rounds(driver, tmp_path, ctx, CG.K, variant, H.graph_text(header, recs), pairs, [3, 3]) == merges
    ctx.close()
