"""The restatement of tests/extend_model.py against the reference itself: ContigExtender::findMatepairSupports (matePair/mergeContigs.cpp:959-1030) run until it
merges nothing (mode `whole`), and the reference's own mergeByMatepairSupports (:1112-1255) handed the list in the order include/sage2ov.h defines (mode `ordered`),
by the reference's objects with one thread on a P.reads a device-less context saved and a graph file its own loader reads (every record pair is an edge:
parse_graph(fold=False)).  Runs only where the reference tree and the objects built from it (oracle/_ref/) are present.  The driver below is our own text; it
includes the reference's headers and links oracle/_ref/libsage2ref_driver.so."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import fixtures as fx
import sage2_amd as s2
import compgen as CG
import extend_model as X
import test_compgen_host as GH
import test_mate_estimate_host as H
import test_mate_support_host as MS

REF = "/root/reference"
REF_DIR = os.path.join(fx.ROOT, "oracle", "_ref")
REF_LIB = os.path.join(REF_DIR, "libsage2ref_driver.so")
pytestmark = pytest.mark.skipif(not (os.path.isdir(REF) and os.path.exists(REF_LIB)), reason="the reference tree or oracle/_ref/libsage2ref_driver.so is absent")

DRIVER_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <algorithm>
#include "matePair/mergeContigs.h"
extern ofstream logStream;
extern int lowThreshold;
static bool bySupport(const SupportedEdgePair& a, const SupportedEdgePair& b) { return a.support > b.support; }
// findMatepairSupports (:959-1030) with the list kept in building order among equal supports: node ascending, the node's list order for the in-edge, then the out-edge
static uint64_t orderedRound(ContigExtender* ext, OverlapGraph* graph, ReadLoader* loader, uint16_t k, int high) {
    std::deque<SupportedEdgePair> list;
    std::unordered_map<std::pair<uint64_t, uint64_t>, SupportedEdgePair, pairHash> search;
    std::unordered_multimap<uint64_t, SupportedEdgePair> del;
    for (uint64_t i = 1; i <= loader->numberOfUniqueReads; i++) {
        if (graph->graph[i] == NULL) continue;
        std::deque<Edge*> ins, outs;
        for (Edge* v = graph->graph[i]; v != NULL; v = v->next)
            if (v->flow >= 1 && v->listOfReads[0].readId > 0 && v->ID != v->fromID) { if (v->typeOfEdge == 0 || v->typeOfEdge == 1) ins.push_back(v->twinEdge); else outs.push_back(v); }
        for (size_t a = 0; a < ins.size(); a++)
            for (size_t b = 0; b < outs.size(); b++) {
                const int s = ext->getSupportOfEdges(ins[a]->twinEdge, outs[b], k);
                if (s <= 1) continue;
                SupportedEdgePair p; p.edge1 = ins[a]; p.edge2 = outs[b]; p.support = s;
                list.push_back(p);
                const std::pair<uint64_t, uint64_t> key(ins[a]->fromID ^ ins[a]->ID, outs[b]->fromID ^ outs[b]->ID);
                auto it = search.find(key);
                if (it == search.end() || s > it->second.support) search[key] = p;
                for (uint64_t node : {(uint64_t)p.edge1->ID, (uint64_t)p.edge1->fromID, (uint64_t)p.edge2->ID, (uint64_t)p.edge2->fromID}) del.insert(std::make_pair(node, p));
            }
    }
    if (list.empty()) return 0;
    std::stable_sort(list.begin(), list.end(), bySupport);
    return ext->mergeByMatepairSupports(list, search, del, high);
}
int main(int argc, char** argv) {      // <whole|ordered> <k> <high> <P.reads> <graph file> <log file> <out prefix> <mates.fa of library 1> [<mates.fa of library 2>]
    omp_set_num_threads(1);
    const bool ordered = strcmp(argv[1], "ordered") == 0;
    const uint16_t k = (uint16_t)atoi(argv[2]); const int high = atoi(argv[3]);
    logStream.open(argv[6]);
    lowThreshold = 1;                                                   // main.cpp:357
    ReadLoader* loader = new ReadLoader(k);
    loader->loadReadsFromFile(argv[4]);
    OverlapGraph* graph = new OverlapGraph(loader);
    graph->loadOverlapGraphFromFile(argv[5]);                           // (sets genomeSize and averageReadLength from the header)
    MatePair* mates = new MatePair(graph, loader);
    for (int lib = 1; 7 + lib < argc; lib++) mates->mapMatePairs(argv[7 + lib], "", lib);
    mates->meanSdEstimation();
    ContigExtender* ext = new ContigExtender(graph, mates, loader);
    printf("x %llu\n", (unsigned long long)mates->maximumUpperBoundOfInsert);
    for (int round = 1; round <= 100; round++) {
        const uint64_t n = ordered ? orderedRound(ext, graph, loader, k, high) : ext->findMatepairSupports(k, high);
        printf("r %d %llu\n", round, (unsigned long long)n);
        graph->saveOverlapGraphInFile(std::string(argv[7]) + "." + std::to_string(round));
        if (round == 1)
            for (uint64_t r = 1; r <= loader->numberOfUniqueReads; r++)
                for (ReadToEdgeMap* e = mates->readToEdgeList[r]; e != NULL; e = e->next) {
                    printf("t %llu %llu %llu %d %u f", (unsigned long long)r, (unsigned long long)e->edge->fromID, (unsigned long long)e->edge->ID, (int)e->edge->typeOfEdge, (unsigned)e->edge->lengthOfEdge);
                    for (uint32_t x = 1; e->locationForward && x <= e->locationForward[0]; x++) printf(" %d", (int)e->locationForward[x]);
                    printf(" r");
                    for (uint32_t x = 1; e->locationReverse && x <= e->locationReverse[0]; x++) printf(" %d", (int)e->locationReverse[x]);
                    printf("\n");
                }
        if (n == 0) break;
    }
    logStream.close();
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("refextend")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(DRIVER_CPP)
    subprocess.run(["g++", "-fopenmp", "-std=c++0x", "-O1", "-w", "-include", os.path.join(fx.ROOT, "oracle", "ref_prelude.h"), "-I", REF, src, "-o", exe,
                    "-L", REF_DIR, "-lsage2ref_driver", "-Wl,-rpath," + REF_DIR, "-lz"], check=True)
    return exe


def body(text):
    return text.split("\n", 3)[3]                                                    # (line 2 is the loader's read count, not the file's)


def table_lines(g):
    """the read-to-edge table of the model's graph as the driver prints it; the merged loops are left out on both sides (sage2ov.h: E of a loop)"""
    out = set()
    for (r, q), e in H.read_edge_table(g.parsed()).items():
        E = g.h[2 * q] if g.h[2 * q]["frm"] < g.h[2 * q]["to"] else g.h[2 * q + 1]
        if E["frm"] != E["to"]:
            out.add("t %d %d %d %d %d f%s r%s" % (r, E["frm"], E["to"], E["type"], E["len"], "".join(" %d" % v for v in e["forward"]), "".join(" %d" % v for v in e["reverse"])))
    return out


def run(driver, tmp_path, mode, ctx, k, text, pairs, high):
    """-> (rounds compared, merges in them): the reference's rounds against the model's until a round the model marks outside_reference (or, in mode `whole`,
    with ties at the threshold) -- merges per round, the graph after every round, the read-to-edge table after the first"""
    g = X.Graph(H.parse_graph(text, fold=False)); b = X.Bounds(g, pairs)
    seqs = H.stored_reads(ctx)
    rp, gp, lp, op = (str(tmp_path / n) for n in ("P.reads", "P.graph", "log.txt", "out.graph"))
    ctx.reads_save(rp); open(gp, "w").write(text)
    mfs = []
    for L in sorted(pairs):
        bs, o = H.mates_ascii(pairs[L], seqs); mf = str(tmp_path / ("m%d.fa" % L)); mfs.append(mf)
        open(mf, "w").write("".join(">m%d\n%s\n" % (i, bs[int(o[i]):int(o[i + 1])].tobytes().decode()) for i in range(len(o) - 1)))
    out = subprocess.run([driver, mode, str(k), str(high), rp, gp, lp, op] + mfs, check=True, stdout=subprocess.PIPE, text=True, timeout=300,
                         env=dict(os.environ, OMP_NUM_THREADS="1")).stdout.splitlines()
    assert "x %d" % b.max_upper in out
    ref_rounds = [int(x.split()[2]) for x in out if x.startswith("r ")]
    compared = merged = 0
    for rd, n in enumerate(ref_rounds, 1):
        r = X.round_(g, pairs, b, k, high)
        if r["outside_reference"] or (mode == "whole" and r["ties"]):
            break
        assert n == len(r["merges"]), rd
        assert body(open("%s.%d" % (op, rd)).read()) == body(g.text()), rd
        if rd == 1:
            loops = {(h["frm"], h["to"]) for h in g.h if h["frm"] == h["to"]}
            got = {x for x in out if x.startswith("t ") and (int(x.split()[2]), int(x.split()[3])) not in loops}
            assert got == table_lines(g)
        compared += 1; merged += n
    else:
        assert ref_rounds[-1] == 0                                                   # every round was compared: the reference has reached its fixed point too
    return compared, merged


def host_store(reads_ascii, k):
    bases, off = reads_ascii
    ctx = s2.Context(k, device=-2); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
    return ctx


def hand_store(N):
    rng = np.random.default_rng(5)
    reads = sorted({"".join(rng.choice(list("ACGT"), size=60)) for _ in range(N)}); assert len(reads) == N
    return host_store((np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(), np.arange(0, (N + 1) * 60, 60, dtype=np.uint64)), MS.HAND_K)


@pytest.mark.parametrize("mode", ["whole", "ordered"])
def test_hand_built_graph_with_c_kept(mode, driver, tmp_path):
    """C with flow 2 stays after C.D: no round deletes its in-edge while A.B is listed, and no two supports are equal: the whole of findMatepairSupports is defined"""
    N, header, recs, pairs = MS.hand_support_graph()
    recs[4]["flow"] = recs[5]["flow"] = 2.0
    ctx = hand_store(N)
    assert run(driver, tmp_path, mode, ctx, MS.HAND_K, H.graph_text(header, recs), pairs, 2) == (3, 2)
    ctx.close()


def test_hand_built_graph_up_to_the_undefined_round(driver, tmp_path):
    """the graph as it stands: C.D deletes C while A.B is listed at the node -- the model says so and the comparison ends before it"""
    N, header, recs, pairs = MS.hand_support_graph()
    ctx = hand_store(N)
    assert run(driver, tmp_path, "ordered", ctx, MS.HAND_K, H.graph_text(header, recs), pairs, 2) == (0, 0)
    assert run(driver, tmp_path, "ordered", ctx, MS.HAND_K, H.graph_text(header, recs), pairs, 6) == (1, 0)
    ctx.close()


GOLDEN_HIGH = {"g4_highcopy_k21": 3, "g9_repeats160k_k40": 3}


@pytest.mark.parametrize("name", sorted(GOLDEN_HIGH))
def test_goldens_in_the_defined_order(name, driver, tmp_path):
    m = fx.golden(name); ctx = host_store(fx.make_reads(m["synth"]), m["k"])
    g = MS.with_flows(H.parse_graph(gzip.open(os.path.join(fx.GOLDEN, name + ".graph4.gz")).read(), fold=False), MS.golden_flow)
    text = H.graph_text(g["header"], [r for _, a, b in g["pairs"] for r in (a, b)])
    pairs = MS.golden_mates(g, ctx.reads_stats().unique_reads)
    compared, merged = run(driver, tmp_path, "ordered", ctx, m["k"], text, pairs, GOLDEN_HIGH[name])
    assert compared >= 1 and merged >= 1                                             # at least one round with a merge inside the comparison's domain
    ctx.close()


@pytest.mark.parametrize("seed", [2, 3])
def test_generated_graph_with_hubs_in_the_defined_order(seed, driver, tmp_path):
    case = CG.case_e(seed); N, header, recs = case
    pairs = CG.mates_e(GH.parsed(case), seed, for_reference=True)
    ctx = GH.host_store(N, 100 + seed)
    compared, merged = run(driver, tmp_path, "ordered", ctx, CG.K, H.graph_text(header, recs), pairs, 2)
    assert compared >= 1 and merged >= 1
    ctx.close()
