"""The restatement of tests/test_links_host.py against the reference itself: the rows ScaffoldMaker::mergeFinal and mergeFinalSmall (matePair/scaffolding.cpp:774-967,
:969-1162) hand to quicksortListOfLongEdges, run by the reference's own objects with one thread on a P.reads a device-less context saved and a graph file its own
loader reads (so every record pair is an edge: parse_graph(fold=False)).  Runs only where the reference tree and the objects built from it (oracle/_ref/) are
present.  The driver below is our own text; it includes the reference's headers and links oracle/_ref/libsage2ref_driver.so.  It defines
ScaffoldMaker::quicksortListOfLongEdges itself -- an ordinary out-of-class member of position-independent objects, so the executable's definition is the one
mergeFinal calls -- prints the rows and does not sort; with highTh = INT_MAX nothing merges and both calls return 0."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import fixtures as fx
import sage2_amd as s2
import test_mate_estimate_host as H
import test_mate_support_host as MS
import test_links_host as LH

REF = "/root/reference"
REF_DIR = os.path.join(fx.ROOT, "oracle", "_ref")
REF_LIB = os.path.join(REF_DIR, "libsage2ref_driver.so")
pytestmark = pytest.mark.skipif(not (os.path.isdir(REF) and os.path.exists(REF_LIB)), reason="the reference tree or oracle/_ref/libsage2ref_driver.so is absent")

DRIVER_CPP = r"""
#include <climits>
#include <cstdio>
#include <cstdlib>
#include "matePair/scaffolding.h"
extern ofstream logStream;
static int phase = 0;
void ScaffoldMaker::quicksortListOfLongEdges(Edge** edge_1, Edge** edge_2, int* pair_support, int32_t* gapDistance, int64_t left, int64_t right) {
    for (int64_t i = left; i <= right; i++) {
        const Edge* a = edge_1[i]->twinEdge; const Edge* b = edge_2[i];
        printf("l %d %llu %llu %d %u %llu %llu %d %u %d %d\n", phase, (unsigned long long)a->fromID, (unsigned long long)a->ID, (int)a->typeOfEdge, (unsigned)a->lengthOfEdge,
               (unsigned long long)b->fromID, (unsigned long long)b->ID, (int)b->typeOfEdge, (unsigned)b->lengthOfEdge, pair_support[i], (int)gapDistance[i]);
    }
}
int main(int argc, char** argv) {      // <k> <P.reads> <graph file> <log file> <mates.fa of library 1> [<mates.fa of library 2>]
    omp_set_num_threads(1);
    logStream.open(argv[4]);
    const uint16_t k = (uint16_t)atoi(argv[1]);
    ReadLoader* loader = new ReadLoader(k);
    loader->loadReadsFromFile(argv[2]);
    OverlapGraph* graph = new OverlapGraph(loader);
    graph->loadOverlapGraphFromFile(argv[3]);
    MatePair* mates = new MatePair(graph, loader);
    for (int lib = 1; 4 + lib < argc; lib++) mates->mapMatePairs(argv[4 + lib], "", lib);
    mates->meanSdEstimation();
    for (int lib = 1; 4 + lib < argc; lib++) printf("u %d %d %d\n", lib, (int)mates->upperBoundOfInsert[lib], (int)mates->Mean[lib]);
    printf("x %llu\n", (unsigned long long)mates->maximumUpperBoundOfInsert);
    ScaffoldMaker* sm = new ScaffoldMaker(graph, mates, loader);
    phase = 1; printf("r 1 %llu\n", (unsigned long long)sm->mergeFinal(k, INT_MAX, 1));
    phase = 2; printf("r 2 %llu\n", (unsigned long long)sm->mergeFinalSmall(k, INT_MAX, 2));
    logStream.close();
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("reflinks")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(DRIVER_CPP)
    subprocess.run(["g++", "-fopenmp", "-std=c++0x", "-O1", "-w", "-include", os.path.join(fx.ROOT, "oracle", "ref_prelude.h"), "-I", REF, src, "-o", exe,
                    "-L", REF_DIR, "-lsage2ref_driver", "-Wl,-rpath," + REF_DIR, "-lz"], check=True)
    return exe


def reference_rows(driver, tmp_path, ctx, k, text, pairs):
    """-> (the driver's output lines, {mode: {(id of a, id of b): (support, gap)}}) of the reference on this graph file and these mates"""
    seqs = H.stored_reads(ctx)
    rp, gp, lp = str(tmp_path / "P.reads"), str(tmp_path / "P.graph"), str(tmp_path / "log.txt")
    ctx.reads_save(rp); open(gp, "w").write(text)
    mfs = []
    for L in sorted(pairs):
        b, o = H.mates_ascii(pairs[L], seqs); mf = str(tmp_path / ("m%d.fa" % L)); mfs.append(mf)
        open(mf, "w").write("".join(">m%d\n%s\n" % (i, b[int(o[i]):int(o[i + 1])].tobytes().decode()) for i in range(len(o) - 1)))
    out = subprocess.run([driver, str(k), rp, gp, lp] + mfs, check=True, stdout=subprocess.PIPE, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="1")).stdout.splitlines()
    rows = {LH.FINAL: {}, LH.SMALL: {}}
    for x in out:
        if x.startswith("l "):
            v = [int(t) for t in x.split()[1:]]
            key = (tuple(v[1:5]), tuple(v[5:9])); assert key not in rows[v[0]]          # each ordered pair at most once
            rows[v[0]][key] = (v[9], v[10])
    return out, rows


def compare(driver, tmp_path, ctx, k, text, pairs):
    """the reference's estimates and the rows of both sweeps against the restatement over every record pair of `text`; -> (restatement rows, reference rows, graph)"""
    g = H.parse_graph(text, fold=False)
    t, ests, (_, hi) = MS.support_inputs(g, pairs)
    for L in sorted(ests):
        assert H.valid_every_round(H.mate_distances(t, H.mate_entries(pairs[L]))), f"library {L}: the reference would divide by zero"
    out, ref = reference_rows(driver, tmp_path, ctx, k, text, pairs)
    assert [x for x in out if x.startswith("u ")] == ["u %d %d %d" % (L, ests[L]["upper"], ests[L]["mean"]) for L in sorted(ests)] and "x %d" % hi in out
    assert "r 1 0" in out and "r 2 0" in out                                           # nothing merged
    rows = LH.links(g, t, pairs, ests, hi, g["header"][2], k)
    LH.same_as_reference(g, rows, ref)
    return rows, ref, g


def host_store(reads_ascii, k):
    bases, off = reads_ascii
    ctx = s2.Context(k, device=-2); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
    return ctx


def leave_different_nodes(g, rows):
    hv = LH.halves_of(g)
    return [r for r in rows if hv[(r[0], r[1])][0]["frm"] != hv[(r[2], r[3])][0]["frm"]]


@pytest.mark.parametrize("variant", [None, 666, 667])
def test_hand_built_graph_like_the_reference(variant, driver, tmp_path):
    N, header, recs, pairs = LH.hand_link_graph(variant, invalid_library=False)      # (library 3 would make the reference divide by zero)
    rng = np.random.default_rng(5)
    reads = sorted({"".join(rng.choice(list("ACGT"), size=60)) for _ in range(N)}); assert len(reads) == N
    ctx = host_store((np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(), np.arange(0, (N + 1) * 60, 60, dtype=np.uint64)), LH.HAND_K)
    assert ctx.reads_stats().unique_reads == N
    rows, ref, g = compare(driver, tmp_path, ctx, LH.HAND_K, H.graph_text(header, recs), pairs)
    d = {r[:4]: r[4:] for r in rows}
    assert d[(LH.qA, 0, LH.qB, 0)][0] == {None: 3, 666: 5, 667: 3}[variant] and (variant is not None or d[(LH.qG, 0, LH.qH, 0)] == (2, -3))
    assert ref[LH.FINAL] and ref[LH.SMALL] and leave_different_nodes(g, rows)
    ctx.close()


def golden_case(name):
    m = fx.golden(name); ctx = host_store(fx.make_reads(m["synth"]), m["k"])
    g = MS.with_flows(H.parse_graph(gzip.open(os.path.join(fx.GOLDEN, name + ".graph4.gz")).read(), fold=False), MS.golden_flow)
    text = H.graph_text(g["header"], [r for _, a, b in g["pairs"] for r in (a, b)])
    pairs = LH.golden_pairs(name, g, ctx.reads_stats().unique_reads)
    return m, ctx, g, text, pairs


@pytest.mark.parametrize("name", ["g4_highcopy_k21", "g9_repeats160k_k40"])
def test_goldens_like_the_reference(name, driver, tmp_path):
    m, ctx, g, text, pairs = golden_case(name)
    rows, ref, g = compare(driver, tmp_path, ctx, m["k"], text, pairs)
    assert ref[LH.FINAL] and ref[LH.SMALL]                                             # (not vacuous: rows under both filters,
    assert leave_different_nodes(g, rows) and any(r[4] >= 3 for r in rows)             # rows whose halves leave different nodes, a support >= 3)
    ctx.close()
