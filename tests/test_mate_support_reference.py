"""The restatement of tests/test_mate_support_host.py against the reference itself: ContigExtender::getSupportOfEdges (matePair/mergeContigs.cpp:1032-1097) for every
incoming x outgoing pair that findMatepairSupports (:970-989) would try, zeros included, run by the reference's own objects with one thread on a P.reads a
device-less context saved and a graph file its own loader reads (so every record pair is an edge: parse_graph(fold=False)).  Runs only where the reference tree and
the objects built from it (oracle/_ref/) are present.  The driver below is our own text; it includes the reference's headers and links
oracle/_ref/libsage2ref_driver.so."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import fixtures as fx
import sage2_amd as s2
import test_mate_estimate_host as H
import test_mate_support_host as MS

REF = "/root/reference"
REF_DIR = os.path.join(fx.ROOT, "oracle", "_ref")
REF_LIB = os.path.join(REF_DIR, "libsage2ref_driver.so")
pytestmark = pytest.mark.skipif(not (os.path.isdir(REF) and os.path.exists(REF_LIB)), reason="the reference tree or oracle/_ref/libsage2ref_driver.so is absent")

DRIVER_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include <deque>
#include "matePair/mergeContigs.h"
extern ofstream logStream;
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
    ContigExtender* ext = new ContigExtender(graph, mates, loader);
    for (int lib = 1; 4 + lib < argc; lib++) printf("u %d %d\n", lib, (int)mates->upperBoundOfInsert[lib]);
    printf("x %llu\n", (unsigned long long)mates->maximumUpperBoundOfInsert);
    for (uint64_t i = 1; i <= loader->numberOfUniqueReads; i++) {
        if (graph->graph[i] == NULL) continue;
        std::deque<Edge*> ins, outs;                                  // the halves leaving i, as mergeContigs.cpp:977-986 sorts them (an in-edge is the twin of `in`)
        for (Edge* v = graph->graph[i]; v != NULL; v = v->next)
            if (v->flow >= 1 && v->listOfReads[0].readId > 0 && v->ID != v->fromID) { if (v->typeOfEdge == 0 || v->typeOfEdge == 1) ins.push_back(v); else outs.push_back(v); }
        for (size_t a = 0; a < ins.size(); a++)
            for (size_t b = 0; b < outs.size(); b++)
                printf("s %llu %llu %d %u %llu %d %u %d\n", (unsigned long long)i, (unsigned long long)ins[a]->ID, (int)ins[a]->typeOfEdge, (unsigned)ins[a]->lengthOfEdge,
                       (unsigned long long)outs[b]->ID, (int)outs[b]->typeOfEdge, (unsigned)outs[b]->lengthOfEdge, ext->getSupportOfEdges(ins[a], outs[b], k));
    }
    logStream.close();
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("refsupport")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(DRIVER_CPP)
    subprocess.run(["g++", "-fopenmp", "-std=c++0x", "-O1", "-w", "-include", os.path.join(fx.ROOT, "oracle", "ref_prelude.h"), "-I", REF, src, "-o", exe,
                    "-L", REF_DIR, "-lsage2ref_driver", "-Wl,-rpath," + REF_DIR, "-lz"], check=True)
    return exe


def compare(driver, tmp_path, ctx, k, text, pairs):
    """the reference's upper bounds and every in x out support against the restatement over every record pair of `text`; -> the restatement's rows"""
    g = H.parse_graph(text, fold=False)
    t, ests, (_, hi) = MS.support_inputs(g, pairs)
    for L in sorted(ests):
        assert H.valid_every_round(H.mate_distances(t, H.mate_entries(pairs[L]))), f"library {L}: the reference would divide by zero"
    seqs = H.stored_reads(ctx)
    rp, gp, lp = str(tmp_path / "P.reads"), str(tmp_path / "P.graph"), str(tmp_path / "log.txt")
    ctx.reads_save(rp); open(gp, "w").write(text)
    mfs = []
    for L in sorted(pairs):
        b, o = H.mates_ascii(pairs[L], seqs); mf = str(tmp_path / ("m%d.fa" % L)); mfs.append(mf)
        open(mf, "w").write("".join(">m%d\n%s\n" % (i, b[int(o[i]):int(o[i + 1])].tobytes().decode()) for i in range(len(o) - 1)))
    out = subprocess.run([driver, str(k), rp, gp, lp] + mfs, check=True, stdout=subprocess.PIPE, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="1")).stdout.splitlines()
    assert [x for x in out if x.startswith("u ")] == ["u %d %d" % (L, ests[L]["upper"]) for L in sorted(ests)] and "x %d" % hi in out
    by_q = {q: (a, b) for q, a, b in g["pairs"]}
    half = lambda q, i: next(h for h in by_q[q] if h["frm"] == i)
    rows = MS.supports(g, t, pairs, ests, hi, g["header"][2], k)
    want = sorted("s %d %d %d %d %d %d %d %d" % (i, half(qa, i)["to"], half(qa, i)["type"], half(qa, i)["len"], half(qb, i)["to"], half(qb, i)["type"], half(qb, i)["len"], s)
                  for (i, qa, qb, s) in rows)
    assert sorted(x for x in out if x.startswith("s ")) == want
    return rows


def host_store(reads_ascii, k):
    bases, off = reads_ascii
    ctx = s2.Context(k, device=-2); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
    return ctx


@pytest.mark.parametrize("variant", [None, 885, 886])
def test_hand_built_graph_like_the_reference(variant, driver, tmp_path):
    N, header, recs, pairs = MS.hand_support_graph(variant)
    rng = np.random.default_rng(5)
    reads = sorted({"".join(rng.choice(list("ACGT"), size=60)) for _ in range(N)}); assert len(reads) == N
    ctx = host_store((np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(), np.arange(0, (N + 1) * 60, 60, dtype=np.uint64)), MS.HAND_K)
    assert ctx.reads_stats().unique_reads == N
    rows = compare(driver, tmp_path, ctx, MS.HAND_K, H.graph_text(header, recs), pairs)
    assert sorted(r[3] for r in rows) == sorted([{None: 3, 885: 7, 886: 5}[variant], 0, 1, 5])
    ctx.close()


@pytest.mark.parametrize("name", ["g4_highcopy_k21", "g9_repeats160k_k40"])
def test_goldens_like_the_reference(name, driver, tmp_path):
    m = fx.golden(name); ctx = host_store(fx.make_reads(m["synth"]), m["k"])
    g = MS.with_flows(H.parse_graph(gzip.open(os.path.join(fx.GOLDEN, name + ".graph4.gz")).read(), fold=False), MS.golden_flow)
    text = H.graph_text(g["header"], [r for _, a, b in g["pairs"] for r in (a, b)])
    pairs = MS.golden_mates(g, ctx.reads_stats().unique_reads)
    rows = compare(driver, tmp_path, ctx, m["k"], text, pairs)
    assert any(r[3] >= 2 for r in rows) and any(r[3] == 0 for r in rows)            # (not vacuous)
    ctx.close()
