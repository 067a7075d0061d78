"""The restatement of tests/test_mate_estimate_host.py (and sage2ov_insert_estimate) against the reference itself: MatePair::mapMatePairs, mapReadsToEdges,
mapReadLocations and computeMeanSD (matePair.cpp:125-569) run by the reference's own objects under OMP_NUM_THREADS=1 on a P.reads a device-less context saved and
a graph file its own loader reads (so every record pair is an edge: parse_graph(fold=False)).  Runs only where the reference tree and the objects built from it
(oracle/_ref/) are present.  The driver below is our own text; it includes the reference's headers and links oracle/_ref/libsage2ref_driver.so."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import fixtures as fx
import sage2_amd as s2
import test_mate_estimate_host as H

REF = "/root/reference"
REF_DIR = os.path.join(fx.ROOT, "oracle", "_ref")
REF_LIB = os.path.join(REF_DIR, "libsage2ref_driver.so")
pytestmark = pytest.mark.skipif(not (os.path.isdir(REF) and os.path.exists(REF_LIB)), reason="the reference tree or oracle/_ref/libsage2ref_driver.so is absent")

DRIVER_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include "matePair/matePair.h"
extern ofstream logStream;
extern uint64_t averageReadLength;
int main(int argc, char** argv) {      // <k> <P.reads> <graph file> <log file> <mates.fa of library 1> [<mates.fa of library 2>]
    omp_set_num_threads(1);
    logStream.open(argv[4]);
    ReadLoader* loader = new ReadLoader((uint16_t)atoi(argv[1]));
    loader->loadReadsFromFile(argv[2]);
    OverlapGraph* graph = new OverlapGraph(loader);
    graph->loadOverlapGraphFromFile(argv[3]);
    MatePair* mates = new MatePair(graph, loader);
    for (int lib = 1; 4 + lib < argc; lib++) mates->mapMatePairs(argv[4 + lib], "", lib);
    mates->mapReadsToEdges();
    mates->mapReadLocations();
    for (uint64_t i = 0; i <= loader->numberOfUniqueReads; i++)
        for (ReadToEdgeMap* e = mates->readToEdgeList[i]; e != NULL; e = e->next) {
            printf("e %llu %llu %llu %d %u", (unsigned long long)i, (unsigned long long)e->edge->fromID, (unsigned long long)e->edge->ID, (int)e->edge->typeOfEdge, (unsigned)e->edge->lengthOfEdge);
            for (uint32_t x = 1; e->locationForward != NULL && x <= e->locationForward[0]; x++) printf(" f%d", (int32_t)e->locationForward[x]);
            for (uint32_t x = 1; e->locationReverse != NULL && x <= e->locationReverse[0]; x++) printf(" r%d", (int32_t)e->locationReverse[x]);
            printf("\n");
        }
    for (uint64_t i = 0; i <= loader->numberOfUniqueReads; i++)
        for (MatePairInfo* w = mates->matePairList[i]; w != NULL; w = w->next)
            printf("m %llu %llu %d %d %d %d\n", (unsigned long long)i, (unsigned long long)w->ID, (int)w->type1, (int)w->type2, (int)w->library, (int)w->flag);
    for (int lib = 1; 4 + lib < argc; lib++) {                      // the loop of meanSdEstimation (:265-291) over computeMeanSD
        int mu = 5000, sd = 5000, rmu = 0, rsd = 0;
        for (int i = 1; i <= 10; i++) {
            mates->computeMeanSD(mu, sd, lib, &rmu, &rsd);
            const bool fin = abs(mu - rmu) <= rmu / 100 && abs(sd - rsd) <= rsd / 100;
            mu = rmu; sd = rsd;
            printf("r %d %d %d %d\n", lib, rmu, rsd, (int)fin);
            if (fin) break;
        }
    }
    printf("a %llu\n", (unsigned long long)averageReadLength);
    logStream.close();
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("refestimate")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(DRIVER_CPP)
    subprocess.run(["g++", "-fopenmp", "-std=c++0x", "-O1", "-w", "-include", os.path.join(fx.ROOT, "oracle", "ref_prelude.h"), "-I", REF, src, "-o", exe,
                    "-L", REF_DIR, "-lsage2ref_driver", "-Wl,-rpath," + REF_DIR, "-lz"], check=True)
    return exe


def compare(driver, tmp_path, ctx, k, text, pairs):
    """the reference's table, flags, rounds and "Mate-pairs considered" against the restatement over every record pair of `text`"""
    g = H.parse_graph(text, fold=False); t = H.read_edge_table(g); arl = g["header"][2]
    seqs = H.stored_reads(ctx)
    want_d = {L: H.mate_distances(t, H.mate_entries(pl)) for L, pl in pairs.items()}
    for L in pairs:
        assert H.valid_every_round(want_d[L]), f"library {L}: the reference would divide by zero"
    rp, gp, lp = str(tmp_path / "P.reads"), str(tmp_path / "P.graph"), str(tmp_path / "log.txt")
    ctx.reads_save(rp); open(gp, "w").write(text if isinstance(text, str) else text.decode())
    mfs = []
    for L in sorted(pairs):
        b, o = H.mates_ascii(pairs[L], seqs); mf = str(tmp_path / ("m%d.fa" % L)); mfs.append(mf)
        open(mf, "w").write("".join(">m%d\n%s\n" % (i, b[int(o[i]):int(o[i + 1])].tobytes().decode()) for i in range(len(o) - 1)))
    out = subprocess.run([driver, str(k), rp, gp, lp] + mfs, check=True, stdout=subprocess.PIPE, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="1")).stdout.splitlines()
    # the table: the reference keeps Edge pointers; an entry is named by its read, E's ends, type and length and its locations (the restatement's pair ordinal has no
    # counterpart there), compared as multisets per read
    pair_len = {q: (a["len"] if a["frm"] < a["to"] else b["len"]) for q, a, b in g["pairs"]}
    want = sorted("e %d %d %d %d %d" % (r, w["frm"], w["to"], w["type"], pair_len[q]) + "".join(" f%d" % v for v in w["forward"]) + "".join(" r%d" % v for v in w["reverse"]) for (r, q), w in t.items())
    assert sorted(x for x in out if x.startswith("e ")) == want and len(want) > 0
    theirs = sorted(tuple(int(v) for v in x.split()[1:]) for x in out if x.startswith("m "))
    ours = []
    for L, pl in pairs.items():
        ent = sorted({(a, b, sa, sb) for a, sa, b, sb in pl} | {(b, a, sb, sa) for a, sa, b, sb in pl})
        ours += [(a, b, ta, tb, L, f) for (a, b, ta, tb), f in zip(ent, H.mate_flags(t, [(a, b) for a, b, _, _ in ent]))]
    assert theirs == sorted(ours)
    considered = [int(v) for v in re.findall(r"Mate-pairs considered: (\d+)", open(lp).read())]
    at = 0
    for L in sorted(pairs):
        w = H.estimate(want_d[L], arl); rounds = [tuple(int(v) for v in x.split()[1:]) for x in out if x.startswith("r %d " % L)]
        assert rounds == [(L, m, s, int(i == w["rounds"] - 1 and w["final"])) for i, (m, s) in enumerate(zip(w["mu"], w["sd"]))]
        assert considered[at:at + w["rounds"]] == w["considered"][:w["rounds"]]; at += w["rounds"]
        H.same_estimate(s2.insert_estimate(np.asarray(want_d[L], dtype=np.uint32), arl), w)
    assert at == len(considered) and out[-1] == "a %d" % arl


@pytest.mark.parametrize("name", ["g1_clean100_k21", "g3_noisy_rep_k21", "g4_highcopy_k21", "g7_palindrome_tandem_k21"])
def test_goldens_like_the_reference(name, driver, tmp_path):
    """g7's loop edge stands twice in the file: two edges to the reference's loader, E of each its second record"""
    m = fx.golden(name); bases, off = fx.make_reads(m["synth"])
    ctx = s2.Context(m["k"], device=-2); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
    text = gzip.open(os.path.join(fx.GOLDEN, name + ".graph4.gz")).read()
    g = H.parse_graph(text, fold=False)
    pairs = H.pairs_from_graph(g, 11, ctx.reads_stats().unique_reads)
    if name.startswith("g7"):
        loops = [(q, a) for q, a, b in g["pairs"] if a["frm"] == a["to"]]; assert len(loops) == 2
        on = [e[0] for e in loops[0][1]["list"]]; pairs[1] += [(on[0], 1, on[0], 1)]          # a mate pair on the loop itself
    compare(driver, tmp_path, ctx, m["k"], text, pairs)
    ctx.close()


def test_hand_built_graph_like_the_reference(driver, tmp_path):
    """a read on three pairs, a read twice on one edge, orientation 0, a record that leaves the larger id, loops, two libraries"""
    N, header, recs = H.hand_graph(); text = H.graph_text(header, recs)
    rng = np.random.default_rng(5)
    reads = sorted({"".join(rng.choice(list("ACGT"), size=60)) for _ in range(N)}); assert len(reads) == N
    bases = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(); off = np.arange(0, (N + 1) * 60, 60, dtype=np.uint64)
    ctx = s2.Context(40, device=-2); ctx.reads_add_ascii(bases, off); ctx.reads_organize(); assert ctx.reads_stats().unique_reads == N
    pairs = {1: [(20, 1, 24, 1), (20, 0, 22, 1), (21, 1, 23, 0), (22, 1, 24, 1), (30, 1, 31, 1), (31, 1, 33, 1), (32, 0, 33, 1), (40, 1, 41, 1), (20, 1, 40, 0), (42, 1, 43, 1),
                 (44, 1, 46, 1), (45, 0, 46, 0), (1, 1, 20, 1), (50, 1, 51, 1), (30, 1, 30, 0), (20, 1, 24, 1)],
             2: [(44, 1, 45, 1), (31, 1, 32, 1), (23, 1, 24, 1), (24, 0, 23, 1), (52, 1, 20, 1)]}
    compare(driver, tmp_path, ctx, 40, text, pairs)
    ctx.close()
