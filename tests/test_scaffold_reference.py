"""The restatement of tests/scaffold_model.py against the reference itself, by the reference's objects with one thread on a P.reads a device-less context saved and
a graph file its own loader reads: OverlapGraph::stringOverlapSize called directly on seeded read pairs, ScaffoldMaker::mergeDisconnectedEdges called on the chosen
reads of the GPU tests (mode `join`), the reference's own mergeFinal / mergeFinalSmall on a freshly loaded graph (mode `whole`), compared where the model says
the round is defined, and the reference's own mergeAccordingToSupport / mergeAccordingToSupport2 handed rows round after round (mode `ordered`).  In mode
`ordered` the rows of rules (a) and (b) are made by the model from its own graph and named to the driver by (from, to, type, length, first list entry); the
driver builds the map and the delete list as scaffolding.cpp:893-916 do and calls the reference's function.  The driver does not rebuild the rows itself: the
link sweep that produces them is compared with the reference's by tests/test_links_reference.py.  Runs only where the reference tree and the objects built from it (oracle/_ref/) are present.  The driver below is our own text; it includes
the reference's headers and links oracle/_ref/libsage2ref_driver.so."""
import os
import subprocess

import numpy as np
import pytest

import fixtures as fx
import sage2_amd as s2
import scaffold_model as SM
import extend_model as X
import test_mate_estimate_host as H
import test_links_host as LH
import test_scaffold_host as SH
import gzip
import compgen as CG
import test_compgen_host as GH
import test_mate_support_host as MS
from test_extend_reference import REF, REF_DIR, REF_LIB, body, hand_store, table_lines

pytestmark = pytest.mark.skipif(not (os.path.isdir(REF) and os.path.exists(REF_LIB)), reason="the reference tree or oracle/_ref/libsage2ref_driver.so is absent")

DRIVER_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include "matePair/scaffolding.h"
extern ofstream logStream;
extern uint64_t averageReadLength;
static Edge* findEdge(OverlapGraph* graph, uint64_t from, uint64_t to, int type, uint64_t len, uint64_t firstRead = 0) {      // firstRead: 2 * read + orientation of the list's first entry (tells a loop's halves apart)
    for (Edge* v = graph->graph[from]; v != NULL; v = v->next)
        if (v->ID == to && v->typeOfEdge == type && v->lengthOfEdge == len && (!firstRead || (v->listOfReads[0].readId > 0 && 2 * (uint64_t)v->listOfReads[1].readId + v->listOfReads[1].orientation == firstRead))) return v;
    return NULL;
}
int main(int argc, char** argv) {      // <overlap|join|whole> <k> <P.reads> <graph file> <log file> <out prefix> <work file> <high> <flag> <small> [<mates.fa> ...]
    omp_set_num_threads(1);
    const std::string mode = argv[1];
    const uint16_t k = (uint16_t)atoi(argv[2]); const int high = atoi(argv[8]), flag = atoi(argv[9]), small = atoi(argv[10]);
    logStream.open(argv[5]);
    ReadLoader* loader = new ReadLoader(k);
    loader->loadReadsFromFile(argv[3]);
    // loadReadsFromFile does not set averageReadLength, and the OverlapGraph constructor takes printGraph's contigLengthThreshold from it (overlapGraph.cpp:32): the
    // graph file's third header line, which the loader reads later, is set first (main.cpp has it from step 1)
    { std::ifstream hd(argv[4]); unsigned long long g0 = 0, n0 = 0, a0 = 0; hd >> g0 >> n0 >> a0; averageReadLength = a0; }
    OverlapGraph* graph = new OverlapGraph(loader);
    graph->loadOverlapGraphFromFile(argv[4]);
    if (mode == "overlap") {                                           // work file: lines "s1 s2"
        std::ifstream in(argv[7]); std::string s1, s2;
        while (in >> s1 >> s2) printf("o %d\n", graph->stringOverlapSize(s1, s2, (int)s1.size(), (int)s2.size()));
        return 0;
    }
    MatePair* mates = new MatePair(graph, loader);
    for (int lib = 1; 10 + lib < argc; lib++) mates->mapMatePairs(argv[10 + lib], "", lib);
    mates->meanSdEstimation();
    ScaffoldMaker* sc = new ScaffoldMaker(graph, mates, loader);
    if (mode == "join") {                                              // work file: lines "from1 to1 type1 len1 from2 to2 type2 len2 gap"
        std::ifstream in(argv[7]); long long f1, t1, y1, l1, f2, t2, y2, l2, gap;
        while (in >> f1 >> t1 >> y1 >> l1 >> f2 >> t2 >> y2 >> l2 >> gap) {
            Edge* a = findEdge(graph, f1, t1, (int)y1, l1); Edge* b = findEdge(graph, f2, t2, (int)y2, l2);
            if (!a || !b) { printf("missing\n"); return 1; }
            Edge* m = sc->mergeDisconnectedEdges(a, b, (int)gap);
            printf("j %llu %llu\n", (unsigned long long)m->lengthOfEdge, (unsigned long long)m->twinEdge->lengthOfEdge);
        }
        graph->saveOverlapGraphInFile(std::string(argv[6]) + ".1");
        return 0;
    }
    if (mode == "ordered") {      // work file: per round "R <rows>" and rows "from1 to1 type1 len1 first1 from2 to2 type2 len2 first2 support gap" in the order of include/sage2ov.h (b)
        std::ifstream in(argv[7]); std::string tag; long long nrows; int round = 0;
        while (in >> tag >> nrows) {
            round++;
            Edge** e1 = (Edge**)malloc((nrows + 1) * sizeof(Edge*)); Edge** e2 = (Edge**)malloc((nrows + 1) * sizeof(Edge*));
            int* sup = (int*)malloc((nrows + 1) * sizeof(int)); int32_t* gp = (int32_t*)malloc((nrows + 1) * sizeof(int32_t));
            unordered_map<pair<uint64_t,uint64_t>,SupportedEdgePair,pairHash> search; unordered_multimap<uint64_t,SupportedEdgePair> del;
            bool ok = true;
            for (long long i = 0; i < nrows; i++) {
                long long f1, t1, y1, l1, r1, f2, t2, y2, l2, r2, s, g; in >> f1 >> t1 >> y1 >> l1 >> r1 >> f2 >> t2 >> y2 >> l2 >> r2 >> s >> g;
                e1[i] = findEdge(graph, f1, t1, (int)y1, l1, r1); e2[i] = findEdge(graph, f2, t2, (int)y2, l2, r2); sup[i] = (int)s; gp[i] = (int32_t)g;
                if (!e1[i] || !e2[i]) { ok = false; continue; }
                SupportedEdgePair p; p.edge1 = e1[i]; p.edge2 = e2[i]; p.support = (int)s;                    // scaffolding.cpp:893-916
                const pair<uint64_t,uint64_t> key(e1[i]->fromID ^ e1[i]->ID, e2[i]->fromID ^ e2[i]->ID);
                auto it = search.find(key);
                if (it == search.end() || (int)s > it->second.support) search[key] = p;
                del.insert({(uint64_t)e1[i]->ID, p}); del.insert({(uint64_t)e1[i]->fromID, p}); del.insert({(uint64_t)e2[i]->ID, p}); del.insert({(uint64_t)e2[i]->fromID, p});
            }
            if (!ok) { printf("missing %d\n", round); break; }
            uint64_t n = 0;
            if (nrows > 0) n = flag == 1 ? sc->mergeAccordingToSupport(e1, e2, sup, gp, nrows, search, del, high) : sc->mergeAccordingToSupport2(e1, e2, sup, gp, nrows, search, del, high);
            printf("r %d %llu\n", round, (unsigned long long)n);
            graph->saveOverlapGraphInFile(std::string(argv[6]) + "." + std::to_string(round));
            if (round == 1)
                for (uint64_t r = 1; r <= loader->numberOfUniqueReads; r++)
                    for (ReadToEdgeMap* e = mates->readToEdgeList[r]; e != NULL; e = e->next) {
                        printf("t %llu %llu %llu %d %u f", (unsigned long long)r, (unsigned long long)e->edge->fromID, (unsigned long long)e->edge->ID, (int)e->edge->typeOfEdge, (unsigned)e->edge->lengthOfEdge);
                        for (uint32_t x = 1; e->locationForward && x <= e->locationForward[0]; x++) printf(" %d", (int)e->locationForward[x]);
                        printf(" r");
                        for (uint32_t x = 1; e->locationReverse && x <= e->locationReverse[0]; x++) printf(" %d", (int)e->locationReverse[x]);
                        printf("\n");
                    }
            free(e1); free(e2); free(sup); free(gp);
        }
        if (small) graph->printGraph(std::string(argv[6]) + "_scaffold", true);      // (`small` doubles as "spell the scaffolds" in this mode: the rows carry the filter already)
        logStream.close();
        return 0;
    }
    // whole: the half-edges' addresses in file order (work file: lines "from to type len", one per record), then rounds
    {
        std::ifstream in(argv[7]); long long f, t, y, l; unsigned long long last = 0; int ascending = 1;
        while (in >> f >> t >> y >> l) { Edge* e = findEdge(graph, f, t, (int)y, l); if (!e) { ascending = 0; break; } if ((unsigned long long)e < last) ascending = 0; last = (unsigned long long)e; }
        printf("a %d\n", ascending);
    }
    for (int round = 1; round <= 3; round++) {
        const uint64_t n = small ? sc->mergeFinalSmall(k, high, flag) : sc->mergeFinal(k, high, flag);
        printf("r %d %llu\n", round, (unsigned long long)n);
        graph->saveOverlapGraphInFile(std::string(argv[6]) + "." + std::to_string(round));
        if (n == 0) break;
    }
    logStream.close();
    return 0;
}
"""


def build_driver(d):
    src, exe = os.path.join(str(d), "driver.cpp"), os.path.join(str(d), "driver")
    open(src, "w").write(DRIVER_CPP)
    subprocess.run(["g++", "-fopenmp", "-std=c++0x", "-O1", "-w", "-include", os.path.join(fx.ROOT, "oracle", "ref_prelude.h"), "-I", REF, src, "-o", exe,
                    "-L", REF_DIR, "-lsage2ref_driver", "-Wl,-rpath," + REF_DIR, "-lz"], check=True)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("refscaffold"))


def call(driver, tmp_path, mode, ctx, k, text, work, high=1, flag=1, small=0, pairs=None):
    rp, gp, lp, op, wp = (str(tmp_path / n) for n in ("P.reads", "P.graph", "log.txt", "out.graph", "work.txt"))
    ctx.reads_save(rp); open(gp, "w").write(text); open(wp, "w").write(work)
    mfs = []; seqs = H.stored_reads(ctx)
    for L in sorted(pairs or {}):
        bs, o = H.mates_ascii(pairs[L], seqs); mf = str(tmp_path / ("m%d.fa" % L)); mfs.append(mf)
        open(mf, "w").write("".join(">m%d\n%s\n" % (i, bs[int(o[i]):int(o[i + 1])].tobytes().decode()) for i in range(len(o) - 1)))
    out = subprocess.run([driver, mode, str(k), rp, gp, lp, op, wp, str(high), str(flag), str(small)] + mfs, check=True, stdout=subprocess.PIPE, text=True, timeout=300,
                         env=dict(os.environ, OMP_NUM_THREADS="1")).stdout.splitlines()
    return out, op, seqs


def unflagged(text):
    """the records with the flag of every list entry set to 0: the reference leaves the flag of the entries a join inserts uninitialised (malloc, overlapGraph.cpp:861-876);
    include/sage2ov.h writes 0"""
    out = []
    for line in body(text).split("\n"):
        f = line.split("\t")
        out.append("\t".join(f[:2] + ["0"] + f[3:]) if len(f) == 5 else line)
    return "\n".join(out)


def tiny():
    """a store and a graph for the calls that need only an OverlapGraph object"""
    header, recs = SH.two_edges(nodes=(1, 2, 3, 4))
    return hand_store(30), H.graph_text(header, recs)


def test_string_overlap_size_on_seeded_pairs(driver, tmp_path):
    """a few hundred pairs with L2 <= L1 (beyond that the reference reads past its string), planted overlaps and none, lengths 11 to 150"""
    rng = np.random.default_rng(23); prs = []
    for n in range(400):
        L1 = int(rng.integers(11, 151)); L2 = int(rng.integers(11, L1 + 1))
        s2_ = SH.rnd(L2, 30000 + n)
        if n % 3 == 0 or L1 < 13:
            s1 = SH.rnd(L1, 31000 + n)
        else:
            sh = int(rng.integers(0, L1 - 10)); bodyl = list((s2_ + SH.rnd(L1, 32000 + n))[:L1])
            for x in rng.integers(0, max(1, min(L1 - sh, L2)), size=int(rng.integers(0, 9))):
                bodyl[int(x)] = SH.other(bodyl[int(x)])
            s1 = (SH.rnd(sh, 33000 + n) + "".join(bodyl))[:L1]
        prs.append((s1, s2_))
    for L in SH.LENGTHS:                                                               # and the pinned cases of equal length
        shift = min(max(1, (L - 10) // 2), L - 11); allowed = (L - shift) // 10 + 1
        prs += [SH.planted(L, L, shift, allowed, 100 + L), SH.planted(L, L, shift, allowed + 1, 100 + L), SH.planted(L, L, L - 11, 2, 200 + L), SH.planted(L, L, L - 11, 3, 200 + L)]
    prs += [("T" * 40, "ACGTACGTACGT"), ("G" * 40, "A" * 12), ("C" * 22, "A" * 12), ("C" * 21, "A" * 12)]
    ctx, text = tiny()
    out, _, _ = call(driver, tmp_path, "overlap", ctx, LH.HAND_K, text, "".join("%s %s\n" % p for p in prs))
    got = [int(x.split()[1]) for x in out if x.startswith("o ")]
    want = [SM.overlap_size(a, b) for a, b in prs]
    assert got == want and sum(v > 0 for v in want) > 100 and sum(v == -1 for v in want) > 50
    ctx.close()


def long_seeded_pairs():
    """150 pairs with L1 in [252, 1018] and L2 <= L1: every second pair of equal lengths (a shorter s2 always passes on a tail of a few bases; -1 needs s2 to reach
    s1's end), every tenth with s1 of 990 bases and more and its shift in the last lane round; planted with 0 to 8 flipped bases, or random"""
    rng = np.random.default_rng(29); prs = []
    for n in range(150):
        L1 = int(rng.integers(990, 1019)) if n % 10 == 0 else int(rng.integers(252, 1019)); L2 = L1 if n % 2 or n % 10 == 0 else int(rng.integers(11, L1 + 1))
        s2_ = SH.rnd(L2, 40000 + n)
        if n % 3 == 1 and n % 10:
            s1 = SH.rnd(L1, 41000 + n)
        else:
            sh = int(rng.integers(960 if n % 10 == 0 else 0, L1 - 10)); bodyl = list((s2_ + SH.rnd(L1, 42000 + n))[:L1])
            for x in rng.integers(0, max(1, min(L1 - sh, L2)), size=int(rng.integers(0, 9))):
                bodyl[int(x)] = SH.other(bodyl[int(x)])
            s1 = (SH.rnd(sh, 43000 + n) + "".join(bodyl))[:L1]
        prs.append((s1, s2_))
    return prs


def test_string_overlap_size_on_the_long_layouts(driver, tmp_path):
    """the model at the lengths of the 16- and 32-word read layouts, 252 to 1018 bases: every long pinned case of tests/test_scaffold_host.py with L2 <= L1 (beyond
    that the reference reads past its string) and 150 seeded pairs.  The counts are conditions on what the model alone says"""
    pinned = [c for top in sorted(SH.LONG_TOPS) for c in SH.pinned_cases_long(top=top) if len(c[1]) <= len(c[0])]
    prs = [(a, b) for a, b, _ in pinned] + long_seeded_pairs()
    want = [SM.overlap_size(a, b) for a, b in prs]
    assert want[:len(pinned)] == [w for _, _, w in pinned] and len(pinned) == 6 * len(SH.LONG_LENGTHS) + 2 * (2 + 4) and len(prs) == len(pinned) + 150
    assert all(252 <= len(a) <= 1018 and len(b) <= len(a) for a, b in prs)
    seeded = want[len(pinned):]
    assert sum(v > 0 for v in want) > 50 and sum(v == -1 for v in want) > 20 and sum(v >= 960 for v in want) >= 5
    assert sum(v > 0 for v in seeded) > 50 and sum(v == -1 for v in seeded) > 20 and sum(v >= 960 for v in seeded) >= 5      # (the seeded pairs meet them on their own)
    ctx, text = tiny()
    out, _, _ = call(driver, tmp_path, "overlap", ctx, LH.HAND_K, text, "".join("%s %s\n" % p for p in prs))
    got = [int(x.split()[1]) for x in out if x.startswith("o ")]
    assert got == want
    ctx.close()


def test_merge_disconnected_edges_on_chosen_reads(driver, tmp_path):
    """the pinned cases of the GPU test as two-edge components over a store of exactly those reads; only pairs of equal read length, since of two unequal reads one
    direction has L2 > L1; gaps negative, zero, positive and beyond the 11-bit field"""
    G = SH
    cases = [c for c in G.pinned_cases() if len(c[0]) == len(c[1])]; strings = G.distinct(cases)
    fillers = [SH.rnd(60, 5000 + i) for i in range(5 * len(cases))]
    reads = sorted(set(list(strings) + fillers))
    bases = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(); off = np.zeros(len(reads) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(r) for r in reads])
    ctx = s2.Context(10, device=-2); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
    seqs = H.stored_reads(ctx); where = {}
    for i, s in seqs.items():
        where[SM.revcomp(s)] = (i, False)
    for i, s in seqs.items():
        where[s] = (i, True)
    header = (0, len(reads), 60)
    recs = G.components([(s1, s2_, (1, 2, 0.5)[n % 3], (3, 1)[n % 2], n) for n, (s1, s2_, _) in enumerate(cases)], where, [where[x][0] for x in fillers])
    text = H.graph_text(header, recs)
    g = SM.Graph(H.parse_graph(text, fold=False))
    gaps = [(-3, 0, 5, 2000)[n % 4] for n in range(len(cases))]
    work = ""; lens = []
    for n, gap in enumerate(gaps):
        a, b = g.h[4 * n], g.h[4 * n + 2]
        work += "%d %d %d %d %d %d %d %d %d\n" % (a["frm"], a["to"], a["type"], a["len"], b["frm"], b["to"], b["type"], b["len"], gap)
    out, op, _ = call(driver, tmp_path, "join", ctx, 10, text, work)
    for n, gap in enumerate(gaps):
        nh = g.join(4 * n, 4 * n + 2, gap, seqs); lens.append("j %d %d" % (g.h[nh]["len"], g.h[nh + 1]["len"]))
    assert [x for x in out if x.startswith("j ")] == lens
    assert unflagged(open(op + ".1").read()) == unflagged(g.text())
    ctx.close()


@pytest.mark.parametrize("high,flag,small,flows", [(2, 1, 0, {2: 2}), (3, 2, 0, {2: 2, 3: 3})])
def test_merge_final_on_the_freshly_loaded_hand_graph(high, flag, small, flows, driver, tmp_path):
    """the reference's own round on the hand-built link graph (flows: C, and D, above 1 so that the join at node 10 keeps its operands): the joins of round 1 and
    the graph after it.  Every input has to lie inside the contract's domain: Edge objects ascending in file order (rule (a)), no tie at or above the threshold
    (rule (b)), not outside the reference (rule (d)), and at least one join"""
    N, header, recs, pairs, _ = SH.hand(flows=flows)
    pairs = {L: pl for L, pl in pairs.items() if L in (1, 2)}                          # (the invalid library has no distance: the reference divides by zero there)
    ctx = hand_store(N); text = H.graph_text(header, recs)
    g = SM.Graph(H.parse_graph(text, fold=False)); b = X.Bounds(g, pairs)
    work = "".join("%d %d %d %d\n" % (h["frm"], h["to"], h["type"], h["len"]) for h in g.h)
    out, op, seqs = call(driver, tmp_path, "whole", ctx, LH.HAND_K, text, work, high, flag, small, pairs)
    ref_rounds = [int(x.split()[2]) for x in out if x.startswith("r ")]
    r = SM.round_(g, pairs, b, LH.HAND_K, high, flag, bool(small), seqs)
    assert "a 1" in out and not r["ties"] and not r["outside_reference"] and len(r["merges"]) >= 1
    assert ref_rounds[0] == len(r["merges"]) and unflagged(open(op + ".1").read()) == unflagged(g.text())
    ctx.close()


# ------------------------------------------------------------------------------------------ mode `ordered`
GOLDEN_CASES = {"hand_flag2": (1, 2, False, "ALL50"), "hand_flag1": (2, 1, False, "C2"), "hand_small": (1, 2, True, "ALL50")}      # tests/golden/scaffold/<name>.json.gz


def golden_case(name):
    """(N, header, records, pairs, high, flag, small) of a case tools/make_golden_scaffold.py records"""
    high, flag, small, fl = GOLDEN_CASES[name]
    N, header, recs, pairs, _ = SH.hand(flows={q: 50 for q in range(13)} if fl == "ALL50" else {2: 2})
    return N, header, recs, {L: pl for L, pl in pairs.items() if L in (1, 2)}, high, flag, small

def ordered(driver, tmp_path, ctx, k, text, pairs, high, flag, small=False, max_rounds=6, fasta=False):
    """the reference's own mergeAccordingToSupport (flag 1) / mergeAccordingToSupport2 (flag 2) handed, round after round, the rows of rule (a) in order (b) as the
    model makes them from its own graph, which is the reference's as long as the rounds agree.  Compared: joins per round, the graph after every round, the
    read-to-edge table after the first -- up to the first round the model marks outside_reference.  The first round has to join and to be inside the reference.
    -> (rounds compared, joins in them, model results of those rounds)"""
    g = SM.Graph(H.parse_graph(text, fold=False)); b = X.Bounds(g, pairs); seqs = H.stored_reads(ctx)
    work = ""; want = []
    for rd in range(max_rounds):
        alive_ids = [(h["frm"], h["to"], h["type"], h["len"], 2 * h["list"][0][0] + h["list"][0][1]) for x, h in enumerate(g.h) if g.alive[x >> 1] and h["list"]]
        r = SM.round_(g, pairs, b, k, high, flag, small, seqs)
        if r["outside_reference"]:
            break
        used = {i for row in r["row_list"] for i in row[:2]}
        assert all(alive_ids.count(i) == 1 for i in used)                              # (from, to, type, length, first read of the list) names one half
        work += "R %d\n" % len(r["row_list"]) + "".join("%d %d %d %d %d %d %d %d %d %d %d %d\n" % (a + c + (s_, gp)) for a, c, s_, gp in r["row_list"])
        want.append((r, unflagged(g.text()), table_lines(g) if rd == 0 else None))
        if not r["merges"]:
            break
    assert want and len(want[0][0]["merges"]) >= 1                                     # a condition, not a measurement
    out, op, _ = call(driver, tmp_path, "ordered", ctx, k, text, work, high, flag, 1 if fasta else 0, pairs)
    assert not any(x.startswith("missing") for x in out)
    ref_rounds = [int(x.split()[2]) for x in out if x.startswith("r ")]
    assert len(ref_rounds) == len(want)
    for rd, (r, txt, tab) in enumerate(want, 1):
        assert ref_rounds[rd - 1] == len(r["merges"]), rd
        assert unflagged(open("%s.%d" % (op, rd)).read()) == txt, rd
        if tab is not None:
            # entries on a loop are left out on both sides, as in test_extend_reference: the reference's table names the forward half of a loop as E, the contract
            # (include/sage2ov.h, the read-to-edge table) the half with the higher index, so the locations stand under `forward` there and `reverse` here
            loops = {(h["frm"], h["to"]) for h in g.h if h["frm"] == h["to"]}
            got = {x for x in out if x.startswith("t ") and (int(x.split()[2]), int(x.split()[3])) not in loops}
            assert got == tab
    return len(want), sum(len(r["merges"]) for r, _, _ in want), [r for r, _, _ in want], op, g


ALL50 = {q: 50 for q in range(13)}                                                 # every pair of the hand graph kept however often it is named


def with_flow(recs, f):
    for r in recs:
        r["flow"] = float(f)
    return recs


@pytest.mark.parametrize("high,flag,small,flows", [(2, 1, False, {2: 2}), (1, 1, False, {2: 2}), (1, 2, False, ALL50), (1, 2, True, ALL50), (3, 2, False, {2: 2, 3: 3})])
def test_ordered_hand_graph_and_variants(high, flag, small, flows, driver, tmp_path):
    N, header, recs, pairs, _ = SH.hand(flows=flows)
    pairs = {L: pl for L, pl in pairs.items() if L in (1, 2)}
    ctx = hand_store(N)
    compared, joined, _, _, _ = ordered(driver, tmp_path, ctx, LH.HAND_K, H.graph_text(header, recs), pairs, high, flag, small)
    assert compared >= 1 and joined >= 1
    ctx.close()


@pytest.mark.parametrize("seed,high,flag,small", [(2, 1, 2, False), (2, 2, 1, False), (3, 1, 2, True), (3, 1, 1, False)])
def test_ordered_generated_graphs_with_hubs(seed, high, flag, small, driver, tmp_path):
    """every edge with flow 2 (flag 2, which names kept operands more often: 50): no join of round 1 deletes an operand, so the round lies inside the reference and kept operands are named again (hypothesis (c) and rule
    (e) decide what becomes of those rows); cycles, blocked rows and rows whose fate the pointer-identity exclusion decides are asserted to occur"""
    case = CG.case_e(seed); N, header, recs = case
    recs = with_flow(recs, 2 if flag == 1 else 50)
    parsed = H.parse_graph(H.graph_text(header, recs), fold=False)
    pairs = LH.merged(CG.mates_e(parsed, seed, for_reference=True), LH.long_range_mates(parsed))
    ctx = GH.host_store(N, 100 + seed)
    compared, joined, rs, _, _ = ordered(driver, tmp_path, ctx, CG.K, H.graph_text(header, recs), pairs, high, flag, small)
    assert compared >= 1 and joined >= 1
    # what the compared rounds held (the model alone says so: not vacuous): cycles, rows refused for their competitors, rows whose fate the pointer-identity
    # exclusion decides, and under flag 2 kept operands named again
    assert sum(r["cycles"] for r in rs) >= 1 and sum(r["blocked"] for r in rs) >= 1 and sum(r["identity_decides"] for r in rs) >= 1
    assert flag == 1 or sum(r["named_again"] for r in rs) >= 3
    ctx.close()


GOLDEN_HIGH = {"g4_highcopy_k21": 2, "g9_repeats160k_k40": 1}


@pytest.mark.parametrize("name", sorted(GOLDEN_HIGH))
def test_ordered_goldens_with_long_range_mates(name, driver, tmp_path):
    from test_extend_reference import host_store
    m = fx.golden(name); ctx = host_store(fx.make_reads(m["synth"]), m["k"])
    g = MS.with_flows(H.parse_graph(gzip.open(os.path.join(fx.GOLDEN, name + ".graph4.gz")).read(), fold=False), lambda q, a: (2.0, 2.0))
    recs = with_flow([r for _, a, b_ in g["pairs"] for r in (a, b_)], 2)
    text = H.graph_text(g["header"], recs)
    parsed = H.parse_graph(text, fold=False)
    pairs = LH.merged(MS.golden_mates(parsed, ctx.reads_stats().unique_reads), LH.long_range_mates(parsed))
    compared, joined, rs, _, _ = ordered(driver, tmp_path, ctx, m["k"], text, pairs, GOLDEN_HIGH[name], 1, False, max_rounds=3)
    assert compared >= 1 and joined >= 1
    ctx.close()
