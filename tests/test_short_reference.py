"""The restatement of tests/short_model.py against the reference itself, by the reference's objects with one thread on a P.reads a device-less context saved and a
graph file its own loader reads: ContigExtender::mergeShortOverlaps round after round on a freshly loaded graph (mode `whole`), compared where the model says the
round is defined (outside_reference 0, no ties), and ContigExtender::mergeShortOverlap handed the model's rows round after round (mode `ordered`), where every row the
reference is given and every join it makes has to be the model's.  In mode `ordered` the rows are named to the driver by (from, to, type, length, first list entry);
the driver builds the map and the delete list as mergeContigs.cpp:1593-1616 do and calls the reference's function.  Also checked here, on the CPU: the three
conditions under which tools/make_golden_short.py's cases were chosen.  Runs only where the reference tree and the objects built from it (oracle/_ref/) are present.
The driver below is our own text; it includes the reference's headers and links oracle/_ref/libsage2ref_driver.so."""
import gzip
import os
import subprocess

import pytest

import fixtures as fx
import scaffold_model as SM
import short_model as SO
import extend_model as X
import test_mate_estimate_host as H
import test_mate_support_host as MS
import test_links_host as LH
import test_scaffold_host as SH
import test_short_host as TH
import compgen as CG
import test_compgen_host as GH
from test_extend_reference import REF, REF_DIR, REF_LIB, hand_store, host_store, table_lines
from test_scaffold_reference import call, unflagged, with_flow

pytestmark = pytest.mark.skipif(not (os.path.isdir(REF) and os.path.exists(REF_LIB)), reason="the reference tree or oracle/_ref/libsage2ref_driver.so is absent")

DRIVER_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include "matePair/mergeContigs.h"
extern ofstream logStream;
extern uint64_t averageReadLength;
static Edge* findEdge(OverlapGraph* graph, uint64_t from, uint64_t to, int type, uint64_t len, uint64_t firstRead = 0) {      // firstRead: 2 * read + orientation of the list's first entry (tells a loop's halves apart)
    for (Edge* v = graph->graph[from]; v != NULL; v = v->next)
        if (v->ID == to && v->typeOfEdge == type && v->lengthOfEdge == len && (!firstRead || (v->listOfReads[0].readId > 0 && 2 * (uint64_t)v->listOfReads[1].readId + v->listOfReads[1].orientation == firstRead))) return v;
    return NULL;
}
int main(int argc, char** argv) {      // <whole|ordered> <k> <P.reads> <graph file> <log file> <out prefix> <work file> <high> <unused> <spell the contigs> [<mates.fa> ...]
    omp_set_num_threads(1);
    const std::string mode = argv[1];
    const uint16_t k = (uint16_t)atoi(argv[2]); const int high = atoi(argv[8]), spell = atoi(argv[10]);
    logStream.open(argv[5]);
    ReadLoader* loader = new ReadLoader(k);
    loader->loadReadsFromFile(argv[3]);
    // loadReadsFromFile does not set averageReadLength; the constructors of OverlapGraph and ContigExtender take their contigLengthThreshold from it (overlapGraph.cpp:32,
    // mergeContigs.cpp:21): the graph file's third header line, which the loader reads later, is set first (main.cpp has it from step 1)
    { std::ifstream hd(argv[4]); unsigned long long g0 = 0, n0 = 0, a0 = 0; hd >> g0 >> n0 >> a0; averageReadLength = a0; }
    OverlapGraph* graph = new OverlapGraph(loader);
    graph->loadOverlapGraphFromFile(argv[4]);
    MatePair* mates = new MatePair(graph, loader);
    for (int lib = 1; 10 + lib < argc; lib++) mates->mapMatePairs(argv[10 + lib], "", lib);
    mates->meanSdEstimation();
    ContigExtender* ex = new ContigExtender(graph, mates, loader);
    if (mode == "ordered") {      // work file: per round "R <rows>" and rows "from1 to1 type1 len1 first1 from2 to2 type2 len2 first2 support gap" in the model's order
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
                SupportedEdgePair p; p.edge1 = e1[i]; p.edge2 = e2[i]; p.support = (int)s;                    // mergeContigs.cpp:1593-1616
                const pair<uint64_t,uint64_t> key(e1[i]->fromID ^ e1[i]->ID, e2[i]->fromID ^ e2[i]->ID);
                auto it = search.find(key);
                if (it == search.end() || (int)s > it->second.support) search[key] = p;
                del.insert({(uint64_t)e1[i]->ID, p}); del.insert({(uint64_t)e1[i]->fromID, p}); del.insert({(uint64_t)e2[i]->ID, p}); del.insert({(uint64_t)e2[i]->fromID, p});
            }
            if (!ok) { printf("missing %d\n", round); break; }
            uint64_t n = 0;
            if (nrows > 0) n = ex->mergeShortOverlap(e1, e2, sup, gp, nrows, search, del, high);
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
        if (spell) graph->printGraph(std::string(argv[6]) + "_contig", false);
        logStream.close();
        return 0;
    }
    // whole: do the half-edges' addresses ascend in file order (work file: lines "from to type len first", one per record)?  Then the reference's own rounds
    {
        std::ifstream in(argv[7]); long long f, t, y, l, fr; unsigned long long last = 0; int ascending = 1;
        while (in >> f >> t >> y >> l >> fr) { Edge* e = findEdge(graph, f, t, (int)y, l, fr); if (!e) { ascending = 0; break; } if ((unsigned long long)e < last) ascending = 0; last = (unsigned long long)e; }
        printf("a %d\n", ascending);
    }
    for (int round = 1; round <= 6; round++) {
        const uint64_t n = ex->mergeShortOverlaps(k, high);
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
    return build_driver(tmp_path_factory.mktemp("refshort"))


def half_id(h):
    return (h["frm"], h["to"], h["type"], h["len"], 2 * h["list"][0][0] + h["list"][0][1] if h["list"] else 0)      # (0: an edge without a list, named by its first four)


def two_libraries(pairs):
    return {L: pl for L, pl in pairs.items() if L in (1, 2)}                           # (the invalid library has no distance: the reference divides by zero there)


# ------------------------------------------------------------------------------------------ mode `whole`
@pytest.mark.parametrize("high,names,kw", [(2, TH.ALL, dict(flows=TH.C2)), (1, TH.ALL, dict(flows=TH.C2)), (2, ["plus", "minus"], dict(flows=TH.C2)), (1, ["zero", "twin"], dict(flows=SH.KEPT)),
                                           (1, [], SH.CYCLE), (3, ["minus", "chain"], dict(flows=TH.C2))])
def test_merge_short_overlaps_on_the_freshly_loaded_hand_graphs(high, names, kw, driver, tmp_path):
    """the reference's own rounds, sweep and sort included, on the hand-built link graph with components: the joins of every round and the graph after it.  Every
    compared round has to lie inside the contract's domain: Edge objects ascending in file order (rule (a)), no tie at or above the threshold (rule (b)), not outside
    the reference (rule (d))"""
    N, header, recs, pairs, _ = TH.short_graph(names, **kw)
    pairs = two_libraries(pairs)
    ctx = hand_store(N); text = H.graph_text(header, recs)
    g = SM.Graph(H.parse_graph(text, fold=False)); b = X.Bounds(g, pairs)
    work = "".join("%d %d %d %d %d\n" % half_id(h) for h in g.h)
    out, op, seqs = call(driver, tmp_path, "whole", ctx, TH.K, text, work, high, 0, 0, pairs)
    ref_rounds = [int(x.split()[2]) for x in out if x.startswith("r ")]
    assert "a 1" in out
    compared = 0
    for rd, n in enumerate(ref_rounds, 1):
        r = SO.round_(g, pairs, b, TH.K, high, seqs)
        if r["ties"] or r["outside_reference"]:
            break
        assert n == len(r["merges"]) and unflagged(open("%s.%d" % (op, rd)).read()) == unflagged(g.text()), rd
        compared += 1
    # the rounds are compared up to the first the model marks as outside the reference (a join that deletes edge_1 while rows filed under its node are listed);
    # the first round is always inside, and joins wherever a component was added
    assert compared >= 1 and ref_rounds[-1] == 0 and (ref_rounds[0] >= 1) == (names != [])
    ctx.close()


# ------------------------------------------------------------------------------------------ mode `ordered`
def ordered(driver, tmp_path, ctx, k, text, pairs, high, max_rounds=6, fasta=False):
    """the reference's own mergeShortOverlap handed, round after round, the model's rows in the model's order, made from the model's own graph, which is the
    reference's as long as the rounds agree.  Compared: joins per round, the graph after every round, the read-to-edge table after the first -- up to the first
    round the model marks outside_reference.  -> (rounds compared, joins in them, model results of those rounds, out prefix, the model's graph)"""
    g = SM.Graph(H.parse_graph(text, fold=False)); b = X.Bounds(g, pairs); seqs = H.stored_reads(ctx)
    work = ""; want = []
    for rd in range(max_rounds):
        alive_ids = [half_id(h) for x, h in enumerate(g.h) if g.alive[x >> 1] and h["list"]]
        ids = {x: half_id(h) for x, h in enumerate(g.h) if g.alive[x >> 1] and h["list"]}
        r = SO.round_(g, pairs, b, k, high, seqs)
        if r["outside_reference"]:
            break
        assert all(alive_ids.count(ids[x]) == 1 for row in r["row_list"] for x in row[:2])      # (from, to, type, length, first read of the list) names one half
        work += "R %d\n" % len(r["row_list"]) + "".join("%d %d %d %d %d %d %d %d %d %d %d %d\n" % (ids[e1] + ids[e2] + (s_, gp)) for e1, e2, s_, gp, _ in r["row_list"])
        want.append((r, unflagged(g.text()), table_lines(g) if rd == 0 else None))
        if not r["merges"]:
            break
    assert want
    out, op, _ = call(driver, tmp_path, "ordered", ctx, k, text, work, high, 0, 1 if fasta else 0, pairs)
    assert not any(x.startswith("missing") for x in out)
    ref_rounds = [int(x.split()[2]) for x in out if x.startswith("r ")]
    assert len(ref_rounds) == len(want)
    for rd, (r, txt, tab) in enumerate(want, 1):
        assert ref_rounds[rd - 1] == len(r["merges"]), rd
        assert unflagged(open("%s.%d" % (op, rd)).read()) == txt, rd
        if tab is not None:
            loops = {(h["frm"], h["to"]) for h in g.h if h["frm"] == h["to"]}           # (entries on a loop are left out on both sides, as in tests/test_scaffold_reference.py)
            got = {x for x in out if x.startswith("t ") and (int(x.split()[2]), int(x.split()[3])) not in loops}
            assert got == tab
    return len(want), sum(len(r["merges"]) for r, _, _ in want), [r for r, _, _ in want], op, g


@pytest.mark.parametrize("high,names,kw", [(2, TH.ALL, dict(flows=TH.C2)), (1, TH.ALL, dict(flows=TH.C2)), (1, ["zero", "twin"], dict(flows=SH.KEPT)), (1, ["chain", "minus"], SH.CYCLE),
                                           (2, ["chain", "minus"], dict(flows=SH.KEPT))])
def test_ordered_hand_graphs(high, names, kw, driver, tmp_path):
    N, header, recs, pairs, _ = TH.short_graph(names, **kw)
    ctx = hand_store(N)
    compared, joined, rs, _, _ = ordered(driver, tmp_path, ctx, TH.K, H.graph_text(header, recs), two_libraries(pairs), high)
    assert compared >= 1 and joined >= 1 and sum(r["blocked"] for r in rs) >= 1 and not any(r["cycles"] for r in rs)
    ctx.close()


@pytest.mark.parametrize("seed,high", [(6, 3), (8, 4), (4, 3)])
def test_ordered_generated_graphs_with_hubs(seed, high, driver, tmp_path):
    """every edge with flow 2: no join deletes an operand, so the rounds lie inside the reference; blocked rows and rows skipped after a join erased their key occur"""
    N, header, recs = CG.case_e(seed)
    recs = with_flow(recs, 2)
    parsed = H.parse_graph(H.graph_text(header, recs), fold=False)
    pairs = LH.merged(CG.mates_e(parsed, seed, for_reference=True), LH.long_range_mates(parsed))
    ctx = GH.host_store(N, 100 + seed)
    compared, joined, rs, _, _ = ordered(driver, tmp_path, ctx, CG.K, H.graph_text(header, recs), pairs, high)
    assert compared >= 1 and joined >= 1 and sum(r["blocked"] for r in rs) >= 1 and sum(r["skipped"] for r in rs) >= 1
    ctx.close()


GOLDEN_HIGH = {"g4_highcopy_k21": 2, "g9_repeats160k_k40": 2}


@pytest.mark.parametrize("name", sorted(GOLDEN_HIGH))
def test_ordered_goldens_with_long_range_mates(name, driver, tmp_path):
    m = fx.golden(name); ctx = host_store(fx.make_reads(m["synth"]), m["k"])
    g = MS.with_flows(H.parse_graph(gzip.open(os.path.join(fx.GOLDEN, name + ".graph4.gz")).read(), fold=False), lambda q, a: (2.0, 2.0))
    recs = with_flow([r for _, a, b_ in g["pairs"] for r in (a, b_)], 2)
    text = H.graph_text(g["header"], recs)
    parsed = H.parse_graph(text, fold=False)
    pairs = LH.merged(MS.golden_mates(parsed, ctx.reads_stats().unique_reads), LH.long_range_mates(parsed))
    compared, joined, rs, _, _ = ordered(driver, tmp_path, ctx, m["k"], text, pairs, GOLDEN_HIGH[name], max_rounds=3)
    assert compared >= 1 and sum(r["rows"] for r in rs) >= 1
    ctx.close()


# ------------------------------------------------------------------------------------------ the recorded cases (tests/golden/short/, tools/make_golden_short.py)
# (every flow of the hand graph 50, or the cycle's flows at high 1 where its star joins nothing: no join deletes an operand whose node still has rows listed, so
# every round up to the empty one lies inside the reference; the components' own edges have flow 1 and are deleted by their joins)
GOLDEN_CASES = {"short_high1": (1, TH.ALL, dict(flows=SH.KEPT)), "short_high2": (2, TH.ALL, dict(flows=SH.KEPT)), "short_cycle": (1, ["minus", "zero", "plus"], SH.CYCLE)}


def golden_case(name):
    """(N, header, records, pairs, high) of a case tools/make_golden_short.py records"""
    high, names, kw = GOLDEN_CASES[name]
    N, header, recs, pairs, _ = TH.short_graph(names, **kw)
    return N, header, recs, two_libraries(pairs), high


def test_the_recorded_cases_meet_their_conditions(driver, tmp_path):
    """for every recorded round the model reports outside_reference == 0 and ties == 0; every case has a join; across the cases there is a blocked row, a row removed
    by gapSum > 0 alone, and a join GAPPED with a gap of 0 -- and the reference, handed the rows, does what was recorded"""
    import json
    blocked = plus_only = gapped_zero = 0
    for name in sorted(GOLDEN_CASES):
        N, header, recs, pairs, high = golden_case(name)
        ctx = hand_store(N); work = tmp_path / name; work.mkdir()
        compared, joined, rs, op, g = ordered(driver, work, ctx, TH.K, H.graph_text(header, recs), pairs, high, fasta=True)
        assert joined >= 1 and not rs[-1]["merges"] and all(not r["outside_reference"] and not r["ties"] for r in rs)
        blocked += sum(r["blocked"] for r in rs); gapped_zero += sum(1 for r in rs for m in r["merges"] if m["gap"] == 0 and m["how"] == (SM.GAPPED, SM.GAPPED))
        g0 = SM.Graph(H.parse_graph(H.graph_text(header, recs), fold=False)); b = X.Bounds(g0, pairs); sums = SO.sums_of(g0, pairs, b, TH.K)
        keep = SO.short_filter(g0, sums)
        plus_only += sum(1 for (qa, sa, qb, sb, s, gs) in sums if 2 * qa + sa < 2 * qb + sb and gs > 0 and keep(qa, qb, s, 0))
        path = os.path.join(fx.GOLDEN, "short", name + ".json.gz")
        if os.path.exists(path):
            rec = json.load(gzip.open(path, "rt"))
            assert rec["joins"] == [len(r["merges"]) for r in rs] and rec["graphs"] == [unflagged(open("%s.%d" % (op, rd)).read()) for rd in range(1, compared + 1)]
            assert rec["fasta"] == open(op + "_contig.fasta").read()
        ctx.close()
    assert blocked >= 1 and plus_only >= 1 and gapped_zero >= 1
