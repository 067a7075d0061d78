"""CPU: the restatement of the fourth loop of extendContigs (tests/short_model.py) pinned with literal numbers on the hand-built link graph of
tests/test_links_host.py, with flows set and with components of two or three edges added that only mates link: the row filter (flows, lengths, the raw gap sum),
the selection that admits no rival and knows no cycle, the threshold, the record sizes against the C compiler and the new calls on a device-less context.  Also the
builders the reference and GPU tests share."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import fixtures as fx
import sage2_amd as s2
import scaffold_model as SM
import short_model as SO
import extend_model as X
import test_mate_estimate_host as H
import test_links_host as LH
import test_scaffold_host as SH

K = LH.HAND_K
N_READS = 450                          # read ids of the graphs below: the hand graph's 100, 12 per added component from 101 on, far ends from 251, 301 and 351 on


# ------------------------------------------------------------------------------------------ builders shared with the reference and GPU tests
def component(i, lenP, lenQ, flowP, flowQ, p, q, twin=False, lenZ=0, flowZ=1):
    """three or two edges in components of their own, ids B = 101 + 12 i on:
      P  PF -> B     type 3, reads B+2 and B+3 (orientation 0) p[0] and p[1] bases from its start.  The record leaves the larger id: E of the pair is the twin, so
                     LINK(P's record, .) has edge_1 = P's twin = E, the only form a short-overlap round can join (the pointer identity of :1863, :1872)
      Q  B+4 -> QE   type 3, reads B+6 and B+7 (orientation 0) q[0] and q[1] bases from its start; twin: orientation 1, q[0] and q[1] bases before its END, so that
                     they stand on Q's twin as they would on the record: the link is LINK(P's record, Q's twin) and edge_2 is not E
      Z  B+8 -> ZE   (lenZ > 0) type 3, read B+11 (orientation 0) 20 bases from its start; Q then holds read B+10 (orientation 1) 8 bases before its end, which stands
                     on Q's twin 8 bases from the start: the mate (B+10, B+11) makes LINK(Q's twin, Z's record), whose edge_1 is Q's record = E, with gapSum 26 - 28 = -2
    PF = 251 + 5 i, QE = 301 + 7 i and ZE = 351 + 11 i lie apart so that no two pairs of a graph share from ^ to, the key of SEARCH (short_graph asserts it).
    Library-1 mates of type (1, 1): a hit needs a distance sum below 221 + 40 - 120 = 141 and adds 146 - 120 - sum = 26 - sum to gapSum.
    -> (records, mates): mates (B+2, B+6), (B+3, B+7) and, with Z, (B+10, B+11)"""
    B = 101 + 12 * i; PF = 251 + 5 * i; QE = 301 + 7 * i; ZE = 351 + 11 * i
    P = H.rec(PF, B, 3, lenP, [(B + 2, 0, 0, p[0], p[1] - p[0]), (B + 3, 0, 0, p[1] - p[0], lenP - p[1])])
    if twin:
        ql = [(B + 7, 1, 0, lenQ - q[1], q[1] - q[0]), (B + 6, 1, 0, q[1] - q[0], q[0])]
    else:
        ql = [(B + 6, 0, 0, q[0], q[1] - q[0]), (B + 7, 0, 0, q[1] - q[0], lenQ - q[1])]
    mates = [(B + 2, 1, B + 6, 1), (B + 3, 1, B + 7, 1)]
    edges = [(P, flowP)]
    if lenZ:
        last = ql[-1]; ql[-1] = last[:4] + (lenQ - q[1] - 8,); ql.append((B + 10, 1, 0, lenQ - q[1] - 8, 8))
        edges += [(H.rec(B + 4, QE, 3, lenQ, ql), flowQ), (H.rec(B + 8, ZE, 3, lenZ, [(B + 11, 0, 0, 20, lenZ - 20)]), flowZ)]
        mates.append((B + 10, 1, B + 11, 1))
    else:
        edges.append((H.rec(B + 4, QE, 3, lenQ, ql), flowQ))
    recs = []
    for r, f in edges:
        t = H.twin_of(r); r["flow"] = t["flow"] = float(f); recs += [r, t]
    return recs, mates


# the components by name: (lenP, lenQ, flowP, flowQ, p, q, ...) and the mates left out
COMPONENTS = {
    "plus":   ((150, 160, 1, 1, (8, 14), (12, 17)), ()),             # 26 - 20 = +6 and 26 - 31 = -5: support 2, gapSum +1, gap 0 -- out by :1587 alone
    "minus":  ((151, 170, 1, 1, (8, 14), (12, 19)), ()),             # +6 and 26 - 33 = -7: support 2, gapSum -1, gap 0 -- in
    "zero":   ((152, 180, 1, 2, (10, 30), (16, 40)), (1,)),          # 26 - 26: support 1, gapSum 0 -- in; Q (flow 2) is kept
    "len60":  ((153, 60, 1, 1, (8, 14), (12, 19)), ()),              # as "minus" with Q of 60 bases: the threshold itself -- out
    "twin":   ((154, 190, 1, 1, (8, 14), (12, 19), True), ()),       # as "minus" on Q's twin: edge_2 is not E, the row's own partner counts against it
    "chain":  ((155, 175, 1, 50, (8, 14), (12, 19), False, 185, 1), ()),      # P . Q (support 2) and Q . Z (support 1) share the kept Q
    "noflow": ((156, 165, 1, 0, (8, 14), (12, 19)), ()),             # as "minus" with flow 0 on Q -- out
}


def short_graph(names, flows=None, extra=None):
    """SH.hand(flows, extra) -- the hand-built link graph -- and the named components behind it, in that order: pair ordinals 13 on, two or three per component.
    -> (N, header, records, pairs, seqs)"""
    _, header, recs, pairs, _ = SH.hand(flows=flows, extra=extra)
    pairs = dict(pairs); more = []
    for i, name in enumerate(names):
        args, left_out = COMPONENTS[name]
        r, m = component(i, *args); recs = recs + r; more += [x for j, x in enumerate(m) if j not in left_out]
    pairs[1] = pairs[1] + more
    keys = [r["frm"] ^ r["to"] for r in recs[26::2]]
    assert len(set(keys)) == len(keys) and not set(keys) & {r["frm"] ^ r["to"] for r in recs[:26]}      # no XOR collision through the added edges
    return N_READS, header, recs, pairs, {i: SH.rnd(60, 1000 + i) for i in range(1, N_READS + 1)}


def run_round(high, names=(), **kw):
    N, header, recs, pairs, seqs = short_graph(names, **kw)
    g = SH.graph_of(header, recs); b = X.Bounds(g, pairs)
    return g, SO.round_(g, pairs, b, K, high, seqs), (pairs, b, seqs)


def sums_by_pairs(names=(), **kw):
    N, header, recs, pairs, seqs = short_graph(names, **kw)
    g = SH.graph_of(header, recs); b = X.Bounds(g, pairs)
    assert (b.min_upper, b.max_upper) == (221, LH.HAND_BOUND) and [(b.ests[L]["mean"], b.ests[L]["upper"]) for L in (1, 2)] == [(146, 221), (113, 233)]      # the added mates sit on two edges each: the estimate is the hand graph's
    sums = SO.sums_of(g, pairs, b, K)
    return g, sums, {r[:4]: r[4:] for r in sums}


C2 = {2: 2}                            # C keeps its place when the round joins C . D: the round stays inside the reference (rule (d))
ALL = ["plus", "minus", "zero", "len60", "twin", "chain", "noflow"]


# ------------------------------------------------------------------------------------------ the gap sums
def test_gap_sums_of_the_hand_graph_and_their_quotients():
    g, sums, d = sums_by_pairs()
    quot = LH.all_links(g.parsed(), short_graph(())[3], K)
    assert [r[:5] + (SO.quotient(r[5], r[4]),) for r in sums] == quot and len(sums) == LH.HAND_ROWS      # the same sweep: LH.links holds the quotient only
    assert d[(LH.qG, 0, LH.qH, 0)] == (2, -7) and SO.quotient(-7, 2) == -3            # not the floor -4
    assert d[(LH.qC, 0, LH.qD, 0)] == (5, -434) and d[(LH.qA, 0, LH.qB, 0)] == (3, -150) and d[(LH.qLq, 0, LH.qG, 0)] == (1, 11)
    assert [SO.quotient(a, b) for a, b in ((1, 2), (-1, 2), (0, 1), (-3, 2), (3, 2), (-434, 5))] == [0, 0, 0, -1, 1, -86]


def test_the_quotient_cannot_stand_in_for_the_sum():
    """support 2 both times and gap 0 both times: +6 - 5 = +1 is out, +6 - 7 = -1 is in and joins GAPPED with no N"""
    g, sums, d = sums_by_pairs(["plus", "minus"])
    assert d[(13, 0, 14, 0)] == (2, 1) and d[(15, 0, 16, 0)] == (2, -1)
    keep = SO.short_filter(g, sums)
    assert not keep(13, 14, 2, 1) and keep(15, 16, 2, -1) and SO.quotient(1, 2) == SO.quotient(-1, 2) == 0
    g, r, _ = run_round(2, ["plus", "minus"], flows=C2)
    assert [row for row in r["row_list"] if row[0] >= 26] == [(31, 32, 2, 0, -1)]      # edge_1 = P's twin, edge_2 = Q's record
    # the ordinals are the file's: the hand graph's two loops are written twice, so pool pairs 15 and 16 are record pairs 17 and 18
    assert SM.joins_rows(r)[1] == (113, 308, 2, 0, 17, 18, 18, -1, -1, 1, 1, 1, SM.GAPPED, SM.GAPPED) and r["gapped"] == 2
    new = g.h[-2]                                                                      # 151 + 170 + 60: D1 = gap + L1 = 60, the read's own length: no N
    assert (new["frm"], new["to"], new["len"]) == (113, 308, 151 + 170 + 60) and new["list"][2:4] == [(256, 0, 0, 8, 60), (117, 1, 0, 60, 12)]
    assert not g.alive[15] and not g.alive[16] and g.alive[13] and g.alive[14]


def test_a_gap_sum_of_zero_is_in():
    g, sums, d = sums_by_pairs(["zero"])
    assert d[(13, 0, 14, 0)] == (1, 0)
    g, r, _ = run_round(1, ["zero"])
    assert SM.joins_rows(r) == [(101, 301, 1, 0, 15, 16, 15, -1, -1, 1, 1, 0, SM.GAPPED, SM.GAPPED)]
    assert g.h[2 * 14]["flow"] == 1.0 and g.alive[14] and not g.alive[13]              # Q had flow 2


def test_lengths_and_flows_of_the_filter():
    g, sums, d = sums_by_pairs(["len60", "noflow"])
    keep = SO.short_filter(g, sums)
    assert d[(13, 0, 14, 0)] == (2, -1) and not keep(13, 14, 2, -1)                    # 60 is not above the threshold 60
    assert d[(15, 0, 16, 0)] == (2, -1) and not keep(15, 16, 2, -1)                    # flow 0 on Q
    assert d[(LH.qLq, 1, LH.qJ, 0)] == (1, -60) and not keep(LH.qLq, LH.qJ, 1, -60)    # the hand graph's loop of 60 bases
    # A (300, flow 2) - G (201, flow 0): both above 200 pass mergeFinal's filter whatever the flows; here there is no such alternative
    assert d[(LH.qA, 0, LH.qG, 0)] == (1, -34) and SO.final_filter(g, False)(LH.qA, LH.qG, 1, -34) and not keep(LH.qA, LH.qG, 1, -34)
    assert (LH.qA, 0, LH.qG, 0) in {r[:4] for r in LH.filtered(g.parsed(), LH.all_links(g.parsed(), short_graph(["len60", "noflow"])[3], K), LH.FINAL)}
    for args, want in (((61, 1, 61, 1, 0), True), ((61, 1, 61, 1, 1), False), ((60, 1, 61, 1, -5), False), ((61, 1, 60, 1, -5), False), ((61, 0, 61, 1, -5), False),
                       ((61, 1, 61, 0, -5), False), ((201, 0, 201, 0, -5), False), ((61, 0.5, 61, 0.5, -(1 << 31)), True), ((61, None, 61, None, -5), False)):
        assert SO.passes(*args, 60) is want, args
    g, r, _ = run_round(1, ["len60", "noflow"])
    assert r["rows"] == 9 and not [row for row in r["row_list"] if row[0] >= 26]      # the hand graph's nine rows alone


def test_no_flow_array_no_rows():
    N, header, recs, pairs, seqs = short_graph(["minus"])
    g = SH.graph_of(header, recs); b = X.Bounds(g, pairs)
    r = SO.round_(g, pairs, b, K, 1, seqs, flows=False)
    assert (r["rows"], r["merges"], r["batches"]) == (0, [], 0)


# ------------------------------------------------------------------------------------------ the selection
def test_one_rival_at_the_threshold_blocks_what_step_7_joins():
    """C's twin . D has support 5; on C's side B stands with support 1 (LINK(B, C)).  At high 1 mergeAccordingToSupport admits one rival and joins, mergeShortOverlap
    admits none; at high 2 the rival is one below and the row joins here too"""
    N, header, recs, pairs, seqs = short_graph((), flows=C2)
    g = SH.graph_of(header, recs); b = X.Bounds(g, pairs)
    r7 = SM.round_(g, pairs, b, K, 1, 1, False, seqs)
    assert r7["verdicts"][0] == ("join", [], [1]) and SM.joins_rows(r7)[0][:4] == (2, 31, 5, -86)
    g, r, _ = run_round(1, flows=C2)
    assert r["verdicts"][0] == ("blocked", [], [1]) and r["row_list"][0] == (5, 6, 5, -86, -434)
    assert (r["rows"], r["blocked"], r["cycles"], r["merges"], r["batches"]) == (9, 9, 0, [], 0)
    g, r, _ = run_round(2, flows=C2)
    assert r["verdicts"][0] == ("join", [], []) and SM.joins_rows(r) == [(2, 31, 5, -86, 1, 3, 2, -2, -2, 0, 0, 0, SM.EQUAL, SM.EQUAL)]
    assert (r["rows"], r["below_threshold"], r["skipped"], r["blocked"], r["outside_reference"], r["ties"]) == (9, 1, 7, 0, False, False)


def test_the_hand_built_cycle_is_blocked_and_no_cycle_is_counted():
    """tests/test_scaffold_host.py's cycle: G, Hh and J linked two by two.  G's twin . Hh (support 2) has J on both sides, a CYCLE for mergeFinal; here it is one of
    the rivals that block the row"""
    N, header, recs, pairs, seqs = short_graph((), **SH.CYCLE)
    g = SH.graph_of(header, recs); b = X.Bounds(g, pairs)
    r7 = SM.round_(g, pairs, b, K, 1, 2, False, seqs)
    assert r7["cycles"] == 4 and r7["verdicts"][2] == ("cycle", [7, 10], [10])
    g, r, _ = run_round(1, **SH.CYCLE)
    assert r["row_list"][2] == (15, 16, 2, -3, -7) and r["verdicts"][2] == ("blocked", [1, 7, 10], [0, 1, 10])      # more rows are in SEARCH here: no "> 200" alternative, but G has a flow now
    assert (r["rows"], r["cycles"], r["blocked"], r["merges"]) == (12, 0, 12, [])


def test_the_rows_own_partner_counts_unless_it_is_the_tables_half():
    """the feasible list holds E of every pair (the pointer the read-to-edge table holds): q == pair(edge_2) is left out only when edge_2 is that half.  "minus" links
    P's record to Q's record (E): it joins.  "twin" links P's record to Q's twin: Q counts on P's side and the row is blocked by its own partner"""
    g, r, _ = run_round(2, ["minus", "twin"], flows=C2)
    rows = {row[:2]: v for row, v in zip(r["row_list"], r["verdicts"])}
    assert rows[(27, 28)] == ("join", [], []) and rows[(31, 33)] == ("blocked", [], [16])
    assert g.is_E(28) and not g.is_E(33) and g.is_E(27) and g.is_E(31)
    # every row of the hand graph but C . D has edge_1 = the twin of E (the records leave the smaller id): its own pair counts on edge_2's side
    g, r, _ = run_round(1, flows=SH.KEPT)
    assert all(v[0] == "blocked" for v in r["verdicts"]) and r["verdicts"][2] == ("blocked", [1, 7, 10], [0, 1]) and r["row_list"][2][:2] == (15, 16)


def test_a_kept_operand_cannot_be_named_again_in_a_short_round():
    """"chain": P . Q (support 2) and Q . Z (support 1) share Q, whose flow of 50 would keep it.  With no rival admitted, two rows in SEARCH that share a pair are
    each other's rival through the XOR key in either order (:1828-1832, :1850-1854): at high 1 both are blocked, at high 2 Q . Z is below and P . Q joins.  So a
    row that names an operand of an earlier join of the round would have been that join's rival: a short round never goes to the device in more than one batch
    (rule (e) serves step 7 alone, tests/test_scaffold_host.py pins it there)"""
    g, r, _ = run_round(1, ["chain"], flows=C2)
    rows = {row[:2]: (row[2:], v) for row, v in zip(r["row_list"], r["verdicts"])}
    assert rows[(27, 28)] == ((2, 0, -1), ("blocked", [15], [])) and rows[(28, 30)] == ((1, -2, -2), ("blocked", [], [13]))
    assert r["named_again"] == 0 and r["batches"] == 0
    g, r, _ = run_round(2, ["chain"], flows=C2)
    assert [m[:4] for m in SM.joins_rows(r)] == [(2, 31, 5, -86), (101, 301, 2, 0)] and r["batches"] == 1 and r["named_again"] == 0
    assert dict(zip([row[:2] for row in r["row_list"]], [v[0] for v in r["verdicts"]]))[(28, 30)] == "below"
    assert g.h[28]["flow"] == 49.0 and g.alive[14]                                     # Q is kept


def test_rounds_until_nothing_joins_and_the_counts_add_up():
    N, header, recs, pairs, seqs = short_graph(ALL, flows=C2)
    g = SH.graph_of(header, recs); b = X.Bounds(g, pairs)
    rs = SO.loop(g, pairs, b, K, 2000, 100, seqs)                                      # coverage 3: high 1
    assert SO.threshold(100, 60, 2000) == 1 and [len(r["merges"]) for r in rs] == [2, 0] and [m[:4] for m in SM.joins_rows(rs[0])] == [(113, 308, 2, 0), (125, 315, 1, 0)]
    for r in rs:
        assert r["rows"] == r["below_threshold"] + r["skipped"] + r["blocked"] + len(r["merges"]) and r["cycles"] == 0
    g2 = SH.graph_of(header, recs)
    rs2 = SO.loop(g2, pairs, b, K, 1000, 100, seqs)                                    # coverage 6: high 1 as well (0.3 * 1.67 = 0.5)
    assert g2.text() == g.text()


def test_the_selection_with_step_7s_parameters_is_step_7s_round():
    """short_model.select is written once for both steps: with mergeFinal's filter, its limit and the cycle test it is scaffold_model.round_, row for row"""
    keys = ("rows", "below_threshold", "skipped", "blocked", "cycles", "batches", "overlaps", "concatenated", "gapped", "ties", "outside_reference", "named_again")
    for kw in (dict(), dict(flows=SH.KEPT), SH.CYCLE):
        for high, flag, small in ((1, 1, False), (1, 2, False), (2, 1, False), (1, 2, True)):
            N, header, recs, pairs, seqs = short_graph(["minus", "chain"], **kw)
            g1 = SH.graph_of(header, recs); g2 = SH.graph_of(header, recs); b = X.Bounds(g1, pairs)
            r1 = SM.round_(g1, pairs, b, K, high, flag, small, seqs); r2 = SO.scaffold_round(g2, pairs, b, K, high, flag, small, seqs)
            assert SM.joins_rows(r1) == SM.joins_rows(r2) and all(r1[k] == r2[k] for k in keys) and g1.text() == g2.text()
            assert [v[0] for v in r1["verdicts"]] == [v[0] for v in r2["verdicts"]]


# ------------------------------------------------------------------------------------------ the threshold
def test_threshold_of_the_fourth_loop():
    # 1000 reads of 100 bases on 2500: coverage 40, 0.05 * 40 * 1 = 2; the quotient is an integer: 999 * 100 / 2500 = 39 -> 1.95 -> 2
    assert s2.extend_short_threshold(1000, 100, 2500) == 2 == SO.threshold(1000, 100, 2500) and s2.extend_short_threshold(999, 100, 2500) == 2
    assert s2.extend_short_threshold(1000, 100, 2500) == s2.scaffold_threshold(1000, 100, 2500, 1, 6)      # the factor of mergeFinal's later iterations
    # a coverage quotient of 0: high 0 (the round is then outside what equality is claimed for)
    assert s2.extend_short_threshold(10, 100, 2500) == 0 == SO.threshold(10, 100, 2500)
    # coverage 6 at read length 60: 0.3 * 1.67 = 0.5 -> 1; coverage 41 at 151: 2.05 * 0.662 = 1.36 -> 2
    assert s2.extend_short_threshold(200, 60, 2000) == 1 == SO.threshold(200, 60, 2000)
    assert s2.extend_short_threshold(41, 151, 151) == 2 == SO.threshold(41, 151, 151)
    # independent of the genome size class: 0.05 below and above 10^9, where the first loop's factor changes
    assert s2.extend_short_threshold(10 ** 9, 100, 2 * 10 ** 9) == SO.threshold(10 ** 9, 100, 2 * 10 ** 9) == 3
    assert s2.Context.extend_short_threshold(1000, 100, 2500) == 2
    for args in ((1000, 0, 2500), (1000, 100, 0)):
        with pytest.raises(s2.Sage2ovError) as e:
            s2.extend_short_threshold(*args)
        assert e.value.code == -1
    assert s2.lib().sage2ov_extend_short_threshold(C.c_uint64(1), C.c_uint64(1), C.c_uint64(1), None) == -1


# ------------------------------------------------------------------------------------------ the C ABI without a GPU
def test_record_sizes_against_the_c_compiler(tmp_path):
    """the short-overlap calls use step 7's records: the header the C compiler reads declares them with those types"""
    src, exe = str(tmp_path / "sz.c"), str(tmp_path / "sz")
    open(src, "w").write('#include <stdio.h>\n#include <stdint.h>\n#include "sage2ov.h"\n'
                         'int (*a)(const sage2ov_ctx*, sage2ov_join*, uint64_t) = sage2ov_extend_short_merges_export;\n'
                         'int (*b)(const sage2ov_ctx*, sage2ov_scaffold_stats*) = sage2ov_extend_short_stats_get;\n'
                         'int (*c)(sage2ov_ctx*, uint32_t, uint32_t, int32_t*, uint64_t) = sage2ov_links_gap_sums;\n'
                         'int (*d)(sage2ov_ctx*, uint64_t, uint64_t*, uint64_t*) = sage2ov_extend_contigs;\n'
                         'int main(void) { printf("%zu %zu %zu %zu", sizeof(sage2ov_join), sizeof(sage2ov_scaffold_counts), sizeof(sage2ov_scaffold_stats), sizeof(int32_t)); return !(a && b && c && d); }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(fx.ROOT, "include"), "-c", src, "-o", exe + ".o"], check=True)
    subprocess.run(["gcc", exe + ".o", "-o", exe, "-L", os.path.join(fx.ROOT, "sage2_amd"), "-lsage2ov", "-Wl,-rpath," + os.path.join(fx.ROOT, "sage2_amd")], check=True)
    got = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got == [s2.JOIN_DTYPE.itemsize, C.sizeof(s2.ScaffoldCounts), C.sizeof(s2.ScaffoldStats), np.dtype(np.int32).itemsize] == [48, 144, 304, 4]


def test_device_less_context_refuses():
    rng = np.random.default_rng(5)
    reads = sorted({"".join(rng.choice(list("ACGT"), size=60)) for _ in range(20)})
    bases = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(); off = np.arange(0, (len(reads) + 1) * 60, 60, dtype=np.uint64)
    ctx = s2.Context(40, device=-2); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
    for call in (ctx.links_gap_sums, lambda: ctx.links_gap_sums(LH.FINAL, 2), lambda: ctx.extend_short_round(2), ctx.extend_by_short_overlaps, ctx.extend_contigs):
        with pytest.raises(s2.Sage2ovError) as e:
            call()
        assert e.value.code == -3
    st = ctx.extend_short_stats(); assert (st.rounds, st.total.rows, st.total.merged, st.total.cycles) == (0, 0, 0, 0) and len(ctx.extend_short_merges()) == 0
    n = C.c_uint64(7); out = (C.c_int32 * 4)()
    assert s2.lib().sage2ov_extend_short_merges_count(None, C.byref(n)) == -1 and s2.lib().sage2ov_extend_short_round(None, C.c_int(1), None) == -1
    assert s2.lib().sage2ov_links_gap_sums(None, C.c_uint32(0), C.c_uint32(1), out, C.c_uint64(4)) == -1
    assert s2.lib().sage2ov_links_gap_sums(ctx._h, C.c_uint32(3), C.c_uint32(1), out, C.c_uint64(4)) == -1      # no such mode, as for sage2ov_links_export
    assert s2.lib().sage2ov_extend_contigs(None, C.c_uint64(0), None, None) == -1 and s2.lib().sage2ov_extend_by_short_overlaps(None, C.c_uint64(0), None, None) == -1
    ctx.close()
