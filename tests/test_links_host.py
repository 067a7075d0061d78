"""CPU: the restatement of the sweep that opens ScaffoldMaker::mergeFinal / mergeFinalSmall (matePair/scaffolding.cpp:786-935, :981-1130) as include/sage2ov.h
states it (LINK(a, b), the table, the filters), pinned on a hand-built graph whose numbers were checked against the reference's own sweep -- and the helpers the
reference and GPU tests of the links share.  Also: the size of sage2ov_link against the C compiler and the new calls on a device-less context."""
import ctypes as C
import math
import os
import subprocess
import numpy as np
import pytest
import fixtures as fx
import sage2_amd as s2
import test_mate_estimate_host as H
import test_mate_support_host as MS

M32 = (1 << 32) - 1
NO_SIGN = 10000000
ALL, FINAL, SMALL = 0, 1, 2


# ------------------------------------------------------------------------------------------ the restatement (include/sage2ov.h)
def halves_of(g):
    """{(ordinal, second): (record, is E of its pair)}: second = 0 for the record the file holds first of its pair, 1 for its twin; E is the half leaving the smaller
    node, of a loop the second record"""
    out = {}
    for q, a, b in g["pairs"]:
        E = a if a["frm"] < a["to"] else b
        out[(q, 0)] = (a, a is E); out[(q, 1)] = (b, b is E)
    return out


def links(g, table, pairs, ests, max_upper, arl, k):
    """g: H.parse_graph(..), table: H.read_edge_table(g), pairs: {L: [(a, sa, b, sb)]}, ests: {L: H.estimate(..)} -> [(pair_a, second_a, pair_b, second_b, support,
    gap)], every ordered (a, b) with support >= 1, ascending"""
    pr = H.by_read(table)
    nodes = {a["frm"] for _, a, b in g["pairs"]} | {a["to"] for _, a, b in g["pairs"]}
    mates = {}
    for L, pl in pairs.items():
        for (a, b, ta, tb) in sorted({(a, b, sa, sb) for a, sa, b, sb in pl} | {(b, a, sb, sa) for a, sa, b, sb in pl}):      # each entry once, whatever its count
            mates.setdefault(a, []).append((b, ta, tb, L))
    hv = halves_of(g)
    unique_pair = lambda r: pr[r][0] if r not in nodes and len(pr.get(r, [])) == 1 else None
    loc = lambda r, q, isE: table[(r, q)]["forward" if isE else "reverse"]
    acc = {}
    for (qa, sa), (a, ea) in hv.items():
        run = 0
        for (m1, o, f, dp, dn) in a["list"]:
            run += dp
            if run > max_upper:                                                        # :833-835
                break
            if unique_pair(m1) != qa:                                                  # :837
                continue
            for (m2, t1, t2, L) in mates.get(m1, []):
                qb = unique_pair(m2)
                if not ests[L]["valid"] or qb is None or qb == qa:                     # :843; pair(a) != pair(b)
                    continue
                for sb in (0, 1):
                    b, eb = hv[(qb, sb)]
                    hit = None
                    for x in loc(m1, qa, ea):                                          # :850-874: the first (x, y) in list order
                        for y in loc(m2, qb, eb):
                            d = abs(x) + abs(y) if (1 if t1 else -1) * x < 0 and (1 if t2 else -1) * y < 0 else NO_SIGN
                            if d + 2 * arl < ests[L]["upper"] + k:
                                hit = d
                                break
                        if hit is not None:
                            break
                    if hit is not None:
                        s, gs = acc.get((qa, sa, qb, sb), (0, 0))
                        acc[(qa, sa, qb, sb)] = (s + 1, (gs + ests[L]["mean"] - (hit + 2 * arl)) & M32)      # :877-878: int32_t gapSum takes a uint64_t expression
    out = []
    for key in sorted(acc):
        s, gs = acc[key]
        gs = gs - (1 << 32) if gs >= (1 << 31) else gs
        out.append(key + (s, -(-gs // s) if gs < 0 else gs // s))                      # :892: an int32_t division truncates towards zero
    return out


def threshold(arl):
    """contigLengthThreshold = (int)ceilf(100*(averageReadLength/100.0)) (scaffolding.cpp:20)"""
    return int(math.ceil(np.float32(100 * (arl / 100.0))))


def passes(mode, len1, flow1, len2, flow2, arl):
    if mode == ALL:
        return True
    if mode == SMALL:
        return len1 < 500 and len2 < 500                                               # :996
    t = threshold(arl)
    return (len1 > 200 and len2 > 200) or ((flow1 > 0 and len1 > t) and (flow2 > 0 and len2 > t))      # :801


def e_half(g):
    """{ordinal: E of the pair}: the half whose lengthOfEdge and flow the filters read"""
    return {q: (a if a["frm"] < a["to"] else b) for q, a, b in g["pairs"]}


def filtered(g, rows, mode, min_support=1):
    E = e_half(g); arl = g["header"][2]
    return [r for r in rows if r[4] >= min_support and passes(mode, E[r[0]]["len"], E[r[0]]["flow"], E[r[2]]["len"], E[r[2]]["flow"], arl)]


def all_links(g, pairs, k):
    t, ests, (_, hi) = MS.support_inputs(g, pairs)
    return links(g, t, pairs, ests, hi, g["header"][2], k)


def long_range_mates(g, seed=9, step=3, reach=5):
    """mates between pairs that share no node by construction of the rule alone: for q = 0, step, 2 step, ... below the pair count - reach, the halves (record of pair
    q, twin of pair q + reach) and (twin of q, record of q + reach); of each such two halves the entries j < 4 of both lists, strands 1 - orientation, the library drawn
    from default_rng(seed)"""
    rng = np.random.default_rng(seed); P = g["pairs"]; out = {1: [], 2: []}
    for i in range(0, len(P) - reach, step):
        for (x, y) in ((P[i][1], P[i + reach][2]), (P[i][2], P[i + reach][1])):
            for j in range(min(4, len(x["list"]), len(y["list"]))):
                ea, eb = x["list"][j], y["list"][j]
                out[int(rng.integers(1, 3))].append((ea[0], 1 - ea[1], eb[0], 1 - eb[1]))
    return out


def merged(*pair_dicts):
    out = {}
    for d in pair_dicts:
        for L, pl in d.items():
            out.setdefault(L, []).extend(pl)
    return out


# ------------------------------------------------------------------------------------------ the reference's rows (tests/test_links_reference.py, tests/golden/*.links.txt.gz)
def half_id(h):
    return (h["frm"], h["to"], h["type"], h["len"])


def same_as_reference(g, rows, ref):
    """rows: the restatement's over g; ref: {FINAL: .., SMALL: ..} of {(id of a, id of b): (support, gap)} as mergeFinal / mergeFinalSmall handed them to the sort.
    Every reference row equals the restatement's row under the same filter; every filtered restatement row has itself or its reverse among the reference's rows
    (of (a, b) and (b, a) the reference keeps whichever malloc placed lower).  Rows that touch a loop are left out: the reference's loader makes two edges of one."""
    hv = halves_of(g); loop = {q for q, a, b in g["pairs"] if a["frm"] == a["to"]}
    ids = [half_id(h) for h, _ in hv.values()]
    for mode in (FINAL, SMALL):
        want = {(half_id(hv[(r[0], r[1])][0]), half_id(hv[(r[2], r[3])][0])): (r[4], r[5]) for r in filtered(g, rows, mode) if r[0] not in loop and r[2] not in loop}
        assert all(ids.count(i) == 1 for i in {i for key in want for i in key})       # (from, to, type, length) names one half among the rows compared
        got = {key: v for key, v in ref[mode].items() if not any(i[0] == i[1] for i in key)}
        for key, v in got.items():
            assert want.get(key) == v, (mode, key, v, want.get(key))
        for (a, b) in want:
            assert (a, b) in got or (b, a) in got, (mode, a, b)


def golden_links(name):
    """the reference's rows as tools/make_golden_links.py recorded them"""
    import gzip
    ref = {FINAL: {}, SMALL: {}}
    for line in gzip.open(os.path.join(fx.GOLDEN, name + ".links.txt.gz"), "rt"):
        v = [int(t) for t in line.split()]
        ref[v[0]][(tuple(v[1:5]), tuple(v[5:9]))] = (v[9], v[10])
    return ref


def golden_pairs(name, g, n_reads):
    """the mates of the golden cases: MS.golden_mates, and on g9 the long-range mates as well"""
    pairs = MS.golden_mates(g, n_reads)
    return merged(pairs, long_range_mates(g)) if name.startswith("g9") else pairs


# ------------------------------------------------------------------------------------------ the hand-built graph
HAND_K = MS.HAND_K
HAND_BOUND = 699                      # maximumUpperBoundOfInsert of the hand graph without a variant (asserted below)


def hand_link_graph(variant=None, invalid_library=True):
    """(N, header, records, pairs): MS.hand_support_graph's star at node 10 (A, B, C, D, F, S and the loop Lp, two libraries estimated from their same-edge mates) and
    six edges in components of their own that only mates link to it and to one another:
      G  20 -> 21  length 201, flow 0    read 77 stands twice (orientation 0 both: locations -25, -75), read 70 at -10
      Hh 22 -> 23  length 200, flow 1    read 78 stands twice: +47 fails the sign test of a type-1 mate, -72 passes; 74 at -12, 79 at -27
      Lq 24 -> 24  length 60 (the average read length), flow 2: a loop with mated unique reads 75, 76
      J  25 -> 26  length 61, flow 1;  I  27 -> 28  length 500, flow 1;  Kk 29 -> 11  length 499, flow 0.5 (its record leaves the larger id: E is the twin)
    read 83 stands on I and on Kk (on two pairs: unique on neither), read 30 is a node, read 62 is on no edge, 40 -> 42 stays on one pair.
    Library 3 (invalid_library) has one cross-edge pair and no distance: valid = 0, its pair never counts.
    variant = dp: read 40 stands a second time on A, dp behind the list's last entry: 150 + dp is the running sum the bound is compared with."""
    N, header, recs, pairs = MS.hand_support_graph(None)
    rec = H.rec
    G = rec(20, 21, 3, 201, [(70, 0, 0, 10, 15), (77, 0, 0, 15, 20), (71, 1, 0, 20, 30), (77, 0, 0, 30, 126)])
    Hh = rec(22, 23, 3, 200, [(74, 0, 0, 12, 15), (79, 0, 0, 15, 20), (78, 1, 0, 20, 25), (78, 0, 0, 25, 128)])
    Lq = rec(24, 24, 2, 60, [(75, 0, 0, 5, 9), (76, 0, 0, 9, 46)])
    J = rec(25, 26, 3, 61, [(80, 0, 0, 7, 54)])
    I = rec(27, 28, 3, 500, [(81, 0, 0, 11, 5), (83, 0, 0, 5, 484)])
    Kk = rec(29, 11, 0, 499, [(82, 0, 0, 13, 6), (83, 0, 0, 6, 480)])
    for r, f in ((G, 0), (Hh, 1), (Lq, 2), (J, 1), (I, 1), (Kk, 0.5)):
        t = H.twin_of(r); r["flow"] = t["flow"] = float(f); recs += [r, t]
    p1 = pairs[1] + [(41, 1, 70, 1),                                  # A - G: two components
                     (70, 1, 74, 1), (70, 1, 79, 1),                  # G - Hh: 26 - 22 = 4 and 26 - 37 = -11: gapSum -7 over support 2
                     (77, 1, 50, 1),                                  # G - B: twice from G (both times through the FIRST location, -25), once from B
                     (78, 1, 51, 1),                                  # Hh - B: the first location fails the sign test, the second passes
                     (75, 1, 70, 1),                                  # the loop Lq - G: 26 - 15 = 11
                     (74, 1, 80, 1), (80, 0, 74, 1), (81, 1, 43, 1), (81, 1, 80, 1), (82, 1, 81, 1),
                     (70, 1, 30, 1), (71, 0, 62, 1), (70, 1, 83, 1), (83, 1, 80, 1),      # m2 a node, m2 on no edge, m2 on two pairs, m1 on two pairs
                     (75, 1, 70, 1)]                                  # a pair given twice
    p2 = pairs[2] + [(76, 0, 80, 1), (82, 1, 40, 1)]
    if variant is not None:
        recs[0]["list"] = recs[0]["list"] + [(40, 0, 0, variant, 10)]
        recs[1] = dict(H.twin_of(recs[0]), flow=recs[0]["flow"])
    out = {1: p1, 2: p2}
    if invalid_library:
        out[3] = [(43, 1, 53, 1)]
    return 100, (0, 200, 60), recs, out


def hand_links(variant=None, invalid_library=True):
    N, header, recs, pairs = hand_link_graph(variant, invalid_library)
    g = H.parse_graph(H.graph_text(header, recs))
    return g, pairs, all_links(g, pairs, HAND_K)


# the pairs' ordinals in the hand graph's text
qA, qB, qC, qD, qF, qS, qLp, qG, qH, qLq, qJ, qI, qK = range(13)


def test_restatement_on_the_hand_built_graph():
    g, pairs, rows = hand_links()
    assert [q for q, _, _ in g["pairs"]] == list(range(13))
    t, ests, (lo, hi) = MS.support_inputs(g, pairs)
    assert [(ests[L]["valid"], ests[L]["mean"], ests[L]["upper"]) for L in (1, 2, 3)] == [(1, 146, 221), (1, 113, 233), (0, 0, 0)] and hi == HAND_BOUND
    d = {r[:4]: r[4:] for r in rows}
    # a hit of library 1 needs dist < 221 + 40 - 120 = 141 and adds 146 - 120 - dist = 26 - dist; library 2: dist < 153, -7 - dist
    assert d[(qG, 0, qH, 0)] == (2, -3) and d[(qH, 0, qG, 0)] == (2, -3)               # gapSum -7 over 2: -3, not the floor -4
    assert d[(qG, 0, qB, 0)] == (2, -14) and d[(qB, 0, qG, 0)] == (1, -14)             # read 77 twice on G, both times through its first location: 26 - (25 + 15)
    assert d[(qH, 0, qB, 0)] == (2, -91)                                               # read 78: +47 fails the sign test, -72 passes: 26 - (72 + 45)
    assert d[(qLq, 0, qG, 0)] == (1, 11) and d[(qG, 0, qLq, 0)] == (1, 11)             # a loop takes part; a positive gap
    assert d[(qA, 0, qG, 0)] == (1, -34)                                               # two components
    assert d[(qA, 0, qB, 0)] == (3, -50)                                               # the three mates sage2ov_mates_supports counts at node 10: (-9 - 69 - 72) / 3
    assert all(r[0] != r[2] for r in rows)
    assert d[(qA, 0, qF, 0)] == (1, -12) and not any(qS in (r[0], r[2]) for r in rows)      # flows are not read: F (flow 0.5) takes part; S has no list
    assert d[(qJ, 1, qH, 0)] == (1, -40) and d[(qH, 0, qJ, 1)] == (1, -40)             # a twin half: read 80 at +54 on J's twin, a type-0 mate
    # the invalid library's pair (43, 53) is also in library 1 and counts there once: without library 3 the table is the same
    assert hand_links(invalid_library=False)[2] == rows
    assert len(rows) == HAND_ROWS and sum(r[4] for r in rows) == HAND_RECORDS
    assert len(filtered(g, rows, FINAL)) == HAND_FINAL and len(filtered(g, rows, SMALL)) == HAND_SMALL and len(filtered(g, rows, ALL, 2)) == HAND_TWO


HAND_ROWS, HAND_RECORDS, HAND_FINAL, HAND_SMALL, HAND_TWO = 34, 50, 28, 28, 8      # rows, the sum of their supports, rows under each filter, rows with support >= 2


def test_filters_on_the_hand_built_graph():
    g, pairs, rows = hand_links()
    fin = {r[:4] for r in filtered(g, rows, FINAL)}; sm = {r[:4] for r in filtered(g, rows, SMALL)}
    assert (qG, 0, qH, 0) not in fin and (qG, 0, qH, 0) in sm                          # 201 / 200: not both above 200; G's flow is 0
    assert (qH, 0, qJ, 0) in fin                                                       # 200 / 61, flows 1 / 1: the second clause
    assert (qLq, 0, qG, 0) not in fin                                                  # 60 is not above the threshold 60, and G's flow is 0
    assert (qI, 0, qA, 0) in fin and (qI, 0, qA, 0) not in sm                          # 500 / 300
    assert (qK, 0, qA, 0) in fin and (qK, 0, qA, 0) in sm                              # 499 / 300
    assert (qK, 0, qI, 0) in fin and (qK, 0, qI, 0) not in sm                          # 499 / 500


@pytest.mark.parametrize("mode,l1,f1,l2,f2,want", [
    (FINAL, 201, 0, 201, 0, True), (FINAL, 200, 0, 201, 0, False), (FINAL, 201, 0, 200, 0, False),
    (FINAL, 61, 0.5, 61, 1, True), (FINAL, 60, 1, 61, 1, False), (FINAL, 61, 1, 60, 1, False), (FINAL, 61, 0, 61, 1, False), (FINAL, 61, 1, 61, 0, False),
    (FINAL, 200, 1, 500, 0, False), (FINAL, 200, 1, 61, 2, True),
    (SMALL, 499, 0, 499, 0, True), (SMALL, 500, 1, 499, 1, False), (SMALL, 499, 1, 500, 1, False), (ALL, 1, 0, 1, 0, True)])
def test_filter_clauses(mode, l1, f1, l2, f2, want):
    assert threshold(60) == 60 and threshold(100) == 100 and threshold(151) == 151
    assert passes(mode, l1, f1, l2, f2, 60) is want


@pytest.mark.parametrize("off,ab", [(0, 5), (1, 3)])
def test_restatement_on_the_bound(off, ab):
    """read 40 stands a second time on A, exactly on the bound or one past it; every standing counts its two mates on B through the first location"""
    g0, pairs, _ = hand_links(1)
    _, _, (_, hi) = MS.support_inputs(g0, pairs)
    g, pairs, rows = hand_links(hi - 150 + off)
    assert MS.support_inputs(g, pairs)[2][1] == hi and sum(e[3] for e in g["pairs"][0][1]["list"]) == hi + off
    d = {r[:4]: r[4:] for r in rows}
    assert d[(qA, 0, qB, 0)][0] == ab


# ------------------------------------------------------------------------------------------ the C ABI without a GPU
def test_link_struct_size_against_the_c_compiler(tmp_path):
    assert s2.LINK_DTYPE.itemsize == 44
    src, exe = str(tmp_path / "sz.c"), str(tmp_path / "sz")
    fields = list(s2.LINK_DTYPE.names)
    open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "sage2ov.h"\nint main(void) { printf("%zu", sizeof(sage2ov_link));\n'
                         + "".join('printf(" %%zu", offsetof(sage2ov_link, %s));\n' % f for f in fields) + 'printf(" %zu", sizeof(sage2ov_link_stats)); return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(fx.ROOT, "include"), src, "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got == [s2.LINK_DTYPE.itemsize] + [s2.LINK_DTYPE.fields[f][1] for f in fields] + [C.sizeof(s2.LinkStats)]
    assert (s2.LINKS_ALL, s2.LINKS_FINAL, s2.LINKS_SMALL) == (ALL, FINAL, SMALL)


def test_device_less_context_refuses():
    rng = np.random.default_rng(5)
    reads = sorted({"".join(rng.choice(list("ACGT"), size=60)) for _ in range(20)})
    bases = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(); off = np.arange(0, (len(reads) + 1) * 60, 60, dtype=np.uint64)
    ctx = s2.Context(40, device=-2); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
    for call in (ctx.links, ctx.links_build, lambda: ctx.links(FINAL, 2)):
        with pytest.raises(s2.Sage2ovError) as e:
            call()
        assert e.value.code == -3
    st = ctx.link_stats(); assert (st.halves, st.records, st.keys) == (0, 0, 0)
    n = C.c_uint64(7)
    assert s2.lib().sage2ov_links_count(None, C.c_uint32(0), C.c_uint32(1), C.byref(n)) == -1 and s2.lib().sage2ov_links(None) == -1
    assert s2.lib().sage2ov_links_count(ctx._h, C.c_uint32(3), C.c_uint32(1), C.byref(n)) == -1      # no such mode
    ctx.close()
