"""CPU: the restatement of the merge rounds (tests/extend_model.py: mergeEdgesAndUpdate, one findMatepairSupports, the loop of extendContigs, its threshold) pinned
on the hand-built graph of test_mate_support_host -- and sage2ov_extend_threshold, the record sizes and the new calls on a device-less context."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import fixtures as fx
import sage2_amd as s2
import extend_model as X
import test_mate_estimate_host as H
import test_mate_support_host as MS

K = MS.HAND_K


def hand(flows=None, extra=None):
    """the hand-built graph as a model graph, its mates and pinned bounds; flows: {record index in the flat list: flow}; extra: mate pairs added to library 1"""
    N, header, recs, pairs = MS.hand_support_graph()
    for x, f in (flows or {}).items():
        recs[x]["flow"] = recs[x ^ 1]["flow"] = float(f)
    if extra:
        pairs = {1: pairs[1] + list(extra), 2: pairs[2]}
    g = X.Graph(H.parse_graph(H.graph_text(header, recs)))
    return g, pairs, X.Bounds(g, pairs), header, recs


def rounds(g, pairs, b, high, low=1):
    out = []
    while True:
        out.append(X.round_(g, pairs, b, K, high, low))
        if not out[-1]["merges"]:
            return out


# the two merged pairs of the hand-built graph, written out by hand from getListOfReads (overlapGraph.cpp:299-336): twin(C) + node 10 + D and twin(A) + node 10 + B
CD = H.rec(2, 31, 0, 570, [(47, 1, 0, 181, 44), (46, 1, 0, 44, 33), (45, 1, 0, 33, 22), (10, 1, 0, 22, 18), (55, 0, 0, 18, 28), (56, 0, 0, 28, 38), (57, 0, 0, 38, 206)])
DC = H.rec(31, 2, 3, 570, [(57, 1, 0, 206, 38), (56, 1, 0, 38, 28), (55, 1, 0, 28, 18), (10, 0, 0, 18, 22), (45, 0, 0, 22, 33), (46, 0, 0, 33, 44), (47, 0, 0, 44, 181)])
AB = H.rec(1, 30, 3, 620, [(44, 1, 0, 150, 35), (43, 1, 0, 35, 40), (42, 0, 0, 40, 25), (41, 1, 0, 25, 30), (40, 1, 0, 30, 20), (10, 1, 0, 20, 15),
                          (50, 0, 0, 15, 30), (51, 0, 0, 30, 25), (52, 1, 0, 25, 40), (53, 0, 0, 40, 60), (54, 0, 0, 60, 150)])
BA = H.rec(30, 1, 0, 620, [(54, 1, 0, 150, 60), (53, 1, 0, 60, 40), (52, 0, 0, 40, 25), (51, 1, 0, 25, 30), (50, 1, 0, 30, 15), (10, 0, 0, 15, 20),
                          (40, 0, 0, 20, 30), (41, 0, 0, 30, 25), (42, 1, 0, 25, 40), (43, 0, 0, 40, 35), (44, 0, 0, 35, 150)])


def with_flow(r, f):
    return dict(r, flow=float(f))


def test_hand_built_graph_round_by_round():
    g, pairs, b, header, recs = hand()
    A, At, B, Bt, Cc, Ct, D, Dt, F, Ft, S, St, Lp, Lt = recs
    assert b.max_upper == 699
    # the file order of the graph as loaded: node 1 (twin of A), node 2 (twin of C), node 10 in pool order, the loop twice
    assert g.text() == H.graph_text(header, [At, A, Ct, Cc, B, Bt, D, Dt, F, Ft, S, St, Lp, Lt, Lt, Lp])
    r1 = X.round_(g, pairs, b, K, 2)
    assert X.merges_rows(r1) == [(10, 2, 31, 5, 1, 3, 1, 1.0, 0, 1, 0)]               # C.D: C (flow 1) goes, D stays; the new pair takes C's place in the file
    assert (r1["entries"], r1["at_threshold"], r1["refused"], r1["blocked"], r1["outside_reference"]) == (2, 2, 0, 0, True)      # A.B went with the node
    D5, Dt5 = with_flow(D, 0.5), with_flow(Dt, 0.5)
    assert g.text() == H.graph_text(header, [At, A, with_flow(CD, 1), with_flow(DC, 1), B, Bt, D5, Dt5, F, Ft, S, St, Lp, Lt, Lt, Lp])
    r2 = X.round_(g, pairs, b, K, 2)
    assert X.merges_rows(r2) == [(10, 1, 30, 3, 0, 2, 1, 1.0, 3, 0, 1)]               # A.B: A goes from 2 to 1 and stays, B goes
    assert (r2["entries"], r2["outside_reference"]) == (1, False)
    A1, At1 = with_flow(A, 1), with_flow(At, 1)
    want = H.graph_text(header, [At1, A1, with_flow(AB, 1), with_flow(BA, 1), with_flow(CD, 1), with_flow(DC, 1), D5, Dt5, F, Ft, S, St, Lp, Lt, Lt, Lp])
    assert g.text() == want                                                          # the new pair 1 -> 30 comes after the older pair written at node 1
    r3 = X.round_(g, pairs, b, K, 2)
    assert r3["merges"] == [] and r3["entries"] == 0 and g.text() == want


def test_hand_built_graph_variants():
    g, pairs, b, _, _ = hand()
    rs = rounds(g, pairs, b, 4)                                                      # A.B (3) is below the threshold: one merge, then a fixed point
    assert [len(r["merges"]) for r in rs] == [1, 0] and [r["at_threshold"] for r in rs] == [1, 0] and rs[1]["entries"] == 1
    g, pairs, b, _, _ = hand()
    t0 = g.text(); rs = rounds(g, pairs, b, 6)
    assert [len(r["merges"]) for r in rs] == [0] and rs[0]["entries"] == 2 and g.text() == t0
    # C.B raised from 1 to 2 by two added pairs (one of them on the wrong strand: it does not count): every entry sees an in- or out-support above low
    g, pairs, b, _, _ = hand(extra=[(45, 1, 50, 1), (46, 0, 51, 1)])
    sup = {(i, qa, qb): s for i, qa, qb, s in MS.supports(g.parsed(), H.read_edge_table(g.parsed()), pairs, b.ests, b.max_upper, b.arl, K)}
    assert sup[(10, 2, 1)] == 2 and sup[(10, 2, 3)] == 5 and sup[(10, 0, 1)] == 3
    t0 = g.text(); rs = rounds(g, pairs, b, 2)
    assert [len(r["merges"]) for r in rs] == [0] and (rs[0]["entries"], rs[0]["refused"]) == (3, 3) and g.text() == t0
    assert len(rounds(g, pairs, b, 2, low=2)[0]["merges"]) == 1                      # (with low = 2 the same entries merge)
    # C with flow 2 keeps the in-edge: inside the reference's defined behaviour, no ties
    g, pairs, b, _, _ = hand(flows={4: 2})
    rs = rounds(g, pairs, b, 2)
    assert [X.merges_rows(r) for r in rs] == [[(10, 2, 31, 5, 1, 3, 2, 1.0, 0, 0, 0)], [(10, 1, 30, 3, 0, 3, 1, 1.0, 3, 0, 1)], []]
    assert not any(r["ties"] or r["outside_reference"] for r in rs)
    assert [h["flow"] for h in g.h[4:8]] == [1.0, 1.0, 0.5, 0.5]


def tiny(t1, t2, f1=1.0, f2=1.0, l1=((7, 0, 0, 11, 12),), l2=((8, 1, 0, 13, 14),), to=3):
    """1 -> 2 (type t1) and 2 -> `to` (type t2) with one-entry lists (or none)"""
    a = H.rec(1, 2, t1, 100, l1); b = H.rec(2, to, t2, 200, l2)
    recs = []
    for r, f in ((a, f1), (b, f2)):
        t = H.twin_of(r); r["flow"] = t["flow"] = float(f); recs += [r, t]
    return X.Graph(H.parse_graph(H.graph_text((0, 10, 50), recs)))


@pytest.mark.parametrize("t1,t2,want", [(0, 0, 0), (1, 2, 0), (0, 1, 1), (1, 3, 1), (2, 0, 2), (3, 2, 2), (2, 1, 3), (3, 3, 3), (0, 2, None), (3, 0, None)])
def test_primitive_types(t1, t2, want):
    g = tiny(t1, t2)
    nh = g.merge(0, 2)
    if want is None:
        assert nh is None and len(g.h) == 4 and all(g.alive)
        return
    assert nh == 4 and g.alive == [False, False, True]                                # both flows 1: both operands go
    fw, tw = g.h[4], g.h[5]
    assert (fw["frm"], fw["to"], fw["type"], fw["len"], fw["flow"]) == (1, 3, want, 300, 1.0) and (tw["frm"], tw["to"], tw["type"], tw["len"]) == (3, 1, H.flip_type(want), 300)
    assert fw["list"] == [(7, 0, 0, 11, 12), (2, 1 if t1 in (1, 3) else 0, 0, 12, 13), (8, 1, 0, 13, 14)]
    assert tw["list"] == [(8, 0, 0, 14, 13), (2, 1 if H.flip_type(t2) in (1, 3) else 0, 0, 13, 12), (7, 1, 0, 12, 11)]


def test_primitive_flows_simple_edges_loops_and_parallels():
    g = tiny(0, 0, 3.0, 2.0); g.merge(0, 2, 2)                                       # type 2: the minimum; e2 goes, e1 keeps 1 on both halves
    assert g.h[4]["flow"] == 2.0 and g.alive == [True, False, True] and (g.h[0]["flow"], g.h[1]["flow"]) == (1.0, 1.0)
    g = tiny(0, 0, 0.0, 0.0); g.merge(0, 2)                                          # both flows 0: flow 0, both go
    assert g.h[4]["flow"] == 0.0 and g.alive == [False, False, True]
    g = tiny(0, 0, 0.0, 2.5); g.merge(0, 2)                                          # one flow 0: type 1 gives 1.0; e1 (0 <= 1) goes, e2 keeps 1.5
    assert g.h[4]["flow"] == 1.0 and g.alive == [False, True, True] and g.h[2]["flow"] == 1.5
    g = tiny(0, 0, l1=()); g.merge(0, 2)                                             # a simple e1: the node entry takes e1's length (the twin of a type-0 edge has type 3: orientation 1)
    assert g.h[4]["list"] == [(2, 0, 0, 100, 13), (8, 1, 0, 13, 14)] and g.h[5]["list"] == [(8, 0, 0, 14, 13), (2, 1, 0, 13, 100)]
    g = tiny(0, 0, l2=()); g.merge(0, 2)                                             # a simple e2
    assert g.h[4]["list"] == [(7, 0, 0, 11, 12), (2, 0, 0, 12, 200)] and g.h[5]["list"] == [(2, 1, 0, 200, 12), (7, 1, 0, 12, 11)]
    g = tiny(0, 0, to=1); assert g.merge(0, 2) == 4                                  # the result is a loop 1 -> 1: written twice
    assert (g.h[4]["frm"], g.h[4]["to"]) == (1, 1) and g.text().count("1\t1\t0\t1\t300\t1\t3\n") + g.text().count("1\t1\t3\t1\t300\t1\t3\n") == 4
    assert g.merge(4, 5) is None and g.merge(4, 4) is None                           # a loop with its own twin, with itself
    g = tiny(0, 0, 2.0, 2.0)
    assert g.merge(0, 2) == 4 and g.alive == [True, True, True] and g.merge(0, 2) == 6      # 1 -> 3 twice: parallel edges, the newer one later in the file
    assert g.alive == [False, False, True, True] and g.first_halves() == [4, 6] and g.ordinals() == {2: 0, 3: 1}
    assert g.merge(0, 2) is None                                                     # dead operands are refused


@pytest.mark.parametrize("reads,arl,gs,it,want", [
    (2099, 100, 10000, 1, 4),            # 209900 / 10000 = 20 (not 20.99): 0.2 * 20 = 4
    (2100, 100, 10000, 1, 5),            # 21: 4.2 -> 5
    (1000, 150, 10000, 1, 2),            # 15: 0.2 * 15 * (100 / 150) = 2.0000000000000004 as a double, 2.0f for ceilf
    (1000, 150, 10000, 9, 2),            # a small genome keeps 0.20 in every iteration
    (10 ** 9, 100, 2 * 10 ** 9, 3, 10), (10 ** 9, 100, 2 * 10 ** 9, 4, 5), (10 ** 9, 100, 2 * 10 ** 9, 6, 5), (10 ** 9, 100, 2 * 10 ** 9, 7, 3),
    (10 ** 9, 100, 10 ** 9, 7, 20),      # 10^9 is not above 10^9
    (5, 100, 10000, 1, 0)])
def test_extend_threshold(reads, arl, gs, it, want):
    assert X.threshold(reads, arl, gs, it) == want
    assert s2.extend_threshold(reads, arl, gs, it) == want


def test_extend_threshold_refuses_zero():
    for args in ((10, 0, 10, 1), (10, 10, 0, 1), (10, 10, 10, 0)):
        with pytest.raises(s2.Sage2ovError) as e:
            s2.extend_threshold(*args)
        assert e.value.code == -1


def test_record_sizes():
    assert s2.MERGE_DTYPE.itemsize == 40 and C.sizeof(s2.ExtendCounts) == 96 and C.sizeof(s2.ExtendStats) == 208
    src = open(os.path.join(fx.ROOT, "include", "sage2ov.h")).read()
    body = re.sub(r"/\*.*?\*/", "", src[src.index("typedef struct sage2ov_merge {") + 30:src.index("} sage2ov_merge;")], flags=re.S)
    names = [n for n in re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)]
    assert names == list(s2.MERGE_DTYPE.names)
    for name in ("sage2ov_graph_merge_pairs", "sage2ov_extend_threshold", "sage2ov_extend_round", "sage2ov_extend_by_supports", "sage2ov_extend_merges_count",
                 "sage2ov_extend_merges_export", "sage2ov_extend_stats_get", "sage2ov_graph6_save"):
        assert hasattr(s2.lib(), name)


def test_device_less_context_refuses(tmp_path):
    rng = np.random.default_rng(5)
    reads = sorted({"".join(rng.choice(list("ACGT"), size=60)) for _ in range(20)})
    bases = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(); off = np.arange(0, (len(reads) + 1) * 60, 60, dtype=np.uint64)
    ctx = s2.Context(40, device=-2); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
    for call in (lambda: ctx.merge_pairs([(0, 0)], [(1, 0)]), lambda: ctx.extend_round(2), ctx.extend_by_supports, lambda: ctx.graph6_save(str(tmp_path / "x.graph6"))):
        with pytest.raises(s2.Sage2ovError) as e:
            call()
        assert e.value.code == -3
    with pytest.raises(s2.Sage2ovError) as e:                                        # decided without a device
        ctx.merge_pairs([(0, 0)], [(1, 0)], type_of_merge=3)
    assert e.value.code == -1
    assert len(ctx.extend_merges()) == 0 and ctx.extend_stats().rounds == 0 and ctx.extend_stats().total.merges == 0
    L = s2.lib(); n = C.c_uint64(7)
    assert L.sage2ov_extend_round(None, C.c_int(2), C.c_int(1), C.byref(n)) == -1 and L.sage2ov_graph_merge_pairs(None, None, None, None, None, C.c_uint64(0), C.c_int(1), None) == -1
    assert L.sage2ov_extend_merges_count(None, C.byref(n)) == -1 and L.sage2ov_graph6_save(None, None) == -1 and L.sage2ov_extend_stats_get(None, None) == -1
    assert not os.path.exists(str(tmp_path / "x.graph6"))
    ctx.close()
