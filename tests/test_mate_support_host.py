"""CPU: the restatement of the sweep of ContigExtender::findMatepairSupports (matePair/mergeContigs.cpp:959-1110) as include/sage2ov.h states it, pinned on a
hand-built graph whose numbers were checked against the reference's own getSupportOfEdges -- and the helpers the reference and GPU tests of the supports share.
Also: the size of sage2ov_support and the new calls on a device-less context."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import fixtures as fx
import sage2_amd as s2
import test_mate_estimate_host as H


# ------------------------------------------------------------------------------------------ the restatement (include/sage2ov.h)
def supports(g, table, pairs, ests, max_upper, arl, k):
    """g: H.parse_graph(..), table: H.read_edge_table(g), pairs: {L: [(a, sa, b, sb)]}, ests: {L: H.estimate(..)} -> [(node, pair in, pair out, support)], every
    candidate, zeros included, in ascending (node, in, out) when the pairs' ordinals ascend with the file"""
    pr = H.by_read(table)
    nodes = {a["frm"] for _, a, b in g["pairs"]} | {a["to"] for _, a, b in g["pairs"]}
    mates = {}
    for L, pl in pairs.items():
        for (a, b, ta, tb) in sorted({(a, b, sa, sb) for a, sa, b, sb in pl} | {(b, a, sb, sa) for a, sa, b, sb in pl}):
            mates.setdefault(a, []).append((b, ta, tb, L))
    halves = []
    for q, a, b in g["pairs"]:
        E = a if a["frm"] < a["to"] else b
        halves += [(q, a, a is E), (q, b, b is E)]
    uniq = lambda r, q: pr.get(r) == [q] and r not in nodes
    loc = lambda r, q, isE: table[(r, q)]["forward" if isE else "reverse"]
    cand = lambda h: h[1]["flow"] >= 1 and len(h[1]["list"]) > 0 and h[1]["frm"] != h[1]["to"]
    out = []; leaving = {}
    for h in halves:                                                               # (grouped once: the goldens have thousands of nodes)
        if cand(h):
            leaving.setdefault(h[1]["frm"], []).append(h)
    for i in sorted(nodes):
        ins = [h for h in leaving.get(i, []) if h[1]["type"] in (0, 1)]
        outs = [h for h in leaving.get(i, []) if h[1]["type"] in (2, 3)]
        for (qa, a, ea) in ins:
            for (qb, b, eb) in outs:
                s = run = 0
                for (m1, o, f, dp, dn) in a["list"]:
                    run += dp
                    if run > max_upper:
                        break
                    if not uniq(m1, qa):
                        continue
                    for (m2, t1, t2, L) in mates.get(m1, []):
                        if uniq(m2, qb) and any((1 if t1 else -1) * x < 0 and (1 if t2 else -1) * y < 0 and abs(x) + abs(y) + 2 * arl < ests[L]["upper"] + k
                                                for x in loc(m1, qa, ea) for y in loc(m2, qb, eb)):
                            s += 1
                out.append((i, qa, qb, s))
    return out


def support_inputs(g, pairs):
    """-> (table, {L: estimate}, (minimum upper, maximum upper)) of a parsed graph and its mates, for every library 1 .. the highest in use"""
    t = H.read_edge_table(g); arl = g["header"][2]; nlib = max(pairs) if pairs else 0
    ests = {L: H.estimate(H.mate_distances(t, H.mate_entries(pairs.get(L, []))), arl) for L in range(1, nlib + 1)}
    return t, ests, H.bounds([ests[L] for L in sorted(ests)], arl)


def all_supports(g, pairs, k):
    t, ests, (_, hi) = support_inputs(g, pairs)
    return supports(g, t, pairs, ests, hi, g["header"][2], k)


def with_flows(g, flow_of):
    """the parsed graph with flow_of(ordinal, record) -> (flow of the record, flow of the twin) written into both records of every pair"""
    for q, a, b in g["pairs"]:
        a["flow"], b["flow"] = flow_of(q, a)
    return g


def golden_flow(q, _a=None):
    """the rule of the golden cases: 0 when q % 7 == 3, else 1 for odd q and 2.5 for even q; the twin carries its record's flow"""
    f = 0.0 if q % 7 == 3 else (1.0 if q % 2 else 2.5)
    return f, f


def golden_mates(g, n_reads, seed=3):
    """H.pairs_from_graph(g, 11, N) plus three cross-node pairs per candidate: the j-th entries of a's and b's lists, j < 3, strands 1 - orientation, flipped for one
    pair in six by a seeded rng, the library chosen by the rng"""
    pairs = H.pairs_from_graph(g, 11, n_reads)
    rng = np.random.default_rng(seed)
    by_q = {q: (a, b) for q, a, b in g["pairs"]}
    for (i, qa, qb, _) in supports(g, H.read_edge_table(g), {}, {}, 0, 0, 0):
        a = next(h for h in by_q[qa] if h["frm"] == i); b = next(h for h in by_q[qb] if h["frm"] == i)
        for j in range(min(3, len(a["list"]), len(b["list"]))):
            ea, eb = a["list"][j], b["list"][j]
            sa, sb = 1 - ea[1], 1 - eb[1]
            if rng.integers(0, 6) == 0:
                sa = 1 - sa
            pairs[int(rng.integers(1, 3))].append((ea[0], sa, eb[0], sb))
    return pairs


# ------------------------------------------------------------------------------------------ the hand-built graph
HAND_K = 40


def hand_support_graph(variant=None):
    """(N, header, records, pairs).  Node 10 with two in-halves (A, C: types 0 / 1, listed from 10 outward) and two out-halves (B, D: types 3 / 2); F has flow 0.5,
    S no list, Lp is a loop: none of them is a candidate.  variant = dp: read 30 (a node) and read 48 (then on two pairs) stand on C and D, mates through them are
    added, and read 40 stands a second time on A, dp behind the list's last entry."""
    rec = H.rec
    A = rec(10, 1, 0, 300, [(40, 0, 0, 20, 30), (41, 0, 0, 30, 25), (42, 1, 0, 25, 40), (43, 0, 0, 40, 35), (44, 0, 0, 35, 150)])
    B = rec(10, 30, 3, 320, [(50, 0, 0, 15, 30), (51, 0, 0, 30, 25), (52, 1, 0, 25, 40), (53, 0, 0, 40, 60), (54, 0, 0, 60, 150)])
    Cc = rec(10, 2, 1, 280, [(45, 0, 0, 22, 33), (46, 0, 0, 33, 44), (47, 0, 0, 44, 181)])
    D = rec(10, 31, 2, 290, [(55, 0, 0, 18, 28), (56, 0, 0, 28, 38), (57, 0, 0, 38, 206)])
    F = rec(10, 32, 2, 200, [(58, 0, 0, 18, 182)])
    S = rec(10, 33, 3, 40, [])
    Lp = rec(10, 10, 2, 90, [(59, 1, 0, 12, 78)])
    p1 = [(40, 1, 42, 1), (41, 1, 44, 1), (50, 1, 53, 1), (51, 1, 54, 0), (45, 1, 47, 1), (55, 0, 57, 1), (40, 1, 50, 1), (41, 1, 51, 1), (43, 1, 53, 1), (44, 1, 54, 1),
          (42, 1, 52, 1), (42, 0, 52, 0), (45, 1, 55, 1), (46, 1, 56, 1), (47, 1, 50, 1), (40, 1, 58, 1), (41, 1, 59, 1), (40, 1, 50, 1)]
    p2 = [(40, 1, 41, 1), (50, 1, 51, 1), (52, 1, 54, 1), (40, 1, 51, 1), (45, 1, 56, 1), (46, 1, 57, 1), (47, 1, 55, 1)]
    if variant is not None:
        Cc["list"] += [(30, 0, 0, 5, 5), (48, 0, 0, 6, 6)]
        D["list"] += [(48, 0, 0, 7, 7)]
        p1 += [(30, 1, 55, 1), (48, 1, 56, 1), (46, 1, 48, 1), (60, 1, 61, 1)]
        A["list"] += [(40, 0, 0, variant, 10)]
    recs = []
    for r, f in ((A, 2), (B, 1), (Cc, 1), (D, 1.5), (F, 0.5), (S, 3), (Lp, 2)):
        t = H.twin_of(r); r["flow"] = t["flow"] = float(f); recs += [r, t]
    return 80, (0, 160, 60), recs, {1: p1, 2: p2}


def hand_supports(variant=None):
    N, header, recs, pairs = hand_support_graph(variant)
    g = H.parse_graph(H.graph_text(header, recs))
    return g, pairs, {(qa, qb): s for (i, qa, qb, s) in all_supports(g, pairs, HAND_K) if i == 10}


def test_restatement_on_the_hand_built_graph():
    g, pairs, s = hand_supports()
    assert [q for q, _, _ in g["pairs"]] == [0, 1, 2, 3, 4, 5, 6] and [a["flow"] for _, a, _ in g["pairs"]] == [2, 1, 1, 1.5, 0.5, 3, 2]
    t, ests, (lo, hi) = support_inputs(g, pairs)
    assert [(ests[L]["mean"], ests[L]["deviation"], ests[L]["lower"], ests[L]["upper"]) for L in (1, 2)] == [(146, 25, 71, 221), (113, 40, 0, 233)]
    assert (lo, hi) == (221, 699)
    assert s == {(0, 1): 3, (0, 3): 0, (2, 1): 1, (2, 3): 5}                           # A.B, A.D, C.B, C.D; F, S and Lp give no candidate
    assert len(all_supports(g, pairs, HAND_K)) == 4


@pytest.mark.parametrize("dp,ab", [(885, 7), (886, 5)])
def test_restatement_on_the_variants(dp, ab):
    """read 30 is a node, read 48 stands on two pairs: neither is unique; the second standing of read 40 lies exactly on the bound (885) or one past it (886)"""
    g, pairs, s = hand_supports(dp)
    _, _, (_, hi) = support_inputs(g, pairs)
    assert hi == 1035 and sum(e[3] for e in g["pairs"][0][1]["list"]) == 150 + dp
    assert s == {(0, 1): ab, (0, 3): 0, (2, 1): 1, (2, 3): 5}


# ------------------------------------------------------------------------------------------ the C ABI without a GPU
def test_support_struct_is_24_bytes():
    assert s2.SUPPORT_DTYPE.itemsize == 24
    for name in ("sage2ov_mates_supports", "sage2ov_mates_supports_count", "sage2ov_mates_supports_export", "sage2ov_support_stats_get", "sage2ov_graph_flow_export",
                 "sage2ov_graph_flow_import"):
        assert hasattr(s2.lib(), name)
    # the struct's text in the header: six uint32_t, in the dtype's order (the library asserts sizeof == 24 when it is compiled)
    src = open(os.path.join(fx.ROOT, "include", "sage2ov.h")).read()
    body = re.sub(r"/\*.*?\*/", "", src[src.index("typedef struct sage2ov_support {") + 32:src.index("} sage2ov_support;")], flags=re.S)
    assert re.findall(r"\w+(?=\s*[,;])", body) == list(s2.SUPPORT_DTYPE.names) and set(re.findall(r"\w+_t", body)) == {"uint32_t"}


def test_device_less_context_refuses():
    rng = np.random.default_rng(5)
    reads = sorted({"".join(rng.choice(list("ACGT"), size=60)) for _ in range(20)})
    bases = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(); off = np.arange(0, (len(reads) + 1) * 60, 60, dtype=np.uint64)
    ctx = s2.Context(40, device=-2); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
    for call in (ctx.mates_supports, ctx.mates_supports_build, ctx.graph_flows, lambda: ctx.graph_set_flows(np.zeros(2, dtype=np.float32))):
        with pytest.raises(s2.Sage2ovError) as e:
            call()
        assert e.value.code == -3
    st = ctx.support_stats(); assert (st.candidates, st.records, st.keys) == (0, 0, 0)
    n = C.c_uint64(7)
    assert s2.lib().sage2ov_mates_supports_count(None, C.c_uint32(1), C.byref(n)) == -1 and s2.lib().sage2ov_graph_flow_import(None, None, C.c_uint64(0)) == -1
    ctx.close()
