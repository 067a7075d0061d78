"""GPU: the flows of the step-4 graph and the mate-pair supports of (incoming, outgoing) edge pairs at a node (sage2ov_graph_flow_*, sage2ov_mates_supports;
DESIGN.md 5.12) against the restatement of tests/test_mate_support_host.py over the text sage2ov_graph4_save wrote.  Every comparison is exact equality; the
candidates with support 0 are checked through the candidate count of the statistics."""
import gzip, os
import numpy as np
import pytest
import fixtures as fx
import sage2_amd as s2
import test_mate_estimate_host as H
import test_mate_support_host as MS
from test_gpu_mate_estimate import add_mates, random_store, load_text

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("minimiser_groups_on")]
RS_TILE = 2048


def saved_graph(ctx, tmp_path, flows_from=None, name="saved.graph4"):
    """the graph as graph4_save writes it (its record pairs' ordinals are the table's), parsed; the flows -- the writer puts 0 -- taken from the records of
    `flows_from` (a flat record list) by their content"""
    out = str(tmp_path / name); ctx.graph4_save(out); text = open(out, "rb").read(); g = H.parse_graph(text)
    if flows_from is not None:
        key = lambda r: (r["frm"], r["to"], r["type"], r["len"], tuple(r["list"]))
        fl = {key(r): r["flow"] for r in flows_from}
        MS.with_flows(g, lambda q, a: (fl[key(a)], fl[key(H.twin_of(a))]))
    return g, text


def flat_flows(g):
    return np.asarray([f for _, a, b in g["pairs"] for f in (a["flow"], b["flow"])], dtype=np.float32)


def want_rows(g, pairs, k):
    """every candidate of the restatement as (node, pair_in, pair_out, to_in, to_out, support), ascending (node, pair_in, pair_out)"""
    by_q = {q: (a, b) for q, a, b in g["pairs"]}
    to = lambda q, i: next(h for h in by_q[q] if h["frm"] == i)["to"]
    return sorted((i, qa, qb, to(qa, i), to(qb, i), s) for (i, qa, qb, s) in MS.all_supports(g, pairs, k))


def census(g, bound):
    """(in-halves, out-halves, list entries of in-halves whose running sum is within the bound) of the whole graph, twins included, by the contract"""
    halves = [h for _, a, b in g["pairs"] for h in (a, b) if h["flow"] >= 1 and h["list"] and h["frm"] != h["to"]]
    ins = [h for h in halves if h["type"] in (0, 1)]
    within = sum(int((np.cumsum([e[3] for e in h["list"]]) <= bound).sum()) for h in ins)
    return len(ins), len(halves) - len(ins), within


def check(ctx, g, pairs, k, min_supports=(1, 2, 6)):
    rows = want_rows(g, pairs, k)
    _, _, bounds = MS.support_inputs(g, pairs)
    for ms in min_supports:
        got = ctx.mates_supports(ms)
        assert [tuple(int(v) for v in r) for r in got] == [r for r in rows if r[5] >= ms], ms
    assert ctx.mates_bounds() == bounds
    st = ctx.support_stats()
    assert (st.candidates, st.keys, st.keys2, st.records) == (len(rows), sum(r[5] >= 1 for r in rows), sum(r[5] >= 2 for r in rows), sum(r[5] for r in rows))
    if st.candidates:                                                              # (without a candidate the later stages may not run at all)
        assert (st.in_halves, st.out_halves, st.entries_within) == census(g, bounds[1])
    return rows, st


def hand(variant):
    N, header, recs, pairs = MS.hand_support_graph(variant)
    return N, header, recs, pairs, H.graph_text(header, recs)


@pytest.mark.parametrize("variant", [None, 885, 886])
def test_hand_built_graph_through_the_loader(variant, tmp_path):
    N, header, recs, pairs, text = hand(variant)
    ctx = random_store(N, 5); load_text(ctx, text, tmp_path)
    g, _ = saved_graph(ctx, tmp_path, recs)
    assert np.array_equal(ctx.graph_flows(), flat_flows(g)) and set(ctx.graph_flows().tolist()) == {0.5, 1.0, 1.5, 2.0, 3.0}
    add_mates(ctx, pairs)
    rows, st = check(ctx, g, pairs, MS.HAND_K)
    ab = {None: 3, 885: 7, 886: 5}[variant]
    assert sorted(r[5] for r in rows) == sorted([ab, 0, 1, 5]) and all(r[0] == 10 for r in rows)
    # the twins count too: A, C, twin of B and twin of C are in-halves; the entries within the bound are those of all four (only node 10 has both kinds)
    assert (st.in_halves, st.out_halves, st.sort_passes) == (4, 4, 2)
    if variant is not None:
        assert ctx.mates_bounds()[1] == 1035 and census(g, 1035)[2] - census(g, 1034)[2] == (1 if variant == 885 else 0)
    ctx.close()


def test_flows_written_zero_then_imported(tmp_path):
    N, header, recs, pairs, text = hand(None)
    ctx = random_store(N, 5); load_text(ctx, text, tmp_path); add_mates(ctx, pairs)
    g, _ = saved_graph(ctx, tmp_path, recs)
    direct = ctx.mates_supports(1).tobytes(); assert len(direct) == 3 * 24
    c2 = random_store(N, 5); load_text(c2, H.graph_text(header, [dict(r, flow=0.0) for r in recs]), tmp_path, "zero.graph4"); add_mates(c2, pairs)
    assert len(c2.mates_supports(1)) == 0 and c2.support_stats().candidates == 0 and not c2.graph_flows().any()
    c2.graph_set_flows(flat_flows(g))
    assert c2.mates_supports(1).tobytes() == direct and np.array_equal(c2.graph_flows(), flat_flows(g))
    with pytest.raises(s2.Sage2ovError) as e:
        c2.graph_set_flows(flat_flows(g)[:-1])
    assert e.value.code == -1
    assert c2.mates_supports(1).tobytes() == direct                                 # a refused import changes nothing
    ctx.close(); c2.close()


@pytest.fixture(scope="module")
def goldens():
    """a golden's P.graph4 loaded, flows by rule through graph_set_flows, mates from the graph: computed once per golden and shared"""
    cache = {}

    def get(name):
        if name not in cache:
            m = fx.golden(name); bases, off = fx.make_reads(m["synth"])
            text = gzip.open(os.path.join(fx.GOLDEN, name + ".graph4.gz")).read()
            g = MS.with_flows(H.parse_graph(text), MS.golden_flow)
            ctx = s2.Context(m["k"]); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
            pairs = MS.golden_mates(g, ctx.reads_stats().unique_reads)
            cache[name] = (ctx, m["k"], text, g, pairs)
        return cache[name]
    yield get
    for c in cache.values():
        c[0].close()


def load_golden(ctx, text, g, pairs, tmp_path):
    src = str(tmp_path / "in.graph4"); open(src, "wb").write(text); ctx.graph_load_composite(src)
    ctx.graph_set_flows(flat_flows(g)); ctx.mates_clear(); add_mates(ctx, pairs)


@pytest.mark.parametrize("name", ["g4_highcopy_k21", "g9_repeats160k_k40"])
def test_goldens_with_flows_by_rule(name, goldens, tmp_path):
    ctx, k, text, g, pairs = goldens(name)
    load_golden(ctx, text, g, pairs, tmp_path)
    before = ([ctx.mates(L)[0].tobytes() for L in pairs], [x.tobytes() for x in ctx.read_edges()])
    rows, st = check(ctx, g, pairs, k)
    assert any(r[5] >= 2 for r in rows) and any(r[5] == 0 for r in rows)            # (not vacuous)
    # nothing else moves: the written graph (flow column 0), the mate table, the read-to-edge table
    out = str(tmp_path / "again.graph4"); ctx.graph4_save(out)
    assert open(out, "rb").read() == text and ([ctx.mates(L)[0].tobytes() for L in pairs], [x.tobytes() for x in ctx.read_edges()]) == before


def test_memory_diet_mode_gives_the_same_table(monkeypatch, goldens, tmp_path):
    ctx, k, text, g, pairs = goldens("g4_highcopy_k21")
    load_golden(ctx, text, g, pairs, tmp_path)
    want = ctx.mates_supports(1).tobytes(); assert len(want) > 0
    monkeypatch.setenv("SAGE2OV_MEMORY_DIET", "1")
    m = fx.golden("g4_highcopy_k21"); bases, off = fx.make_reads(m["synth"])
    c2 = s2.Context(k); c2.reads_add_ascii(bases, off); c2.reads_organize()
    load_golden(c2, text, g, pairs, tmp_path)
    assert c2.mates_supports(1).tobytes() == want
    c2.close()


@pytest.mark.parametrize("name", ["g1_clean100_k21", "g4_highcopy_k21"])
def test_steps_1_to_4_leave_flows_of_zero_then_flows_by_rule(name, tmp_path):
    """after graph_simplify every flow is 0: an empty table and no error; with flows handed in the table is the restatement's; a second graph_simplify drops it.
    g1 is one edge (no candidate whatever the flows), g4 has 551 candidates"""
    m = fx.golden(name); bases, off = fx.make_reads(m["synth"])
    ctx = s2.Context(m["k"]); ctx.reads_add_ascii(bases, off); ctx.reads_organize(); ctx.run_steps23(); ctx.graph_simplify()
    g, text = saved_graph(ctx, tmp_path)
    assert text == gzip.open(os.path.join(fx.GOLDEN, name + ".graph4.gz")).read()
    assert not ctx.graph_flows().any() and len(ctx.graph_flows()) == 2 * len(g["pairs"])
    pairs = MS.golden_mates(MS.with_flows(g, MS.golden_flow), ctx.reads_stats().unique_reads)
    add_mates(ctx, pairs)
    assert len(ctx.mates_supports(1)) == 0 and ctx.support_stats().candidates == 0
    ctx.graph_set_flows(flat_flows(g))
    rows, _ = check(ctx, g, pairs, m["k"], min_supports=(1, 2))
    assert len(rows) == (0 if name.startswith("g1") else 551)
    ctx.graph_simplify()
    assert not ctx.graph_flows().any() and len(ctx.mates_supports(1)) == 0 and ctx.support_stats().candidates == 0
    ctx.close()


def test_star_across_the_sort_tiles(tmp_path):
    """one node, 3 in-halves and 3 out-halves with lists of 3 000 entries (distPrevious 1): one key with more than two radix tiles of records, more than three
    tiles in all, every entry within the bound"""
    n, c = 3000, 1
    ids = iter(range(8, 8 + 6 * n))
    lists = [[(next(ids), 0, 0, 1, 1) for _ in range(n)] for _ in range(6)]
    recs = []
    for x in range(6):
        r = H.rec(c, 2 + x, (0, 1, 0, 3, 2, 3)[x], 4000, lists[x]); t = H.twin_of(r); r["flow"] = t["flow"] = 1.0; recs += [r, t]
    N = 8 + 6 * n; header = (0, 2 * N, 60)
    same = [(lst[i][0], 1, lst[i + (2000 if i % 2 else 2900)][0], 1) for lst in lists for i in range(0, 100)]          # insert sizes far above the lists' length
    cross = []
    for a in range(3):
        for b in range(3, 6):
            if (a, b) == (0, 3):
                cross += [(lists[a][j][0], 1, lists[b][j + d][0], 1) for j in range(1500) for d in (0, 1, 2)]
            else:
                cross += [(lists[a][j][0], 1, lists[b][j][0], 1) for j in range(250)]
    pairs = {1: same + cross}
    g = H.parse_graph(H.graph_text(header, recs))
    t, ests, (_, hi) = MS.support_inputs(g, pairs)
    assert ests[1]["valid"] == 1 and ests[1]["upper"] > n + 2 * 60 and hi > n
    sup = {(qa, qb): s for _, qa, qb, s in MS.all_supports(g, pairs, 40)}
    assert len(sup) == 9 and sup[(0, 3)] >= 2 * RS_TILE and sum(sup.values()) >= 3 * RS_TILE and min(sup.values()) == 250      # the restatement says so
    ctx = random_store(N, 9); load_text(ctx, H.graph_text(header, recs), tmp_path)
    gs, _ = saved_graph(ctx, tmp_path, recs)
    assert [q for q, _, _ in gs["pairs"]] == [q for q, _, _ in g["pairs"]]
    add_mates(ctx, pairs)
    rows, st = check(ctx, gs, pairs, 40, min_supports=(1, 2 * RS_TILE))
    assert (st.in_halves, st.out_halves, st.entries_within, st.sort_passes) == (6, 6, 6 * n, 2)      # (the twins of the six halves are three ins and three outs at the far ends)
    ctx.close()


def test_staleness_and_call_order(tmp_path):
    N, header, recs, pairs, text = hand(None)
    ctx = random_store(N, 5)
    for call in (ctx.mates_supports, ctx.mates_supports_build, ctx.graph_flows, lambda: ctx.graph_set_flows(np.zeros(14, dtype=np.float32))):      # no graph
        with pytest.raises(s2.Sage2ovError) as e:
            call()
        assert e.value.code == -1
    load_text(ctx, text, tmp_path)
    g, _ = saved_graph(ctx, tmp_path, recs)
    rows, _ = check(ctx, g, {}, MS.HAND_K, min_supports=(1,))                        # before any mates: four candidates, an empty table
    assert len(rows) == 4 and len(ctx.mates_supports(1)) == 0
    add_mates(ctx, {1: pairs[1]}); check(ctx, g, {1: pairs[1]}, MS.HAND_K)
    add_mates(ctx, {2: pairs[2]}); check(ctx, g, pairs, MS.HAND_K)                  # mates added: recomputed
    ctx.mates_clear(); assert len(ctx.mates_supports(1)) == 0
    add_mates(ctx, pairs); check(ctx, g, pairs, MS.HAND_K)
    fl = flat_flows(g); f2 = fl.copy(); f2[0] = f2[1] = 0.5                          # A is no candidate any more
    ctx.graph_set_flows(f2)
    for q, a, b in g["pairs"]:
        if q == 0:
            a["flow"] = b["flow"] = 0.5
    rows, _ = check(ctx, g, pairs, MS.HAND_K); assert sorted(r[5] for r in rows) == [1, 5]
    # another graph: the old table is gone
    N2, header2, recs2, pairs2, text2 = hand(885)
    load_text(ctx, text2, tmp_path, "v.graph4"); g2, _ = saved_graph(ctx, tmp_path, recs2, "v.saved")
    ctx.mates_clear(); add_mates(ctx, pairs2)
    rows, _ = check(ctx, g2, pairs2, MS.HAND_K); assert max(r[5] for r in rows) == 7
    ctx.close()
