"""GPU: the scaffold links of half-edge pairs (sage2ov_links) against the restatement of tests/test_links_host.py over the text sage2ov_graph4_save
wrote -- rows, order, the three filters and min_support -- and against the rows the reference itself computed (tests/golden/*.links.txt.gz, by the subset rule of
LH.same_as_reference).  Every comparison is exact equality."""
import gzip, os
import numpy as np
import pytest
import fixtures as fx
import sage2_amd as s2
import test_mate_estimate_host as H
import test_mate_support_host as MS
import test_links_host as LH
from test_gpu_mate_estimate import add_mates, random_store, load_text
from test_gpu_mate_support import saved_graph, flat_flows

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("minimiser_groups_on")]
RS_TILE = 2048


def want_rows(g, rows):
    """the restatement's rows as LINK_DTYPE tuples"""
    hv = LH.halves_of(g); E = LH.e_half(g); out = []
    for (qa, sa, qb, sb, s, gap) in rows:
        a, b = hv[(qa, sa)][0], hv[(qb, sb)][0]
        out.append((qa, qb, a["frm"], a["to"], b["frm"], b["to"], E[qa]["len"], E[qb]["len"], s, gap, sa, sb, a["type"], b["type"]))
    return out


def census(g, pairs, k):
    """(halves walked, entries within the bound, unique entries, mate entries probed) by the contract"""
    t, ests, (_, hi) = MS.support_inputs(g, pairs)
    pr = H.by_read(t); nodes = {a["frm"] for _, a, b in g["pairs"]} | {a["to"] for _, a, b in g["pairs"]}; arl = g["header"][2]
    counts = {}
    for L, pl in pairs.items():
        if ests[L]["valid"] and ests[L]["upper"] + k - 2 * arl > 0:
            for (a, b, ta, tb) in {(a, b, sa, sb) for a, sa, b, sb in pl} | {(b, a, sb, sa) for a, sa, b, sb in pl}:
                counts[a] = counts.get(a, 0) + 1
    halves = within = unique = probed = 0
    for q, a, b in g["pairs"]:
        for h in (a, b):
            halves += 1 if h["list"] else 0; run = 0
            for e in h["list"]:
                run += e[3]
                if run > hi:
                    break
                within += 1
                if e[0] not in nodes and pr.get(e[0]) == [q]:
                    unique += 1; probed += counts.get(e[0], 0)
    return halves, within, unique, probed


def check(ctx, g, pairs, k, min_supports=(1, 2, 3)):
    rows = LH.all_links(g, pairs, k)
    for mode in (LH.ALL, LH.FINAL, LH.SMALL):
        for ms in min_supports:
            got = ctx.links(mode, ms)
            assert [tuple(int(v) for v in r) for r in got] == want_rows(g, LH.filtered(g, rows, mode, ms)), (mode, ms)
    st = ctx.link_stats()
    assert (st.keys, st.records) == (len(rows), sum(r[4] for r in rows))
    if st.records:                                                                 # (without a record the later stages do not run)
        assert (st.halves, st.entries_within, st.unique_entries, st.mate_entries) == census(g, pairs, k)
    return rows, st


def hand(variant):
    N, header, recs, pairs = LH.hand_link_graph(variant)
    return N, header, recs, pairs, H.graph_text(header, recs)


@pytest.mark.parametrize("variant", [None, 666, 667])
def test_hand_built_graph_through_the_loader(variant, tmp_path):
    N, header, recs, pairs, text = hand(variant)
    ctx = random_store(N, 5); load_text(ctx, text, tmp_path)
    g, _ = saved_graph(ctx, tmp_path, recs)
    add_mates(ctx, pairs)
    rows, st = check(ctx, g, pairs, LH.HAND_K)
    assert ctx.mates_insert(3).valid == 0 and ctx.mates_bounds()[1] == (LH.HAND_BOUND if variant is None else 816)
    by_ends = {(r["from_a"], r["to_a"], r["from_b"], r["to_b"]): (int(r["support"]), int(r["gap"])) for r in ctx.links()}
    if variant is None:
        assert (len(rows), st.records) == (LH.HAND_ROWS, LH.HAND_RECORDS)
        assert by_ends[(20, 21, 22, 23)] == (2, -3) and by_ends[(20, 21, 10, 30)] == (2, -14) and by_ends[(10, 30, 20, 21)] == (1, -14) and by_ends[(24, 24, 20, 21)] == (1, 11)
        assert by_ends[(22, 23, 10, 30)] == (2, -91) and by_ends[(26, 25, 22, 23)] == (1, -40)      # the second location passes the sign test; a twin half as a
    else:
        assert by_ends[(10, 1, 10, 30)][0] == (5 if variant == 666 else 3)          # read 40's second standing: on the bound, one past it
    ctx.close()


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
            # the mates are those the reference's rows were recorded with: chosen from the file's record pairs as its loader sees them (a loop written twice: two)
            pairs = LH.golden_pairs(name, MS.with_flows(H.parse_graph(text, fold=False), MS.golden_flow), ctx.reads_stats().unique_reads)
            cache[name] = (ctx, m["k"], text, g, pairs)
        return cache[name]
    yield get
    for c in cache.values():
        c[0].close()


def load_golden(ctx, text, g, pairs, tmp_path):
    src = str(tmp_path / "in.graph4"); open(src, "wb").write(text); ctx.graph_load_composite(src)
    ctx.graph_set_flows(flat_flows(g)); ctx.mates_clear(); add_mates(ctx, pairs)


def everything_else(ctx, pairs, tmp_path, name):
    out = str(tmp_path / name); ctx.graph4_save(out)
    return (open(out, "rb").read(), [x.tobytes() for L in pairs for x in ctx.mates(L)], [x.tobytes() for x in ctx.read_edges()], ctx.mates_supports(1).tobytes(),
            ctx.contigs().tobytes())


@pytest.mark.parametrize("name", ["g4_highcopy_k21", "g9_repeats160k_k40"])
def test_goldens_against_the_restatement_and_the_reference_rows(name, goldens, tmp_path):
    ctx, k, text, g, pairs = goldens(name)
    load_golden(ctx, text, g, pairs, tmp_path)
    before = everything_else(ctx, pairs, tmp_path, "before.graph4")
    rows, st = check(ctx, g, pairs, k)
    LH.same_as_reference(g, rows, LH.golden_links(name))
    hv = LH.halves_of(g)
    assert any(hv[(r[0], r[1])][0]["frm"] != hv[(r[2], r[3])][0]["frm"] for r in rows) and any(r[4] >= 3 for r in rows)      # (not vacuous)
    assert LH.filtered(g, rows, LH.FINAL) and LH.filtered(g, rows, LH.SMALL)
    # nothing else moves: the written graph, the mate table, the read-to-edge table, the supports at a node, the contig table
    assert everything_else(ctx, pairs, tmp_path, "after.graph4") == before and before[0] == text


def test_memory_diet_mode_gives_the_same_table(monkeypatch, goldens, tmp_path):
    ctx, k, text, g, pairs = goldens("g4_highcopy_k21")
    load_golden(ctx, text, g, pairs, tmp_path)
    want = [ctx.links(mode).tobytes() for mode in (LH.ALL, LH.FINAL, LH.SMALL)]; assert all(len(w) > 0 for w in want)
    monkeypatch.setenv("SAGE2OV_MEMORY_DIET", "1")
    m = fx.golden("g4_highcopy_k21"); bases, off = fx.make_reads(m["synth"])
    c2 = s2.Context(k); c2.reads_add_ascii(bases, off); c2.reads_organize()
    load_golden(c2, text, g, pairs, tmp_path)
    assert [c2.links(mode).tobytes() for mode in (LH.ALL, LH.FINAL, LH.SMALL)] == want
    c2.close()


@pytest.mark.parametrize("name", ["g1_clean100_k21", "g4_highcopy_k21"])
def test_steps_1_to_4_in_process(name, tmp_path):
    """the graph step 4 left in HBM, flows 0: FINAL's second clause never holds.  g1 is one edge: no two pairs, an empty table and no error"""
    m = fx.golden(name); bases, off = fx.make_reads(m["synth"])
    ctx = s2.Context(m["k"]); ctx.reads_add_ascii(bases, off); ctx.reads_organize(); ctx.run_steps23(); ctx.graph_simplify()
    g, text = saved_graph(ctx, tmp_path)
    assert text == gzip.open(os.path.join(fx.GOLDEN, name + ".graph4.gz")).read()
    pairs = MS.golden_mates(MS.with_flows(H.parse_graph(text), MS.golden_flow), ctx.reads_stats().unique_reads)
    MS.with_flows(g, lambda q, a: (0.0, 0.0))
    add_mates(ctx, pairs)
    rows, _ = check(ctx, g, pairs, m["k"], min_supports=(1, 2))
    assert (len(rows) == 0) == name.startswith("g1")
    ctx.graph_simplify()                                                            # a second step 4: the table goes with the graph, and comes back the same
    assert [tuple(int(v) for v in r) for r in ctx.links()] == want_rows(g, rows)
    ctx.close()


def test_hub_across_the_sort_tiles(tmp_path):
    """one hub half U (four unique reads) linked by mates to 1 600 partner edges of two reads each, none sharing a node with it: 6 400 records carry U as `a` (more than
    three radix tiles of one first word), 12 800 in all; Z only gives the library its insert size"""
    n = 1600
    nodes = iter(range(1, 2 * (n + 2) + 1)); reads = iter(range(2 * (n + 2) + 1, 2 * (n + 2) + 1 + 4 + 300 + 2 * n))
    rec = H.rec
    U = rec(next(nodes), next(nodes), 3, 300, [(next(reads), 0, 0, 1, 1) for _ in range(4)])
    Z = rec(next(nodes), next(nodes), 3, 4000, [(next(reads), 0, 0, 1, 1) for _ in range(300)])
    P = [rec(next(nodes), next(nodes), 3, 100 + (i % 5) * 100, [(next(reads), 0, 0, 1, 1) for _ in range(2)]) for i in range(n)]
    recs = []
    for i, r in enumerate([U, Z] + P):
        t = H.twin_of(r); r["flow"] = t["flow"] = float(i % 2); recs += [r, t]
    N = 2 * (n + 2) + 4 + 300 + 2 * n; header = (0, 2 * N, 60)
    same = [(Z["list"][i][0], 1, Z["list"][i + (200 if i % 2 else 290)][0], 1) for i in range(10)]
    cross = [(u[0], 1, p["list"][0][0], 1) for u in U["list"] for p in P]
    pairs = {1: same + cross}
    g = H.parse_graph(H.graph_text(header, recs))
    t, ests, (_, hi) = MS.support_inputs(g, pairs)
    assert ests[1]["valid"] == 1 and ests[1]["upper"] + 40 - 120 > 6
    want = LH.all_links(g, pairs, 40)
    from_u = [r for r in want if r[:2] == (0, 0)]
    assert len(from_u) == n and all(r[4] == 4 for r in from_u) and sum(r[4] for r in from_u) > 3 * RS_TILE and sum(r[4] for r in want) == 8 * n      # the restatement says so
    ctx = random_store(N, 9); load_text(ctx, H.graph_text(header, recs), tmp_path)
    gs, _ = saved_graph(ctx, tmp_path, recs)
    assert [q for q, _, _ in gs["pairs"]] == [q for q, _, _ in g["pairs"]]
    add_mates(ctx, pairs)
    rows, st = check(ctx, gs, pairs, 40, min_supports=(1, 4, 5))
    assert rows == want and st.records == 8 * n and st.sort_passes == 4              # 3 204 half-edges: two digits in each word
    ctx.close()


def test_staleness_and_call_order(tmp_path):
    N, header, recs, pairs, text = hand(None)
    ctx = random_store(N, 5)
    for call in (ctx.links, ctx.links_build):                                       # no graph
        with pytest.raises(s2.Sage2ovError) as e:
            call()
        assert e.value.code == -1
    load_text(ctx, text, tmp_path)
    g, _ = saved_graph(ctx, tmp_path, recs)
    rows, _ = check(ctx, g, {}, LH.HAND_K, min_supports=(1,))                        # links before any estimate and before any mates: it estimates itself; an empty table
    assert rows == [] and len(ctx.links()) == 0
    add_mates(ctx, {1: pairs[1]}); check(ctx, g, {1: pairs[1]}, LH.HAND_K)           # links before estimate, again: mates added, the estimate is stale
    add_mates(ctx, {2: pairs[2]}); check(ctx, g, {1: pairs[1], 2: pairs[2]}, LH.HAND_K)
    ctx.mates_clear(); assert len(ctx.links()) == 0 and ctx.link_stats().records == 0
    add_mates(ctx, pairs); rows, st = check(ctx, g, pairs, LH.HAND_K); assert len(rows) == LH.HAND_ROWS
    with pytest.raises(s2.Sage2ovError) as e:
        ctx.links(3)
    assert e.value.code == -1
    # a flow import does not make the table stale -- the filters read the flows at export
    built = (st.records_ms, st.sort_ms, st.reduce_ms)
    iH = next(i for i, (q, a, b) in enumerate(g["pairs"]) if {a["frm"], a["to"]} == {22, 23})
    fl = flat_flows(g); f2 = fl.copy(); f2[2 * iH] = f2[2 * iH + 1] = 0.0            # Hh's flow goes: (Hh, J), 200 / 61, passed FINAL by its second clause only
    ctx.graph_set_flows(f2)
    g["pairs"][iH][1]["flow"] = g["pairs"][iH][2]["flow"] = 0.0
    got = ctx.links(LH.FINAL)
    assert [tuple(int(v) for v in r) for r in got] == want_rows(g, LH.filtered(g, rows, LH.FINAL)) and len(got) < LH.HAND_FINAL
    assert len(ctx.links()) == LH.HAND_ROWS
    st = ctx.link_stats(); assert (st.records_ms, st.sort_ms, st.reduce_ms) == built and st.records == LH.HAND_RECORDS      # not rebuilt
    # another graph: the old table is gone
    N2, header2, recs2, pairs2, text2 = hand(666)
    load_text(ctx, text2, tmp_path, "v.graph4"); g2, _ = saved_graph(ctx, tmp_path, recs2, "v.saved")
    ctx.mates_clear(); add_mates(ctx, pairs2)
    check(ctx, g2, pairs2, LH.HAND_K)
    ctx.close()
