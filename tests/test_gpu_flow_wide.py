"""GPU: step 5's solver with 128-bit prices (sage2ov_mcf_solve_wide, sage2ov_flow_solution_export_wide, the width sage2ov_flow_solve chooses; DESIGN.md 5.20;
kernels_flow.inc with P = __int128).  The lever: on a network the 64-bit path admits both widths give the same flows, prices and counters, number for number;
beyond it the device equals the model in Python integers (tests/flow_model_wide.py) and its certificate holds.

A record's cost and the statistics' total cost are int64, and neither 10^7 * 2^40 nor the optimum 4 * 10^7 * 2^38 is one: on the device the goldens' costs are
multiplied by 2^37, the largest power of two whose optimum the library can report; (n + 1) * 10^7 * 2^37 is beyond 2^62 for each of them, so the 64-bit path
refuses all three as it refuses 2^40 (tests/test_flow_wide_host.py has 2^40 on the model, which takes any integer)."""
import os

import numpy as np
import pytest

import fixtures as fx
import flow_model as fm
import flow_model_wide as fw
import flowgen as fg
import sage2_amd as s2
from test_gpu_copycount import gold, golden_ctx, saved

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("minimiser_groups_on")]
UNIQUE = {"g1_clean100_k21": 40000060, "g6_k70_150": 39990900, "g7_palindrome_tandem_k21": 39996484}
ERR_ARG, ERR_LIMIT = -1, -5
SHIFT = 37
COUNTERS = ("phases", "rounds", "pushes", "relabels", "price_updates")


@pytest.fixture(scope="module")
def ctx():
    c = s2.Context(21)
    yield c
    c.close()


def golden_network(name):
    n, fr, to, lo, up, co = fm.parse_input_cs2(os.path.join(fx.GOLDEN, name + ".input.cs2.gz"))
    a = np.zeros(len(fr), fg.ARC); a["from"], a["to"], a["lower"], a["upper"], a["cost"] = fr, to, lo, up, co
    return n, a


def named(name):
    if name in fg.GENERATED: return fg.generated(name)
    if name.startswith("two_arcs_"): return 40, fg.arcs_of([(1, 2, 0, 1, 1 << int(name[9:])), (2, 1, 0, 1, 0)])
    if name.endswith("*"):
        n, a = golden_network(name[:-1]); a = a.copy(); a["cost"] <<= SHIFT; return n, a
    return golden_network(name)


# ------------------------------------------------------------------------------------------ both widths on what 64 bits admit
BOTH = ["g1_clean100_k21", "g7_palindrome_tandem_k21", "g6_k70_150", "g13_noisy300_k55", "shape_s3", "ring_600"] + [k for k in fg.GENERATED if k.startswith("hub_")]


@pytest.mark.parametrize("name", BOTH)
def test_both_widths_give_the_same_numbers(ctx, name):
    n, arcs = named(name)
    f1, p1, s1 = ctx.mcf_solve(n, arcs)
    f2, p2, s2_ = ctx.mcf_solve(n, arcs, wide=True)
    print(name, "narrow form", s1.form, "rounds", s1.rounds, "solve ms", round(s1.solve_ms, 2), "| wide rounds", s2_.rounds, "solve ms", round(s2_.solve_ms, 2))
    assert (s1.price_words, s2_.price_words, s2_.form) == (1, 2, s2.MCF_FORM_LAUNCHES)
    if name in ("g1_clean100_k21", "g7_palindrome_tandem_k21"): assert s1.form == s2.MCF_FORM_LDS
    assert np.array_equal(f1, f2) and p1.tolist() == p2
    assert [getattr(s1, c) for c in COUNTERS] == [getattr(s2_, c) for c in COUNTERS] and s1.total_cost == s2_.total_cost
    assert ctx.mcf_stats().price_words == 2


# ------------------------------------------------------------------------------------------ beyond 64 bits
BEYOND = [g + "*" for g in UNIQUE] + ["two_arcs_56", "two_arcs_61"]


@pytest.mark.parametrize("name", BEYOND)
def test_beyond_64_bits_the_device_equals_the_model(ctx, name):
    n, arcs = named(name); net = fg.split(arcs)
    with pytest.raises(s2.Sage2ovError) as e: ctx.mcf_solve(n, arcs)                    # 64-bit prices: refused as before
    assert e.value.code == ERR_LIMIT and fm.solve(n, *net).status == fm.OVERFLOW
    flow, price, st = ctx.mcf_solve(n, arcs, wide=True)
    r = fw.solve(n, *net)
    assert r.status == fm.OK and (st.price_words, st.form, st.scale) == (2, s2.MCF_FORM_LAUNCHES, n + 1)
    assert flow.tolist() == r.flow.tolist() and price == r.price
    assert [getattr(st, c) for c in COUNTERS] == [r.phases, r.rounds, r.pushes, r.relabels, r.updates]
    cost = fw.certificate(n, *net, flow, price, st.scale)
    if name.endswith("*"):
        base = name[:-1]
        assert cost == UNIQUE[base] << SHIFT and max(abs(x) for x in price) >= 1 << 62
        # a unique optimum (the totals per (from, to); parallel arcs of one cost may share them differently): the flows of the unscaled network
        assert fm.pair_totals(net[0], net[1], flow) == fm.pair_totals(net[0], net[1], ctx.mcf_solve(*golden_network(base))[0])
        assert ctx.mcf_stats().total_cost == UNIQUE[base]
    else: assert cost == 0 and flow.tolist() == [0, 0]
    f2, p2, _ = ctx.mcf_solve(n, arcs, wide=True)                                       # the same network twice: the same bits
    assert np.array_equal(flow, f2) and price == p2


def test_wide_guard_returns_before_any_allocation(ctx):
    arcs = fg.arcs_of([(1, 2, 0, 1, 1 << 62), (2, 1, 0, 1, 0)])
    with pytest.raises(s2.Sage2ovError) as e: ctx.mcf_solve(3_000_000_000, arcs, wide=True)      # (arrays of n words would be some 200 GB)
    assert e.value.code == ERR_LIMIT and "128 bits" in str(e.value)
    st = ctx.mcf_stats(); assert (st.nodes, st.rounds, st.price_words) == (3_000_000_000, 0, 2)


def test_wide_errors_and_round_budget(ctx):
    for n, rows in fg.INFEASIBLE.values():
        with pytest.raises(s2.Sage2ovError) as e: ctx.mcf_solve(n, fg.arcs_of(rows), wide=True)
        assert e.value.code == ERR_ARG and "infeasible" in str(e.value)
    for n, rows in fg.BAD.values():
        with pytest.raises(s2.Sage2ovError) as e: ctx.mcf_solve(n, fg.arcs_of(rows), wide=True)
        assert e.value.code == ERR_ARG and "bad arc" in str(e.value)
    n, arcs = fg.generated("shape_s1"); need = ctx.mcf_solve(n, arcs)[2].rounds
    with pytest.raises(s2.Sage2ovError) as e: ctx.mcf_solve(n, arcs, max_rounds=1, wide=True)
    st = ctx.mcf_stats()
    assert e.value.code == ERR_LIMIT and (st.rounds, st.pushes, st.price_words) == (1, fm.solve(n, *fg.split(arcs), max_rounds=1).pushes, 2)
    assert ctx.mcf_solve(n, arcs, max_rounds=need, wide=True)[2].rounds == need
    with pytest.raises(s2.Sage2ovError): ctx.mcf_solve(n, arcs, max_rounds=need - 1, wide=True)


# ------------------------------------------------------------------------------------------ the resident network
@pytest.fixture
def always_wide(monkeypatch):
    monkeypatch.setenv("SAGE2OV_TEST_MCF_WIDE", "1")
    return monkeypatch


@pytest.mark.parametrize("name", list(UNIQUE))
def test_resident_network_with_128_bit_prices(always_wide, name, tmp_path):
    c = golden_ctx(name, tmp_path)
    c.genome_size(); c.flow_network_build()
    st = c.flow_solve()
    assert (st.price_words, st.form, st.total_cost) == (2, s2.MCF_FORM_LAUNCHES, UNIQUE[name])
    with pytest.raises(s2.Sage2ovError) as e: c.flow_solution()                        # 64-bit price words of a 128-bit solution
    assert e.value.code == ERR_LIMIT
    flow, price, scale = c.flow_solution_wide()
    c.flow_commit()
    g5 = saved(c, tmp_path, c.graph5_save, "wide.graph5")
    if name != "g7_palindrome_tandem_k21": assert g5 == gold(name, ".graph5.gz")
    # g7 through the loader: one loop pair is folded (test_gpu_copycount.py), so the golden P.graph5 is what this loader writes from the reference's output.cs2
    c3 = golden_ctx(name, tmp_path); out = str(tmp_path / "ref.output.cs2"); open(out, "wb").write(gold(name, ".output.cs2.gz")); c3.flow_load(out)
    assert saved(c3, tmp_path, c3.graph5_save, "ref.graph5") == g5
    c3.close()
    always_wide.delenv("SAGE2OV_TEST_MCF_WIDE"); c.options_reload()
    st1 = c.flow_solve(); f1, p1, sc1 = c.flow_solution()
    assert st1.price_words == 1 and np.array_equal(flow, f1) and price == p1.tolist() and scale == sc1
    assert [getattr(st, x) for x in COUNTERS] == [getattr(st1, x) for x in COUNTERS]
    f2, p2, _ = c.flow_solution_wide()                                                  # 64-bit prices, sign-extended
    assert np.array_equal(f1, f2) and p2 == price
    c.close()


def test_copy_counts_with_128_bit_prices(always_wide, tmp_path):
    name = "g1_clean100_k21"
    c = golden_ctx(name, tmp_path); c.copy_counts()
    assert c.mcf_stats().price_words == 2 and saved(c, tmp_path, c.graph5_save, "cc.graph5") == gold(name, ".graph5.gz")
    c.close()


def test_wide_round_budget_leaves_the_graph_and_the_solution_alone(always_wide, tmp_path):
    c = golden_ctx("g6_k70_150", tmp_path)
    c.flow_network_build()
    before = saved(c, tmp_path, c.graph4_save, "before.graph4")
    with pytest.raises(s2.Sage2ovError) as e: c.flow_solve(max_rounds=1)
    assert e.value.code == ERR_LIMIT and (c.mcf_stats().rounds, c.mcf_stats().price_words) == (1, 2)
    assert saved(c, tmp_path, c.graph4_save, "after.graph4") == before
    with pytest.raises(s2.Sage2ovError) as e: c.flow_commit()                           # nothing was solved: nothing to commit
    assert e.value.code == ERR_ARG
    c.flow_solve(); flow, price, _ = c.flow_solution_wide()
    with pytest.raises(s2.Sage2ovError): c.flow_solve(max_rounds=1)
    f2, p2, _ = c.flow_solution_wide()                                                  # the earlier solution stays
    assert np.array_equal(flow, f2) and price == p2
    assert saved(c, tmp_path, c.graph4_save, "after2.graph4") == before
    c.close()


# ------------------------------------------------------------------------------------------ the width the library chooses
# 290 000 noisy reads (tests/diag/flow_solve_wide.py --reads 290000 --err-ppm 1000 makes the same) give a network of 162 722 nodes and 502 781 arcs: the smallest
# multiple of 10 000 reads that 64-bit prices refuse at round 0 (280 000 reads, 157 482 nodes, get past their first price update).  The guard before the layout
# still admits it -- that one ends near 211 000 nodes --, the guard before the first price update does not: the solve stops with the range flag at round 0, and
# the automatic choice starts again with 128-bit prices.  The whole 128-bit solve of such a network takes about a minute (350 000 reads, 44 297
# rounds, 65 s), so it is the diagnostic's, not the suite's; here the round budget ends it, and the statistics show the width that was chosen.
AUTO_READS, AUTO_NODES = 290_000, 162_722


def test_the_library_chooses_the_width(monkeypatch, tmp_path):
    n = AUTO_READS
    p = fx.synth_params(dict(seed=2, genome_len=3 * n, n_reads=n, read_len=150, err_ppm=1000))
    bases, off = s2.synth_reads_ascii(p, s2.synth_genome(p))
    monkeypatch.setenv("SAGE2OV_TEST_MCF_WIDE", "0")
    c = s2.Context(40); c.reads_add_ascii(bases, off); c.reads_organize(); c.run_steps23(); c.graph_simplify(); c.genome_size(); c.flow_network_build()
    nodes = c.copycount_stats().network_nodes
    print("reads", n, "network nodes", nodes, "arcs", c.copycount_stats().network_arcs)
    assert nodes == AUTO_NODES
    before = saved(c, tmp_path, c.graph4_save, "before.graph4")
    with pytest.raises(s2.Sage2ovError) as e: c.flow_solve()                            # never wide: today's refusal
    st = c.mcf_stats()
    assert e.value.code == ERR_LIMIT and (st.rounds, st.price_words, st.nodes) == (0, 1, nodes)
    monkeypatch.delenv("SAGE2OV_TEST_MCF_WIDE"); c.options_reload()
    with pytest.raises(s2.Sage2ovError) as e: c.flow_solve(max_rounds=96)               # 64 bits first, then 128 bits from the start: the statistics are the second solve's
    st = c.mcf_stats()
    assert e.value.code == ERR_LIMIT and "round budget" in str(e.value) and (st.rounds, st.price_words, st.form, st.price_updates) == (96, 2, s2.MCF_FORM_LAUNCHES, 2)
    with pytest.raises(s2.Sage2ovError) as e: c.flow_commit()                           # nothing was solved
    assert e.value.code == ERR_ARG and saved(c, tmp_path, c.graph4_save, "after.graph4") == before
    c.close()
