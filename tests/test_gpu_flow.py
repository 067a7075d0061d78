"""GPU: step 5's solver on the device (sage2ov_mcf_solve, sage2ov_flow_solve, sage2ov_flow_solution_*, sage2ov_copy_counts; kernels_flow.inc).
Every solved network is held against the certificate (bounds, conservation, 1-optimality in scaled units: tests/flow_model.py) and against its recorded optimum
(the table of DESIGN 5.20 for the goldens, tests/golden/flow/generated.json for the generated ones); networks of up to a few hundred nodes -- and the hubs, which
the model solves in a moment -- are held against the model exactly: flows, prices and counters.  The contract is optimal, not identical to the reference: P.graph5 is
compared byte for byte only on the goldens whose optimum is unique."""
import json, os, subprocess

import numpy as np
import pytest

import fixtures as fx
import flow_model as fm
import flowgen as fg
import sage2_amd as s2
from test_gpu_copycount import gold, golden_ctx, saved

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("minimiser_groups_on")]
OPTIMA = {"g1_clean100_k21": 40000060, "g6_k70_150": 39990900, "g7_palindrome_tandem_k21": 39996484, "g12_lowcomplexity_k21": 120400260,
          "g4_highcopy_k21": 2227089582, "g13_noisy300_k55": 19999938}
UNIQUE = ["g1_clean100_k21", "g6_k70_150", "g7_palindrome_tandem_k21"]
RECORDED = json.load(open(os.path.join(fx.GOLDEN, "flow", "generated.json")))
ERR_ARG, ERR_LIMIT = -1, -5


@pytest.fixture(scope="module")
def ctx():
    c = s2.Context(21)
    yield c
    c.close()


@pytest.fixture
def launches(monkeypatch, ctx):
    """the multi-launch form for networks that fit the single-workgroup one"""
    monkeypatch.setenv("SAGE2OV_TEST_MCF_LDS", "0"); ctx.options_reload()
    yield
    monkeypatch.delenv("SAGE2OV_TEST_MCF_LDS"); ctx.options_reload()


_models = {}


def model(name, n, arcs):
    if name not in _models: _models[name] = fm.solve(n, *fg.split(arcs))
    return _models[name]


def solve_and_check(ctx, n, arcs, optimum, exact=None):
    flow, price, st = ctx.mcf_solve(n, arcs)
    cost = fm.certificate(n, *fg.split(arcs), flow, price, st.scale)
    print(f"n {n} arcs {len(arcs)} form {st.form} phases {st.phases} rounds {st.rounds} pushes {st.pushes} relabels {st.relabels} updates {st.price_updates} cost {cost} "
          f"build {st.build_ms:.2f} ms solve {st.solve_ms:.2f} ms")
    assert cost == optimum == st.total_cost and (st.nodes, st.arcs, st.scale) == (n, len(arcs), n + 1)
    if exact is not None:
        assert exact.status == fm.OK
        assert np.array_equal(flow, exact.flow) and np.array_equal(price, exact.price)
        assert (st.phases, st.rounds, st.pushes, st.relabels, st.price_updates) == (exact.phases, exact.rounds, exact.pushes, exact.relabels, exact.updates)
    return flow, price, st


# ------------------------------------------------------------------------------------------ hand cases and generated networks
@pytest.mark.parametrize("name", list(fg.HAND))
def test_hand_cases(ctx, name):
    n, arcs = fg.hand(name)
    _, _, st = solve_and_check(ctx, n, arcs, RECORDED[name]["optimum"], model(name, n, arcs))
    assert st.form == s2.MCF_FORM_LDS


@pytest.mark.parametrize("name", list(fg.HAND))
def test_hand_cases_by_launches(ctx, launches, name):
    n, arcs = fg.hand(name)
    _, _, st = solve_and_check(ctx, n, arcs, RECORDED[name]["optimum"], model(name, n, arcs))
    assert st.form == s2.MCF_FORM_LAUNCHES


def test_negative_cycle_is_saturated_and_upper_zero_carries_nothing(ctx):
    n, arcs = fg.hand("negative_cycle"); flow, _, _ = ctx.mcf_solve(n, arcs)
    assert list(flow) == [4, 4, 4]
    n, arcs = fg.hand("upper_zero"); flow, price, _ = ctx.mcf_solve(n, arcs)
    assert list(flow[arcs["upper"] == 0]) == [0, 0, 0] and list(flow[arcs["upper"] > 0]) == [2, 2, 2]
    n, arcs = fg.hand("forced_dear"); flow, _, _ = ctx.mcf_solve(n, arcs)
    assert flow[1] == 2 and flow[0] == 1


# the hub's list has the degree of the name: a lane walks it up to 64 entries, the workgroup beyond, 256 entries at a time (one chunk up to 256, more beyond)
HUBS = [k for k in fg.GENERATED if k.startswith("hub_")]


@pytest.mark.parametrize("name", HUBS)
def test_hubs_on_both_sides_of_the_thresholds(ctx, launches, name):
    n, arcs = fg.generated(name)
    solve_and_check(ctx, n, arcs, RECORDED[name]["optimum"], model(name, n, arcs))


@pytest.mark.parametrize("name", [k for k in HUBS if "5000" not in k])
def test_hubs_in_one_workgroup(ctx, name):
    n, arcs = fg.generated(name)
    _, _, st = solve_and_check(ctx, n, arcs, RECORDED[name]["optimum"], model(name, n, arcs))
    assert st.form == s2.MCF_FORM_LDS


def test_a_network_that_just_fits_one_workgroup_and_the_same_by_launches(ctx, monkeypatch):
    n, arcs = fg.generated("ring_lds_fit")
    assert (n, 2 * len(arcs)) == (512, 2048)
    f1, p1, s1 = solve_and_check(ctx, n, arcs, RECORDED["ring_lds_fit"]["optimum"], model("ring_lds_fit", n, arcs))
    monkeypatch.setenv("SAGE2OV_TEST_MCF_LDS", "0"); ctx.options_reload()
    try:
        f2, p2, s2_ = solve_and_check(ctx, n, arcs, RECORDED["ring_lds_fit"]["optimum"])
    finally:
        monkeypatch.delenv("SAGE2OV_TEST_MCF_LDS"); ctx.options_reload()
    assert (s1.form, s2_.form) == (s2.MCF_FORM_LDS, s2.MCF_FORM_LAUNCHES)
    assert np.array_equal(f1, f2) and np.array_equal(p1, p2)
    assert (s1.phases, s1.rounds, s1.pushes, s1.relabels, s1.price_updates) == (s2_.phases, s2_.rounds, s2_.pushes, s2_.relabels, s2_.price_updates)
    # one node more, or one arc more, no longer fits
    n3, arcs3 = fg.ring(11, 513, 1024); assert ctx.mcf_solve(n3, arcs3)[2].form == s2.MCF_FORM_LAUNCHES
    n4, arcs4 = fg.ring(11, 512, 1025); assert ctx.mcf_solve(n4, arcs4)[2].form == s2.MCF_FORM_LAUNCHES


@pytest.mark.parametrize("name", ["shape_s1", "shape_s2", "ring_600"])
def test_generated_networks_against_the_model(ctx, name):
    n, arcs = fg.generated(name)
    solve_and_check(ctx, n, arcs, RECORDED[name]["optimum"], model(name, n, arcs))


def test_generated_network_of_1602_nodes(ctx):
    n, arcs = fg.generated("shape_s3")
    _, _, st = solve_and_check(ctx, n, arcs, RECORDED["shape_s3"]["optimum"])
    assert st.form == s2.MCF_FORM_LAUNCHES and n > 6 * 256


# ------------------------------------------------------------------------------------------ goldens
def golden_network(name):
    n, fr, to, lo, up, co = fm.parse_input_cs2(os.path.join(fx.GOLDEN, name + ".input.cs2.gz"))
    a = np.zeros(len(fr), fg.ARC); a["from"], a["to"], a["lower"], a["upper"], a["cost"] = fr, to, lo, up, co
    return n, a


@pytest.mark.parametrize("name", list(OPTIMA))
def test_golden_networks_twice(ctx, name):
    n, arcs = golden_network(name)
    small = name in ("g1_clean100_k21", "g6_k70_150", "g7_palindrome_tandem_k21", "g12_lowcomplexity_k21")      # up to a few hundred nodes: the model, exactly
    f1, p1, s1 = solve_and_check(ctx, n, arcs, OPTIMA[name], model(name, n, arcs) if small else None)
    f2, p2, s2_ = ctx.mcf_solve(n, arcs)
    assert np.array_equal(f1, f2) and np.array_equal(p1, p2) and (s1.rounds, s1.pushes, s1.relabels) == (s2_.rounds, s2_.pushes, s2_.relabels)
    if name in UNIQUE:
        ref = fm.parse_output_cs2(os.path.join(fx.GOLDEN, name + ".output.cs2.gz"))
        fr, to = arcs["from"], arcs["to"]
        assert fm.pair_totals(fr, to, f1, arcs["upper"] > 0) == fm.pair_totals(ref[:, 0], ref[:, 1], ref[:, 2])


# ------------------------------------------------------------------------------------------ errors
@pytest.mark.parametrize("name", list(fg.INFEASIBLE))
@pytest.mark.parametrize("form", ["lds", "launches"])
def test_infeasible_networks(ctx, monkeypatch, name, form):
    n, rows = fg.INFEASIBLE[name]
    if form == "launches": monkeypatch.setenv("SAGE2OV_TEST_MCF_LDS", "0")
    ctx.options_reload()
    try:
        with pytest.raises(s2.Sage2ovError) as e: ctx.mcf_solve(n, fg.arcs_of(rows))
    finally:
        monkeypatch.delenv("SAGE2OV_TEST_MCF_LDS", raising=False); ctx.options_reload()
    assert e.value.code == ERR_ARG and "infeasible" in str(e.value)


@pytest.mark.parametrize("name", list(fg.BAD))
def test_bad_arcs(ctx, name):
    n, rows = fg.BAD[name]
    with pytest.raises(s2.Sage2ovError) as e: ctx.mcf_solve(n, fg.arcs_of(rows))
    assert e.value.code == ERR_ARG and "bad arc" in str(e.value)


def test_overflow_guard(ctx):
    # (n + 1) * max |cost| fits 64 bits, the price range of the phases does not; and a cost whose scaled value alone does not
    for cost in (1 << 56, 1 << 61):
        with pytest.raises(s2.Sage2ovError) as e: ctx.mcf_solve(40, fg.arcs_of([(1, 2, 0, 1, cost), (2, 1, 0, 1, 0)]))
        assert e.value.code == ERR_LIMIT
    # the largest cost the guard of the model lets through is solved
    n, arcs = 3, fg.arcs_of([(1, 2, 1, 2, 1 << 52), (2, 3, 0, 2, -(1 << 52)), (3, 1, 0, 2, 5)])
    assert fm.solve(n, *fg.split(arcs)).status == fm.OK
    solve_and_check(ctx, n, arcs, 5, fm.solve(n, *fg.split(arcs)))


@pytest.mark.parametrize("form", ["lds", "launches"])
def test_round_budget(ctx, monkeypatch, form):
    n, arcs = fg.generated("shape_s1")
    if form == "launches": monkeypatch.setenv("SAGE2OV_TEST_MCF_LDS", "0")
    ctx.options_reload()
    try:
        with pytest.raises(s2.Sage2ovError) as e: ctx.mcf_solve(n, arcs, max_rounds=1)
        st = ctx.mcf_stats(); one = fm.solve(n, *fg.split(arcs), max_rounds=1)
        assert one.status == fm.LIMIT
        assert e.value.code == ERR_LIMIT and (st.rounds, st.nodes, st.arcs, st.pushes) == (1, n, len(arcs), one.pushes)
        # the budget the model needs, to the round, is enough; one less is not
        need = model("shape_s1", n, arcs).rounds
        assert ctx.mcf_solve(n, arcs, max_rounds=need)[2].rounds == need
        with pytest.raises(s2.Sage2ovError): ctx.mcf_solve(n, arcs, max_rounds=need - 1)
    finally:
        monkeypatch.delenv("SAGE2OV_TEST_MCF_LDS", raising=False); ctx.options_reload()


# ------------------------------------------------------------------------------------------ through the graph
def network_cost_and_certificate(ctx):
    arcs = ctx.flow_network(); flow, price, scale = ctx.flow_solution()
    cost = np.trunc(arcs["cost"].astype(np.float64)).astype(np.int64)                   # the %lld rule on the record's float
    nodes = ctx.copycount_stats().network_nodes
    return fm.certificate(nodes, arcs["from"].astype(np.int64), arcs["to"].astype(np.int64), arcs["lower"], arcs["upper"], cost, flow, price, scale)


@pytest.mark.parametrize("name", list(OPTIMA))
def test_goldens_through_the_loader_and_copy_counts(name, tmp_path):
    c = golden_ctx(name, tmp_path)
    with pytest.raises(s2.Sage2ovError) as e: c.flow_solve()                            # before the network is built
    assert e.value.code == ERR_ARG
    g = c.copy_counts()
    assert g == c.genome_size()
    assert network_cost_and_certificate(c) == OPTIMA[name] == c.mcf_stats().total_cost
    g5 = saved(c, tmp_path, c.graph5_save, "solved.graph5")
    sol = str(tmp_path / "ours.output.cs2"); c.flow_solution_save(sol)
    c2 = golden_ctx(name, tmp_path); c2.flow_load(sol)
    assert saved(c2, tmp_path, c2.graph5_save, "reloaded.graph5") == g5
    assert (c2.copycount_stats().t_to_s_flow, c2.copycount_stats().flow_different) == (c.copycount_stats().t_to_s_flow, c.copycount_stats().flow_different)
    if name in UNIQUE:
        c3 = golden_ctx(name, tmp_path); out = str(tmp_path / "ref.output.cs2"); open(out, "wb").write(gold(name, ".output.cs2.gz")); c3.flow_load(out)
        assert saved(c3, tmp_path, c3.graph5_save, "ref.graph5") == g5
        c3.close()
    c.close(); c2.close()


def test_round_budget_leaves_the_graph_and_the_solution_alone(tmp_path):
    c = golden_ctx("g6_k70_150", tmp_path)
    c.flow_network_build()
    before = saved(c, tmp_path, c.graph4_save, "before.graph4")
    with pytest.raises(s2.Sage2ovError) as e: c.flow_solve(max_rounds=1)
    assert e.value.code == ERR_LIMIT and c.mcf_stats().rounds == 1
    assert saved(c, tmp_path, c.graph4_save, "after.graph4") == before
    with pytest.raises(s2.Sage2ovError) as e: c.flow_commit()                           # nothing was solved: nothing to commit
    assert e.value.code == ERR_ARG
    c.flow_solve(); flow, price, _ = c.flow_solution()
    with pytest.raises(s2.Sage2ovError): c.flow_solve(max_rounds=1)
    f2, p2, _ = c.flow_solution()                                                       # the earlier solution stays
    assert np.array_equal(flow, f2) and np.array_equal(price, p2)
    assert saved(c, tmp_path, c.graph4_save, "after2.graph4") == before
    c.close()


def contig_file(c, tmp_path, fname):
    c.contigs_build(0, c.genome_size())
    return saved(c, tmp_path, lambda p: c.contigs_save(p), fname)


def test_steps_1_to_4_then_copy_counts_then_contigs(tmp_path):
    """no file in between; the contigs are those of a context that loaded P.graph4 and the reference's output.cs2 (g1's optimum is unique)"""
    name = "g1_clean100_k21"
    c = golden_ctx(name, tmp_path, steps=True)
    c.copy_counts()
    assert network_cost_and_certificate(c) == OPTIMA[name]
    assert saved(c, tmp_path, c.graph5_save, "t.graph5") == gold(name, ".graph5.gz")
    c3 = golden_ctx(name, tmp_path); out = str(tmp_path / "ref.output.cs2"); open(out, "wb").write(gold(name, ".output.cs2.gz")); c3.flow_load(out)
    got = contig_file(c, tmp_path, "a_contig.fasta")
    assert got == contig_file(c3, tmp_path, "b_contig.fasta") and got.count(b">") >= 1
    c.close(); c3.close()


def test_cli_flow_solve(tmp_path):
    name = "g1_clean100_k21"; m = fx.golden(name)
    fa = str(tmp_path / "reads.fa"); s2.synth_write_fasta(fx.synth_params(m["synth"]), fa)
    out = str(tmp_path / "out")
    exe = os.path.join(os.path.dirname(s2.__file__), "sage2ov")
    r = subprocess.run([exe, "-f", fa, "-k", str(m["k"]), "-M", "4", "--flowSolve", "-s", "--contigs", "-o", out, "-p", "P"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rd = lambda f: open(os.path.join(out, f), "rb").read()
    assert rd("P.graph5") == gold(name, ".graph5.gz")
    assert rd("input.cs2") == gold(name, ".input.cs2.gz")
    ours = np.array(rd("output.cs2").split(), np.int64).reshape(-1, 3)
    ref = fm.parse_output_cs2(os.path.join(fx.GOLDEN, name + ".output.cs2.gz"))
    assert fm.pair_totals(ours[:, 0], ours[:, 1], ours[:, 2]) == fm.pair_totals(ref[:, 0], ref[:, 1], ref[:, 2])
    assert list(ours[:, 0]) == sorted(ours[:, 0])                                      # our order: by tail
    c = golden_ctx(name, tmp_path, steps=True); c.copy_counts()
    assert rd("P_contig.fasta") == contig_file(c, tmp_path, "api_contig.fasta")
    c.close()
    assert "Min-cost flow:" in rd("P.log").decode() and "Step 5 (with its solver)" in rd("P.log").decode()
    r = subprocess.run([exe, "-f", fa, "-k", str(m["k"]), "-M", "4", "--flowSolve", "--flowSolution", "x", "-o", out, "-p", "Q"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "[ERROR] Options --flowSolve and --flowSolution are mutually exclusive!" in r.stdout and not os.path.exists(os.path.join(out, "Q.log"))
