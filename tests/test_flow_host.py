"""CPU: the numpy restatement of the device min-cost-flow solver (tests/flow_model.py) on the six golden networks and on generated ones, the
certificate, scipy's LP where scipy is present, the recorded optima (tests/golden/flow/generated.json, tools/make_golden_flow.py) and the C ABI of the solver as far as it
goes without a GPU.  tests/test_gpu_flow.py holds the device against this model."""
import ctypes as C
import json, os, subprocess

import numpy as np
import pytest

import fixtures as fx
import flow_model as fm
import flowgen as fg
import sage2_amd as s2

# nodes, arcs, optimum with the costs as %lld reads them
TABLE = {"g1_clean100_k21": (10, 15, 40000060), "g6_k70_150": (362, 1249, 39990900), "g7_palindrome_tandem_k21": (18, 59, 39996484),
         "g12_lowcomplexity_k21": (42, 79, 120400260), "g4_highcopy_k21": (5198, 19755, 2227089582), "g13_noisy300_k55": (18914, 57463, 19999938)}
UNIQUE = ["g1_clean100_k21", "g6_k70_150", "g7_palindrome_tandem_k21"]
RECORDED = json.load(open(os.path.join(fx.GOLDEN, "flow", "generated.json")))
_cache = {}


def golden(name):
    if name not in _cache:
        net = fm.parse_input_cs2(os.path.join(fx.GOLDEN, name + ".input.cs2.gz"))
        _cache[name] = (net, fm.solve(*net))
    return _cache[name]


def test_the_cost_is_the_integer_prefix_of_the_text():
    assert [fm.trunc_cost(t) for t in ("-691.348000", "-0.700000", "0.999999", "100000000.000000", "10.000000", "-1.000000", "+7.9")] == [-691, 0, 0, 100000000, 10, -1, 7]
    # the goldens have such texts: negative costs between -1 and 0 become 0
    import gzip
    txt = gzip.open(os.path.join(fx.GOLDEN, "g6_k70_150.input.cs2.gz"), "rt").read().split("\n")
    costs = [l.split()[5] for l in txt if l.startswith("a ")]
    assert any(c.startswith("-0.") for c in costs) and any(c.startswith("-") and not c.startswith("-0.") for c in costs)


@pytest.mark.parametrize("name", list(TABLE))
def test_model_reaches_the_optimum_of_the_golden_networks(name):
    (n, fr, to, lo, up, co), r = golden(name)
    assert (n, len(fr)) == TABLE[name][:2] and r.status == fm.OK and r.scale == n + 1
    assert fm.certificate(n, fr, to, lo, up, co, r.flow, r.price, r.scale) == TABLE[name][2] == r.total_cost
    assert r.phases == len(fm.eps_sequence(max(1, (n + 1) * int(np.abs(co).max())))) and r.per_refine[-1][0] == 1 and r.updates >= r.phases
    if name in UNIQUE:                                                                 # the optimum is unique there: the reference's totals per (from, to)
        ref = fm.parse_output_cs2(os.path.join(fx.GOLDEN, name + ".output.cs2.gz"))
        assert fm.pair_totals(fr, to, r.flow, up > 0) == fm.pair_totals(ref[:, 0], ref[:, 1], ref[:, 2])


@pytest.mark.parametrize("name", ["g1_clean100_k21", "g6_k70_150", "g7_palindrome_tandem_k21", "g12_lowcomplexity_k21"])
def test_model_without_price_updates_reaches_the_same_optimum(name):
    (n, fr, to, lo, up, co), _ = golden(name)
    r = fm.solve(n, fr, to, lo, up, co, period=0)
    assert r.status == fm.OK and r.updates == 0 and fm.certificate(n, fr, to, lo, up, co, r.flow, r.price, r.scale) == TABLE[name][2]


def test_the_certificate_refuses_what_is_not_optimal():
    n, arcs = fg.hand("parallel_classes"); net = fg.split(arcs); r = fm.solve(n, *net)
    assert fm.certificate(n, *net, r.flow, r.price, r.scale) == 34
    worse = r.flow.copy(); worse[0] += 1; worse[1] -= 1                               # still feasible and conserved, one unit on a dearer arc
    with pytest.raises(AssertionError): fm.certificate(n, *net, worse, r.price, r.scale)
    broken = r.flow.copy(); broken[3] -= 1
    with pytest.raises(AssertionError): fm.certificate(n, *net, broken, r.price, r.scale)
    over = r.flow.copy(); over[1] += 1; over[3] += 1
    with pytest.raises(AssertionError): fm.certificate(n, *net, over, r.price, r.scale)


@pytest.mark.parametrize("name", list(fg.GENERATED) + list(fg.HAND))
def test_model_on_generated_networks_against_the_recorded_optima(name):
    n, arcs = fg.generated(name) if name in fg.GENERATED else fg.hand(name)
    assert (RECORDED[name]["nodes"], RECORDED[name]["arcs"]) == (n, len(arcs))
    net = fg.split(arcs); r = fm.solve(n, *net)
    assert r.status == fm.OK and fm.certificate(n, *net, r.flow, r.price, r.scale) == RECORDED[name]["optimum"]
    again = fm.solve(n, *net)
    assert np.array_equal(r.flow, again.flow) and np.array_equal(r.price, again.price) and r.rounds == again.rounds


def test_hub_lists_have_the_degree_of_their_name():
    for d in (63, 64, 65, 256, 257, 5000):
        n, arcs = fg.hub(d, 5)
        deg = np.bincount(np.concatenate([arcs["from"], arcs["to"]]).astype(np.int64), minlength=n + 1)
        assert deg[1] == d and deg[2] == d and deg[3:].max() == 2


def test_model_refuses(monkeypatch):
    for name, (n, rows) in fg.INFEASIBLE.items(): assert fm.solve(n, *fg.split(fg.arcs_of(rows))).status == fm.INFEASIBLE, name
    for name, (n, rows) in fg.BAD.items(): assert fm.solve(n, *fg.split(fg.arcs_of(rows))).status == fm.BAD_ARC, name
    for cost in (1 << 56, 1 << 61): assert fm.solve(40, *fg.split(fg.arcs_of([(1, 2, 0, 1, cost), (2, 1, 0, 1, 0)]))).status == fm.OVERFLOW
    n, arcs = fg.generated("shape_s1"); net = fg.split(arcs); full = fm.solve(n, *net)
    one = fm.solve(n, *net, max_rounds=1)
    assert (one.status, one.rounds, one.flow) == (fm.LIMIT, 1, None)
    assert fm.solve(n, *net, max_rounds=full.rounds).status == fm.OK and fm.solve(n, *net, max_rounds=full.rounds - 1).status == fm.LIMIT


def lp_optimum(n, fr, to, lo, up, co):
    from scipy.optimize import linprog
    from scipy.sparse import coo_matrix
    m = len(fr)
    A = coo_matrix((np.concatenate([np.ones(m), -np.ones(m)]), (np.concatenate([to - 1, fr - 1]), np.concatenate([np.arange(m), np.arange(m)]))), shape=(n, m))
    r = linprog(co.astype(float), A_eq=A.tocsr(), b_eq=np.zeros(n), bounds=list(zip(lo.tolist(), up.tolist())), method="highs")
    assert r.status == 0
    return r.fun


@pytest.mark.parametrize("name", list(TABLE) + ["shape_s1", "shape_s2", "shape_s3", "ring_600", "hub_257_few"])
def test_model_against_scipy(name):
    pytest.importorskip("scipy")
    if name in TABLE: net, r = golden(name)
    else:
        n, arcs = fg.generated(name); net = (n,) + fg.split(arcs); r = fm.solve(*net)
    assert abs(lp_optimum(*net) - r.total_cost) <= 1e-6 * max(1, abs(r.total_cost))


# ------------------------------------------------------------------------------------------ the C ABI, without a GPU
def test_symbols_and_struct_sizes(tmp_path):
    L = s2.lib()
    for sym in ("sage2ov_mcf_solve", "sage2ov_flow_solve", "sage2ov_flow_solution_export", "sage2ov_flow_solution_save", "sage2ov_flow_solution_commit", "sage2ov_copy_counts",
                "sage2ov_mcf_stats_get"):
        assert hasattr(L, sym), sym
    assert s2.MCF_ARC_DTYPE.itemsize == 24 and fg.ARC == s2.MCF_ARC_DTYPE
    src, exe = str(tmp_path / "sz.c"), str(tmp_path / "sz")
    fields = list(s2.MCF_ARC_DTYPE.names)
    open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "sage2ov.h"\nint main(void) { printf("%zu", sizeof(sage2ov_mcf_arc));\n'
                         + "".join('printf(" %%zu", offsetof(sage2ov_mcf_arc, %s));\n' % f for f in fields)
                         + 'printf(" %zu %zu %zu %d %d %d %llu", sizeof(sage2ov_mcf_stats), offsetof(sage2ov_mcf_stats, total_cost), offsetof(sage2ov_mcf_stats, refine_ms), SAGE2OV_MCF_PHASES,'
                           ' SAGE2OV_MCF_FORM_LDS, SAGE2OV_MCF_FORM_LAUNCHES, (unsigned long long)SAGE2OV_MCF_DEFAULT_ROUNDS); return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(fx.ROOT, "include"), src, "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got == [24] + [s2.MCF_ARC_DTYPE.fields[f][1] for f in fields] + [C.sizeof(s2.McfStats), s2.McfStats.total_cost.offset, s2.McfStats.refine_ms.offset, s2.MCF_PHASES,
                                                                            s2.MCF_FORM_LDS, s2.MCF_FORM_LAUNCHES, fm.DEFAULT_MAX_ROUNDS]
    assert C.sizeof(s2.McfStats) == 8 * 8 + 8 + 8 + 16 + 2 * 8 * s2.MCF_PHASES


def test_device_less_context_and_null_arguments(tmp_path):
    ctx = s2.Context(21, device=-2)
    n, arcs = fg.hand("one_path")
    for call in (lambda: ctx.mcf_solve(n, arcs), ctx.flow_solve, ctx.flow_solution, ctx.flow_commit, ctx.copy_counts, lambda: ctx.flow_solution_save(str(tmp_path / "o.cs2"))):
        with pytest.raises(s2.Sage2ovError) as e: call()
        assert e.value.code == -3
    assert not os.path.exists(tmp_path / "o.cs2")
    st = ctx.mcf_stats(); assert (st.nodes, st.rounds, st.form) == (0, 0, 0)
    L = s2.lib(); z = C.c_uint64(0)
    assert L.sage2ov_mcf_solve(None, z, None, z, z, None, None, None) == -1 and L.sage2ov_flow_solve(None, z, None) == -1 and L.sage2ov_copy_counts(None, None) == -1
    assert L.sage2ov_flow_solution_commit(None) == -1 and L.sage2ov_flow_solution_save(ctx._h, None) == -1 and L.sage2ov_mcf_stats_get(ctx._h, None) == -1
    assert L.sage2ov_flow_solution_export(None, None, z, None, z, None) == -1
    assert L.sage2ov_mcf_solve(ctx._h, C.c_uint64(4), None, C.c_uint64(3), z, None, None, None) == -1          # arcs promised, none given
    ctx.close()
