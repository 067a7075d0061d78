"""CPU: the min-cost-flow model in Python integers (tests/flow_model_wide.py; DESIGN.md 5.20, the 128-bit form) against the int64 model on every network both admit,
on networks whose prices leave 64 bits, its guard against +-2^126, and the C ABI of the wide calls as far as it goes without a GPU.  tests/test_gpu_flow_wide.py
holds the device's 128-bit kernels against this model."""
import ctypes as C
import os, subprocess

import numpy as np
import pytest

import fixtures as fx
import flow_model as fm
import flow_model_wide as fw
import flowgen as fg
import sage2_amd as s2

# the optima of the goldens whose optimal flows are unique
UNIQUE = {"g1_clean100_k21": 40000060, "g6_k70_150": 39990900, "g7_palindrome_tandem_k21": 39996484}
GOLDENS = list(UNIQUE) + ["g12_lowcomplexity_k21"]
HUBS = ["hub_%d_%s" % (d, k) for d in (63, 64, 65, 256, 257) for k in ("few", "all")]
BOTH = GOLDENS + list(fg.HAND) + ["shape_s1", "shape_s2", "shape_s3", "ring_lds_fit"] + HUBS
TWO_ARCS = {"two_arcs_2^56": 1 << 56, "two_arcs_2^61": 1 << 61}
BEYOND = [g + "*2^40" for g in UNIQUE] + list(TWO_ARCS)
_nets, _narrow = {}, {}


def network(name):
    """(n, from, to, lower, upper, cost as Python integers) of a golden, a hand case, a generated network, or one of the networks beyond 64 bits"""
    if name not in _nets:
        if name in TWO_ARCS: n, fr, to, lo, up, co = (40,) + fg.split(fg.arcs_of([(1, 2, 0, 1, 0), (2, 1, 0, 1, 0)])); co = [TWO_ARCS[name], 0]
        elif name.endswith("*2^40"): n, fr, to, lo, up, co = network(name[:-5]); co = [c << 40 for c in co]
        elif name in GOLDENS: n, fr, to, lo, up, co = fm.parse_input_cs2(os.path.join(fx.GOLDEN, name + ".input.cs2.gz"))
        else: n, arcs = fg.generated(name) if name in fg.GENERATED else fg.hand(name); fr, to, lo, up, co = fg.split(arcs)
        _nets[name] = (n, fr, to, lo, up, [int(c) for c in co])
    return _nets[name]


def narrow(name):
    if name not in _narrow: _narrow[name] = fm.solve(*network(name))
    return _narrow[name]


@pytest.mark.parametrize("name", BOTH)
def test_wide_model_equals_the_int64_model(name):
    net = network(name); a = narrow(name); b = fw.solve(*net)
    assert a.status == b.status == fm.OK
    assert a.flow.tolist() == b.flow.tolist() and [int(x) for x in a.price] == b.price
    assert (a.scale, a.phases, a.rounds, a.pushes, a.relabels, a.updates, a.total_cost) == (b.scale, b.phases, b.rounds, b.pushes, b.relabels, b.updates, b.total_cost)
    assert a.per_refine == b.per_refine
    assert fw.certificate(*net, b.flow, b.price, b.scale) == a.total_cost


def test_wide_model_gives_the_same_verdicts():
    for name, (n, rows) in fg.INFEASIBLE.items():
        net = fg.split(fg.arcs_of(rows)); assert fw.solve(n, *net).status == fm.solve(n, *net).status == fm.INFEASIBLE, name
    for name, (n, rows) in fg.BAD.items():
        net = fg.split(fg.arcs_of(rows)); assert fw.solve(n, *net).status == fm.solve(n, *net).status == fm.BAD_ARC, name
    net = network("shape_s1"); full = narrow("shape_s1")
    one = fw.solve(*net, max_rounds=1)
    assert (one.status, one.rounds, one.flow, one.pushes) == (fm.LIMIT, 1, None, fm.solve(*net, max_rounds=1).pushes)
    assert fw.solve(*net, max_rounds=full.rounds).status == fm.OK and fw.solve(*net, max_rounds=full.rounds - 1).status == fm.LIMIT


@pytest.mark.parametrize("name", BEYOND)
def test_beyond_64_bits(name):
    n, fr, to, lo, up, co = network(name)
    if name in TWO_ARCS:
        assert fm.solve(n, fr, to, lo, up, np.array(co, np.int64)).status == fm.OVERFLOW
        optimum, flows = 0, [0, 0]
    else:
        # 10^7 * 2^40 is beyond int64 itself; the int64 model's guard is held on the largest multiple it can be given at all
        assert not fm.price_floor(n, (n + 1) * max(abs(c) for c in co)) < fm.I64_GUARD
        assert fm.solve(n, fr, to, lo, up, np.array([c >> 1 for c in co], np.int64)).status == fm.OVERFLOW
        base = name[:-5]; optimum, flows = UNIQUE[base] << 40, narrow(base).flow.tolist()
    r = fw.solve(n, fr, to, lo, up, co)
    assert r.status == fm.OK and (name in TWO_ARCS or max(abs(x) for x in r.price) >= 1 << 62)
    assert fw.certificate(n, fr, to, lo, up, co, r.flow, r.price, r.scale) == optimum == r.total_cost
    assert r.flow.tolist() == flows


def test_the_certificate_in_python_integers_refuses_what_is_not_optimal():
    n, fr, to, lo, up, co = network("parallel_classes"); co = [c << 70 for c in co]
    r = fw.solve(n, fr, to, lo, up, co)
    assert fw.certificate(n, fr, to, lo, up, co, r.flow, r.price, r.scale) == 34 << 70
    worse = r.flow.copy(); worse[0] += 1; worse[1] -= 1
    with pytest.raises(AssertionError): fw.certificate(n, fr, to, lo, up, co, worse, r.price, r.scale)
    broken = r.flow.copy(); broken[3] -= 1
    with pytest.raises(AssertionError): fw.certificate(n, fr, to, lo, up, co, broken, r.price, r.scale)


# (nodes, largest |cost|): the issue's case; what the old sum would wrap on (the terms pass 2^128); the edge of the guard on either side
GUARD_CASES = [(3_000_000_000, 1 << 62), (0xFFFFFFEF, 1 << 63), (0xFFFFFFEF, (1 << 63) - 1), (3_000_000_000, 1 << 59), (3_000_000_000, 1 << 58), (5_545_026, 100_000_000),
               (40, 1 << 62), (40, 1 << 63), (1 << 28, 1 << 63), (1 << 31, 1 << 61), (1 << 30, 1 << 62), (1, 1 << 63), (1, 0)]


def test_wide_guard_of_the_model():
    assert not fw.guard(3_000_000_000, 1 << 62)
    assert fw.guard(5_545_026, 100_000_000) and not fm.price_floor(5_545_026, 5_545_027 * 10_000_000) < fm.I64_GUARD      # the 10 M-read network: 128 bits, not 64
    r = fw.solve(3_000_000_000, [1], [2], [0], [1], [1 << 62])
    assert r.status == fm.OVERFLOW and r.flow is None                                  # (before any array of n words)
    assert any(fw.guard(*c) for c in GUARD_CASES) and not all(fw.guard(*c) for c in GUARD_CASES)


@pytest.mark.parametrize("n,maxc", GUARD_CASES)
def test_wide_guard_of_the_library_does_not_wrap(n, maxc):
    """sage2ov_mcf_solve_wide holds its guard on the arcs given before it asks for the device: on a device-less context a refused network is SAGE2OV_ERR_LIMIT, an
    admitted one SAGE2OV_ERR_DEVICE.  The verdict is the model's, whose integers cannot wrap"""
    ctx = s2.Context(21, device=-2)
    arcs = fg.arcs_of([(1, 2, 0, 1, 0), (2, 1, 0, 1, 0)]) if n >= 2 else fg.arcs_of([])
    if len(arcs): arcs["cost"][0] = -maxc if maxc == 1 << 63 else maxc               # (|-2^63| is the largest a record can hold)
    with pytest.raises(s2.Sage2ovError) as e: ctx.mcf_solve(n, arcs, wide=True)
    assert e.value.code == (-3 if fw.guard(n, maxc if len(arcs) else 0) else -5)
    st = ctx.mcf_stats(); assert (st.nodes, st.price_words, st.rounds) == (n, 2, 0)
    ctx.close()


# ------------------------------------------------------------------------------------------ the C ABI, without a GPU
def test_symbols_struct_and_header(tmp_path):
    L = s2.lib()
    for sym in ("sage2ov_mcf_solve_wide", "sage2ov_flow_solution_export_wide"): assert hasattr(L, sym), sym
    proto, src, exe = str(tmp_path / "proto.c"), str(tmp_path / "w.c"), str(tmp_path / "w")
    # the header declares both calls with these types: an initialiser of another type does not compile
    open(proto, "w").write('#include "sage2ov.h"\n'
                           'int (*a)(sage2ov_ctx*, uint64_t, const sage2ov_mcf_arc*, uint64_t, uint64_t, int64_t*, uint64_t*, sage2ov_mcf_stats*) = sage2ov_mcf_solve_wide;\n'
                           'int (*b)(sage2ov_ctx*, int64_t*, uint64_t, uint64_t*, uint64_t, uint64_t*) = sage2ov_flow_solution_export_wide;\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(fx.ROOT, "include"), "-c", proto, "-o", str(tmp_path / "proto.o")], check=True)
    open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "sage2ov.h"\n'
                         'int main(void) { sage2ov_mcf_stats s; s.price_words = 2; printf("%zu %zu %zu %zu %u", sizeof s, offsetof(sage2ov_mcf_stats, form), offsetof(sage2ov_mcf_stats, price_words),'
                         ' offsetof(sage2ov_mcf_stats, build_ms), s.price_words); return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(fx.ROOT, "include"), src, "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    size = 8 * 8 + 8 + 8 + 16 + 2 * 8 * s2.MCF_PHASES                                   # as before the word had a name
    assert got == [size, 72, 76, 80, 2] and C.sizeof(s2.McfStats) == size
    assert (s2.McfStats.form.offset, s2.McfStats.price_words.offset, s2.McfStats.build_ms.offset) == (72, 76, 80) and not hasattr(s2.McfStats, "reserved")


def test_wide_prices_are_twos_complement_low_word_first():
    w = np.array([5, 0, (1 << 64) - 1, (1 << 64) - 1, 0, 1 << 63, 7, 1], np.uint64)
    assert s2.wide_prices(w) == [5, -1, -(1 << 127), (1 << 64) + 7]


def test_device_less_context_and_null_arguments():
    ctx = s2.Context(21, device=-2)
    n, arcs = fg.hand("one_path")
    for call in (lambda: ctx.mcf_solve(n, arcs, wide=True), ctx.flow_solution_wide):
        with pytest.raises(s2.Sage2ovError) as e: call()
        assert e.value.code == -3
    L = s2.lib(); z = C.c_uint64(0)
    assert L.sage2ov_mcf_solve_wide(None, z, None, z, z, None, None, None) == -1 and L.sage2ov_flow_solution_export_wide(None, None, z, None, z, None) == -1
    assert L.sage2ov_mcf_solve_wide(ctx._h, C.c_uint64(4), None, C.c_uint64(3), z, None, None, None) == -1      # arcs promised, none given
    ctx.close()
