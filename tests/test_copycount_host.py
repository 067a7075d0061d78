"""CPU: step 5 around its solver.  The Python restatement (tests/copycount_model.py) is pinned on files the reference binary wrote (tests/golden/*.input.cs2.gz,
*.output.cs2.gz, *.graph5.gz, step5/*.step5.json; made by tests/copycount_ref.py): the estimates of every round, input.cs2 byte for byte, and -- fed with the reference's
output.cs2 -- P.graph5.  The host half of the library (sage2ov_genome_size_rounds, the struct layouts, the refusals of a device-less context) is checked here too.

g3's output.cs2 is not committed (1 MB), so its P.graph5 cannot be rebuilt here: of g3 the estimates, the counters and input.cs2 (md5 and size) are checked.
g7 has a loop, which the reference holds as two edges and writes four times, while the model writes the records it loaded: g7's flows are compared record by
record with the reference's P.graph5 instead of byte for byte."""
import ctypes as C
import gzip, hashlib, json, os, subprocess

import numpy as np
import pytest

import copycount_model as M
import fixtures as fx
import sage2_amd as s2
import test_mate_estimate_host as H

INPUT_GOLDENS = ["g1_clean100_k21", "g6_k70_150", "g7_palindrome_tandem_k21", "g12_lowcomplexity_k21", "g4_highcopy_k21", "g13_noisy300_k55"]
TWO63 = 1 << 63
_cache = {}


def md5(b):
    return hashlib.md5(b).hexdigest()


def gold(name, suffix):
    return gzip.open(os.path.join(fx.GOLDEN, name + suffix)).read()


def golden_state(name):
    """(meta of step 5, graph as the reference loads it, frequencies, n, the model's estimate and network): computed once per golden and shared, never changed"""
    if name not in _cache:
        m = fx.golden(name); bases, off = fx.make_reads(m["synth"])
        ctx = s2.Context(m["k"], device=-2); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
        freq = ctx.reads_export()[2]; good = ctx.reads_stats().good_reads; ctx.close()
        g = H.parse_graph(gold(name, ".graph4.gz"), fold=False)
        assert g["header"][1] == good
        n = M.present_reads(g, freq)
        est = M.genome_size(g, freq, n)
        net = M.network(g, freq, n, est["genome_size"])
        _cache[name] = (json.load(open(os.path.join(fx.GOLDEN, "step5", name + ".step5.json"))), g, freq, n, est, net)
    return _cache[name]


@pytest.mark.parametrize("name", INPUT_GOLDENS + ["g3_noisy_rep_k21"])
def test_model_estimates_counters_and_input_cs2(name):
    meta, g, freq, n, est, net = golden_state(name)
    assert est["estimates"] == meta["estimates"] and est["agreed"] == meta["agreed"] and est["genome_size"] == meta["genome_size"]
    assert est["degenerate"] == (1 if meta["genome_size"] == TWO63 else 0)
    assert net["counters"] == {f: meta[f] for f in ("nodes", "edges", "simple", "once", "many")}
    text = M.cs2_text(net)
    assert text.split(b"\n", 1)[0].decode() == meta["p_min"]
    assert (len(text), md5(text)) == (meta["input_cs2_size"], meta["input_cs2_md5"])
    if name in INPUT_GOLDENS:
        assert text == gold(name, ".input.cs2.gz")


@pytest.mark.parametrize("name", ["g1_clean100_k21", "g6_k70_150", "g12_lowcomplexity_k21", "g4_highcopy_k21", "g13_noisy300_k55", "g7_palindrome_tandem_k21"])
def test_model_applies_the_reference_solution(name):
    meta, g0, freq, n, est, net = golden_state(name)
    g = H.parse_graph(gold(name, ".graph4.gz"), fold=False)                          # (apply changes the flows: a graph of its own)
    out = gold(name, ".output.cs2.gz")
    assert (len(out), md5(out)) == (meta["output_cs2_size"], meta["output_cs2_md5"])
    r = M.apply_solution(g, net["node_index"], M.parse_solution(out.decode()))
    assert (r["t_to_s_flow"], r["flow_different"]) == (meta["t_to_s_flow"], meta["flow_different"])
    if name == "g7_palindrome_tandem_k21":                                             # the loop: four records in the reference's file, flows 0; every other record as written
        want = H.parse_graph(gold(name, ".graph5.gz"), fold=False)
        key = lambda r: (r["frm"], r["to"], r["type"], r["len"], tuple(r["list"]))
        flows = {key(r): r["flow"] for _, a, b in want["pairs"] for r in (a, b)}
        for _, a, b in g["pairs"]:
            for r in (a, b):
                assert float(r["flow"]) == flows[key(r)] and (r["frm"] != r["to"] or float(r["flow"]) == 0.0)
        assert want["header"][:2] == (est["genome_size"], n)
        return
    text = M.graph5_text(g, est["genome_size"], n)
    assert (len(text), md5(text)) == (meta["graph5_size"], meta["graph5_md5"])
    if name != "g13_noisy300_k55":
        assert text == gold(name, ".graph5.gz")


def pair_inputs(g, freq):
    recs = [r for _, a, b in g["pairs"] for r in (a, b) if r["frm"] < r["to"]]
    return np.asarray([r["len"] for r in recs], dtype=np.uint32), np.asarray([M.k_of(r, freq) for r in recs], dtype=np.uint64)


@pytest.mark.parametrize("name", INPUT_GOLDENS + ["g3_noisy_rep_k21"])
def test_library_rounds_against_the_reference_log(name):
    meta, g, freq, n, est, net = golden_state(name)
    length, k = pair_inputs(g, freq)
    e = s2.genome_size_rounds(length, k, n)
    assert list(e.estimate[:e.rounds]) == meta["estimates"] and e.rounds == len(meta["estimates"])
    assert (e.genome_size, e.agreed, e.degenerate) == (meta["genome_size"], 1, 1 if meta["genome_size"] == TWO63 else 0)


def test_rounds_on_hand_inputs():
    # nothing qualifies: kSum = deltaSum = 0, the float is NaN -> 2^63, and the second round agrees with it
    e = s2.genome_size_rounds([400, 500], [10, 20], 1000)
    assert (e.rounds, e.genome_size, e.degenerate, e.agreed) == (2, TWO63, 1, 1) and list(e.estimate[:2]) == [TWO63, TWO63] and e.k_sum[0] == 0
    # a qualifying pair without reads: n / 0 * delta is an infinity -> 2^63 by the named rule
    e = s2.genome_size_rounds([501], [0], 1000)
    assert (e.genome_size, e.degenerate) == (TWO63, 1) and e.delta_sum[0] == 500
    # no pair at all
    e = s2.genome_size_rounds([], [], 5)
    assert (e.rounds, e.genome_size, e.degenerate, e.agreed) == (2, TWO63, 1, 1)
    # agreement at round 2: one long pair, a = delta * n / G - k log 2 is far above 3, the sums repeat
    e = s2.genome_size_rounds([20001], [4000], 8000)
    assert (e.rounds, e.agreed, e.degenerate, e.genome_size) == (2, 1, 0, 40000) and list(e.estimate[:2]) == [40000, 40000]
    # lengthOfEdge 500 / 501 in round 1; delta 999 / 1000 afterwards
    assert s2.genome_size_rounds([500], [7], 100).degenerate == 1 and s2.genome_size_rounds([501], [7], 100).estimate[0] == int(np.float32(100) / np.float32(7) * np.float32(500))
    e = s2.genome_size_rounds([1000, 1001], [10, 10], 10000)
    assert e.delta_sum[0] == 999 + 1000 and e.delta_sum[1] == 1000 and e.k_sum[1] == 10
    # the model runs the same rounds
    rng = np.random.default_rng(11)
    for _ in range(20):
        length = rng.integers(2, 6000, size=40).astype(np.uint32); k = rng.integers(0, 3000, size=40).astype(np.uint64); n = int(rng.integers(100, 200000))

        want = model_rounds(length, k, n); e = s2.genome_size_rounds(length, k, n)
        assert list(e.estimate[:e.rounds]) == want["estimates"] and (e.agreed, e.degenerate) == (int(want["agreed"]), want["degenerate"])


def model_rounds(length, k, n):
    def sums(prev):
        ds = ks = 0
        with np.errstate(all="ignore"):
            ratio = M.u2f(n) / M.u2f(prev) if prev else None
            for L, kk in zip(np.asarray(length).tolist(), np.asarray(k).tolist()):
                ok = (M.a_stat(L - 1, kk, ratio, M.logf(2)) >= 3 and L - 1 >= 1000) if prev else L > 500
                if ok:
                    ds += L - 1; ks += kk
        return ds, ks
    return M.rounds(sums, n)


def test_ten_rounds_without_agreement():
    """A pair qualifies while delta / k >= (log 2 + 3 / k) * deltaSum / kSum, so a round can only drop the pairs with the lowest delta / k, and the estimate
    then rises.  Thirty pairs with delta / k = r0 * 1.5^i and k = 2^(50 - i): the k-weighted mean of delta / k over the pairs from j on is about 2 * r0 * 1.5^j,
    inside (1.443, 2.164] * r0 * 1.5^j, so every round drops exactly the lowest pair left: ten different estimates, no final one."""
    length = np.array([int(4.0e9 * 0.75 ** i) + 1 for i in range(30)], dtype=np.uint32)
    k = np.array([2 ** (50 - i) for i in range(30)], dtype=np.uint64)
    n = 10 ** 12
    e = s2.genome_size_rounds(length, k, n)
    assert (e.rounds, e.agreed, e.degenerate) == (10, 0, 0) and e.genome_size == e.estimate[9]
    est = [int(v) for v in e.estimate]
    assert all(a < b for a, b in zip(est, est[1:]))
    assert [int(v) for v in e.delta_sum] == [int(length[j:].astype(np.uint64).sum()) - (30 - j) for j in range(10)]      # round j + 1 sums the pairs from j on
    want = model_rounds(length, k, n)
    assert want["estimates"] == est and not want["agreed"]


def test_struct_sizes_against_the_c_compiler(tmp_path):
    assert s2.FLOW_ARC_DTYPE.itemsize == 20
    src, exe = str(tmp_path / "sz.c"), str(tmp_path / "sz")
    fields = list(s2.FLOW_ARC_DTYPE.names)
    open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "sage2ov.h"\nint main(void) { printf("%zu", sizeof(sage2ov_flow_arc));\n'
                         + "".join('printf(" %%zu", offsetof(sage2ov_flow_arc, %s));\n' % f for f in fields)
                         + 'printf(" %zu %zu %d", sizeof(sage2ov_genome_estimate), sizeof(sage2ov_copycount_stats), SAGE2OV_GENOME_ROUNDS); return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(fx.ROOT, "include"), src, "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got == [20] + [s2.FLOW_ARC_DTYPE.fields[f][1] for f in fields] + [C.sizeof(s2.GenomeEstimate), C.sizeof(s2.CopyCountStats), s2.GENOME_ROUNDS]
    assert C.sizeof(s2.GenomeEstimate) == 8 + 3 * 80 + 16


def test_device_less_context_refuses(tmp_path):
    rng = np.random.default_rng(5)
    reads = sorted({"".join(rng.choice(list("ACGT"), size=60)) for _ in range(20)})
    bases = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(); off = np.arange(0, (len(reads) + 1) * 60, 60, dtype=np.uint64)
    ctx = s2.Context(40, device=-2); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
    one = np.ones(1, dtype=np.uint64)
    for call in (ctx.genome_size, ctx.flow_network_build, ctx.flow_network, lambda: ctx.flow_network_save(str(tmp_path / "input.cs2")), lambda: ctx.flow_apply(one, one, one),
                 lambda: ctx.flow_load(str(tmp_path / "none.cs2")), lambda: ctx.graph5_save(str(tmp_path / "t.graph5"))):
        with pytest.raises(s2.Sage2ovError) as e:
            call()
        assert e.value.code == -3
    assert not os.path.exists(tmp_path / "input.cs2") and not os.path.exists(tmp_path / "t.graph5")
    st = ctx.copycount_stats(); assert (st.genome_size, st.rounds, st.network_arcs) == (0, 0, 0)
    L = s2.lib()
    assert L.sage2ov_genome_size_estimate(None, None) == -1 and L.sage2ov_flow_network_build(None) == -1 and L.sage2ov_graph5_save(ctx._h, None) == -1
    assert L.sage2ov_genome_size_rounds(None, None, C.c_uint64(1), C.c_uint64(1), None) == -1
    ctx.close()
