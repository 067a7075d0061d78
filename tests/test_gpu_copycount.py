"""GPU: step 5 around its solver on the device (sage2ov_genome_size_estimate, sage2ov_flow_network_*, sage2ov_flow_solution_*, sage2ov_graph5_save)
against files the reference wrote (tests/golden/*.input.cs2.gz, *.output.cs2.gz, *.graph5.gz, step5/*.step5.json) and against the restatement tests/copycount_model.py
(pinned on those files by tests/test_copycount_host.py) over the text sage2ov_graph4_save wrote.  Every comparison is exact: bytes, integers, float bit patterns."""
import gzip, hashlib, json, os

import numpy as np
import pytest

import compgen
import copycount_model as M
import fixtures as fx
import sage2_amd as s2
import test_mate_estimate_host as H
import test_mate_support_host as MS
from test_gpu_mate_estimate import add_mates, load_text
from test_gpu_mate_support import check as check_supports

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("minimiser_groups_on")]
TWO63 = 1 << 63
LOADER_GOLDENS = ["g1_clean100_k21", "g6_k70_150", "g7_palindrome_tandem_k21", "g12_lowcomplexity_k21", "g4_highcopy_k21", "g13_noisy300_k55"]


def gold(name, suffix):
    return gzip.open(os.path.join(fx.GOLDEN, name + suffix)).read()


def meta5(name):
    return json.load(open(os.path.join(fx.GOLDEN, "step5", name + ".step5.json")))


def golden_ctx(name, tmp_path, steps=False):
    """organised reads and the committed P.graph4 through the loader -- or, steps, steps 1-4 on the device with no file in between"""
    m = fx.golden(name); bases, off = fx.make_reads(m["synth"])
    ctx = s2.Context(m["k"]); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
    if steps:
        ctx.run_steps23(); ctx.graph_simplify()
    else:
        src = str(tmp_path / "in.graph4"); open(src, "wb").write(gold(name, ".graph4.gz")); ctx.graph_load_composite(src)
    return ctx


def saved(ctx, tmp_path, call, name):
    p = str(tmp_path / name); call(p)
    return open(p, "rb").read()


def check_counters(st, meta):
    assert (st.nodes, st.edges, st.simple, st.once, st.many) == tuple(meta[f] for f in ("nodes", "edges", "simple", "once", "many"))
    nn, na = (int(x) for x in meta["p_min"].split()[2:])
    assert (st.network_nodes, st.network_arcs) == (nn, na)


# ------------------------------------------------------------------------------------------ (a) goldens through the loader
@pytest.mark.parametrize("name", LOADER_GOLDENS)
def test_goldens_through_the_loader(name, tmp_path):
    meta = meta5(name); ctx = golden_ctx(name, tmp_path)
    before = saved(ctx, tmp_path, ctx.graph4_save, "before.graph4")
    assert ctx.genome_size() == meta["genome_size"]
    st = ctx.copycount_stats()
    assert list(st.estimate[:st.rounds]) == meta["estimates"] and (st.agreed, st.degenerate) == (1, 1 if meta["genome_size"] == TWO63 else 0)
    assert saved(ctx, tmp_path, ctx.flow_network_save, "input.cs2") == gold(name, ".input.cs2.gz")
    check_counters(ctx.copycount_stats(), meta)
    arcs = ctx.flow_network()
    assert len(arcs) == ctx.copycount_stats().network_arcs and tuple(arcs[0])[:3] == (2, 1, 1)
    out = str(tmp_path / "output.cs2"); open(out, "wb").write(gold(name, ".output.cs2.gz")); ctx.flow_load(out)
    st = ctx.copycount_stats()
    assert (st.t_to_s_flow, st.flow_different) == (meta["t_to_s_flow"], meta["flow_different"])
    g5 = saved(ctx, tmp_path, ctx.graph5_save, "t.graph5")
    if name == "g7_palindrome_tandem_k21":
        # the loader folds the loop the file holds twice into one pair, the reference writes it four times: the flows of every other pair, and 0 on the loop
        want = H.parse_graph(gold(name, ".graph5.gz"), fold=False); got = H.parse_graph(g5, fold=False)
        key = lambda r: (r["frm"], r["to"], r["type"], r["len"], tuple(r["list"]))
        flows = {key(r): r["flow"] for _, a, b in want["pairs"] for r in (a, b)}
        loops = 0
        for _, a, b in got["pairs"]:
            for r in (a, b):
                assert r["flow"] == flows[key(r)]
                if r["frm"] == r["to"]:
                    loops += 1; assert r["flow"] == 0.0
        assert loops == 4 and got["header"] == want["header"]
    else:
        assert (len(g5), hashlib.md5(g5).hexdigest()) == (meta["graph5_size"], meta["graph5_md5"])
        if name != "g13_noisy300_k55":
            assert g5 == gold(name, ".graph5.gz")
    # nothing else moves
    assert saved(ctx, tmp_path, ctx.graph4_save, "after.graph4") == before
    ctx.close()


# ------------------------------------------------------------------------------------------ (b) steps 1-4 on the device, no file in between
@pytest.mark.parametrize("name", ["g6_k70_150", "g4_highcopy_k21"])
def test_after_steps_1_to_4_on_the_device(name, tmp_path):
    meta = meta5(name); ctx = golden_ctx(name, tmp_path, steps=True)
    assert saved(ctx, tmp_path, ctx.flow_network_save, "input.cs2") == gold(name, ".input.cs2.gz")      # (build without an estimate: it estimates first)
    st = ctx.copycount_stats()
    assert st.genome_size == meta["genome_size"] and list(st.estimate[:st.rounds]) == meta["estimates"]
    check_counters(st, meta)
    out = str(tmp_path / "output.cs2"); open(out, "wb").write(gold(name, ".output.cs2.gz")); ctx.flow_load(out)
    assert saved(ctx, tmp_path, ctx.graph5_save, "t.graph5") == gold(name, ".graph5.gz")
    ctx.close()


# ------------------------------------------------------------------------------------------ (c) built graphs against the model
def store_with_frequencies(n, seed, freq, L=60, k=40):
    """n unique reads, read i written freq[i] times (which id gets which frequency is the organiser's business: the tests read the frequencies back)"""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n + n // 8, L))]
    reads = sorted({r.tobytes() for r in a})[:n]
    assert len(reads) == n
    flat = np.frombuffer(b"".join(r * int(f) for r, f in zip(reads, freq)), dtype=np.uint8).copy()
    off = np.arange(0, len(flat) + 1, L, dtype=np.uint64)
    ctx = s2.Context(k); ctx.reads_add_ascii(flat, off); ctx.reads_organize()
    assert ctx.reads_stats().unique_reads == n
    return ctx


def entries(rng, ids):
    """a read list over these ids: distances 1 .. 3, distNext of an entry = distPrevious of the next"""
    d = rng.integers(1, 4, size=len(ids) + 1).tolist()
    return [(int(r), int(rng.integers(0, 2)), 0, d[j], d[j + 1]) for j, r in enumerate(ids)]


def graph_text(N, specs, seed):
    """specs: (from, to, type, lengthOfEdge, list length) -> the text of a P.graph4 with these record pairs (record, twin), reads drawn from 1 .. N"""
    rng = np.random.default_rng(seed); recs = []
    for frm, to, typ, length, n in specs:
        a = H.rec(frm, to, typ, length, entries(rng, rng.integers(1, N + 1, size=n)))
        recs += [a, dict(H.twin_of(a), len=length)]
    return H.graph_text((0, N, 60), recs)


def model_of(ctx, tmp_path):
    """the model over what the library would write: (graph, freq, n, estimate, network, the saved text)"""
    text = saved(ctx, tmp_path, ctx.graph4_save, "model.graph4")
    g = H.parse_graph(text, fold=False); freq = ctx.reads_export()[2]
    n = M.present_reads(g, freq); est = M.genome_size(g, freq, n)
    return g, freq, n, est, M.network(g, freq, n, est["genome_size"]), text


def check_against_model(ctx, tmp_path):
    g, freq, n, est, net, text = model_of(ctx, tmp_path)
    assert ctx.genome_size() == est["genome_size"]
    st = ctx.copycount_stats()
    assert list(st.estimate[:st.rounds]) == est["estimates"] and (st.agreed, st.degenerate, st.reads_present) == (int(est["agreed"]), est["degenerate"], n)
    arcs = ctx.flow_network(); want = net["arcs"]
    assert len(arcs) == len(want)
    w = np.zeros(len(want), dtype=s2.FLOW_ARC_DTYPE)
    for f, col in zip(("from", "to", "lower", "upper", "cost"), zip(*want)):
        w[f] = np.asarray(col, dtype=s2.FLOW_ARC_DTYPE.fields[f][0])
    for f in ("from", "to", "lower", "upper"):
        assert np.array_equal(arcs[f], w[f]), f
    assert np.array_equal(arcs["cost"].view(np.uint32), w["cost"].view(np.uint32))      # the costs as float bit patterns
    assert saved(ctx, tmp_path, ctx.flow_network_save, "input.cs2") == M.cs2_text(net)
    st = ctx.copycount_stats(); c = net["counters"]
    assert (st.nodes, st.edges, st.simple, st.once, st.many, st.network_nodes, st.network_arcs) == (c["nodes"], c["edges"], c["simple"], c["once"], c["many"], net["network_nodes"], len(want))
    assert saved(ctx, tmp_path, ctx.graph4_save, "after.graph4") == text
    return g, freq, n, est, net


SHAPE_LISTS = [1, 35, 36, 63, 64, 65, 255, 256, 257, 5000]


def shapes_graph(N):
    """list lengths on the `> 35` rule and on the wave and block edges of the segmented sum and of the cost fold, lengthOfEdge 500 / 501, delta 999 / 1000 / 1001,
    three parallel pairs of different types, a loop, a node without edges between nodes with edges (5), a hub (40) whose 3000 records cross a sort tile"""
    specs = []
    nodes = iter(range(100, 100 + 4 * len(SHAPE_LISTS) * 5, 2))                      # (even ids: the odd ones between them have no edge)
    for n in SHAPE_LISTS:
        for length in (500, 501, 1000, 1001, 1002):
            a, b = next(nodes), next(nodes)
            specs.append((a, b, int(n + length) % 4, length, n) if (n + length) % 3 else (b, a, int(n + length) % 4, length, n))
    specs += [(4, 6, 3, 1500, 40), (4, 6, 0, 700, 0), (6, 4, 2, 900, 36)]             # parallel pairs; 5 has no edge
    specs += [(7, 7, 3, 1200, 50)]                                                   # a loop
    specs += [(40, 1000 + i, i % 4, 30 + i % 50, 0) if i % 2 else (1000 + i, 40, i % 4, 30 + i % 50, 0) for i in range(1500)]      # the hub, simple edges
    return specs


def test_built_graph_shapes_and_random_frequencies(tmp_path):
    N = 2600
    rng = np.random.default_rng(77)
    freq = rng.integers(1, 40, size=N); freq[rng.integers(0, N, size=200)] = 1; freq[17] = 65535; freq[1900] = 65535
    ctx = store_with_frequencies(N, 21, freq)
    load_text(ctx, graph_text(N, shapes_graph(N), 5), tmp_path)
    g, f, n, est, net = check_against_model(ctx, tmp_path)
    assert set(np.unique(f[1:]).tolist()) >= {1, 65535} and len(np.unique(f)) > 20
    assert net["counters"]["many"] >= 30 and net["counters"]["simple"] >= 1500 and net["counters"]["edges"] == len(shapes_graph(N)) + 3      # (the loop counts four times)
    lbs = {r[2] for r in net["arcs"] if r[3] == 3}
    assert lbs >= {0, 1}                                                             # the `> 35` rule on both sides
    ctx.close()


def thresholds_graph():
    """every frequency 1, so k = the list length.  U (delta 2 000 000, k 200 000) outweighs everything else in the sums, so X = delta * n / G stays within 1 % of
    0.1 * delta whichever of the small pairs qualify (lighter U: the pairs near the threshold drop out or join in a cascade).  For delta = 2000: k = 278 .. 294
    puts a_1 = X - k log 2 on both sides of 3, and a_j < -3 < 3 < a_{j+1} needs (X + 3) / log((j+1)/j) < k < (X - 3) / log((j+2)/(j+1)): k = 400 for j = 1,
    1600 for j = 7 and about 4010 for j = 19"""
    specs = [(10, 20, 3, 2000001, 200000)]
    specs += [(100 + 2 * i, 101 + 2 * i, i % 4, 2001, k) for i, k in enumerate(range(278, 295))]
    specs += [(60, 61, 0, 2001, 400), (62, 63, 1, 2001, 1600)] + [(65 + 2 * i, 64 + 2 * i, 2, 2001, k) for i, k in enumerate((3990, 4010, 4030))]
    specs += [(80, 81, 3, 1001, 120), (82, 83, 3, 1002, 120), (84, 85, 3, 1000, 120)]      # delta 1000: never `delta > 1000`; 1001: the loop over j runs
    return specs


def test_built_graph_class_thresholds_and_three_rounds(tmp_path):
    N = 6000
    ctx = store_with_frequencies(N, 22, np.ones(N, dtype=np.int64))
    load_text(ctx, graph_text(N, thresholds_graph(), 6), tmp_path)
    g, f, n, est, net = check_against_model(ctx, tmp_path)
    assert est["rounds"] >= 3 and est["degenerate"] == 0
    lbs = {r[2] + 0 for r in net["arcs"] if r[3] == 3} | {r[2] + 3 for r in net["arcs"] if r[3] == 2 and r[2]} | {r[2] + 5 for r in net["arcs"] if r[3] == 995 and r[2]}
    assert lbs >= {2, 8, 20}, lbs
    recs = [r for _, a, b in g["pairs"] for r in (a, b) if r["frm"] >= r["to"] and r["len"] == 2001 and 270 < len(r["list"]) < 300]
    a1 = [float(M.a_stats(2000, len(r["list"]), n, est["genome_size"])[1]) for r in recs]
    assert any(3 <= a < 6 for a in a1) and any(0 < a < 3 for a in a1), a1            # a_1 on both sides of 3
    assert net["counters"]["once"] >= 2 and net["counters"]["many"] >= 8
    ctx.close()


def test_built_graph_without_a_qualifying_pair_is_degenerate(tmp_path):
    N = 400
    ctx = store_with_frequencies(N, 23, np.random.default_rng(2).integers(1, 9, size=N))
    load_text(ctx, graph_text(N, [(1, 2, 3, 500, 40), (2, 3, 0, 300, 0), (9, 3, 1, 499, 36), (11, 11, 3, 450, 3)], 7), tmp_path)
    g, f, n, est, net = check_against_model(ctx, tmp_path)
    assert (ctx.genome_size(), est["degenerate"], est["rounds"]) == (TWO63, 1, 2) and ctx.copycount_stats().degenerate == 1
    assert net["counters"] == dict(nodes=5, edges=7, simple=1, once=0, many=6)
    ctx.close()


def test_generated_composite_graph(tmp_path):
    """a graph of tests/compgen.py: hubs, loops written once and twice, reads on many pairs, all four types"""
    N, header, recs = compgen.composite_graph(31, 160, hubs=2, list_len=(0, 70), loops_once=2, loops_twice=2, lengths={3: 1400, 9: 1001, 17: 2600, 40: 520})
    ctx = store_with_frequencies(N, 24, np.random.default_rng(3).integers(1, 30, size=N))
    load_text(ctx, H.graph_text(header, recs), tmp_path)
    g, f, n, est, net = check_against_model(ctx, tmp_path)
    assert net["counters"]["many"] > 20 and net["counters"]["edges"] > 160
    ctx.close()


# ------------------------------------------------------------------------------------------ (d) apply
def solution_for(net, seed):
    """a line for every arc of the network with a flow of 0 .. 3 (no solver: any numbers exercise the apply rule)"""
    rng = np.random.default_rng(seed); a = net["arcs"]
    return [(fr, to, int(rng.integers(0, 4))) for fr, to, _, _, _ in a]


def flows_by_ordinal(ctx, text):
    """graph_flows (two values per record pair in the save order, a loop at its first writing) -> {ordinal of the pair in the saved file: (flow, flow of the twin)}"""
    fl = ctx.graph_flows(); keep = [q for q, _, _ in H.parse_graph(text)["pairs"]]
    assert len(fl) == 2 * len(keep)
    return {q: (float(fl[2 * x]), float(fl[2 * x + 1])) for x, q in enumerate(keep)}


def model_apply(ctx, text, g, net, lines):
    """the model's flows after these lines, starting from the library's present flows; a loop's second writing stays as the reference holds it (0)"""
    for q, (fa, fb) in flows_by_ordinal(ctx, text).items():
        g["pairs"][q][1]["flow"], g["pairs"][q][2]["flow"] = fa, fb
    return M.apply_solution(g, net["node_index"], lines)


def apply_graph(tmp_path, seed=8):
    N = 500
    ctx = store_with_frequencies(N, 25, np.random.default_rng(4).integers(1, 6, size=N))
    specs = [(4, 6, 3, 1500, 40), (4, 6, 0, 700, 0), (6, 4, 2, 900, 36), (6, 4, 1, 800, 2), (7, 7, 3, 1200, 50), (6, 9, 3, 600, 5), (9, 12, 2, 2000, 3), (12, 4, 1, 90, 0), (3, 9, 0, 2100, 60)]
    load_text(ctx, graph_text(N, specs, seed), tmp_path)
    return ctx


def test_apply_a_shuffled_solution_and_lines_that_do_not_count(tmp_path):
    ctx = apply_graph(tmp_path); g, f, n, est, net, text = model_of(ctx, tmp_path)
    lines = solution_for(net, 1)
    lines += [(1, 7, 5), (8, 2, 5), (3, 4, 7), (5, 6, 7)]                               # the source, the sink, and arcs inside one graph node (rank 0: cs2 nodes 3 .. 6)
    lines[0] = (2, 1, 13)
    fr, to, fl = (np.asarray(c, dtype=np.uint64) for c in zip(*lines))
    r = model_apply(ctx, text, g, net, lines)                                          # (from the flows of the file: all 0)
    ctx.flow_apply(fr, to, fl)
    st = ctx.copycount_stats()
    assert (st.t_to_s_flow, st.flow_different, st.solution_lines) == (13, r["flow_different"], len(lines)) and r["flow_different"] > 0 and r["t_to_s_flow"] == 13
    want = {q: (float(a["flow"]), float(b["flow"])) for q, a, b in g["pairs"]}
    got = flows_by_ordinal(ctx, text)
    assert got == {q: want[q] for q in got} and any(v[0] for v in got.values())
    loop = [q for q, a, b in g["pairs"] if a["frm"] == a["to"]]
    assert loop and all(got.get(q, (0.0, 0.0)) == (0.0, 0.0) for q in loop)
    # the same lines in another order give the same flows
    c2 = apply_graph(tmp_path); p = np.random.default_rng(9).permutation(len(lines)); c2.flow_apply(fr[p], to[p], fl[p])
    assert np.array_equal(c2.graph_flows(), ctx.graph_flows()) and c2.copycount_stats().flow_different == st.flow_different
    # flows add onto the flows already present: the same lines again, against the model started from the present flows
    r2 = model_apply(ctx, text, g, net, lines); ctx.flow_apply(fr, to, fl)
    got = flows_by_ordinal(ctx, text)
    assert got == {q: (float(g["pairs"][q][1]["flow"]), float(g["pairs"][q][2]["flow"])) for q in got} and ctx.copycount_stats().flow_different == r2["flow_different"]
    assert saved(ctx, tmp_path, ctx.graph4_save, "after.graph4") == text
    ctx.close(); c2.close()


def test_apply_refuses_a_node_outside_the_network(tmp_path):
    ctx = apply_graph(tmp_path); g, f, n, est, net, text = model_of(ctx, tmp_path)
    lines = solution_for(net, 2); fr, to, fl = (np.asarray(c, dtype=np.uint64) for c in zip(*lines))
    ctx.flow_apply(fr, to, fl); before = ctx.graph_flows().copy(); stats = bytes(ctx.copycount_stats())
    for bad in (net["network_nodes"] + 1, 0, 1 << 40):
        f2 = fr.copy(); f2[len(f2) // 2] = bad
        with pytest.raises(s2.Sage2ovError) as e:
            ctx.flow_apply(f2, to, fl)
        assert e.value.code == -1
        with pytest.raises(s2.Sage2ovError) as e:
            ctx.flow_apply(fr, f2, fl)
        assert e.value.code == -1
    assert np.array_equal(ctx.graph_flows(), before) and bytes(ctx.copycount_stats()) == stats
    bad = str(tmp_path / "bad.cs2"); open(bad, "w").write("3 4 1\n7 x 2\n")
    with pytest.raises(s2.Sage2ovError) as e:
        ctx.flow_load(bad)
    assert e.value.code == -2 and np.array_equal(ctx.graph_flows(), before)
    with pytest.raises(s2.Sage2ovError) as e:
        ctx.flow_network_save(str(tmp_path / "no" / "such" / "input.cs2"))
    assert e.value.code == -2
    import ctypes as C
    small = np.zeros(3, dtype=s2.FLOW_ARC_DTYPE)
    assert s2.lib().sage2ov_flow_network_export(ctx._h, C.c_void_p(small.ctypes.data), C.c_uint64(3)) == -1 and not small["from"].any()      # too small: nothing written
    ctx.close()


# ------------------------------------------------------------------------------------------ (e) staleness and call order
def test_calls_without_a_graph_and_a_graph_change(tmp_path):
    m = fx.golden("g6_k70_150"); bases, off = fx.make_reads(m["synth"])
    ctx = s2.Context(m["k"]); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
    for call in (ctx.genome_size, ctx.flow_network_build, ctx.flow_network, lambda: ctx.graph5_save(str(tmp_path / "x.graph5"))):
        with pytest.raises(s2.Sage2ovError) as e:
            call()
        assert e.value.code == -1
    src = str(tmp_path / "in.graph4"); open(src, "wb").write(gold("g6_k70_150", ".graph4.gz")); ctx.graph_load_composite(src)
    ctx.flow_network_build()                                                          # build without an estimate
    st = ctx.copycount_stats(); assert st.genome_size == meta5("g6_k70_150")["genome_size"] and st.network_arcs > 0
    # another graph: estimate and network are dropped and made again
    N, header, recs = compgen.composite_graph(5, 60, n_reads=ctx.reads_stats().unique_reads, list_len=(0, 50))
    load_text(ctx, H.graph_text(header, recs), tmp_path, "other.graph4")
    st = ctx.copycount_stats(); assert (st.genome_size, st.rounds, st.network_arcs, st.nodes) == (0, 0, 0, 0)
    check_against_model(ctx, tmp_path)
    ctx.close()


def test_supports_are_recomputed_after_a_solution(tmp_path):
    """g4: the supports of the graph with all flows 0 are none; after flow_load of the reference's output.cs2 the table is the restatement's
    (tests/test_mate_support_host.py) run on the flows of the committed P.graph5"""
    name = "g4_highcopy_k21"; ctx = golden_ctx(name, tmp_path); k = fx.golden(name)["k"]
    g5 = H.parse_graph(gold(name, ".graph5.gz")); flows = {q: (a["flow"], b["flow"]) for q, a, b in g5["pairs"]}
    g = MS.with_flows(H.parse_graph(gold(name, ".graph4.gz")), lambda q, a: flows[q])
    pairs = MS.golden_mates(g, ctx.reads_stats().unique_reads)
    add_mates(ctx, pairs)
    assert len(ctx.mates_supports(1)) == 0
    before = ([ctx.mates(L)[0].tobytes() for L in pairs], [x.tobytes() for x in ctx.read_edges()])
    out = str(tmp_path / "output.cs2"); open(out, "wb").write(gold(name, ".output.cs2.gz")); ctx.flow_load(out)
    rows, st = check_supports(ctx, g, pairs, k, min_supports=(1, 2))
    assert any(r[5] >= 1 for r in rows)
    assert ([ctx.mates(L)[0].tobytes() for L in pairs], [x.tobytes() for x in ctx.read_edges()]) == before      # the mate table and the read-to-edge table do not move
    ctx.close()


def test_memory_diet_mode(monkeypatch, tmp_path):
    monkeypatch.setenv("SAGE2OV_MEMORY_DIET", "1")
    name = "g4_highcopy_k21"; meta = meta5(name); ctx = golden_ctx(name, tmp_path, steps=True)
    before = saved(ctx, tmp_path, ctx.graph4_save, "before.graph4")
    assert saved(ctx, tmp_path, ctx.flow_network_save, "input.cs2") == gold(name, ".input.cs2.gz")
    out = str(tmp_path / "output.cs2"); open(out, "wb").write(gold(name, ".output.cs2.gz")); ctx.flow_load(out)
    assert saved(ctx, tmp_path, ctx.graph5_save, "t.graph5") == gold(name, ".graph5.gz")
    assert saved(ctx, tmp_path, ctx.graph4_save, "after.graph4") == before and ctx.copycount_stats().flow_different == meta["flow_different"]
    ctx.close()


# ------------------------------------------------------------------------------------------ the command line
def test_cli_flow_network_then_flow_solution(tmp_path):
    """`sage2ov -M 4 --flowNetwork`, then `sage2ov -m 5 --flowSolution output.cs2 --contigs` on the files of the first run: the reference's input.cs2 and P.graph5"""
    import subprocess
    name = "g6_k70_150"; m = fx.golden(name); meta = meta5(name); exe = os.path.join(fx.ROOT, "sage2_amd", "sage2ov")
    fa = str(tmp_path / "x.fa"); s2.synth_write_fasta(fx.synth_params(m["synth"]), fa)
    out = str(tmp_path / "out")
    r = subprocess.run([exe, "-f", fa, "-k", str(m["k"]), "-o", out, "-p", "t", "--flowNetwork"], check=True, stdout=subprocess.PIPE, text=True)      # ends at step 3
    assert "[ERROR] --flowNetwork and --flowSolution need the graph after step 4" in r.stdout and not os.path.exists(os.path.join(out, "input.cs2"))
    r = subprocess.run([exe, "-f", fa, "-k", str(m["k"]), "-o", out, "-p", "t", "-M", "4", "--flowNetwork"], check=True, stdout=subprocess.PIPE, text=True)
    e = meta["estimates"]
    want = "".join("\tGenome Size: %d (Estimation %d)\n" % (v, i + 1) for i, v in enumerate(e[:-1])) + "\tGenome Size: %d (Final estimation)\n" % e[-1]
    assert want in r.stdout
    assert open(os.path.join(out, "input.cs2"), "rb").read() == gold(name, ".input.cs2.gz") and not os.path.exists(os.path.join(out, "t.graph5"))
    sol = os.path.join(out, "output.cs2"); open(sol, "wb").write(gold(name, ".output.cs2.gz"))
    subprocess.run([exe, "-k", str(m["k"]), "-o", out, "-p", "t", "-m", "5", "--flowSolution", sol, "--contigs"], check=True, stdout=subprocess.DEVNULL)
    assert open(os.path.join(out, "t.graph5"), "rb").read() == gold(name, ".graph5.gz")
    assert os.path.getsize(os.path.join(out, "t_contig.fasta")) > 0
    log = open(os.path.join(out, "t.log")).read()
    assert "Flow from T to S: %d" % meta["t_to_s_flow"] in log and "Flow different in edges: %d" % meta["flow_different"] in log
