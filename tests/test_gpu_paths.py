"""GPU: the path supports and their merge rounds (sage2ov_path_supports, sage2ov_extend_paths_round, sage2ov_extend_by_paths) against the restatement
of tests/path_model.py: the table's rows and every counter of the sweep, the written graph byte for byte, the merges of every round, the counts, the flows, the rebuilt
read-to-edge table, and the insert bounds and estimate flags that must not move."""
import os
import subprocess
import numpy as np
import pytest
import fixtures as fx
import sage2_amd as s2
import compgen as CG
import extend_model as X
import path_model as PM
import test_mate_estimate_host as H
import test_mate_support_host as MS
from test_gpu_mate_estimate import add_mates, random_store, load_text
from test_gpu_extend import saved6, start, same_round, table_set, operands

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("minimiser_groups_on")]
K = MS.HAND_K
COUNTERS = ("claimed_reads", "claiming_nodes", "start_nodes", "paths", "capped_nodes", "eligible_entries", "voting_entries", "records", "rows", "key_collisions", "mirrored")


def same_sweep(ctx, g, pairs, est):
    """the device's table and counters against the model's sweep of g"""
    sw = PM.sweep(g, pairs, est)
    got = ctx.path_supports()
    assert [tuple(int(v) for v in list(row)[:8]) for row in got] == PM.export_rows(g, sw["rows"])
    st = ctx.path_stats()
    assert {k: getattr(st, k) for k in COUNTERS} == sw["stats"]
    return sw


def same_path_round(ctx, g, pairs, est, high, variant, hdr, tmp_path, name):
    r = PM.round_(g, pairs, est, high, 1, variant)
    n = ctx.extend_paths_round(high, 1, variant)
    same_round(ctx, n, r)
    st = ctx.path_stats()                                                             # the sweep's figures stand through the merges that dropped its table
    assert st.order_dependent == r["order_dependent"] and {k: getattr(st, k) for k in COUNTERS} == r["stats"]
    assert saved6(ctx, tmp_path, name) == g.text(hdr)
    assert np.array_equal(ctx.graph_flows(), g.flows())
    return r


@pytest.mark.parametrize("case", sorted(PM.CASES))
def test_table_and_counters_on_the_hand_built_graphs(case, tmp_path):
    N, header, recs, pairs, g, est = PM.load(case)
    ctx, g, hdr = start(N, header, recs, pairs, tmp_path)
    ctx.mates_estimate()
    assert ctx.mates_bounds() == (est.min_upper, est.max_upper) == ((278585, 835755) if case == "unclaimed" else (701, 2103))
    sw = same_sweep(ctx, g, pairs, est)
    if case == "unclaimed":                                                          # a mate that no node claims, and the row its entry votes for
        assert 550 not in sw["claim"] and sw["rows"] == [(10, 0, 2, 1)] and sw["stats"]["voting_entries"] == 1
    assert sw["stats"]["capped_nodes"] == (1 if case == "ladder" else 0) and sw["stats"]["key_collisions"] == (1 if case == "chain" else 0)
    assert len(ctx.path_supports(2)) == sum(1 for r in sw["rows"] if r[3] >= 2)
    ctx.close()


@pytest.mark.parametrize("variant", [0, 1])
def test_rounds_on_the_fork_with_a_third_in_edge(variant, tmp_path):
    """round 1 merges C.E and D.F (support 5); in round 2 the rows of A and B at node 10 meet G's: variant 0 refuses, variant 1 merges"""
    N, header, recs, pairs, g, est = PM.load("third")
    ctx, g, hdr = start(N, header, recs, pairs, tmp_path)
    ctx.mates_estimate(); bounds = ctx.mates_bounds(); ins = bytes(ctx.mates_insert(1))
    merged = []
    for rd in range(4):
        r = same_path_round(ctx, g, pairs, est, 2, variant, hdr, tmp_path, f"r{rd}.graph6")
        assert table_set(ctx) == X.read_edge_set(g)                                  # rebuilt from the merged graph
        assert ctx.mates_bounds() == bounds and bytes(ctx.mates_insert(1)) == ins    # the estimate stands
        same_sweep(ctx, g, pairs, est)                                               # ... and so do its flags: the next sweep's eligible entries are the model's
        merged.append(len(r["merges"]))
        if not r["merges"]:
            break
    assert merged == ([2, 0] if variant == 0 else [2, 1, 1, 0])                       # variant 1: A.CE in round 2, B.DF in round 3 (a merge takes every row filed under node 10 with it)
    ctx.close()


@pytest.mark.parametrize("variant", [0, 1])
def test_loops_on_the_fork(variant, tmp_path):
    N, header, recs, pairs, g, est = PM.load("third")
    ctx, g, hdr = start(N, header, recs, pairs, tmp_path)
    gs = hdr[1] * header[2] // 6                                                    # coverage 6: highTh = 2
    assert X.threshold(hdr[1], header[2], gs) == 2
    rs = PM.extend(g, pairs, est, gs, hdr[1], variant)
    assert ctx.extend_by_paths(gs, variant) == (len(rs), sum(len(r["merges"]) for r in rs))
    assert saved6(ctx, tmp_path) == g.text(hdr) and np.array_equal(ctx.graph_flows(), g.flows())
    assert ctx.extend_by_paths(gs, variant) == (1, 0)                                # a fixed point
    ctx.close()


def test_a_pair_on_one_edge_after_a_merge_keeps_its_estimate_flag(tmp_path):
    """43 stands on A and 63 in the middle of a C of 5 000 bases, beyond the bound from either end: no node claims it.  After MERGE(A, C) both stand on one edge.  The
    flags of the graph as it now is say 0, the estimate's say 1: the entry is eligible before and after"""
    N, header, recs, pairs = PM.fork_graph(long_c=True, extra=[(43, 1, 63, 0)])
    ctx, g, hdr = start(N, header, recs, pairs, tmp_path)
    est = PM.Estimate(g, pairs)
    ctx.mates_estimate()
    sw = same_sweep(ctx, g, pairs, est); before = sw["stats"]["eligible_entries"]
    assert 63 not in sw["claim"] and sw["claim"][43] == 1
    f, s_ = operands(g, [(0, 4)])
    assert ctx.merge_pairs(f, s_).tolist() == [1] and g.merge(0, 4) is not None
    now = PM.Estimate(g, pairs)
    at = PM.entries_of(pairs, 1).index((43, 63, 1, 0))
    assert est.flags[1][at] == 1 and now.flags[1][at] == 0 and int(ctx.mates_flags(1)[at]) == 0
    after = same_sweep(ctx, g, pairs, est)["stats"]["eligible_entries"]
    assert after == before                                                            # (with the flags of the merged graph the model counts one less)
    assert PM.sweep(g, pairs, now)["stats"]["eligible_entries"] == after - 1
    ctx.close()


@pytest.mark.parametrize("seed,variant", [(2, 0), (3, 1)])
def test_generated_graph_with_hubs_sweep_and_rounds(seed, variant, tmp_path):
    """about 200 pairs with a hub, loops written once and twice, simple edges, reads on many pairs and twice on an edge, flows from (0, 0.5, 1, 2): more than 64
    claiming nodes, more than one block of list entries"""
    N, header, recs = CG.case_e(seed)
    parsed = H.parse_graph(H.graph_text(header, recs)); pairs = CG.mates_e(parsed, seed)
    ctx, g, hdr = start(N, header, recs, pairs, tmp_path, seed=9)
    est = PM.Estimate(g, pairs)
    ctx.mates_estimate()
    assert ctx.mates_bounds() == (est.min_upper, est.max_upper)
    sw = same_sweep(ctx, g, pairs, est)
    assert sw["stats"]["claiming_nodes"] > 64 and sum(len(r["list"]) for r in recs) > 2 * 256 and sw["stats"]["voting_entries"] > 50
    total = refused = blocked = 0
    for rd in range(12):
        r = same_path_round(ctx, g, pairs, est, 2, variant, hdr, tmp_path, f"r{rd}.graph6")
        total += len(r["merges"]); refused += r["refused"]; blocked += r["blocked"]
        if not r["merges"]:
            break
    assert total >= 10 and blocked and rd >= 2 and (refused or variant == 1)          # (the model alone says so: not vacuous)
    assert table_set(ctx) == X.read_edge_set(g)
    assert ctx.mates_bounds() == (est.min_upper, est.max_upper)
    ctx.close()


def test_first_loop_then_loops_two_and_three_on_one_context(tmp_path):
    seed = 4
    N, header, recs = CG.case_e(seed)
    parsed = H.parse_graph(H.graph_text(header, recs)); pairs = CG.mates_e(parsed, seed)
    ctx, g, hdr = start(N, header, recs, pairs, tmp_path, seed=9)
    est = PM.Estimate(g, pairs)
    gs = hdr[1] * header[2] // 6
    r1 = X.extend(g, pairs, est, CG.K, gs, hdr[1])
    assert ctx.extend_by_supports(gs) == (len(r1), sum(len(r["merges"]) for r in r1))
    total = 0
    for variant in (0, 1):
        rs = PM.extend(g, pairs, est, gs, hdr[1], variant)
        assert ctx.extend_by_paths(gs, variant) == (len(rs), sum(len(r["merges"]) for r in rs))
        assert saved6(ctx, tmp_path, f"v{variant}.graph6") == g.text(hdr)
        total += sum(len(r["merges"]) for r in rs)
    assert sum(len(r["merges"]) for r in r1) >= 1 and total >= 1
    assert np.array_equal(ctx.graph_flows(), g.flows()) and table_set(ctx) == X.read_edge_set(g)
    assert ctx.mates_bounds() == (est.min_upper, est.max_upper)
    ctx.close()


def test_after_step_4_every_flow_is_zero_and_the_table_is_empty(tmp_path):
    name = "g4_highcopy_k21"; m = fx.golden(name); bases, off = fx.make_reads(m["synth"])
    ctx = s2.Context(m["k"]); ctx.reads_add_ascii(bases, off); ctx.reads_organize(); ctx.run_steps23(); ctx.graph_simplify()
    p4 = str(tmp_path / "s.graph4"); ctx.graph4_save(p4)
    parsed = H.parse_graph(open(p4).read())
    add_mates(ctx, MS.golden_mates(parsed, ctx.reads_stats().unique_reads))
    assert len(ctx.path_supports()) == 0 and ctx.path_stats().paths == 0
    assert ctx.extend_paths_round(2) == 0 and ctx.extend_paths_round(2, 1, 1) == 0 and len(ctx.extend_merges()) == 0
    p6 = str(tmp_path / "s.graph6"); ctx.graph6_save(p6)
    assert H.parse_graph(open(p6).read())["pairs"] == parsed["pairs"]
    ctx.close()


def test_abi_error_paths(tmp_path):
    import ctypes as C
    lib = s2.lib()
    assert lib.sage2ov_path_supports(None) == -1 and lib.sage2ov_path_stats_get(None, None) == -1 and lib.sage2ov_extend_paths_round(None, 2, 1, 0, None) == -1
    assert lib.sage2ov_extend_by_paths(None, C.c_uint64(0), 0, None, None) == -1
    ctx = random_store(90, 5)                                                        # reads, no graph
    for call in (ctx.path_supports, ctx.path_supports_build, lambda: ctx.extend_paths_round(2), lambda: ctx.extend_by_paths(1000)):
        with pytest.raises(s2.Sage2ovError) as e:
            call()
        assert e.value.code == -1
    N, header, recs, pairs, g, est = PM.load("fork")
    load_text(ctx, H.graph_text(header, recs), tmp_path); add_mates(ctx, pairs)
    for variant in (2, -1):
        with pytest.raises(s2.Sage2ovError) as e:
            ctx.extend_paths_round(2, 1, variant)
        assert e.value.code == -1
        with pytest.raises(s2.Sage2ovError) as e:
            ctx.extend_by_paths(1000, variant)
        assert e.value.code == -1
    n = C.c_uint64(0)
    assert lib.sage2ov_path_supports_count(ctx._h, C.c_uint32(1), C.byref(n)) == 0 and n.value == 4
    buf = np.zeros(4, dtype=s2.PATH_SUPPORT_DTYPE)
    assert lib.sage2ov_path_supports_export(ctx._h, C.c_uint32(1), C.c_void_p(buf.ctypes.data), C.c_uint64(3)) == -1 and not buf["support"].any()
    assert lib.sage2ov_path_supports_export(ctx._h, C.c_uint32(1), None, C.c_uint64(4)) == -1
    assert lib.sage2ov_path_supports_count(ctx._h, C.c_uint32(1), None) == -1
    host = s2.Context(K, device=-2)                                                  # no device: the sweep runs there only
    with pytest.raises(s2.Sage2ovError) as e:
        host.path_supports()
    assert e.value.code == -3
    ctx.close(); host.close()


def test_cli_extend_with_and_without_paths(tmp_path):
    """sage2ov -m 6 --extend --paths against the same calls on a context; --extend alone against the first loop's expectation"""
    N, header, recs, pairs, g, est = PM.load("third")
    ctx, g, hdr = start(N, header, recs, None, tmp_path)
    out = str(tmp_path / "out") + "/"; os.makedirs(out)
    ctx.reads_save(out + "t.reads"); ctx.graph5_save(out + "t.graph5")
    seqs = H.stored_reads(ctx)
    b_, o = H.mates_ascii(pairs[1], seqs); fa = str(tmp_path / "mates.fa")
    open(fa, "w").write("".join(">m%d\n%s\n" % (i, b_[int(o[i]):int(o[i + 1])].tobytes().decode()) for i in range(len(o) - 1)))
    gs = hdr[1] * header[2] // 6
    exe = os.path.join(fx.ROOT, "sage2_amd", "sage2ov")
    base = [exe, "-k", str(K), "-o", out, "-i", "t", "-m", "6", "-f", fa, "--genomeSize", str(gs)]
    subprocess.run(base + ["-p", "plain", "--extend"], check=True, stdout=subprocess.DEVNULL, timeout=120)
    g1 = X.Graph(H.parse_graph(H.graph_text(header, recs)))
    r1 = X.extend(g1, pairs, est, K, gs, hdr[1])
    assert open(out + "plain.graph6").read() == g1.text(hdr) and "findPathSupports" not in open(out + "plain.log").read()
    subprocess.run(base + ["-p", "paths", "--extend", "--paths"], check=True, stdout=subprocess.DEVNULL, timeout=120)
    add_mates(ctx, pairs)
    first = ctx.extend_by_supports(gs); two = ctx.extend_by_paths(gs, 0); three = ctx.extend_by_paths(gs, 1)
    assert first == (len(r1), sum(len(r["merges"]) for r in r1)) and two[1] + three[1] >= 3
    assert open(out + "paths.graph6").read() == saved6(ctx, tmp_path)
    log = open(out + "paths.log").read()
    assert "Rounds of findPathSupports: %d " % two[0] in log and "Rounds of findPathSupportsNew: %d " % three[0] in log
    assert "Total number of extended contigs: %d\n" % (first[1] + two[1] + three[1]) in log
    bad = subprocess.run([exe, "-k", str(K), "-o", out, "-i", "t", "-p", "bad", "-m", "6", "-M", "6", "-f", fa, "--paths"], stdout=subprocess.PIPE, text=True, timeout=120)
    assert "[ERROR] --paths goes with -m 6 --extend" in bad.stdout and not os.path.exists(out + "bad.graph6")      # --paths without --extend
    ctx.close()
