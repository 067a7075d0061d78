"""GPU: the fourth loop of extendContigs (sage2ov_links_gap_sums, sage2ov_extend_short_round, sage2ov_extend_by_short_overlaps, sage2ov_extend_contigs,
`sage2ov -m 6 --extend --paths --shortOverlaps`) against the restatement of tests/short_model.py: the raw gap sum of every link row, the joins and
counts of every round, the written graph byte for byte, the flows, the rebuilt read-to-edge table, the insert bounds that must not move -- and against what the
reference itself did (tests/golden/short/).  Every comparison is exact equality."""
import gzip
import json
import os
import subprocess
import numpy as np
import pytest
import fixtures as fx
import sage2_amd as s2
import scaffold_model as SM
import short_model as SO
import extend_model as X
import test_mate_estimate_host as H
import test_mate_support_host as MS
import test_links_host as LH
import test_scaffold_host as SH
import test_short_host as TH
from test_gpu_mate_estimate import add_mates, random_store, load_text
from test_gpu_mate_support import saved_graph, flat_flows
from test_gpu_extend import saved6, table_set

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("minimiser_groups_on")]
K = LH.HAND_K
MODES = (LH.ALL, LH.FINAL, LH.SMALL)


# ------------------------------------------------------------------------------------------ the gap sums
def want_sums(g, pairs, k):
    t, ests, (_, hi) = MS.support_inputs(g, pairs)
    return SO.link_sums(g, t, pairs, ests, hi, g["header"][2], k)


def by_ends(g, sums):
    """{(a.from, a.to, b.from, b.to): (support, gapSum)}: the file's ordinals move when a loop is written twice, the ends do not"""
    hv = LH.halves_of(g)
    return {(hv[(r[0], r[1])][0]["frm"], hv[(r[0], r[1])][0]["to"], hv[(r[2], r[3])][0]["frm"], hv[(r[2], r[3])][0]["to"]): r[4:] for r in sums}


def check_sums(ctx, g, pairs, k, min_supports=(1, 2)):
    """links_gap_sums under every filter against the restatement; gap == trunc(gapSum / support) row by row; the export's bytes before and after"""
    sums = want_sums(g, pairs, k); E = LH.e_half(g); arl = g["header"][2]
    for mode in MODES:
        for ms in min_supports:
            before = ctx.links(mode, ms).tobytes()
            got = ctx.links_gap_sums(mode, ms); rows = ctx.links(mode, ms)
            assert rows.tobytes() == before and got.dtype == np.int32 and len(got) == len(rows)
            want = [r for r in sums if r[4] >= ms and LH.passes(mode, E[r[0]]["len"], E[r[0]]["flow"], E[r[2]]["len"], E[r[2]]["flow"], arl)]
            assert got.tolist() == [r[5] for r in want], (mode, ms)
            assert [int(r["gap"]) for r in rows] == [SO.quotient(int(s), int(r["support"])) for s, r in zip(got, rows)]
    return sums


@pytest.mark.parametrize("variant", [None, 666, 667, "components"])
def test_gap_sums_on_the_hand_graph_and_its_variants(variant, tmp_path):
    if variant == "components":
        N, header, recs, pairs, _ = TH.short_graph(TH.ALL, flows=TH.C2)
    else:
        N, header, recs, pairs = LH.hand_link_graph(variant)
    ctx = random_store(N, 5); load_text(ctx, H.graph_text(header, recs), tmp_path)
    g, _ = saved_graph(ctx, tmp_path, recs); add_mates(ctx, pairs)
    sums = check_sums(ctx, g, pairs, K)
    d = by_ends(g, sums)
    if variant is None:
        assert len(sums) == LH.HAND_ROWS and d[(20, 21, 22, 23)] == (2, -7) and d[(24, 24, 20, 21)] == (1, 11)      # G - Hh, the loop Lq - G
    if variant == "components":
        assert d[(251, 101, 105, 301)] == (2, 1) and d[(256, 113, 117, 308)] == (2, -1) and d[(261, 125, 129, 315)] == (1, 0)      # "plus", "minus", "zero": gap 0 all three
    with pytest.raises(s2.Sage2ovError) as e:
        ctx.links_gap_sums(3)
    assert e.value.code == -1
    out = (np.zeros(1, dtype=np.int32))
    assert s2.lib().sage2ov_links_gap_sums(ctx._h, s2.C.c_uint32(0), s2.C.c_uint32(1), s2.C.c_void_p(out.ctypes.data), s2.C.c_uint64(1)) == -1      # cap below the rows
    ctx.close()


def golden_loaded(name, tmp_path, diet=False):
    m = fx.golden(name); bases, off = fx.make_reads(m["synth"])
    text = gzip.open(os.path.join(fx.GOLDEN, name + ".graph4.gz")).read()
    g = MS.with_flows(H.parse_graph(text), MS.golden_flow)
    ctx = s2.Context(m["k"]); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
    if diet:
        ctx.index_build()                                                              # memory-diet mode releases the id-ordered store here
    pairs = LH.golden_pairs(name, MS.with_flows(H.parse_graph(text, fold=False), MS.golden_flow), ctx.reads_stats().unique_reads)
    src = str(tmp_path / "in.graph4"); open(src, "wb").write(text); ctx.graph_load_composite(src)
    ctx.graph_set_flows(flat_flows(g)); add_mates(ctx, pairs)
    return ctx, m["k"], g, pairs


@pytest.mark.parametrize("name", ["g4_highcopy_k21", "g9_repeats160k_k40"])
def test_gap_sums_on_the_goldens_with_long_range_mates(name, tmp_path):
    ctx, k, g, pairs = golden_loaded(name, tmp_path)
    sums = check_sums(ctx, g, pairs, k)
    assert any(r[4] >= 2 and r[5] % r[4] for r in sums) and any(r[5] <= 0 for r in sums) and len(sums) > 500      # (not vacuous: quotients that truncate; the positive sums are the hub's, below)
    ctx.close()


def test_gap_sums_in_memory_diet_mode(monkeypatch, tmp_path):
    ctx, k, g, pairs = golden_loaded("g4_highcopy_k21", tmp_path)
    want = [ctx.links_gap_sums(mode).tobytes() for mode in MODES]; assert all(len(w) > 0 for w in want)
    monkeypatch.setenv("SAGE2OV_MEMORY_DIET", "1")
    c2, _, _, _ = golden_loaded("g4_highcopy_k21", tmp_path, diet=True)
    assert [c2.links_gap_sums(mode).tobytes() for mode in MODES] == want
    check_sums(c2, g, pairs, k, min_supports=(1,))
    ctx.close(); c2.close()


def test_gap_sums_of_the_hub_across_the_sort_tiles(tmp_path):
    """tests/test_gpu_links.py's hub: one half linked to 1 600 partner edges, 6 400 records under one first word (more than three radix tiles); every row's sum is
    four records' worth"""
    n = 1600
    nodes = iter(range(1, 2 * (n + 2) + 1)); reads = iter(range(2 * (n + 2) + 1, 2 * (n + 2) + 1 + 4 + 300 + 2 * n))
    rec = H.rec
    U = rec(next(nodes), next(nodes), 3, 300, [(next(reads), 0, 0, 1 + j, 1) for j in range(4)])
    Z = rec(next(nodes), next(nodes), 3, 4000, [(next(reads), 0, 0, 1, 1) for _ in range(300)])
    P = [rec(next(nodes), next(nodes), 3, 100 + (i % 5) * 100, [(next(reads), 0, 0, 1 + i % 97, 1) for _ in range(2)]) for i in range(n)]
    recs = []
    for i, r in enumerate([U, Z] + P):
        t = H.twin_of(r); r["flow"] = t["flow"] = float(i % 2); recs += [r, t]
    N = 2 * (n + 2) + 4 + 300 + 2 * n; header = (0, 2 * N, 60)
    same = [(Z["list"][i][0], 1, Z["list"][i + (200 if i % 2 else 290)][0], 1) for i in range(10)]
    cross = [(u[0], 1, p["list"][0][0], 1) for u in U["list"] for p in P]
    pairs = {1: same + cross}
    ctx = random_store(N, 9); load_text(ctx, H.graph_text(header, recs), tmp_path)
    g, _ = saved_graph(ctx, tmp_path, recs); add_mates(ctx, pairs)
    sums = check_sums(ctx, g, pairs, 40, min_supports=(1, 4))
    from_u = [r for r in sums if r[:2] == (0, 0)]
    assert len(from_u) == n and all(r[4] == 4 for r in from_u) and sum(r[4] for r in from_u) > 3 * 2048 and len({r[5] for r in from_u}) > 50 and all(r[5] > 0 for r in from_u)      # the restatement says so
    ctx.close()


def test_gap_sums_go_stale_with_the_table(tmp_path):
    N, header, recs, pairs, _ = TH.short_graph(["plus", "minus"])
    ctx = random_store(N, 5); load_text(ctx, H.graph_text(header, recs), tmp_path)
    g, _ = saved_graph(ctx, tmp_path, recs)
    assert len(ctx.links_gap_sums()) == 0                                              # before any mates: it estimates and sweeps itself; an empty table
    add_mates(ctx, {1: pairs[1][:-1]})                                                 # without "minus"'s second mate: support 1, gapSum +6
    first = {1: pairs[1][:-1]}
    d = by_ends(g, check_sums(ctx, g, first, K))
    assert d[(256, 113, 117, 308)] == (1, 6)
    add_mates(ctx, {1: pairs[1][-1:], 2: pairs[2]})                                    # a mate add: the table is stale, gap_sums rebuilds it
    d = by_ends(g, check_sums(ctx, g, {1: pairs[1], 2: pairs[2]}, K))
    assert d[(256, 113, 117, 308)] == (2, -1)
    ctx.mates_clear(); assert len(ctx.links_gap_sums()) == 0
    ctx.close()


# ------------------------------------------------------------------------------------------ rounds
def start(tmp_path, names, seed=5, **kw):
    N, header, recs, pairs, _ = TH.short_graph(names, **kw)
    ctx = random_store(N, seed); text = H.graph_text(header, recs); load_text(ctx, text, tmp_path)
    g = SM.Graph(H.parse_graph(text)); hdr = (ctx.genome_size(), ctx.copycount_stats().reads_present, header[2])
    assert saved6(ctx, tmp_path, "before.graph6") == g.text(hdr)
    add_mates(ctx, pairs)
    return ctx, g, hdr, pairs, H.stored_reads(ctx)


def same_round(ctx, n, r):
    got = ctx.extend_short_merges()
    assert n == len(r["merges"]) == len(got)
    assert [tuple(v.item() for v in list(row)[:14]) for row in got] == SM.joins_rows(r)
    st = ctx.extend_short_stats().last
    assert (st.rows, st.below_threshold, st.skipped, st.blocked, st.cycles, st.merged, st.batches) == (r["rows"], r["below_threshold"], r["skipped"], r["blocked"], 0, len(r["merges"]), r["batches"])
    assert (st.overlaps, st.concatenated, st.gapped, st.outside_reference) == (r["overlaps"], r["concatenated"], r["gapped"], int(r["outside_reference"]))
    assert st.pairs_deleted == sum(m["first_deleted"] + m["second_deleted"] for m in r["merges"])


@pytest.mark.parametrize("high,names,kw,first", [(1, TH.ALL, dict(flows=TH.C2), 2), (2, TH.ALL, dict(flows=TH.C2), 3), (2, ["plus", "minus"], dict(), 2), (1, ["zero", "twin"], dict(flows=SH.KEPT), 1),
                                                 (1, [], SH.CYCLE, 0), (2, ["chain", "noflow", "len60"], SH.CYCLE, 2), (3, ["minus"], dict(flows=TH.C2), 1), (0, ["minus", "zero"], dict(flows=TH.C2), None)])
def test_hand_built_graphs_round_by_round(high, names, kw, first, tmp_path):
    """every case of tests/test_short_host.py on the device; high 0 lies outside what equality with the reference is claimed for, the model and the device still agree"""
    ctx, g, hdr, pairs, seqs = start(tmp_path, names, **kw)
    b = X.Bounds(g, pairs)
    ctx.mates_estimate(); bounds = ctx.mates_bounds(); ins = [bytes(ctx.mates_insert(L)) for L in (1, 2)]
    assert bounds == (b.min_upper, b.max_upper)
    for rd in range(6):
        r = SO.round_(g, pairs, b, K, high, seqs)
        n = ctx.extend_short_round(high)
        assert first is None or rd or n == first
        same_round(ctx, n, r)
        assert saved6(ctx, tmp_path, f"r{rd}.graph6") == g.text(hdr)
        assert np.array_equal(ctx.graph_flows(), g.flows())
        assert table_set(ctx) == X.read_edge_set(g)
        assert ctx.mates_bounds() == bounds and [bytes(ctx.mates_insert(L)) for L in (1, 2)] == ins      # the estimate stands
        if not n:
            break
    assert not n and ctx.extend_short_stats().rounds == rd + 1
    ctx.close()


def test_a_graph_without_flows_has_no_rows(tmp_path):
    """step 4's own graph carries no flow array until step 5 or the caller hands one in: no row passes, and the graph stays as it is"""
    name = "g4_highcopy_k21"; m = fx.golden(name); bases, off = fx.make_reads(m["synth"])
    ctx = s2.Context(m["k"]); ctx.reads_add_ascii(bases, off); ctx.reads_organize(); ctx.run_steps23(); ctx.graph_simplify()
    p4 = str(tmp_path / "s.graph4"); ctx.graph4_save(p4)
    parsed = H.parse_graph(open(p4).read())
    add_mates(ctx, LH.merged(MS.golden_mates(parsed, ctx.reads_stats().unique_reads), LH.long_range_mates(parsed)))
    assert len(ctx.links()) > 0 and ctx.extend_short_round(1) == 0
    st = ctx.extend_short_stats().last; assert (st.rows, st.merged, st.batches) == (0, 0, 0)
    ctx.graph4_save(str(tmp_path / "t.graph4")); assert open(str(tmp_path / "t.graph4")).read() == open(p4).read()
    ctx.close()


@pytest.mark.parametrize("seed,high", [(2, 3), (3, 3)])
def test_generated_graphs_with_hubs_round_by_round(seed, high, tmp_path):
    """about 200 pairs with a hub, loops and reads on many pairs, every flow 2, mates at the nodes and long-range ones: a few hundred rows of which most are below
    the threshold, blocked by a rival, or skipped because a join erased their key"""
    import compgen as CG
    N, header, recs = CG.case_e(seed)
    for r in recs:
        r["flow"] = 2.0
    parsed = H.parse_graph(H.graph_text(header, recs)); pairs = LH.merged(CG.mates_e(parsed, seed), LH.long_range_mates(parsed))
    ctx = random_store(N, 9); text = H.graph_text(header, recs); load_text(ctx, text, tmp_path)
    g = SM.Graph(H.parse_graph(text)); hdr = (ctx.genome_size(), ctx.copycount_stats().reads_present, header[2])
    add_mates(ctx, pairs); seqs = H.stored_reads(ctx)
    b = X.Bounds(g, pairs); total = blocked = skipped = rows = 0
    for rd in range(4):
        r = SO.round_(g, pairs, b, CG.K, high, seqs)
        n = ctx.extend_short_round(high)
        same_round(ctx, n, r)
        assert saved6(ctx, tmp_path, f"r{rd}.graph6") == g.text(hdr) and np.array_equal(ctx.graph_flows(), g.flows())
        total += n; blocked += r["blocked"]; skipped += r["skipped"]; rows = max(rows, r["rows"])
        if not n:
            break
    assert not n and total >= 2 and blocked and skipped and rows > 200                 # (the model alone says so: not vacuous)
    assert table_set(ctx) == X.read_edge_set(g) and ctx.mates_bounds() == (b.min_upper, b.max_upper)
    ctx.close()


def test_after_steps_1_to_4_with_flows_handed_in(tmp_path):
    """the graph step 4 left in HBM, not a loaded one: g4 with every flow 2, the golden mates and long-range mates.  Rule (a) compares pool indices, which the model,
    reading the written file, cannot see: as in tests/test_gpu_scaffold.py the device's own joins are replayed through the model's JOIN.  Checked per round: every
    join is a row of the model's unfiltered links (its pairs, ends, support, gap = gapSum / support) with a support at or above `high`, a gapSum <= 0 and lengths and
    flows that pass the filter; the counts add up; and after the replay the written graph, the flows and the rebuilt read-to-edge table are the model's"""
    name = "g4_highcopy_k21"; m = fx.golden(name); bases, off = fx.make_reads(m["synth"]); k = m["k"]; high = 2
    ctx = s2.Context(k); ctx.reads_add_ascii(bases, off); ctx.reads_organize(); ctx.run_steps23(); ctx.graph_simplify()
    p4 = str(tmp_path / "s.graph4"); ctx.graph4_save(p4)
    parsed = MS.with_flows(H.parse_graph(open(p4).read()), lambda q, a: (2.0, 2.0))
    pairs = LH.merged(MS.golden_mates(parsed, ctx.reads_stats().unique_reads), LH.long_range_mates(parsed))
    g = SM.Graph(parsed); b = X.Bounds(g, pairs)
    add_mates(ctx, pairs); ctx.graph_set_flows(g.flows()); seqs = H.stored_reads(ctx)
    hdr = (ctx.genome_size(), ctx.copycount_stats().reads_present, parsed["header"][2])
    total = 0
    for rd in range(3):
        sums = SO.sums_of(g, pairs, b, k); keep = SO.short_filter(g, sums)
        o = g.ordinals()
        n = ctx.extend_short_round(high)
        if rd == 0:
            assert ctx.mates_bounds() == (b.min_upper, b.max_upper)
        st = ctx.extend_short_stats().last; joins = ctx.extend_short_merges()
        assert n == len(joins) == st.merged and st.rows == st.below_threshold + st.skipped + st.blocked + st.merged and st.cycles == 0
        for j in joins:
            cand = [(2 * qa + sa, 2 * qb + sb) for (qa, sa, qb, sb, s_, gs) in sums
                    if (o[qa], o[qb], s_, SO.quotient(gs, s_)) == (int(j["pair_first"]), int(j["pair_second"]), int(j["support"]), int(j["gap"])) and s_ >= high
                    and gs <= 0 and keep(qa, qb, s_, gs)
                    and (g.h[(2 * qa + sa) ^ 1]["frm"], g.h[2 * qb + sb]["to"]) == (int(j["from"]), int(j["to"]))
                    and SM.join_type(g.h[(2 * qa + sa) ^ 1]["type"], g.h[2 * qb + sb]["type"]) == int(j["type"])]
            assert len(cand) >= 1, j                                                   # a row of the unfiltered table that passes the filter, at or above the threshold
            a, e2 = cand[0]
            g.join(a ^ 1, e2, int(j["gap"]), seqs)
            assert (int(j["overlap_forward"]), int(j["overlap_twin"])) == g.last["overlap"] and (int(j["how_forward"]), int(j["how_twin"])) == g.last["how"]
            assert [int(j["first_deleted"]), int(j["second_deleted"])] == [int(x) for x in g.last["deleted"]]
        assert saved6(ctx, tmp_path, f"r{rd}.graph6") == g.text(hdr) and np.array_equal(ctx.graph_flows(), g.flows())
        total += n
        if not n:
            break
    assert total >= 1
    assert table_set(ctx) == X.read_edge_set(g)
    ctx.close()


# ------------------------------------------------------------------------------------------ the loop, extend_contigs, and what a short round leaves alone
def test_the_loop_against_the_model_and_the_scaffolds_records_untouched(tmp_path):
    ctx, g, hdr, pairs, seqs = start(tmp_path, TH.ALL, flows=TH.C2)
    b = X.Bounds(g, pairs)
    assert ctx.scaffold_round(6, 1) == 0                                               # a scaffold round first, so that its records hold something: rows, all below 6
    sc_before = bytes(ctx.scaffold_stats()); assert ctx.scaffold_stats().rounds == 1 and ctx.scaffold_stats().last.rows > 0
    gs = hdr[1] * hdr[2] // 6                                                          # coverage 6 at read length 60: high 1
    assert s2.extend_short_threshold(hdr[1], hdr[2], gs) == 1
    rs = SO.loop(g, pairs, b, K, gs, hdr[1], seqs)
    joined = sum(len(r["merges"]) for r in rs)
    assert ctx.extend_by_short_overlaps(gs) == (len(rs), joined) and joined == 2
    assert saved6(ctx, tmp_path) == g.text(hdr) and np.array_equal(ctx.graph_flows(), g.flows())
    st = ctx.extend_short_stats()
    assert st.rounds == len(rs) and st.total.merged == joined and st.total.cycles == 0 and st.total.gapped == sum(r["gapped"] for r in rs) == 4
    assert st.total.rows == sum(r["rows"] for r in rs) and st.total.blocked == sum(r["blocked"] for r in rs)
    # step 7's own last-round records and totals have not seen the short rounds; the short records have not seen the scaffold round
    assert bytes(ctx.scaffold_stats()) == sc_before and len(ctx.scaffold_merges()) == 0
    assert ctx.scaffold_round(1, 2) >= 1 and ctx.extend_short_stats().rounds == len(rs) and bytes(ctx.extend_short_stats()) == bytes(st)
    ctx.close()


def test_extend_contigs_is_the_four_loops_one_by_one(tmp_path):
    ctx, g, hdr, pairs, seqs = start(tmp_path, TH.ALL, flows=TH.C2)
    c2, _, _, _, _ = start(tmp_path, TH.ALL, flows=TH.C2)
    gs = hdr[1] * hdr[2] // 6
    rounds, merged = ctx.extend_contigs(gs)
    one = [c2.extend_by_supports(gs), c2.extend_by_paths(gs, 0), c2.extend_by_paths(gs, 1), c2.extend_by_short_overlaps(gs)]
    assert (rounds, merged) == ([x[0] for x in one], [x[1] for x in one]) and merged[3] >= 1 and all(r >= 1 for r in rounds)
    assert saved6(ctx, tmp_path, "a.graph6") == saved6(c2, tmp_path, "b.graph6") and np.array_equal(ctx.graph_flows(), c2.graph_flows())
    assert bytes(ctx.extend_short_stats().total)[:104] == bytes(c2.extend_short_stats().total)[:104]      # the counters (the five times behind them are measured)
    assert ctx.extend_stats().rounds == c2.extend_stats().rounds and ctx.mates_bounds() == c2.mates_bounds()
    ctx.close(); c2.close()


# ------------------------------------------------------------------------------------------ the command line
def test_cli_extend_paths_short_overlaps_contigs(tmp_path):
    """sage2ov -m 6 --extend --paths --shortOverlaps --contigs: the whole extendContigs on P.graph5, P.graph6 and P_contig.fasta out, against a context that does the
    same by calls"""
    ctx, g, hdr, pairs, seqs = start(tmp_path, TH.ALL, flows=TH.C2)
    out = str(tmp_path / "out") + "/"; os.makedirs(out)
    ctx.reads_save(out + "t.reads"); ctx.graph5_save(out + "t.graph5")
    b_, o = H.mates_ascii(pairs[1], seqs); fa = str(tmp_path / "mates.fa")             # (-f is library 1 alone)
    open(fa, "w").write("".join(">m%d\n%s\n" % (i, b_[int(o[i]):int(o[i + 1])].tobytes().decode()) for i in range(len(o) - 1)))
    gs = hdr[1] * hdr[2] // 6
    exe = os.path.join(fx.ROOT, "sage2_amd", "sage2ov")
    subprocess.run([exe, "-k", str(K), "-o", out, "-p", "u", "-i", "t", "-m", "6", "-f", fa, "--extend", "--paths", "--shortOverlaps", "--contigs", "--genomeSize", str(gs)],
                   check=True, stdout=subprocess.DEVNULL, timeout=120)
    c2 = random_store(len(seqs), 5); c2.graph_load_composite(out + "t.graph5"); add_mates(c2, {1: pairs[1]})
    c2.mates_estimate(); rounds, merged = c2.extend_contigs(gs)
    assert open(out + "u.graph6").read() == saved6(c2, tmp_path, "calls.graph6") and merged[3] >= 1
    c2.contigs_build(0, gs); c2.contigs_save(str(tmp_path / "calls.fasta"), 0)
    assert open(out + "u_contig.fasta").read() == open(str(tmp_path / "calls.fasta")).read() and os.path.getsize(out + "u_contig.fasta") > 0
    log = open(out + "u.log").read(); ss = c2.extend_short_stats().total
    assert "Total number of extended contigs: %d\n" % sum(merged) in log and "Rounds of mergeShortOverlaps: %d (%d rows, " % (rounds[3], ss.rows) in log
    assert "with a gap %d; %d merges)" % (ss.gapped, merged[3]) in log and "\tStep 6 in " in log and "First loop of step 6" not in log
    bad = subprocess.run([exe, "-k", str(K), "-o", out, "-p", "v", "-i", "t", "-m", "7", "-f", fa, "--scaffold", "--shortOverlaps"], stdout=subprocess.PIPE, text=True, timeout=120)
    assert "--shortOverlaps goes with -m 6 --extend" in bad.stdout
    ctx.close(); c2.close()


# ------------------------------------------------------------------------------------------ what the reference itself did (tests/golden/short/, tools/make_golden_short.py)
@pytest.mark.parametrize("name", ["short_high1", "short_high2", "short_cycle"])
def test_rounds_and_contigs_against_the_reference_goldens(name, tmp_path):
    """the reference's own mergeShortOverlap on the rows of rules (a) and (b): joins per round, its saved graph after every round, and the P_contig.fasta its
    printGraph wrote -- against the device, with no model in between"""
    import test_short_reference as R
    from test_scaffold_reference import unflagged
    rec = json.load(gzip.open(os.path.join(fx.GOLDEN, "short", name + ".json.gz"), "rt"))
    N, header, recs, pairs, high = R.golden_case(name)
    assert rec["high"] == high and sum(rec["joins"]) >= 1
    rng = np.random.default_rng(5)                                                     # the reads the goldens were made on (test_extend_reference.hand_store)
    reads = sorted({"".join(rng.choice(list("ACGT"), size=60)) for _ in range(N)}); assert len(reads) == N
    ctx = s2.Context(K); ctx.reads_add_ascii(np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(), np.arange(0, (N + 1) * 60, 60, dtype=np.uint64)); ctx.reads_organize()
    load_text(ctx, H.graph_text(header, recs), tmp_path); add_mates(ctx, pairs)
    for rd, (n, graph) in enumerate(zip(rec["joins"], rec["graphs"])):
        assert ctx.extend_short_round(high) == n and not ctx.extend_short_stats().last.outside_reference
        assert [[int(j[f]) for f in ("from", "to", "support", "gap")] for j in ctx.extend_short_merges()] == [list(x) for x in rec["merges"][rd]]
        assert unflagged(saved6(ctx, tmp_path, f"r{rd}.graph6")) == graph
    ctx.contigs_build(0, 0); out = str(tmp_path / "c.fasta"); ctx.contigs_save(out, 0)

    def records(text):                                                                 # as in tests/test_gpu_scaffold.py: the reference's sort leaves the order of edges of equal length open
        res = []
        for blk in text.split(">")[1:]:
            head, seq = blk.split("\n", 1); f = head.split(" gapCount=")
            res.append((f[0].split(" ", 1)[1], seq, f[1], int(f[0].split(" ", 1)[0].split("_")[1])))
        return res
    got, want = records(open(out).read()), records(rec["fasta"])
    assert sorted(x[:2] for x in got) == sorted(x[:2] for x in want) and got[-1][2] == want[-1][2] and len(want) >= 10
    # the sort key is the row's lengthOfEdge (include/sage2ov.h, ORDER of the contigs), which the record's name does not print: taken from the table, by the ordinal
    rows = ctx.contigs(); keys = [int(rows[x[3] - 1]["edge_length"]) for x in got]
    assert keys == sorted(keys, reverse=True)
    assert all(keys.count(keys[i]) > 1 for i in range(len(want)) if got[i][:2] != want[i][:2])      # only edges of equal length change places
    ctx.close()
