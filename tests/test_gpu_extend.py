"""GPU: the merge rounds of ContigExtender::extendContigs' first loop (sage2ov_graph_merge_pairs, sage2ov_extend_round, sage2ov_extend_by_supports,
sage2ov_graph6_save) against the restatement of tests/extend_model.py: the written graph, byte for byte, the merges of every round, the counts,
the rebuilt read-to-edge table and the insert bounds that must not move."""
import os
import subprocess
import numpy as np
import pytest
import fixtures as fx
import sage2_amd as s2
import compgen as CG
import extend_model as X
import test_mate_estimate_host as H
import test_mate_support_host as MS
from test_gpu_mate_estimate import add_mates, random_store, load_text

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("minimiser_groups_on")]
K = MS.HAND_K


def saved6(ctx, tmp_path, name="o.graph6"):
    p = str(tmp_path / name); ctx.graph6_save(p)
    return open(p).read()


def start(N, header, recs, pairs, tmp_path, seed=5):
    """a context with the graph loaded and the mates added, the model of the same text, and the header lines graph6_save keeps (those of graph5_save before a merge)"""
    text = H.graph_text(header, recs)
    ctx = random_store(N, seed); load_text(ctx, text, tmp_path)
    if pairs:
        add_mates(ctx, pairs)
    g = X.Graph(H.parse_graph(text))
    hdr = (ctx.genome_size(), ctx.copycount_stats().reads_present, header[2])
    assert saved6(ctx, tmp_path, "before.graph6") == g.text(hdr)                      # without a merge: graph5_save's text
    return ctx, g, hdr


def hand(flows=None, extra=None):
    N, header, recs, pairs = MS.hand_support_graph()
    for x, f in (flows or {}).items():
        recs[x]["flow"] = recs[x ^ 1]["flow"] = float(f)
    if extra:
        pairs = {1: pairs[1] + list(extra), 2: pairs[2]}
    return N, header, recs, pairs


def same_round(ctx, n, r):
    got = ctx.extend_merges()
    assert n == len(r["merges"]) == len(got)
    assert [tuple(v.item() for v in list(row)[:11]) for row in got] == X.merges_rows(r)
    st = ctx.extend_stats().last
    assert (st.entries, st.at_threshold, st.refused, st.blocked, st.merges) == (r["entries"], r["at_threshold"], r["refused"], r["blocked"], len(r["merges"]))
    assert st.batches == (1 if r["merges"] else 0) and st.pairs_deleted == sum(m["in_deleted"] + m["out_deleted"] for m in r["merges"])


def table_set(ctx):
    ent, loc, off = ctx.read_edges()
    return {(int(e["read"]), int(e["pair"]), tuple(int(v) for v in loc[e["location"]:e["location"] + e["n_forward"]]),
             tuple(int(v) for v in loc[e["location"] + e["n_forward"]:e["location"] + e["n_forward"] + e["n_reverse"]])) for e in ent}


@pytest.mark.parametrize("case,high,merges", [("plain", 2, [1, 1, 0]), ("plain", 4, [1, 0]), ("plain", 6, [0]), ("c_flow_2", 2, [1, 1, 0]), ("cb_2", 2, [0])])
def test_hand_built_graph_round_by_round(case, high, merges, tmp_path):
    N, header, recs, pairs = hand(flows={4: 2} if case == "c_flow_2" else None, extra=[(45, 1, 50, 1), (46, 0, 51, 1)] if case == "cb_2" else None)
    ctx, g, hdr = start(N, header, recs, pairs, tmp_path)
    b = X.Bounds(g, pairs)
    ctx.mates_estimate(); bounds = ctx.mates_bounds(); ins = [bytes(ctx.mates_insert(L)) for L in (1, 2)]
    assert bounds == (b.min_upper, b.max_upper)
    copied = 0
    for rd, want in enumerate(merges):
        r = X.round_(g, pairs, b, K, high)
        n = ctx.extend_round(high)
        assert n == want
        same_round(ctx, n, r)
        assert saved6(ctx, tmp_path, f"r{rd}.graph6") == g.text(hdr)
        assert np.array_equal(ctx.graph_flows(), g.flows())
        assert table_set(ctx) == X.read_edge_set(g)                                  # rebuilt from the merged graph
        assert ctx.mates_bounds() == bounds and [bytes(ctx.mates_insert(L)) for L in (1, 2)] == ins      # the estimate stands
        copied += sum(2 * len(g.h[-2 * (len(r["merges"]) - i)]["list"]) for i in range(len(r["merges"])))
    st = ctx.extend_stats()
    assert st.rounds == len(merges) and st.total.merges == sum(merges) and st.total.entries_copied == copied
    ctx.close()


def test_extend_by_supports_on_the_hand_built_graph(tmp_path, monkeypatch):
    N, header, recs, pairs = hand()
    ctx, g, hdr = start(N, header, recs, pairs, tmp_path)
    b = X.Bounds(g, pairs)
    gs = hdr[1] * header[2] // 6                                                    # coverage 6: highTh = ceil(0.2 * 6 * (100 / 60)) = 2
    assert X.threshold(hdr[1], header[2], gs) == 2 == s2.extend_threshold(hdr[1], header[2], gs)
    rs = X.extend(g, pairs, b, K, gs, hdr[1])
    assert ctx.extend_by_supports(gs) == (len(rs), sum(len(r["merges"]) for r in rs)) == (3, 2)
    want = g.text(hdr)
    assert saved6(ctx, tmp_path) == want
    assert ctx.extend_by_supports(gs) == (1, 0) and saved6(ctx, tmp_path) == want      # a fixed point
    # an explicit estimate on the merged graph replaces the one that stood
    ctx.mates_estimate()
    t, ests, bnd = MS.support_inputs(g.parsed(), pairs)
    assert ctx.mates_bounds() == bnd
    # memory-diet mode gives the same graph
    monkeypatch.setenv("SAGE2OV_MEMORY_DIET", "1")
    c2 = random_store(N, 5); load_text(c2, H.graph_text(header, recs), tmp_path, "d.graph4"); add_mates(c2, pairs)
    assert c2.extend_by_supports(gs) == (3, 2) and saved6(c2, tmp_path, "d.graph6") == want
    with pytest.raises(s2.Sage2ovError) as e:                                        # no genome size at all: the header's is what graph5_save writes, never 0 here; 0 reads
        s2.extend_threshold(hdr[1], 0, gs)
    assert e.value.code == -1
    ctx.close(); c2.close()


def operands(g, halves):
    """[(e1, e2)] of the model's pool -> the (pair ordinal, reversed) operand lists of merge_pairs, by the ordinals the model's graph has now"""
    where = {}
    for n, x in enumerate(g.save_order()):
        if x not in where:
            where[x] = (n, 0); where[x ^ 1] = (n, 1)
    return [where[a] for a, b in halves], [where[b] for a, b in halves]


CASES = [(0, 0, 1.0, 1.0, 1, 1), (1, 2, 2.0, 1.0, 1, 1), (0, 1, 1.0, 2.5, 2, 1), (1, 3, 0.0, 0.0, 1, 1), (2, 0, 0.0, 2.0, 1, 1), (3, 2, 3.0, 3.0, 0, 1), (2, 1, 1.0, 1.0, 1, 0),
         (3, 3, 2.0, 1.5, 1, 1), (0, 2, 1.0, 1.0, 1, 1), (3, 0, 1.0, 1.0, 1, 1), (1, 1, 1.0, 1.0, 1, 1), (0, 0, 0.0, 0.0, 0, 0)]


def chains():
    """disjoint two-edge chains 3 j + 1 -> 3 j + 2 -> 3 j + 3, one per case (e1 type, e2 type, flows, list lengths): all eight valid rows of combinedEdgeType, three
    invalid ones, flows 0, simple operands on either side and on both; then 61 -> 62 -> 61, whose merge is a loop, and 71 -> 72 -> 73 with a simple e1 of 3 000 bases.
    Chain j's edges are pool pairs 2 j and 2 j + 1"""
    recs = []; rid = 100
    ends = [(3 * j + 1, 3 * j + 2, 3 * j + 3) + c for j, c in enumerate(CASES)] + [(61, 62, 61, 0, 0, 1.0, 1.0, 1, 1), (71, 72, 73, 0, 0, 1.0, 1.0, 0, 1)]
    for j, (n1, n2, n3, t1, t2, f1, f2, c1, c2) in enumerate(ends):
        for (frm, to, t, f, n, ln) in ((n1, n2, t1, f1, c1, 3000 if n1 == 71 else 90 + j), (n2, n3, t2, f2, c2, 150 + j)):
            lst = [(rid + x, (x + j) % 2, 0, 10 + x + j, 20 + x + j) for x in range(n)]; rid += n
            r = H.rec(frm, to, t, ln, lst); tw = H.twin_of(r); r["flow"] = tw["flow"] = f; recs += [r, tw]
    return 200, (0, 400, 60), recs


def test_primitive_rows_flows_simple_edges_and_refusals(tmp_path):
    N, header, recs = chains()
    ctx, g, hdr = start(N, header, recs, None, tmp_path)
    nc = len(CASES); pairs_in_file = len(g.save_order())
    f, s_ = operands(g, [(4 * j, 4 * j + 2) for j in range(nc)])
    for tm in (3, 0):
        with pytest.raises(s2.Sage2ovError) as e:
            ctx.merge_pairs(f, s_, tm)
        assert e.value.code == -1
    for a, b in (([f[0], f[0]], [s_[0], s_[1]]), ([f[0], f[1]], [s_[0], s_[0]]),   # a pair named by two merges
                 ([(pairs_in_file, 0)], [s_[0]]), ([f[0]], [(pairs_in_file, 0)]),    # an ordinal beyond the pairs
                 ([f[0]], [s_[1]]), ([(f[0][0], 1)], [s_[0]])):                      # ends that do not meet
        with pytest.raises(s2.Sage2ovError) as e:
            ctx.merge_pairs(a, b)
        assert e.value.code == -1
    fl, sl = operands(g, [(4 * (nc + 1), 4 * (nc + 1) + 2)])
    with pytest.raises(s2.Sage2ovError) as e:                                        # the simple edge of 3 000 bases does not fit a list entry
        ctx.merge_pairs(f[:2] + fl, s_[:2] + sl)
    assert e.value.code == -5
    assert saved6(ctx, tmp_path) == g.text(hdr)                                      # nothing changed
    # two batches, type 1 for the even chains (and the loop-maker) and type 2 for the odd ones; the second batch is named by the ordinals after the first
    for tm, js in ((1, [j for j in range(nc) if j % 2 == 0] + [nc]), (2, [j for j in range(nc) if j % 2 == 1])):
        halves = [(4 * j, 4 * j + 2) for j in js]
        f, s_ = operands(g, halves)
        want = [0 if g.merge(a, b, tm) is None else 1 for a, b in halves]
        assert ctx.merge_pairs(f, s_, tm).tolist() == want == [int((CASES[j][0], CASES[j][1]) in X.COMBINED) if j < nc else 1 for j in js]
        assert saved6(ctx, tmp_path, f"t{tm}.graph6") == g.text(hdr)
        assert np.array_equal(ctx.graph_flows(), g.flows())
    # merges the reference refuses are no error: the loop with itself and with its twin, a merged edge with its own twin
    loop = next(x for x in range(len(g.h)) if g.alive[x >> 1] and g.h[x]["frm"] == g.h[x]["to"] == 61); new = len(g.h) - 2
    for a, b in ((loop, loop), (loop, loop ^ 1), (new, new ^ 1)):
        f, s_ = operands(g, [(a, b)])
        assert ctx.merge_pairs(f, s_).tolist() == [0] and g.merge(a, b) is None
    assert saved6(ctx, tmp_path, "t3.graph6") == g.text(hdr)
    assert ctx.simplify_stats().edges == sum(g.alive) and len(ctx.extend_merges()) == 0
    ctx.close()


def test_one_batch_with_simple_operands_on_either_side(tmp_path):
    """one batch whose merges have a simple e1, a simple e2, both and neither among composite ones: the middle entry takes its distances from the neighbouring
    list entry, or from the length of the operand that has no list"""
    N, header, recs = chains()
    ctx, g, hdr = start(N, header, recs, None, tmp_path)
    js = [5, 0, 6, 2, 11]
    assert {(CASES[j][4] > 0, CASES[j][5] > 0) for j in js} == {(False, True), (True, False), (False, False), (True, True)}
    halves = [(4 * j, 4 * j + 2) for j in js]
    f, s_ = operands(g, halves)
    want = [0 if g.merge(a, b) is None else 1 for a, b in halves]
    assert ctx.merge_pairs(f, s_).tolist() == want == [1] * len(js)
    assert saved6(ctx, tmp_path) == g.text(hdr) and np.array_equal(ctx.graph_flows(), g.flows())
    ctx.close()


def test_a_batch_of_many_blocks(tmp_path):
    """hundreds of merges in one batch (k_mg_plan and k_sp_commit on several blocks, thousands of list entries): one entering and one leaving half per node, no pair
    twice, whatever their types -- the refused ones stand among the merged ones"""
    N, header, recs = CG.case_a_pairs(1500)
    ctx, g, hdr = start(N, header, recs, None, tmp_path, seed=9)
    leaving = {}
    for x, h in enumerate(g.h):
        leaving.setdefault(h["frm"], []).append(x)
    used = set(); halves = []
    for node in sorted(leaving):
        out = [x for x in leaving[node] if x >> 1 not in used and g.h[x]["frm"] != g.h[x]["to"]]
        for a in out:
            b = next((y for y in out if y >> 1 != a >> 1 and y >> 1 not in used), None)
            if b is not None and a >> 1 not in used:
                halves.append((a ^ 1, b)); used |= {a >> 1, b >> 1}
    assert len(halves) > 2 * 256
    f, s_ = operands(g, halves)
    want = [0 if g.merge(a, b) is None else 1 for a, b in halves]
    assert 256 < sum(want) < len(want)
    assert ctx.merge_pairs(f, s_).tolist() == want
    assert saved6(ctx, tmp_path) == g.text(hdr) and np.array_equal(ctx.graph_flows(), g.flows())
    ctx.close()


@pytest.mark.parametrize("seed", [2, 3])
def test_generated_graph_with_hubs_round_by_round(seed, tmp_path):
    """about 200 pairs with a hub, loops, simple edges and reads on many pairs: rounds with refused and blocked entries and with ties at the threshold"""
    N, header, recs = CG.case_e(seed)
    parsed = H.parse_graph(H.graph_text(header, recs)); pairs = CG.mates_e(parsed, seed)
    ctx, g, hdr = start(N, header, recs, pairs, tmp_path, seed=9)
    b = X.Bounds(g, pairs)
    total = refused = blocked = 0
    for rd in range(20):
        r = X.round_(g, pairs, b, CG.K, 2)
        n = ctx.extend_round(2)
        same_round(ctx, n, r)
        assert saved6(ctx, tmp_path, f"r{rd}.graph6") == g.text(hdr)
        total += n; refused += r["refused"]; blocked += r["blocked"]
        if not n:
            break
    assert total >= 6 and refused and blocked and rd >= 1                            # (the model alone says so: not vacuous)
    assert table_set(ctx) == X.read_edge_set(g)
    assert ctx.mates_bounds() == (b.min_upper, b.max_upper)
    ctx.close()


def test_after_steps_1_to_4_with_flows_by_rule(tmp_path):
    """the graph step 4 left in HBM (pools with room to spare, no flows until they are handed in), not a loaded one: g4 with the golden cases' flows and mates.
    The model's pool is the written file's order, the device's is step 4's: within a node they agree, which is all the tie order and the file order ask"""
    name = "g4_highcopy_k21"; m = fx.golden(name); bases, off = fx.make_reads(m["synth"])
    ctx = s2.Context(m["k"]); ctx.reads_add_ascii(bases, off); ctx.reads_organize(); ctx.run_steps23(); ctx.graph_simplify()
    p4 = str(tmp_path / "s.graph4"); ctx.graph4_save(p4)
    parsed = MS.with_flows(H.parse_graph(open(p4).read()), MS.golden_flow)
    pairs = MS.golden_mates(parsed, ctx.reads_stats().unique_reads)
    g = X.Graph(parsed); b = X.Bounds(g, pairs)
    add_mates(ctx, pairs); ctx.graph_set_flows(g.flows())
    hdr = (ctx.genome_size(), ctx.copycount_stats().reads_present, parsed["header"][2])
    total = 0
    for rd in range(10):
        r = X.round_(g, pairs, b, m["k"], 3)
        n = ctx.extend_round(3)
        same_round(ctx, n, r)
        assert saved6(ctx, tmp_path, f"r{rd}.graph6") == g.text(hdr) and np.array_equal(ctx.graph_flows(), g.flows())
        total += n
        if not n:
            break
    assert total >= 10 and rd >= 1
    assert table_set(ctx) == X.read_edge_set(g)
    ctx.close()


def test_cli_extend_from_graph5(tmp_path):
    """sage2ov -m 6 --extend: P.reads + P.graph5 + the mates' file in, P.graph6 and P_contig.fasta out; the genome size is chosen so that highTh is 2"""
    N, header, recs, pairs = hand()
    ctx, g, hdr = start(N, header, recs, None, tmp_path)
    out = str(tmp_path / "out") + "/"; os.makedirs(out)
    ctx.reads_save(out + "t.reads"); ctx.graph5_save(out + "t.graph5")
    seqs = H.stored_reads(ctx)
    b_, o = H.mates_ascii(pairs[1], seqs); fa = str(tmp_path / "mates.fa")             # (-f is library 1 alone, main.cpp:240)
    open(fa, "w").write("".join(">m%d\n%s\n" % (i, b_[int(o[i]):int(o[i + 1])].tobytes().decode()) for i in range(len(o) - 1)))
    one = {1: pairs[1]}; b = X.Bounds(g, one)
    gs = hdr[1] * header[2] // 6
    rs = X.extend(g, one, b, K, gs, hdr[1])
    assert sum(len(r["merges"]) for r in rs) >= 1
    exe = os.path.join(fx.ROOT, "sage2_amd", "sage2ov")
    subprocess.run([exe, "-k", str(K), "-o", out, "-p", "u", "-i", "t", "-m", "6", "-f", fa, "--extend", "--contigs", "--genomeSize", str(gs)], check=True, stdout=subprocess.DEVNULL, timeout=120)
    assert open(out + "u.graph6").read() == g.text(hdr)
    log = open(out + "u.log").read()
    assert "Total number of extended contigs: %d\n" % sum(len(r["merges"]) for r in rs) in log and "Rounds of findMatepairSupports: %d " % len(rs) in log
    # the contigs are those of the merged graph: what a context that loads P.graph6 spells
    c2 = random_store(N, 5); c2.graph_load_composite(out + "u.graph6"); c2.contigs_build(0, gs); c2.contigs_save(str(tmp_path / "again.fasta"))
    assert open(out + "u_contig.fasta").read() == open(str(tmp_path / "again.fasta")).read() and os.path.getsize(out + "u_contig.fasta") > 0
    ctx.close(); c2.close()
