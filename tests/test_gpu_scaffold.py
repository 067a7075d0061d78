"""GPU: step 7 (sage2ov_graph_join_pairs, sage2ov_scaffold_round, sage2ov_scaffold, `sage2ov -m 7 --scaffold`) against the restatement of
tests/scaffold_model.py: the overlap search of every join, the written graph byte for byte, the joins and counts of every round, the flows, the rebuilt
read-to-edge table, the insert bounds that must not move, and the scaffolds' N runs."""
import os
import subprocess
import numpy as np
import pytest
import fixtures as fx
import sage2_amd as s2
import scaffold_model as SM
import extend_model as X
import test_mate_estimate_host as H
import test_links_host as LH
import test_scaffold_host as SH
from test_gpu_mate_estimate import add_mates, random_store, load_text
from test_gpu_extend import saved6, operands, table_set
from test_scaffold_host import components, pinned_cases, pinned_cases_long, distinct

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("minimiser_groups_on")]
K = LH.HAND_K


def chosen_store(strings, k=10):
    """a context whose read set is exactly these reads (distinct, also against each other's reverse complements) -> (ctx, {id: stored read}, {spelling: (id, stored
    as spelled)})"""
    reads = sorted(set(strings))
    bases = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(); off = np.zeros(len(reads) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(r) for r in reads])
    ctx = s2.Context(k); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
    assert ctx.reads_stats().unique_reads == len(reads)
    seqs = H.stored_reads(ctx); where = {}
    for i, s in seqs.items():
        where[SM.revcomp(s)] = (i, False)
    for i, s in seqs.items():
        where[s] = (i, True)
    return ctx, seqs, where


def loaded(ctx, header, recs, tmp_path):
    text = H.graph_text(header, recs); load_text(ctx, text, tmp_path)
    g = SM.Graph(H.parse_graph(text))
    hdr = (ctx.genome_size(), ctx.copycount_stats().reads_present, header[2])
    assert saved6(ctx, tmp_path, "before.graph6") == g.text(hdr)
    return g, hdr


def join_both(ctx, g, seqs, halves, gaps):
    """the batch on the device and, join by join, on the model -> (device (overlap, how), model (overlap, how))"""
    f, s_ = operands(g, halves)
    ov, how = ctx.join_pairs(f, s_, gaps)
    mo, mh = [], []
    for (a, b), gap in zip(halves, gaps):
        g.join(a, b, gap, seqs); mo.append(list(g.last["overlap"])); mh.append(list(g.last["how"]))
    return (ov.tolist(), how.tolist()), (mo, mh)


def test_overlap_search_on_every_pinned_case(tmp_path):
    cases = pinned_cases(); strings = distinct(cases)
    fillers = [SH.rnd(60, 5000 + i) for i in range(5 * len(cases))]
    ctx, seqs, where = chosen_store(list(strings) + fillers)
    recs = components([(s1, s2_, 1, 1, n) for n, (s1, s2_, _) in enumerate(cases)], where, [where[x][0] for x in fillers])
    g, hdr = loaded(ctx, (0, 400, 60), recs, tmp_path)
    halves = [(4 * n, 4 * n + 2) for n in range(len(cases))]; gaps = [(-3, 0, 5, 2000)[n % 4] for n in range(len(cases))]
    (ov, how), (mo, mh) = join_both(ctx, g, seqs, halves, gaps)
    assert [o[0] for o in mo] == [want for _, _, want in cases]                        # the model's forward search is the pinned value
    assert ov == mo and how == mh
    assert {h for hw in how for h in hw} == {SM.OVERLAP, SM.CONCAT, SM.GAPPED} and any(o[0] != o[1] for o in ov)
    assert saved6(ctx, tmp_path) == g.text(hdr) and np.array_equal(ctx.graph_flows(), g.flows())
    ctx.close()


def test_a_seeded_batch_of_512_searches_with_mixed_lengths(tmp_path):
    rng = np.random.default_rng(17); cases = []
    for n in range(256):
        L1, L2 = (int(v) for v in rng.integers(11, 151, size=2))
        s2_ = SH.rnd(L2, 7000 + n)
        kind = n % 4
        if kind == 0 or L1 < 13:
            s1 = SH.rnd(L1, 8000 + n)
        else:
            sh = int(rng.integers(0, L1 - 10)); body = list((s2_ + SH.rnd(L1, 9000 + n))[:L1])
            for x in rng.integers(0, max(1, min(L1 - sh, L2)), size=kind - 1):         # 0, 1 or 2 mismatches in the part that faces s2
                body[int(x)] = SH.other(body[int(x)])
            s1 = (SH.rnd(sh, 9500 + n) + "".join(body))[:L1]
        cases.append((s1, s2_, None))
    strings = distinct(cases)
    fillers = [SH.rnd(60, 5000 + i) for i in range(5 * len(cases))]
    ctx, seqs, where = chosen_store(list(strings) + fillers)
    recs = components([(s1, s2_, 1 + n % 3, (n % 5) / 2, n) for n, (s1, s2_, _) in enumerate(cases)], where, [where[x][0] for x in fillers])
    g, hdr = loaded(ctx, (0, 400, 60), recs, tmp_path)
    halves = [(4 * n, 4 * n + 2) for n in range(len(cases))]; gaps = [int(v) for v in rng.integers(-50, 300, size=len(cases))]
    (ov, how), (mo, mh) = join_both(ctx, g, seqs, halves, gaps)
    assert ov == mo and how == mh
    found = [o for pair in ov for o in pair]
    assert sum(o > 0 for o in found) > 100 and sum(o == -1 for o in found) > 20 and sum(o > 63 for o in found) > 5      # (the model alone says so: not vacuous)
    assert saved6(ctx, tmp_path) == g.text(hdr) and np.array_equal(ctx.graph_flows(), g.flows())
    ctx.close()


# ------------------------------------------------------------------------------------------ the 16- and 32-word read layouts (252 to 504 and 505 to 1018 bases)
LONG_WORDS = {504: 16, 1018: 32}
LONG_GAPS = (-3, 0, 5, 1030, 2000)
# (case, gap, read length, edge length, distance in the entry) of one join without an overlap per layout whose gap + L passes 2047: 1030 + 1018 = 2048 is 0 in the
# entry's 11 bits, 2000 + 503 = 2503 is 455; X has 300 + n % 7 bases and Y 250 + n % 5 (components)
LONG_WRAP = {504: (29, 2000, 503, 301 + 254 + 2503, 455), 1018: (43, 1030, 1018, 301 + 253 + 2048, 0)}


def found_in(ov):
    return [o for pair in ov for o in pair]


@pytest.mark.parametrize("top", sorted(LONG_WORDS))
def test_overlap_search_on_the_long_layouts(top, tmp_path):
    """every long pinned case of a layout (tests/test_scaffold_host.py: the middle, the last and the first shift at the word and layout edges, several passing lane
    rounds, unequal lengths) in one store with 60-base fillers, all four type combinations, gaps that wrap the entry's 11 bits"""
    cases = pinned_cases_long(top=top); strings = distinct(cases); nc = len(cases)
    fillers = [SH.rnd(60, 5000 + i) for i in range(5 * nc)]
    ctx, seqs, where = chosen_store(list(strings) + fillers)
    st = ctx.reads_stats(); assert (st.words_per_read, st.max_read_length) == (LONG_WORDS[top], top)
    recs = components([(s1, s2_, 1, 1, n) for n, (s1, s2_, _) in enumerate(cases)], where, [where[x][0] for x in fillers])
    g, hdr = loaded(ctx, (0, 400, 60), recs, tmp_path)
    halves = [(4 * n, 4 * n + 2) for n in range(nc)]; gaps = [LONG_GAPS[n % 5] for n in range(nc)]
    (ov, how), (mo, mh) = join_both(ctx, g, seqs, halves, gaps)
    assert [o[0] for o in mo] == [want for _, _, want in cases]                        # the model's forward search is the pinned value
    assert ov == mo and how == mh
    # (the model alone says so: not vacuous) a hit in the layout's last word of 32 shifts, directions that differ, every distance case
    assert any(o >= 32 * (LONG_WORDS[top] - 1) for o in found_in(mo)) and (top != 1018 or any(o >= 960 for o in found_in(mo)))
    assert any(o[0] != o[1] for o in mo) and {h for hw in mh for h in hw} == {SM.OVERLAP, SM.CONCAT, SM.GAPPED}
    n, gap, L, length, entry = LONG_WRAP[top]; new = g.h[len(g.h) - 2 * (nc - n)]
    assert (gaps[n], len(cases[n][0]), len(cases[n][1]), mo[n], mh[n]) == (gap, L, L, [-1, -1], [SM.GAPPED, SM.GAPPED])
    assert new["len"] == length and gap + L > 2047 and new["list"][2][4] == new["list"][3][3] == entry == (gap + L) & 0x7FF      # the wrap is in the entry only
    assert saved6(ctx, tmp_path) == g.text(hdr) and np.array_equal(ctx.graph_flows(), g.flows())
    ctx.close()


@pytest.mark.parametrize("top", sorted(LONG_WORDS))
def test_a_seeded_batch_on_the_long_layouts(top, tmp_path):
    """128 joins, 256 searches: reads of more than half the layout's longest, a quarter of the second reads of 11 to 150 bases, planted shifts in every lane round"""
    rng = np.random.default_rng(19 + top); cases = SH.long_batch(top); strings = distinct(cases); nc = len(cases)
    fillers = [SH.rnd(60, 5000 + i) for i in range(5 * nc)]
    ctx, seqs, where = chosen_store(list(strings) + fillers)
    st = ctx.reads_stats(); assert st.words_per_read == LONG_WORDS[top] and top - 28 <= st.max_read_length == max(len(s) for s in strings) <= top
    recs = components([(s1, s2_, 1 + n % 3, (n % 5) / 2, n) for n, (s1, s2_, _) in enumerate(cases)], where, [where[x][0] for x in fillers])
    g, hdr = loaded(ctx, (0, 400, 60), recs, tmp_path)
    halves = [(4 * n, 4 * n + 2) for n in range(nc)]; gaps = [int(v) for v in rng.integers(-50, 2100, size=nc)]
    (ov, how), (mo, mh) = join_both(ctx, g, seqs, halves, gaps)
    assert nc == 128 and SH.batch_conditions(top, found_in(mo))                        # (the model alone says so: not vacuous)
    assert ov == mo and how == mh
    assert saved6(ctx, tmp_path) == g.text(hdr) and np.array_equal(ctx.graph_flows(), g.flows())
    ctx.close()


def on_the_locality_route(ctx, seqs, diet):
    """memory-diet mode releases the id-ordered store in the index build and nowhere else: with `diet` the index is built, and one id looked up shows which store
    a reader finds (tests/test_gpu_contigs.py) -> whether the locality-ordered one"""
    if diet:
        ctx.index_build()
    q = np.frombuffer(seqs[1].encode(), dtype=np.uint8)
    assert ctx.reads_find_ids(q, np.array([0, len(q)], dtype=np.uint64)).tolist() == [1]
    return ctx.reads_find_stats().route == s2.FIND_ROUTE_LOCALITY


def uniform_long_cases():
    """1018 bases throughout: shifts in the first word, on either side of a word and of half the read, in the last lane round and the last one of all, each with the
    allowed mismatches or fewer; and a pair without an overlap"""
    out = []
    for n, (shift, mism) in enumerate([(1, 102), (31, 50), (32, 0), (511, 51), (512, 3), (960, 6), (1007, 2)]):
        s1, s2_ = SH.planted(1018, 1018, shift, mism, 600 + n); out.append((s1, s2_, shift))
    return out + [(SH.rnd(1018, 700), SH.rnd(1018, 701), -1)]


@pytest.mark.parametrize("diet", [0, 1])
def test_uniform_long_reads_on_both_store_routes(diet, tmp_path, monkeypatch):
    """every read has 1018 bases: no length is read out of a slot, and the last word's bits below the bases are zero.  With SAGE2OV_MEMORY_DIET and an index built
    the id-ordered store is gone: the search reads the locality-ordered one through posOf"""
    if diet:
        monkeypatch.setenv("SAGE2OV_MEMORY_DIET", "1")
    else:
        monkeypatch.delenv("SAGE2OV_MEMORY_DIET", raising=False)
    cases = uniform_long_cases(); strings = distinct(cases); nc = len(cases)
    fillers = [SH.rnd(1018, 5000 + i) for i in range(5 * nc)]
    ctx, seqs, where = chosen_store(list(strings) + fillers, k=40)
    st = ctx.reads_stats(); assert (st.words_per_read, st.max_read_length, {len(s) for s in seqs.values()}) == (32, 1018, {1018})
    assert on_the_locality_route(ctx, seqs, diet) == bool(diet)                        # before the join: which store it will read
    recs = components([(s1, s2_, (1, 2, 0.5)[n % 3], (3, 1)[n % 2], n) for n, (s1, s2_, _) in enumerate(cases)], where, [where[x][0] for x in fillers])
    g, hdr = loaded(ctx, (0, 400, 60), recs, tmp_path)
    halves = [(4 * n, 4 * n + 2) for n in range(nc)]; gaps = [0, -1, 7, 1990, 3, 1030, 12, 5]
    (ov, how), (mo, mh) = join_both(ctx, g, seqs, halves, gaps)
    assert [o[0] for o in mo] == [want for _, _, want in cases] == [1, 31, 32, 511, 512, 960, 1007, -1]
    assert ov == mo and how == mh
    assert saved6(ctx, tmp_path) == g.text(hdr) and np.array_equal(ctx.graph_flows(), g.flows())
    ctx.close()


def uniform_cases():
    out = []
    for n, (shift, mism) in enumerate([(1, 6), (1, 7), (25, 4), (25, 5), (49, 2), (49, 3), (0, 7), (30, 0)]):
        s1, s2_ = SH.planted(60, 60, shift, mism, 300 + n); out.append((s1, s2_, None))
    return out


@pytest.mark.parametrize("diet", [0, 1])
def test_both_store_routes_and_the_distance_cases(diet, tmp_path, monkeypatch):
    """reads of one length: with SAGE2OV_MEMORY_DIET and an index built the id-ordered store is gone and the search reads the locality-ordered one through posOf
    (reads_organize alone releases nothing: the route is asserted).  Also equal end nodes, the 11-bit wrap, kept operands, and the argument errors that leave
    everything as it was"""
    if diet:
        monkeypatch.setenv("SAGE2OV_MEMORY_DIET", "1")
    else:
        monkeypatch.delenv("SAGE2OV_MEMORY_DIET", raising=False)
    cases = uniform_cases(); strings = distinct(cases)
    fillers = [SH.rnd(60, 5000 + i) for i in range(5 * len(cases) + 12)]
    ctx, seqs, where = chosen_store(list(strings) + fillers, k=40)
    assert ctx.reads_stats().words_per_read == 4
    assert on_the_locality_route(ctx, seqs, diet) == bool(diet)                        # before the joins: which store they will read
    fid = [where[x][0] for x in fillers]
    recs = components([(s1, s2_, (1, 2, 0.5)[n % 3], (3, 1)[n % 2], n) for n, (s1, s2_, _) in enumerate(cases)], where, fid)
    nc = len(cases)
    # two edges that meet in a node (one entry), and a simple edge
    eq1 = H.rec(fid[-1], fid[-2], 3, 90, [(fid[-3], 1, 0, 20, 70)]); eq2 = H.rec(fid[-2], fid[-4], 3, 80, [(fid[-5], 0, 0, 11, 69)]); simple = H.rec(fid[-6], fid[-7], 3, 40, [])
    for r in (eq1, eq2, simple):
        t = H.twin_of(r); r["flow"] = t["flow"] = 1.0; recs += [r, t]
    g, hdr = loaded(ctx, (0, 400, 60), recs, tmp_path)
    f, s_ = operands(g, [(4 * n, 4 * n + 2) for n in range(nc)] + [(4 * nc, 4 * nc + 2)])
    pairs_in_file = len(g.save_order()); simple_op = operands(g, [(4 * nc + 4, 0)])[0][0]
    for a, b, gp in (([f[0], f[0]], [s_[0], s_[1]], [1, 1]), ([f[0], f[1]], [s_[0], s_[0]], [1, 1]), ([f[0]], [(f[0][0], 1)], [1]),      # a pair named twice
                     ([(pairs_in_file, 0)], [s_[0]], [1]), ([f[0]], [(pairs_in_file, 0)], [1]),                                          # an ordinal beyond the pairs
                     ([simple_op], [s_[0]], [1]), ([f[0]], [simple_op], [1])):                                                           # an operand without a list
        with pytest.raises(s2.Sage2ovError) as e:
            ctx.join_pairs(a, b, gp)
        assert e.value.code == -1
    assert saved6(ctx, tmp_path) == g.text(hdr)                                        # nothing changed
    halves = [(4 * n, 4 * n + 2) for n in range(nc)] + [(4 * nc, 4 * nc + 2)]; gaps = [0, -1, 7, 1990, 3, 2047, 12, 5, 33]
    (ov, how), (mo, mh) = join_both(ctx, g, seqs, halves, gaps)
    assert ov == mo and how == mh and ov[-1] == [-2, -2] and how[-1] == [SM.EQUAL, SM.EQUAL]
    assert [o[0] for o in ov[:nc]] == [1, -1, 25, -1, 49, -1, 0, 30]
    assert g.h[-2 * (nc + 1) + 2 * 3]["len"] == 303 + 253 + 1990 + 60                   # the wrap is in the entry only
    assert saved6(ctx, tmp_path) == g.text(hdr) and np.array_equal(ctx.graph_flows(), g.flows())
    ctx.close()


def test_a_batch_that_crosses_a_pool_reallocation_and_ordinals_in_save_order(tmp_path):
    """a loaded graph's pools have no room to spare: 300 joins grow every pool; the second batch is named by the ordinals after the first"""
    cases = [(SH.rnd(60, 20000 + 2 * n), SH.rnd(60, 20001 + 2 * n), None) for n in range(300)]; strings = distinct(cases)
    fillers = [SH.rnd(60, 5000 + i) for i in range(5 * len(cases))]
    ctx, seqs, where = chosen_store(list(strings) + fillers, k=40)
    recs = components([(s1, s2_, 2, 2, n) for n, (s1, s2_, _) in enumerate(cases)], where, [where[x][0] for x in fillers])
    g, hdr = loaded(ctx, (0, 400, 60), recs, tmp_path)
    halves = [(4 * n, 4 * n + 2) for n in range(300)]
    (ov, how), (mo, mh) = join_both(ctx, g, seqs, halves, [n - 20 for n in range(300)])
    assert ov == mo and how == mh and saved6(ctx, tmp_path, "a.graph6") == g.text(hdr)
    new = [len(g.h) - 2 * (300 - n) for n in range(300)]                               # the kept operands (flow 2 -> 1) are joined again, and new edges with new edges
    halves2 = [(4 * n + 3, 4 * n + 1) for n in range(0, 300, 3)] + [(new[n], new[n + 1] ^ 1) for n in range(1, 299, 3)]
    (ov, how), (mo, mh) = join_both(ctx, g, seqs, halves2, [3] * len(halves2))
    assert ov == mo and how == mh and saved6(ctx, tmp_path, "b.graph6") == g.text(hdr) and np.array_equal(ctx.graph_flows(), g.flows())
    ctx.close()


def test_merges_then_joins_on_one_graph_whose_flows_are_all_zero(tmp_path):
    """a batch of merges, one of them refused (the rank of a new pair is not its index), then a batch of joins on the same context: an operand the merges made,
    equal end nodes (one middle entry on the join path), a negative and a positive gap.  Every flow is 0: the merged edges have 0, the joined ones 1.0, and every
    operand goes"""
    cases = uniform_cases() + [(SH.rnd(60, 30000 + 2 * n), SH.rnd(60, 30001 + 2 * n), None) for n in range(4)]; strings = distinct(cases)
    nc = len(cases); fillers = [SH.rnd(60, 5000 + i) for i in range(5 * nc + 25)]
    ctx, seqs, where = chosen_store(list(strings) + fillers, k=40)
    fid = [where[x][0] for x in fillers]
    recs = components([(s1, s2_, 0, 0, n) for n, (s1, s2_, _) in enumerate(cases)], where, fid)
    # five chains u -> v -> w of two composite edges that meet in v: pool halves 4 nc + 4 j (into v) and 4 nc + 4 j + 2 (out of v); (3, 0) is no row of combinedEdgeType
    for j, (t1, t2) in enumerate([(3, 3), (3, 0), (0, 1), (2, 0), (3, 3)]):
        u, v, w, r1, r2 = fid[5 * nc + 5 * j:5 * nc + 5 * j + 5]
        for r in (H.rec(u, v, t1, 90 + j, [(r1, 1, 0, 20, 70 + j)]), H.rec(v, w, t2, 80 + j, [(r2, 0, 0, 11, 69 + j)])):
            recs += [r, H.twin_of(r)]
    g, hdr = loaded(ctx, (0, 400, 60), recs, tmp_path)
    assert not ctx.graph_flows().any()
    chain = [(4 * nc + 4 * j, 4 * nc + 4 * j + 2) for j in range(5)]
    f, s_ = operands(g, chain[:4])
    want = [0 if g.merge(a, b) is None else 1 for a, b in chain[:4]]
    assert ctx.merge_pairs(f, s_).tolist() == want == [1, 0, 1, 1]
    assert not ctx.graph_flows().any() and saved6(ctx, tmp_path, "a.graph6") == g.text(hdr)
    made = len(g.h) - 6                                                               # the pair of chain 0; chain 2's is the second new pair, not the third
    assert g.h[made + 2]["frm"] == g.h[chain[2][0]]["frm"] and g.h[made + 2]["to"] == g.h[chain[2][1]]["to"]
    halves = [(made, 4 * 5), chain[4], (4 * 1, 4 * 1 + 2), (4 * 3, 4 * 3 + 2)]; gaps = [0, 3, -1, 12]
    (ov, how), (mo, mh) = join_both(ctx, g, seqs, halves, gaps)
    assert ov == mo and how == mh
    assert ov[1] == [-2, -2] and how[1] == [SM.EQUAL, SM.EQUAL] and (ov[2][0], how[2][0]) == (-1, SM.CONCAT) and (ov[3][0], how[3][0]) == (-1, SM.GAPPED)
    assert saved6(ctx, tmp_path, "b.graph6") == g.text(hdr)
    fl = ctx.graph_flows()
    assert np.array_equal(fl, g.flows()) and set(fl.tolist()) == {0.0, 1.0} and fl.sum() == 8.0 and all(h["flow"] == 1.0 for h in g.h[-8:])
    assert not any(g.alive[e >> 1] for ab in halves for e in ab) and ctx.simplify_stats().edges == sum(g.alive)
    ctx.close()


# ------------------------------------------------------------------------------------------ rounds
def hand_start(tmp_path, seed=5, name="h.graph4", **kw):
    N, header, recs, pairs, _ = SH.hand(**kw)
    ctx = random_store(N, seed); g, hdr = loaded(ctx, header, recs, tmp_path)
    add_mates(ctx, pairs)
    return ctx, g, hdr, pairs, H.stored_reads(ctx)


def same_round(ctx, n, r):
    got = ctx.scaffold_merges()
    assert n == len(r["merges"]) == len(got)
    assert [tuple(v.item() for v in list(row)[:14]) for row in got] == SM.joins_rows(r)
    st = ctx.scaffold_stats().last
    assert (st.rows, st.below_threshold, st.skipped, st.blocked, st.cycles, st.merged, st.batches) == (r["rows"], r["below_threshold"], r["skipped"], r["blocked"], r["cycles"], len(r["merges"]), r["batches"])
    assert (st.overlaps, st.concatenated, st.gapped, st.outside_reference) == (r["overlaps"], r["concatenated"], r["gapped"], int(r["outside_reference"]))
    assert st.pairs_deleted == sum(m["first_deleted"] + m["second_deleted"] for m in r["merges"])


KEPT = {q: 50 for q in range(13)}      # every pair kept however often a round names it: a kept operand named again (two and three batches), a row the pointer identity decides


@pytest.mark.parametrize("high,flag,small,first,flows", [(2, 1, False, 1, None), (1, 1, False, 1, None), (1, 2, False, 3, None), (1, 2, True, 3, None), (6, 2, False, 0, None),
                                                         (1, 2, False, 4, KEPT), (1, 1, False, 1, KEPT), (1, 2, True, 4, KEPT),
                                                         (1, 2, False, 2, SH.CYCLE), (1, 1, False, 1, SH.CYCLE)])      # the hand-built cycle: 4 cycles, under flag 1 two blocked rows as well
def test_hand_built_graph_round_by_round(high, flag, small, first, flows, tmp_path):
    ctx, g, hdr, pairs, seqs = hand_start(tmp_path, **(flows if flows is SH.CYCLE else dict(flows=flows)))
    b = X.Bounds(g, pairs)
    ctx.mates_estimate(); bounds = ctx.mates_bounds(); ins = [bytes(ctx.mates_insert(L)) for L in (1, 2)]
    assert bounds == (b.min_upper, b.max_upper)
    for rd in range(14):
        r = SM.round_(g, pairs, b, K, high, flag, small, seqs)
        n = ctx.scaffold_round(high, flag, small)
        if rd == 0:
            assert n == first
        same_round(ctx, n, r)
        assert saved6(ctx, tmp_path, f"r{rd}.graph6") == g.text(hdr)
        assert np.array_equal(ctx.graph_flows(), g.flows())
        assert table_set(ctx) == X.read_edge_set(g)
        assert ctx.mates_bounds() == bounds and [bytes(ctx.mates_insert(L)) for L in (1, 2)] == ins      # the estimate stands
        if not n:
            break
    assert not n and ctx.scaffold_stats().rounds == rd + 1
    ctx.close()


@pytest.mark.parametrize("seed,high,flag,small", [(2, 2, 1, False), (2, 1, 2, False), (3, 1, 2, True)])
def test_generated_graph_with_hubs_round_by_round(seed, high, flag, small, tmp_path):
    """about 200 pairs with a hub, loops and reads on many pairs, mates at the nodes and long-range ones: rounds with ties, blocked rows, cycles, rows that name a
    spent or a deleted operand, and a kept operand named again, so that a round goes to the device in more than one batch"""
    import compgen as CG
    N, header, recs = CG.case_e(seed)
    parsed = H.parse_graph(H.graph_text(header, recs)); pairs = LH.merged(CG.mates_e(parsed, seed), LH.long_range_mates(parsed))
    ctx = random_store(N, 9); g, hdr = loaded(ctx, header, recs, tmp_path)
    add_mates(ctx, pairs); seqs = H.stored_reads(ctx)
    b = X.Bounds(g, pairs)
    total = blocked = cycles = 0; most = 0
    for rd in range(4):
        r = SM.round_(g, pairs, b, CG.K, high, flag, small, seqs)
        n = ctx.scaffold_round(high, flag, small)
        same_round(ctx, n, r)
        assert saved6(ctx, tmp_path, f"r{rd}.graph6") == g.text(hdr) and np.array_equal(ctx.graph_flows(), g.flows())
        total += n; blocked += r["blocked"]; cycles += r["cycles"]; most = max(most, r["batches"])
        if not n:
            break
    assert total >= 10 and blocked and cycles and most >= (2 if (seed, flag) != (3, 2) else 1)      # (the model alone says so: not vacuous)
    assert table_set(ctx) == X.read_edge_set(g) and ctx.mates_bounds() == (b.min_upper, b.max_upper)
    ctx.close()


def test_scaffold_as_a_whole_and_the_scaffolds_it_spells(tmp_path):
    ctx, g, hdr, pairs, seqs = hand_start(tmp_path)
    b = X.Bounds(g, pairs)
    gs = hdr[1] * hdr[2] // 6                                                        # coverage 6 at read length 60: T(0.10) = T(0.05) = 1
    assert s2.scaffold_threshold(hdr[1], hdr[2], gs, 1, 1) == 1 == SM.threshold(hdr[1], hdr[2], gs, 1, 6)
    rs = SM.scaffold(g, pairs, b, K, gs, hdr[1], seqs)
    joined = sum(len(r["merges"]) for _, _, r in rs)
    assert ctx.scaffold(gs) == (len(rs), joined) and joined >= 3
    want = g.text(hdr)
    assert saved6(ctx, tmp_path) == want
    tot = ctx.scaffold_stats().total
    assert tot.gapped == sum(r["gapped"] for _, _, r in rs) > 0 and tot.batches == sum(r["batches"] for _, _, r in rs)
    # the scaffolds: every join with a gap stands as a run of N in the string of its edge, as long as the gap
    ctx.contigs_build(0, gs); out = str(tmp_path / "s.fasta"); ctx.contigs_save(out, 1)
    text = open(out).read(); rows = ctx.contigs()
    assert text.startswith(">scaffold_1 ") and sum(int(r["n_count"]) for r in rows) > 0
    gaps = {(m["frm"], m["to"]): m["gap"] for _, _, r in rs for m in r["merges"] if m["how"][0] == SM.GAPPED and m["gap"] > 0}
    assert gaps
    lens = {i: len(s) for i, s in seqs.items()}
    ns = lambda x: sum(dp - lens[i] for (i, o, f, dp, dn) in g.h[x]["list"] if dp > lens[i])      # overlapGraph.cpp:666-669
    for row in rows:
        cands = [x for x in range(len(g.h)) if g.alive[x >> 1] and g.h[x]["frm"] == int(row["from"]) and g.h[x]["to"] == int(row["to"]) and g.h[x]["len"] == int(row["edge_length"])]
        assert cands and int(row["n_count"]) in {ns(x) for x in cands}
    assert "N" * min(gaps.values()) in text.replace("\n", "")
    rs2 = SM.scaffold(g, pairs, b, K, gs, hdr[1], seqs)                                # once more, on the scaffolded graph
    assert ctx.scaffold(gs) == (len(rs2), sum(len(r["merges"]) for _, _, r in rs2)) and saved6(ctx, tmp_path, "again.graph6") == g.text(hdr)
    ctx.close()


def test_cli_scaffold_from_graph6(tmp_path):
    """sage2ov -m 7 --scaffold: P.reads + P.graph6 + the mates' file in, P_scaffold.fasta out, against a context that does the same by calls"""
    ctx, g, hdr, pairs, seqs = hand_start(tmp_path)
    out = str(tmp_path / "out") + "/"; os.makedirs(out)
    ctx.reads_save(out + "t.reads"); ctx.graph6_save(out + "t.graph6")
    b_, o = H.mates_ascii(pairs[1], seqs); fa = str(tmp_path / "mates.fa")             # (-f is library 1 alone, main.cpp:282)
    open(fa, "w").write("".join(">m%d\n%s\n" % (i, b_[int(o[i]):int(o[i + 1])].tobytes().decode()) for i in range(len(o) - 1)))
    gs = hdr[1] * hdr[2] // 6
    exe = os.path.join(fx.ROOT, "sage2_amd", "sage2ov")
    subprocess.run([exe, "-k", str(K), "-o", out, "-p", "u", "-i", "t", "-m", "7", "-f", fa, "--scaffold", "--genomeSize", str(gs)], check=True, stdout=subprocess.DEVNULL, timeout=120)
    c2 = random_store(len(seqs), 5); c2.graph_load_composite(out + "t.graph6"); add_mates(c2, {1: pairs[1]})
    c2.mates_estimate(); rounds, joined = c2.scaffold(gs)
    c2.contigs_build(0, gs); c2.contigs_save(str(tmp_path / "calls.fasta"), 1)
    assert open(out + "u_scaffold.fasta").read() == open(str(tmp_path / "calls.fasta")).read() and os.path.getsize(out + "u_scaffold.fasta") > 0
    log = open(out + "u.log").read()
    assert "Total number of merged scaffolds: %d\n" % joined in log and "Rounds of mergeFinal: %d " % rounds in log and joined >= 1
    ctx.close(); c2.close()


# ------------------------------------------------------------------------------------------ what the reference itself did (tests/golden/scaffold/, tools/make_golden_scaffold.py)
@pytest.mark.parametrize("name", ["hand_flag1", "hand_flag2", "hand_small"])
def test_rounds_and_scaffolds_against_the_reference_goldens(name, tmp_path):
    """the reference's own mergeAccordingToSupport* on the rows of rules (a) and (b): joins per round, its saved graph after every round, and the P_scaffold.fasta its
    printGraph(.., true) wrote -- against the device, with no model in between"""
    import gzip, json
    import test_scaffold_reference as R
    rec = json.load(gzip.open(os.path.join(fx.GOLDEN, "scaffold", name + ".json.gz"), "rt"))
    N, header, recs, pairs, high, flag, small = R.golden_case(name)
    assert (rec["high"], rec["flag"], rec["small"]) == (high, flag, small) and sum(rec["joins"]) >= 1
    rng = np.random.default_rng(5)                                                     # the reads the goldens were made on (test_extend_reference.hand_store)
    reads = sorted({"".join(rng.choice(list("ACGT"), size=60)) for _ in range(N)}); assert len(reads) == N
    ctx = s2.Context(K); ctx.reads_add_ascii(np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(), np.arange(0, (N + 1) * 60, 60, dtype=np.uint64)); ctx.reads_organize()
    load_text(ctx, H.graph_text(header, recs), tmp_path); add_mates(ctx, pairs)
    for rd, (n, graph) in enumerate(zip(rec["joins"], rec["graphs"])):
        assert ctx.scaffold_round(high, flag, small) == n and not ctx.scaffold_stats().last.outside_reference
        assert [[int(j[f]) for f in ("from", "to", "support", "gap")] for j in ctx.scaffold_merges()] == [list(x) for x in rec["merges"][rd]]
        assert R.unflagged(saved6(ctx, tmp_path, f"r{rd}.graph6")) == graph
    ctx.contigs_build(0, 0); out = str(tmp_path / "s.fasta"); ctx.contigs_save(out, 1)
    # the reference's sort leaves the order of edges of equal length open (include/sage2ov.h, ORDER of the contigs; the hand graph has two of 200 bases): the records
    # are compared without their ordinal and running counters, the totals of the last record with them, and the whole file byte for byte where no length is shared
    def records(text):
        out = []
        for blk in text.split(">")[1:]:
            head, seq = blk.split("\n", 1); f = head.split(" gapCount=")
            out.append((f[0].split(" ", 1)[1], seq, f[1]))
        return out
    got, want = records(open(out).read()), records(rec["fasta"])
    assert sorted(x[:2] for x in got) == sorted(x[:2] for x in want) and got[-1][2] == want[-1][2] and len(want) >= 10
    lengths = [x[0].split("Edge length=")[1].split(" ")[0] for x in want]
    swapped = [i for i in range(len(want)) if got[i][:2] != want[i][:2]]
    assert all(lengths.count(lengths[i]) > 1 for i in swapped)                         # only edges of equal length change places
    if len(set(lengths)) == len(lengths):
        assert open(out).read() == rec["fasta"]
    assert name != "hand_flag2" or "N" * 20 in rec["fasta"].replace("\n", "")          # (flag 2 joins across components with gaps)
    ctx.close()


def test_g4_loaded_with_flows_and_long_range_mates(tmp_path):
    """the step-4 graph of the g4 golden case as its file holds it, every flow 2, the golden mates and the long-range ones: the input the reference test runs in its
    `ordered` mode, here on the device against the model, round by round"""
    import gzip
    import test_mate_support_host as MS
    name = "g4_highcopy_k21"; m = fx.golden(name); bases, off = fx.make_reads(m["synth"])
    ctx = s2.Context(m["k"]); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
    parsed = MS.with_flows(H.parse_graph(gzip.open(os.path.join(fx.GOLDEN, name + ".graph4.gz")).read()), lambda q, a: (2.0, 2.0))
    recs = [r for _, a, b_ in parsed["pairs"] for r in (a, b_)]
    g, hdr = loaded(ctx, parsed["header"], recs, tmp_path)
    parsed = H.parse_graph(H.graph_text(parsed["header"], recs))
    pairs = LH.merged(MS.golden_mates(parsed, ctx.reads_stats().unique_reads), LH.long_range_mates(parsed))
    add_mates(ctx, pairs); seqs = H.stored_reads(ctx)
    b = X.Bounds(g, pairs); total = 0
    for rd in range(3):
        r = SM.round_(g, pairs, b, m["k"], 2, 1, False, seqs)
        n = ctx.scaffold_round(2, 1, False)
        same_round(ctx, n, r)
        assert saved6(ctx, tmp_path, f"r{rd}.graph6") == g.text(hdr) and np.array_equal(ctx.graph_flows(), g.flows())
        total += n
        if not n:
            break
    assert total >= 1
    ctx.close()


def test_after_steps_1_to_4_with_flows_handed_in(tmp_path):
    """the graph step 4 left in HBM (pools with room to spare, step 4's own pool order, no flows until they are handed in), not a loaded one: g4 with every flow 2,
    the golden mates and long-range mates.  Rule (a) compares pool indices, which the model, reading the written file, cannot see: the device's own joins are
    replayed through the model's JOIN instead.  Checked per round: every join is a row of the model's unfiltered links (its pairs, ends, support and gap) with a
    support at or above `high`; the counts add up; and after the replay the written graph, the flows and the rebuilt read-to-edge table are the model's"""
    import test_mate_support_host as MS
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
        raw = LH.links(g.parsed(), H.read_edge_table(g.parsed()), pairs, b.ests, b.max_upper, b.arl, k)
        o = g.ordinals()
        n = ctx.scaffold_round(high, 1, False)
        if rd == 0:
            assert ctx.mates_bounds() == (b.min_upper, b.max_upper)
        st = ctx.scaffold_stats().last; joins = ctx.scaffold_merges()
        assert n == len(joins) == st.merged and st.rows == st.below_threshold + st.skipped + st.blocked + st.cycles + st.merged
        for j in joins:
            cand = [(2 * qa + sa, 2 * qb + sb) for (qa, sa, qb, sb, s_, gap) in raw
                    if (o[qa], o[qb], s_, gap) == (int(j["pair_first"]), int(j["pair_second"]), int(j["support"]), int(j["gap"])) and s_ >= high
                    and (g.h[(2 * qa + sa) ^ 1]["frm"], g.h[2 * qb + sb]["to"]) == (int(j["from"]), int(j["to"]))
                    and SM.join_type(g.h[(2 * qa + sa) ^ 1]["type"], g.h[2 * qb + sb]["type"]) == int(j["type"])]
            assert len(cand) >= 1, j                                                   # a row of the unfiltered table, at or above the threshold
            a, e2 = cand[0]
            nh = g.join(a ^ 1, e2, int(j["gap"]), seqs)
            assert (int(j["overlap_forward"]), int(j["overlap_twin"])) == g.last["overlap"] and (int(j["how_forward"]), int(j["how_twin"])) == g.last["how"]
            assert [int(j["first_deleted"]), int(j["second_deleted"])] == [int(x) for x in g.last["deleted"]]
        assert saved6(ctx, tmp_path, f"r{rd}.graph6") == g.text(hdr) and np.array_equal(ctx.graph_flows(), g.flows())
        total += n
        if not n:
            break
    assert total >= 1
    assert table_set(ctx) == X.read_edge_set(g)
    ctx.close()


def test_cli_extend_then_scaffold_on_the_resident_graph(tmp_path):
    """sage2ov -m 6 --extend --scaffold: step 6's first loop, then step 7 on the graph that stays resident, with the estimate of step 6 -- against a context that
    calls extend_by_supports and scaffold one after the other"""
    ctx, g, hdr, pairs, seqs = hand_start(tmp_path)
    out = str(tmp_path / "out") + "/"; os.makedirs(out)
    ctx.reads_save(out + "t.reads"); ctx.graph5_save(out + "t.graph5")
    b_, o = H.mates_ascii(pairs[1], seqs); fa = str(tmp_path / "mates.fa")
    open(fa, "w").write("".join(">m%d\n%s\n" % (i, b_[int(o[i]):int(o[i + 1])].tobytes().decode()) for i in range(len(o) - 1)))
    gs = hdr[1] * hdr[2] // 6
    exe = os.path.join(fx.ROOT, "sage2_amd", "sage2ov")
    subprocess.run([exe, "-k", str(K), "-o", out, "-p", "u", "-i", "t", "-m", "6", "-f", fa, "--extend", "--scaffold", "--genomeSize", str(gs)], check=True, stdout=subprocess.DEVNULL, timeout=120)
    c2 = random_store(len(seqs), 5); c2.graph_load_composite(out + "t.graph5"); add_mates(c2, {1: pairs[1]})
    c2.mates_estimate(); bounds = c2.mates_bounds()
    er, em = c2.extend_by_supports(gs)
    assert open(out + "u.graph6").read() == saved6(c2, tmp_path, "calls.graph6") and em >= 1
    rounds, joined = c2.scaffold(gs)
    assert c2.mates_bounds() == bounds                                                 # no new estimate between the steps
    c2.contigs_build(0, gs); c2.contigs_save(str(tmp_path / "calls.fasta"), 1)
    assert open(out + "u_scaffold.fasta").read() == open(str(tmp_path / "calls.fasta")).read() and os.path.getsize(out + "u_scaffold.fasta") > 0
    log = open(out + "u.log").read()
    assert "Total number of extended contigs: %d\n" % em in log and "Total number of merged scaffolds: %d\n" % joined in log and "Rounds of mergeFinal: %d " % rounds in log and joined >= 1
    ctx.close(); c2.close()
