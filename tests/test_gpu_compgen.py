"""GPU: the four step 6/7 device sweeps -- read-to-edge table and insert sizes, supports at a node, scaffold links, contigs -- on generated
composite graphs (tests/compgen.py), against the restatements over the text sage2ov_graph4_save wrote.  Every comparison is exact equality.  What these graphs have
and the goldens lack (there every read lies on one record pair, once):
  A  sort digits: half-edges on both sides of 2^16, reads on both sides of 2^16, a longest contig on both sides of 2^16
  B  reads on 2 .. 33 pairs, some twice on an edge: the seams of the 8-lane groups of the mate join
  C  more than 262 144 distances of one library: the second sweep of the grid-stride loop of the estimation rounds
  D  a list pool whose distPrevious add up to more than 2^32: the running sums taken from one scan modulo 2^32
  E  twenty seeds of small graphs with every knob on, two of them again in memory-diet mode
That none of this is vacuous is shown from the restatements alone in tests/test_compgen_host.py."""
import numpy as np
import pytest
import compgen as CG
import test_compgen_host as GH
import test_mate_estimate_host as H
import test_links_host as LH
import test_contigs_host as CH
from test_gpu_mate_estimate import random_store, load_text, add_mates, check_all
from test_gpu_mate_support import saved_graph, flat_flows, check as check_supports
from test_gpu_links import check as check_links
from test_gpu_contigs import check as check_contigs, strings_of

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("minimiser_groups_on")]
K = CG.K


def loaded(case, store_seed, tmp):
    """a fresh store with the case's graph loaded: (context, parsed saved graph with the case's flows, saved text, parsed loaded text).  The pair ordinals of the
    tables are those of the saved text; the order of the contig table among edges of one length and one node is that of the half-edge indices, which are the
    loaded text's (CH.contig_table works out the ordinals itself)"""
    N, header, recs = case[:3]; text = H.graph_text(header, recs)
    ctx = random_store(N, store_seed, k=K); load_text(ctx, text, tmp)
    g, saved = saved_graph(ctx, tmp, recs)
    assert np.array_equal(ctx.graph_flows(), flat_flows(g))                          # the loader took the flows of the file
    return ctx, g, saved, H.parse_graph(text)


def readmap(ctx, g, saved, pairs, valid):
    out = check_all(ctx, saved, pairs, valid=valid)
    t = H.read_edge_table(g); st = ctx.readmap_stats()
    for L, pl in pairs.items():
        assert st.distances[L] == len(H.mate_distances(t, H.mate_entries(pl))), L
    assert st.sort_passes == GH.sort_passes_by_rule(ctx.reads_stats().unique_reads, len(g["pairs"]))
    return out


def four_sweeps(ctx, g, saved, g_loaded, pairs, valid, tmp, thresholds=(0, 20)):
    readmap(ctx, g, saved, pairs, valid)
    sup, _ = check_supports(ctx, g, pairs, K)
    lk, _ = check_links(ctx, g, pairs, K)
    seqs = H.stored_reads(ctx)
    for thr in thresholds:
        check_contigs(ctx, g_loaded, seqs, tmp, threshold=thr, name="c%d.fasta" % thr)
    return sup, lk


def exports(ctx, pairs):
    ctx.contigs_build(20, 0)
    return ([x.tobytes() for x in ctx.read_edges()] + [ctx.mates_flags(L).tobytes() + ctx.mates_distances(L).tobytes() for L in pairs] +
            [ctx.mates_supports(1).tobytes()] + [ctx.links(m).tobytes() for m in (LH.ALL, LH.FINAL, LH.SMALL)] + [ctx.contigs().tobytes(), "".join(strings_of(ctx)).encode()])


# ------------------------------------------------------------------------------------------ E: twenty seeds, every knob
@pytest.mark.parametrize("seed", CG.E_SEEDS)
def test_e_small_mixed_graphs(seed, tmp_path, monkeypatch):
    case = CG.case_e(seed); pairs = CG.mates_e(GH.parsed(case), seed)
    ctx, g, saved, g_loaded = loaded(case, 100 + seed, tmp_path); add_mates(ctx, pairs)
    four_sweeps(ctx, g, saved, g_loaded, pairs, [1, 2, 3], tmp_path)
    assert ctx.mates_insert(4).valid == 0 and ctx.mates_insert(3).upper + K - 2 * 60 <= 0
    if seed < 2:                                                                    # again in memory-diet mode, a fresh context: byte-equal exports
        want = exports(ctx, pairs)
        monkeypatch.setenv("SAGE2OV_MEMORY_DIET", "1")
        c2, g2, saved2, _ = loaded(case, 100 + seed, tmp_path); add_mates(c2, pairs)
        assert saved2 == saved and exports(c2, pairs) == want
        c2.close()
    ctx.close()


# ------------------------------------------------------------------------------------------ B: reads on many pairs
def test_b_reads_on_many_pairs(tmp_path):
    case = CG.case_b(); pairs = CG.mates_b(GH.parsed(case))
    ctx, g, saved, _ = loaded(case, 31, tmp_path)
    per = GH.distances_per_entry(g, pairs[1]); pr = H.by_read(H.read_edge_table(g))      # from the restatement, before the library is asked anything
    assert {len(v) for v in pr.values()} >= {2, 7, 8, 9, 15, 16, 17, 33} and GH.max_times_on_an_edge(g) == 2
    assert {c for c, _ in per.values()} >= {0, 1, 7, 8, 9, 17}
    nine = {e for e, (c, d) in per.items() if d >= 9}; fewer = {e for e, (c, d) in per.items() if c == 17 and 0 < d < 17}
    assert nine and fewer and len(nine | fewer) >= 2
    add_mates(ctx, pairs)
    readmap(ctx, g, saved, pairs, [1, 2])
    check_supports(ctx, g, pairs, K)                                                # (their census counters -- entries within the bound, unique entries, mate entries -- included)
    rows, st = check_links(ctx, g, pairs, K)
    assert st.records > 0 and ctx.support_stats().candidates > 0
    ctx.close()


# ------------------------------------------------------------------------------------------ C: the estimation rounds beyond one sweep
def test_c_more_distances_than_one_sweep(tmp_path):
    N, header, recs, pairs = CG.case_c()
    g0 = H.parse_graph(H.graph_text(header, recs))
    want_d = H.mate_distances(H.read_edge_table(g0), H.mate_entries(pairs[1])); e = H.estimate(want_d, header[2])
    assert len(want_d) > 262144 and e["rounds"] >= 3 and e["considered"][0] < e["considered"][-1] and H.valid_every_round(want_d)
    ctx = random_store(N, 41, k=K); load_text(ctx, H.graph_text(header, recs), tmp_path)
    g, saved = saved_graph(ctx, tmp_path, recs); assert [a["list"] for _, a, _ in g["pairs"]] == [a["list"] for _, a, _ in g0["pairs"]]
    add_mates(ctx, pairs); ctx.mates_map_reads(); ctx.mates_estimate()
    got = ctx.mates_distances(1)
    assert len(got) == len(want_d) and np.array_equal(got, np.asarray(want_d, dtype=np.uint32))
    ins = ctx.mates_insert(1); H.same_estimate(ins, e)
    assert list(ins.considered)[:e["rounds"]] == e["considered"][:e["rounds"]] and ctx.readmap_stats().distances[1] == len(want_d)
    ctx.close()


# ------------------------------------------------------------------------------------------ A: the digits of the four sorts
@pytest.fixture(scope="module")
def a_pairs(tmp_path_factory):
    """a graph of n record pairs, loaded, with its mates: built once per n and shared by the sweeps' tests"""
    cache = {}

    def get(n):
        if n not in cache:
            case = CG.case_a_pairs(n); pairs, triples = CG.mates_a(GH.parsed(case)); tmp = tmp_path_factory.mktemp("a%d" % n)
            ctx, g, saved, g_loaded = loaded(case, 11, tmp); add_mates(ctx, pairs)
            assert len(g["pairs"]) == n and not any(a["frm"] == a["to"] for _, a, _ in g["pairs"])      # no loops: a pair's ordinal is its index, half-edges = 2 n
            cache[n] = (ctx, g, saved, pairs, g_loaded, triples)
        return cache[n]
    yield get
    for c in cache.values():
        c[0].close()


def half_indices(g_loaded):
    """{(from, to): index of the half-edge in the resident graph}: the halves of the p-th record pair of the loaded text are 2 p and 2 p + 1 (no loops; two nodes
    are joined by one pair at most).  The sorts of the supports and of the links go by these indices"""
    out = {}
    for p, (_, a, b) in enumerate(g_loaded["pairs"]):
        out[(a["frm"], a["to"])] = 2 * p; out[(b["frm"], b["to"])] = 2 * p + 1
    return out


def across_two_to_the_16(idx):
    return any(a >= 65536 > b for a, b in idx) and any(b >= 65536 > a for a, b in idx)


@pytest.mark.parametrize("n", [32767, 33024])
def test_a_pairs_readmap(n, a_pairs):
    ctx, g, saved, pairs, _, _ = a_pairs(n)
    ent, _, _ = readmap(ctx, g, saved, pairs, [1, 2])
    assert ctx.readmap_stats().sort_passes == (2 if n < 32768 else 3) + 3 and 65536 <= ctx.reads_stats().unique_reads < 1 << 17
    if n > 32768:
        assert (ent["pair"] >= 32768).any() and (ent["pair"] < 32768).any()


@pytest.mark.parametrize("n,passes", [(32767, 4), (32768, 6), (33024, 6)])
def test_a_pairs_supports(n, passes, a_pairs):
    ctx, g, saved, pairs, g_loaded, _ = a_pairs(n)
    rows, st = check_supports(ctx, g, pairs, K, min_supports=(1, 2))
    assert st.sort_passes == passes and st.keys2 > 0
    if n == 33024:                                                                  # by the restatement's rows: supported rows across 2^16 half-edges, both orders
        ix = half_indices(g_loaded)
        assert across_two_to_the_16([(ix[(i, ta)], ix[(i, tb)]) for (i, qa, qb, ta, tb, s) in rows if s >= 1])


@pytest.mark.parametrize("n,passes", [(32767, 4), (32768, 6), (33024, 6)])
def test_a_pairs_links(n, passes, a_pairs):
    ctx, g, saved, pairs, g_loaded, triples = a_pairs(n)
    rows, st = check_links(ctx, g, pairs, K, min_supports=(1, 2))
    assert st.sort_passes == passes and st.records > 0
    if n == 33024:
        ix = half_indices(g_loaded); hv = LH.halves_of(g); at = lambda q, s: ix[(hv[(q, s)][0]["frm"], hv[(q, s)][0]["to"])]
        assert across_two_to_the_16([(at(r[0], r[1]), at(r[2], r[3])) for r in rows])
        # one half with records to b and to b + 65 536 in turns (CG.mates_a): only a sort by every digit brings each key's records together
        sup = {(at(r[0], r[1]), at(r[2], r[3])): r[4] for r in rows}
        assert len(triples) == 3 and all(ix[b] == ix[c] + 65536 and sup[(ix[a], ix[b])] == 2 and sup[(ix[a], ix[c])] == 2 for a, b, c in triples)


@pytest.mark.parametrize("n", [32767, 33024])
def test_a_pairs_contigs(n, a_pairs):
    """the table, its order and the statistics in full; the strings of the first and the last twenty rows"""
    ctx, g, saved, pairs, g_loaded, _ = a_pairs(n)
    rows, st, thr = CH.contig_table(g_loaded, H.stored_reads(ctx))
    ctx.contigs_build(0, 0)
    assert CH.got_tuples(ctx.contigs()) == CH.table_tuples(rows) and len(rows) > 10000
    CH.same_stats(ctx.contig_stats(), st)
    assert strings_of(ctx, 0, 20) == [r["string"] for r in rows[:20]] and strings_of(ctx, len(rows) - 20, 20) == [r["string"] for r in rows[-20:]]


@pytest.mark.parametrize("N", [65535, 65536])
def test_a_reads_third_digit_of_the_read_id(N, tmp_path):
    case = CG.case_a_reads(N); pairs = CG.mates_for(GH.parsed(case), 10, libraries=2, for_reference=True, k=K)
    named = [r for r in CG.A_READS if r <= N]
    pairs[1] += [(named[i], 1, named[i + 1], 0) for i in range(len(named) - 1)]
    ctx, g, saved, _ = loaded(case, 13, tmp_path); add_mates(ctx, pairs)
    assert {e[0] for _, a, _ in g["pairs"] for e in a["list"]} >= set(named)
    ent, loc, off = readmap(ctx, g, saved, pairs, [1, 2])
    assert set(named) <= set(ent["read"].tolist()) and ctx.readmap_stats().sort_passes == (2 if N < 65536 else 3) + 2
    ctx.close()


@pytest.mark.parametrize("longest", [65535, 65536, 70000])
def test_a_longest_contig(longest, tmp_path):
    case = CG.case_a_longest(longest)
    ctx, g, saved, g_loaded = loaded(case, 7, tmp_path)
    rows, fasta = check_contigs(ctx, g_loaded, H.stored_reads(ctx), tmp_path)
    lens = [r["len"] for r in rows[1:]]
    assert rows[0]["len"] == longest and len(rows) >= 301 and len(set(lens)) < len(lens) // 4 and ((longest - min(lens)) >> 16 != 0) == (longest == 70000)
    ctx.close()


# ------------------------------------------------------------------------------------------ D: the pool scan across 2^32
def test_d_pool_sums_beyond_two_to_the_32(tmp_path):
    N, header, text, long_, short, pairs = CG.case_d()
    assert sum(int(d[:-1].sum()) for _, _, d in long_) > 1 << 32                       # the E halves alone; the pool holds the twins' lists too
    ctx = random_store(N, 17, k=K); load_text(ctx, text, tmp_path)
    out = str(tmp_path / "saved.graph4"); ctx.graph4_save(out)
    assert open(out).read() == text and len(text) > 75000000                        # (the writer's order and ordinals are the generator's)
    ctx.graph_set_flows(np.ones(10, dtype=np.float32)); add_mates(ctx, pairs)
    # ---- the read-to-edge table by contract, with cumsum
    want_ent, want_loc = CG.case_d_table(header, long_, short)
    ts = H.read_edge_table(H.parse_graph(H.graph_text(header, short)))
    ent, loc, off = ctx.read_edges()
    got_ent = np.stack([ent[n].astype(np.int64) for n in ("read", "pair", "from", "to", "type", "n_forward", "n_reverse", "location")], axis=1)
    assert np.array_equal(got_ent, want_ent) and np.array_equal(loc, want_loc)
    assert np.array_equal(off, np.searchsorted(ent["read"].astype(np.int64), np.arange(N + 2)))
    assert int(ent["n_forward"].max()) >= CG.D_LONG // CG.D_CYCLE and len(loc) == 2 * (3 * CG.D_LONG + 50)
    # ---- the estimate (the short edges' reads stand nowhere else) and the bound
    want_d = H.mate_distances(ts, H.mate_entries(pairs[1])); e = H.estimate(want_d, header[2]); assert H.valid_every_round(want_d)
    ctx.mates_estimate(); H.same_estimate(ctx.mates_insert(1), e)
    lo, hi = H.bounds([e], header[2]); assert ctx.mates_bounds() == (lo, hi)
    # ---- entries within the bound: the first few of each long list, wherever it lies in the pool
    within = lambda dists: int((np.cumsum(dists) <= hi).sum())
    twins = sum(within(d[:0:-1]) for _, _, d in long_) + sum(within([x[3] for x in short[i]["list"]]) for i in (1, 3))
    firsts = sum(within(d[:-1]) for _, _, d in long_) + sum(within([x[3] for x in short[i]["list"]]) for i in (0, 2))
    assert all(0 < within(d[:-1]) < 20 and 0 < within(d[:0:-1]) < 20 for _, _, d in long_)
    ctx.mates_supports(1)
    st = ctx.support_stats(); assert (st.in_halves, st.out_halves, st.candidates, st.entries_within) == (5, 5, 2, twins)      # the in-halves (types 0, 1) are the twins
    assert len(ctx.links()) > 0
    sl = ctx.link_stats(); assert (sl.halves, sl.entries_within) == (10, twins + firsts) and sl.records > 0
    ctx.close()
