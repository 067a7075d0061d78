"""GPU: sage2ov_reads_find_ids (ReadLoader::getIdOfRead, readLoader.cpp:319-353, batched) on the HIP path -- k_org_classify, k_find_pack, k_find_dir and
k_find_search<S, BYPOS> (kernels_find.inc) against the resident read store.  The cases and the expected value (a restatement of readLoader.cpp:319-353 over the
exported store) are those of tests/test_find_ids_host.py, run here with device 0; on top of them: the batch seam, every state of the store (the released
id-ordered store of memory-diet mode among them), device against host, and that a look-up disturbs nothing the steps read or write."""
import numpy as np
import pytest

import fixtures as fx
import sage2_amd as s2
import test_find_ids_host as H
from test_find_ids_host import LAYOUT_TOPS, check, find, input_reads, organised, rnd

pytestmark = pytest.mark.gpu
GPU = 0


@pytest.mark.parametrize("L,k", [(100, 21), (150, 40)], ids=["L100k21", "L150k40"])
def test_every_input_read_finds_itself(L, k):
    H.case_every_input_read_finds_itself(GPU, L, k)


def test_compare_is_bytes_then_length():
    H.case_compare_is_bytes_then_length(GPU)


def test_bad_and_odd_queries():
    H.case_bad_and_odd_queries(GPU)


def test_self_reverse_complement_reads():
    H.case_self_reverse_complement(GPU)


@pytest.mark.parametrize("top,words", LAYOUT_TOPS, ids=[f"top{t}" for t, _ in LAYOUT_TOPS])
@pytest.mark.parametrize("k", [21, 64])
def test_every_layout(k, top, words):
    H.case_layout(GPU, top, words, k)


def test_heavy_bucket():
    H.case_heavy_bucket(GPU)


def test_edges_of_the_search():
    for n in H.search_edge_counts():
        H.case_search_edges(GPU, n)
    empty = s2.Context(21, device=GPU); empty.reads_organize()           # an empty store: nothing is found, nothing fails
    assert find(empty, ["ACGTACGTACGTACGTACGTACGTACGTAC", "ACGT"]).tolist() == [0, 0]
    st = empty.reads_find_stats()
    assert (st.found, st.not_good, st.not_found) == (0, 1, 1)
    empty.close()


def test_batch_seam(monkeypatch):
    """SAGE2OV_TEST_FIND_BATCH = queries per chunk: the result of every chunking equals the unbatched one, and `launches` shows that the chunks happened"""
    L, k = 100, 21
    monkeypatch.delenv("SAGE2OV_TEST_FIND_BATCH", raising=False)
    bases, off = fx.make_reads(dict(recipe="tiling", seed=5000, n_unique=700, read_len=L, step=7, dup_every=4, dup_copies=1))
    ctx = organised(k, (bases, off), GPU)
    reads = input_reads(bases, off); rng = np.random.default_rng(5001)
    queries = reads + [rnd(rng, L) for _ in range(60)] + [r[:-1] + "N" for r in reads[:40]] + ["", "ACGT"] + [r[:k] for r in reads[:23]]
    n = len(queries); assert 950 <= n <= 1050
    whole = check(ctx, queries, k)
    st = ctx.reads_find_stats()
    assert st.launches == 1 and st.route == s2.FIND_ROUTE_ID_STORE
    for batch in (1, 63, 64, 65, n - 1):
        monkeypatch.setenv("SAGE2OV_TEST_FIND_BATCH", str(batch)); ctx.options_reload()
        assert np.array_equal(check(ctx, queries, k), whole)
        assert ctx.reads_find_stats().launches == (n + batch - 1) // batch
    ctx.close()


def test_store_states(tmp_path, monkeypatch):
    """after reads_organize only, after run_steps23 on the default route, after run_steps23 in memory-diet mode on one-length reads (the id-ordered store is
    released: the search goes through posOf[] into the locality-ordered store), after reads_load of a P.reads we wrote, after reads_import_words: the same ids"""
    monkeypatch.delenv("SAGE2OV_MEMORY_DIET", raising=False)
    queries, first = H.case_store_states(GPU, tmp_path)                  # organise / reads_load / reads_import_words
    k = 21
    bases, off = fx.make_reads(dict(recipe="tiling", seed=4800, n_unique=1500, read_len=100, step=7, dup_every=5, dup_copies=1))
    a = organised(k, (bases, off), GPU)
    a.run_steps23()
    assert np.array_equal(check(a, queries, k), first) and a.reads_find_stats().route == s2.FIND_ROUTE_ID_STORE
    assert a.reads_find_stats().directory_ms > 0
    check(a, queries, k)
    assert a.reads_find_stats().directory_ms == 0                        # the directory is built by the first call and kept
    a.close()
    monkeypatch.setenv("SAGE2OV_MEMORY_DIET", "1")
    b = organised(k, (bases, off), GPU)                                  # the directory is built from the id-ordered store, the search moves to the other one
    assert np.array_equal(check(b, queries, k), first) and b.reads_find_stats().route == s2.FIND_ROUTE_ID_STORE
    b.run_steps23()
    assert np.array_equal(check(b, queries, k), first) and b.reads_find_stats().route == s2.FIND_ROUTE_LOCALITY
    b.run_steps23()
    assert np.array_equal(check(b, queries, k), first) and b.reads_find_stats().route == s2.FIND_ROUTE_LOCALITY
    b.close()
    c = organised(k, (bases, off), GPU)                                  # the directory itself is built through posOf[]
    c.run_steps23()
    assert np.array_equal(check(c, queries, k), first)
    st = c.reads_find_stats()
    assert st.route == s2.FIND_ROUTE_LOCALITY and st.directory_ms > 0
    c.close()


def test_device_equals_host():
    k = 40
    bases, off = fx.make_reads(dict(seed=5100, genome_len=30000, n_reads=6000, read_len=150, read_len_min=60, err_ppm=2000))      # the generator's reads: mixed lengths, errors
    reads = input_reads(bases, off); rng = np.random.default_rng(5101)
    queries = reads + [fx.revcomp(r) for r in reads[::2]] + [rnd(rng, 150) for _ in range(200)] + [r[:-1] for r in reads[:200]]
    g, h = organised(k, (bases, off), GPU), organised(k, (bases, off), H.HOST)
    assert g.reads_stats().unique_reads == h.reads_stats().unique_reads > 3000
    ig, ih = check(g, queries, k), check(h, queries, k)
    assert np.array_equal(ig, ih)
    assert g.reads_find_stats().route == s2.FIND_ROUTE_ID_STORE and h.reads_find_stats().route == s2.FIND_ROUTE_HOST
    g.close(); h.close()


@pytest.mark.parametrize("route", ["default", "memory_diet"])
def test_nothing_is_disturbed(route, monkeypatch):
    """run_steps23, look ids up, run_steps23 again: the second edge list and the per-read records are those of the first"""
    if route == "memory_diet":
        monkeypatch.setenv("SAGE2OV_MEMORY_DIET", "1")
    else:
        monkeypatch.delenv("SAGE2OV_MEMORY_DIET", raising=False)
    k = 40
    bases, off = fx.make_reads(dict(seed=5200, genome_len=20000, n_reads=8000, read_len=150, err_ppm=500))
    ctx = organised(k, (bases, off), GPU)
    ctx.run_steps23()
    e1, r1, st1 = ctx.edges().copy(), ctx.overlap_export_initial(), ctx.overlap_stats()
    ids = check(ctx, input_reads(bases, off), k)
    assert np.all(ids != 0) and len(e1) > 0
    e_mid, r_mid = ctx.edges(), ctx.overlap_export_initial()             # what the steps left is still there
    assert e_mid.tobytes() == e1.tobytes() and all(np.array_equal(x, y) for x, y in zip(r1, r_mid))
    ctx.run_steps23()
    e2, r2, st2 = ctx.edges(), ctx.overlap_export_initial(), ctx.overlap_stats()
    assert e2.tobytes() == e1.tobytes() and all(np.array_equal(x, y) for x, y in zip(r1, r2))
    assert (st1.verified_overlaps, st1.edges, st1.transitive_removed) == (st2.verified_overlaps, st2.edges, st2.transitive_removed)
    assert np.array_equal(check(ctx, input_reads(bases, off), k), ids)
    ctx.close()


def test_cpp_mirror(tmp_path):
    H.case_cpp_mirror(GPU, tmp_path)
