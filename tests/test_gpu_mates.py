"""GPU: the mate-pair table (sage2ov_mates_*) on the HIP path -- the chunk body of the read-id look-up with the ids left in HBM, k_mate_keep, k_mate_records,
the k_rs_* passes, k_mate_heads, k_headpos, k_mate_reduce, k_mate_merge and k_mate_offsets (kernels_mates.inc).  The cases and the expected value (a
restatement of matePair.cpp:161-239, one thread) are those of tests/test_mates_host.py, run here with device 0; on top of them: the chunk seam and the flush
bound, every state of the store, device against host, and that the table and the steps do not disturb each other."""
import numpy as np
import pytest

import fixtures as fx
import sage2_amd as s2
import test_mates_host as M
from test_find_ids_host import HOST, input_reads, organised, rnd
from test_mates_host import Restated, add, compare, ordinary_pairs

pytestmark = pytest.mark.gpu
GPU = 0
FIELDS = ("from", "to", "type1", "type2", "count", "first", "freq", "library")


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in FIELDS)


def test_ordinary_pairs():
    M.case_ordinary(GPU)


def test_freq_wraps_like_a_uint8():
    M.case_freq_wrap(GPU)


def test_self_pairs():
    M.case_self_pairs(GPU)


def test_skipped_pairs():
    M.case_skipped_pairs(GPU)


def test_calls():
    M.case_calls(GPU)


@pytest.mark.parametrize("N", M.DIGIT_EDGE_COUNTS)
def test_digit_edges(N):
    M.case_digit_edges(GPU, N)


@pytest.mark.parametrize("P", M.TILE_SEAM_PAIRS)
def test_tile_seams(P):
    M.case_tile_seams(GPU, P)


def test_libraries(tmp_path):
    M.case_libraries(GPU, tmp_path)


def test_files(tmp_path, monkeypatch):
    M.case_files(GPU, tmp_path, monkeypatch)


def test_cpp_mirror(tmp_path):
    M.case_cpp_mirror(GPU, tmp_path)


def test_errors():
    M.case_errors(GPU)


def test_chunk_seam(monkeypatch):
    """SAGE2OV_TEST_FIND_BATCH = queries per chunk (an odd value is rounded up to the next even one: a pair is never cut from its ids), SAGE2OV_TEST_MATE_FLUSH =
    pending records per flush: every chunking gives the unchunked table, and the stats show that the chunks and the flushes happened"""
    k = 21
    monkeypatch.delenv("SAGE2OV_TEST_FIND_BATCH", raising=False); monkeypatch.delenv("SAGE2OV_TEST_MATE_FLUSH", raising=False)
    ctx, reads = M.tiling_store(GPU, 400, 100, k, 7100, dup_every=4, dup_copies=1)
    rng = np.random.default_rng(7101)
    mates = ordinary_pairs(reads)[:900] + [rnd(rng, 100) for _ in range(30)] + [r[:-1] + "N" for r in reads[:30]] + ["", "ACGT"] + [r[:k] for r in reads[:21]] + ordinary_pairs(reads[:60])
    n = len(mates); assert 950 <= n <= 1100 and n % 2 == 1
    R = Restated(); st = add(ctx, R, mates, k)
    whole = compare(ctx, R)
    assert (st.chunks, st.flushes, st.route) == (1, 1, s2.MATE_ROUTE_DEVICE) and st.pairs_not_good > 20 and st.pairs_not_found > 10
    passes = M.radix_passes(400)
    assert st.sort_passes == passes
    for batch in (1, 2, 63, 64, 65, n - 1):
        monkeypatch.setenv("SAGE2OV_TEST_FIND_BATCH", str(batch)); ctx.options_reload()
        ctx.mates_clear(); R = Restated(); st = add(ctx, R, mates, k)
        even = (batch + 1) & ~1
        assert st.chunks == ((n & ~1) + even - 1) // even and st.flushes == 1
        assert same(compare(ctx, R), whole)
    monkeypatch.setenv("SAGE2OV_TEST_FIND_BATCH", "64")
    for flush in (1, 100, 101):
        monkeypatch.setenv("SAGE2OV_TEST_MATE_FLUSH", str(flush)); ctx.options_reload()
        ctx.mates_clear(); R = Restated(); st = add(ctx, R, mates, k)
        assert st.flushes > 3 and st.sort_passes == passes * (2 * st.flushes - 1)      # every flush but the first one merges
        assert same(compare(ctx, R), whole)
    ctx.close()


def test_store_states_and_no_disturbance(monkeypatch):
    """mates added after reads_organize, after run_steps23, after run_steps23 in memory-diet mode (the id-ordered store is released: the look-up goes through
    posOf[]): the same table.  run_steps23, the mates calls, run_steps23: the edge list and the initial records are those of the first run, byte for byte."""
    monkeypatch.delenv("SAGE2OV_MEMORY_DIET", raising=False)
    k = 40
    bases, off = fx.make_reads(dict(seed=7200, genome_len=20000, n_reads=8000, read_len=150, err_ppm=500))
    reads = input_reads(bases, off); mates = reads[:3000] + [fx.revcomp(r) for r in reads[3000:4000]]
    tables = []
    for diet in (False, True):
        if diet:
            monkeypatch.setenv("SAGE2OV_MEMORY_DIET", "1")
        ctx = organised(k, (bases, off), GPU)
        R = Restated(); add(ctx, R, mates[:2000], k)
        ctx.run_steps23()
        e1, r1 = ctx.edges().copy(), ctx.overlap_export_initial()
        assert len(e1) > 0
        add(ctx, R, mates[2000:], k)                                     # between: the table begun before the steps goes on after them
        assert ctx.mates_stats().route == s2.MATE_ROUTE_DEVICE
        tables.append(compare(ctx, R).copy())
        assert ctx.edges().tobytes() == e1.tobytes() and all(np.array_equal(x, y) for x, y in zip(r1, ctx.overlap_export_initial()))
        ctx.run_steps23()
        assert ctx.edges().tobytes() == e1.tobytes() and all(np.array_equal(x, y) for x, y in zip(r1, ctx.overlap_export_initial()))
        assert same(ctx.mates(1)[0], tables[-1])                         # the steps left the table alone
        R2 = Restated(); add(ctx, R2, mates, k, library=2)               # after: one call
        after = compare(ctx, R2, 2)
        assert all(np.array_equal(after[f], tables[-1][f]) for f in FIELDS if f != "library")
        ctx.close()
    assert same(tables[0], tables[1])


def test_device_equals_host():
    k = 40
    bases, off = fx.make_reads(dict(seed=7300, genome_len=30000, n_reads=6000, read_len=150, read_len_min=60, err_ppm=2000))      # the generator's reads as interleaved mates
    mates = input_reads(bases, off)
    g, h = organised(k, (bases, off), GPU), organised(k, (bases, off), HOST)
    assert g.reads_stats().unique_reads == h.reads_stats().unique_reads > 3000
    g.mates_add_ascii(bases, off, 1); h.mates_add_ascii(bases, off, 1)
    sg, sh = g.mates_stats(), h.mates_stats()
    assert (sg.route, sh.route) == (s2.MATE_ROUTE_DEVICE, s2.MATE_ROUTE_HOST)
    assert (sg.pairs_seen, sg.pairs_added, sg.pairs_not_good, sg.pairs_not_found) == (sh.pairs_seen, sh.pairs_added, sh.pairs_not_good, sh.pairs_not_found) == (3000, 3000, 0, 0)
    (eg, og), (eh, oh) = g.mates(1), h.mates(1)
    assert same(eg, eh) and np.array_equal(og, oh) and len(eg) > 5000
    R = Restated(); R.add(g, mates, k, 1); compare(g, R)
    g.close(); h.close()
