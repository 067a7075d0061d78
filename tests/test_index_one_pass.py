"""GPU: the index build's two routes -- the locality-ordered copy and the tuples in one visit of the id-ordered store (`k_ix_tuples_loc`, quad of lanes per
read) with the window boundaries by search, and `SAGE2OV_INDEX_SEPARATE_PASSES=1` (`k_loc_scatter`, `k_ix_tuples`, `k_pt_bounds`) -- against the reference's
golden files, against each other and against the oracle, at the sizes and key positions where the quad form can go wrong."""
import re

import numpy as np
import pytest

import fixtures as fx
import oracle_lib as ol
import sage2_amd as s2
from test_gpu_parity import assert_equals_oracle, run_oracle

pytestmark = pytest.mark.gpu

SWITCH = "SAGE2OV_INDEX_SEPARATE_PASSES"


def gpu_ctx(k, bases, off, monkeypatch, separate, steps=True):
    """a context on the default route or on the separate passes (the switch is read through Options: set, then reloaded)"""
    if separate:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    ctx = s2.Context(k)
    ctx.options_reload()
    ctx.reads_add_ascii(bases, off)
    ctx.reads_organize()
    if steps:
        ctx.run_steps23()
    return ctx


def ascii_reads(reads):
    bases = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy()
    off = np.zeros(len(reads) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(r) for r in reads])
    return bases, off


def assert_prefix_suffix_keys(ctx, o, k, ids):
    """index_lookup of the prefix and the suffix key of the reads `ids`: bucket contents in order, against the oracle"""
    fwd, ln, _ = o.export_reads()
    h = min(k, 64)
    for rid in ids:
        b = bytes(fwd[rid])
        for start in (0, int(ln[rid]) - h):
            v0, v1 = (0, ol.get64(b, start, h)) if h <= 32 else (ol.get64(b, start, h - 32), ol.get64(b, start + h - 32, 32))
            want, wn = o.lookup(v0, v1); got, gn = ctx.index_lookup(v0, v1)
            assert gn == wn >= 1 and got == want[:len(got)], (rid, start)


def edges_equal(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in ("from", "to", "type", "length", "length_twin"))


# g2: 8-word layout, one length; g5: mixed lengths; g6: a 64-base key (k = 70) over three pieces of the slot; g1: 4-word layout; g10: 32-word layout (separate kernels)
@pytest.mark.parametrize("name,groups", [("g2_clean150_k40", None), ("g2_clean150_k40", "1"), ("g5_mixedlen_k21", None), ("g6_k70_150", None), ("g1_clean100_k21", None),
                                         ("g10_long900_k55", None)])
def test_both_routes_reproduce_the_golden_files(name, groups, tmp_path, monkeypatch):
    """steps 2-3 on both routes: the edge lists are equal to each other and P.graph3 is the reference's; the P.hashTable files of the two routes are byte-equal.
    groups = "1": the 4-dword tuple format {K, M, entry, tag} through the quad routine."""
    if groups:
        monkeypatch.setenv("SAGE2OV_MINIMIZER_INDEX", groups)
    else:
        monkeypatch.delenv("SAGE2OV_MINIMIZER_INDEX", raising=False)
    m = fx.golden(name)
    bases, off = fx.make_reads(m["synth"])
    out = []
    for separate in (False, True):
        ctx = gpu_ctx(m["k"], bases, off, monkeypatch, separate)
        gp, hp = str(tmp_path / f"t{int(separate)}.graph3"), str(tmp_path / f"t{int(separate)}.hashTable")
        ctx.graph_save(gp); ctx.hashtable_save(hp)
        assert fx.graph3_matches(gp, name)
        assert ctx.index_stats().long_buckets == m["counters"]["long_buckets"]
        out.append((ctx.edges(), open(hp, "rb").read()))
        ctx.close()
    assert edges_equal(out[0][0], out[1][0])
    assert out[0][1] == out[1][1] and len(out[0][1]) > 0
    monkeypatch.delenv(SWITCH, raising=False)


# a workgroup covers one tile of 8192 tuples = 2048 reads, a quad one read: one read, a quad short of a wave, one read short of a tile, a whole tile, a tile and a read
@pytest.mark.parametrize("n", [1, 3, 2047, 2048, 2049])
def test_tile_and_quad_edges_match_oracle(n, monkeypatch):
    k = 40
    bases, off = fx.make_reads(dict(recipe="tiling", seed=500 + n, n_unique=n, read_len=150, step=9))
    o = run_oracle(dict(k=k), bases, off)
    for separate in (False, True):
        ctx = gpu_ctx(k, bases, off, monkeypatch, separate)
        assert ctx.reads_stats().unique_reads == n == o.counter("N")
        assert_equals_oracle(ctx, o)
        if n <= 2047:
            assert_prefix_suffix_keys(ctx, o, k, range(1, n + 1))
        ctx.close()
    o.close()
    monkeypatch.delenv(SWITCH, raising=False)


def test_suffix_key_at_piece_boundaries_matches_oracle(monkeypatch):
    """8-word layout, k = 40: read lengths that put the first base of the suffix key at 63, 64, 65, 127 and 128 -- the ends of the slot's 16-byte pieces (64 bases
    each): the key's words come from one, two or three lanes of the quad."""
    k, step = 40, 6
    lengths = [63 + k, 64 + k, 65 + k, 127 + k, 128 + k, 150]
    rng = np.random.default_rng(77)
    n = 600
    genome = fx._rnd(rng, (n - 1) * step + max(lengths))
    reads = []
    for i in range(n):
        s = genome[i * step:i * step + lengths[i % len(lengths)]]
        reads.append(s if i % 2 == 0 else fx.revcomp(s))
    bases, off = ascii_reads(reads)
    o = run_oracle(dict(k=k), bases, off)
    _, ln, _ = o.export_reads()
    assert {int(x) - k for x in ln[1:]} >= {63, 64, 65, 127, 128}
    for separate in (False, True):
        ctx = gpu_ctx(k, bases, off, monkeypatch, separate)
        assert ctx.reads_stats().unique_reads == o.counter("N")
        assert_equals_oracle(ctx, o)
        assert_prefix_suffix_keys(ctx, o, k, range(1, len(ln)))
        ctx.close()
    o.close()
    monkeypatch.delenv(SWITCH, raising=False)


@pytest.mark.parametrize("seed", [11, 12, 13, 14])
def test_empty_windows_match_oracle(seed, monkeypatch, capfd):
    """Eight reads (32 tuples) in a table of 64 windows -- 64 times the default table: most windows are empty, in runs at the front, in the middle and at the end
    (four read sets, so that every place is met).  The window boundaries come from the search on the default route; the device's own check of the partition
    (SAGE2OV_VERIFY_PARTITION) must find the sorted tuples in order and no window of negative size."""
    k, n = 40, 8
    bases, off = fx.make_reads(dict(recipe="tiling", seed=seed, n_unique=n, read_len=150, step=11))
    default_slots = 4096                                     # max(one window, 8 N rounded up to whole windows) for N = 8
    monkeypatch.setenv("SAGE2OV_TEST_TABLE_SLOTS", str(64 * default_slots))
    o = run_oracle(dict(k=k), bases, off)
    for separate in (False, True):
        ctx = gpu_ctx(k, bases, off, monkeypatch, separate)
        assert ctx.index_stats().slots == 64 * default_slots and ctx.reads_stats().unique_reads == n
        assert_equals_oracle(ctx, o)
        assert_prefix_suffix_keys(ctx, o, k, range(1, n + 1))
        ctx.close()
    monkeypatch.delenv(SWITCH, raising=False)
    capfd.readouterr()
    monkeypatch.setenv("SAGE2OV_VERIFY_PARTITION", "1")
    ctx = gpu_ctx(k, bases, off, monkeypatch, False, steps=False)
    ctx.index_build()
    err = capfd.readouterr().err
    rep = re.findall(r"\[verify-partition\] (\d+) tuples, (\d+) windows: (\d+) order violations, largest window (\d+) tuples, (\d+) negative windows", err)
    assert rep and all((int(r[0]), int(r[1]), int(r[2]), int(r[4])) == (4 * n, 64, 0, 0) for r in rep), err
    ctx.close(); o.close()


# the existing reseed test's input (4-word layout: separate kernels on every attempt) and the same recipe with 150-base reads (8-word layout: the fused first
# attempt, then reseeded attempts through k_ix_tuples)
@pytest.mark.parametrize("read_len", [100, 150])
def test_reseeded_rebuilds_match_oracle(read_len, monkeypatch):
    """Impure long buckets make the build reseed and run again.  The existing reseed test gets there with 7-bit tags on the high-copy fixture; the fingerprints are
    shrunk with them (SAGE2OV_TEST_FP_BITS), which by itself rebuilds nothing."""
    m = fx.golden("g4_highcopy_k21")
    pd = dict(m["synth"], read_len=read_len)
    bases, off = fx.make_reads(pd)
    monkeypatch.setenv("SAGE2OV_TEST_TAG_BITS", "7")
    monkeypatch.setenv("SAGE2OV_TEST_FP_BITS", "4")
    o = run_oracle(m, bases, off)
    ctx = gpu_ctx(m["k"], bases, off, monkeypatch, False)
    assert ctx.index_stats().rebuilds > 0
    assert_equals_oracle(ctx, o)
    ctx.close(); o.close()
