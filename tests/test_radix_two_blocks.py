"""GPU: the radix passes of the locality order, the index tables and the edge-list conversion on their default route -- two workgroups per CU on tiles
staged in LDS in two halves (`k_pt_scatter2`), the scan in two launches -- against
`SAGE2OV_PT_ONE_BLOCK=1` (`k_pt_scatter`, one workgroup of sixteen waves on the whole tile), and against the reference's golden files where there are some.
Equal means: the edge lists field by field, the P.hashTable files byte for byte (the order inside a bucket is the table sort's stability) and the per-read
records of the whole position range byte for byte (they are indexed by position and name neighbours by position: equal only if the locality order is the
same permutation).  Sizes: a read gives 4 table tuples and one element of the order; a tile is 8192 of either, a half 4096."""
import numpy as np
import pytest

import fixtures as fx
import sage2_amd as s2
from sage2_amd.shard import RECORD_BYTES
from test_gpu_parity import _Hip, run_oracle
from test_index_one_pass import ascii_reads, assert_prefix_suffix_keys, edges_equal

pytestmark = pytest.mark.gpu

SWITCH = "SAGE2OV_PT_ONE_BLOCK"
TABLE_FILE_MIN = 12501                    # P.hashTable is defined from this many unique reads on (hashtable_save refuses below)


def outputs(k, bases, off, monkeypatch, one_block, tmp_path, graph3_of=None, oracle=None):
    """(unique reads, edges, P.hashTable bytes, records of all positions) of one route.  Below TABLE_FILE_MIN reads there is no table file: with an oracle, the
    buckets of every read's prefix and suffix key are compared with the oracle's instead, entry by entry in bucket order."""
    if one_block:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    ctx = s2.Context(k)
    ctx.options_reload()
    ctx.reads_add_ascii(bases, off); ctx.reads_organize(); ctx.run_steps23()
    n = ctx.reads_stats().unique_reads
    table = b""
    if n >= TABLE_FILE_MIN:
        hp = str(tmp_path / f"t{int(one_block)}.hashTable")
        ctx.hashtable_save(hp)
        table = open(hp, "rb").read()
        assert len(table) > 0
    if oracle is not None:
        assert n == oracle.counter("N")
        assert_prefix_suffix_keys(ctx, oracle, k, range(1, n + 1))
    if graph3_of:
        gp = str(tmp_path / f"t{int(one_block)}.graph3")
        ctx.graph_save(gp)
        assert fx.graph3_matches(gp, graph3_of)
    edges = ctx.edges()
    ctx.close()
    # the records: one rank that owns every position, straight after the probe pass
    c = s2.Context(k, device=0, rank=0, world=1)
    c.options_reload()
    c.reads_add_ascii(bases, off); c.reads_organize(); c.index_build(); c.overlap_probe_shard()
    assert c.shard_range() == (1, n + 1)
    hip = _Hip()
    p = hip.alloc(n * RECORD_BYTES); c.shard_export_records(p, n)
    records = hip.to_host(p, n * RECORD_BYTES)
    hip.free(); c.close()
    monkeypatch.delenv(SWITCH, raising=False)
    return n, edges, table, records


def assert_routes_equal(k, bases, off, monkeypatch, tmp_path, n_unique=None, graph3_of=None, oracle=None):
    a = outputs(k, bases, off, monkeypatch, False, tmp_path, graph3_of, oracle)
    b = outputs(k, bases, off, monkeypatch, True, tmp_path, graph3_of, oracle)
    if n_unique is not None:
        assert a[0] == n_unique
    assert a[0] == b[0] > 0
    assert edges_equal(a[1], b[1])
    assert a[2] == b[2] and (len(a[2]) > 0) == (a[0] >= TABLE_FILE_MIN)
    assert np.array_equal(a[3], b[3]) and len(a[3]) == a[0] * RECORD_BYTES
    return a


# table tuples (4 per read, 2048 reads per tile): last tile shorter than a half, a read over a half, a read short of whole, whole, a read over, three tiles and a
# read, seven tiles and a read (the smallest such set with a table file); elements of the order (1 per read): 4097 = a read over a half, 8193 = a read over a
# tile.  8 reads: the table is one window -- no pass, the copy.
# The scans of these runs have 2047 / 2048 / 2049 / 8193 items and one or two more (flags and degrees of the reads) and 512 x tiles (the passes' counters): under,
# at and over a block of the one-by-one tail, under, at (16 tiles) and over one block of 8192.
@pytest.mark.parametrize("n", [8, 1023, 1025, 2047, 2048, 2049, 4097, 3 * 2048 + 1, 8193, 7 * 2048 + 1])
def test_tile_and_half_edges(n, monkeypatch, tmp_path):
    bases, off = fx.make_reads(dict(recipe="tiling", seed=900 + n, n_unique=n, read_len=150, step=9))
    o = run_oracle(dict(k=40), bases, off) if n <= 2049 else None
    _, edges, _, _ = assert_routes_equal(40, bases, off, monkeypatch, tmp_path, n_unique=n, oracle=o)
    assert len(edges) > 0
    if o is not None:
        o.close()


# The scan sums the blocks in front of a block inside the final kernel up to a bound on the number of blocks, beyond it a kernel in between does.  The bound
# lowered to 0 (every scan in three launches) and to 1 block of 8192 items: 8193 reads scan 8193 .. 8195 items (two blocks, three launches) beside the passes'
# counters (512 x 2 and 512 x 5 items: one block, two launches); 4 x 8192 + 1 reads put the table's counters at 512 x 17 items, a block and a half.
@pytest.mark.parametrize("n,bound", [(8193, "0"), (8193, "1"), (4 * 8192 + 1, "1"), (4 * 8192 + 1, "2")])
def test_scan_forms_around_the_bound(n, bound, monkeypatch, tmp_path):
    bases, off = fx.make_reads(dict(recipe="tiling", seed=700 + n, n_unique=n, read_len=150, step=9))
    ref = outputs(40, bases, off, monkeypatch, True, tmp_path)
    monkeypatch.setenv("SAGE2OV_TEST_SCAN_DIRECT_BLOCKS", bound)
    got = outputs(40, bases, off, monkeypatch, False, tmp_path)
    monkeypatch.delenv("SAGE2OV_TEST_SCAN_DIRECT_BLOCKS", raising=False)
    assert got[0] == ref[0] == n
    assert edges_equal(got[1], ref[1]) and len(ref[1]) > 0
    assert got[2] == ref[2] and (len(ref[2]) > 0) == (n >= TABLE_FILE_MIN)
    assert np.array_equal(got[3], ref[3])


def poly_a_reads(rng, n):
    """n distinct reads of 150 bases that begin with sixteen A and have no run of sixteen A or T after them: the minimiser hash is 0 (the smallest there is), at
    offset 0, on the same strand in every read -- all elements of the order carry ONE digit in each of its five passes"""
    reads = set()
    while len(reads) < n:
        tail = "C" + fx._rnd(rng, 133)
        if "A" * 16 not in tail and "T" * 16 not in tail:
            reads.add("A" * 16 + tail)
    return sorted(reads)


@pytest.mark.parametrize("mixed", [False, True])
def test_one_digit_tiles_and_runs_across_the_half(mixed, monkeypatch, tmp_path):
    """5000 reads with one minimiser: the order's tile is a single (tile, digit) run that lies across the half boundary at 4096 and is written in two
    pieces.  Mixed: the same reads half and half with ordinary ones, alternating -- a long run beside many short ones."""
    rng = np.random.default_rng(4242)
    reads = poly_a_reads(rng, 5000)
    if mixed:
        tiling = fx.recipe_reads(dict(recipe="tiling", seed=4243, n_unique=2500, read_len=150, step=9))
        reads = [r for pair in zip(reads[:2500], tiling) for r in pair]
    bases, off = ascii_reads(reads)
    assert_routes_equal(40, bases, off, monkeypatch, tmp_path, n_unique=5000)


# 4-word and 8-word layouts against the reference's files; g2 with the minimiser groups: 4-dword tuples {K, M, entry, tag} in the table sort
@pytest.mark.parametrize("name,groups", [("g1_clean100_k21", None), ("g2_clean150_k40", None), ("g2_clean150_k40", "1")])
def test_golden_sets_on_both_routes(name, groups, monkeypatch, tmp_path):
    if groups:
        monkeypatch.setenv("SAGE2OV_MINIMIZER_INDEX", groups)
    else:
        monkeypatch.delenv("SAGE2OV_MINIMIZER_INDEX", raising=False)
    m = fx.golden(name)
    bases, off = fx.make_reads(m["synth"])
    assert_routes_equal(m["k"], bases, off, monkeypatch, tmp_path, graph3_of=name)
