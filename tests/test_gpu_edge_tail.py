"""GPU: from the probe's per-read records to the canonical edge list -- the status by position with its copy by id on demand (default) against the copy written
by the reciprocal pass itself (`SAGE2OV_STATUS_EAGER=1`), the one list of unresolved reads per reciprocal pass, and convert's compaction (`k_conv_emit`) at the
edges of its blocks of 2048 candidates: against the reference's golden files, against each other and against the oracle.

The list of unresolved reads has no entry point of its own in the C ABI: it is checked through what is made from it (the hit lists, the replay's and the device
reduction's counters, the edge list) and its length through the exported status."""
import functools

import numpy as np
import pytest

import fixtures as fx
import oracle_lib as ol
import sage2_amd as s2
from test_gpu_parity import assert_equals_oracle
from test_index_one_pass import ascii_reads, edges_equal

pytestmark = pytest.mark.gpu

SWITCH = "SAGE2OV_STATUS_EAGER"
ROUTE_ENVS = ("SAGE2OV_TEST_GENERAL_COLLECT", "SAGE2OV_DEVICE_REDUCE_MIN", "SAGE2OV_HOST_REDUCE")
CONV_BLOCK = 2048                                        # candidates per block of k_conv_emit = items per partial sum of the scan (kernels_scan.inc: SCAN_BLOCK)


def set_route(monkeypatch, env):
    for name in ROUTE_ENVS:
        monkeypatch.delenv(name, raising=False)
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)


def new_ctx(k, bases, off, monkeypatch, eager):
    """an organised context on the default route or on the eager one (the switch is read through Options: set, then reloaded)"""
    if eager:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    ctx = s2.Context(k)
    ctx.options_reload()
    ctx.reads_add_ascii(bases, off)
    ctx.reads_organize()
    return ctx


def circular_tiling(seed, n, read_len, step):
    """n reads that tile a circular genome of n * step bases, strands alternating: every read has both neighbours, so none is unresolved, and every read owns
    exactly one edge -- n candidates, all kept"""
    rng = np.random.default_rng(seed)
    g = fx._rnd(rng, n * step)
    gg = g + g[:read_len]
    reads = [gg[i * step:i * step + read_len] for i in range(n)]
    return ascii_reads([r if x % 2 == 0 else fx.revcomp(r) for x, r in enumerate(reads)])


SETS = {
    "circular1200": lambda: (21, circular_tiling(5, 1200, 100, 5)),
    "cov155x_100_noisy": lambda: (31, fx.make_reads(dict(seed=92, genome_len=9000, n_reads=14000, read_len=100, err_ppm=8000))),
    "unrelated3": lambda: (21, ascii_reads([fx._rnd(np.random.default_rng(900 + x), 100) for x in range(3)])),
}
for _n in (CONV_BLOCK - 1, CONV_BLOCK, CONV_BLOCK + 1):
    SETS[f"circular{_n}"] = functools.partial(lambda n: (21, circular_tiling(40 + n, n, 100, 5)), _n)
SETS["circular5000"] = lambda: (21, circular_tiling(2, 5000, 100, 5))


@functools.lru_cache(maxsize=None)
def reads_of(name):
    if name in SETS:
        k, (bases, off) = SETS[name]()
    else:
        m = fx.golden(name)
        k, (bases, off) = m["k"], fx.make_reads(m["synth"])
    return k, bases, off


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """(finished oracle, its own count of unresolved reads: status 0 after the initial pass, before its reduce phase walks them); shared by the tests, never changed"""
    k, bases, off = reads_of(name)
    o = ol.Oracle(k, threads=8)
    o.add_reads_ascii(bases, off); o.organize(); o.build_index(); o.initial()
    unresolved = int((o.export_initial()[2][1:] == 0).sum())
    o.reduce(); o.convert()
    return o, unresolved


def initial_classes(status):
    """the oracle's reduce phase advances the unresolved reads to 1 / 2: the classes of the initial pass"""
    return np.where(np.isin(status, (1, 2)), 0, status)


def assert_status_is_oracles(ctx, o):
    gs, os_ = ctx.overlap_export_initial()[2], o.export_initial()[2]
    assert np.array_equal(initial_classes(gs[1:]), initial_classes(os_[1:]))
    return gs


def both_routes(name, monkeypatch, env=None):
    """steps 2-3 on both status routes: [(edges, exported records)], default route first; each equal to the oracle's"""
    k, bases, off = reads_of(name)
    o, _ = oracle_of(name)
    set_route(monkeypatch, env)
    out = []
    for eager in (False, True):
        ctx = new_ctx(k, bases, off, monkeypatch, eager)
        ctx.run_steps23()
        assert_equals_oracle(ctx, o)
        assert_status_is_oracles(ctx, o)
        out.append((ctx, ctx.edges(), ctx.overlap_export_initial()))
    return out


def close_routes(out, monkeypatch):
    for ctx, _, _ in out:
        ctx.close()
    monkeypatch.delenv(SWITCH, raising=False)
    set_route(monkeypatch, None)


GENERAL, DEVICE, HOST = {"SAGE2OV_TEST_GENERAL_COLLECT": "1"}, {"SAGE2OV_DEVICE_REDUCE_MIN": "1"}, {"SAGE2OV_HOST_REDUCE": "1"}


# what each case takes, by the oracle's count of unresolved reads (lo <= count <= hi): a handful (<= 1024: the short-list collect of the host replay, which the
# default route takes below 4096 unresolved reads), the general collect, the device reduce (g4: long buckets, its ranked form), the host replay of many reads
@pytest.mark.parametrize("name,env,lo,hi", [
    ("g2_clean150_k40", None, 1, 1024), ("g1_clean100_k21", HOST, 1, 1024), ("g7_palindrome_tandem_k21", None, 1, 1024), ("g11_freqwrap_k21", HOST, 1, 1024),
    ("g12_lowcomplexity_k21", None, 1, 1024),
    ("g2_clean150_k40", GENERAL, 1, 1024), ("g13_noisy300_k55", HOST, 1025, 1 << 20),
    ("g3_noisy_rep_k21", DEVICE, 4096, 1 << 20), ("g4_highcopy_k21", DEVICE, 4096, 1 << 20), ("g13_noisy300_k55", None, 4096, 1 << 20),
    ("g3_noisy_rep_k21", HOST, 4096, 1 << 20),
])
def test_both_status_routes_reproduce_the_golden_files(name, env, lo, hi, tmp_path, monkeypatch):
    _, unresolved = oracle_of(name)
    assert lo <= unresolved <= hi
    out = both_routes(name, monkeypatch, env)
    for x, (ctx, _, _) in enumerate(out):
        gp = str(tmp_path / f"t{x}.graph3")
        ctx.graph_save(gp)
        assert fx.graph3_matches(gp, name)
    assert edges_equal(out[0][1], out[1][1])
    assert all(np.array_equal(a, b) for a, b in zip(out[0][2], out[1][2]))
    close_routes(out, monkeypatch)


@pytest.mark.parametrize("name,env", [("g2_clean150_k40", None), ("g13_noisy300_k55", DEVICE), ("g3_noisy_rep_k21", HOST), ("g4_highcopy_k21", DEVICE)])
def test_status_by_id_after_everything_that_can_change_it(name, env, monkeypatch):
    """the exported status after the initial pass, after the reduce phase and after a second run of steps 2-3 on the same context: the eager route's, and the oracle's"""
    k, bases, off = reads_of(name)
    o, unresolved = oracle_of(name)
    set_route(monkeypatch, env)
    seen = []
    for eager in (False, True):
        ctx = new_ctx(k, bases, off, monkeypatch, eager)
        ctx.index_build(); ctx.overlap_initial()
        st = [assert_status_is_oracles(ctx, o)]
        ctx.overlap_reduce()
        st.append(assert_status_is_oracles(ctx, o))
        ctx.overlap_convert()
        ctx.run_steps23()
        st.append(assert_status_is_oracles(ctx, o))
        assert_equals_oracle(ctx, o)
        assert all(int((s[1:] == 0).sum()) == unresolved for s in st)
        seen.append(st); ctx.close()
    assert all(np.array_equal(a, b) for a, b in zip(seen[0], seen[1]))
    monkeypatch.delenv(SWITCH, raising=False); set_route(monkeypatch, None)


@pytest.mark.parametrize("name,want,env", [("circular1200", 0, None), ("circular1200", 0, HOST), ("g2_clean150_k40", 2, None), ("g2_clean150_k40", 2, HOST),
                                           ("g2_clean150_k40", 2, DEVICE)])
def test_unresolved_list_of_none_and_of_two(name, want, env, monkeypatch):
    """no unresolved read (nothing is launched for the list) and two: the default route lists them once in the device reduce's entry and hands the same list to the
    host replay, SAGE2OV_HOST_REDUCE lists them in the replay's own call, the device reduce consumes the list where it stands"""
    o, unresolved = oracle_of(name)
    assert unresolved == want
    out = both_routes(name, monkeypatch, env)
    for _, _, (_, _, status, _) in out:
        assert len(np.flatnonzero(status[1:] == 0)) == want
    assert edges_equal(out[0][1], out[1][1])
    close_routes(out, monkeypatch)


# seed 7, 1.3 M reads of 100 bases, 0.8 % errors, k = 31: what the oracle computes (a minute on the host, so recorded here instead of run by the test)
BIG = dict(seed=7, genome_len=2_600_000, n_reads=1_300_000, read_len=100, err_ppm=8000)
BIG_ORACLE = dict(N=1239447, unresolved=1239270, long_buckets=0, edges=2259584, n_ov=28453774, edges_inserted=28451622, transitive_removed=23933142)


def test_unresolved_list_beyond_2_to_20():
    """more unresolved reads than the 2^20 the list used to have room for at first: the list is sized by the reciprocal pass's count"""
    assert BIG_ORACLE["unresolved"] > 1 << 20
    bases, off = fx.make_reads(BIG)
    ctx = s2.Context(31)
    ctx.reads_add_ascii(bases, off); ctx.reads_organize(); ctx.run_steps23()
    status = ctx.overlap_export_initial()[2]
    assert ctx.reads_stats().unique_reads == BIG_ORACLE["N"] and ctx.index_stats().long_buckets == BIG_ORACLE["long_buckets"]
    assert len(np.flatnonzero(status[1:] == 0)) == BIG_ORACLE["unresolved"]
    st = ctx.overlap_stats()
    assert (st.edges, st.verified_overlaps) == (BIG_ORACLE["edges"], BIG_ORACLE["n_ov"])
    # the hit lists are those of the listed reads, and every hit is an inserted edge (no long bucket: the device reduce's unranked form)
    assert st.unresolved_hits == st.edges_inserted == BIG_ORACLE["edges_inserted"] and st.transitive_removed == BIG_ORACLE["transitive_removed"]
    ctx.close()


@pytest.mark.parametrize("n", [CONV_BLOCK - 1, CONV_BLOCK, CONV_BLOCK + 1])
def test_convert_one_block_exactly_one_more_and_one_less(n, monkeypatch):
    name = f"circular{n}"
    o, unresolved = oracle_of(name)
    assert unresolved == 0 and o.counter("N") == n and o.counter("edges") == n
    out = both_routes(name, monkeypatch)
    assert out[0][0].shard_edges_count() == n                     # candidates: one per read, none dropped
    close_routes(out, monkeypatch)


def test_convert_without_candidates(monkeypatch):
    o, _ = oracle_of("unrelated3")
    assert o.counter("N") == 3 and o.counter("edges") == 0
    out = both_routes("unrelated3", monkeypatch)
    assert out[0][0].shard_edges_count() == 0 and len(out[0][1]) == 0
    close_routes(out, monkeypatch)


def test_convert_run_across_a_block_edge(monkeypatch):
    """5000 candidates, all kept, so the oracle's edge list is the sorted candidate list: a read whose list of two starts at the last entry of a block and ends in
    the next one"""
    o, unresolved = oracle_of("circular5000")
    frm = o.export_edges()[:, 0]
    assert unresolved == 0 and len(frm) == 5000
    assert frm[CONV_BLOCK - 2] != frm[CONV_BLOCK - 1] == frm[CONV_BLOCK]
    out = both_routes("circular5000", monkeypatch)
    assert out[0][0].shard_edges_count() == 5000
    close_routes(out, monkeypatch)


@pytest.mark.parametrize("name,env", [("cov155x_100_noisy", None), ("cov155x_100_noisy", HOST), ("g8_noisy250_k45", None)])
def test_convert_long_lists_across_many_block_edges(name, env, monkeypatch):
    """155x of 100-base reads with 0.8 % errors, and 250-base reads with errors: the reduce phase leaves lists of 16 and more entries per read, in a candidate
    list of many blocks (the clean high-coverage sets have two candidates per read at most)"""
    o, _ = oracle_of(name)
    frm = o.export_edges()[:, 0]
    assert len(frm) > 4 * CONV_BLOCK and np.unique(frm, return_counts=True)[1].max() >= 16
    out = both_routes(name, monkeypatch, env)
    assert out[0][0].shard_edges_count() >= len(frm)
    assert edges_equal(out[0][1], out[1][1])
    close_routes(out, monkeypatch)
