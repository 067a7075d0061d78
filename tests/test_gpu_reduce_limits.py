"""GPU: the reduce phase (kernels_reduce.inc, the reduce_* stages of sage2ov_device.hip) on read sets built to sit ON its list limits (tests/redgen.py:
fans of planted reads decide how long every list is).  Every case on every reduce path of tests/test_gpu_parity.py: the oracle's edges, counters and per-read records,
exactly; Context.reduce_stats() -- which form ran, how many lists went to which size class, what the short cut did, the removals -- equal to the case's model, which
tests/test_redgen_host.py shows to have the property the case is named after; a second pass over the resident reads with the same edges and the same stats.

The mixed case again with the marks' grid bound to 1 and 3 blocks (SAGE2OV_TEST_MARK_BLOCKS: four waves walk every read, so the prefetch rotation of the first size class
and the loop over mid[] of the second run many iterations), with the potential lists in slices, with undersized buffers and with the marks shared by two contexts."""
import numpy as np
import pytest

import redgen as rd
import sage2_amd as s2
from test_gpu_parity import run_gpu, run_oracle, assert_equals_oracle, reduce_path, _Hip      # noqa: F401 (reduce_path: the fixture)

pytestmark = pytest.mark.gpu

SWITCHES = ("SAGE2OV_TEST_MARK_BLOCKS", "SAGE2OV_TEST_RANK_SLICE", "SAGE2OV_TEST_SMALL_BUFFERS", "SAGE2OV_TEST_GENERAL_COLLECT")


@pytest.fixture(scope="module")
def inputs():
    """reads, finished oracle and model of a case, made once for all paths"""
    cache = {}

    def get(name):
        if name not in cache:
            c = rd.get_case(name); bases, off = c.arrays()
            o = run_oracle(dict(k=c.k), bases, off)
            cache[name] = (dict(k=c.k), bases, off, o, c.model(o))
        return cache[name]
    yield get
    for c in cache.values():
        c[3].close()


def assert_stats(got, want):
    """every counter the model fixes (None: left open, see redgen.Model.stats)"""
    assert {n: v for n, v in got.items() if want[n] is not None} == {n: v for n, v in want.items() if v is not None}


@pytest.mark.parametrize("case", list(rd.CASES))
def test_edges_equal_the_oracle_and_the_stats_are_the_models(case, reduce_path, inputs, monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    m, bases, off, o, model = inputs(case)
    g = run_gpu(m, bases, off)
    assert_equals_oracle(g, o)
    first, want = g.reduce_stats(), model.stats(reduce_path)
    print(case, reduce_path, "reduce stats", first, "model", want)
    assert want["removed"] == o.counter("transitive_removed")
    assert_stats(first, want)
    if reduce_path == "host":
        assert first["form"] in (0, 3)
    if reduce_path == "device_walk":
        assert (first["shortcut_lists"], first["shortcut_reads"]) == (0, 0)
    e1 = g.edges().tobytes()
    g.run_steps23(); assert_equals_oracle(g, o)                            # (a second pass over the resident reads)
    assert g.reduce_stats() == first and g.edges().tobytes() == e1
    g.close()


@pytest.fixture(scope="module")
def plain(inputs):
    """the mixed case on the device form with nothing else set: edges and stats the other settings must reproduce"""
    import os
    m, bases, off, o, model = inputs("mixed")
    keep = {n: os.environ.pop(n, None) for n in SWITCHES + ("SAGE2OV_HOST_REDUCE", "SAGE2OV_RA_NO_SHORTCUT", "SAGE2OV_DEVICE_REDUCE_MIN")}
    os.environ["SAGE2OV_DEVICE_REDUCE_MIN"] = "1"
    try:
        g = run_gpu(m, bases, off)
        assert_equals_oracle(g, o)
        res = (g.edges().tobytes(), g.reduce_stats())
        g.close()
    finally:
        del os.environ["SAGE2OV_DEVICE_REDUCE_MIN"]
        for n, v in keep.items():
            if v is not None:
                os.environ[n] = v
    assert res[1]["form"] == 2 and res[1]["slices"] == 1
    return res


@pytest.mark.parametrize("switch,value", [("SAGE2OV_TEST_MARK_BLOCKS", "1"), ("SAGE2OV_TEST_MARK_BLOCKS", "3"), ("SAGE2OV_TEST_RANK_SLICE", "1024"), ("SAGE2OV_TEST_SMALL_BUFFERS", "1")])
def test_mixed_case_under_a_bound_grid_slices_and_small_buffers(switch, value, inputs, plain, monkeypatch):
    for name in SWITCHES + ("SAGE2OV_HOST_REDUCE", "SAGE2OV_RA_NO_SHORTCUT"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SAGE2OV_DEVICE_REDUCE_MIN", "1"); monkeypatch.setenv(switch, value)
    m, bases, off, o, model = inputs("mixed")
    g = run_gpu(m, bases, off)
    st = g.reduce_stats()
    print(switch, value, st)
    assert g.edges().tobytes() == plain[0]
    assert_equals_oracle(g, o)
    if switch == "SAGE2OV_TEST_RANK_SLICE":
        assert st["slices"] >= 3
    assert {n: v for n, v in st.items() if n != "slices"} == {n: v for n, v in plain[1].items() if n != "slices"}
    if switch != "SAGE2OV_TEST_RANK_SLICE":
        assert st["slices"] == plain[1]["slices"]
    g.close()


def test_mixed_case_with_the_marks_shared_by_two_contexts(inputs, plain, monkeypatch):
    """world = 2 on one GPU, the collectives replaced by concatenation (as test_sharded_contexts_on_one_gpu_match_reference drives it): a rank's share [wlo, whi) of the
    unresolved reads cuts through the gadgets.  Every rank ends with the plain run's edges; the counters of the marks add up to the plain run's, the others are equal."""
    from sage2_amd.shard import RECORD_BYTES, EDGE_BYTES, shard_range, max_shard
    for name in SWITCHES + ("SAGE2OV_HOST_REDUCE", "SAGE2OV_RA_NO_SHORTCUT"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SAGE2OV_DEVICE_REDUCE_MIN", "1")
    m, bases, off, o, model = inputs("mixed")
    world, hip, ctxs = 2, _Hip(), []
    for r in range(world):
        c = s2.Context(m["k"], device=0, rank=r, world=world)
        c.reads_add_ascii(bases, off); c.reads_organize(); c.index_build(); c.overlap_probe_shard()
        ctxs.append(c)
    n = ctxs[0].reads_stats().unique_reads
    ms = max_shard(n, world)
    sends, planes = [], []
    for c in ctxs:
        p = hip.alloc(ms * RECORD_BYTES); c.shard_export_records(p, ms); sends.append(p)
        q = hip.alloc(c.shard_flags_bytes()); c.shard_export_flags(q); planes.append(hip.to_host(q, c.shard_flags_bytes()))
    orp = hip.to_dev(np.maximum.reduce(planes))
    for c in ctxs:
        for r in range(world):
            lo, hi = shard_range(n, r, world)
            if hi > lo:
                c.shard_import_records(sends[r], lo, hi - lo)
        c.shard_import_flags(orp)
        c.overlap_reciprocal()
    parts = []
    for c in ctxs:
        ne = c.shard_edges_count()
        p = hip.alloc(max(ne, 1) * EDGE_BYTES); c.shard_edges_export(p, max(ne, 1)); parts.append(hip.to_host(p, ne * EDGE_BYTES))
    allb = np.concatenate(parts); total = allb.size // EDGE_BYTES
    dall = hip.to_dev(allb)
    sparts, removed, stats = [], 0, []
    for c in ctxs:
        c.shard_edges_set(dall if total else 0, total)
        c.overlap_reduce()
        stats.append(c.reduce_stats())
        ns, rem = c.shard_survivors_count(); removed += rem
        p = hip.alloc(max(ns, 1) * EDGE_BYTES); c.shard_survivors_export(p, max(ns, 1)); sparts.append(hip.to_host(p, ns * EDGE_BYTES))
    alls = np.concatenate(sparts); stotal = alls.size // EDGE_BYTES
    dsurv = hip.to_dev(alls)
    print("ranks", stats, "plain", plain[1])
    assert removed == plain[1]["removed"] == o.counter("transitive_removed")
    for name in ("form", "unresolved", "potential_over_1024", "slices"):
        assert [st[name] for st in stats] == [plain[1][name]] * world
    for name in ("lists_over_128", "lists_over_512", "shortcut_lists", "shortcut_reads", "removed"):
        assert sum(st[name] for st in stats) == plain[1][name]
    for c in ctxs:
        c.shard_survivors_set(dsurv if stotal else 0, stotal, removed)
        c.overlap_convert()
        assert c.edges().tobytes() == plain[0]
        c.close()
    hip.free()
