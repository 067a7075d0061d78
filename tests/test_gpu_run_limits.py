"""GPU: run mode of the fast probe kernel (kernels_probe_fast.inc) on reads built to sit ON its limits (tests/rungen.py: planted minimisers decide the
locality order, so the test decides which read follows which, at which shift and on which strand).  Every case, under every run setting and on both look-up routes:
the oracle's extension records, connection counts, edges and counters, exactly; the kernel's run counters (Context.probe_run_stats) equal to the route model's, which
tests/test_rungen_host.py shows to have the property the case is named after; a second pass over the resident reads with the same records and counters.

SAGE2OV_PROBE_TAIL=0: one launch of the sequential-groups clean form, the only one with run mode, over all positions (visits of 32 positions: chunkShift 7, four waves
per block); the reads it lists go through the passes behind it, so those are part of the result.  The cases and the families A - H they belong to: rungen.CASES."""
import pytest

import rungen as rg
import sage2_amd as s2
from test_gpu_parity import run_gpu, run_oracle, assert_equals_oracle

pytestmark = pytest.mark.gpu

SETTINGS = {"default": {}, "loops": {"SAGE2OV_RUN_LANES": "0"}, "lanes_min_1": {"SAGE2OV_RUN_LANES_MIN": "1"}, "run_mode_off": {"SAGE2OV_NO_RUN_MODE": "1"}}
LANES_MIN = {"default": rg.RUN_LANES_MIN, "loops": 0, "lanes_min_1": 1}
SWITCHES = ("SAGE2OV_RUN_LANES", "SAGE2OV_RUN_LANES_MIN", "SAGE2OV_NO_RUN_MODE", "SAGE2OV_MINIMIZER_INDEX", "SAGE2OV_PROBE_SAMPLE_MIN", "SAGE2OV_PROBE_SEQ", "SAGE2OV_FAST_CHUNK_SHIFT")


@pytest.fixture(scope="module")
def inputs():
    """reads, finished oracle and model of a case, made once for all settings"""
    cache = {}

    def get(name):
        if name not in cache:
            c = rg.get_case(name); bases, off = c.arrays()
            cache[name] = (dict(k=c.k), bases, off, run_oracle(dict(k=c.k), bases, off), c.model())
        return cache[name]
    yield get
    for c in cache.values():
        c[3].close()


def set_switches(monkeypatch, setting, groups):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SAGE2OV_PROBE_TAIL", "0")
    monkeypatch.setenv("SAGE2OV_MINIMIZER_INDEX", "1" if groups else "0")
    for name, v in SETTINGS[setting].items():
        monkeypatch.setenv(name, v)


def expected(model, setting):
    return (0, 0, 0, 0) if setting == "run_mode_off" else model.route(LANES_MIN[setting])[0]


@pytest.mark.parametrize("groups", [False, True], ids=["uniform_table", "minimiser_groups"])
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("case", list(rg.CASES))
def test_records_equal_the_oracle_and_the_route_is_the_models(case, setting, groups, inputs, monkeypatch):
    set_switches(monkeypatch, setting, groups)
    m, bases, off, o, model = inputs(case)
    g = run_gpu(m, bases, off)
    assert_equals_oracle(g, o)
    first = g.probe_run_stats(); want = expected(model, setting)
    print(case, setting, groups, "run counters", first, "model", want)
    assert first == want
    if setting == "loops":
        assert first[2:] == (0, 0)
    g.run_steps23(); assert_equals_oracle(g, o)                            # (a second pass over the resident reads)
    assert g.probe_run_stats() == first
    g.close()


@pytest.mark.parametrize("case", list(rg.CASES))
def test_reads_and_steps_are_the_same_under_the_three_run_settings(case, inputs, monkeypatch):
    m, bases, off, o, model = inputs(case)
    st = {}
    for setting in SETTINGS:
        set_switches(monkeypatch, setting, False)
        g = run_gpu(m, bases, off); st[setting] = g.probe_run_stats(); g.close()
    print(case, st)
    assert st["run_mode_off"] == (0, 0, 0, 0)
    assert st["default"][:2] == st["loops"][:2] == st["lanes_min_1"][:2] == expected(model, "default")[:2]
    assert st["loops"][2:] == (0, 0)
    assert st["lanes_min_1"][2] >= st["default"][2] and st["lanes_min_1"][3] >= st["default"][3]
    if not model.capable():
        assert st["default"] == (0, 0, 0, 0)
