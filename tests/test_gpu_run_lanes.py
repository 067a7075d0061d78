"""GPU: run mode of the fast probe kernel with a lane per read of a step (kernels_probe_fast.inc: the plan of a step, its own-entry checks and its records computed
with lane r = read r) against the loops over the reads it replaces: the oracle's extension records, connection counts, edges and counters with the
library's threshold, with the loops everywhere (SAGE2OV_RUN_LANES=0) and with every planned step in the lane form (SAGE2OV_RUN_LANES_MIN=1), and the kernel's own
run counters (Context.probe_run_stats) to show that the lane form ran where it should and that the route -- reads per step, steps -- is the same every way."""
import numpy as np
import pytest

import fixtures as fx
import sage2_amd as s2
from test_gpu_parity import run_gpu, run_oracle, assert_equals_oracle

pytestmark = pytest.mark.gpu


def tandem_reads(seed=195, genome_len=20000, n_reads=12000, read_len=150, unit="ACGTTGA", units=12, every=1000):
    """reads at random positions and strands of a random genome that carries `units` copies of a 7-base unit every `every` bases: a read inside a stretch of them has
    its own prefix key again at later windows, and the windows of the stretch hold several left- and right-type entries each"""
    rng = np.random.default_rng(seed)
    g = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=genome_len)].copy()
    rep = np.frombuffer((unit * units).encode(), dtype=np.uint8)
    for p in range(every // 2, genome_len - len(rep), every):
        g[p:p + len(rep)] = rep
    comp = np.zeros(256, dtype=np.uint8); comp[list(b"ACGT")] = list(b"TGCA")
    starts = rng.integers(0, genome_len - read_len + 1, size=n_reads); rc = rng.integers(0, 2, size=n_reads).astype(bool)
    reads = g[starts[:, None] + np.arange(read_len)[None, :]]
    reads[rc] = comp[reads[rc]][:, ::-1]
    return reads.reshape(-1).copy(), np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(read_len)


SHAPES = {
    # 50x, clean: the ordinary mix of 1 to about 8 reads per step, strand changes by mirroring
    "cov50": (dict(seed=191, genome_len=90000, n_reads=30000, read_len=150, err_ppm=0), 40),
    # 90x: steps that reach RUN_MMAX reads, plans cut by RUN_DMAX, rings near 128 slots that wrap
    "cov90": (dict(seed=192, genome_len=50000, n_reads=30000, read_len=150, err_ppm=0), 40),
    # 100x of 100-base reads: the 4-word layout and the wide form, which keeps its loops
    "wide100": (dict(seed=193, genome_len=40000, n_reads=40000, read_len=100, err_ppm=0), 21),
    # tandem repeats: own entries in foreign windows, windows with several left- and right-type slots (both tie rules)
    "tandem": (None, 40),
    # the first shape with a read error now and then: runs that end and restart, steps shortened after the plan was made
    "err60": (dict(seed=191, genome_len=90000, n_reads=30000, read_len=150, err_ppm=60), 40),
}
SETTINGS = {"default": {}, "loops": {"SAGE2OV_RUN_LANES": "0"}, "lanes_min_1": {"SAGE2OV_RUN_LANES_MIN": "1"}}


@pytest.fixture(scope="module")
def inputs():
    """reads and finished oracle of a shape, made once for the three settings"""
    cache = {}

    def get(shape):
        if shape not in cache:
            pd, k = SHAPES[shape]
            bases, off = tandem_reads() if pd is None else fx.make_reads(pd)
            cache[shape] = (dict(k=k), bases, off, run_oracle(dict(k=k), bases, off))
        return cache[shape]
    yield get
    for c in cache.values():
        c[3].close()


def set_switches(monkeypatch, setting):
    monkeypatch.delenv("SAGE2OV_MINIMIZER_INDEX", raising=False)          # (the library's own route on small inputs)
    monkeypatch.setenv("SAGE2OV_PROBE_SAMPLE_MIN", "2048")               # (sample launch, the rest and the listed reads all run their forms)
    for name in ("SAGE2OV_RUN_LANES", "SAGE2OV_RUN_LANES_MIN"):
        monkeypatch.delenv(name, raising=False)
    for name, v in SETTINGS[setting].items():
        monkeypatch.setenv(name, v)


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_records_with_a_lane_per_read_equal_the_oracle(shape, setting, inputs, monkeypatch):
    set_switches(monkeypatch, setting)
    m, bases, off, o = inputs(shape)
    g = run_gpu(m, bases, off)
    assert_equals_oracle(g, o)
    first = g.probe_run_stats()
    g.run_steps23(); assert_equals_oracle(g, o)                            # (a second pass over the resident reads)
    assert g.probe_run_stats() == first                                    # (the counters are those of the last pass, not a running sum)
    g.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_run_counters_show_the_lane_form_and_one_route(shape, inputs, monkeypatch):
    """reads off the ring and steps are the same with every setting; the lane form answers steps of several reads by default and none when switched off"""
    m, bases, off, _ = inputs(shape)
    st = {}
    for setting in SETTINGS:
        set_switches(monkeypatch, setting)
        g = run_gpu(m, bases, off); st[setting] = g.probe_run_stats(); g.close()
    print(shape, st)
    reads, steps = st["default"][:2]
    assert steps > 0 and reads >= steps
    assert st["loops"][:2] == (reads, steps) and st["lanes_min_1"][:2] == (reads, steps)
    assert st["loops"][2:] == (0, 0)
    if shape in ("cov50", "cov90"):
        lane_reads, lane_steps = st["default"][2:]
        assert lane_steps > 0 and lane_reads >= 2 * lane_steps
        assert st["lanes_min_1"][3] >= lane_steps and st["lanes_min_1"][2] >= lane_reads
