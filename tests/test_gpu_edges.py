"""GPU: the input edges the read generator (synth.cpp) never reaches -- unique-read counts at the kernels' own boundaries, the shortest legal reads, low-complexity
sequence, frequencies past the reference's 16-bit counter, read sets that follow one another in one process.  Every case runs the HIP path through the C ABI and
the oracle on the same hand-made input (tests/fixtures.py: recipes) and compares what assert_equals_oracle compares (connection counts, extension records, the
canonical edge list with both lengths, reduce counters, N_ov) plus the read store; and every case asserts that its input really sits on the edge it is named for."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (this module is also the script of its own fresh-process child)
import fixtures as fx                                                                # noqa: E402
import oracle_lib as ol                                                              # noqa: E402
import sage2_amd as s2                                                               # noqa: E402
from test_gpu_parity import (GROUPS_FORM_MODES, PROBE_KERNEL_MODES, assert_equals_oracle, force_groups_form, force_probe_kernel,     # noqa: E402
                             reduce_path, run_gpu, run_oracle)      # noqa: F401  (reduce_path: the fixture, used by name)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("minimiser_groups_on")]      # (small inputs: the groups' half of the look-up code is exercised by request, conftest.py)


def assert_reads_equal_oracle(ctx, o):
    """step 1: ids (= row order), packed bytes, lengths and frequencies of the read store"""
    gp, gl, gf = ctx.reads_export(); op, ol_, of = o.export_reads()
    w = min(gp.shape[1], op.shape[1])
    assert ctx.reads_stats().unique_reads == o.counter("N")
    assert np.array_equal(gl, ol_) and np.array_equal(gf, of) and np.array_equal(gp[:, :w - 1], op[:, :w - 1])


def result_digest(ctx):
    """one md5 over everything a finished context exports: edges, per-read records, read store, counters"""
    h = hashlib.md5(ctx.edges().tobytes())
    for a in ctx.overlap_export_initial() + ctx.reads_export():
        h.update(np.ascontiguousarray(a).tobytes())
    st = ctx.overlap_stats()
    h.update(repr((st.verified_overlaps, st.contained_extension, st.contained_size, st.left_to_explore, st.edges_inserted, st.transitive_removed, st.edges)).encode())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------------- unique-read counts at the kernels' boundaries
COUNT_BOUNDARIES = [
    (1, "a single read"), (2, "one pair"), (3, "the smallest transitive triple"),
    (63, "wave - 1"), (64, "one wave of 64 lanes"), (65, "wave + 1"),
    (127, "FAST_CHUNK - 1"), (128, "FAST_CHUNK: a probe block's visit with chunk_shift 7"), (129, "FAST_CHUNK + 1"),
    (255, "block - 1"), (256, "a 256-thread block = a probe block's visit with chunk_shift 8 = ORG_RUN_LIMIT"), (257, "block + 1"),
    (511, "IX_W / 8 - 1"), (512, "IX_W / 8: 8 N slots fill exactly one table window; 4 N keys = IX_GW"), (513, "IX_W / 8 + 1: a second table window"),
    (1023, "IX_W / 4 - 1"), (1024, "IX_W / 4: 4 N keys = IX_W; PT_SC_THREADS"), (1025, "IX_W / 4 + 1"),
    (2047, "tile - 1"), (2048, "RS_TILE = SCAN_BLOCK = IX_GW = 256 x COND_PER_THREAD reads; 4 N = PT_TILE tuples"), (2049, "tile + 1"),
    (3071, "FEW_MAX - 1"), (3072, "FEW_MAX = IXW_CSR_CAP = IXW_T x IXW_R"), (3073, "FEW_MAX + 1"),
    (4095, "IX_W - 1"), (4096, "IX_W = 256 x EMIT_PER_THREAD = 256 x UNRES_PER_THREAD reads"), (4097, "IX_W + 1"),
    (8191, "PT_TILE - 1"), (8192, "PT_TILE = S4_WALK_CAP reads"), (8193, "PT_TILE + 1"),
]
COUNT_SHAPES = [(100, 21, 7), (150, 40, 9)]                         # (read length, k, tiling step)


@pytest.mark.parametrize("route", ["default", "memory_diet"])
@pytest.mark.parametrize("L,k,step", COUNT_SHAPES, ids=["L100k21", "L150k40"])
@pytest.mark.parametrize("n", [c[0] for c in COUNT_BOUNDARIES])
def test_unique_read_counts_at_kernel_boundaries(n, L, k, step, route, monkeypatch):
    """EXACTLY n unique reads (a tiling, every fifth read given twice more), n at and one either side of the sizes the kernels are cut by (COUNT_BOUNDARIES names
    the constant of kernels_*.inc / sage2ov_device.hip beside each), in the default route and in memory-diet mode; a second run_steps23() on the same context gives
    the same bytes."""
    if route == "memory_diet":
        monkeypatch.setenv("SAGE2OV_MEMORY_DIET", "1")
    else:
        monkeypatch.delenv("SAGE2OV_MEMORY_DIET", raising=False)
    bases, off = fx.make_reads(dict(recipe="tiling", seed=1000 + n, n_unique=n, read_len=L, step=step, dup_every=5, dup_copies=2))
    m = dict(k=k)
    g, o = run_gpu(m, bases, off), run_oracle(m, bases, off)
    assert g.reads_stats().unique_reads == n == o.counter("N")                     # the edge itself
    assert_reads_equal_oracle(g, o)
    assert_equals_oracle(g, o)
    assert (len(g.edges()) > 0 and o.counter("n_ov") > 0) if n >= 2 else len(g.edges()) == 0
    first = result_digest(g)
    g.run_steps23()
    assert result_digest(g) == first
    assert_equals_oracle(g, o)
    g.close(); o.close()


# ---------------------------------------------------------------------------------------------------------------- the shortest legal reads
LAYOUT_TOPS = [(123, 4), (251, 8), (504, 16), (1018, 32)]           # (longest read of the layout, words per read)


@pytest.mark.parametrize("top,words", LAYOUT_TOPS, ids=[f"top{t}" for t, _ in LAYOUT_TOPS])
@pytest.mark.parametrize("k", [15, 21, 32, 33, 64, 70])
def test_shortest_legal_reads_next_to_the_longest_of_a_layout(k, top, words):
    """Reads of k + 1, k + 2 and k + 3 bases -- a good read is longer than k, so k + 1 is the shortest there is: two windows, prefix and suffix key overlapping in all
    but one base (k = 70: h = 64, eight windows) -- in one set with reads up to the longest of each read-store layout."""
    bases, off = fx.make_reads(dict(recipe="short_reads", seed=2000 + k + top, k=k, top=top, step=5, n_reads=1500))
    m = dict(k=k)
    g, o = run_gpu(m, bases, off), run_oracle(m, bases, off)
    _, ln, _ = o.export_reads()
    st = g.reads_stats()
    assert st.words_per_read == words and st.max_read_length == top == int(ln.max())
    for L in (k + 1, k + 2, k + 3):
        assert int((ln[1:] == L).sum()) >= 50, f"too few reads of {L} bases in the store"
    assert int(ln[1:].min()) == k + 1                                               # L - h + 1 = 2 windows for k <= 64
    assert_reads_equal_oracle(g, o)
    assert_equals_oracle(g, o)
    assert len(g.edges()) > 0 and g.overlap_stats().contained_extension > 0
    g.close(); o.close()


# ---------------------------------------------------------------------------------------------------------------- low complexity
LOW_COMPLEXITY_SHAPES = [(100, 21), (150, 40), (250, 31), (300, 55), (600, 31)]


def low_complexity_params(L, step=2):
    return dict(recipe="low_complexity", seed=3000 + L, read_len=L, block=2 * L, flank=400, step=step)


def assert_low_complexity_edges_hit(g, o, bases, off, k):
    """the input is what it claims: the homopolymer key is a long bucket, many reads carry a key twice and more, some reads equal their own reverse complement"""
    assert g.index_stats().long_buckets == o.counter("long_buckets") > 0
    h = min(k, 64)
    seqs = [bytes(bases[int(off[i]):int(off[i + 1])]).decode() for i in range(0, len(off) - 1, 3)]
    repeated = sum(1 for s in seqs if len({s[j:j + h] for j in range(len(s) - h + 1)}) < len(s) - h + 1)
    assert repeated > 100, "reads with a key at two and more of their own windows"
    assert any(s == fx.revcomp(s) for s in seqs if set(s) == {"A", "T"}), "an (AT)n read equal to its own reverse complement"
    assert any(set(s) == {"A"} for s in seqs) and any(set(s) == {"T"} for s in seqs)
    _, _, fr = o.export_reads()
    assert int(fr.max()) > 10                                                       # the reads inside a block collapse to a few


@pytest.mark.parametrize("run_mode", ["on", "off"])
@pytest.mark.parametrize("L,k", LOW_COMPLEXITY_SHAPES)
def test_low_complexity_sequence_matches_oracle(L, k, run_mode, reduce_path, monkeypatch):
    """poly-A / poly-T, (AT)n and microsatellites of period 2, 3 and 6, each longer than a read (fixtures.LOW_COMPLEXITY_UNITS), in all four read-store layouts, with
    every form of the reduce phase and with run mode on and off"""
    if run_mode == "off":
        monkeypatch.setenv("SAGE2OV_NO_RUN_MODE", "1")
    bases, off = fx.make_reads(low_complexity_params(L))
    m = dict(k=k)
    g, o = run_gpu(m, bases, off), run_oracle(m, bases, off)
    assert_low_complexity_edges_hit(g, o, bases, off, k)
    assert_reads_equal_oracle(g, o)
    assert_equals_oracle(g, o)
    assert len(g.edges()) > 0
    g.close(); o.close()


@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("form", ["probe:" + x for x in PROBE_KERNEL_MODES] + ["groups:" + x for x in GROUPS_FORM_MODES])
def test_low_complexity_sequence_in_every_forced_kernel_form(form, step, monkeypatch):
    """the 150-base shape through the forms that test_probe_kernel_choice_is_exact and test_sequential_groups_form_and_wide_pass_are_exact force (their switch
    tables, imported), tiled at step 1 (150x) and 3"""
    kind, mode = form.split(":")
    (force_probe_kernel if kind == "probe" else force_groups_form)(mode, monkeypatch)
    bases, off = fx.make_reads(low_complexity_params(150, step))
    m = dict(k=40)
    g, o = run_gpu(m, bases, off), run_oracle(m, bases, off)
    assert_low_complexity_edges_hit(g, o, bases, off, 40)
    assert_equals_oracle(g, o)
    assert len(g.edges()) > 0
    g.close(); o.close()


# ---------------------------------------------------------------------------------------------------------------- frequency wrap
def test_frequencies_wrap_at_16_bits_like_the_reference(tmp_path, monkeypatch):
    """Three reads given 65 535, 65 536 and 65 537 times: the reference counts in a uint16_t (readLoader.cpp:232), so P.reads says 65 535, 0 and 1.  The device
    organiser (k_org_gather), the host organiser and the oracle each restate that: ids, lengths, frequencies, packed bytes and the P.reads file must be the same
    three times.  (tests/golden/g11_freqwrap_k21 pins the same wrap on the reference binary itself.)"""
    pd = dict(recipe="heavy_duplicates", seed=11, n_unique=600, read_len=100, step=7)
    bases, off = fx.make_reads(pd)
    out = {}
    for mode in ("device", "host"):
        if mode == "host":
            monkeypatch.setenv("SAGE2OV_HOST_ORGANIZE", "1")
        else:
            monkeypatch.delenv("SAGE2OV_HOST_ORGANIZE", raising=False)
        g = s2.Context(21, device=0); g.reads_add_ascii(bases, off); g.reads_organize()
        p = str(tmp_path / (mode + ".reads")); g.reads_save(p)
        out[mode] = (g.reads_export(), g.reads_stats().unique_reads, g.timings().organize_ms, fx.md5_file(p), g)
    monkeypatch.delenv("SAGE2OV_HOST_ORGANIZE", raising=False)
    o = ol.Oracle(21, 8); o.add_reads_ascii(bases, off); o.organize()
    po = str(tmp_path / "oracle.reads"); o.write_reads(po)
    (dp, dl, df), dn, dms, dmd5, dg = out["device"]; (hp, hl, hf), hn, hms, hmd5, hg = out["host"]
    assert dms > 0 and hms == 0, "the device organiser must be the one that ran by default"
    assert dn == hn == o.counter("N") == 600
    assert sorted(c & 0xFFFF for c in fx.HEAVY_COPIES) == [0, 1, 65535]
    for fr in (df, hf, o.export_reads()[2]):                                        # 65 535, 0 and (with the 597 plain reads) 1
        assert sorted(int(x) for x in fr[1:] if x != 1) == [0, 65535] and int((fr[1:] == 1).sum()) == 598
    assert np.array_equal(dl, hl) and np.array_equal(df, hf) and np.array_equal(dp, hp)
    assert_reads_equal_oracle(dg, o); assert_reads_equal_oracle(hg, o)
    assert dmd5 == hmd5 == fx.md5_file(po)
    dg.run_steps23(); o.run_all(); assert_equals_oracle(dg, o)                      # (and the frequencies change nothing downstream)
    assert len(dg.edges()) > 0
    dg.close(); hg.close(); o.close()


# ---------------------------------------------------------------------------------------------------------------- state carried between read sets
STATE_K = 40
STATE_SETS = {
    "large": dict(recipe="tiling", seed=41, n_unique=20000, read_len=150, step=9, dup_every=7, dup_copies=1),         # 8-word layout, one length
    "tiny": dict(recipe="low_complexity", seed=42, read_len=100, block=300, flank=60, step=1),                         # 4-word layout, long buckets
}


def _run_set(name):
    bases, off = fx.make_reads(STATE_SETS[name])
    return run_gpu(dict(k=STATE_K), bases, off)


def _fresh_process_digest(name):
    """the result of one read set in a process that has done nothing else"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("RESULT_DIGEST ")]
    assert r.returncode == 0 and len(lines) == 1, r.stdout.decode()[-2000:]
    return lines[0].split()[1]


@pytest.mark.parametrize("order", [("large", "tiny", "large"), ("tiny", "large", "tiny")], ids=["large_first", "tiny_first"])
def test_read_sets_one_after_the_other_in_one_process(order, tmp_path):
    """What one read set leaves behind must not reach the next (the `runStartFrac` kind of bug): process-wide state (g_tag_mask, the step-4 block cache, the
    workspace arena) and the state of a context that is given a second read set.  A large set (20 000 reads of 150 bases) and a tiny low-complexity one (100 bases:
    another layout) in both orders, three ways: contexts opened and closed back to back, step 4 included; contexts open side by side, run a second time in reverse
    order; and ONE context that takes each set in turn through reads_load.  Every result must be the oracle's, and the digest of a fresh process that ran that set
    alone."""
    fresh = {name: _fresh_process_digest(name) for name in STATE_SETS}
    oracles = {}
    for name, pd in STATE_SETS.items():
        bases, off = fx.make_reads(pd)
        oracles[name] = run_oracle(dict(k=STATE_K), bases, off)
    assert oracles["large"].counter("N") == 20000 and 0 < oracles["tiny"].counter("N") < 1000
    assert oracles["tiny"].counter("edges") > 0 and oracles["tiny"].counter("long_buckets") > 0
    for name in order:                                                              # back to back: create, run, close
        g = _run_set(name)
        assert_equals_oracle(g, oracles[name]); assert result_digest(g) == fresh[name], name
        g.graph_simplify()                                                          # (step 4 too: its block cache is sized by this set)
        g.close()
    held = [(_run_set(name), name) for name in order]                               # side by side
    for g, name in reversed(held):
        g.run_steps23()
        assert_equals_oracle(g, oracles[name]); assert result_digest(g) == fresh[name], name
    files, totals = {}, {}
    for g, name in held[:2]:
        files[name] = str(tmp_path / (name + ".reads")); g.reads_save(files[name])
        totals[name] = (g.reads_stats().good_reads, g.reads_stats().total_bp)
    for g, _ in held:
        g.close()
    c = s2.Context(STATE_K, device=0)                                               # one context, one read set after the other
    for name in order:
        c.reads_load(files[name]); c.reads_set_totals(*totals[name]); c.run_steps23()
        assert_equals_oracle(c, oracles[name]); assert result_digest(c) == fresh[name], name
    c.close()
    for o in oracles.values():
        o.close()


if __name__ == "__main__":                                                          # the fresh process of test_read_sets_one_after_the_other_in_one_process
    ctx = _run_set(sys.argv[1])
    print("RESULT_DIGEST", result_digest(ctx), flush=True)
    ctx.close()
