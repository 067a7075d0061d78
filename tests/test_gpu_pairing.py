"""GPU: the mate table from step 1's own pass (sage2ov_reads_pair_library + sage2ov_mates_from_reads) on the HIP path -- k_org_ids and
k_org_ids_raw behind the organiser, k_pair_slots, k_pair_keep, then k_mate_records and everything behind it unchanged.  The cases and the expected value (the
mates_add_* route on a second context organised from the same input with pairing off) are those of tests/test_pairing_host.py, run here with device 0: the
ASCII cases go through k_org_classify / k_org_pack, the file cases through the host-packed staging and k_org_canon.  On top of them the shapes where the new
kernels can go wrong, and that a context with pairing off does what it did before."""
import numpy as np
import pytest

import fixtures as fx
import sage2_amd as s2
import test_pairing_host as P
from test_find_ids_host import input_reads, rnd
from test_pairing_host import K, both_routes, random_reads, with_n, write_fasta

pytestmark = pytest.mark.gpu
GPU = 0


@pytest.fixture(autouse=True)
def _no_test_switches(monkeypatch):
    for v in ("SAGE2OV_TEST_FIND_BATCH", "SAGE2OV_TEST_MATE_FLUSH", "SAGE2OV_TEST_FULL_SORT", "SAGE2OV_MEMORY_DIET", "SAGE2OV_SEQUENTIAL_READER"):
        monkeypatch.delenv(v, raising=False)


# ---------------------------------------------------------------------------------------------------------------- the host cases on the device
def test_ascii_rules():
    P.case_ascii(GPU)


def test_first_continues_from_earlier_calls():
    P.case_first_continues(GPU)


@pytest.mark.parametrize("sequential", [False, True], ids=["parallel_reader", "sequential_reader"])
def test_interleaved_fasta(tmp_path, monkeypatch, sequential):
    P.case_fasta(GPU, tmp_path, monkeypatch, sequential)


def test_four_line_fastq(tmp_path, monkeypatch):
    P.case_fastq(GPU, tmp_path, monkeypatch)


def test_gzip(tmp_path, monkeypatch):
    P.case_gz(GPU, tmp_path, monkeypatch)


@pytest.mark.parametrize("extra", [0, 1], ids=["n1_eq_n2", "n1_eq_n2_plus_1"])
def test_two_mate_files(tmp_path, monkeypatch, extra):
    P.case_two_files(GPU, tmp_path, monkeypatch, extra)


def test_list_of_two_datasets(tmp_path, monkeypatch):
    P.case_list(GPU, tmp_path, monkeypatch)


def test_errors():
    P.case_errors(GPU)


# ---------------------------------------------------------------------------------------------------------------- shapes of the new kernels
def both_stagings(calls_ascii, tmp_path, **kw):
    """the ASCII calls as they are (raw staging: k_org_classify, k_org_pack, k_org_ids_raw) and as small FASTA files (host-packed staging through the sequential
    reader: k_org_canon, k_pair_slots); returns the stats of the two"""
    out = []
    A, t, st = both_routes(GPU, calls_ascii, **kw); out.append((t, st)); A.close()
    files = [("file", write_fasta(str(tmp_path / f"c{i}.fa"), c[1]), None, c[2]) for i, c in enumerate(calls_ascii)]
    A, t2, st2 = both_routes(GPU, files, **kw); out.append((t2, st2)); A.close()
    assert P.same_tables(t, t2)
    return out


def test_one_pair_only(tmp_path):
    rng = np.random.default_rng(9100)
    r = random_reads(rng, 2)
    for (t, st) in both_stagings([("ascii", r, 1)], tmp_path):
        assert (st.pairs_seen, st.pairs_added) == (1, 1) and len(t[0][0]) == 2


def test_no_surviving_pair(tmp_path):
    rng = np.random.default_rng(9101)
    r = random_reads(rng, 6)
    reads = [with_n(r[0]), r[1], r[2], with_n(r[3]), r[4][:K], r[5], r[0]]
    for (t, st) in both_stagings([("ascii", reads, 1)], tmp_path):
        assert (st.pairs_seen, st.pairs_added, st.pairs_not_good) == (3, 0, 3) and len(t[0][0]) == 0


@pytest.mark.parametrize("staged", [63, 64, 65, 2047, 2048, 2049])
def test_wave_and_tile_edges(staged, tmp_path):
    """staged read counts on a wave (64) and on a radix tile (2 048), with two records in front that are not staged: the ordinals are not the staging indices"""
    rng = np.random.default_rng(9200 + staged)
    r = random_reads(rng, staged, 60, 110)
    reads = [with_n(r[0]), r[1][:K]] + r
    for (t, st) in both_stagings([("ascii", reads, 1)], tmp_path):
        assert st.pairs_seen == (staged + 2) // 2 and st.pairs_added == st.pairs_seen - 1
    A, _, _ = both_routes(GPU, [("ascii", reads, 1)]); assert A.reads_stats().good_reads == staged; A.close()


def test_long_run_takes_the_full_sort(tmp_path):
    """a read given 300 times (and its reverse complement 40 times): a run above ORG_RUN_LIMIT sends the organiser through the sort on every word"""
    rng = np.random.default_rng(9300)
    r = random_reads(rng, 41, 70, 120)
    reads = []
    for i in range(300):
        reads += [r[0], r[1 + i % 40]]
    reads += [fx.revcomp(r[0]), r[5]] * 40
    for (t, st) in both_stagings([("ascii", reads, 1)], tmp_path):
        assert st.pairs_added == 340 and int(t[0][0]["count"].max()) >= 7


def test_forced_full_sort_gives_the_same_table(monkeypatch):
    calls, _ = P.ascii_calls(9350)
    A, t, _ = both_routes(GPU, calls); A.close()
    monkeypatch.setenv("SAGE2OV_TEST_FULL_SORT", "1")
    A, t2, _ = both_routes(GPU, calls); A.close()
    assert P.same_tables(t, t2)


def test_mixed_lengths_32_word_layout(tmp_path):
    rng = np.random.default_rng(9400)
    r = random_reads(rng, 30) + [rnd(rng, 600)]
    reads = r[:10] + [r[30], r[3]] + r[10:30] + [fx.revcomp(r[30]), r[4]]
    for (t, st) in both_stagings([("ascii", reads, 1)], tmp_path):
        assert st.pairs_added == 17
    A, _, _ = both_routes(GPU, [("ascii", reads, 1)]); assert A.reads_stats().words_per_read == 32; A.close()


def test_flush_in_the_middle_of_a_call(monkeypatch, tmp_path):
    """SAGE2OV_TEST_FIND_BATCH = records per chunk of pairs, SAGE2OV_TEST_MATE_FLUSH = pending records per flush (the switches of tests/test_gpu_mates.py): the
    pending buffer is flushed between the chunks of one call and merged into the table, and the table is the unchunked one"""
    calls, _ = P.ascii_calls(9500)
    A, whole, st = both_routes(GPU, calls)
    assert (st.chunks, st.flushes, st.route) == (1, 1, s2.MATE_ROUTE_DEVICE); A.close()
    monkeypatch.setenv("SAGE2OV_TEST_FIND_BATCH", "64"); monkeypatch.setenv("SAGE2OV_TEST_MATE_FLUSH", "100")
    for (t, st) in both_stagings(calls, tmp_path):
        assert st.chunks == (2 * (255 + 256 + 257) + 63) // 64 and st.flushes > 3 and P.same_tables(t, whole)


def test_after_steps23_in_memory_diet_mode(monkeypatch):
    """the id-ordered store is released by the index build (uniform read length): mates_from_reads does not read the store, the mates_add_* route looks the ids up
    through posOf[]; the steps' results are not disturbed"""
    monkeypatch.setenv("SAGE2OV_MEMORY_DIET", "1")
    k = 40
    bases, off = fx.make_reads(dict(seed=9600, genome_len=20000, n_reads=6000, read_len=150, err_ppm=500))
    reads = input_reads(bases, off)
    edges = []

    def steps(ctx):
        ctx.run_steps23(); edges.append(ctx.edges().copy())

    A, t, st = both_routes(GPU, [("ascii", reads, 1)], k=k, between=steps)
    assert st.pairs_seen == 3000 == st.pairs_added and edges[0].tobytes() == edges[1].tobytes() and len(edges[0]) > 0
    assert A.edges().tobytes() == edges[0].tobytes()
    A.close()


def test_pairing_off_is_the_parent(tmp_path):
    """with pairing off step 1 makes the golden's P.reads, mates_from_reads is refused, and steps 2-3 launch what they launch with pairing on (nothing of the
    pairing runs inside them); with pairing on step 1 makes the same store"""
    m = fx.golden("g1_clean100_k21")
    bases, off = fx.make_reads(m["synth"])
    got = []
    for lib in (0, 1):
        ctx = s2.Context(m["k"], device=GPU)
        ctx.reads_pair_library(lib); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
        rp = str(tmp_path / f"p{lib}.reads"); ctx.reads_save(rp)
        assert fx.md5_file(rp) == m["reads_md5"]
        if lib == 0:
            with pytest.raises(s2.Sage2ovError) as e:
                ctx.mates_from_reads()
            assert e.value.code == -1
        ctx.timings_reset(); ctx.run_steps23(); tm = ctx.timings()
        got.append((tm.probe_kernel_launches, tm.probe_fast_launches, tm.sequential_reads, ctx.edges().tobytes(), [x.tobytes() for x in ctx.reads_export()]))
        ctx.close()
    assert got[0] == got[1] and got[0][0] + got[0][1] > 0
