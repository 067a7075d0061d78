"""GPU: the contigs of the resident step-4 graph (sage2ov_contigs_*) against the restatement of tests/test_contigs_host.py -- table, strings and
the saved FASTA, exactly -- and against the reference's own P_contig.fasta committed under tests/golden/ (rows of equal edge length, whose order the reference
leaves open, as sets).  On the clean goldens every string must be a substring of the genome the reads were drawn from: that check needs no oracle."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import fixtures as fx
import sage2_amd as s2
import test_mate_estimate_host as H
import test_contigs_host as CH
from test_gpu_mate_estimate import add_mates, load_text

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("minimiser_groups_on")]
ROOT = fx.ROOT


def strings_of(ctx, first=0, count=None):
    seq, off = ctx.contig_sequences(first, count)
    text = seq.tobytes().decode()
    return [text[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def check(ctx, g, seqs, tmp_path, threshold=0, genome_size=0, name="c.fasta"):
    """table, statistics, every string and the saved file against the restatement; -> (rows, the file's text)"""
    rows, st, thr = CH.contig_table(g, seqs, threshold, genome_size)
    ctx.contigs_build(threshold, genome_size)
    table = ctx.contigs()
    assert CH.got_tuples(table) == CH.table_tuples(rows)
    CH.same_stats(ctx.contig_stats(), st)
    assert ctx.contigs_count() == (len(rows), sum(r["string_length"] for r in rows))
    assert strings_of(ctx) == [r["string"] for r in rows]
    out = str(tmp_path / name); ctx.contigs_save(out)
    text = open(out).read()
    assert text == CH.fasta_text(rows)
    return rows, text


def golden_ctx(name, **kw):
    m = fx.golden(name)
    ctx = s2.Context(m["k"], **kw); ctx.reads_add_ascii(*fx.make_reads(m["synth"])); ctx.reads_organize()
    return m, ctx


def golden_graph4(name):
    return gzip.open(os.path.join(fx.GOLDEN, name + ".graph4.gz")).read()


def load_bytes(ctx, text, tmp_path, name="in.graph4"):
    p = str(tmp_path / name); open(p, "wb").write(text); ctx.graph_load_composite(p)


# ------------------------------------------------------------------------------------------ the hand-built graph
def test_hand_built_graph_through_the_loader(tmp_path):
    ctx, seqs = CH.hand_store(device=-1)
    text = H.graph_text(CH.HAND_HEADER, CH.hand_contig_graph()); g = H.parse_graph(text)
    load_text(ctx, text, tmp_path)
    rows, fasta = check(ctx, g, seqs, tmp_path, genome_size=5000)
    assert len(rows) == 10 and fasta.count(">") == 8 and ctx.contig_stats().gaps == 3 and ctx.contig_stats().n_bases == 2016
    want = [r["string"] for r in rows]
    for i in range(len(rows)):                                                        # one row at a time
        assert strings_of(ctx, i, 1) == want[i:i + 1]
    assert strings_of(ctx, 3, 4) == want[3:7] and strings_of(ctx, 9, 1) == want[9:] and strings_of(ctx, 4, 0) == [] and strings_of(ctx, 10, 0) == []
    # a buffer that is too short, a range outside the table: refused, nothing written
    lens = ctx.contigs()["string_length"]
    buf = np.full(int(lens.sum()), 7, dtype=np.uint8); off = np.full(11, 9, dtype=np.uint64)
    import ctypes as C
    for first, count, cap in ((0, 10, int(lens.sum()) - 1), (9, 2, len(buf)), (11, 0, len(buf))):
        rc = s2.lib().sage2ov_contigs_sequences(ctx._h, C.c_uint64(first), C.c_uint64(count), C.c_void_p(buf.ctypes.data), C.c_uint64(cap), C.c_void_p(off.ctypes.data))
        assert rc == -1 and (buf == 7).all() and (off == 9).all()
    tab = np.zeros(9, dtype=s2.CONTIG_DTYPE)
    assert s2.lib().sage2ov_contigs_export(ctx._h, C.c_void_p(tab.ctypes.data), C.c_uint64(9)) == -1 and not tab["from"].any()
    # other thresholds: 20 takes in the edge of 49 and the edge of 20, which is `wrapped` (20 < L(to) / 2): in the table with contig_length 0, not in the file
    rows, fasta = check(ctx, g, seqs, tmp_path, threshold=20, genome_size=5000, name="t20.fasta")
    assert len(rows) == 12 and ctx.contig_stats().wrapped == 1 and fasta.count(">") == 11
    rows, fasta = check(ctx, g, seqs, tmp_path, threshold=3000, name="t3000.fasta")
    assert rows == [] and fasta == "" and ctx.contig_stats().contigs == 0
    scaff = str(tmp_path / "s.fasta"); ctx.contigs_build(0, 0); ctx.contigs_save(scaff, scaffold=True)
    assert open(scaff).read() == CH.fasta_text(CH.contig_table(g, seqs)[0], scaffold=True)
    ctx.close()


def test_inconsistent_lists_stay_inside_the_string(tmp_path):
    """pieces that add up to more than len, and to less: characters beyond the string are dropped, positions not reached stay N, both edges are counted"""
    ctx, seqs = CH.hand_store(device=-1)
    long_ = H.rec(12, 11, 2, 60, [(13, 1, 0, 50, 50), (14, 0, 0, 50, 50)])              # 50 + 50 + 50 > 60
    short = H.rec(16, 15, 1, 300, [(10, 1, 0, 2047, 3), (17, 0, 0, 3, 10)])             # a gap that alone passes the string
    short2 = H.rec(20, 19, 3, 200, [(13, 1, 0, 10, 20)])                                # 10 + 20 < 200: N up to the end
    recs = [r for x in (long_, short, short2) for r in (H.twin_of(x), x)]
    text = H.graph_text(CH.HAND_HEADER, recs); g = H.parse_graph(text)
    load_text(ctx, text, tmp_path)
    rows, fasta = check(ctx, g, seqs, tmp_path)
    assert ctx.contig_stats().inconsistent == 3 and rows[1]["string"].endswith("N" * 170) and rows[0]["string"][60:] == "N" * 300
    ctx.close()


# ------------------------------------------------------------------------------------------ the goldens: the reference's own file, both graph routes, the genome
@pytest.fixture(scope="module")
def goldens():
    """name -> (manifest, context with the golden's P.graph4 loaded, parsed graph, stored reads): built once per golden and shared; no test changes graph or reads"""
    cache = {}

    def get(name, tmp_path):
        if name not in cache:
            m, ctx = golden_ctx(name); text = golden_graph4(name)
            load_bytes(ctx, text, tmp_path)
            cache[name] = (m, ctx, H.parse_graph(text), H.stored_reads(ctx))
        return cache[name]
    yield get
    for c in cache.values():
        c[1].close()


@pytest.mark.parametrize("name", ["g1_clean100_k21", "g5_mixedlen_k21", "g7_palindrome_tandem_k21", "g10_long900_k55"])
def test_committed_reference_fasta(name, goldens, tmp_path):
    """S = 4 words per read for g1, g5 and g7, 32 for g10"""
    m, ctx, g, seqs = goldens(name, tmp_path)
    assert ctx.reads_stats().words_per_read == (32 if name.startswith("g10") else 4)
    rows, fasta = check(ctx, g, seqs, tmp_path, genome_size=int(m["synth"].get("genome_len", 0)))
    ref = gzip.open(os.path.join(fx.GOLDEN, name + ".contig.fasta.gz")).read().decode()
    groups = CH.same_fasta_up_to_ties(ref, rows)
    assert CH.parse_fasta(fasta) and (groups > 0 or fasta == ref)                    # without ties the file is the reference's, byte for byte
    out = str(tmp_path / "again.graph4"); ctx.graph4_save(out)
    assert open(out, "rb").read() == golden_graph4(name)                            # the graph is as it was


@pytest.mark.parametrize("name,words", [("g2_clean150_k40", 8), ("g13_noisy300_k55", 16)])
def test_the_other_slot_sizes(name, words, goldens, tmp_path):
    """8 and 16 words per read (4 and 32: the committed files above), against the restatement"""
    m, ctx, g, seqs = goldens(name, tmp_path)
    assert ctx.reads_stats().words_per_read == words
    rows, _ = check(ctx, g, seqs, tmp_path)
    assert len(rows) > 0


@pytest.mark.parametrize("name", ["g1_clean100_k21", "g2_clean150_k40"])
def test_strings_are_substrings_of_the_genome(name, goldens, tmp_path):
    """clean reads: whatever steps 1-4 and the spelling did, every string lies in the genome or in its reverse complement"""
    m, ctx, g, seqs = goldens(name, tmp_path)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[s2.synth_genome(fx.synth_params(m["synth"]))].tobytes().decode()      # (the generator gives codes 0 .. 3)
    rev = fx.revcomp(genome)
    ctx.contigs_build(0, len(genome))
    strings = strings_of(ctx)
    assert strings and all(s in genome or s in rev for s in strings)
    assert ctx.contig_stats().longest > len(genome) // 2 and ctx.contig_stats().n50_ordinal == 1


def test_steps_1_to_4_in_process(goldens, tmp_path):
    m, ctx, g, seqs = goldens("g1_clean100_k21", tmp_path)
    ctx.contigs_build(0, 40000); want = (ctx.contigs().tobytes(), strings_of(ctx))
    m, c2 = golden_ctx("g1_clean100_k21"); c2.run_steps23(); c2.graph_simplify()
    c2.contigs_build(0, 40000)
    assert (c2.contigs().tobytes(), strings_of(c2)) == want
    a, b = str(tmp_path / "a.fasta"), str(tmp_path / "b.fasta"); ctx.contigs_save(a); c2.contigs_save(b)
    assert open(a).read() == open(b).read() == gzip.open(os.path.join(fx.GOLDEN, "g1_clean100_k21.contig.fasta.gz")).read().decode()
    c2.close()


def test_ranges_give_the_one_shot_result(goldens, tmp_path, monkeypatch):
    """g10: 3 902 rows, 5.8 M characters.  contig_sequences in ranges of 1, 7, 500 and all rows; contigs_save with its range bound lowered to 4 KB and to 16 bytes
    (SAGE2OV_TEST_CONTIG_RANGE): every range of one row -- the same file"""
    m, ctx, g, seqs = goldens("g10_long900_k55", tmp_path)
    monkeypatch.delenv("SAGE2OV_TEST_CONTIG_RANGE", raising=False); ctx.options_reload()
    ctx.contigs_build(0, 150000)
    lens = ctx.contigs()["string_length"]; n = len(lens)
    whole, off = ctx.contig_sequences(0, n, lens)
    assert int(off[-1]) == int(lens.sum()) and np.array_equal(np.diff(off.astype(np.int64)), lens.astype(np.int64))
    for step in (7, 500):
        parts = [ctx.contig_sequences(a, min(step, n - a), lens)[0] for a in range(0, n, step)]
        assert np.array_equal(np.concatenate(parts), whole)
    for a in list(range(0, n, 397)) + [n - 1]:
        assert np.array_equal(ctx.contig_sequences(a, 1, lens)[0], whole[int(off[a]):int(off[a + 1])])
    one = str(tmp_path / "one.fasta"); ctx.contigs_save(one); want = open(one, "rb").read()
    for bound in ("4096", "16"):
        monkeypatch.setenv("SAGE2OV_TEST_CONTIG_RANGE", bound); ctx.options_reload()
        out = str(tmp_path / ("r%s.fasta" % bound)); ctx.contigs_save(out)
        assert open(out, "rb").read() == want
    monkeypatch.delenv("SAGE2OV_TEST_CONTIG_RANGE"); ctx.options_reload()


def test_memory_diet_mode_gives_the_same(monkeypatch, tmp_path):
    """steps 1-4 in memory-diet mode release the id-ordered read store (reads of one length): the strings come out of the locality-ordered one through posOf[]"""
    name = "g4_highcopy_k21"
    monkeypatch.delenv("SAGE2OV_MEMORY_DIET", raising=False)
    m, a = golden_ctx(name); a.run_steps23(); a.graph_simplify()
    a.contigs_build(0, 0); want = (a.contigs().tobytes(), strings_of(a)); fa = str(tmp_path / "a.fasta"); a.contigs_save(fa)
    assert len(want[1]) > 10
    monkeypatch.setenv("SAGE2OV_MEMORY_DIET", "1")
    m, b = golden_ctx(name); b.run_steps23(); b.graph_simplify()
    q = np.frombuffer(H.stored_reads(b)[1].encode(), dtype=np.uint8); assert b.reads_find_ids(q, np.array([0, len(q)], dtype=np.uint64)).tolist() == [1]
    assert b.reads_find_stats().route == s2.FIND_ROUTE_LOCALITY                     # the id-ordered store is gone
    b.contigs_build(0, 0); fb = str(tmp_path / "b.fasta"); b.contigs_save(fb)
    assert (b.contigs().tobytes(), strings_of(b)) == want and open(fa, "rb").read() == open(fb, "rb").read()
    a.close(); b.close()


# ------------------------------------------------------------------------------------------ staleness, call order, the CLI
def test_staleness_and_call_order(tmp_path):
    ctx, seqs = CH.hand_store(device=-1)
    for call in (ctx.contigs_build, ctx.contigs, ctx.contigs_count, lambda: ctx.contigs_save(str(tmp_path / "no.fasta"))):      # no graph
        with pytest.raises(s2.Sage2ovError) as e:
            call()
        assert e.value.code == -1
    assert not os.path.exists(tmp_path / "no.fasta")
    recs = CH.hand_contig_graph(); text = H.graph_text(CH.HAND_HEADER, recs); g = H.parse_graph(text)
    load_text(ctx, text, tmp_path)
    saved = str(tmp_path / "s.graph4"); ctx.graph4_save(saved); graph_before = open(saved, "rb").read()
    add_mates(ctx, {1: [(11, 1, 13, 1), (12, 0, 13, 1), (10, 1, 14, 0), (16, 1, 17, 1)]}); mates_before = [x.tobytes() for x in ctx.mates(1)]; assert len(ctx.mates(1)[0]) == 8
    rows, fasta = check(ctx, g, seqs, tmp_path, genome_size=5000)
    # flows change: only flow= changes (the calls rebuild the table with the threshold and genome size of the last build)
    fl = ctx.graph_flows(); ctx.graph_set_flows(fl * 2 + 0.25)
    t2 = ctx.contigs()
    assert np.allclose(t2["flow"], np.array([r["flow"] for r in rows], dtype=np.float32) * 2 + 0.25)
    assert [t[:9] + t[10:] for t in CH.got_tuples(t2)] == [t[:9] + t[10:] for t in CH.table_tuples(rows)]
    f2 = str(tmp_path / "f2.fasta"); ctx.contigs_save(f2)
    strip = lambda t: [x.split(" flow=")[0] + " " + x.split(" Edge length=")[1] if x.startswith(">") else x for x in t.splitlines()]
    assert strip(open(f2).read()) == strip(fasta) and open(f2).read() != fasta and ctx.contig_stats().n50_ordinal == 4
    ctx.graph_set_flows(fl)
    assert CH.got_tuples(ctx.contigs()) == CH.table_tuples(rows)
    # nothing else moved: the written graph, the mate calls
    ctx.graph4_save(saved); assert open(saved, "rb").read() == graph_before
    ents = [x.tobytes() for x in ctx.read_edges()]
    ctx.contigs_build(20, 0); strings_of(ctx)
    assert [x.tobytes() for x in ctx.read_edges()] == ents and [x.tobytes() for x in ctx.mates(1)] == mates_before
    # another graph: the table is rebuilt
    other = [r for x in (H.rec(12, 11, 2, 70, []), H.rec(14, 13, 3, 80, [(15, 1, 0, 30, 50)])) for r in (H.twin_of(x), x)]
    text2 = H.graph_text(CH.HAND_HEADER, other); load_text(ctx, text2, tmp_path, "o.graph4")
    rows2, _ = check(ctx, H.parse_graph(text2), seqs, tmp_path, name="o.fasta")
    assert [(r["frm"], r["to"]) for r in rows2] == [(14, 13), (12, 11)]
    ctx.close()


def test_cli_writes_the_same_file(tmp_path):
    """-M 4 --contigs on g1 writes P_contig.fasta as the API does; -m 5 --contigs writes it from P.reads and P.graph4; without the option the directory is as before"""
    name = "g1_clean100_k21"; m = fx.golden(name)
    fa = str(tmp_path / "x.fa"); s2.synth_write_fasta(fx.synth_params(m["synth"]), fa)
    exe = os.path.join(ROOT, "sage2_amd", "sage2ov"); plain, out = str(tmp_path / "plain"), str(tmp_path / "out")
    subprocess.run([exe, "-f", fa, "-k", str(m["k"]), "-o", plain, "-p", "t", "-M", "4", "-s"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run([exe, "-f", fa, "-k", str(m["k"]), "-o", out, "-p", "t", "-M", "4", "-s", "--contigs", "--genomeSize", "40000"], check=True, stdout=subprocess.DEVNULL)
    assert sorted(os.listdir(out)) == sorted(os.listdir(plain) + ["t_contig.fasta"])
    for f in os.listdir(plain):
        if not f.endswith(".log"):
            assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(out, f), "rb").read(), f
    m, ctx = golden_ctx(name); load_bytes(ctx, golden_graph4(name), tmp_path); api = str(tmp_path / "api.fasta"); ctx.contigs_build(0, 40000); ctx.contigs_save(api); ctx.close()
    want = open(api, "rb").read(); assert want == gzip.open(os.path.join(fx.GOLDEN, name + ".contig.fasta.gz")).read()
    assert open(os.path.join(out, "t_contig.fasta"), "rb").read() == want
    assert "N50: 39999 BP (1)" in open(os.path.join(out, "t.log")).read() and "_contig" not in open(os.path.join(plain, "t.log")).read()
    subprocess.run([exe, "-k", str(m["k"]), "-o", out, "-p", "u", "-i", "t", "-m", "5", "-M", "5", "--contigs"], check=True, stdout=subprocess.DEVNULL)
    assert open(os.path.join(out, "u_contig.fasta"), "rb").read() == want
