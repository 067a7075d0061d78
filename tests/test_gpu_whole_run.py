"""GPU: the whole assembly in one process -- `sage2ov -f reads.fa -k K -M 7` runs steps 1-7 on one context, the graph stays resident, the mate table of step 6
comes from step 1's own pass.  Its files against (1) a Python Context that makes the same calls in the same order, (2) a second run from
the files it left (`-m 4 -M 7`: the mates_add_file route), (3) the chained restarts that were the only way before (`-M 4`, `-m 5 --flowSolve`, `-m 6 --extend
--paths --shortOverlaps --scaffold`), (4) the reference's own one-shot run where its binary is built (oracle/_ref/SAGE2), compared as the contig and scaffold
suites compare with it: rows of equal length may change places."""
import os
import subprocess

import pytest

import fixtures as fx
import sage2_amd as s2
from test_find_ids_host import input_reads

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("minimiser_groups_on")]      # (as tests/test_gpu_tail.py: small inputs)
REF = os.path.join(fx.ROOT, "oracle", "_ref", "SAGE2")
CLI = os.path.join(fx.ROOT, "sage2_amd", "sage2ov")
G1 = "g1_clean100_k21"
ALL7 = ["t.reads", "t.graph3", "t.graph4", "t.graph5", "t.graph6", "t_contig.fasta", "t_scaffold.fasta"]


def data(path):
    return open(path, "rb").read()


def same(a, b):
    return os.path.exists(a) and os.path.exists(b) and data(a) == data(b)


def fasta_of(name, tmp_path):
    m = fx.golden(name); fa = str(tmp_path / "x.fa")
    if "recipe" in m["synth"]:
        bases, off = fx.make_reads(m["synth"])
        with open(fa, "w") as f:
            f.write("".join(f">{i}\n{r}\n" for i, r in enumerate(input_reads(bases, off))))
    else:
        s2.synth_write_fasta(fx.synth_params(m["synth"]), fa)
    return m, fa


def cli(*args, **kw):
    return subprocess.run([CLI] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, **kw)


def whole_run(name, tmp_path, out="whole"):
    m, fa = fasta_of(name, tmp_path); d = str(tmp_path / out)
    r = cli("-f", fa, "-k", m["k"], "-o", d, "-p", "t", "-M", 7, "-s")
    assert r.returncode == 0, r.stderr
    assert "continue with the reference" not in r.stdout
    return m, fa, d


@pytest.fixture(scope="module")
def g1_whole(tmp_path_factory):
    """the whole run on g1, once for the tests of this module (they only read its files)"""
    tmp = tmp_path_factory.mktemp("whole_g1")
    return whole_run(G1, tmp) + (tmp,)


def test_whole_run_equals_the_same_calls_on_a_context(g1_whole, tmp_path):
    m, fa, d, _ = g1_whole
    for f in ALL7 + ["t.hashTable", "input.cs2", "output.cs2", "t.log"]:
        assert os.path.exists(os.path.join(d, f)), f
    assert fx.md5_file(os.path.join(d, "t.reads")) == m["reads_md5"]
    log = open(os.path.join(d, "t.log")).read()
    for block in ("STEP 1:", "STEP 4:", "STEP 5:", "STEP 6:", "STEP 7:", "Rounds of findMatepairSupports", "Rounds of mergeShortOverlaps", "Rounds of mergeFinal", "t_scaffold.fasta written"):
        assert block in log, block
    p = lambda n: str(tmp_path / n)
    ctx = s2.Context(m["k"], device=0)
    ctx.reads_pair_library(1); ctx.reads_add_file(fa); ctx.reads_organize(); ctx.reads_save(p("t.reads"))
    ctx.run_steps23(); ctx.graph_save(p("t.graph3"))
    ctx.graph_simplify(); ctx.graph4_save(p("t.graph4"))
    gs = ctx.copy_counts(); ctx.graph5_save(p("t.graph5"))
    ctx.mates_from_reads(); st = ctx.mates_stats(); ctx.mates_estimate(); ctx.extend_contigs(); ctx.graph6_save(p("t.graph6"))
    ctx.contigs_build(0, gs); ctx.contigs_save(p("t_contig.fasta"))
    ctx.scaffold(); ctx.contigs_build(0, gs); ctx.contigs_save(p("t_scaffold.fasta"), scaffold=True)
    ctx.close()
    assert st.pairs_seen == m["synth"]["n_reads"] // 2 and st.pairs_added > 0 and st.pairs_not_found == 0
    for f in ALL7:
        assert same(os.path.join(d, f), p(f)), f"{f}: the CLI's file differs from the context's"
    assert len(data(p("t_scaffold.fasta"))) > m["synth"]["genome_len"] // 2


def test_restart_at_step_4_takes_the_second_pass_and_ends_the_same(g1_whole, tmp_path):
    """-m 4 -M 7 from the files of the whole run: the reads come from t.reads, so the mate table comes from mates_add_file"""
    m, fa, d, _ = g1_whole
    r = cli("-f", fa, "-k", m["k"], "-o", d, "-p", "u", "-i", "t", "-m", 4, "-M", 7, "-s")
    assert r.returncode == 0, r.stderr
    for sfx in (".graph4", ".graph5", ".graph6", "_contig.fasta", "_scaffold.fasta"):
        assert same(os.path.join(d, "t" + sfx), os.path.join(d, "u" + sfx)), sfx


def chained(m, fa, d, upto):
    r = cli("-f", fa, "-k", m["k"], "-o", d, "-p", "t", "-M", 4); assert r.returncode == 0, r.stderr
    r = cli("-k", m["k"], "-o", d, "-p", "t", "-m", 5, "--flowSolve"); assert r.returncode == 0, r.stderr
    if upto >= 6:
        r = cli("-f", fa, "-k", m["k"], "-o", d, "-p", "t", "-m", 6, "--extend", "--paths", "--shortOverlaps", "--scaffold", "--contigs"); assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("name", ["g6_k70_150", "g7_palindrome_tandem_k21"])
def test_graph4_and_graph5_equal_the_chained_restarts(name, tmp_path):
    m, fa, d = whole_run(name, tmp_path)
    c = str(tmp_path / "chain"); chained(m, fa, c, 5)
    for sfx in (".graph4", ".graph5"):
        assert same(os.path.join(d, "t" + sfx), os.path.join(c, "t" + sfx)), f"{name}: {sfx}"


def test_g1_equals_the_chained_restarts_to_the_scaffolds(g1_whole, tmp_path):
    """the resident graph after step 4 keeps step 4's pool order, a reloaded P.graph5 has the file's: DESIGN.md 5.17 rule (a) compares pool indices, so this is where
    the two routes could part.  On g1 they do not."""
    m, fa, d, _ = g1_whole
    c = str(tmp_path / "chain"); chained(m, fa, c, 7)
    for sfx in (".graph4", ".graph5", ".graph6", "_contig.fasta", "_scaffold.fasta"):
        assert same(os.path.join(d, "t" + sfx), os.path.join(c, "t" + sfx)), sfx


def records(text):
    """tests/test_gpu_scaffold.py: (header without ordinal and running counters, sequence, the running counters)"""
    out = []
    for blk in text.split(">")[1:]:
        head, seq = blk.split("\n", 1); f = head.split(" gapCount=")
        out.append((f[0].split(" ", 1)[1], seq, f[1]))
    return out


def test_g1_against_the_references_own_run(g1_whole, tmp_path):
    if not os.path.exists(REF):
        pytest.skip("oracle/_ref/SAGE2 not built (it is built in the build container and travels with the snapshot)")
    m, fa, d, _ = g1_whole
    full = str(tmp_path / "full")
    subprocess.run([REF, "-f", fa, "-k", str(m["k"]), "-o", full, "-p", "t", "-M", "7"], check=True, env=dict(os.environ, OMP_NUM_THREADS="8", LC_ALL="C"), stdout=subprocess.DEVNULL, cwd=str(tmp_path))
    for f in ("t_contig.fasta", "t_scaffold.fasta"):
        got_text, want_text = open(os.path.join(d, f)).read(), open(os.path.join(full, f)).read()
        got, want = records(got_text), records(want_text)
        assert len(want) >= 1 and sorted(x[:2] for x in got) == sorted(x[:2] for x in want) and got[-1][2] == want[-1][2], f
        lengths = [x[0].split("Edge length=")[1].split(" ")[0] for x in want]
        assert all(lengths.count(lengths[i]) > 1 for i in range(len(want)) if got[i][:2] != want[i][:2]), f      # only rows of equal length change places
        if len(set(lengths)) == len(lengths):
            assert got_text == want_text, f


def test_errors(g1_whole, tmp_path):
    m, fa, d, _ = g1_whole
    out = str(tmp_path / "e1"); sol = os.path.join(d, "output.cs2")
    r = cli("-f", fa, "-k", m["k"], "-o", out, "-p", "t", "-m", 1, "-M", 6, "--flowSolution", sol)
    assert "[ERROR]" in r.stdout and "--flowSolution" in r.stdout and "outside solver" in r.stdout
    assert not os.path.exists(os.path.join(out, "t.graph5")) and not os.path.exists(os.path.join(out, "t.reads"))
    r = cli("-f", fa, "-k", m["k"], "-o", out, "-p", "t", "-M", 7, "--flowNetwork")
    assert "[ERROR]" in r.stdout and not os.path.exists(os.path.join(out, "t.graph5"))
    r = cli("-k", m["k"], "-o", d, "-p", "v", "-i", "t", "-m", 4, "-M", 7)
    assert "[ERROR]" in r.stdout and "needs the mate pairs" in r.stdout and not os.path.exists(os.path.join(d, "v.graph4"))
