"""The restatement of tests/test_contigs_host.py against the reference itself: OverlapGraph::printGraph (overlapGraph.cpp:507-784) run by the reference's own
objects with one thread on a P.reads a device-less context saved and a graph file its own loader reads (so every record pair is an edge:
parse_graph(fold=False)).  The .fasta is compared record by record; rows of equal edge length, whose order std::sort leaves open, as sets
(test_contigs_host.same_fasta_up_to_ties).  The committed tests/golden/<name>.contig.fasta.gz are what this reference writes.  Runs only where the reference tree and
the objects built from it (oracle/_ref/) are present.  The driver (tools/make_golden_contigs.py) is our own text; it includes the reference's headers and links
oracle/_ref/libsage2ref_driver.so."""
import gzip
import os
import sys

import pytest

import fixtures as fx
import sage2_amd as s2
import test_mate_estimate_host as H
import test_contigs_host as CH

sys.path.insert(0, os.path.join(fx.ROOT, "tools"))
import make_golden_contigs as MG      # noqa: E402

pytestmark = pytest.mark.skipif(not MG.available(), reason="the reference tree or oracle/_ref/libsage2ref_driver.so is absent")
GOLDENS = ["g1_clean100_k21", "g5_mixedlen_k21", "g7_palindrome_tandem_k21", "g10_long900_k55"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return MG.build_driver(str(tmp_path_factory.mktemp("refcontigs")))


def compare(driver, tmp_path, ctx, k, text, genome_size):
    g = H.parse_graph(text, fold=False)
    rows, st, thr = CH.contig_table(g, H.stored_reads(ctx), 0, genome_size)
    fasta, stats = MG.reference_contigs(driver, str(tmp_path), ctx, k, text, genome_size)
    groups = CH.same_fasta_up_to_ties(fasta, rows)
    # longest, covered and the N50 / N90 lengths hold whatever the order inside a group is only when the group's rows agree on them: covered always does
    assert stats[1] == st["covered"]
    if all(a["len"] != b["len"] or a["contig_length"] == b["contig_length"] for a, b in zip(rows, rows[1:])):
        assert stats == [st["longest"], st["covered"], st["n50"], st["n50_ordinal"], st["n90"], st["n90_ordinal"]]
    return rows, st, fasta, groups


def test_hand_built_graph_like_the_reference(driver, tmp_path):
    ctx, seqs = CH.hand_store()
    text = H.graph_text(CH.HAND_HEADER, CH.hand_contig_graph())
    rows, st, fasta, groups = compare(driver, tmp_path, ctx, CH.HAND_K, text, 5000)
    assert len(rows) == 10 and fasta.count(">") == 8 and groups == 1 and st["inconsistent"] == 0
    # the rows outside the one group of equal lengths: the reference's text, line for line
    ours = CH.fasta_text(rows)
    cut = lambda t: t[:t.index(">contig_6 ")] + t[t.index(">contig_10 "):]
    assert cut(fasta) == cut(ours)
    ctx.close()


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_like_the_reference(name, driver, tmp_path):
    m = fx.golden(name)
    ctx = s2.Context(m["k"], device=-2); ctx.reads_add_ascii(*fx.make_reads(m["synth"])); ctx.reads_organize()
    text = gzip.open(os.path.join(fx.GOLDEN, name + ".graph4.gz")).read()
    rows, st, fasta, groups = compare(driver, tmp_path, ctx, m["k"], text, MG.genome_len(m))
    assert len(rows) > 0 and st["written"] > 0
    committed = os.path.join(fx.GOLDEN, name + ".contig.fasta.gz")
    if os.path.exists(committed):
        assert gzip.open(committed).read().decode() == fasta                         # the fixture is this reference's output
    ctx.close()
