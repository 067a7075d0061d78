"""The four restatements against the reference itself on generated composite graphs (tests/compgen.py): so far they had met reads on more than one record pair
almost only on the hand-built graphs.  The inputs: the seeds of GPU case E, a reduced case B (reads on up to 17 pairs) and one graph whose longest contig has
65 537 bases.  The comparisons are those of the four test_*_reference.py modules, imported; like them this module runs only where the reference tree and the objects
built from it (oracle/_ref/) are present."""
import pytest

import compgen as CG
import test_compgen_host as GH
import test_mate_estimate_host as H
import test_mate_estimate_reference as ER
import test_mate_support_reference as SR
import test_links_reference as LR
import test_contigs_reference as CR
from test_mate_estimate_reference import driver as estimate_driver          # noqa: F401  (module-scoped fixtures: each compiles its module's driver once)
from test_mate_support_reference import driver as support_driver            # noqa: F401
from test_links_reference import driver as links_driver                     # noqa: F401
from test_contigs_reference import driver as contigs_driver                 # noqa: F401

pytestmark = ER.pytestmark

B_REDUCED = ((17, 0), (9, 0), (7, 0), (8, 9), (2, 16), (16, 20), (15, 40), 2, 7, 8, 9)


def all_four(case, pairs, store_seed, drivers, tmp_path_factory):
    N, header, recs = case; text = H.graph_text(header, recs)
    ctx = GH.host_store(N, store_seed)
    ed, sd, ld, cd = drivers
    ER.compare(ed, tmp_path_factory.mktemp("e"), ctx, CG.K, text, pairs)
    sup = SR.compare(sd, tmp_path_factory.mktemp("s"), ctx, CG.K, text, pairs)
    lk, ref, g = LR.compare(ld, tmp_path_factory.mktemp("l"), ctx, CG.K, text, pairs)
    rows, st, fasta, groups = CR.compare(cd, tmp_path_factory.mktemp("c"), ctx, CG.K, text, 0)
    ctx.close()
    return sup, lk, ref, rows, st


@pytest.mark.parametrize("seed", CG.E_SEEDS)
def test_case_e_like_the_reference(seed, estimate_driver, support_driver, links_driver, contigs_driver, tmp_path_factory):
    case = CG.case_e(seed); pairs = CG.mates_e(GH.parsed(case), seed, for_reference=True)
    sup, lk, ref, rows, st = all_four(case, pairs, 100 + seed, (estimate_driver, support_driver, links_driver, contigs_driver), tmp_path_factory)
    assert len(rows) > 0 and st["inconsistent"] == 0


def test_reduced_case_b_like_the_reference(estimate_driver, support_driver, links_driver, contigs_driver, tmp_path_factory):
    case = CG.case_b(pairs=300, copies=B_REDUCED); g = GH.parsed(case); pairs = CG.mates_b(g, for_reference=True)
    per = GH.distances_per_entry(g, pairs[1])
    assert GH.max_pairs_per_read(g) == 17 and {c for c, _ in per.values()} >= {0, 1, 7, 8, 9} and max(d for _, d in per.values()) >= 5
    sup, lk, ref, rows, st = all_four(case, pairs, 31, (estimate_driver, support_driver, links_driver, contigs_driver), tmp_path_factory)
    assert lk and any(r[3] >= 1 for r in sup)


def test_longest_contig_of_65537_bases_like_the_reference(contigs_driver, tmp_path):
    case = CG.case_a_longest(65537); N, header, recs = case
    ctx = GH.host_store(N, 7)
    rows, st, fasta, groups = CR.compare(contigs_driver, tmp_path, ctx, CG.K, H.graph_text(header, recs), 0)
    assert rows[0]["len"] == 65537 and rows[0]["string_length"] == 65537 + 60 and len(rows) >= 301 and groups > 0 and st["inconsistent"] == 0
    ctx.close()
