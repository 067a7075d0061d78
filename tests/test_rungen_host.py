"""CPU: the planted-minimiser generator and the route model of run mode (tests/rungen.py), from the model and the oracle alone: every case of tests/test_gpu_run_limits.py
has the property it is named after, and the model's buckets are the oracle's (connection counts of every read).  No GPU."""
import numpy as np
import pytest

import oracle_lib as ol
import rungen as rg
from rungen import CAP, RUN_DMAX, RUN_LANES_MIN, RUN_MMAX, RUN_NMAX


# ---------------------------------------------------------------------------------------------------------------- the minimiser restatement
@pytest.mark.parametrize("L", [100, 150, 300])                  # the 4-, 8- and 16-word layouts
def test_minimiser_restatement_equals_the_naive_one(L):
    rng = np.random.default_rng(L)
    for _ in range(40):
        r = rg.rnd(rng, L)
        for s in (r, rg.revcomp(r)):
            assert rg.minimiser(s) == rg.minimiser_naive(s)


def test_minimiser_tie_first_position_wins():
    rng = np.random.default_rng(5)
    M = rg.planted(1)
    r = list(rg.rnd(rng, 150)); r[30:46] = M; r[90:106] = rg.revcomp(M); r = "".join(r)          # the same canonical 16-mer twice: hash 1 at offsets 30 and 90
    assert rg.minimiser(r) == rg.minimiser_naive(r) == (1, (255 - 30) | 256)
    r2 = rg.revcomp(r)                                                                             # ... at 44 (as it stands: the canonical one) and 104
    assert rg.minimiser(r2) == rg.minimiser_naive(r2) == (1, (255 - 44) | 256)
    r3 = r[:30] + rg.revcomp(M) + r[46:90] + M + r[106:]                                           # the first one is the reverse complement: strand 0
    assert rg.minimiser(r3) == rg.minimiser_naive(r3) == (1, 255 - 30)


def test_planted_16_mers_are_the_ones_of_their_hashes():
    assert [rg.planted(h) for h in (1, 2, 3, 5, 6)] == ["AATGGAGTAGTTCCAC", "ACTCACCGCCTGGGAG", "AGGTGGACGATCTTAT", "CAGAGTCTTGTAGCCC", "CCCTCAATACGTTGCG"]
    for h in rg.HASHES:
        m = rg.planted(h)
        assert (rg.mer_value(m) * rg.MUL) & 0xFFFFFFFF == h
    assert not any(4 * a == b for a in rg.HASHES for b in rg.HASHES)                               # no two 16-mers a shift of each other


def test_every_read_over_a_planted_16_mer_has_it_as_its_minimiser():
    """a 700-base random locus with the hash-1 16-mer at 350: all 135 forward reads of 150 bases and their reverse complements"""
    rng = np.random.default_rng(11)
    while True:
        g = list(rg.rnd(rng, 700)); g[350:366] = rg.planted(1); g = "".join(g)
        if min(rg.minimiser_naive(g[p:p + 16])[0] for p in range(216, 485) if p != 350) > 1: break
    for s in range(216, 351):
        r = g[s:s + 150]
        assert rg.minimiser(r) == (1, (255 - (350 - s)) | 256)
        assert rg.minimiser(rg.revcomp(r)) == (1, 255 - (s + 150 - 366))


# ---------------------------------------------------------------------------------------------------------------- the cases
@pytest.fixture(scope="module")
def routed():
    """case, model, counters and trace with the library's threshold, built once"""
    cache = {}

    def get(name):
        if name not in cache:
            c = rg.get_case(name); m = c.model(); ctr, tr = m.route()
            cache[name] = (c, m, ctr, tr)
        return cache[name]
    return get


def ok_steps(c, name, tr):
    return [t for t in c.steps_of(name, tr) if t["ended"] is None]


@pytest.mark.parametrize("name", list(rg.CASES))
def test_the_bucket_model_agrees_with_the_oracle(name, routed):
    """unique reads, ids and buckets: the model's verified overlaps of EVERY read are the oracle's connection count; the loci stand in front of the order as written,
    with the meta words the generator intends; the reads the case is about have records"""
    c, m, ctr, tr = routed(name)
    bases, off = c.arrays()
    o = ol.Oracle(c.k, 4); o.add_reads_ascii(bases, off); o.organize(); o.run_all()
    assert o.counter("N") == m.N and o.counter("long_buckets") == m.long_buckets()
    right, left, status, conn = o.export_initial()
    assert [int(conn[m.idOf[p]]) for p in range(1, m.N + 1)] == [m.hits(p) for p in range(1, m.N + 1)]
    hashes = [l.h for l in c.loci.values()]
    for lname, l in c.loci.items():
        ps = c.positions(lname)
        assert len(ps) == len(l.reads()) and all(m.hash[p] == l.h for p in ps)
        if hashes.count(l.h) == 1:
            first = c.first_pos(lname)
            assert ps == list(range(first, first + len(ps))) and [m.seq[p] for p in ps] == l.reads()
            assert [m.meta[p] & 0x1FF for p in ps] == l.expected_metas() and m.meta[first] & 0x200 and not any(m.meta[p] & 0x200 for p in ps[1:])
        if len(ps) > 1:
            assert all(right[m.idOf[p]] or left[m.idOf[p]] for p in ps)
    o.close()


def test_family_A_shifts(routed):
    c, m, ctr, tr = routed("shifts")
    for d in (1, 63, 64):
        p = c.first_pos("d%d" % d)
        assert m.hash[p] == m.hash[p + 1] and m.meta[p] & 0x100 == m.meta[p + 1] & 0x100 and (m.meta[p + 1] & 255) - (m.meta[p] & 255) == d
        assert [(t["i"], t["d1"], t["m"]) for t in ok_steps(c, "d%d" % d, tr)] == [(p + 1, d, 1)]
    p = c.first_pos("d65")
    assert (m.meta[p + 1] & 255) - (m.meta[p] & 255) == 65 == RUN_DMAX + 1 and not ok_steps(c, "d65", tr)
    assert [t["ended"] for t in c.steps_of("d65", tr) if t["i"] == p + 1] == ["shift"]
    assert [t["d1"] for t in ok_steps(c, "chain64", tr)] == [64, 64]
    # one hash in two unrelated genomes: offsets 50, 50, 45, 40 -- a shift of 0, a true shift of 5, a shift of 5 onto another genome
    two = [t for t in c.steps_of("twoX", tr) if t["i"] > c.positions("twoX")[0] - 0 and t["hash"] == c.loci["twoX"].h]
    assert [(t["d1"], t["ended"]) for t in two][-3:] == [(0, "shift"), (5, None), (5, "own entry")]
    ps = sorted(c.positions("twoX") + c.positions("twoY"))
    assert [m.meta[p] & 255 for p in ps] == [255 - 50, 255 - 50, 255 - 45, 255 - 40]


def test_family_B_strand_changes(routed):
    c, m, ctr, tr = routed("mirror")
    for d in (1, 64):
        a = [t for t in ok_steps(c, "d1_%d" % d, tr) if t["flip"]]; b = [t for t in ok_steps(c, "d2_%d" % d, tr) if t["flip"]]
        assert [(t["d1"], t["d2"]) for t in a] == [(d, 0)] and [(t["d1"], t["d2"]) for t in b] == [(0, d)]
        # ... and the run goes on behind the mirror
        assert [t["d1"] for t in ok_steps(c, "d1_%d" % d, tr) if not t["flip"]] == [3] and [t["d1"] for t in ok_steps(c, "d2_%d" % d, tr) if not t["flip"]] == [3]
    assert [(t["d1"], t["ended"]) for t in c.steps_of("d1_65", tr) if t["flip"] and t["i"] in c.positions("d1_65")[1:]] == [(65, "shift")]
    assert [(t["d2"], t["ended"]) for t in c.steps_of("d2_65", tr) if t["flip"] and t["i"] in c.positions("d2_65")[1:]] == [(65, "shift")]
    t = [t for t in c.steps_of("dl0_Y", tr) if t["flip"] and t["i"] in c.positions("dl0_Y")]
    assert [(x["i"], x["d1"], x["d2"], x["ended"]) for x in t] == [(c.positions("dl0_Y")[0], 0, 0, "own entry")] and c.positions("dl0_X")[0] + 1 == c.positions("dl0_Y")[0]
    both = ok_steps(c, "both", tr)
    assert [t["flip"] for t in both] == [False, True, False] and both[0]["m"] == 2 and both[2]["m"] == 3
    # a window that holds one read twice: the mirror declines
    c, m, ctr, tr = routed("twice")
    ps = c.positions("palindrome"); q = ps[-1]                     # Q: the last read of strand 1
    P = m.seq[q][:c.k]
    assert P == rg.revcomp(P) and list(m.entries(P)) == [q * 4, q * 4 + 3]
    assert [(t["i"], t["flip"], t["ended"]) for t in c.steps_of("palindrome", tr)] == [(ps[1], False, None), (ps[2], True, "mirror")]
    assert m._start(q) is None                                      # (a palindromic own entry starts no run)


def test_family_C_plans(routed):
    c, m, ctr, tr = routed("plans")
    def ms(name): return [(t["m"], t["plan_cut"]) for t in ok_steps(c, name, tr) if not t["flip"]]
    assert ms("n3") == [(RUN_LANES_MIN - 1, "bit9")] and ms("n4") == [(RUN_LANES_MIN, "bit9")]
    assert [t["lanes"] for t in ok_steps(c, "n3", tr)] == [False] and [t["lanes"] for t in ok_steps(c, "n4", tr)] == [True]
    assert ms("n16")[0][0] == RUN_MMAX - 1 and ms("n17") == [(RUN_MMAX, "mmax")]
    assert [x[0] for x in ms("n18")] == [RUN_MMAX, 1] and ms("n18")[0][1] == "mmax"
    assert [x[0] for x in ms("n34")] == [RUN_MMAX, RUN_MMAX, 1]
    s5 = ok_steps(c, "shift5", tr)
    assert (s5[0]["m"], s5[0]["plan_cut"], s5[0]["d1"]) == (12, "dmax", 5) and 12 * 5 <= RUN_DMAX < 13 * 5
    assert ("strand" in [t["plan_cut"] for t in ok_steps(c, "strand", tr) if not t["flip"]])
    assert "visit" in [t.get("plan_cut") for t in tr if t["ended"] is None]


def test_family_D_ring(routed):
    c, m, ctr, tr = routed("ring")
    for n, want in ((126, CAP - 1), (127, CAP), (128, CAP + 1)):
        assert max(m.tot(p) for p in c.positions("n%d" % n)) == want
    assert any(t["tot_after"] == CAP for t in ok_steps(c, "n127", tr)) and not any(t.get("tot_after", 0) > CAP for t in tr)
    # a planned step that finds no room and is retried with one read; a ring whose start has gone round; a read's slots across ring-relative slot 64
    c, m, ctr, tr = routed("dense")
    steps = ok_steps(c, "fw127", tr) + ok_steps(c, "fw100", tr)
    assert any(t["rc2"] and t["planned"] > 1 and t["m"] == 1 for t in steps)
    assert any(t["lanes"] and any(sa < 64 < sb for sa, sb in t["ranges"]) for t in steps)
    assert any(t["lanes"] and t["ring_start"] % CAP + t["ring_at_records"] > CAP for t in steps)          # (the ring's slots go round the end of the array)
    c, m, ctr, tr = routed("wrap")
    steps = [t for t in ok_steps(c, "wrap", tr) if not t["flip"]]
    assert any(a["run"] == b["run"] and a["ring_start"] < CAP <= b["ring_start"] for a in steps for b in steps)         # ... and its start does, within one run
    assert max(m.tot(p) for p in c.positions("wrap")) <= CAP
    # the full ring with an empty window last in a read's range, inside a planned step in the lane form
    c, m, ctr, tr = routed("full_ring")
    t = ok_steps(c, "block", tr)[0]
    assert t["m"] >= 3 and t["lanes"] and t["ring_at_records"] == CAP and t["empty_edge_window"]
    last = t["i"] + t["m"] - 1
    assert m.window_counts(last)[-1] == 0 and len(m.bucket[m.seq[last][-c.k:]]) == 101 and m.long_buckets() == 2
    assert t["ranges"][-1][1] == CAP
    # RUN_NMAX
    c, m, ctr, tr = routed("limits")
    assert [t["nNew"] for t in ok_steps(c, "nmax_64", tr)][-1] == RUN_NMAX
    assert [(t["nNew"], t["ended"]) for t in c.steps_of("nmax_65", tr)][-1] == (RUN_NMAX + 1, "step 2")


@pytest.mark.parametrize("name,cp", [("compares", 6), ("compares_L100", 8)])
def test_family_E_compares(name, cp, routed):
    c, m, ctr, tr = routed(name)
    assert ok_steps(c, "new_%d" % (3 * cp), tr)[-1]["nNew"] == 3 * cp and ok_steps(c, "new_%d" % (3 * cp + 1), tr)[-1]["nNew"] == 3 * cp + 1      # three passes; the first beyond RUN_NPRE
    assert [t.get("grown_by_type") for t in ok_steps(c, "grow0", tr)] == [0] and [t.get("grown_by_type") for t in ok_steps(c, "grow2", tr)] == [2]
    mutants = c.extra                                                # in the order of the loci: first dword, last dword, last base, middle
    for lname, mut in zip(("mut_first_dword", "mut_last_dword", "mut_last_base", "mut_middle"), mutants):
        t = c.steps_of(lname, tr)[-1]
        assert t["ended"] == "step 1" and t["failed_slot"][2] and m.seq[t["failed_slot"][0] >> 2] == mut


def test_family_E_frame_full_and_family_F_windows(routed):
    c, m, ctr, tr = routed("limits")
    t = c.steps_of("frame_full", tr)[-1]
    assert t["ended"] == "step 1" and t["frame_full"] > rg.RUN_F and [x["flip"] for x in ok_steps(c, "frame_full", tr)] == [True, False, False]
    a, b = c.steps_of("win_64", tr)[-1], c.steps_of("win_65", tr)[-1]
    assert (a["max_window"], a["nNew"], a["ended"]) == (64, 64, "step 1") and (b["max_window"], b["nNew"], b["ended"]) == (65, 65, "step 2")
    c, m, ctr, tr = routed("twice")
    for p in c.positions("self_again"):                             # the read's prefix k-mer is its suffix k-mer too: both own entries in its first and in its last window
        w = m.window_counts(p)
        assert m.seq[p][:c.k] == m.seq[p][-c.k:] and w[0] == w[-1] == 2 and m._start(p) is None


@pytest.mark.parametrize("name", list(rg.CAPABILITY))
def test_family_G_capability_edge(name, routed):
    c, m, ctr, tr = routed(name)
    kw, capable = rg.CAPABILITY[name]
    assert m.capable() == capable
    nwin = m.maxL - m.h + 1
    if name == "k23_128_windows": assert nwin == 128
    if name == "k22_129_windows": assert nwin == 129
    if name == "four_words_L100_k21": assert 2 * m.maxL + 9 <= 256
    if name == "eight_words_L160_k33": assert nwin == 128 and m.maxL == 160 and 2 * m.maxL + 9 > 256
    if name == "mixed_lengths": assert m.uniL == 0
    if capable:
        assert ctr[0] > 0 and any(t["flip"] for t in ok_steps(c, "mirror", tr)) and any(t["m"] == RUN_MMAX for t in ok_steps(c, "chain", tr))
    else:
        assert ctr == (0, 0, 0, 0)


def test_family_H_visits(routed):
    c, m, ctr, tr = routed("visits")
    V = rg.VISIT
    assert [c.first_pos(n) - 1 for n in ("b31", "c32", "g63")] == [V, 2 * V - 1, 3 * V - 1]        # minimiser changes at the first and at the last position of a nominal range
    v = m.visits()
    assert v[0] == (1, 1 + V) and v[1] == (1 + V, 3 * V) and v[2][0] == 3 * V                      # visit 2 starts at item 95, the last of [64, 96): visit 1 has 63 reads
    assert all(a < b for a, b in v) and all(v[x][1] == v[x + 1][0] for x in range(len(v) - 1)) and v[-1][1] == m.N + 1
    assert [len(c.positions(n)) for n in ("g63", "g64", "g65", "big_fw", "big_rc")] == [63, 64, 65, 133, 133]
    ps = sorted(c.positions("big_fw") + c.positions("big_rc"))
    assert ps == list(range(ps[0], ps[0] + 266)) and sum(1 for p in ps if m.meta[p] & 0x200) == 1
    assert max(m.tot(p) for p in ps) > CAP                                                          # (some of its reads have more candidates than the form has slots)


def test_counters_do_not_depend_on_the_form_of_the_records(routed):
    for name in rg.CASES:
        c, m, ctr, tr = routed(name)
        loops, all_lanes = m.route(0)[0], m.route(1)[0]
        flips = sum(1 for t in tr if t["ended"] is None and t["flip"])                                # (a strand change is one read, never in the lane form)
        assert loops[:2] == ctr[:2] == all_lanes[:2] and loops[2:] == (0, 0) and all_lanes[2:] == (ctr[0] - flips, ctr[1] - flips)
