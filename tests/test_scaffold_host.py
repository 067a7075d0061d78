"""CPU: the restatement of step 7 (tests/scaffold_model.py: stringOverlapSize, mergeDisconnectedEdges, a mergeFinal round, the loops' thresholds) pinned with literal
expectations on hand-built graphs whose end reads are chosen, the threshold call against hand values, the record sizes against the C compiler and the new calls on
a device-less context.  Also the builders the GPU tests share."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import fixtures as fx
import sage2_amd as s2
import scaffold_model as SM
import extend_model as X
import test_mate_estimate_host as H
import test_links_host as LH

LENGTHS = [11, 12, 32, 33, 64, 65, 75, 150]


def rnd(n, seed):
    return "".join(np.random.default_rng(seed).choice(list("ACGT"), size=n))


def other(c):
    return "ACGT"[("ACGT".index(c) + 1) % 4]


def planted(L1, L2, shift, mism, seed):
    """(s1, s2): s2 is random, s1 is `shift` bases that match nothing followed by s2's prefix with exactly `mism` mismatches in the part that faces s2, spread
    from its far end.  No smaller shift can pass for the seeds used (asserted by the callers through the two restatements)"""
    s2_ = rnd(L2, seed); n = min(L2 - shift, L1 - shift)
    head = "".join(other(other(s2_[j % L2])) for j in range(shift))                    # differs from s2 at shift 0 everywhere
    body = list(s2_[:L1 - shift]) + list(rnd(max(0, L1 - shift - L2), seed + 1))
    for x in range(mism):
        j = n - 1 - 3 * x
        body[j] = other(body[j])
    s1 = (head + "".join(body))[:L1]
    assert len(s1) == L1 and sum(1 for j in range(n) if s1[shift + j] != s2_[j]) == mism
    return s1, s2_


# ------------------------------------------------------------------------------------------ builders shared with the reference and GPU tests
def components(cases, where, fillers):
    """cases: [(s1, s2, flow1, flow2, variant)] -> records of two edges per case, X = filler -> read s1 and Y = read s2 -> filler, typed so that the forward list of
    JOIN(X, Y) spells node1 as s1 and node2 as s2 whichever strand the store keeps; variant picks the other type of the same spelling.  Pool halves 4 i (X), 4 i + 2 (Y)"""
    recs = []; f = iter(fillers)
    for n, (s1, s2_, f1, f2, variant) in enumerate(cases):
        (n1, fwd1), (n2, fwd2) = where[s1], where[s2_]
        tx = ((1, 3) if fwd1 else (0, 2))[variant & 1]; ty = ((2, 3) if fwd2 else (0, 1))[(variant >> 1) & 1]
        Xr = H.rec(next(f), n1, tx, 300 + n % 7, [(next(f), n % 2, 0, 30 + n % 11, 70), (next(f), 1, 0, 70, 41 + n % 5)])
        Yr = H.rec(n2, next(f), ty, 250 + n % 5, [(next(f), 1 - n % 2, 0, 50 + n % 3, 60)])
        for r, fl in ((Xr, f1), (Yr, f2)):
            t = H.twin_of(r); r["flow"] = t["flow"] = float(fl); recs += [r, t]
    return recs


def pinned_cases():
    """(s1, s2, expected forward overlap): every pinned case of tests/test_scaffold_host.py that two distinct reads can make"""
    out = []
    for L in LENGTHS:
        shift = min(max(1, (L - 10) // 2), L - 11); allowed = (L - shift) // 10 + 1
        s1, s2_ = planted(L, L, shift, allowed, 100 + L); out.append((s1, s2_, shift))
        s1, s2_ = planted(L, L, shift, allowed + 1, 1100 + L); out.append((s1, s2_, SM.overlap_rule(s1, s2_)))      # (not at `shift`: asserted below)
        assert out[-1][2] == -1 or out[-1][2] > shift
        for mism in (2, 3):
            s1, s2_ = planted(L, L, L - 11, mism, 200 + 1000 * mism + L); out.append((s1, s2_, L - 11 if mism == 2 else -1))
    unit = rnd(60, 7); per = (unit * 3)[:150]
    out += [(rnd(10, 8) + per[:140], per, 10), (rnd(70, 9) + per[:80], per[:149] + other(per[149]), 70)]
    out += [("T" * 40, "ACGTACGTACGT", 11), ("G" * 41, "AAAAAAAAAAAA", 11), ("C" * 23, "A" * 13, 12), ("C" * 21, "AG" * 6, -1)]
    s75 = rnd(75, 11); out.append((s75[:64], s75, -1))
    s65 = rnd(65, 12); out.append((s65[:64], s65, 0))                               # a hit at shift 0: the gap branch
    s75b = rnd(75, 21); out.append((s75b, s75b[20:53], 20))                        # forward 20, twin none
    return out


def distinct(cases):
    seen = set()
    for s1, s2_, _ in cases:
        for s in (s1, s2_):
            assert s not in seen and SM.revcomp(s) not in seen, s
            seen.add(s)
    return seen


# the two read-store layouts above 8 words (tests/test_gpu_edges.py LAYOUT_TOPS): 16 words hold 252 to 504 bases, 32 words 505 to 1018; the lengths sit on the
# layouts' ends and on either side of a 32-base word, of the last word (992 = 31 * 32) and of half a layout
LONG_TOPS = {504: [252, 253, 256, 257, 503, 504], 1018: [505, 512, 513, 991, 992, 993, 1017, 1018]}
LONG_LENGTHS = LONG_TOPS[504] + LONG_TOPS[1018]


def long_rows(L):
    """(shift, planted mismatches, seed, pinned result) of the six cases of one length: the middle shift, the last one and shift 1, each with exactly the allowed
    mismatches and with one more (shift 1 at 1018 bases: 102 and 103 mismatches, the largest count there is)"""
    mid = (L - 10) // 2
    return [(mid, (L - mid) // 10 + 1, 100 + L, mid), (mid, (L - mid) // 10 + 2, 1100 + L, -1), (L - 11, 2, 2200 + L, L - 11), (L - 11, 3, 3200 + L, -1),
            (1, (L - 1) // 10 + 1, 4100 + L, 1), (1, (L - 1) // 10 + 2, 5100 + L, -1)]


def periodic_cases(top):
    """reads of period 300 as long as the layout allows: (s1, s2, the shifts that pass one by one); the first of them is the pinned result.  70 bases in front: 70, 370
    and at 1018 bases 670 and 970 as well (lane rounds 1, 5, 10 and 15); top - 318 in front: 700 and 1000 at 1018 bases (rounds 10 and 15), 186 and 486 at 504"""
    unit = rnd(300, 7 + top); per = (unit * 4)[:top]
    return [(rnd(70, 8 + top) + per[:top - 70], per, list(range(70, top - 10, 300))), (rnd(top - 318, 9 + top) + per[:318], per[:top - 1] + other(per[top - 1]), [top - 318, top - 18])]


def unequal_cases(top):
    """(s1, s2, pinned forward result) of reads of two lengths, in one layout by the longer: a short read against the longest and the other way round, half the
    layout against all of it, one base and 118 bases over, and a read whose first 18 bases are the long one's last.  Where s2 is the shorter by more than 10, a
    single facing base may mismatch (1 <= 1 / 10 + 1), so some shift below L2 always passes: a tail of a few bases decides before the empty comparison at i == L2
    is reached, at a shift the seeds fix.  The results are what both restatements say (test_unequal_lengths_on_the_long_layouts)"""
    half = 252 if top == 504 else 504                                                  # 252 against 504: the 16-word layout's own ends; 504 against 1018: two layouts' tops
    tails = {504: (37, 251, 31), 1018: (36, 502, 30)}[top]
    s = rnd(top, 60 + top); t = rnd(top, 61 + top); u = rnd(top, 62 + top); v = rnd(33, 63 + top); x = rnd(top, 64 + top); y = rnd(top - 8, 65 + top)
    return [(rnd(40, 50 + top), rnd(top, 51 + top), -1),                               # L2 - L1 = top - 40 positions of s2 face nothing: never passes
            (rnd(top, 52 + top), rnd(40, 53 + top), tails[0]),                         # a tail of s2 passes in lane round 1
            (rnd(half, 54 + top), rnd(top, 55 + top), -1), (rnd(top, 56 + top), rnd(half, 57 + top), tails[1]),      # a tail again: the last shift before s2 runs out
            (s[:top - 1], s, 0),                                                       # one base over, a hit at shift 0: the gap branch
            (t[:top - 118], t, -1),                                                    # 118 over: more than top / 10 + 1
            (u[:top - 18] + v[:18], v, tails[2]),                                      # 33 bases sit at s1's far end, but a tail passes before: forward early, the twin direction none
            (x[:top - 18] + y[:18], y, top - 18)]                                      # s2 is 8 bases shorter: forward passes in the last lane round, 10 bases facing 18; the twin has L2 > L1


def pinned_cases_long(lengths=None, top=None):
    """(s1, s2, expected forward overlap) on the 16- and 32-word layouts.  `lengths`: the six rows of long_rows() for each; `top` (504 or 1018): that layout's
    lengths and its periodic and unequal cases as well"""
    out = []
    for L in (lengths if lengths is not None else LONG_TOPS[top] if top else LONG_LENGTHS):
        for shift, mism, seed, want in long_rows(L):
            s1, s2_ = planted(L, L, shift, mism, seed); out.append((s1, s2_, want))
    if top is not None:
        out += [(s1, s2_, passing[0]) for s1, s2_, passing in periodic_cases(top)] + unequal_cases(top)
    return out



# ------------------------------------------------------------------------------------------ stringOverlapSize
@pytest.mark.parametrize("L", LENGTHS)
def test_overlap_at_a_shift_with_exactly_the_allowed_mismatches_and_one_more(L):
    shift = min(max(1, (L - 10) // 2), L - 11); allowed = (L - shift) // 10 + 1      # (11 bases have shift 0 alone)
    s1, s2_ = planted(L, L, shift, allowed, 100 + L)
    assert SM.overlap_size(s1, s2_) == SM.overlap_rule(s1, s2_) == shift
    t1, t2 = planted(L, L, shift, allowed + 1, 100 + L)
    got = SM.overlap_size(t1, t2)
    assert got == SM.overlap_rule(t1, t2) and (got == -1 or got > shift)


@pytest.mark.parametrize("L", LENGTHS)
def test_overlap_in_the_last_possible_shift(L):
    shift = L - 11                                                                     # the last i of [0, L1 - 10): 11 bases face each other, 2 mismatches allowed
    s1, s2_ = planted(L, L, shift, 2, 200 + L)
    assert SM.overlap_size(s1, s2_) == SM.overlap_rule(s1, s2_) == shift
    s1, s2_ = planted(L, L, shift, 3, 200 + L)
    assert SM.overlap_size(s1, s2_) == SM.overlap_rule(s1, s2_) == -1


def test_the_smaller_of_two_passing_shifts_wins_across_lane_rounds():
    """150 bases of period 60: a read that holds the other from base 10 on holds it from bases 70 and 130 on as well: shifts in the first, second and third group of
    64 shifts pass and the first wins; with 70 bases in front, the second group's shift 70 wins over 130 and the first group has none"""
    unit = rnd(60, 7); s2_ = (unit * 3)[:150]
    s1 = rnd(10, 8) + s2_[:140]
    assert [SM.overlap_rule(s1[i:] + "N" * i, s2_[:150 - i]) == 0 for i in (10, 70, 130)] == [True, True, True]
    assert SM.overlap_size(s1, s2_) == SM.overlap_rule(s1, s2_) == 10
    s1 = rnd(70, 9) + s2_[:80]
    assert SM.overlap_size(s1, s2_) == SM.overlap_rule(s1, s2_) == 70
    assert SM.overlap_size(s2_, s2_) == 0 and SM.overlap_size(rnd(5, 8) + s2_[:145], s2_) == 5


def test_a_shorter_second_read_runs_out_of_bases():
    """L2 < L1: at i = L2 nothing faces s1 and the empty comparison passes (0 <= 0 / 10 + 1); beyond it L2 - i is negative and no shift passes"""
    s2_ = "ACGTACGTACGT"; s1 = "T" * 40                                                # 12 against 40: every base of s2 but the Ts mismatches
    # i = 0..8: 12 - i bases, threshold (12 - i) / 10 + 1 = 2 or 1; mismatches 9, 8, 8, 7 (i = 3: ACGTACGTA has 2 T), ..., i = 10: AC, 2 mismatches > 1; i = 11: A, 1 <= 1
    assert SM.overlap_size(s1, s2_) == SM.overlap_rule(s1, s2_) == 11
    s1 = "G" * 40; s2_ = "AAAAAAAAAAAA"                                                # i = 11: one base, one mismatch allowed
    assert SM.overlap_size(s1, s2_) == 11
    s2_ = rnd(11, 3); s1 = "".join(other(c) for c in (s2_ * 4))[:33]                   # periodic mismatch everywhere: only the single-base and the empty comparisons pass
    assert SM.overlap_size(s1, s2_) == SM.overlap_rule(s1, s2_) == 10
    # L1 - 10 <= L2: the empty comparison is never reached
    assert SM.overlap_size("C" * 22, "A" * 12) == 11 and SM.overlap_size("C" * 21, "A" * 12) == -1 and SM.overlap_rule("C" * 21, "A" * 12) == -1


def test_a_longer_second_read_counts_the_overhang_as_mismatches():
    s2_ = rnd(75, 11); s1 = s2_[:64]                                                   # 64 against 75: 11 bases of s2 face nothing: 11 > 75 / 10 + 1
    assert SM.overlap_size(s1, s2_) == SM.overlap_rule(s1, s2_) == -1
    s2_ = rnd(65, 12); s1 = s2_[:64]                                                   # one base over: 1 <= 7
    assert SM.overlap_size(s1, s2_) == 0


@pytest.mark.parametrize("seed", range(6))
def test_the_two_restatements_agree_on_seeded_pairs(seed):
    rng = np.random.default_rng(seed)
    for _ in range(60):
        L1, L2 = (int(v) for v in rng.integers(11, 151, size=2))
        s2_ = rnd(L2, int(rng.integers(1 << 30)))
        if rng.integers(2) and L1 > 12:
            sh = int(rng.integers(0, L1 - 10)); s1 = (rnd(sh, int(rng.integers(1 << 30))) + s2_ + rnd(L1, 5))[:L1]
        else:
            s1 = rnd(L1, int(rng.integers(1 << 30)))
        assert SM.overlap_size(s1, s2_) == SM.overlap_rule(s1, s2_)


# ------------------------------------------------------------------------------------------ stringOverlapSize on reads of 252 to 1018 bases
@pytest.mark.parametrize("L", LONG_LENGTHS)
def test_long_reads_at_the_middle_the_last_and_the_first_shift(L):
    """six planted pairs per length: the allowed number of mismatches passes at the planted shift, one more passes nowhere"""
    rows = long_rows(L)
    assert [(r[0], r[3]) for r in rows] == [((L - 10) // 2, (L - 10) // 2), ((L - 10) // 2, -1), (L - 11, L - 11), (L - 11, -1), (1, 1), (1, -1)]
    assert L != 1018 or [(r[0], r[1]) for r in rows] == [(504, 52), (504, 53), (1007, 2), (1007, 3), (1, 102), (1, 103)]
    for (shift, mism, seed, want), (s1, s2_, pinned) in zip(rows, pinned_cases_long([L])):
        assert len(s1) == len(s2_) == L and pinned == want
        assert SM.overlap_size(s1, s2_) == SM.overlap_rule(s1, s2_) == want, (L, shift, mism)


@pytest.mark.parametrize("top", sorted(LONG_TOPS))
def test_the_smallest_of_several_passing_lane_rounds_wins_on_the_long_layouts(top):
    (a1, a2, pa), (b1, b2, pb) = periodic_cases(top)
    assert (pa, pb) == {504: ([70, 370], [186, 486]), 1018: ([70, 370, 670, 970], [700, 1000])}[top]
    for s1, s2_, passing in ((a1, a2, pa), (b1, b2, pb)):
        assert len(s1) == len(s2_) == top
        assert all(SM.overlap_rule(s1[i:] + "N" * i, s2_[:top - i]) == 0 for i in passing)      # each of them passes on its own
        assert SM.overlap_size(s1, s2_) == SM.overlap_rule(s1, s2_) == passing[0]
    assert {i >> 6 for i in pa + pb} == ({1, 5, 2, 7} if top == 504 else {1, 5, 10, 15})       # the groups of 64 shifts they lie in


@pytest.mark.parametrize("top", sorted(LONG_TOPS))
def test_unequal_lengths_on_the_long_layouts(top):
    cases = unequal_cases(top)
    assert [(len(a), len(b)) for a, b, _ in cases] == [(40, top), (top, 40), (top // 2 if top == 504 else 504, top), (top, top // 2 if top == 504 else 504),
                                                        (top - 1, top), (top - 118, top), (top, 33), (top, top - 8)]
    for s1, s2_, want in cases:
        assert SM.overlap_size(s1, s2_) == SM.overlap_rule(s1, s2_) == want, (len(s1), len(s2_))
    assert [w for _, _, w in cases] == {504: [-1, 37, -1, 251, 0, -1, 31, 486], 1018: [-1, 36, -1, 502, 0, -1, 30, 1000]}[top]
    assert all(0 < cases[n][2] < len(cases[n][1]) for n in (1, 3, 6))                  # the tails: below L2, before the empty comparison
    # the twin direction of the last two differs from the forward one
    for s1, s2_, want in cases[6:]:
        t = SM.overlap_size(SM.revcomp(s2_), SM.revcomp(s1))
        assert t == SM.overlap_rule(SM.revcomp(s2_), SM.revcomp(s1)) and t != want


@pytest.mark.parametrize("top", sorted(LONG_TOPS))
def test_the_long_cases_are_distinct_reads(top):
    cases = pinned_cases_long(top=top)
    assert len(cases) == 6 * len(LONG_TOPS[top]) + 2 + 8 and len(distinct(cases)) == 2 * len(cases)
    assert max(len(s) for c in cases for s in c[:2]) == top and min(len(s) for c in cases[:6 * len(LONG_TOPS[top])] for s in c[:2]) == (252 if top == 504 else 505)
    assert len(distinct(pinned_cases_long(LONG_LENGTHS))) == 2 * 6 * len(LONG_LENGTHS)


def long_batch(top, joins=128):
    """(s1, s2, None) of a seeded batch on one long layout: s1 of top // 2 + 1 to top bases; s2 as long, every fourth of 11 to 150 bases (the longer read decides
    the layout, the shorter one's words end early), every eighth as long as s1 with the planted shift in s1's last 58 bases; s1 random (every fourth) or s2's prefix
    behind `shift` bases with 0 to 8 flipped bases"""
    rng = np.random.default_rng(31 + top); cases = []
    for n in range(joins):
        L1 = int(rng.integers(top - 28, top + 1)) if n % 8 == 1 else int(rng.integers(top // 2 + 1, top + 1))
        L2 = L1 if n % 8 == 1 else int(rng.integers(11, 151)) if n % 4 == 3 else int(rng.integers(top // 2 + 1, top + 1))
        s2_ = rnd(L2, 50000 + 7 * top + n)
        if n % 4 == 0:
            s1 = rnd(L1, 60000 + 7 * top + n)
        else:
            sh = int(rng.integers(L1 - 58 if n % 8 == 1 else 0, L1 - 10)); body = list((s2_ + rnd(L1, 70000 + 7 * top + n))[:L1])
            for x in rng.integers(0, max(1, min(L1 - sh, L2)), size=int(rng.integers(0, 9))):
                body[int(x)] = other(body[int(x)])
            s1 = (rnd(sh, 80000 + 7 * top + n) + "".join(body))[:L1]
        cases.append((s1, s2_, None))
    return cases


def batch_conditions(top, found):
    """what a batch on a long layout has to hold, by the model's values of both directions: hits, misses, hits from lane round 4 on and, with 1018 bases, hits in
    the last round, where the words past the read are read"""
    return sum(o > 0 for o in found) > 50 and sum(o == -1 for o in found) > 10 and sum(o > 191 for o in found) > 10 and (top != 1018 or sum(o >= 960 for o in found) > 3)


@pytest.mark.parametrize("top", sorted(LONG_TOPS))
def test_the_seeded_long_batch_is_not_vacuous(top):
    cases = long_batch(top); distinct(cases)
    found = [o for s1, s2_, _ in cases for o in (SM.overlap_size(s1, s2_), SM.overlap_size(SM.revcomp(s2_), SM.revcomp(s1)))]
    assert len(found) == 256 and batch_conditions(top, found), [sum(o > 0 for o in found), sum(o == -1 for o in found), sum(o > 191 for o in found), sum(o >= 960 for o in found)]
    assert max(len(s1) for s1, _, _ in cases) > (251 if top == 504 else 504)           # the layout the batch is meant for


# ------------------------------------------------------------------------------------------ JOIN on chosen reads
def two_edges(t1=3, t2=3, f1=1.0, f2=1.0, nodes=(1, 2, 3, 4), lens=(100, 120)):
    """two composite edges in components of their own: X = nodes[0] -> nodes[1], Y = nodes[2] -> nodes[3]; pool halves 0 (X), 1, 2 (Y), 3"""
    Xr = H.rec(nodes[0], nodes[1], t1, lens[0], [(20, 1, 0, 30, 70)]); Yr = H.rec(nodes[2], nodes[3], t2, lens[1], [(21, 1, 0, 50, 70)])
    recs = []
    for r, f in ((Xr, f1), (Yr, f2)):
        t = H.twin_of(r); r["flow"] = t["flow"] = float(f); recs += [r, t]
    return (0, 30, 60), recs


def graph_of(header, recs):
    return SM.Graph(H.parse_graph(H.graph_text(header, recs)))


def test_two_components_joined_with_a_gap_written_out_by_hand():
    header, recs = two_edges()
    g = graph_of(header, recs)
    seqs = {2: rnd(60, 1), 3: rnd(60, 2)}
    assert SM.overlap_rule(seqs[2], seqs[3]) == -1 and SM.overlap_rule(SM.revcomp(seqs[3]), SM.revcomp(seqs[2])) == -1
    assert g.join(0, 2, 7, seqs) == 4
    fw = dict(frm=1, to=4, type=3, reducible=1, len=287, flow=1.0, list=[(20, 1, 0, 30, 70), (2, 1, 0, 70, 67), (3, 1, 0, 67, 50), (21, 1, 0, 50, 70)])
    tw = dict(frm=4, to=1, type=0, reducible=1, len=287, flow=1.0, list=[(21, 0, 0, 70, 50), (3, 0, 0, 50, 67), (2, 0, 0, 67, 70), (20, 0, 0, 70, 30)])
    assert g.text() == H.graph_text(header, [fw, tw])                                  # both operands had flow 1: only the new pair is left
    assert g.last == dict(type=3, deleted=[True, True], overlap=(-1, -1), how=(SM.GAPPED, SM.GAPPED))


def test_the_three_distance_cases_and_the_wrap():
    header, recs = two_edges()
    s3 = rnd(60, 2); s2_ = rnd(25, 9) + s3[:35]                                        # read 2 ends in read 3's first 35 bases: shift 25
    for gap, seqs, want_len, d, how, ov in ((7, {2: s2_, 3: s3}, 245, (25, 25), SM.OVERLAP, 25),
                                            (-5, {2: rnd(60, 1), 3: s3}, 280, (60, 60), SM.CONCAT, -1),
                                            (0, {2: rnd(60, 1), 3: s3}, 280, (60, 60), SM.GAPPED, -1),
                                            (1990, {2: rnd(60, 1), 3: s3}, 2270, (2, 2), SM.GAPPED, -1),      # 2050 wraps to 2 in the entry, the length keeps it
                                            (7, {2: s3, 3: s3}, 287, (67, 67), SM.GAPPED, 0)):               # an overlap at shift 0 is the gap branch
        g = graph_of(header, recs); g.join(0, 2, gap, seqs)
        fw, tw = g.h[4], g.h[5]
        assert (fw["len"], tw["len"]) == (want_len, want_len) and g.last["how"] == (how, how) and g.last["overlap"] == (ov, ov)
        assert fw["list"][1] == (2, 1, 0, 70, d[0]) and fw["list"][2] == (3, 1, 0, d[1], 50)


def test_equal_end_nodes_make_one_entry():
    header, recs = two_edges(nodes=(1, 2, 2, 4))
    g = graph_of(header, recs); g.join(0, 2, 50, {})
    assert g.h[4]["list"] == [(20, 1, 0, 30, 70), (2, 1, 0, 70, 50), (21, 1, 0, 50, 70)] and g.h[4]["len"] == 220 and g.last["how"] == (SM.EQUAL, SM.EQUAL)
    assert g.h[5]["list"] == [(21, 0, 0, 70, 50), (2, 0, 0, 50, 70), (20, 0, 0, 70, 30)] and g.last["overlap"] == (-2, -2)


def test_unequal_read_lengths_where_forward_and_twin_disagree():
    """read 2 has 75 bases, read 3 has 33 and sits inside read 2 from base 20 on: forward OVERLAP(read 2, read 3) = 20 (all 33 bases face read 2); the twin
    compares rc(read 3) with rc(read 2): a shift would need rc(read 2)'s 75 bases to face at most 33: none passes but the ones that run out, none here (33 - 10 = 23 shifts)"""
    s2_ = rnd(75, 21); s3 = s2_[20:53]
    header, recs = two_edges()
    g = graph_of(header, recs); g.join(0, 2, 4, {2: s2_, 3: s3})
    assert g.last["overlap"] == (20, -1) and g.last["how"] == (SM.OVERLAP, SM.GAPPED)
    assert (g.h[4]["len"], g.h[5]["len"]) == (100 + 120 + 20, 100 + 120 + 4 + 33)      # the twin's node1 is read 3: gap + 33
    assert g.h[5]["list"][1] == (3, 0, 0, 50, 37) and g.h[5]["list"][2] == (2, 0, 0, 79, 70)


@pytest.mark.parametrize("t1,t2,want", [(0, 0, 0), (1, 2, 0), (0, 1, 1), (1, 3, 1), (2, 0, 2), (3, 2, 2), (2, 1, 3), (3, 3, 3), (0, 2, 0), (3, 0, 2), (1, 1, 1), (2, 3, 3)])
def test_the_type_rule_never_refuses(t1, t2, want):
    assert SM.join_type(t1, t2) == want


def test_an_operand_with_flow_2_is_kept_and_loses_one():
    header, recs = two_edges(f1=2.0, f2=0.0)
    g = graph_of(header, recs); g.join(0, 2, 3, {2: rnd(60, 1), 3: rnd(60, 2)})
    assert g.last["deleted"] == [False, True] and g.alive == [True, False, True] and g.h[0]["flow"] == g.h[1]["flow"] == 1.0 and g.h[4]["flow"] == 1.0


# ------------------------------------------------------------------------------------------ the thresholds
def test_thresholds_of_the_five_loops():
    # 1000 reads of 100 bases on 2500: coverage 40; T(0.10) = ceil(4 * 1) = 4, T(0.05) = 2
    for loop in (1, 2):
        assert [s2.scaffold_threshold(1000, 100, 2500, loop, it) for it in (1, 5, 6, 9)] == [4, 4, 2, 2] == [SM.threshold(1000, 100, 2500, loop, it) for it in (1, 5, 6, 9)]
    assert [s2.scaffold_threshold(1000, 100, 2500, loop, it) for loop in (3, 4, 5) for it in (1, 7)] == [2, 2, 1, 1, 1, 1]
    # the quotient is an integer: 999 * 100 / 2500 = 39 -> 0.10 * 39 = 3.9 -> 4; 0.05 * 39 = 1.95 -> 2
    assert (s2.scaffold_threshold(999, 100, 2500, 1, 1), s2.scaffold_threshold(999, 100, 2500, 1, 6)) == (4, 2)
    # coverage 6 at read length 60: 0.6 * (100 / 60) = 1.0 -> 1 and 0.3 * 1.67 = 0.5 -> 1: the two values coincide, loop 1 can end in its first round
    assert (s2.scaffold_threshold(200, 60, 2000, 1, 1), s2.scaffold_threshold(200, 60, 2000, 1, 6)) == (1, 1) == (SM.threshold(200, 60, 2000, 1, 1), SM.threshold(200, 60, 2000, 1, 6))
    for args in ((1000, 0, 2500, 1, 1), (1000, 100, 0, 1, 1), (1000, 100, 2500, 0, 1), (1000, 100, 2500, 6, 1), (1000, 100, 2500, 1, 0)):
        with pytest.raises(s2.Sage2ovError) as e:
            s2.scaffold_threshold(*args)
        assert e.value.code == -1


# ------------------------------------------------------------------------------------------ rounds on the hand-built link graph
def hand(flows=None, extra=None):
    """LH.hand_link_graph with flows set on pairs {ordinal: flow} and extra library-1 mates; seqs: seeded 60-mers for every node (no two overlap)"""
    N, header, recs, pairs = LH.hand_link_graph()
    for q, f in (flows or {}).items():
        recs[2 * q]["flow"] = recs[2 * q + 1]["flow"] = float(f)
    if extra:
        pairs = dict(pairs); pairs[1] = pairs[1] + list(extra)
    seqs = {i: rnd(60, 1000 + i) for i in range(1, N + 1)}
    return N, header, recs, pairs, seqs


def run_round(high, flag=1, small=False, **kw):
    N, header, recs, pairs, seqs = hand(**kw)
    g = graph_of(header, recs); b = X.Bounds(g, pairs)
    return g, SM.round_(g, pairs, b, LH.HAND_K, high, flag, small, seqs), (pairs, b, seqs)


def test_round_on_the_hand_graph_rows_follow_rule_a_and_the_order():
    g, r, _ = run_round(99)
    # 28 rows pass the FINAL filter in both directions together; rule (a) keeps the direction whose first half has the lower pool index
    assert r["rows"] == 14 and r["below_threshold"] == 14 and not r["merges"] and r["batches"] == 0 and not r["outside_reference"]
    g, r, _ = run_round(99, small=True)
    assert r["rows"] == 14


def test_round_joins_the_best_supported_row_and_erases_by_its_node():
    """high 2: the row of support 5 is LINK(C, D) -- C = 10 -> 2 (type 1, flow 1) has the lower pool index -- so edge_1 = C's twin 2 -> 10 and edge_2 = D = 10 -> 31 (flow
    1.5): the end nodes are equal, no search; C goes, D stays with 0.5.  Every row filed under node 10 leaves the map, and the rows that name C afterwards are
    rule (d)'s.  Four rows lie below 2."""
    g, r, _ = run_round(2)
    assert SM.joins_rows(r) == [(2, 31, 5, -86, 1, 3, 1, -2, -2, 0, 1, 0, SM.EQUAL, SM.EQUAL)]
    assert (r["rows"], r["below_threshold"], r["skipped"], r["blocked"], r["cycles"], r["batches"], r["ties"], r["outside_reference"]) == (14, 4, 9, 0, 0, 1, False, True)
    new = g.h[-2]
    assert (new["frm"], new["to"], new["type"], new["len"], new["flow"]) == (2, 31, 0, 280 + 290, 1.0) and g.h[6]["flow"] == 0.5 and not g.alive[2] and g.alive[3]
    assert r["rows"] == r["below_threshold"] + r["skipped"] + r["blocked"] + r["cycles"] + len(r["merges"])


def test_rows_with_competitors_are_blocked_under_flag_1_and_joined_under_flag_2():
    """high 1: after the join at node 10 four rows are left whose operands have two rows of support >= 1 on one side: mergeAccordingToSupport (<= 1) refuses
    them, mergeAccordingToSupport2 (<= 2) joins two of them across components, with gaps 2 and 7 spelled as N runs, and skips the two that name their operands"""
    g1, r1, _ = run_round(1, flag=1)
    assert (len(r1["merges"]), r1["blocked"], r1["skipped"], r1["ties"]) == (1, 4, 9, True)
    g2, r2, _ = run_round(1, flag=2)
    assert SM.joins_rows(r2) == [(2, 31, 5, -86, 1, 3, 1, -2, -2, 0, 1, 0, SM.EQUAL, SM.EQUAL),
                                 (28, 11, 1, 2, 14, 8, 8, -1, -1, 0, 1, 1, SM.GAPPED, SM.GAPPED), (23, 26, 1, 7, 10, 13, 10, -1, -1, 1, 1, 1, SM.GAPPED, SM.GAPPED)]
    assert (r2["blocked"], r2["skipped"], r2["gapped"], r2["batches"]) == (0, 11, 4, 1)
    # mergeFinalSmall's filter (both lengths below 500) brings other rows: G . Hh with the negative gap -3 is concatenated
    g3, r3, _ = run_round(1, flag=2, small=True)
    assert [(m["frm"], m["to"], m["gap"], m["how"]) for m in r3["merges"]] == [(2, 31, -86, (0, 0)), (21, 23, -3, (SM.CONCAT, SM.CONCAT)), (24, 26, -60, (SM.CONCAT, SM.CONCAT))]
    assert g3.h[-4]["len"] == 201 + 200 + 60 and g3.h[-4]["list"][4:6] == [(20, 0, 0, 10, 60), (22, 1, 0, 60, 12)]      # edge_1 is G's twin 21 -> 20: its last distNext is G's first distPrevious


def test_model_round_is_deterministic_and_a_second_round_sees_the_new_graph():
    g, r, (pairs, b, seqs) = run_round(1)
    g_, r_, _ = run_round(1)
    assert g.text() == g_.text() and SM.joins_rows(r) == SM.joins_rows(r_)
    before = sum(g.alive)
    r2 = SM.round_(g, pairs, b, LH.HAND_K, 1, 1, False, seqs)
    assert sum(g.alive) == before - sum(m["first_deleted"] + m["second_deleted"] - 1 for m in r2["merges"])


KEPT = {q: 50 for q in range(13)}      # flows that keep every operand however often a round names it


def test_a_kept_operand_is_named_again_in_the_same_round():
    """every flow 50, `high` 1, flag 2: G's twin . Hh (21 -> 23, gap -3, concatenated) keeps Hh; the later row Hh's twin . J (23 -> 26, gap 7) names Hh again.  By (c) Hh
    is spent: it has no feasible pairs any more and counts on no side, so the row joins, and by (e) the first batch is applied before it: two batches"""
    g, r, _ = run_round(1, flag=2, flows=KEPT)
    assert SM.joins_rows(r) == [(2, 31, 5, -86, 1, 3, 2, -2, -2, 0, 0, 0, SM.EQUAL, SM.EQUAL), (21, 23, 2, -3, 9, 10, 12, -1, -1, 1, 0, 0, SM.CONCAT, SM.CONCAT),
                                (28, 11, 1, 2, 14, 8, 10, -1, -1, 0, 0, 0, SM.GAPPED, SM.GAPPED), (23, 26, 1, 7, 10, 13, 14, -1, -1, 1, 0, 0, SM.GAPPED, SM.GAPPED)]
    assert (r["named_again"], r["batches"], r["skipped"], r["outside_reference"]) == (1, 2, 11, False)
    assert g.h[2 * 8]["flow"] == 48.0 and sum(g.alive) == 13 + 4                      # Hh lost 1.0 twice; nothing was deleted


def test_a_row_whose_own_partner_is_not_the_tables_half(monkeypatch):
    """every flow 50, `high` 1, flag 1: one row's edge_2 (or edge_1) is not E of its pair, so the feasible list's entry for that pair is another pointer and the
    row's own partner counts as a competitor (:565, :573).  With the test of identity inverted the round ends differently: the case is decided by it"""
    g, r, _ = run_round(1, flag=1, flows=KEPT)
    assert (len(r["merges"]), r["blocked"], r["skipped"], r["identity_decides"]) == (1, 5, 9, 1)
    real = SM.Graph.is_E
    monkeypatch.setattr(SM.Graph, "is_E", lambda self, x: not real(self, x))
    g2, r2, _ = run_round(1, flag=1, flows=KEPT)
    assert (len(r2["merges"]), r2["blocked"]) != (len(r["merges"]), r["blocked"])


CYCLE = dict(extra=[(70, 1, 80, 1)], flows={2: 2, 7: 1, 11: 2, 12: 2})      # one more library-1 mate, read 70 on G with read 80 on J: G, Hh and J are linked two by two


def test_a_cycle_by_hand():
    """G (pair 7), Hh (8) and J (10) sit in components of their own; mates link G-Hh (support 2) and Hh-J (1), and the added mate links G-J (1).  C, G, I and Kk
    have flows that keep the round inside the reference (no operand is deleted while its rows are listed).  `high` 1, mergeFinal's filter.  Rows in order (b):
      0  C's twin . D (support 5)   joins at node 10; every row filed under node 10 leaves the map: rows 1, 4-6, 8-12 are skipped
      2  G's twin . Hh (2)          J counts on Hh's side (SEARCH[J, Hh] through the mirrored key) and on G's side (SEARCH[G, J]): a CYCLE, with 2 and 1 counted --
                                    within flag 2's limit; on Hh's side G itself counts too, because edge_1 is G's twin and not the table's half of its pair
      3  I's twin . Kk (1)          no common pair: on Kk's side I itself counts (edge_1 is I's twin, not the table's half), on I's side J and Kk itself: 1 and 2 --
                                    flag 1 refuses it (BLOCKED), flag 2 joins it, after the cycle
      7  J's twin . I (1)           flag 1: blocked (2 and 2); flag 2: I is spent by row 3's join, the key went with node 28's rows: skipped
      13 G's twin . J, 14 Hh's twin . J, 15 Hh's twin . J's twin (1 each): cycles through Hh, G and G; under flag 1 row 13 counts 3 on J's side as well: over
                                    the limit AND a cycle -- the cycle test comes first (:602 tests both, the counters tell them apart here)"""
    g2, r2, _ = run_round(1, flag=2, **CYCLE)
    v = {i: x for i, x in enumerate(r2["verdicts"]) if x[0] != "skipped"}
    assert v == {0: ("join", [], [1]), 2: ("cycle", [7, 10], [10]), 3: ("join", [11], [10, 12]), 13: ("cycle", [7, 8], [8]), 14: ("cycle", [7, 8], [7]), 15: ("cycle", [7, 8], [7, 10])}
    assert SM.joins_rows(r2) == [(2, 31, 5, -86, 1, 3, 2, -2, -2, 0, 0, 0, SM.EQUAL, SM.EQUAL), (28, 11, 1, 2, 14, 8, 10, -1, -1, 0, 0, 0, SM.GAPPED, SM.GAPPED)]
    assert (r2["rows"], r2["cycles"], r2["blocked"], r2["skipped"], r2["outside_reference"]) == (16, 4, 0, 10, False)
    g1, r1, _ = run_round(1, flag=1, **CYCLE)
    v = {i: x for i, x in enumerate(r1["verdicts"]) if x[0] != "skipped"}
    assert v == {0: ("join", [], [1]), 2: ("cycle", [7, 10], [10]), 3: ("blocked", [11], [10, 12]), 7: ("blocked", [10, 12], [7, 8]),
                 13: ("cycle", [7, 8, 11], [8]), 14: ("cycle", [7, 8, 11], [7]), 15: ("cycle", [7, 8, 11], [7, 10])}
    assert len(r1["merges"]) == 1 and (r1["cycles"], r1["blocked"], r1["skipped"], r1["outside_reference"]) == (4, 2, 9, False)
    # without the added mate G's twin . Hh is no cycle: it joins (flag 2)
    g0, r0, _ = run_round(1, flag=2, flows=CYCLE["flows"])
    assert r0["cycles"] == 0


def test_generated_graph_reaches_cycles_blocked_rows_and_a_second_batch():
    """the generated hub graph of tests/compgen.py with node mates and long-range mates, `high` 1 under flag 2: round 1 joins 28 rows, refuses 113 for their
    competitors and 4 for a cycle, and names a kept operand again twice (three batches)"""
    import compgen as CG
    N, header, recs = CG.case_e(2)
    parsed = H.parse_graph(H.graph_text(header, recs)); pairs = LH.merged(CG.mates_e(parsed, 2), LH.long_range_mates(parsed))
    seqs = {i: rnd(60, 4000 + i) for i in range(1, N + 1)}
    g = SM.Graph(parsed); b = X.Bounds(g, pairs)
    r = SM.round_(g, pairs, b, CG.K, 1, 2, False, seqs)
    assert (len(r["merges"]), r["rows"], r["blocked"], r["cycles"], r["batches"], r["skipped"], r["ties"]) == (28, 238, 113, 4, 3, 93, True)
    assert r["rows"] == r["below_threshold"] + r["skipped"] + r["blocked"] + r["cycles"] + len(r["merges"])
    g = SM.Graph(parsed)
    r = SM.round_(g, pairs, b, CG.K, 1, 1, False, seqs)                                # mergeAccordingToSupport admits one competitor, not two
    assert (len(r["merges"]), r["blocked"], r["cycles"], r["batches"]) == (4, 228, 4, 1)


# ------------------------------------------------------------------------------------------ the C ABI without a GPU
def test_record_sizes_against_the_c_compiler(tmp_path):
    assert s2.JOIN_DTYPE.itemsize == 48 and C.sizeof(s2.ScaffoldCounts) == 144 and C.sizeof(s2.ScaffoldStats) == 304
    src, exe = str(tmp_path / "sz.c"), str(tmp_path / "sz")
    fields = list(s2.JOIN_DTYPE.names)
    open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "sage2ov.h"\nint main(void) { printf("%zu", sizeof(sage2ov_join));\n'
                         + "".join('printf(" %%zu", offsetof(sage2ov_join, %s));\n' % f for f in fields)
                         + 'printf(" %zu %zu", sizeof(sage2ov_scaffold_counts), sizeof(sage2ov_scaffold_stats)); return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(fx.ROOT, "include"), src, "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got == [48] + [s2.JOIN_DTYPE.fields[f][1] for f in fields] + [144, 304]
    assert (s2.JOIN_EQUAL, s2.JOIN_OVERLAP, s2.JOIN_CONCAT, s2.JOIN_GAPPED) == (SM.EQUAL, SM.OVERLAP, SM.CONCAT, SM.GAPPED)


def test_device_less_context_refuses():
    rng = np.random.default_rng(5)
    reads = sorted({"".join(rng.choice(list("ACGT"), size=60)) for _ in range(20)})
    bases = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(); off = np.arange(0, (len(reads) + 1) * 60, 60, dtype=np.uint64)
    ctx = s2.Context(40, device=-2); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
    for call in (lambda: ctx.join_pairs([(0, 0)], [(1, 0)], [3]), lambda: ctx.scaffold_round(2), lambda: ctx.scaffold_round(1, 2, True), ctx.scaffold):
        with pytest.raises(s2.Sage2ovError) as e:
            call()
        assert e.value.code == -3
    st = ctx.scaffold_stats(); assert (st.rounds, st.total.rows, st.total.merged) == (0, 0, 0) and len(ctx.scaffold_merges()) == 0
    n = C.c_uint64(7)
    assert s2.lib().sage2ov_scaffold_merges_count(None, C.byref(n)) == -1 and s2.lib().sage2ov_scaffold_round(None, C.c_int(1), C.c_int(1), C.c_int(0), None) == -1
    with pytest.raises(s2.Sage2ovError) as e:
        ctx.scaffold_round(2, 3)                                                       # no such flag
    assert e.value.code == -1
    ctx.close()
