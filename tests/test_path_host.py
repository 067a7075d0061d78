"""CPU: the restatement of PATH SUPPORTS (include/sage2ov.h; tests/path_model.py) pinned by hand on a hand-built graph -- a fork behind short edges, which the first
loop of extendContigs cannot merge and the second can -- and on the edges of every rule: claims, rows and merges are written out here.  Also: the sizes of the new
records and the new calls on a device-less context."""
import ctypes as C
import types
import numpy as np
import pytest
import sage2_amd as s2
import extend_model as X
import path_model as PM
import test_mate_estimate_host as H
import test_mate_support_host as MS

# the pool of PM.fork_graph: pair p = halves 2 p, 2 p + 1
A, B, Cc, D, E, F, Z = 0, 2, 4, 6, 8, 10, 12


def test_estimate_of_the_hand_built_graphs():
    N, header, recs, pairs, g, est = PM.load("fork")
    e = est.ests[1]
    assert (e["valid"], e["mean"], e["lower"], e["upper"]) == (1, 476, 251, 701) and (est.min_upper, est.max_upper) == (701, 2103)
    # the pairs on Z have both mates on one edge: flag 0; every pair across the fork: flag 1
    flags = dict(zip(PM.entries_of(pairs, 1), est.flags[1]))
    assert flags[(71, 75, 1, 0)] == 0 and flags[(75, 71, 0, 1)] == 0 and flags[(42, 52, 1, 1)] == 1 and sum(est.flags[1]) == 12


def test_the_fork_claims_rows_and_what_the_first_loop_sees():
    N, header, recs, pairs, g, est = PM.load("fork")
    sw = PM.sweep(g, pairs, est)
    assert sw["claim"] == {41: 1, 42: 1, 43: 1, 44: 2, 45: 2, 46: 2, 51: 11, 52: 11, 53: 11, 54: 12, 55: 12, 56: 12, 61: 10, 62: 10,
                           71: 30, 72: 30, 73: 30, 74: 30, 75: 30, 76: 30, 77: 30, 78: 30, 79: 30}
    assert sw["starts"] == {1: [1, 10], 2: [2, 10], 10: [10, 11, 12], 11: [11, 21], 12: [12, 22], 30: [30, 31]}
    # from node 10, newest first: D, D F, C, C E, then the twins of B and A
    assert [p for p in sw["paths"][1] if g.h[p[0][0]]["frm"] == 10] == [((D,), 0), ((D, F), 60), ((Cc,), 0), ((Cc, E), 60), ((B ^ 1,), 0), ((A ^ 1,), 0)]
    assert sw["rows"] == [(10, B, D, 3), (10, A, Cc, 3), (11, Cc, E, 3), (12, D, F, 3)]
    assert PM.export_rows(g, sw["rows"]) == [(10, 1, 3, 2, 12, 3, 0, 0), (10, 0, 2, 1, 11, 3, 0, 0), (11, 2, 4, 10, 21, 3, 0, 0), (12, 3, 5, 10, 22, 3, 0, 0)]
    assert sw["stats"] == dict(claimed_reads=23, claiming_nodes=6, start_nodes=13, paths=54, capped_nodes=0, eligible_entries=6, voting_entries=6, records=12, rows=4,
                               key_collisions=0, mirrored=0)
    # the first loop finds nothing to merge here: no mate of A or B stands on C or D
    assert all(s == 0 for (_, _, _, s) in MS.all_supports(g.parsed(), pairs, MS.HAND_K))
    assert X.round_(g, pairs, est, MS.HAND_K, 2)["merges"] == []
    r = PM.round_(g, pairs, est, 2)
    assert [(m["node"], m["frm"], m["to"], m["support"]) for m in r["merges"]] == [(10, 2, 12, 3)] and r["order_dependent"] == 1      # (two rows of node 10 at the threshold)


def test_a_third_in_edge_divides_the_variants():
    """G's mates reach E and F.  Round 1 merges C.E and D.F, whose rows every pair voted for; then A's and B's rows meet G's (support 2 > low) among the ins: variant 0
    refuses both, variant 1 merges one per round (a merge takes every row filed under node 10 with it)"""
    want = {0: [[(11, 10, 21, 5), (12, 10, 22, 5)], []], 1: [[(11, 10, 21, 5), (12, 10, 22, 5)], [(10, 2, 22, 3)], [(10, 1, 21, 3)], []]}
    for variant in (0, 1):
        N, header, recs, pairs, g, est = PM.load("third")
        assert PM.sweep(g, pairs, est)["rows"] == [(10, 14, D, 2), (10, 14, Cc, 2), (10, B, D, 3), (10, A, Cc, 3), (11, Cc, E, 5), (12, D, F, 5)]
        got = []
        for rd in range(5):
            r = PM.round_(g, pairs, est, 2, 1, variant)
            got.append([(m["node"], m["frm"], m["to"], m["support"]) for m in r["merges"]])
            if rd == 1:
                assert (r["entries"], r["at_threshold"], r["refused"]) == ((4, 4, 4) if variant == 0 else (4, 4, 0))
            if not r["merges"]:
                break
        assert got == want[variant]
        rs = PM.extend(X.Graph(H.parse_graph(H.graph_text(header, recs))), pairs, est, 180 * 60 // 6, 180, variant)
        assert [len(r["merges"]) for r in rs] == [len(x) for x in want[variant]]


def test_seven_levels_and_no_eighth():
    N, header, recs, pairs, g, est = PM.load("chain")
    sw = PM.sweep(g, pairs, est)
    assert ((2, 4, 6, 8, 10, 12, 14), 300) in sw["paths"][1] and max(len(p[0]) for p in sw["paths"][1]) == 7
    # 41 -> 48 is found through the 7-edge path and votes for its seven pairs; 41 -> 49 is eligible and has no path
    assert sw["rows"] == [(j + 1, 2 * j - 2, 2 * j, 1) for j in range(1, 8)] and (sw["stats"]["eligible_entries"], sw["stats"]["voting_entries"]) == (2, 1)
    assert sw["stats"]["key_collisions"] == 1                                        # (1 ^ 2, 2 ^ 3) == (5 ^ 6, 6 ^ 7)


def test_extension_is_refused_at_the_bound():
    for case, reached in (("bound", False), ("below_bound", True)):
        N, header, recs, pairs, g, est = PM.load(case)
        assert est.max_upper == 2103 and g.h[2]["len"] == (2002 if reached else 2003)
        assert (((0, 2, 4), 100 + g.h[2]["len"]) in PM.sweep(g, pairs, est)["paths"][1]) == reached      # 100 + 2003 == the bound: strict


def test_check_flow_at_uses_equal_to_flow():
    N, header, recs, pairs, g, est = PM.load("flow")
    p = [x[0] for x in PM.sweep(g, pairs, est)["paths"][1]]
    lp, s = 2, 4
    assert (0, lp, lp) in p and not any(x.count(lp) > 2 for x in p)                  # with a list: uses < flow
    assert (0, s, s, s) in p and not any(x.count(s) > 3 for x in p)                  # without: uses <= flow


def test_distance_at_either_bound_is_rejected():
    rows = lambda case: PM.sweep(*[PM.load(case)[i] for i in (4, 3, 5)])["rows"]
    assert rows("at_lower") == rows("at_upper") == [(10, B, D, 3), (10, A, Cc, 3), (11, Cc, E, 3), (12, D, F, 3)]      # 100 + 100 + 51 == 251; 300 + 300 + 101 == 701
    assert rows("above_lower") == rows("below_upper") == [(10, B, D, 3), (10, A, Cc, 4), (11, Cc, E, 4), (12, D, F, 3)]


def test_who_is_eligible():
    fork = PM.sweep(*[PM.load("fork")[i] for i in (4, 3, 5)])["stats"]["eligible_entries"]
    # 61 and 62 are both claimed by node 10: neither direction votes
    assert PM.sweep(*[PM.load("same_claim")[i] for i in (4, 3, 5)])["stats"]["eligible_entries"] == fork == 6
    # 52 stands on E and on F: 42 -> 52 is out, and so is the table's share of it
    sw = PM.sweep(*[PM.load("two_pairs")[i] for i in (4, 3, 5)])
    assert sw["stats"]["eligible_entries"] == 5 and sw["rows"] == [(10, B, D, 3), (10, A, Cc, 2), (11, Cc, E, 2), (12, D, F, 3)]
    # a pair flagged 0 at the estimate is never eligible, a pair flagged 1 stays so after a merge puts both mates on one edge; a mate that no node claims votes
    N, header, recs, pairs = PM.fork_graph(long_c=True, extra=[(43, 1, 63, 0)])
    g = X.Graph(H.parse_graph(H.graph_text(header, recs))); est = PM.Estimate(g, pairs)
    before = PM.sweep(g, pairs, est)
    assert 63 not in before["claim"] and before["stats"]["eligible_entries"] == 7 and before["rows"] == [(10, B, D, 3), (12, D, F, 3)]      # |x| + |y| = 100 + 2400 is far above the upper bound
    wide = types.SimpleNamespace(ests={1: dict(est.ests[1], upper=3000)}, flags=est.flags, max_upper=est.max_upper)
    assert PM.sweep(g, pairs, wide)["rows"] == [(10, B, D, 3), (10, A, Cc, 1), (12, D, F, 3)]
    assert g.merge(A, Cc) is not None
    assert PM.sweep(g, pairs, est)["stats"]["eligible_entries"] == 7 and PM.sweep(g, pairs, PM.Estimate(g, pairs))["stats"]["eligible_entries"] == 6


def test_an_unclaimed_mate_votes_through_the_distance_of_a_failed_sign_test():
    N, header, recs, pairs, g, est = PM.load("unclaimed")
    assert (est.ests[1]["lower"], est.ests[1]["upper"], est.max_upper) == (0, 278585, 835755)
    sw = PM.sweep(g, pairs, est)
    assert 550 not in sw["claim"] and sw["claim"][43] == 1 and sw["claim"][100 + 416] == 10 and 100 + 417 not in sw["claim"]      # 417 * 2000 <= 835755 < 418 * 2000
    # 43 -> 550 with type1 0: the location of 43 on A's twin is negative, the sign test fails, the distance is 100 000 (:614) and lies inside (0, 278585)
    assert sw["rows"] == [(10, 0, 2, 1)] and (sw["stats"]["eligible_entries"], sw["stats"]["voting_entries"]) == (1, 1)
    pairs2 = {1: [p for p in pairs[1] if p[0] != 43] + [(43, 1, 550, 0)]}                # the strands that pass the sign test: 100 + 902 000 is far above the upper bound
    assert PM.sweep(g, pairs2, PM.Estimate(g, pairs2))["rows"] == []


def test_the_cap_on_a_ladder():
    N, header, recs, pairs, g, est = PM.load("ladder")
    sw = PM.sweep(g, pairs, est)
    assert sw["starts"][1] == [1, 2, 3, 4] and sw["stats"]["capped_nodes"] == 1
    per_start = [sum(1 for p in sw["paths"][1] if g.h[p[0][0]]["frm"] == s) for s in (1, 2, 3, 4)]
    # 2 + 4 + .. + 128 forwards, and the rungs behind a start node; start 4 would save 264: its walk stops descending once 1000 are passed (:362)
    assert per_start == [254, 256, 260, 236] and len(sw["paths"][1]) == 1006
    assert all(len(p) <= 1000 for i, p in sw["paths"].items() if i != 1)


def test_record_sizes_and_a_device_less_context():
    assert s2.PATH_SUPPORT_DTYPE.itemsize == 28 and C.sizeof(s2.PathStats) == 152
    rng = np.random.default_rng(5)
    reads = sorted({"".join(rng.choice(list("ACGT"), size=60)) for _ in range(20)})
    bases = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(); off = np.arange(0, (len(reads) + 1) * 60, 60, dtype=np.uint64)
    ctx = s2.Context(40, device=-2); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
    for call in (ctx.path_supports, ctx.path_supports_build, lambda: ctx.extend_paths_round(2), lambda: ctx.extend_by_paths(1000, 1)):
        with pytest.raises(s2.Sage2ovError) as e:
            call()
        assert e.value.code == -3
    st = ctx.path_stats(); assert (st.paths, st.records, st.rows) == (0, 0, 0)
    n = C.c_uint64(7)
    assert s2.lib().sage2ov_path_supports_count(None, C.c_uint32(1), C.byref(n)) == -1 and s2.lib().sage2ov_extend_paths_round(None, 2, 1, 0, None) == -1
    with pytest.raises(s2.Sage2ovError) as e:
        ctx.extend_paths_round(2, 1, 2)
    assert e.value.code == -1
    ctx.close()
