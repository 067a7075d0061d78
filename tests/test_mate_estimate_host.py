"""CPU: the round arithmetic of MatePair::meanSdEstimation (sage2ov_insert_estimate, matePair.cpp:265-308, :318-381) against a restatement in Python
integers -- and the helpers the reference and GPU tests of the read-to-edge table share: a parser and a writer of the graph file text, the restatement of
mapReadsToEdges / mapReadLocations / computeMeanSD as include/sage2ov.h states them, and mates built from a graph."""
import math
import numpy as np
import pytest
import sage2_amd as s2

M32 = (1 << 32) - 1


# ------------------------------------------------------------------------------------------ the graph file text (overlapGraph.cpp:12-20, :338-443)
def flip_type(t):
    return 3 if t == 0 else (0 if t == 3 else t)


def parse_graph(text, fold=True):
    """-> dict(header=(genome size, reads, average length), pairs=[(ordinal, record, twin)]); a record is dict(frm, to, type, reducible, len, flow, list) with
    list = [(read, orientation, flag, distPrevious, distNext)].  ordinal = number of the record pair in the file.  fold: a loop's record pair that directly
    follows its mirror image is the second writing of one edge (the writer visits both halves of a loop) and is left out, as sage2ov_graph_load_composite
    does; fold=False keeps every pair, as the reference's loader does."""
    if isinstance(text, bytes):
        text = text.decode()
    tok = text.split()
    header = (int(tok[0]), int(tok[1]), int(tok[2])); p = 3; recs = []
    while p < len(tok):
        n = int(tok[p + 6])
        lst = [tuple(int(x) for x in tok[p + 7 + 5 * j: p + 12 + 5 * j]) for j in range(n)]
        recs.append(dict(frm=int(tok[p]), to=int(tok[p + 1]), type=int(tok[p + 2]), reducible=int(tok[p + 3]), len=int(tok[p + 4]), flow=float(tok[p + 5]), list=lst))
        p += 7 + 5 * n
    assert len(recs) % 2 == 0
    pairs = []; took = False
    for q in range(len(recs) // 2):
        a, b = recs[2 * q], recs[2 * q + 1]
        if fold and pairs and not took and a["frm"] == a["to"] and pairs[-1][0] == q - 1 and a == pairs[-1][2] and b == pairs[-1][1]:
            took = True
            continue
        took = False
        pairs.append((q, a, b))
    return dict(header=header, pairs=pairs)


def twin_of(r):
    """the twin record of a record: ends swapped, type reversed (utils.cpp:212), the list in reverse order with the distances swapped"""
    return dict(frm=r["to"], to=r["frm"], type=flip_type(r["type"]), reducible=1, len=r["len"], flow=0.0,
                list=[(i, 1 - o, f, dn, dp) for (i, o, f, dp, dn) in reversed(r["list"])])


def rec(frm, to, typ, length, lst):
    return dict(frm=frm, to=to, type=typ, reducible=1, len=length, flow=0.0, list=[tuple(x) for x in lst])


def graph_text(header, records):
    """the text saveOverlapGraphInFile writes for these records (a flat list: record, twin, record, twin, ...)"""
    out = ["%d\n%d\n%d\n" % header]
    for r in records:
        out.append("%d\t%d\t%d\t%d\t%d\t%g\t%d\n" % (r["frm"], r["to"], r["type"], r["reducible"], r["len"], r["flow"], len(r["list"])))
        out += ["%d\t%d\t%d\t%d\t%d\n" % e for e in r["list"]]
        out.append("\n")
    return "".join(out)


# ------------------------------------------------------------------------------------------ the restatement (include/sage2ov.h; matePair.cpp as run with one thread)
def _locations(lst):
    out = {}; run = 0
    for (i, o, f, dp, dn) in lst:
        run = (run + dp) & M32
        v = run if o else (-run) & M32
        out.setdefault(i, []).append(v - (1 << 32) if v >= (1 << 31) else v)
    return out


def read_edge_table(graph):
    """{(read, ordinal): dict(frm, to, type of E, forward, reverse)}"""
    table = {}
    for q, a, b in graph["pairs"]:
        E, T = (a, b) if a["frm"] < a["to"] else (b, a)          # the half leaving the smaller id; a loop: the second record (first in the node's newest-first list)
        fw, rv = _locations(E["list"]), _locations(T["list"])
        for r in set(fw) | set(rv):
            table[(r, q)] = dict(frm=E["frm"], to=E["to"], type=E["type"], forward=fw.get(r, []), reverse=rv.get(r, []))
    return table


def by_read(table):
    d = {}
    for (r, q) in sorted(table):
        d.setdefault(r, []).append(q)
    return d


def mate_flags(table, mates):
    """mates: iterable of (from, to); 0 when both reads have an entry for one pair"""
    pr = by_read(table)
    return [0 if set(pr.get(a, [])) & set(pr.get(b, [])) else 1 for a, b in mates]


def mate_distances(table, mates):
    """one d per mate entry with from < to and common pair where both reads have exactly one forward location; entry order, then ascending pair"""
    pr = by_read(table); out = []
    for a, b in mates:
        if a < b:
            for q in sorted(set(pr.get(a, [])) & set(pr.get(b, []))):
                fa, fb = table[(a, q)]["forward"], table[(b, q)]["forward"]
                if len(fa) == 1 and len(fb) == 1:
                    out.append(abs(abs(fa[0]) - abs(fb[0])))
    return out


def estimate(d, arl):
    """the rounds: dict(valid, rounds, final, considered, mu, sd, mean, deviation, lower, upper) in Python integers"""
    mu = sd = 5000; o = dict(valid=0, rounds=0, final=0, considered=[], mu=[], sd=[], mean=0, deviation=0, lower=0, upper=0)
    rmu = rsd = 0
    for i in range(10):
        sel = [int(x) for x in d if x < 4 * mu]
        o["considered"].append(len(sel))
        if len(sel) < 2:
            return o
        rmu = sum(sel) // len(sel)
        rsd = math.isqrt(sum((mu - x) ** 2 for x in sel) // (len(sel) - 1))      # floor(sqrt(sq / (count - 1))) = isqrt(floor(sq / (count - 1)))
        fin = abs(mu - rmu) <= rmu // 100 and abs(sd - rsd) <= rsd // 100
        mu, sd = rmu, rsd
        o["mu"].append(rmu); o["sd"].append(rsd); o["rounds"] = i + 1
        if fin:
            o["final"] = 1
            break
    o.update(valid=1, mean=rmu + arl, deviation=rsd)
    o.update(lower=max(0, o["mean"] - 3 * rsd), upper=o["mean"] + 3 * rsd)
    return o


def bounds(estimates, arl):
    """minimumUpperBoundOfInsert, maximumUpperBoundOfInsert over the valid libraries (matePair.cpp:292-308)"""
    lo, hi = 1000000, 0
    for e in estimates:
        if e["valid"]:
            lo = e["upper"] if lo >= e["upper"] else lo
            hi = e["upper"] if hi <= e["upper"] else hi
    return lo, hi * 3 * ((arl + 99) // 100)


def same_estimate(got: s2.Insert, want):
    n = want["rounds"]
    assert (got.valid, got.rounds, got.final_round) == (want["valid"], n, want["final"])
    assert list(got.considered)[:len(want["considered"])] == want["considered"]
    assert list(got.mu)[:n] == want["mu"] and list(got.sd)[:n] == want["sd"]
    assert (got.mean, got.deviation, got.lower, got.upper) == (want["mean"], want["deviation"], want["lower"], want["upper"])


def valid_every_round(d):
    """every round of the estimation considers at least two distances (the reference divides by zero otherwise)"""
    e = estimate(d, 0)
    return e["valid"] == 1 and all(c >= 2 for c in e["considered"])


# ------------------------------------------------------------------------------------------ mates from a graph
def pairs_from_graph(graph, seed, n_reads, libraries=2):
    """{library: [(read a, strand a, read b, strand b)]} chosen from the graph's own lists: both reads on one edge a chosen number of list entries apart
    (library L: 3 L .. 12 L entries, so the libraries have different insert sizes and every one has distances far below the first round's threshold),
    reads far apart on one edge, reads on different edges, self pairs, reverse-complemented mates (strand 0), a mate that is an end node (on no list),
    a pair given twice, a pair of arbitrary reads."""
    rng = np.random.default_rng(seed)
    lists = [[e[0] for e in a["list"]] for _, a, b in graph["pairs"] if a["list"]]
    ends = sorted({a["frm"] for _, a, b in graph["pairs"]} | {a["to"] for _, a, b in graph["pairs"]})
    out = {L: [] for L in range(1, libraries + 1)}
    for L in out:
        for lst in sorted(lists, key=len, reverse=True)[:40]:
            for _ in range(min(12, len(lst))):
                i = int(rng.integers(0, len(lst))); j = min(len(lst) - 1, i + int(rng.integers(3 * L, 12 * L + 1)))
                if rng.integers(0, 2):
                    i, j = j, i
                out[L].append((lst[i], int(rng.integers(0, 2)), lst[j], int(rng.integers(0, 2))))          # same edge (i == j: a self pair)
            out[L].append((lst[0], 1, lst[-1], 0)); out[L].append((lst[0], 0, lst[0], 1))                    # the whole edge apart; a self pair
        for _ in range(8):
            if len(lists) > 1:
                x, y = (int(v) for v in rng.choice(len(lists), size=2, replace=False))
                out[L].append((lists[x][0], 1, lists[y][-1], 0))                                            # different edges
        if lists and ends:
            out[L].append((ends[0], 1, lists[0][0], 1)); out[L].append((lists[-1][-1], 0, ends[-1], 1))      # an end node is on no list
        if out[L]:
            out[L].append(out[L][0])                                                                         # the same pair again: count 2, one distance
        out[L].append((int(rng.integers(1, n_reads + 1)), 1, int(rng.integers(1, n_reads + 1)), 1))
    return out


def mate_entries(pairs):
    """the (from, to) of the mate table these pairs make, in its order: ascending (from, to, type1, type2), both directions, distinct"""
    return [(a, b) for (a, b, ta, tb) in sorted({(a, b, sa, sb) for a, sa, b, sb in pairs} | {(b, a, sb, sa) for a, sa, b, sb in pairs})]


def mates_ascii(pairs, seqs):
    """the mates as the reads a sequencer would give: (bases, offsets) for sage2ov_mates_add_ascii; seqs[id] = the stored (canonical) read"""
    comp = str.maketrans("ACGT", "TGCA"); reads = []
    for a, sa, b, sb in pairs:
        reads.append(seqs[a] if sa else seqs[a].translate(comp)[::-1]); reads.append(seqs[b] if sb else seqs[b].translate(comp)[::-1])
    off = np.zeros(len(reads) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(), off


def stored_reads(ctx):
    """{id: ASCII of the stored read} of a context with organised reads"""
    packed, length, _ = ctx.reads_export()
    bits = np.unpackbits(packed, axis=1); codes = bits[:, 0::2] * 2 + bits[:, 1::2]
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    return {i: lut[codes[i, :length[i]]].tobytes().decode() for i in range(1, len(length))}


def hand_graph():
    """(N, header, records): composite edges the pipeline does not produce after step 4 -- read 20 on three pairs; read 30 twice on one edge (two locations:
    its pairs are not considered); orientation-0 entries; a loop written once, a loop written twice (record pair + mirror image); a simple edge"""
    N = 60
    e1 = rec(1, 2, 3, 400, [(20, 1, 0, 50, 60), (21, 0, 0, 60, 70), (22, 1, 0, 70, 40), (23, 1, 0, 40, 90), (24, 0, 0, 90, 30)])
    e2 = rec(2, 3, 3, 500, [(20, 0, 0, 30, 100), (30, 1, 0, 100, 20), (31, 1, 0, 20, 200), (30, 0, 0, 200, 15), (32, 1, 0, 15, 80), (33, 1, 0, 80, 11)])
    e3 = rec(5, 4, 0, 300, [(20, 1, 0, 10, 2047), (40, 1, 0, 2047, 5), (41, 0, 0, 5, 9)])                # first record leaves the LARGER id: E is its twin
    lp1 = rec(6, 6, 1, 120, [(42, 1, 0, 33, 44), (43, 0, 0, 44, 7)])                                     # a loop, written once
    lp2 = rec(7, 7, 2, 90, [(44, 1, 0, 12, 13), (45, 1, 0, 13, 14), (46, 1, 0, 14, 15)])                 # a loop as the writer leaves it: pair, then mirror image
    simple = rec(8, 9, 3, 40, [])
    recs = [e1, twin_of(e1), e2, twin_of(e2), e3, twin_of(e3), lp1, twin_of(lp1), lp2, twin_of(lp2), twin_of(lp2), lp2, simple, twin_of(simple)]
    return N, (0, 120, 100), recs


# ------------------------------------------------------------------------------------------ sage2ov_insert_estimate
def _check(d, arl=100):
    d = np.asarray(d, dtype=np.uint32)
    same_estimate(s2.insert_estimate(d, arl), estimate(d.tolist(), arl))
    return estimate(d.tolist(), arl)


def test_final_round_before_the_tenth():
    rng = np.random.default_rng(1)
    e = _check(rng.normal(3000, 150, size=4000).clip(1, None).astype(np.uint32))
    assert e["final"] == 1 and 2 <= e["rounds"] < 10


def test_ten_rounds_without_a_final_one():
    # 2^j copies of 3000 * 2^j: the mean stays above half the largest value taken, so every round's threshold takes in one level more and the mean
    # nearly doubles: the 1 % rule is never met
    d = [3000 << j for j in range(13) for _ in range(1 << j)]
    e = _check(d)
    assert e["valid"] == 1 and e["rounds"] == 10 and e["final"] == 0


def test_threshold_is_strict():
    # mu = 5000 in round 1: d == 20000 is left out, 19999 is taken
    e = _check([19999, 19999, 20000, 20000, 20000])
    assert e["considered"][0] == 2
    e = _check([20000, 20000, 20000])
    assert e["valid"] == 0 and e["considered"] == [0]


@pytest.mark.parametrize("d", [[], [7], [30000, 8], [100, 30000000, 30000000]])
def test_fewer_than_two_considered_is_not_valid(d):
    e = _check(d)
    assert e["valid"] == 0 and e["mean"] == e["upper"] == 0
    got = s2.insert_estimate(np.asarray(d, dtype=np.uint32), 100)
    assert (got.mean, got.deviation, got.lower, got.upper) == (0, 0, 0, 0)


def test_a_later_round_that_runs_dry():
    # round 1 takes 5 and 6 (mu becomes 5); round 2's threshold 20 still holds them; with 5, 15000: round 1 mu = 7502, round 2 keeps both ... a dry round needs the
    # mean to fall below a quarter of all but one value: 0, 0, 0, 19000 -> mu 4750 -> all kept; instead 0 x 9 and 19999: mu 1999, round 2 drops 19999, mu 0, round 3: none
    e = _check([0] * 9 + [19999])
    assert e["valid"] == 0 and e["rounds"] == 2 and e["considered"] == [10, 9, 0]


def test_squared_error_above_two_to_the_64():
    # every level lies just below the threshold its predecessors' mean allows and has twice as many copies as all levels before it: the mean grows about
    # 2.7-fold per round, and the last rounds sum some 10^4 squares of some 10^7..10^8 each
    d, mu = [], 5000
    for _ in range(10):
        d += [4 * mu - 1] * max(2, 2 * len(d)); mu = sum(d) // len(d)
    assert max(d) < 1 << 32
    e = estimate(d, 100)
    mus = [5000] + e["mu"]
    assert any(sum((m - x) ** 2 for x in d if x < 4 * m) > 1 << 64 for m in mus[:e["rounds"]])
    _check(d)


def test_bound_formulas():
    e = _check([100, 100, 100, 19000, 19000], arl=7)                    # SD far above the mean: the lower bound stops at 0
    assert e["valid"] and e["mean"] < 3 * e["deviation"] and e["lower"] == 0 and e["upper"] == e["mean"] + 3 * e["deviation"]
    e = _check([1000, 1001, 1002, 1003] * 50, arl=151)
    assert e["lower"] == e["mean"] - 3 * e["deviation"] > 0 and e["mean"] == e["mu"][-1] + 151
    assert bounds([e, estimate([], 151)], 151) == (e["upper"], e["upper"] * 3 * 2)


def test_restatement_on_the_hand_built_graph():
    """the helpers themselves: E of a record that leaves the larger id, wrapped and negated locations, the folded loop"""
    N, header, recs = hand_graph()
    g = parse_graph(graph_text(header, recs)); gr = parse_graph(graph_text(header, recs), fold=False)
    assert [q for q, _, _ in g["pairs"]] == [0, 1, 2, 3, 4, 6] and len(gr["pairs"]) == 7
    t = read_edge_table(g)
    assert sorted(q for (r, q) in t if r == 20) == [0, 1, 2]
    assert t[(20, 2)]["frm"] == 4 and t[(20, 2)]["forward"] == [-(5 + 9 + 2047)] and t[(20, 2)]["reverse"] == [10]      # E = the twin (4 -> 5); its list is reversed and flipped
    assert t[(30, 1)]["forward"] == [130, -350] and t[(21, 0)]["forward"] == [-110]
    assert t[(42, 3)]["frm"] == 6 and t[(42, 3)]["forward"] == [-(7 + 44)] and t[(42, 3)]["reverse"] == [33]            # a loop: E = the second record
    assert mate_flags(t, [(20, 24), (20, 40), (24, 40), (1, 20), (30, 30), (50, 50)]) == [0, 0, 1, 1, 0, 1]
    assert mate_distances(t, [(20, 24), (24, 20), (20, 30), (31, 32), (21, 21)]) == [abs(50 - 310), abs(150 - 365)]
