"""The restatement of the second and third loop of ContigExtender::extendContigs (matePair/mergeContigs.cpp:62-99) as include/sage2ov.h states them under PATH
SUPPORTS: the estimate flags, the claim of reads by nodes, the start nodes, the capped depth-first walk, the pair votes, the table, both selections, a round, the
loops and the four counters of the deliberate differences -- in Python, over extend_model.Graph.  Shared by the CPU, reference and GPU tests; not a test module."""
import sys
import extend_model as X
import test_mate_estimate_host as H

LEVELS, CAP, NO_SIGN = 7, 1000, 100000


def match(t1, t2):
    """matchEdgeType (:392-397)"""
    return (t1 in (1, 3) and t2 in (2, 3)) or (t1 in (0, 2) and t2 in (0, 1))


def entries_of(pairs, L):
    """the mate entries of library L in the table's order: (m1, m2, type1, type2)"""
    pl = pairs.get(L, [])
    return sorted({(a, b, sa, sb) for a, sa, b, sb in pl} | {(b, a, sb, sa) for a, sa, b, sb in pl})


class Estimate(X.Bounds):
    """the insert estimates of one meanSdEstimation and, with them, every library's mate flags on the graph they were made on (ESTIMATE FLAGS)"""

    def __init__(self, g, pairs):
        super().__init__(g, pairs)
        pr = H.by_read(H.read_edge_table(g.parsed()))
        self.flags = {L: [0 if set(pr.get(a, [])) & set(pr.get(b, [])) else 1 for (a, b, _, _) in entries_of(pairs, L)] for L in self.ests}


def sweep(g, pairs, est):
    """one sweep on g -> dict(claim={read: node}, starts={node: [start nodes]}, paths={node: [(halves, length)]}, votes={(a, b): support}, rows=[(node, a, b, support)]
    in table order, entries=[dict(library, m1, m2, type1, type2, node, survivors=[(a, b)], mirrored)] of the eligible mate entries, stats=dict(claimed_reads, claiming_nodes, start_nodes, paths, capped_nodes, eligible_entries, voting_entries, records, rows, key_collisions, mirrored))"""
    h = g.h; bound = est.max_upper
    alive = [x for x in range(len(h)) if g.alive[x >> 1]]
    # CLAIM (:190-216)
    claim = {}
    for x in alive:
        run = 0; node = min(h[x]["frm"], h[x]["to"])
        for (r, o, f, dp, dn) in h[x]["list"]:
            run += dp
            if run > bound:
                break
            claim[r] = min(claim.get(r, node), node)
    table = H.read_edge_table(g.parsed()); pr = H.by_read(table)
    nodes = {h[x]["frm"] for x in alive}
    uniq = lambda r: pr[r][0] if len(pr.get(r, [])) == 1 and r not in nodes else None
    # START NODES (:220-239)
    starts = {}
    for r, i in claim.items():
        for q in pr.get(r, []):
            starts.setdefault(i, set()).update((h[2 * q]["frm"], h[2 * q]["to"]))
    starts = {i: sorted(s) for i, s in starts.items()}
    leaving = {}
    for x in reversed(alive):                                                         # newest first
        leaving.setdefault(h[x]["frm"], []).append(x)
    # PATHS (:359-429)
    sys.setrecursionlimit(10000)
    paths = {}; capped = 0
    for i in sorted(starts):
        saved = []; path = [None] * (LEVELS + 2); plen = [0] * (LEVELS + 2)

        def explore(node, level):
            if level > LEVELS or len(saved) > CAP:
                return
            for v in leaving.get(node, []):
                if level == 1:
                    if h[v]["list"] and h[v]["flow"] > 0:
                        path[1] = v; plen[1] = 0
                        saved.append((tuple(path[1:2]), 0)); explore(h[v]["to"], 2)
                else:
                    pv = path[level - 1]
                    uses = sum(1 for k in range(1, level) if path[k] in (v, v ^ 1))
                    flow_ok = uses <= h[v]["flow"] if not h[v]["list"] else uses < h[v]["flow"]
                    if match(h[pv]["type"], h[v]["type"]) and flow_ok and plen[level - 1] + h[pv]["len"] < bound:
                        path[level] = v; plen[level] = plen[level - 1] + h[pv]["len"]
                        saved.append((tuple(path[1:level + 1]), plen[level])); explore(h[v]["to"], level + 1)
        for s in starts[i]:
            explore(s, 1)
        paths[i] = saved; capped += len(saved) > CAP
    # PAIR VOTES (:254-300, :539-743)
    E_of = lambda q: 2 * q if h[2 * q]["frm"] < h[2 * q]["to"] else 2 * q + 1
    votes = {}; eligible = voting = mirrored = 0; entries = []
    for L in sorted(est.ests):
        e = est.ests[L]
        if not e["valid"]:
            continue
        for (m1, m2, t1, t2), flag in zip(entries_of(pairs, L), est.flags[L]):
            i = claim.get(m1); q1, q2 = uniq(m1), uniq(m2)
            if flag != 1 or i is None or not (claim.get(m2) is None or claim[m2] > i) or q1 is None or q2 is None:
                continue
            eligible += 1
            s1, s2 = (1 if t1 else -1), (1 if t2 else -1)
            firstp = None; surv = []; mirr = []
            for x in range(4):
                edge1, edge2 = E_of(q1) ^ (x >> 1), E_of(q2) ^ (x & 1)
                d1 = table[(m1, q1)]["forward" if x >> 1 else "reverse"]; d2 = table[(m2, q2)]["forward" if not x & 1 else "reverse"]
                if not d1 or not d2:
                    continue
                for (hv, ln) in paths.get(i, []):
                    if h[hv[0]]["frm"] != h[edge1]["to"] or not match(h[edge1]["type"], h[hv[0]]["type"]) or hv[-1] != edge2:
                        continue
                    dist = lambda a, b: abs(a) + abs(b) + ln if s1 * a < 0 and s2 * b < 0 else NO_SIGN
                    if not any(e["lower"] < dist(a, b) < e["upper"] for a in d1 for b in d2):
                        continue
                    seq = (edge1,) + hv
                    if firstp is None:
                        firstp = seq; surv = [True] * len(hv); mirr = [False] * len(hv)
                        continue
                    for k in range(len(firstp) - 1):
                        if not surv[k]:
                            continue
                        a, b = firstp[k], firstp[k + 1]
                        direct = any(seq[l] == a and seq[l + 1] == b for l in range(len(seq) - 1))
                        mirror = any(seq[l + 1] ^ 1 == a and seq[l] ^ 1 == b for l in range(len(seq) - 1))
                        if not direct and not mirror:
                            surv[k] = False
                        if not direct and mirror:
                            mirr[k] = True
            got = [(firstp[k], firstp[k + 1]) for k in range(len(firstp) - 1) if surv[k]] if firstp is not None else []
            entries.append(dict(library=L, m1=m1, m2=m2, type1=t1, type2=t2, node=i, survivors=got, mirrored=sum(m for k, m in enumerate(mirr) if surv[k])))
            if not got:
                continue
            voting += 1
            for k in range(len(firstp) - 1):
                if surv[k]:
                    votes[(firstp[k], firstp[k + 1])] = votes.get((firstp[k], firstp[k + 1]), 0) + 1; mirrored += mirr[k]
    rows = sorted(((h[a]["to"], a, b, s) for (a, b), s in votes.items()), key=lambda r: (r[0], -r[1], -r[2]))
    xk = lambda x: h[x]["frm"] ^ h[x]["to"]
    stats = dict(claimed_reads=len(claim), claiming_nodes=len(set(claim.values())), start_nodes=sum(len(s) for s in starts.values()), paths=sum(len(p) for p in paths.values()),
                 capped_nodes=capped, eligible_entries=eligible, voting_entries=voting, records=sum(votes.values()), rows=len(rows),
                 key_collisions=len(rows) - len({(xk(a), xk(b)) for (_, a, b, _) in rows}), mirrored=mirrored)
    return dict(claim=claim, starts=starts, paths=paths, votes=votes, rows=rows, stats=stats, entries=entries)


def export_rows(g, rows):
    """the table as sage2ov_path_supports_export gives it: (node, pair_a, pair_b, from_a, to_b, support, second_a, second_b)"""
    o = g.ordinals(); first = {x >> 1: x for x in reversed(g.first_halves())}
    return [(n, o[a >> 1], o[b >> 1], g.h[a]["frm"], g.h[b]["to"], s, int(first[a >> 1] != a), int(first[b >> 1] != b)) for (n, a, b, s) in rows]


def round_(g, pairs, est, high, low=1, variant=0):
    """one findPathSupports(high) (variant 0) or findPathSupportsNew(high) (1) on g (changed in place).  -> dict(merges=[...] as extend_model.round_, entries,
    at_threshold, refused, blocked, order_dependent, stats: the sweep's)"""
    sw = sweep(g, pairs, est); h = g.h
    before = g.ordinals()
    xk = lambda x: h[x]["frm"] ^ h[x]["to"]
    key = lambda x, y: (xk(x), xk(y))
    ents = [dict(e1=a, e2=b, sup=s, node=n, key=key(a, b)) for (n, a, b, s) in sw["rows"]]
    search = {}; filed = {}
    for n, e in enumerate(ents):
        search[e["key"]] = search.get(e["key"], 0) + e["sup"]
        for nd in (h[e["e1"]]["to"], h[e["e1"]]["frm"], h[e["e2"]]["to"], h[e["e2"]]["frm"]):
            filed.setdefault(nd, []).append(n)
    order = sorted(range(len(ents)), key=lambda n: -ents[n]["sup"])                 # (stable: ties in table order)
    top = [ents[n] for n in order if ents[n]["sup"] >= high]
    at = [e["node"] for e in top]
    dependent = len(set(at)) != len(at) or any(nd != e["node"] and nd in at for e in top for nd in (h[e["e1"]]["frm"], h[e["e2"]]["to"]))
    out = dict(merges=[], entries=len(ents), at_threshold=len(top), refused=0, blocked=0, order_dependent=int(dependent), stats=sw["stats"])
    blocked = set(); new_halves = []
    alive = lambda x: g.alive[x >> 1]
    leaving = lambda node: [x for x in range(len(h) - 1, -1, -1) if alive(x) and h[x]["frm"] == node]
    for n in order:
        e = ents[n]; e1, e2 = e["e1"], e["e2"]
        if not alive(e1) or not alive(e2) or e["key"] not in search:
            continue
        node = h[e1]["to"]
        if node in blocked:
            out["blocked"] += 1
            continue
        if e["sup"] < high:
            continue
        unique_in = unique_out = True
        for v in leaving(node):
            if not (h[v]["flow"] >= 1 and h[v]["frm"] != h[v]["to"]):
                continue
            if (v ^ 1) != e1 and match(h[v ^ 1]["type"], h[e2]["type"]):
                if search.get(key(v ^ 1, e2), search.get(key(e2 ^ 1, v), 0)) > low:
                    unique_in = False
            if v != e2 and match(h[e1]["type"], h[v]["type"]):
                if search.get(key(e1, v), search.get(key(v ^ 1, e1 ^ 1), 0)) > low:
                    unique_out = False
        if not ((unique_in and unique_out) if variant == 0 else (unique_in or unique_out)):
            out["refused"] += 1
            continue
        blocked |= {h[v]["to"] for v in leaving(node) if h[v]["to"] != h[v]["frm"]}
        m = dict(node=node, frm=h[e1]["frm"], to=h[e2]["to"], support=e["sup"], pair_in=before.get(e1 >> 1, X.NONE), pair_out=before.get(e2 >> 1, X.NONE))
        nh = g.merge(e1, e2, 1)
        if nh is None:
            continue
        m.update(flow=g.last["flow"], type=g.last["type"], in_deleted=int(g.last["deleted"][0]), out_deleted=int(g.last["deleted"][1]))
        for x in filed.get(node, []):
            search.pop(ents[x]["key"], None)
        out["merges"].append(m); new_halves.append(nh)
    after = g.ordinals()
    for m, nh in zip(out["merges"], new_halves):
        m["pair_new"] = after.get(nh >> 1, X.NONE)
    return out


def extend(g, pairs, est, genome_size, reads, variant, low=1, max_rounds=10000):
    """one of the loops of :62-99 -> the rounds' results, the last one with no more merges than the stop value"""
    stop = 10 if genome_size > 1000000000 else 0; rounds = []
    for it in range(1, max_rounds + 1):
        r = round_(g, pairs, est, X.threshold(reads, g.header[2], genome_size, it), low, variant)
        rounds.append(r)
        if len(r["merges"]) <= stop:
            return rounds
    raise RuntimeError("no fixed point")


# ------------------------------------------------------------------------------------------ the hand-built graph: a fork behind short edges
def fork_graph(third=False, **kw):
    """(N, header, records, pairs).  Node 10 has the in-edges A (1 -> 10), B (2 -> 10) and the short out-edges C (10 -> 11), D (10 -> 12) that lead on to E (11 -> 21)
    and F (12 -> 22); every edge is of type 3.  Mates run A <-> E and B <-> F, three pairs each: C and D carry one read each, too few for the first loop.  Z (30 -> 31)
    carries the pairs the insert size is estimated from.  third: a third in-edge G (3 -> 10) whose mates reach E and F, twice each.
    kw: lenC (60), long_c, dup, flows {name: flow}, extra pairs for library 1"""
    rec = H.rec; lenC = kw.get("lenC", 60)
    step = lambda first, o, n=3: [(first + j, o, 0, 100, 100) for j in range(n)]
    e = dict(A=rec(1, 10, 3, 400, step(41, 1)), B=rec(2, 10, 3, 400, step(44, 1)), C=rec(10, 11, 3, lenC, [(61, 1, 0, lenC // 2, lenC - lenC // 2)]),
             D=rec(10, 12, 3, 60, [(62, 1, 0, 30, 30)]), E=rec(11, 21, 3, 400, step(51, 0)), F=rec(12, 22, 3, 400, step(54, 0)),
             Z=rec(30, 31, 3, 1000, [(71 + j, 1, 0, 100, 100) for j in range(9)]))
    if third:
        e["G"] = rec(3, 10, 3, 400, step(47, 1))
    if kw.get("long_c"):                                                              # read 63 lies beyond the bound from either end of C
        e["C"] = rec(10, 11, 3, 5000, [(61, 1, 0, 1000, 1400), (63, 1, 0, 1400, 1300), (64, 1, 0, 1300, 1300)])
    if kw.get("dup"):                                                                 # read 52 stands on F too: unique on no pair
        e["F"]["list"] = e["F"]["list"] + [(52, 0, 0, 10, 10)]
    p1 = [(42, 1, 52, 1), (43, 1, 53, 1), (41, 1, 51, 1), (45, 1, 55, 1), (46, 1, 56, 1), (44, 1, 54, 1),
          (71, 1, 75, 0), (72, 1, 76, 0), (71, 1, 74, 0), (73, 1, 78, 0), (72, 1, 77, 0), (74, 1, 78, 0)]
    if third:
        p1 += [(48, 1, 52, 1), (49, 1, 53, 1), (48, 1, 55, 1), (49, 1, 56, 1)]
    p1 += list(kw.get("extra", []))
    recs = []
    for name, r in e.items():
        t = H.twin_of(r); r["flow"] = t["flow"] = float(kw.get("flows", {}).get(name, 1)); recs += [r, t]
    return 90, (0, 180, 60), recs, {1: p1}


Z_PAIRS = [(71, 1, 75, 0), (72, 1, 76, 0), (71, 1, 74, 0), (73, 1, 78, 0), (72, 1, 77, 0), (74, 1, 78, 0)]      # distances 400, 400, 300, 500, 500, 400: bounds 251 / 701 / 2103


def _with_z(edges, pairs, flows=None):
    """the records of `edges` (name -> record) and of Z, flows 1 unless named"""
    edges = dict(edges, Z=H.rec(30, 31, 3, 1000, [(71 + j, 1, 0, 100, 100) for j in range(9)])); recs = []
    for name, r in edges.items():
        t = H.twin_of(r); r["flow"] = t["flow"] = float((flows or {}).get(name, 1)); recs += [r, t]
    return 90, (0, 180, 60), recs, {1: list(pairs) + Z_PAIRS}


def chain_graph(nodes=tuple(range(1, 11))):
    """K1 .. K9 along `nodes` (by default node j -> j + 1), 50 bases and one read (40 + j) each.  Read 41's mate 48 is reached by the 7-edge path K2 .. K8 (300 + 25 +
    25 bases), its mate 49 only by one of 8 edges"""
    e = {"K%d" % j: H.rec(nodes[j - 1], nodes[j], 3, 50, [(40 + j, 1, 0, 25, 25)]) for j in range(1, 10)}
    return _with_z(e, [(41, 1, 48, 0), (41, 1, 49, 0)])


def bound_graph(mid=2003):
    """P1 (1 -> 2, 100 bases), P2 (2 -> 3, `mid`), P3 (3 -> 4): from node 1 the walk reaches P3 only when 100 + mid < 2103"""
    e = dict(P1=H.rec(1, 2, 3, 100, [(41, 1, 0, 50, 50)]), P2=H.rec(2, 3, 3, mid, [(42, 1, 0, 1000, mid - 1000)]), P3=H.rec(3, 4, 3, 100, [(43, 1, 0, 50, 50)]))
    return _with_z(e, [])


def flow_graph():
    """A (1 -> 10) in front of two loops at node 10: Lp with a list and S without, flow 2 each.  checkFlow lets Lp stand twice in a path (uses < flow) and S three
    times (uses <= flow)"""
    e = dict(A=H.rec(1, 10, 3, 100, [(41, 1, 0, 50, 50)]), Lp=H.rec(10, 10, 3, 40, [(42, 1, 0, 20, 20)]), S=H.rec(10, 10, 3, 30, []))
    return _with_z(e, [], flows=dict(Lp=2, S=2))


def bubble_graph():
    """A (1 -> 10), X (10 -> 11), a bubble C1 / C2 (11 -> 12, 50 and 51 bases), E (12 -> 13).  The mates of A's reads on E have the two qualifying paths X C1 E and
    X C2 E: of the first path's pairs only (A, X) stands in both"""
    step = lambda first, o: [(first + j, o, 0, 100, 100) for j in range(3)]
    e = dict(A=H.rec(1, 10, 3, 400, step(41, 1)), X=H.rec(10, 11, 3, 60, [(61, 1, 0, 30, 30)]), C1=H.rec(11, 12, 3, 50, [(62, 1, 0, 25, 25)]),
             C2=H.rec(11, 12, 3, 51, [(63, 1, 0, 25, 26)]), E=H.rec(12, 13, 3, 400, step(51, 0)))
    return _with_z(e, [(42, 1, 52, 1), (43, 1, 53, 1), (41, 1, 51, 1)])


def unclaimed_graph():
    """A mate that no node claims, and votes.  W (10 -> 11) has 900 reads 2 000 bases apart; read 550 in its middle lies beyond maximumUpperBoundOfInsert from either
    end.  No distance through it is below an upper bound -- the bound is three times the largest -- so its entry can only pass through the distance of 100 000 that the
    reference gives a pair of locations that fails the sign test (:614): the library's pairs on Z (15 000, 50 000 and 150 000 bases apart) bring its upper bound to
    278 585, and 43 -> 550 is given the strand that fails.  It votes for (A, W)"""
    e = dict(A=H.rec(1, 10, 3, 400, [(41 + j, 1, 0, 100, 100) for j in range(3)]), W=H.rec(10, 11, 3, 901 * 2000, [(100 + j, 1, 0, 2000, 2000) for j in range(900)]),
             Z=H.rec(30, 31, 3, 161 * 1000, [(1000 + j, 1, 0, 1000, 1000) for j in range(160)]))
    pairs = [(1000 + i, 1, 1000 + i + gap, 0) for gap, n in ((15, 2), (50, 4), (150, 10)) for i in range(n)] + [(43, 0, 550, 1)]
    recs = []
    for r in e.values():
        t = H.twin_of(r); r["flow"] = t["flow"] = 1.0; recs += [r, t]
    return 1200, (0, 2400, 60), recs, {1: pairs}


def ladder_graph():
    """nodes 1 .. 11, every node joined to the next by two edges of type 3 (50 and 51 bases, one read each): 2 + 4 + .. + 128 = 254 paths from a start node with seven
    rungs ahead.  Read 41 stands on a rung 1 -> 2 and on a rung 3 -> 4: node 1 claims it and has the four start nodes 1 .. 4, 1016 paths without the cap"""
    e = {}
    for j in range(1, 11):
        e["U%d" % j] = H.rec(j, j + 1, 3, 50, [(40 + 2 * j, 1, 0, 25, 25)]); e["V%d" % j] = H.rec(j, j + 1, 3, 51, [(41 + 2 * j, 1, 0, 25, 26)])
    e["U1"]["list"] = [(41, 1, 0, 10, 15)] + e["U1"]["list"]; e["U3"]["list"] = [(41, 1, 0, 10, 15)] + e["U3"]["list"]
    return _with_z(e, [(42, 1, 44, 0)])


CASES = dict(fork=lambda: fork_graph(), third=lambda: fork_graph(True), at_lower=lambda: fork_graph(lenC=51, extra=[(43, 1, 51, 1)]), above_lower=lambda: fork_graph(lenC=52, extra=[(43, 1, 51, 1)]),
             at_upper=lambda: fork_graph(lenC=101, extra=[(41, 1, 53, 1)]), below_upper=lambda: fork_graph(lenC=100, extra=[(41, 1, 53, 1)]),
             same_claim=lambda: fork_graph(extra=[(61, 1, 62, 1)]), two_pairs=lambda: fork_graph(dup=True), chain=chain_graph, bound=bound_graph,
             below_bound=lambda: bound_graph(2002), flow=flow_graph, ladder=ladder_graph, bubble=bubble_graph, unclaimed=unclaimed_graph)


def load(case):
    """-> (N, header, records, pairs, the model's graph, its estimate)"""
    N, header, recs, pairs = CASES[case]()
    g = X.Graph(H.parse_graph(H.graph_text(header, recs)))
    return N, header, recs, pairs, g, Estimate(g, pairs)


def fork_mates(g, sw, seed, n=200):
    """mate pairs placed across forks of g: for seeded saved paths of two to seven edges of the sweep sw, a read on an edge that enters the path's start node and
    matches its first edge, and a read on the path's last edge, both on one pair only, strands by the sign of their locations (so that the sign test passes; the
    distance falls where it may).  Pairs of different edges do not move an insert estimate"""
    import numpy as np
    rng = np.random.default_rng(seed); h = g.h
    table = H.read_edge_table(g.parsed()); pr = H.by_read(table)
    nodes = {h[x]["frm"] for x in range(len(h)) if g.alive[x >> 1]}
    uniq = lambda r: len(pr.get(r, [])) == 1 and r not in nodes
    E_of = lambda q: 2 * q if h[2 * q]["frm"] < h[2 * q]["to"] else 2 * q + 1
    entering = {}
    for x in range(len(h)):
        if g.alive[x >> 1] and h[x]["list"]:
            entering.setdefault(h[x]["to"], []).append(x)
    long_paths = [(i, p) for i in sorted(sw["paths"]) for (p, _) in sw["paths"][i] if len(p) >= 2 and h[p[-1]]["list"]]
    out = []
    for k in rng.permutation(len(long_paths))[:4 * n]:
        i, p = long_paths[int(k)]
        ins = [a for a in entering.get(h[p[0]]["frm"], []) if match(h[a]["type"], h[p[0]]["type"]) and a >> 1 != p[0] >> 1]
        if not ins:
            continue
        a = ins[int(rng.integers(0, len(ins)))]
        m1 = h[a]["list"][-1][0]; m2 = h[p[-1]]["list"][0][0]
        if not (uniq(m1) and uniq(m2)) or sw["claim"].get(m1) != i or a >> 1 == p[-1] >> 1:
            continue
        d1 = table[(m1, a >> 1)]["forward" if (a ^ 1) == E_of(a >> 1) else "reverse"]; d2 = table[(m2, p[-1] >> 1)]["forward" if p[-1] == E_of(p[-1] >> 1) else "reverse"]
        if d1 and d2:
            out.append((m1, 1 if d1[0] < 0 else 0, m2, 1 if d2[0] < 0 else 0))
        if len(out) >= n:
            break
    return out
