"""The restatement of the fourth loop of ContigExtender::extendContigs, mergeShortOverlaps (matePair/mergeContigs.cpp:101-110, :1474-1648, :1788-1908), as
include/sage2ov.h states it (SHORT OVERLAPS): the raw gap sum of every link row, the rows of a round, the selection with no rival allowed and no cycle test, the
loop and its threshold -- on top of tests/scaffold_model.py (its graph form, its JOIN) and the link sweep of tests/test_links_host.py.  The selection is written
once, with the three parameters in which mergeShortOverlap and mergeAccordingToSupport / mergeAccordingToSupport2 differ, so that the CPU tests can hold it against
scaffold_model.round_ with step 7's parameters.  Shared by the CPU and GPU tests of the short-overlap rounds; not a test module."""
import math
import numpy as np
import extend_model as X
import scaffold_model as SM
import test_mate_estimate_host as H
import test_links_host as LH

NONE = X.NONE
M32 = LH.M32


def link_sums(g, table, pairs, ests, max_upper, arl, k):
    """the sweep of :1494-1585 (line for line scaffolding.cpp:831-892, LH.links) keeping what :1587 reads: [(pair_a, second_a, pair_b, second_b, support, gapSum)],
    every ordered (a, b) with support >= 1, ascending; gapSum is the int32_t of :1577"""
    pr = H.by_read(table)
    nodes = {a["frm"] for _, a, b in g["pairs"]} | {a["to"] for _, a, b in g["pairs"]}
    mates = {}
    for L, pl in pairs.items():
        for (a, b, ta, tb) in sorted({(a, b, sa, sb) for a, sa, b, sb in pl} | {(b, a, sb, sa) for a, sa, b, sb in pl}):
            mates.setdefault(a, []).append((b, ta, tb, L))
    hv = LH.halves_of(g)
    unique_pair = lambda r: pr[r][0] if r not in nodes and len(pr.get(r, [])) == 1 else None      # isUniqueInEdge (:1102-1110)
    loc = lambda r, q, isE: table[(r, q)]["forward" if isE else "reverse"]
    acc = {}
    for (qa, sa), (a, ea) in hv.items():
        run = 0
        for (m1, o, f, dp, dn) in a["list"]:
            run += dp
            if run > max_upper:                                                        # :1533
                break
            if unique_pair(m1) != qa:                                                  # :1536
                continue
            for (m2, t1, t2, L) in mates.get(m1, []):
                qb = unique_pair(m2)
                if not ests[L]["valid"] or qb is None or qb == qa:                     # :1542
                    continue
                for sb in (0, 1):
                    b, eb = hv[(qb, sb)]
                    hit = None
                    for x in loc(m1, qa, ea):                                          # :1549-1573: the first (x, y) in list order
                        for y in loc(m2, qb, eb):
                            d = abs(x) + abs(y) if (1 if t1 else -1) * x < 0 and (1 if t2 else -1) * y < 0 else LH.NO_SIGN
                            if d + 2 * arl < ests[L]["upper"] + k:                     # :1565
                                hit = d
                                break
                        if hit is not None:
                            break
                    if hit is not None:
                        s, gs = acc.get((qa, sa, qb, sb), (0, 0))
                        acc[(qa, sa, qb, sb)] = (s + 1, (gs + ests[L]["mean"] - (hit + 2 * arl)) & M32)      # :1576-1577
    out = []
    for key in sorted(acc):
        s, gs = acc[key]
        out.append(key + (s, gs - (1 << 32) if gs >= (1 << 31) else gs))
    return out


def quotient(gap_sum, support):
    """gapSum / support of :1592: an int32_t division truncates towards zero"""
    return -(-gap_sum // support) if gap_sum < 0 else gap_sum // support


def threshold(reads, arl, genome_size):
    """highTh of :43 and :102: the coverage is a float of an integer quotient, the product a double that ceilf takes as a float"""
    coverage = np.float32((reads * arl) // genome_size)
    return int(math.ceil(np.float32((0.05 * float(coverage)) * (100.0 / arl))))


def passes(len1, flow1, len2, flow2, gap_sum, arl):
    """:1500 and :1587; flows None: the graph carries none, no row"""
    if flow1 is None or flow2 is None:
        return False
    t = LH.threshold(arl)                                                              # mergeContigs.cpp:21 is scaffolding.cpp:20
    return (flow1 > 0 and len1 > t) and (flow2 > 0 and len2 > t) and gap_sum <= 0


def short_filter(g, sums, flows=True):
    """the row filter of a short-overlap round over the rows of link_sums; flows False: a graph whose host copy has no flow array"""
    p = g.parsed(); E = LH.e_half(p); arl = g.header[2]
    return lambda qa, qb, s, gs: passes(E[qa]["len"], E[qa]["flow"] if flows else None, E[qb]["len"], E[qb]["flow"] if flows else None, gs, arl)


def final_filter(g, small):
    """step 7's filters in the same form (scaffold_model.rows_of)"""
    p = g.parsed(); E = LH.e_half(p); arl = g.header[2]; mode = LH.SMALL if small else LH.FINAL
    return lambda qa, qb, s, gs: LH.passes(mode, E[qa]["len"], E[qa]["flow"], E[qb]["len"], E[qb]["flow"], arl)


def rows_of(g, sums, keep):
    """rule (a) and the filter, in the table's export order; a row's gap is the quotient"""
    o = g.ordinals(); first = set(g.first_halves())
    out = []
    for (qa, sa, qb, sb, s, gs) in sums:
        a, b = 2 * qa + sa, 2 * qb + sb
        if a < b and keep(qa, qb, s, gs):
            out.append(((o[qa], 0 if a in first else 1, o[qb], 0 if b in first else 1), dict(e1=a ^ 1, e2=b, sup=s, gap=quotient(gs, s), gap_sum=gs)))
    return [r for _, r in sorted(out, key=lambda x: x[0])]


def select(g, sums, rows, high, limit, cycle_test, seqs):
    """the selection both steps share (scaffolding.cpp:488-769, mergeContigs.cpp:1788-1908) on g (changed in place): `limit` rivals at or above `high` are allowed on
    each side, a rival on both sides is a CYCLE only with cycle_test -> the dict of scaffold_model.round_"""
    before = g.ordinals(); h = g.h
    feasible = {}
    for (qa, sa, qb, sb, s, gs) in sums:
        feasible.setdefault(qa, []); feasible.setdefault(qb, [])
        if qb not in feasible[qa]:
            feasible[qa].append(qb)
        if qa not in feasible[qb]:
            feasible[qb].append(qa)
    xk = lambda x: h[x]["frm"] ^ h[x]["to"]
    search = {}; filed = {}
    for r in rows:
        r["key"] = (xk(r["e1"]), xk(r["e2"])); r["len"] = h[r["e1"]]["len"] + h[r["e2"]]["len"]
        if r["key"] not in search or r["sup"] > search[r["key"]]:
            search[r["key"]] = r["sup"]
        for nd in (h[r["e1"]]["to"], h[r["e1"]]["frm"], h[r["e2"]]["to"], h[r["e2"]]["frm"]):
            filed.setdefault(nd, []).append(r["key"])
    rows = sorted(rows, key=lambda r: (-r["sup"], -r["len"]))                          # (stable: ties keep the export order)
    at = [(r["sup"], r["len"]) for r in rows if r["sup"] >= high]
    out = dict(merges=[], rows=len(rows), below_threshold=0, skipped=0, blocked=0, cycles=0, batches=0, overlaps=0, concatenated=0, gapped=0,
               ties=len(set(at)) != len(at), outside_reference=False, named_again=0, verdicts=[])
    look = lambda x, y: search.get((x, y), search.get((y, x), 0))
    spent = set(); in_batch = set(); new_halves = []
    for r in rows:
        e1, e2 = r["e1"], r["e2"]; p1, p2 = e1 >> 1, e2 >> 1
        if not g.alive[p1] or not g.alive[p2]:
            out["outside_reference"] = True; out["skipped"] += 1; out["verdicts"].append(("skipped", None, None))      # (d)
            continue
        if r["key"] not in search:
            out["skipped"] += 1; out["verdicts"].append(("skipped", None, None))
            continue
        if r["sup"] < high:
            out["below_threshold"] += 1; out["verdicts"].append(("below", None, None))
            continue
        feas = lambda q: [] if q in spent else [x for x in feasible.get(q, []) if x not in spent]
        side2 = [q for q in feas(p1) if not (q == p2 and g.is_E(e2)) and look(xk(e1), xk(2 * q)) >= high]
        side1 = [q for q in feas(p2) if not (q == p1 and g.is_E(e1)) and look(xk(2 * q), xk(e2)) >= high]
        if cycle_test and set(side1) & set(side2):
            out["cycles"] += 1; out["verdicts"].append(("cycle", sorted(side1), sorted(side2)))
            continue
        if len(side1) > limit or len(side2) > limit:
            out["blocked"] += 1; out["verdicts"].append(("blocked", sorted(side1), sorted(side2)))
            continue
        out["verdicts"].append(("join", sorted(side1), sorted(side2)))
        out["named_again"] += (p1 in spent) + (p2 in spent)
        if p1 in in_batch or p2 in in_batch:                                           # (e): a kept operand is named again: the batch so far goes first
            out["batches"] += 1; in_batch = set()
        node = h[e1]["to"]
        m = dict(frm=h[e1]["frm"], to=h[e2]["to"], support=r["sup"], gap=r["gap"], pair_first=before.get(p1, NONE), pair_second=before.get(p2, NONE))
        nh = g.join(e1, e2, r["gap"], seqs)
        m.update(type=g.last["type"], first_deleted=int(g.last["deleted"][0]), second_deleted=int(g.last["deleted"][1]), overlap=g.last["overlap"], how=g.last["how"])
        for hw in g.last["how"]:
            out["overlaps"] += hw == SM.OVERLAP; out["concatenated"] += hw == SM.CONCAT; out["gapped"] += hw == SM.GAPPED
        in_batch |= {p1, p2}; spent |= {p1, p2}
        if m["first_deleted"] and [kk for kk in filed.get(node, []) if kk != r["key"] and kk in search]:
            out["outside_reference"] = True                                            # (d): the reference reads the erase key from the freed edge_1 (:1887)
        for kk in filed.get(node, []):
            search.pop(kk, None)
        out["merges"].append(m); new_halves.append(nh)
    if out["merges"]:
        out["batches"] += 1
    after = g.ordinals()
    for m, nh in zip(out["merges"], new_halves):
        m["pair_new"] = after.get(nh >> 1, NONE)
    out["row_list"] = [(r["e1"], r["e2"], r["sup"], r["gap"], r["gap_sum"]) for r in rows]
    return out


def sums_of(g, pairs, bounds, k):
    p = g.parsed()
    return link_sums(p, H.read_edge_table(p), pairs, bounds.ests, bounds.max_upper, bounds.arl, k)


def round_(g, pairs, bounds, k, high, seqs, flows=True):
    """one mergeShortOverlaps(k, high) on g (changed in place)"""
    sums = sums_of(g, pairs, bounds, k)
    return select(g, sums, rows_of(g, sums, short_filter(g, sums, flows)), high, 0, False, seqs)


def scaffold_round(g, pairs, bounds, k, high, flag, small, seqs):
    """step 7's round through the same selection: what scaffold_model.round_ computes"""
    sums = sums_of(g, pairs, bounds, k)
    return select(g, sums, rows_of(g, sums, final_filter(g, small)), high, 1 if flag == 1 else 2, True, seqs)


def loop(g, pairs, bounds, k, genome_size, reads, seqs, max_rounds=10000):
    """:101-110: rounds at one threshold until one joins nothing -> the rounds' results"""
    high = threshold(reads, g.header[2], genome_size); out = []
    while True:
        assert len(out) < max_rounds
        out.append(round_(g, pairs, bounds, k, high, seqs))
        if not out[-1]["merges"]:
            return out
