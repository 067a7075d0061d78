"""The restatement of step 7, ScaffoldMaker::makeScaffolds (matePair/scaffolding.cpp:31-98), as include/sage2ov.h states it: stringOverlapSize (OVERLAP),
mergeDisconnectedEdges (JOIN), one mergeFinal / mergeFinalSmall round (rows by rule (a), the XOR-keyed map, the order, the selection with its spent pairs, the erase
by node), the five loops and their thresholds -- in Python, over the graph form of tests/extend_model.py and the links of tests/test_links_host.py.  The insert
bounds are pinned (estimated once, on the first graph); the read-to-edge table and the links are rebuilt for every round.  seqs = {read id: the stored read}.
Shared by the CPU and GPU tests of the scaffold rounds; not a test module."""
import math
import numpy as np
import extend_model as X
import test_mate_estimate_host as H
import test_links_host as LH

NONE = X.NONE
EQUAL, OVERLAP, CONCAT, GAPPED = 0, 1, 2, 3
NO_SEARCH = -2
COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s.translate(COMP)[::-1]


def spell(stored, forward):
    """bytesToChars(readInt) or bytesToChars(readReverseInt) (overlapGraph.cpp:800-824)"""
    return stored if forward else revcomp(stored)


def overlap_size(s1, s2, L1=None, L2=None):
    """stringOverlapSize (overlapGraph.cpp:884-907), the loops as they stand; a position of s1 from L1 on is a mismatch (the reference reads past its string)"""
    L1 = len(s1) if L1 is None else L1; L2 = len(s2) if L2 is None else L2
    for i in range(0, L1 - 10):
        mis = 0; j = 0
        while j < L2 - i:
            if i + j >= L1 or s1[i + j] != s2[j]:
                mis += 1
                if mis > int((L2 - i) / 10) + 1:                                       # (C division truncates towards zero; L2 - i is positive here)
                    break
            j += 1
        if j == L2 - i:
            return i
    return -1


def overlap_rule(s1, s2):
    """the same by the sentence of the header: the smallest i in [0, L1 - 10) with L2 - i >= 0 and at most (L2 - i) / 10 + 1 mismatches over [0, L2 - i)"""
    L1, L2 = len(s1), len(s2)
    for i in range(0, L1 - 10):
        if L2 - i < 0:
            continue
        if sum(1 for j in range(L2 - i) if i + j >= L1 or s1[i + j] != s2[j]) <= (L2 - i) // 10 + 1:
            return i
    return -1


def threshold(reads, arl, genome_size, loop, iteration=1):
    """highTh of scaffolding.cpp:38-94: the coverage is a float of an integer quotient, the product a double that ceilf takes as a float"""
    if loop >= 3:
        return 2 if loop == 3 else 1
    coverage = np.float32((reads * arl) // genome_size)
    return int(math.ceil(np.float32(((0.05 if iteration > 5 else 0.10) * float(coverage)) * (100.0 / arl))))


def join_type(t1, t2):
    return (2 if t1 in (2, 3) else 0) | (1 if t2 in (1, 3) else 0)                     # scaffolding.cpp:290-297


class Graph(X.Graph):
    def is_E(self, x):
        """the half the read-to-edge table names: the one leaving the smaller node, of a loop the one with the higher index"""
        h = self.h[x]
        return h["frm"] < h["to"] or (h["frm"] == h["to"] and (x & 1) == 1)

    def join(self, e1, e2, gap, seqs):
        """mergeDisconnectedEdges(e1, e2, gap): the new forward half's index; self.last = dict(type, deleted, overlap, how) with overlap and how per list"""
        a, b, at, bt = self.h[e1], self.h[e2], self.h[e1 ^ 1], self.h[e2 ^ 1]
        assert e1 >> 1 != e2 >> 1 and self.alive[e1 >> 1] and self.alive[e2 >> 1] and a["list"] and b["list"]
        t = join_type(a["type"], b["type"])

        def reads(x, y):                                                               # getListOfReadsInDisconnectedEdges (overlapGraph.cpp:789-882)
            n1, n2 = x["to"], y["frm"]; o1 = 1 if x["type"] in (1, 3) else 0; o2 = 1 if y["type"] in (2, 3) else 0
            P, Q = x["list"][-1][4], y["list"][0][3]
            if n1 == n2:
                return list(x["list"]) + [(n1, o1, 0, P, Q)] + list(y["list"]), x["len"] + y["len"], NO_SEARCH, EQUAL
            s1, s2 = spell(seqs[n1], o1), spell(seqs[n2], o2); L1, L2 = len(s1), len(s2)
            o = overlap_size(s1, s2)
            if o > 0:
                d1 = d2 = o; how = OVERLAP
            elif gap < 0:
                d1, d2, how = L1, L2, CONCAT
            else:
                d1, d2, how = gap + L1, gap + L2, GAPPED
            return list(x["list"]) + [(n1, o1, 0, P, d1 & 0x7FF), (n2, o2, 0, d2 & 0x7FF, Q)] + list(y["list"]), x["len"] + y["len"] + d1, o, how
        lf, nf, of, hf = reads(a, b); lt, nt, ot, ht = reads(bt, at)
        fw = dict(frm=a["frm"], to=b["to"], type=t, reducible=1, len=nf, flow=1.0, list=lf)
        tw = dict(frm=b["to"], to=a["frm"], type=H.flip_type(t), reducible=1, len=nt, flow=1.0, list=lt)
        self.h += [fw, tw]; self.alive.append(True)
        self.last = dict(type=t, deleted=[], overlap=(of, ot), how=(hf, ht))
        for e in (e1, e2):
            if self.h[e]["flow"] <= 1.0:
                self.alive[e >> 1] = False; self.last["deleted"].append(True)
            else:
                self.h[e]["flow"] = X.f32(self.h[e]["flow"] - 1.0); self.h[e ^ 1]["flow"] = X.f32(self.h[e ^ 1]["flow"] - 1.0); self.last["deleted"].append(False)
        return len(self.h) - 2


def rows_of(g, raw, small):
    """the rows of a round from the unfiltered link rows `raw` of LH.links over g.parsed() (pairs under their pool numbers, second = the half's low bit): rule (a),
    the filter, in the table's export order (pair ordinal in the file, the half written first before its twin)"""
    p = g.parsed(); E = LH.e_half(p); arl = g.header[2]
    o = g.ordinals(); first = set(g.first_halves())
    mode = LH.SMALL if small else LH.FINAL
    out = []
    for (qa, sa, qb, sb, s, gap) in raw:
        a, b = 2 * qa + sa, 2 * qb + sb
        if a < b and LH.passes(mode, E[qa]["len"], E[qa]["flow"], E[qb]["len"], E[qb]["flow"], arl):
            out.append(((o[qa], 0 if a in first else 1, o[qb], 0 if b in first else 1), dict(e1=a ^ 1, e2=b, sup=s, gap=gap)))
    return [r for _, r in sorted(out, key=lambda x: x[0])]


def round_(g, pairs, bounds, k, high, flag, small, seqs):
    """one mergeFinal(k, high, flag) / mergeFinalSmall on g (changed in place) -> dict(merges=[..], rows, below_threshold, skipped, blocked, cycles, batches, overlaps,
    concatenated, gapped, ties, outside_reference)"""
    p = g.parsed(); table = H.read_edge_table(p)
    raw = LH.links(p, table, pairs, bounds.ests, bounds.max_upper, bounds.arl, k)
    before = g.ordinals(); h = g.h
    feasible = {}
    for (qa, sa, qb, sb, s, gap) in raw:
        feasible.setdefault(qa, [])
        feasible.setdefault(qb, [])
        if qb not in feasible[qa]:
            feasible[qa].append(qb)
        if qa not in feasible[qb]:
            feasible[qb].append(qa)
    rows = rows_of(g, raw, small)
    xk = lambda x: h[x]["frm"] ^ h[x]["to"]
    search = {}; filed = {}
    for r in rows:
        r["key"] = (xk(r["e1"]), xk(r["e2"])); r["len"] = h[r["e1"]]["len"] + h[r["e2"]]["len"]
        if r["key"] not in search or r["sup"] > search[r["key"]]:
            search[r["key"]] = r["sup"]
        for nd in (h[r["e1"]]["to"], h[r["e1"]]["frm"], h[r["e2"]]["to"], h[r["e2"]]["frm"]):
            filed.setdefault(nd, []).append(r["key"])
    rows.sort(key=lambda r: (-r["sup"], -r["len"]))                                   # (stable: ties keep the export order)
    at = [(r["sup"], r["len"]) for r in rows if r["sup"] >= high]
    out = dict(merges=[], rows=len(rows), below_threshold=0, skipped=0, blocked=0, cycles=0, batches=0, overlaps=0, concatenated=0, gapped=0,
               ties=len(set(at)) != len(at), outside_reference=False, identity_decides=0, named_again=0)
    hid = lambda x: (h[x]["frm"], h[x]["to"], h[x]["type"], h[x]["len"], 2 * h[x]["list"][0][0] + h[x]["list"][0][1])
    out["verdicts"] = []                                                             # per row in order: (verdict, pairs that count on edge_2's side, on edge_1's side)
    out["row_list"] = [(hid(r["e1"]), hid(r["e2"]), r["sup"], r["gap"]) for r in rows]      # the rows in order (b), the halves by (from, to, type, length, 2 * read + orientation of the first list entry)
    look = lambda x, y: search.get((x, y), search.get((y, x), 0))
    spent = set(); in_batch = set(); new_halves = []; limit = 1 if flag == 1 else 2
    for r in rows:
        e1, e2 = r["e1"], r["e2"]; p1, p2 = e1 >> 1, e2 >> 1
        if not g.alive[p1] or not g.alive[p2]:
            out["outside_reference"] = True; out["skipped"] += 1                        # (d)
            out["verdicts"].append(("skipped", None, None))
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
        verdict = lambda a, b: "cycle" if set(a) & set(b) else ("blocked" if len(a) > limit or len(b) > limit else "join")
        raw2 = [q for q in feas(p1) if look(xk(e1), xk(2 * q)) >= high]; raw1 = [q for q in feas(p2) if look(xk(2 * q), xk(e2)) >= high]
        if verdict(side1, side2) != verdict(raw1, raw2):
            out["identity_decides"] += 1                                               # the pointer-identity exclusion (is_E) changes what becomes of this row
        out["verdicts"].append((verdict(side1, side2), sorted(side1), sorted(side2)))
        if set(side1) & set(side2):
            out["cycles"] += 1
            continue
        if len(side1) > limit or len(side2) > limit:
            out["blocked"] += 1
            continue
        out["named_again"] += (p1 in spent) + (p2 in spent)
        if p1 in in_batch or p2 in in_batch:                                           # (e): a kept operand is named again: the batch so far goes first
            out["batches"] += 1; in_batch = set()
        node = h[e1]["to"]
        m = dict(frm=h[e1]["frm"], to=h[e2]["to"], support=r["sup"], gap=r["gap"], pair_first=before.get(p1, NONE), pair_second=before.get(p2, NONE))
        nh = g.join(e1, e2, r["gap"], seqs)
        m.update(type=g.last["type"], first_deleted=int(g.last["deleted"][0]), second_deleted=int(g.last["deleted"][1]), overlap=g.last["overlap"], how=g.last["how"])
        for hw in g.last["how"]:
            out["overlaps"] += hw == OVERLAP; out["concatenated"] += hw == CONCAT; out["gapped"] += hw == GAPPED
        in_batch |= {p1, p2}; spent |= {p1, p2}
        gone = [kk for kk in filed.get(node, []) if kk != r["key"] and kk in search]
        if m["first_deleted"] and gone:
            out["outside_reference"] = True                                            # (d): the reference reads the erase key from the freed edge_1 (:607)
        for kk in filed.get(node, []):
            search.pop(kk, None)
        out["merges"].append(m); new_halves.append(nh)
    if out["merges"]:
        out["batches"] += 1
    after = g.ordinals()
    for m, nh in zip(out["merges"], new_halves):
        m["pair_new"] = after.get(nh >> 1, NONE)
    return out


def scaffold(g, pairs, bounds, k, genome_size, reads, seqs, max_rounds=10000):
    """the five loops of :31-98 -> the rounds' results as (loop, high, result)"""
    arl = g.header[2]; low = threshold(reads, arl, genome_size, 1, 6); rounds = []
    for loop in (1, 2, 3, 4, 5):
        it = 1
        while True:
            assert len(rounds) < max_rounds
            high = threshold(reads, arl, genome_size, loop, it)
            r = round_(g, pairs, bounds, k, high, 2 if loop in (2, 5) else 1, loop == 5, seqs)
            rounds.append((loop, high, r)); it += 1
            if not r["merges"] and (loop > 2 or high == low):
                break
    return rounds


def joins_rows(r):
    """a round's joins as tuples in JOIN_DTYPE's order (without the padding)"""
    return [(m["frm"], m["to"], m["support"], m["gap"], m["pair_first"], m["pair_second"], m["pair_new"], m["overlap"][0], m["overlap"][1], m["type"], m["first_deleted"],
             m["second_deleted"], m["how"][0], m["how"][1]) for m in r["merges"]]
