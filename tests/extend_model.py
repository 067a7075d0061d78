"""The restatement of the first loop of ContigExtender::extendContigs (matePair/mergeContigs.cpp:47-60) as include/sage2ov.h states it: mergeEdgesAndUpdate
(the primitive), one findMatepairSupports (list, XOR-keyed map, selection, blocked nodes, erase by node), the loop and its threshold -- in Python, over the
parsed-graph form of test_mate_estimate_host / test_mate_support_host.  The insert bounds are pinned (estimated once, on the first graph); the read-to-edge table is
rebuilt for every round.  Shared by the CPU, reference and GPU tests of the merge rounds; not a test module."""
import copy
import math
import numpy as np
import test_mate_estimate_host as H
import test_mate_support_host as MS

COMBINED = {(0, 0): 0, (1, 2): 0, (0, 1): 1, (1, 3): 1, (2, 0): 2, (3, 2): 2, (2, 1): 3, (3, 3): 3}      # overlapGraph.cpp:259-266
NONE = 0xFFFFFFFF


def f32(x):
    return float(np.float32(x))


def threshold(reads, arl, genome_size, iteration=1):
    """highTh of mergeContigs.cpp:43-54: the coverage is a float of an integer quotient, the product a double that ceilf takes as a float"""
    coverage = np.float32((reads * arl) // genome_size)
    factor = 0.20
    if genome_size > 1000000000:
        factor = 0.10 if 4 <= iteration <= 6 else (0.05 if iteration > 6 else 0.20)
    return int(math.ceil(np.float32((factor * float(coverage)) * (100.0 / arl))))


class Graph:
    """the half-edge pool: pair p = halves 2 p (the record) and 2 p + 1 (its twin), the index is the age.  From H.parse_graph(text): pairs in file order, as
    sage2ov_graph_load_composite makes them"""

    def __init__(self, parsed):
        self.header = parsed["header"]; self.h = []; self.alive = []
        for _, a, b in parsed["pairs"]:
            self.h += [copy.deepcopy(a), copy.deepcopy(b)]; self.alive.append(True)

    def save_order(self):
        """the halves sage2ov_graph4_save opens a record pair with: node ascending, then pool order; both halves of a loop"""
        return sorted((x for x in range(len(self.h)) if self.alive[x >> 1] and self.h[x]["frm"] <= self.h[x]["to"]), key=lambda x: (self.h[x]["frm"], x))

    def first_halves(self):
        """ordinal -> the half that opens the pair's record (a loop: at its first writing)"""
        seen = set(); out = []
        for x in self.save_order():
            if x >> 1 not in seen:
                seen.add(x >> 1); out.append(x)
        return out

    def ordinals(self):
        """pair -> the ordinal of its record pair in the file (a loop, written twice: the first time), as in sage2ov_read_edge and sage2ov_support"""
        out = {}
        for o, x in enumerate(self.save_order()):
            out.setdefault(x >> 1, o)
        return out

    def half(self, ordinal, reversed_):
        return self.save_order()[ordinal] ^ (1 if reversed_ else 0)

    def text(self, header=None):
        recs = [self.h[y] for x in self.save_order() for y in (x, x ^ 1)]
        return H.graph_text(header or self.header, recs)

    def parsed(self):
        """the alive pairs under their pool numbers, for MS.supports / H.read_edge_table"""
        return dict(header=self.header, pairs=[(p, self.h[2 * p], self.h[2 * p + 1]) for p in range(len(self.alive)) if self.alive[p]])

    def flows(self):
        return np.asarray([self.h[y]["flow"] for x in self.first_halves() for y in (x, x ^ 1)], dtype=np.float32)

    def merge(self, e1, e2, type_of_merge=1):
        """mergeEdgesAndUpdate(e1, e2): the new forward half's index, or None when the reference refuses"""
        a, b = self.h[e1], self.h[e2]
        t = COMBINED.get((a["type"], b["type"]))
        if e1 == e2 or e1 == (e2 ^ 1) or not self.alive[e1 >> 1] or not self.alive[e2 >> 1] or t is None:
            return None
        f1, f2 = a["flow"], b["flow"]
        f = 0.0 if (f1 == 0 and f2 == 0) else (1.0 if type_of_merge == 1 else min(f1, f2))

        def reads(x, y):                                                             # getListOfReads (overlapGraph.cpp:299-336)
            node = (x["to"], 1 if x["type"] in (1, 3) else 0, 0, x["list"][-1][4] if x["list"] else x["len"], y["list"][0][3] if y["list"] else y["len"])
            return list(x["list"]) + [node] + list(y["list"])
        at, bt = self.h[e1 ^ 1], self.h[e2 ^ 1]
        fw = dict(frm=a["frm"], to=b["to"], type=t, reducible=1, len=a["len"] + b["len"], flow=f, list=reads(a, b))
        tw = dict(frm=b["to"], to=a["frm"], type=H.flip_type(t), reducible=1, len=at["len"] + bt["len"], flow=f, list=reads(bt, at))
        self.h += [fw, tw]; self.alive.append(True)
        self.last = dict(flow=f, type=t, deleted=[])
        for e, fl in ((e1, f1), (e2, f2)):
            if fl <= f:
                self.alive[e >> 1] = False; self.last["deleted"].append(True)
            else:
                self.h[e]["flow"] = f32(self.h[e]["flow"] - f); self.h[e ^ 1]["flow"] = f32(self.h[e ^ 1]["flow"] - f); self.last["deleted"].append(False)
        return len(self.h) - 2


class Bounds:
    """the insert estimates of one meanSdEstimation: those of the graph they are made on, kept for every later round"""

    def __init__(self, g, pairs):
        p = g.parsed()
        _, self.ests, (self.min_upper, self.max_upper) = MS.support_inputs(p, pairs)
        self.arl = g.header[2]


def round_(g, pairs, bounds, k, high, low=1):
    """one findMatepairSupports(k, high) on g (changed in place).  -> dict(merges=[dict(node, frm, to, support, pair_in, pair_out, pair_new, flow, type, in_deleted,
    out_deleted)], entries, at_threshold, refused, blocked, ties, outside_reference)"""
    p = g.parsed(); table = H.read_edge_table(p)
    before = g.ordinals()
    h = g.h
    lst = []
    for (i, qa, qb, s) in MS.supports(p, table, pairs, bounds.ests, bounds.max_upper, bounds.arl, k):
        if s > 1:
            a = next(x for x in (2 * qa, 2 * qa + 1) if h[x]["frm"] == i); b = next(x for x in (2 * qb, 2 * qb + 1) if h[x]["frm"] == i)
            lst.append((i, a, b, s))
    lst.sort(key=lambda e: (e[0], -e[1], -e[2]))                                      # node ascending, in-half newest first, out-half newest first
    ents = [dict(e1=a ^ 1, e2=b, sup=s, node=i) for (i, a, b, s) in lst]
    xk = lambda x: h[x]["frm"] ^ h[x]["to"]
    key = lambda x, y: (xk(x), xk(y))
    search = {}; filed = {}
    for n, e in enumerate(ents):
        kk = key(e["e1"], e["e2"]); e["key"] = kk
        if kk not in search or e["sup"] > search[kk]:
            search[kk] = e["sup"]
        for nd in (h[e["e1"]]["to"], h[e["e1"]]["frm"], h[e["e2"]]["to"], h[e["e2"]]["frm"]):
            filed.setdefault(nd, []).append(n)
    order = sorted(range(len(ents)), key=lambda n: -ents[n]["sup"])                 # (stable)
    at = [ents[n]["sup"] for n in order if ents[n]["sup"] >= high]
    out = dict(merges=[], entries=len(ents), at_threshold=len(at), refused=0, blocked=0, ties=len(set(at)) != len(at), outside_reference=False)
    blocked = set(); new_halves = []
    alive = lambda x: g.alive[x >> 1]

    def leaving(node):                                                               # the node's list as it is now, newest first
        return [x for x in range(len(h) - 1, -1, -1) if alive(x) and h[x]["frm"] == node]
    for n in order:
        e = ents[n]; e1, e2 = e["e1"], e["e2"]
        if not alive(e1) or not alive(e2):
            continue
        if e["key"] not in search:
            continue
        node = h[e1]["to"]
        if node in blocked:
            out["blocked"] += 1
            continue
        if e["sup"] < high:
            break
        unique = True
        for v in leaving(node):
            if not (h[v]["flow"] >= 1 and h[v]["list"] and h[v]["frm"] != h[v]["to"]):
                continue
            if (v ^ 1) != e1 and (h[v ^ 1]["type"], h[e2]["type"]) in COMBINED:
                if search.get(key(v ^ 1, e2), search.get(key(e2 ^ 1, v), 0)) > low:
                    unique = False
            if v != e2 and (h[e1]["type"], h[v]["type"]) in COMBINED:
                if search.get(key(e1, v), search.get(key(v ^ 1, e1 ^ 1), 0)) > low:
                    unique = False
        if not unique:
            out["refused"] += 1
            continue
        blocked |= {h[v]["to"] for v in leaving(node) if h[v]["to"] != h[v]["frm"]}
        m = dict(node=node, frm=h[e1]["frm"], to=h[e2]["to"], support=e["sup"], pair_in=before.get(e1 >> 1, NONE), pair_out=before.get(e2 >> 1, NONE))
        nh = g.merge(e1, e2, 1)
        if nh is None:
            continue
        m.update(flow=g.last["flow"], type=g.last["type"], in_deleted=int(g.last["deleted"][0]), out_deleted=int(g.last["deleted"][1]))
        listed = [x for x in filed.get(node, []) if x != n and ents[x]["key"] in search and ents[x]["node"] == node]
        if m["in_deleted"] and listed:
            out["outside_reference"] = True                                          # the reference reads the freed edge1 here (difference 2)
        for x in filed.get(node, []):
            search.pop(ents[x]["key"], None)
        out["merges"].append(m); new_halves.append(nh)
    after = g.ordinals()
    for m, nh in zip(out["merges"], new_halves):
        m["pair_new"] = after.get(nh >> 1, NONE)
    return out


def extend(g, pairs, bounds, k, genome_size, reads, low=1, max_rounds=10000):
    """the loop of :47-60 -> the rounds' results, the last one without a merge"""
    rounds = []
    for it in range(1, max_rounds + 1):
        r = round_(g, pairs, bounds, k, threshold(reads, g.header[2], genome_size, it), low)
        rounds.append(r)
        if not r["merges"]:
            return rounds
    raise RuntimeError("no fixed point")


def read_edge_set(g):
    """the read-to-edge table of g as a set of (read, pair ordinal, forward locations, reverse locations)"""
    o = g.ordinals()
    return {(r, o[q], tuple(e["forward"]), tuple(e["reverse"])) for (r, q), e in H.read_edge_table(g.parsed()).items()}


def merges_rows(r):
    """a round's merges as tuples in MERGE_DTYPE's order (without the padding)"""
    return [(m["node"], m["frm"], m["to"], m["support"], m["pair_in"], m["pair_out"], m["pair_new"], m["flow"], m["type"], m["in_deleted"], m["out_deleted"]) for m in r["merges"]]
