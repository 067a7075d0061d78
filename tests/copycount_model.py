"""tests/copycount_model.py -- TEST INFRASTRUCTURE: step 5 (CopyCountEstimator, overlapGraph/copycountEstimator.cpp) around its solver, restated in Python.

The state restated is the reference's after loadOverlapGraphFromFile: `graph` is test_mate_estimate_host.parse_graph(text, fold=False), every record pair of the
file in file order (a loop's pair twice, as the writer writes it), and a node's edge list is the reverse of file order over the records that start at the node
(insertIntoList puts the newest first).  `freq[id]` is Read::frequency (uint16).  `n` is numberOfReads as step 5 sees it: checkIfAllReadsPresent
(overlapGraph.cpp:445-493, called at main.cpp:199) has replaced the good reads of the file's header by present_reads(), and P.graph5 carries that number.

Arithmetic: numpy float32 / float64, one operation per line where the order or the width matters.  Every `log` is glibc's logf / log through ctypes -- the
functions the reference's translation unit calls: with <cmath> and `using namespace std`, log(float) is the float overload and log(uint64_t) the double one.
"""
import ctypes
import ctypes.util

import numpy as np

f32, f64 = np.float32, np.float64
TWO63 = 1 << 63
M64 = (1 << 64) - 1
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = ctypes.c_float; _libm.logf.argtypes = [ctypes.c_float]
_libm.log.restype = ctypes.c_double; _libm.log.argtypes = [ctypes.c_double]


def logf(x):
    return f32(_libm.logf(float(f32(x))))


def logd(x):
    return f64(_libm.log(float(x)))


def u2f(v):
    """(float)v of a uint64_t: one rounding"""
    return np.array(v & M64, dtype=np.uint64).astype(np.float32)[()]


def u2d(v):
    return np.array(v & M64, dtype=np.uint64).astype(np.float64)[()]


def k_of(rec, freq):
    return sum(int(freq[e[0]]) for e in rec["list"])


def present_reads(graph, freq):
    """checkIfAllReadsPresent: the frequencies of the reads that are a node with an edge or stand on a list"""
    seen = set()
    for _, a, b in graph["pairs"]:
        for r in (a, b):
            seen.add(r["frm"]); seen.update(e[0] for e in r["list"])
    return sum(int(freq[i]) for i in seen)


# ---- genome size (:29-100)
def to_u64(x):
    """(uint64_t)x as the reference's build leaves it: a float that does not fit gives 2^63 -> (value, degenerate)"""
    if not np.isfinite(x) or x >= f32(2.0 ** 64) or x < 0:
        return TWO63, 1
    return int(x), 0


def size_of_sums(n, delta_sum, k_sum):
    with np.errstate(all="ignore"):
        q = u2f(n) / u2f(k_sum)
        x = q * u2f(delta_sum)
    return to_u64(x)


def a_stat(delta, k, ratio, lg):
    t1 = f32(delta) * ratio
    t2 = u2f(k) * lg
    return f32(t1 - t2)


def round_sums(graph, freq, n, previous):
    """deltaSum, kSum of findGenomeSize(previous): the records with from < to (each non-loop pair once; a loop never)"""
    ds = ks = 0
    with np.errstate(all="ignore"):
        ratio = u2f(n) / u2f(previous) if previous else None
        l2 = logf(2)
        for _, a, b in graph["pairs"]:
            for r in (a, b):
                if r["frm"] < r["to"]:
                    delta = r["len"] - 1; k = k_of(r, freq)
                    if previous:
                        ok = a_stat(delta, k, ratio, l2) >= 3 and delta >= 1000
                    else:
                        ok = r["len"] > 500
                    if ok:
                        ds += delta; ks += k
    return ds, ks


def rounds(sums, n):
    """genomeSizeEstimation over sums(previous) -> (deltaSum, kSum): dict(estimates, rounds, genome_size, degenerate, agreed)"""
    previous = 0; est = []; deg = 0; agreed = False
    for _ in range(10):
        ds, ks = sums(previous)
        cur, dg = size_of_sums(n, ds, ks)
        est.append(cur); deg = dg
        if cur == previous:
            agreed = True
            break
        previous = cur
    return dict(estimates=est, rounds=len(est), genome_size=est[-1], degenerate=deg, agreed=agreed)


def genome_size(graph, freq, n):
    return rounds(lambda prev: round_sums(graph, freq, n, prev), n)


# ---- classes (:124-153, :286-320)
def a_stats(delta, k, n, G):
    with np.errstate(all="ignore"):
        ratio = u2f(n) / u2f(G)
        return [None] + [a_stat(delta, k, ratio, logf(f32(j + 1) / f32(j))) for j in range(1, 21)]


def classify(rec, freq, n, G):
    """-> (class, flow_lb): 'simple', 'once' or 'many'"""
    if not rec["list"]:
        return "simple", 0
    delta = rec["len"] - 1
    a = a_stats(delta, k_of(rec, freq), n, G)
    if a[1] >= 3 and delta >= 1000:
        return "once", 1
    lb = 0
    if delta > 1000:
        for j in range(1, 20):
            if a[j] < -3 and a[j + 1] > 3:
                lb = j + 1
                break
    elif len(rec["list"]) > 35:
        lb = 1
    return "many", lb


# ---- costs of a many-pair (:321-342): three float accumulators folded over the list in list order
def costs(rec, freq, n, G):
    """-> the three printed costs (float32, already * 10)"""
    N = G
    xi = np.asarray([int(freq[e[0]]) for e in rec["list"]], dtype=np.int64)
    m = [(n - int(x)) & M64 for x in xi]                        # (n - xi): uint64_t
    md = np.asarray([u2d(v) for v in m], dtype=f64); mf = np.asarray([u2f(v) for v in m], dtype=f32)
    xf = xi.astype(f32)                                          # xi * <float>: the int goes to float
    l1, l3, l5, l1000 = logf(1), logf(3), logf(5), logf(1000)
    dN3, dN1000 = logd(u2d(N - 3)), logd(u2d(N - 1000))          # log(N - first_UB), log(N - third_UB): integer argument -> double
    fN1, fN3, fN5 = logf(u2f(N - 1)), logf(u2f(N - 3)), logf(u2f(N - 5))
    with np.errstate(all="ignore"):
        # cost_1: -(xi*log(3f)) - (n-xi)*log(N-3) - (-(xi*log(1f)) - (n-xi)*log((float)(N-1)))
        a = xf * l3
        b = md * dN3
        t = (-a).astype(f64) - b
        c = xf * l1
        d = mf * fN1
        inner = (-c) - d
        term1 = t - inner.astype(f64)
        # cost_2: every log has a float argument: float throughout
        a = xf * l5
        b = mf * fN5
        t = (-a) - b
        c = xf * l3
        d = mf * fN3
        inner = (-c) - d
        term2 = t - inner
        # cost_3: -(xi*log(1000f)) - (n-xi)*log(N-1000) - (-(xi*log(5f)) - (n-xi)*log((float)(N-5)))
        a = xf * l1000
        b = md * dN1000
        t = (-a).astype(f64) - b
        c = xf * l5
        d = mf * fN5
        inner = (-c) - d
        term3 = t - inner.astype(f64)
        c1 = f32(0); c3 = f32(0)
        for v in term1:
            c1 = f32(f64(c1) + v)
        for v in term3:
            c3 = f32(f64(c3) + v)
        c2 = np.add.accumulate(term2, dtype=f32)[-1] if len(term2) else f32(0)      # (sequential in float; 0 + t is t)
        c1 = c1 / f32(2); c2 = c2 / f32(2); c3 = c3 / f32(995)
        return f32(c1 * f32(10)), f32(c2 * f32(10)), f32(c3 * f32(10))


# ---- the network (:183-355)
def node_lists(graph):
    """node -> its edge list after loading: [(file position of the record, record, its twin)], newest first"""
    lists = {}; pos = 0
    for _, a, b in graph["pairs"]:
        for r, t in ((a, b), (b, a)):
            lists.setdefault(r["frm"], []).insert(0, (pos, r, t)); pos += 1
    return lists


def end_points(rec, ni):
    u = ni[rec["frm"]]; v = ni[rec["to"]]
    u1i, u1o, u2i, u2o = u, u + 1, u + 2, u + 3
    v1i, v1o, v2i, v2o = v, v + 1, v + 2, v + 3
    return {0: (v1o, u1i, u2o, v2i), 1: (u2o, v1i, v2o, u1i), 2: (u1o, v2i, v1o, u2i), 3: (u1o, v1i, v2o, u2i)}[rec["type"]]


def network(graph, freq, n, G):
    """-> dict(arcs=[(from, to, lower, upper, cost float32)], counters, node_index): the arcs in input.cs2's order, the 2 -> 1 arc first"""
    lists = node_lists(graph); nodes = sorted(lists)
    ni = {i: 3 + 4 * r for r, i in enumerate(nodes)}
    cnt = dict(nodes=len(nodes), edges=0, simple=0, once=0, many=0)
    edge_arcs = []
    for i in nodes:
        for _, r, _t in lists[i]:
            if i >= r["to"]:
                cnt["edges"] += 1
                cls, lb = classify(r, freq, n, G); cnt[cls] += 1
                n1, n2, n3, n4 = end_points(r, ni)
                if cls == "simple":
                    rows = [(0, 100, f32(f32(10000) * f32(10)))]
                elif cls == "once":
                    rows = [(1, 1, f32(f32(1) * f32(10)))]
                else:
                    c1, c2, c3 = costs(r, freq, n, G)
                    rows = [(min(lb, 3), 3, c1), (max(0, min(lb, 5) - 3), 2, c2), (max(0, min(lb, 1000) - 5), 995, c3)]
                for lo, up, c in rows:
                    edge_arcs += [(n1, n2, lo, up, c), (n3, n4, lo, up, c)]
    n_nodes = 4 * len(nodes) + 2
    arcs = [(2, 1, 1, 100 * n_nodes, f32(0))]
    big, one = f32(f32(1000000) * f32(10)), f32(f32(1) * f32(10))
    for i in nodes:
        c = ni[i]
        arcs += [(1, c, 0, 100, big), (c + 1, 2, 0, 100, big), (1, c + 2, 0, 100, big), (c + 3, 2, 0, 100, big), (c, c + 1, 0, 100, one), (c + 2, c + 3, 0, 100, one)]
    arcs += edge_arcs
    assert len(arcs) == 1 + 6 * cnt["nodes"] + 2 * (cnt["edges"] - cnt["many"]) + 6 * cnt["many"]
    return dict(arcs=arcs, counters=cnt, node_index=ni, network_nodes=n_nodes)


def cs2_text(net):
    """input.cs2: the header, the two node lines, the arcs; costs as `ostream << std::fixed << float` prints them.  The 2 -> 1 arc's cost is the literal 0"""
    out = ["p min %d %d\nn 1 0\nn 2 0\n" % (net["network_nodes"], len(net["arcs"]))]
    a = net["arcs"][0]
    out.append("a %d %d %d %d 0\n" % a[:4])
    out += ["a %d %d %d %d %f\n" % (fr, to, lo, up, float(c)) for fr, to, lo, up, c in net["arcs"][1:]]
    return "".join(out).encode()


# ---- a solver's flows back onto the graph (:362-403)
def parse_solution(text):
    t = text.split()
    return [(int(t[i]), int(t[i + 1]), int(t[i + 2])) for i in range(0, len(t) - 2, 3)]


def apply_solution(graph, node_index, lines):
    """adds the lines' flows to the records' `flow` in place, then averages the halves -> dict(t_to_s_flow, flow_different)"""
    lists = node_lists(graph)
    inv = {}
    for i, c in node_index.items():
        for x in range(4):
            inv[c + x] = i
    tts = None
    for fr, to, fl in lines:
        if (fr, to) in ((1, 2), (2, 1)):
            tts = fl
        elif fr > 2 and to > 2:
            a, b = inv[fr], inv[to]
            if a != b:
                for _, r, _t in lists[a]:
                    if r["to"] == b:
                        r["flow"] = f32(f32(r["flow"]) + u2f(fl))
                        break
    diff = 0
    for i in sorted(lists):
        for _, r, t in lists[i]:
            avg = f32((f32(r["flow"]) + f32(t["flow"])) / f32(2))
            if f32(r["flow"]) != f32(t["flow"]):
                diff += 1
            r["flow"] = avg; t["flow"] = avg
    return dict(t_to_s_flow=tts, flow_different=diff)


def graph5_text(graph, G, n):
    """P.graph5: saveOverlapGraphInFile's text of the loaded graph -- the records in file order again, the genome size in line 1"""
    import test_mate_estimate_host as H
    recs = [r for _, a, b in graph["pairs"] for r in (a, b)]
    return H.graph_text((G, n, graph["header"][2]), [dict(r, flow=float(r["flow"])) for r in recs]).encode()
