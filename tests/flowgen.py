"""Seeded min-cost-flow networks for the solver tests (tests/test_flow_host.py, tests/test_gpu_flow.py): circulations of the shape step 5 builds
(copycountEstimator.cpp:185-355), and small hand cases.  A network is (n, arcs) with arcs a numpy record array of (from, to, lower, upper, cost): the layout of
sage2ov_mcf_arc.  Nothing here depends on the library."""
import numpy as np

ARC = np.dtype([("from", np.uint32), ("to", np.uint32), ("lower", np.int32), ("upper", np.int32), ("cost", np.int64)])
BIG = 10_000_000


def arcs_of(rows):
    a = np.zeros(len(rows), ARC)
    for i, r in enumerate(rows): a[i] = tuple(r)
    return a


def split(arcs):
    return (arcs["from"].astype(np.int64), arcs["to"].astype(np.int64), arcs["lower"].astype(np.int64), arcs["upper"].astype(np.int64), arcs["cost"].astype(np.int64))


def reference_shape(seed, graph_nodes, edges):
    """source 1, sink 2, `2 1 1 U 0`; four network nodes and six arcs per graph node (source / sink arcs of cost 10^7, in-out arcs of cost 10); per edge and strand
    an out -> in arc pair: simple (0 100 100000), once (1 1 10), or three parallel classes (bounds as :333-338) with costs out of order, some negative"""
    rng = np.random.default_rng(seed)
    n = 4 * graph_nodes + 2
    rows = [(2, 1, 1, 100 * n, 0)]
    for r in range(graph_nodes):
        c = 3 + 4 * r
        rows += [(1, c, 0, 100, BIG), (c + 1, 2, 0, 100, BIG), (1, c + 2, 0, 100, BIG), (c + 3, 2, 0, 100, BIG), (c, c + 1, 0, 100, 10), (c + 2, c + 3, 0, 100, 10)]
    for _ in range(edges):
        u, v = rng.integers(0, graph_nodes, 2)
        if u == v: v = (u + 1) % graph_nodes
        cu, cv = 3 + 4 * int(u), 3 + 4 * int(v)
        ends = [((cv + 1, cu), (cu + 3, cv + 2)), ((cu + 3, cv), (cv + 3, cu)), ((cu + 1, cv + 2), (cv + 1, cu + 2)), ((cu + 1, cv), (cv + 3, cu + 2))][int(rng.integers(0, 4))]
        kind = int(rng.integers(0, 4))
        if kind == 0: cls = [(0, 100, 100000)]
        elif kind == 1: cls = [(1, 1, 10)]
        else:
            lb = int(rng.integers(0, 7))
            costs = [int(x) for x in rng.integers(-900, 900, 3)]                      # non-monotone, some negative
            cls = [(min(lb, 3), 3, costs[0]), (max(min(lb, 5) - 3, 0), 2, costs[1]), (max(lb - 5, 0), 995, costs[2])]
        for lo, up, co in cls:
            for a, b in ends: rows.append((a, b, lo, up, co))
    return n, arcs_of(rows)


def ring(seed, n, m, lower_every=7):
    """a ring 1 -> 2 -> ... -> n -> 1 of wide arcs and m - n chords with mixed costs; every lower_every-th chord has a lower bound the ring can carry back"""
    rng = np.random.default_rng(seed)
    rows = [(i, i % n + 1, 0, 1000, int(rng.integers(0, 50))) for i in range(1, n + 1)]
    for j in range(m - n):
        u, v = (int(x) for x in rng.integers(1, n + 1, 2))
        if u == v: v = u % n + 1
        lo = int(rng.integers(1, 4)) if j % lower_every == 0 else 0
        rows.append((u, v, lo, lo + int(rng.integers(0, 9)), int(rng.integers(-300, 300))))
    return n, arcs_of(rows)


def hub(degree, forced, seed=5):
    """node 1 is a hub whose list has exactly `degree` entries: degree - 1 arcs of capacity 1 to leaves with costs out of order, and the entry of the arc that
    brings `forced` units back from the sink (node 2, the same degree); leaves are 3 .. degree + 1.  forced < degree - 1: the hub's excess is smaller than what
    its admissible arcs take; in the early phases, when only the cheap arcs are admissible, it is larger"""
    rng = np.random.default_rng(seed + degree)
    d = degree - 1
    rows = [(2, 1, forced, forced, 0)]
    costs = rng.integers(-50, 2000, d)
    for i in range(d): rows.append((1, 3 + i, 0, 1, int(costs[i])))
    for i in range(d): rows.append((3 + i, 2, 0, 1, int(rng.integers(0, 30))))
    return d + 2, arcs_of(rows)


HAND = {
    # the `2 1` arc with one path
    "one_path": (4, [(2, 1, 1, 400, 0), (1, 3, 0, 100, BIG), (3, 4, 0, 100, 10), (4, 2, 0, 100, BIG)]),
    # a lower bound forces flow over the dearest arc
    "forced_dear": (3, [(1, 2, 0, 5, 1), (1, 2, 2, 5, 900), (2, 3, 0, 9, 0), (3, 1, 3, 9, 0)]),
    # a negative cycle of bounded arcs is saturated
    "negative_cycle": (3, [(1, 2, 0, 4, -5), (2, 3, 0, 7, -5), (3, 1, 0, 6, 2)]),
    # three parallel classes with costs out of order
    "parallel_classes": (2, [(1, 2, 0, 3, 40), (1, 2, 0, 2, -7), (1, 2, 0, 995, 12), (2, 1, 6, 6, 0)]),
    # arcs with upper == 0, and a node (5) without arcs
    "upper_zero": (5, [(1, 2, 0, 0, -100), (2, 1, 0, 0, -100), (1, 3, 0, 2, -3), (3, 4, 0, 2, -3), (4, 1, 0, 2, 1), (3, 1, 0, 0, -50)]),
    # costs of +-10^7 beside 0 and -1
    "wide_costs": (4, [(1, 2, 0, 3, BIG), (2, 3, 0, 3, -BIG), (3, 1, 1, 3, 0), (1, 3, 0, 2, -1), (3, 4, 0, 2, 0), (4, 1, 0, 2, -1), (2, 4, 0, 1, BIG)]),
}
# infeasible: the lower bound of 3 -> 4 is more than the 100-unit source / sink arcs can carry; and a forced arc into a node with no way out
INFEASIBLE = {
    "lower_beyond_source": (4, [(2, 1, 1, 400, 0), (1, 3, 0, 100, BIG), (3, 4, 150, 200, 10), (4, 2, 0, 100, BIG)]),
    "dead_end": (3, [(1, 2, 2, 5, 1), (2, 1, 0, 1, 0), (1, 3, 0, 4, 0)]),
}
BAD = {
    "from_is_to": (3, [(1, 1, 0, 1, 0)]),
    "node_zero": (3, [(0, 1, 0, 1, 0)]),
    "node_beyond": (3, [(1, 4, 0, 1, 0)]),
    "lower_above_upper": (3, [(1, 2, 3, 2, 0)]),
    "negative_bound": (3, [(1, 2, -1, 2, 0)]),
}


def hand(name):
    n, rows = HAND[name]; return n, arcs_of(rows)


# the generated networks whose optima tools/make_golden_flow.py records (tests/golden/flow/generated.json): name -> (function, arguments)
GENERATED = {
    "shape_s1": (reference_shape, (1, 12, 30)),
    "shape_s2": (reference_shape, (2, 60, 150)),
    "shape_s3": (reference_shape, (3, 400, 1000)),
    "ring_lds_fit": (ring, (11, 512, 1024)),                                          # just fits the single-workgroup form (512 nodes, 2048 entries)
    "ring_600": (ring, (12, 600, 1500)),                                              # active nodes in three workgroups
    "hub_63_few": (hub, (63, 20)), "hub_64_few": (hub, (64, 20)), "hub_65_few": (hub, (65, 20)), "hub_256_few": (hub, (256, 100)), "hub_257_few": (hub, (257, 100)),
    "hub_63_all": (hub, (63, 62)), "hub_64_all": (hub, (64, 63)), "hub_65_all": (hub, (65, 64)), "hub_256_all": (hub, (256, 255)), "hub_257_all": (hub, (257, 256)),
    "hub_5000_few": (hub, (5000, 1800)), "hub_5000_all": (hub, (5000, 4999)),
}


def generated(name):
    f, args = GENERATED[name]; return f(*args)
