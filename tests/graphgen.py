"""Synthetic overlap graphs for the step-4 tests: chains between branching nodes (parallel ones, closed ones, tips), cycles, two-cycles,
nodes whose two edges do not combine, multi-edges -- with the ids scattered at random, since the reference's sweeps are id-ordered.
Edges come out as graph3 holds them: from < to, one per (from, to, type), ascending; reads all have one length, so the twin's
lengthOfEdge equals the edge's (overlapGraph.cpp:147-150)."""
import numpy as np

EDGE_DTYPE = np.dtype([("from", "<u8"), ("to", "<u8"), ("length", "<u4"), ("length_twin", "<u4"), ("type", "u1"), ("pad", "u1", (7,))])


def _rev(t):
    return {0: 3, 3: 0, 1: 1, 2: 2}[t]


def random_graph(seed, n_anchor=30, n_paths=60, max_len=12, n_cycles=3, p_bad=0.03, len_hi=25):
    rng = np.random.default_rng(seed)
    nodes = 0
    def new():
        nonlocal nodes
        nodes += 1; return nodes
    anchors = [new() for _ in range(n_anchor)]
    raw = []                                           # (x, y, ox, oy, len): x -> y leaving x with orientation ox, entering y with oy
    def path(seq, closed=False):
        o = {v: int(rng.integers(0, 2)) for v in seq}
        pairs = list(zip(seq[:-1], seq[1:])) + ([(seq[-1], seq[0])] if closed else [])
        for j, (x, y) in enumerate(pairs):
            ox = o[x] if (j > 0 or closed) else int(rng.integers(0, 2))         # path ends join their node in any orientation
            oy = o[y] if (j < len(pairs) - 1 or closed) else int(rng.integers(0, 2))
            if rng.random() < p_bad: oy ^= 1
            raw.append((x, y, ox, oy, int(rng.integers(1, len_hi))))
    for _ in range(n_paths):
        kind = rng.random()
        u = anchors[int(rng.integers(0, n_anchor))]
        v = u if kind < 0.12 else anchors[int(rng.integers(0, n_anchor))]
        if kind > 0.85: v = new()                      # a tip
        m = int(rng.integers(0, max_len + 1))
        if u == v and m < 2: m = 2
        path([u] + [new() for _ in range(m)] + [v])
    for _ in range(n_cycles):
        m = int(rng.integers(2, max_len + 3))
        path([new() for _ in range(m)], closed=True)
    N = nodes
    perm = rng.permutation(N) + 1                      # scatter the ids
    seen, out = set(), []
    for x, y, ox, oy, ln in raw:
        a, b = int(perm[x - 1]), int(perm[y - 1])
        if a == b: continue
        t = (ox << 1) | oy
        if a > b: a, b, t = b, a, _rev(t)
        if (a, b, t) in seen: continue
        seen.add((a, b, t)); out.append((a, b, t, ln))
    out.sort()
    e = np.zeros(len(out), dtype=EDGE_DTYPE)
    for i, (a, b, t, ln) in enumerate(out):
        e[i]["from"], e[i]["to"], e[i]["type"], e[i]["length"], e[i]["length_twin"] = a, b, t, ln, ln
    return N, e


def write_graph3(path, N, e, read_len=100):
    with open(path, "w") as f:
        f.write(f"0\n{N}\n{read_len}\n")
        for r in e:
            f.write(f"{r['from']}\t{r['to']}\t{r['type']}\t1\t{r['length']}\t0\t0\n\n")
            f.write(f"{r['to']}\t{r['from']}\t{_rev(int(r['type']))}\t1\t{r['length_twin']}\t0\t0\n\n")


def write_reads(path, N, read_len=100, seed=0):
    """a .reads file with N distinct reads (readLoader.cpp:29-36: frequency, length, forward, reverse complement)"""
    rng = np.random.default_rng(seed + 12345)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    seqs = set()
    while len(seqs) < N:
        seqs.add("".join(rng.choice(list("ACGT"), size=read_len)))
    with open(path, "w") as f:
        f.write(f"{N}\n")
        for s in sorted(seqs):
            f.write(f"1\t{read_len}\t{s}\t{''.join(comp[c] for c in reversed(s))}\n")


# ---- directed families: small graphs built to reach the branches of removeDeadEnds and removeBubbles that random_graph hardly reaches.
# An instance is a few nodes with local ids 1..n whose RELATIVE order is part of the design (the sweeps are id-ordered); compose() lays
# instances out over one id space (in sequence, or interleaved so that neighbours in id belong to different instances) and never changes
# the order inside an instance.  All paths are forward-forward (type 3); an instance may be mirrored as a whole (reverse complement: types
# 3 <-> 0 and 1 <-> 2, the two lengths of every pair swapped), which swaps "in" and "out" everywhere and changes no decision.
# An anchor is a node with a two-cycle partner: the first contractCompositePaths turns the partner into a loop a -> a (one read, one "in" and
# one "out" half), after which the node is never contracted (three or more list entries), never a dead end and never a bubble candidate.
# `built` says how often an instance is designed to take a branch -- the floors of tests/test_step4_oracle.py; `keep` / `gone` name nodes that
# must (not) be an end of a surviving edge.  The sweeps run: dead(0) bubbles(10) contract, then per loop iteration r = 1, 2, ...
# dead(min(r-1, 3)) bubbles(min(10r, 50)) contract, until an iteration changes nothing.
TIERS = (10, 20, 30, 40, 50)


def _split(total, n):
    assert total >= n
    out = [total // n] * n; out[-1] += total - (total // n) * n
    return out


class _Inst:
    def __init__(self):
        self.n = 0; self.rows = []; self.built = {}; self.keep = []; self.gone = []; self.fixed = False
    def new(self):
        self.n += 1; return self.n
    def news(self, k):
        return [self.new() for _ in range(k)]
    def edge(self, x, y, ln, ln_t=None, t=3):
        self.rows.append((x, y, t, ln, ln if ln_t is None else ln_t))
    def path(self, seq, total, total_t=None, last_t=3):
        n = len(seq) - 1; f = _split(total, n); b = _split(total if total_t is None else total_t, n)
        for j in range(n):
            self.edge(seq[j], seq[j + 1], f[j], b[j], last_t if j == n - 1 else 3)
    def anchor(self):
        a, p = self.new(), self.new(); self.edge(a, p, 7, 5); self.edge(p, a, 11, 13); return a
    def add(self, **kw):
        for k, v in kw.items(): self.built[k] = self.built.get(k, 0) + v


def _bubble(I, m, k, low, d_c, d_i, tw_c=None, tw_i=None, a=None, b=None):
    """a -> chain of m -> b beside a -> k nodes -> b.  The side named by `low` ("chain" or "iside") gets the lower ids, contracts first and
    becomes the edge a -> b carrying all its nodes; the other side contracts down to its highest id (its neighbours a and b are adjacent by
    then), which is the bubble's node i with n1 = its side's node count.  Returns (i, n1, n2)."""
    if low == "chain": chain = I.news(m); iside = I.news(k)
    else: iside = I.news(k); chain = I.news(m)
    a = a or I.anchor(); b = b or I.anchor()
    I.path([a] + chain + [b], d_c, tw_c); I.path([a] + iside + [b], d_i, tw_i)
    return (max(iside), k, m) if low == "chain" else (max(chain), m, k)


def _judge(I, i, n1, n2, diff):
    """book the designed outcome of one bubble whose two lengths differ by `diff`"""
    tier = next((c for c in TIERS if diff < c), None)
    I.add(cand=1)
    if tier is None: I.add(far=1); I.keep.append(i)
    elif n1 < n2 // 2: I.add(dec1=1, **{f"dec1_{tier}": 1}); I.gone.append(i)
    elif n2 < n1 // 2: I.add(dec2=1, **{f"dec2_{tier}": 1}); I.gone.append(i)
    else: I.add(undecided=1); I.keep.append(i)
    if tier is not None and tier > 10: I.add(far=1)


def _spine(I, n, descending):
    """s1 -> s2 -> ... -> sn, every node with a second "out" edge, s1 without an "in" edge: s1 is a dead end, and s(j+1) is one once sj is gone.
    Ascending ids: one sweep takes all n (n rounds of the device's fixed point); the second edge goes to a leaf of higher id, which is alone
    by the time it is visited.  Descending ids: one node per sweep, so n sweeps in n consecutive loop iterations; here the second edge goes to an
    anchored hub, because a true leaf of sj would be visited (and removed as a dead end itself) while sj still stands."""
    if descending:
        s = I.news(n)[::-1]; hub = I.anchor()
        for x in s: I.edge(x, hub, 9, 8)
        I.edge(s[-1], hub, 6, 4, t=2)
        for j in range(n): I.add(**{f"dead{min(max(j - 1, 0), 3)}": 1})
    else:
        s = I.news(n); leaves = I.news(n); end = I.anchor()
        for x, l in zip(s, leaves): I.edge(x, l, 9, 8)
        I.edge(s[-1], end, 6, 4)
        I.add(dead0=n); I.gone += leaves
    for x, y in zip(s[:-1], s[1:]): I.edge(x, y, 12, 14)
    I.gone += s; I.keep.append(hub if descending else end)


def _fam_b(twins=False, ms=range(1, 8), ks=range(1, 5)):
    """B1 / B2: both sides of n1 < n2/2 and n2 < n1/2 with n1, n2 in 1..7 (odd and even halves), lengths within 10 of each other; every
    shape in both id arrangements, so that the same counts meet as (n1, n2) and as (n2, n1).  twins: the other half of every pair is 75
    longer on the chain side, which puts a bubble judged from the wrong halves out of every tier."""
    out = []
    for m in ms:
        for k in ks:
            for low in ("chain", "iside"):
                I = _Inst(); diff = (3 * m + 5 * k) % 10; d_c = 120; d_i = d_c + (diff if (m + k) % 2 else -diff)
                i, n1, n2 = _bubble(I, m, k, low, d_c, d_i, d_c + 75 if twins else None, d_i if twins else None)
                _judge(I, i, n1, n2, diff); out.append(I)
    return out


def _keeper(n=2):
    I = _Inst(); _spine(I, n, True); return I


def _fam_bl(twins=False):
    """BL: one bubble per length difference 0, 9, 10, 19, ..., 49, 50, 51 and per side (n1, n2 = 1, 4 and 4, 1), on a row of anchors that
    neighbouring bubbles share.  A tier goes in the first sweep whose closeLength admits it: 0 and 9 before the loop, 10 and 19 in
    iteration 2, ..., 40 and 49 in iteration 5; 50 and 51 stay.  Iteration 1 (closeLength 10 again) is kept alive by a descending two-node
    spine, each later one by the tier before it.  twins: the other halves differ by 75 more (tiers below 50: out of reach when judged from
    the wrong halves) or by 45 less (tiers 50 and 51: within 10)."""
    I = _Inst(); diffs = [0, 9, 10, 19, 20, 29, 30, 39, 40, 49, 50, 51]
    for low in ("chain", "iside"):
        # ids: the low sides of all bubbles first, then the high sides, then the anchors
        lows = [I.news(4 if low == "chain" else 1) for _ in diffs]; highs = [I.news(1 if low == "chain" else 4) for _ in diffs]
        anchors = [I.anchor() for _ in range(len(diffs) + 1)]
        for j, diff in enumerate(diffs):
            d_c = 150; d_i = d_c - diff if j % 2 else d_c + diff
            tw_c = (d_c + 75 if diff < 50 else d_i + 5) if twins else None
            chain, iside = (lows[j], highs[j]) if low == "chain" else (highs[j], lows[j])
            I.path([anchors[j]] + chain + [anchors[j + 1]], d_c, tw_c); I.path([anchors[j]] + iside + [anchors[j + 1]], d_i, d_i if twins else None)
            _judge(I, max(highs[j]), len(highs[j]), len(lows[j]), diff)
    return [I, _keeper()]


def _fam_bm():
    """BM: two or three edges a -> b of different types (simple ones: a contraction never adds an edge between adjacent nodes, so parallel
    edges all come from the input and carry no reads) that differ in length, beside a two-node side (n1 = 2 > 2 * 0).  The list is walked
    newest first, which is type 3, 2, 1 for a < b and type 2, 1, 3 for a > b.  (1) first seen far, second close: nothing goes.  (2) first seen
    close, second far: the first goes, the node stays.  (3) two sides i < i' between the same anchors: both choose the first edge; it is i's,
    and i' falls through to the second in the same sweep; the third edge is far and keeps both."""
    out = []                                                   # (never mirrored: that would change which type is seen first)
    I = _Inst(); x = I.news(2); a = I.anchor(); b = I.anchor()
    I.path([a] + x + [b], 90); I.edge(a, b, 150, 150, t=3); I.edge(a, b, 90, 90, t=2)
    I.add(cand=1, multi=1, far=1); I.keep.append(max(x)); out.append(I)
    I = _Inst(); x = I.news(2); b = I.anchor(); a = I.anchor()
    I.path([a] + x + [b], 90); I.edge(a, b, 150, 150, t=3); I.edge(a, b, 88, 88, t=2)
    I.add(cand=2, multi=1, far=1, dec2=1, dec2_10=1); I.keep.append(max(x)); out.append(I)
    I = _Inst(); x = I.news(2); y = I.news(2); a = I.anchor(); b = I.anchor()
    I.path([a] + x + [b], 90); I.path([a] + y + [b], 94); I.edge(a, b, 92, 92, t=3); I.edge(a, b, 96, 96, t=2); I.edge(a, b, 30, 30, t=1)
    I.add(cand=2, multi=2, dec2=2, dec2_10=2, far=1); I.keep += [max(x), max(y)]; out.append(I)
    for I in out: I.fixed = True
    return out


def _fam_bc(depth=4):
    """BC: i1, i2, ... where i(j+1) has one "in" and one "out" edge only after ij took its own two edges away (a -> ij -> i(j+1), beside
    a heavy edge a -> i(j+1) that is i(j+1)'s remaining "in").  That heavy edge counts into n1 of i(j+1), whose own decision then needs an
    edge a -> i(j+2) of more than twice as many reads: the read counts grow as 4, 12, 28, 60, so the depth is logarithmic in the size.
    (A bubble node has exactly two edges when it decides, and the edge a -> b it is judged against lies between its two neighbours; removing
    that edge leaves both neighbours their path edge, so only the "own edges" side can hand a candidate on, and it always hands on the heavy
    edge.)  Ascending ids: the whole cascade in one sweep; descending: one node per sweep."""
    out = []
    for descending in (False, True):
        I = _Inst(); heavy = []; r = 4
        for _ in range(depth): heavy.append(I.news(r)); r = 2 * (1 + r) + 2
        i = I.news(depth + 1)                                   # the last one is the far end, anchored below by two more edges
        if descending: i = i[:-1][::-1] + i[-1:]
        a = I.anchor(); end = I.anchor()
        I.edge(a, i[0], 30, 31); ln = 0
        for j in range(depth):
            I.edge(i[j], i[j + 1], 30, 33); ln = ln + 30 + (30 if j == 0 else 0) + (1 if j < 2 else 2)
            I.path([a] + heavy[j] + [i[j + 1]], ln, ln + 40)
            cl = TIERS[max(j - 1, 0)] if descending else 10
            I.add(cand=1, dec1=1, **{f"dec1_{cl}": 1})
        I.edge(i[depth], end, 20, 22); I.edge(i[depth], end, 24, 26, t=2)
        I.gone += i[:-1]; I.keep.append(i[depth]); out.append(I)
    return out


def _fam_d():
    """D: tips whose one edge carries 0, 1, 2, 3, 4 reads (a chain of that many nodes, contracted first), "in" tips and "out" tips: they go
    at thresholds 0, 1, 2, 3 -- before the loop and in iterations 2, 3, 4 (a descending two-node spine keeps iteration 1 alive) -- and the
    four-read tip never.  Beside each, a node whose edge is one read heavier and that has two edges of the other direction: never a dead end.
    Two nodes with a loop whose two halves are both "in" (a two-cycle of types 1 and 3, contracted): one with one more "in" edge, one with
    two; only the loop test keeps them once the threshold reaches the loop's one read."""
    I = _Inst()
    chains = {(k, d): I.news(k) for k in range(5) for d in "io"}; chains2 = {k: I.news(k + 1) for k in range(4)}
    hub, hub2 = I.anchor(), I.anchor()
    for (k, d), c in chains.items():
        t = I.new(); seq = [hub] + c + [t]
        I.path(seq if d == "i" else seq[::-1], 20 * (k + 1), 21 * (k + 1))
        if k < 4: I.gone.append(t); I.add(**{f"dead{k}": 1})
        else: I.keep.append(t)
        if 1 <= k <= 3: I.add(reads_keep=1)
    for k, c in chains2.items():
        t = I.new(); I.path([hub] + c + [t], 20 * (k + 2)); I.edge(t, hub2, 15, 16); I.edge(t, hub2, 17, 18, t=2); I.keep.append(t); I.add(reads_keep=int(k + 1 <= 3))
    for n_in in (1, 2):
        u, q = I.new(), I.new(); I.edge(u, q, 9, 10, t=1); I.edge(q, u, 11, 12)
        I.edge(hub, u, 14, 15)
        if n_in == 2: I.edge(hub2, u, 16, 17)
        I.keep.append(u); I.add(loop_keep=1, reads_keep=1)
    return [I, _keeper()]


def _fam_dc(n=300):
    out = []
    for descending in (False, True):
        I = _Inst(); _spine(I, n, descending); out.append(I)
    return out


FAMILIES = {
    "B": _fam_b, "BL": _fam_bl, "BM": _fam_bm, "BC": _fam_bc, "D": _fam_d, "DC": _fam_dc,
    "TB": lambda: _fam_b(twins=True, ms=(3, 4, 5), ks=(1, 2)), "TL": lambda: _fam_bl(twins=True),
}
COUNTERS = ["dead0", "dead1", "dead2", "dead3", "loop_keep", "reads_keep", "cand", "multi", "dec1", "dec2"] + [f"dec1_{c}" for c in TIERS] + [f"dec2_{c}" for c in TIERS] + ["undecided", "far"]


class Layout:
    """what compose() made: the graph, the summed `built` counts and the global ids of the keep / gone nodes"""
    def __init__(self, instances, seed, interleave):
        rng = np.random.default_rng(seed)
        order = rng.permutation(len(instances)); instances = [instances[int(x)] for x in order]
        owner = np.repeat(np.arange(len(instances)), [I.n for I in instances])
        if interleave: rng.shuffle(owner)
        self.N = int(len(owner)); self.built = {}; self.keep = []; self.gone = []
        seen, rows = set(), []
        for x, I in enumerate(instances):
            ids = np.flatnonzero(owner == x) + 1 if interleave else None      # ascending: the order inside the instance stays
            base = int(np.searchsorted(owner, x)) if not interleave else 0
            g = (lambda v: int(ids[v - 1])) if interleave else (lambda v: base + v)
            mirror = bool(rng.integers(0, 2)) and not I.fixed
            for a, b, t, ln, lt in I.rows:
                a, b = g(a), g(b)
                if mirror: t, ln, lt = 3 - t, lt, ln
                if a > b: a, b, t, ln, lt = b, a, _rev(t), lt, ln
                assert a != b and (a, b, t) not in seen
                seen.add((a, b, t)); rows.append((a, b, t, ln, lt))
            for k, v in I.built.items(): self.built[k] = self.built.get(k, 0) + v
            self.keep += [g(v) for v in I.keep]; self.gone += [g(v) for v in I.gone]
        rows.sort()
        self.edges = np.zeros(len(rows), dtype=EDGE_DTYPE)
        for c, name in enumerate(("from", "to", "type", "length", "length_twin")):
            self.edges[name] = [r[c] for r in rows]


def layout(names, seed, copies=1, interleave=True, **sizes):
    """the instances of the named families (`copies` times each), laid out by `seed`; sizes: depth for BC, n for DC"""
    inst = []
    for _ in range(copies):
        for name in names:
            kw = {"depth": sizes["depth"]} if name == "BC" and "depth" in sizes else {"n": sizes["n"]} if name == "DC" and "n" in sizes else {}
            inst += FAMILIES[name](**kw)
    return Layout(inst, seed, interleave)


def compose(names, seed, copies=1, interleave=True, **sizes):
    L = layout(names, seed, copies, interleave, **sizes); return L.N, L.edges


def family(name, seed):
    """one family on its own, instances in sequence: (N, edges) like random_graph"""
    return compose([name], seed, interleave=False)


def composed_layout(seed=1, copies=60):
    """every family, DC and BC at reduced sizes, `copies` times over interleaved ids (about 2 000 nodes per copy)"""
    return layout(list(FAMILIES), seed, copies, True, depth=3, n=12)
