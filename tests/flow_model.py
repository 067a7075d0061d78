"""The device min-cost-flow solver (kernels_flow.inc) restated in numpy: the same scale, epsilon sequence, phase order and list order, so that
flows, prices and the round counters of a solve are equal to the device's, number for number.  Integers only (int64, Python ints for the guards).

Method: Goldberg-Tarjan cost scaling with round-synchronous push-relabel.
  network    nodes 1..n, arcs (from, to, lower, upper, cost).  Entry 2 i is arc i forwards (residual upper - lower, cost * scale), entry 2 i + 1 backwards
             (residual 0, -cost * scale); the entries are sorted stably by tail: a node's list is its entries in ascending entry number.  excess[from] -= lower,
             excess[to] += lower.  scale = n + 1; prices start at 0.
  epsilon    cmax = max(1, scale * max|cost|); eps = cmax, then max(1, eps // ALPHA) until a refine has run at 1.
  refine     floor -= (1 + ALPHA) * scale * eps.  Every entry with residual > 0 and reduced cost < 0 is saturated.  Then rounds until one ends without an active node;
             before the first round and then every PRICE_UPDATE_PERIOD rounds of the refine a price update (price_update below), which lowers the floor by the same amount:
    push     every node with excess > 0 at the start of the phase walks its list in order and pushes min(residual, what is left of that excess) along every entry
             with residual > 0 and reduced cost < 0, prices as they stand; what a node receives is kept apart until the phase has ended.
    relabel  the received amounts are added.  A node with excess > 0 and no admissible entry gets p = max over its entries with residual > 0 of p(head) - cost - eps,
             from the prices at the start of the phase.  No such entry, or a price below the floor: the network is infeasible.
  a round that would be number max_rounds + 1: the budget is spent (LIMIT)."""
import gzip

import numpy as np

ALPHA = 8
DEFAULT_MAX_ROUNDS = 1 << 22
PRICE_UPDATE_PERIOD = 64                 # rounds of a refine between two price updates (0: none); the first comes before the first round
OK, INFEASIBLE, LIMIT, BAD_ARC, OVERFLOW = "ok", "infeasible", "limit", "bad arc", "overflow"
I64_GUARD = 1 << 62


class Result:
    def __init__(self):
        self.status = OK; self.flow = None; self.price = None; self.scale = 0
        self.phases = self.rounds = self.pushes = self.relabels = self.updates = 0; self.total_cost = 0
        self.per_refine = []                  # (eps, rounds, pushes, relabels)


def eps_sequence(cmax, alpha=ALPHA):
    out = [cmax]
    while out[-1] > 1: out.append(max(1, out[-1] // alpha))
    return out


def price_floor(n, cmax, alpha=ALPHA):
    """the lowest price a feasible network can reach (Python int, positive): the sum of (1 + alpha) * scale * eps over the phases"""
    return sum((1 + alpha) * (n + 1) * e for e in eps_sequence(cmax, alpha))


def check_arcs(n, frm, to, lower, upper):
    frm = np.asarray(frm, np.int64); to = np.asarray(to, np.int64); lower = np.asarray(lower, np.int64); upper = np.asarray(upper, np.int64)
    return not (np.any(frm < 1) or np.any(frm > n) or np.any(to < 1) or np.any(to > n) or np.any(frm == to) or np.any(lower < 0) or np.any(lower > upper))


def price_update(n, scale, alpha, eps, st, head, sis, cs, rcap, start, excess, p):
    """d(v) = the shortest distance from v to a node with excess < 0 over the entries with residual > 0, an entry's length being 0 for a negative reduced cost and
    min(cp // eps + 1, D) otherwise, D = (1 + alpha) * scale; d is cut at D (unreachable nodes: D); p(v) -= eps * d(v).  d(v) <= d(w) + length keeps every residual
    reduced cost at -eps or above.  A node with excess > 0 that reaches no deficit: the network is infeasible (False).  The distances are unique, so any
    shortest-path method gives them: here Dijkstra over the entries that point into a node, which are the sisters of its own list."""
    import heapq
    D = (1 + alpha) * scale
    cp = cs + p[st] - p[head]
    length = np.where(cp < 0, 0, np.minimum(cp // eps + 1, D))
    INF = 1 << 62
    d = [INF] * (n + 2); heap = []
    for v in np.nonzero(excess < 0)[0]: d[int(v)] = 0; heap.append((0, int(v)))
    heapq.heapify(heap)
    sl = start.tolist(); sisl = sis.tolist(); stl = st.tolist(); rl = rcap.tolist(); ll = length.tolist()
    while heap:
        dw, w = heapq.heappop(heap)
        if dw > d[w] or dw >= D: continue
        for t in range(sl[w], sl[w + 1]):
            s_ = sisl[t]                                                               # the entry v -> w
            if rl[s_] > 0:
                v = stl[s_]; c = dw + ll[s_]
                if c < d[v]: d[v] = c; heapq.heappush(heap, (c, v))
    unreach = np.array([x >= INF for x in d[:n + 2]])
    if np.any(unreach[1:n + 1] & (excess[1:n + 1] > 0)): return False
    dd = np.array([min(x, D) for x in d[:n + 2]], np.int64)
    dd[0] = 0; dd[n + 1] = 0
    p -= eps * dd
    return True


def solve(n, frm, to, lower, upper, cost, max_rounds=0, alpha=ALPHA, progress=None, period=None):
    R = Result()
    frm = np.asarray(frm, np.int64); to = np.asarray(to, np.int64); lower = np.asarray(lower, np.int64); upper = np.asarray(upper, np.int64); cost = np.asarray(cost, np.int64)
    m = len(frm); scale = n + 1; R.scale = scale
    if max_rounds <= 0: max_rounds = DEFAULT_MAX_ROUNDS
    if not check_arcs(n, frm, to, lower, upper): R.status = BAD_ARC; return R
    maxc = max((abs(int(c)) for c in (cost.min(), cost.max()))) if m else 0
    cmax = max(1, scale * maxc)
    if price_floor(n, cmax, alpha) + 2 * cmax + 1 >= I64_GUARD: R.status = OVERFLOW; return R
    tail = np.empty(2 * m, np.int64); tail[0::2] = frm; tail[1::2] = to
    order = np.argsort(tail, kind="stable")
    pos = np.empty(2 * m, np.int64); pos[order] = np.arange(2 * m)
    st = tail[order]                                                                  # tail of every sorted entry
    e = order; arc = e >> 1; back = (e & 1).astype(bool)
    head = np.where(back, frm[arc], to[arc])
    cs = np.where(back, -cost[arc], cost[arc]) * scale
    rcap = np.where(back, 0, upper[arc] - lower[arc]).astype(np.int64)
    sis = pos[e ^ 1]
    start = np.searchsorted(st, np.arange(n + 2), side="left")                      # start[v] .. start[v + 1]: the list of node v
    excess = np.zeros(n + 2, np.int64)
    np.subtract.at(excess, frm, lower); np.add.at(excess, to, lower)
    p = np.zeros(n + 2, np.int64)
    has_list = start[1:] > start[:-1]; has_list = np.append(has_list, False)          # per node v (index v)
    seg = start[:-1][has_list[:-1]]                                                   # reduceat offsets of the nodes with a list
    seg_nodes = np.nonzero(has_list)[0]
    NEG = np.int64(-(1 << 62))
    floor = 0
    if period is None: period = PRICE_UPDATE_PERIOD
    for eps in eps_sequence(cmax, alpha):
        R.phases += 1
        floor -= (1 + alpha) * scale * eps
        r0, pu0, rl0 = R.rounds, R.pushes, R.relabels
        cp = cs + p[st] - p[head]
        sat = np.nonzero((rcap > 0) & (cp < 0))[0]
        if len(sat):
            amt = rcap[sat].copy(); rcap[sat] = 0; rcap[sis[sat]] += amt
            np.subtract.at(excess, st[sat], amt); np.add.at(excess, head[sat], amt)
        since = period                                                                 # the first round of a refine follows a price update
        while True:
            if R.rounds == max_rounds: R.status = LIMIT; break
            if period and since >= period:
                since = 0
                floor -= (1 + alpha) * scale * eps
                if -floor + 2 * cmax + 1 >= I64_GUARD: R.status = OVERFLOW; break
                if not price_update(n, scale, alpha, eps, st, head, sis, cs, rcap, start, excess, p): R.status = INFEASIBLE; break
                R.updates += 1
            since += 1
            R.rounds += 1
            # ---- push
            cp = cs + p[st] - p[head]
            adm = (excess[st] > 0) & (rcap > 0) & (cp < 0)
            if adm.any():
                amt = np.where(adm, rcap, 0)
                c = np.cumsum(amt); excl = c - amt
                within = excl - excl[start[st]]                                        # admissible residual in front of the entry, in its node's list
                push = np.clip(excess[st] - within, 0, amt)
                rcap -= push
                rcap[sis] += push                                                      # (sis is a permutation)
                np.subtract.at(excess, st, push)
                delta = np.zeros(n + 2, np.int64); np.add.at(delta, head, push)
                R.pushes += int(np.count_nonzero(push))
                excess += delta
            # ---- relabel
            act = excess > 0
            nact = int(act.sum())
            if nact:
                adm = (rcap > 0) & (cp < 0)
                has = np.zeros(n + 2, bool)
                if len(seg): has[seg_nodes] = np.logical_or.reduceat(adm, seg)
                rl = act & ~has
                if rl.any():
                    cand = np.where(rcap > 0, p[head] - cs - eps, NEG)
                    best = np.full(n + 2, NEG, np.int64)
                    if len(seg): best[seg_nodes] = np.maximum.reduceat(cand, seg)
                    if np.any(best[rl] < floor): R.status = INFEASIBLE; break
                    p = np.where(rl, best, p)
                    R.relabels += int(rl.sum())
            if nact == 0: break
        R.per_refine.append((int(eps), R.rounds - r0, R.pushes - pu0, R.relabels - rl0))
        if progress: progress(R.per_refine[-1])
        if R.status != OK: return R
    # the flow of arc i: what its backward entry holds, on top of the lower bound
    R.flow = lower + rcap[pos[1::2]]
    R.price = p[1:n + 1].copy()
    R.total_cost = sum(int(f) * int(c) for f, c in zip(R.flow, cost) if f)
    return R


# ---- the certificate: bounds, conservation, 1-optimality in scaled units.  These three prove optimality: a negative residual cycle would have at most n arcs of
# reduced cost >= -1 each, so a scaled cost above -(n + 1) = -scale, while every scaled cost is a multiple of scale.
def certificate(n, frm, to, lower, upper, cost, flow, price, scale):
    frm = np.asarray(frm, np.int64); to = np.asarray(to, np.int64); lower = np.asarray(lower, np.int64); upper = np.asarray(upper, np.int64)
    cost = np.asarray(cost, np.int64); flow = np.asarray(flow, np.int64); price = np.asarray(price, np.int64)
    assert scale == n + 1 and len(flow) == len(frm) and len(price) == n
    assert np.all(flow >= lower) and np.all(flow <= upper), "a flow outside its bounds"
    bal = np.zeros(n + 1, np.int64); np.add.at(bal, to, flow); np.subtract.at(bal, frm, flow)
    assert not bal.any(), "a node is not conserved"
    p = np.concatenate([[0], price])
    cp = cost * scale + p[frm] - p[to]
    assert np.all(cp[flow < upper] >= -1), "an arc with room and reduced cost below -1"
    assert np.all(cp[flow > lower] <= 1), "an arc with flow to take back and reduced cost above 1"
    return int(sum(int(f) * int(c) for f, c in zip(flow, cost) if f))


# ---- input.cs2 / output.cs2 as the reference's solver reads and writes them
def trunc_cost(text):
    """parser_cs2.h reads the cost with %lld: the integer prefix of the text, truncation towards zero (`-0.700000` is 0)"""
    t = text.strip(); neg = t.startswith("-"); t = t.lstrip("+-")
    digits = t.split(".")[0]
    v = int(digits) if digits else 0
    return -v if neg else v


def parse_input_cs2(path):
    op = gzip.open if str(path).endswith(".gz") else open
    n = 0; fr, to, lo, up, co = [], [], [], [], []
    with op(path, "rt") as f:
        for line in f:
            w = line.split()
            if not w: continue
            if w[0] == "p": n = int(w[2])
            elif w[0] == "a":
                fr.append(int(w[1])); to.append(int(w[2])); lo.append(int(w[3])); up.append(int(w[4])); co.append(trunc_cost(w[5]))
    return n, np.array(fr, np.int64), np.array(to, np.int64), np.array(lo, np.int64), np.array(up, np.int64), np.array(co, np.int64)


def parse_output_cs2(path):
    op = gzip.open if str(path).endswith(".gz") else open
    with op(path, "rt") as f:
        v = np.array(f.read().split(), np.int64).reshape(-1, 3)
    return v


def pair_totals(frm, to, flow, only=None):
    """flow summed per (from, to), as a dict; only: a mask of the arcs that count"""
    out = {}
    for i in range(len(frm)):
        if only is not None and not only[i]: continue
        k = (int(frm[i]), int(to[i])); out[k] = out.get(k, 0) + int(flow[i])
    return out
