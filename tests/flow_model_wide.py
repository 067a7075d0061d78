"""tests/flow_model.py with prices that do not end at 64 bits: the same scale, epsilon sequence, phase order, list order and price updates, so that on a network
the 64-bit model admits every flow, price and counter is equal, and beyond it the numbers are those of the device's 128-bit kernels (kernels_flow.inc with
P = __int128).  Prices, scaled and reduced costs, epsilon and the floor are Python integers (object arrays); excesses, residuals and distances
stay int64, as on the device.  The guard is the device's: the lowest price the phases can reach, with room for one reduced cost, inside +-2^126.

Reduced costs are only worked out where a decision reads them (the entries of nodes with excess > 0): object arrays are slow, the numbers are the same."""
import heapq

import numpy as np

from flow_model import ALPHA, DEFAULT_MAX_ROUNDS, PRICE_UPDATE_PERIOD, OK, INFEASIBLE, LIMIT, BAD_ARC, OVERFLOW, Result, check_arcs, eps_sequence, price_floor

WIDE_GUARD = 1 << 126


def guard(n, maxc, alpha=ALPHA):
    """whether n nodes with that largest |cost| are admitted (Python integers: nothing to wrap)"""
    cmax = max(1, (n + 1) * int(maxc))
    return price_floor(n, cmax, alpha) + 2 * cmax + 1 < WIDE_GUARD


def obj(a):
    out = np.empty(len(a), object); out[:] = [int(x) for x in a]; return out


def price_update(n, scale, alpha, eps, st, sis, cs, rcap, start, excess, p, head):
    """flow_model.price_update in Python integers: an entry's length is 0 for a negative reduced cost and min(cp // eps + 1, D) otherwise"""
    D = (1 + alpha) * scale
    cp = (cs + p[st] - p[head]).tolist()
    ll = [0 if c < 0 else min(c // eps + 1, D) for c in cp]
    INF = 1 << 62
    d = [INF] * (n + 2); heap = []
    for v in np.nonzero(excess < 0)[0]: d[int(v)] = 0; heap.append((0, int(v)))
    heapq.heapify(heap)
    sl = start.tolist(); sisl = sis.tolist(); stl = st.tolist(); rl = rcap.tolist()
    while heap:
        dw, w = heapq.heappop(heap)
        if dw > d[w] or dw >= D: continue
        for t in range(sl[w], sl[w + 1]):
            s_ = sisl[t]                                                               # the entry v -> w
            if rl[s_] > 0:
                v = stl[s_]; c = dw + ll[s_]
                if c < d[v]: d[v] = c; heapq.heappush(heap, (c, v))
    ex = excess.tolist()
    if any(d[v] >= INF and ex[v] > 0 for v in range(1, n + 1)): return False
    for v in range(1, n + 1): p[v] -= eps * min(d[v], D)
    return True


def solve(n, frm, to, lower, upper, cost, max_rounds=0, alpha=ALPHA, period=None):
    """cost: any sequence of Python integers"""
    R = Result()
    frm = np.asarray(frm, np.int64); to = np.asarray(to, np.int64); lower = np.asarray(lower, np.int64); upper = np.asarray(upper, np.int64)
    cost = [int(c) for c in cost]
    m = len(frm); scale = n + 1; R.scale = scale
    if max_rounds <= 0: max_rounds = DEFAULT_MAX_ROUNDS
    if not check_arcs(n, frm, to, lower, upper): R.status = BAD_ARC; return R
    maxc = max((abs(c) for c in cost), default=0)
    cmax = max(1, scale * maxc)
    if not guard(n, maxc, alpha): R.status = OVERFLOW; return R
    tail = np.empty(2 * m, np.int64); tail[0::2] = frm; tail[1::2] = to
    order = np.argsort(tail, kind="stable")
    pos = np.empty(2 * m, np.int64); pos[order] = np.arange(2 * m)
    st = tail[order]
    e = order; arc = e >> 1; back = (e & 1).astype(bool)
    head = np.where(back, frm[arc], to[arc])
    cs = obj([(-cost[a] if b else cost[a]) * scale for a, b in zip(arc.tolist(), back.tolist())])
    rcap = np.where(back, 0, upper[arc] - lower[arc]).astype(np.int64)
    sis = pos[e ^ 1]
    start = np.searchsorted(st, np.arange(n + 2), side="left")
    excess = np.zeros(n + 2, np.int64)
    np.subtract.at(excess, frm, lower); np.add.at(excess, to, lower)
    p = obj([0] * (n + 2))
    NEG = -WIDE_GUARD
    floor = 0
    if period is None: period = PRICE_UPDATE_PERIOD
    for eps in eps_sequence(cmax, alpha):
        R.phases += 1
        floor -= (1 + alpha) * scale * eps
        r0, pu0, rl0 = R.rounds, R.pushes, R.relabels
        res = np.nonzero(rcap > 0)[0]
        if len(res):
            sat = res[(cs[res] + p[st[res]] - p[head[res]]) < 0]
            if len(sat):
                amt = rcap[sat].copy(); rcap[sat] = 0; rcap[sis[sat]] += amt
                np.subtract.at(excess, st[sat], amt); np.add.at(excess, head[sat], amt)
        since = period
        while True:
            if R.rounds == max_rounds: R.status = LIMIT; break
            if period and since >= period:
                since = 0
                floor -= (1 + alpha) * scale * eps
                if -floor + 2 * cmax + 1 >= WIDE_GUARD: R.status = OVERFLOW; break
                if not price_update(n, scale, alpha, eps, st, sis, cs, rcap, start, excess, p, head): R.status = INFEASIBLE; break
                R.updates += 1
            since += 1
            R.rounds += 1
            # ---- push: the entries with residual of the nodes with excess
            idx = np.nonzero((excess[st] > 0) & (rcap > 0))[0]
            if len(idx): idx = idx[(cs[idx] + p[st[idx]] - p[head[idx]]) < 0]
            if len(idx):
                amt = np.zeros(2 * m, np.int64); amt[idx] = rcap[idx]
                c = np.cumsum(amt); excl = c - amt
                within = excl - excl[start[st]]
                push = np.clip(excess[st] - within, 0, amt)
                rcap -= push
                rcap[sis] += push
                np.subtract.at(excess, st, push)
                delta = np.zeros(n + 2, np.int64); np.add.at(delta, head, push)
                R.pushes += int(np.count_nonzero(push))
                excess += delta
            # ---- relabel, from the same prices
            act = excess > 0
            nact = int(act.sum())
            if nact:
                idx = np.nonzero(act[st] & (rcap > 0))[0]
                has = np.zeros(n + 2, bool)
                if len(idx): has[st[idx[(cs[idx] + p[st[idx]] - p[head[idx]]) < 0]]] = True
                rl = act & ~has
                if rl.any():
                    best = {int(v): NEG for v in np.nonzero(rl)[0]}
                    idx = idx[rl[st[idx]]]
                    for v, x in zip(st[idx].tolist(), (p[head[idx]] - cs[idx] - eps).tolist()):
                        if x > best[v]: best[v] = x
                    if any(x < floor for x in best.values()): R.status = INFEASIBLE; break
                    for v, x in best.items(): p[v] = x
                    R.relabels += len(best)
            if nact == 0: break
        R.per_refine.append((int(eps), R.rounds - r0, R.pushes - pu0, R.relabels - rl0))
        if R.status != OK: return R
    R.flow = lower + rcap[pos[1::2]]
    R.price = [int(x) for x in p[1:n + 1]]
    R.total_cost = sum(int(f) * c for f, c in zip(R.flow.tolist(), cost) if f)
    return R


def certificate(n, frm, to, lower, upper, cost, flow, price, scale):
    """flow_model.certificate in Python integers; returns the cost of the flow"""
    frm = [int(x) for x in frm]; to = [int(x) for x in to]; lower = [int(x) for x in lower]; upper = [int(x) for x in upper]
    cost = [int(x) for x in cost]; flow = [int(x) for x in flow]; p = [0] + [int(x) for x in price]
    assert scale == n + 1 and len(flow) == len(frm) and len(p) == n + 1
    bal = [0] * (n + 1)
    for i in range(len(frm)):
        assert lower[i] <= flow[i] <= upper[i], "a flow outside its bounds"
        bal[to[i]] += flow[i]; bal[frm[i]] -= flow[i]
        cp = cost[i] * scale + p[frm[i]] - p[to[i]]
        if flow[i] < upper[i]: assert cp >= -1, "an arc with room and reduced cost below -1"
        if flow[i] > lower[i]: assert cp <= 1, "an arc with flow to take back and reduced cost above 1"
    assert not any(bal), "a node is not conserved"
    return sum(f * c for f, c in zip(flow, cost) if f)
