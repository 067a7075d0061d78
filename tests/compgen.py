"""A seeded generator of composite graphs and of mates on them, for the tests of the step 6/7 device sweeps (tests/test_compgen_host.py, test_compgen_reference.py,
test_gpu_compgen.py).  The golden P.graph4 files are step-4 output of clean reads: every read lies on exactly one record pair and exactly once on its edge.  The
graphs made here have what graph5 / graph6 files have and those lack -- reads on many pairs, reads twice on an edge, hubs, loops, flows -- with a knob for each.
Pure Python and numpy: records come from H.rec / H.twin_of and text from H.graph_text, so the parser, the writer and the restatements stay the single source."""
import numpy as np
import test_mate_estimate_host as H

MAX_DIST = 2047                       # the loader refuses larger distances


def _chain_for_length(rng, n, length, max_dist):
    """n + 1 distances in [1, max_dist] that add up to `length`"""
    d = np.full(n + 1, length // (n + 1), dtype=np.int64); d[:length % (n + 1)] += 1
    assert d.min() >= 1 and d.max() <= max_dist, (n, length)
    for _ in range(4 * (n + 1)):
        i, j = (int(v) for v in rng.integers(0, n + 1, size=2))
        if i != j:
            x = int(rng.integers(0, min(d[i] - 1, max_dist - d[j]) + 1)); d[i] -= x; d[j] += x
    return d.tolist()


def composite_graph(seed, pairs, n_reads=None, node_share=0.6, hubs=1, list_len=(0, 6), empty_share=0.15, loops_once=1, loops_twice=1, dense_edges=2,
                    flows=(0.0, 0.5, 1.0, 2.0), dist=(1, 120), far_share=0.04, max_dist=MAX_DIST, read_copies=(), twice_on_edge=0.0, inconsistent_share=0.0,
                    lengths=None, simple_len=(20, 400), use_reads=(), arl=60):
    """-> (N, header, records): `pairs` record pairs (record, twin; a loop written twice: record, twin, twin, record) over reads 1 .. N.
    node_share   nodes per record pair; a node carries at most 8 half-edges; two nodes are joined by at most one pair (so (from, to, type, length) names a half)
    hubs         nodes that get four in-halves (types 0, 1) and four out-halves (types 2, 3) first
    list_len     (lowest, highest) number of entries of a list, uniform; empty_share: the share of simple edges (no list) on top of that
    loops_once / loops_twice   loops, written as one record pair or as the writer leaves them (pair, then mirror image)
    dense_edges  pairs whose lists have 6 .. 10 entries 1 .. 3 bases apart: a library of mates on them has an upper bound the sweeps skip
    flows        the flow of a pair (record and twin carry the same) is drawn from these
    dist         (lowest, highest) distPrevious / distNext, uniform; with probability far_share a distance is drawn from (highest, max_dist] instead
    read_copies  multiplicities to realise: an entry m (or (m, start)) is one more read that lies on m pairs, those at [start, start + m) of one seeded order
                 of the list-bearing pairs -- two such reads share the pairs where their ranges overlap
    twice_on_edge   the share of (read, pair) placements that stand a second time on that edge
    inconsistent_share   the share of list edges whose length is NOT sum(distPrevious) + last distNext (off by -7 .. 7)
    lengths      {pair index: length of the edge}: the list is made to add up to it (more entries where 2047 a step would not reach); without entries: a simple edge
    use_reads    read ids that must stand on a list (never nodes): the first reads handed out
    Orientations 0 and 1 and all four edge types are drawn uniformly; a record leaves the larger id as often as the smaller.  distNext of an entry is distPrevious
    of the next, as the pipeline leaves them, so the twin's list adds up to the same length."""
    rng = np.random.default_rng(seed); lengths = dict(lengths or {})
    n_loops = loops_once + loops_twice
    assert pairs >= n_loops + dense_edges + 8 * hubs
    kind = ["loop1"] * loops_once + ["loop2"] * loops_twice + ["dense"] * dense_edges
    kind += ["plain"] * (pairs - len(kind))
    kind = [kind[i] for i in rng.permutation(pairs)] if pairs > 1 else kind
    # ---- how many entries each list gets
    n_of = []
    for j in range(pairs):
        if kind[j] == "dense":
            n = int(rng.integers(6, 11))
        else:
            n = 0 if rng.random() < empty_share else int(rng.integers(list_len[0], list_len[1] + 1))
        if j in lengths and kind[j] != "dense":
            L = lengths[j]; n = min(max(n, -(-L // 1800) - 1), L - 1)
        n_of.append(n)
    copies = [(c, None) if isinstance(c, (int, np.integer)) else tuple(c) for c in read_copies]
    bearing = [j for j in range(pairs) if kind[j] != "dense" and j not in lengths]
    order = [bearing[i] for i in rng.permutation(len(bearing))] if bearing else []
    n_nodes = max(2 + 8 * hubs, int(pairs * node_share) + 1)
    needed = sum(n_of) + len(copies)
    N = n_reads if n_reads is not None else n_nodes + needed + needed // 10 + 8
    forced = [int(r) for r in use_reads]; assert all(1 <= r <= N for r in forced) and len(set(forced)) == len(forced)
    free = np.setdiff1d(np.arange(1, N + 1), np.asarray(forced, dtype=np.int64)); free = free[rng.permutation(len(free))]
    assert len(free) >= n_nodes + needed - len(forced), "too few reads for this graph"
    nodes = sorted(int(v) for v in free[:n_nodes]); pool = iter(forced + [int(v) for v in free[n_nodes:]])
    # ---- ends and types
    deg = {v: 0 for v in nodes}; joined = set(); ends = [None] * pairs
    plain = [j for j in range(pairs) if not kind[j].startswith("loop")]; at = 0
    for h in range(hubs):
        hub = nodes[int(rng.integers(0, len(nodes)))]
        while deg[hub]:
            hub = nodes[int(rng.integers(0, len(nodes)))]
        for typ in (0, 1, 0, 1, 2, 3, 2, 3):
            x = hub
            while x == hub or (min(x, hub), max(x, hub)) in joined or deg[x] >= 7:
                x = nodes[int(rng.integers(0, len(nodes)))]
            joined.add((min(x, hub), max(x, hub))); deg[hub] += 1; deg[x] += 1
            ends[plain[at]] = (hub, x, typ) if rng.integers(0, 2) else (x, hub, H.flip_type(typ)); at += 1
    for j in range(pairs):
        if ends[j] is not None:
            continue
        while True:
            u = nodes[int(rng.integers(0, len(nodes)))]; v = u if kind[j].startswith("loop") else nodes[int(rng.integers(0, len(nodes)))]
            if u == v and not kind[j].startswith("loop"):
                continue
            if (deg[u] + 2 > 8) if u == v else (deg[u] >= 8 or deg[v] >= 8 or (min(u, v), max(u, v)) in joined):
                continue
            break
        joined.add((min(u, v), max(u, v))); deg[u] += 1; deg[v] += 1
        # A loop written once gets type 0 or 3 only.  The rows of the reference's link sweep name a half by (from, to, type, length); the two halves of a loop of
        # type 1 or 2 carry one name, so its rows cannot be told apart (test_links_reference.reference_rows refuses them).  A loop written twice is two edges to the
        # reference's loader: its reads lie on two pairs, give no row there, and any type is safe -- the device, which folds the two writings, gets types 1 and 2 here.
        ends[j] = (u, v, int(rng.integers(0, 4)) if kind[j] != "loop1" else 3 * int(rng.integers(0, 2)))
    # ---- reads on lists: fresh ones, then the reads on many pairs, then the second standings
    reads_on = [[next(pool) for _ in range(n_of[j])] for j in range(pairs)]
    for m, start in copies:
        assert m <= len(order), "more copies than list-bearing pairs"
        r = next(pool); s = int(rng.integers(0, len(order))) if start is None else start
        for i in range(m):
            lst = reads_on[order[(s + i) % len(order)]]; lst.insert(int(rng.integers(0, len(lst) + 1)), r)
    for j in range(pairs):
        if j in lengths:
            continue
        for r in sorted(set(reads_on[j])):
            if rng.random() < twice_on_edge:
                reads_on[j].insert(int(rng.integers(0, len(reads_on[j]) + 1)), r)
    # ---- distances, lengths, records
    def draw():
        if rng.random() < far_share and dist[1] < max_dist:
            return max_dist if rng.integers(0, 8) == 0 else int(rng.integers(dist[1] + 1, max_dist + 1))      # (the limit itself, one time in eight)
        return int(rng.integers(dist[0], dist[1] + 1))
    records = []
    for j in range(pairs):
        u, v, typ = ends[j]; n = len(reads_on[j])
        if kind[j] == "dense":
            d = [int(x) for x in rng.integers(1, 4, size=n + 1)]; length = sum(d)
        elif j in lengths:
            length = lengths[j]; d = _chain_for_length(rng, n, length, max_dist) if n else []
        elif n:
            d = [draw() for _ in range(n + 1)]; length = sum(d)
            if rng.random() < inconsistent_share:
                length = max(1, length + int(rng.choice([-7, -1, 1, 7])))
        else:
            d = []; length = int(rng.integers(simple_len[0], simple_len[1] + 1))
        lst = [(reads_on[j][i], int(rng.integers(0, 2)), 0, d[i], d[i + 1]) for i in range(n)]
        r = H.rec(u, v, typ, length, lst); t = H.twin_of(r); r["flow"] = t["flow"] = float(flows[int(rng.integers(0, len(flows)))])
        records += [r, t, t, r] if kind[j] == "loop2" else [r, t]
    header = (0, 2 * N, arl)
    _assert_loadable(N, records, max_dist)
    return N, header, records


def _assert_loadable(N, records, max_dist=MAX_DIST):
    """the loader's rules: every record followed by its twin, ids within 1 .. N, distances within the limit"""
    assert len(records) % 2 == 0
    for a, b in zip(records[0::2], records[1::2]):
        assert dict(H.twin_of(a), flow=b["flow"]) == b and 1 <= a["frm"] <= N and 1 <= a["to"] <= N and a["len"] >= 1
        for (i, o, f, dp, dn) in a["list"]:
            assert 1 <= i <= N and o in (0, 1) and 0 <= dp <= max_dist and 0 <= dn <= max_dist


def text_of(header, records):
    return H.graph_text(header, records)


# ------------------------------------------------------------------------------------------ mates
def _dense(h):
    return len(h["list"]) >= 4 and all(e[3] <= 3 for e in h["list"])


def mates_for(graph, seed, libraries=2, for_reference=False, k=40, same_edge_share=1.0, cross_share=1.0):
    """{library: [(read a, strand a, read b, strand b)]} on a parsed graph, in the spirit of H.pairs_from_graph.
    Libraries 1 .. `libraries`: same-edge pairs L entries apart on the ordinary lists (so the libraries differ in insert size and each passes
    H.valid_every_round, asserted here), pairs through a node (the first three entries of an in-half and an out-half of one node, strands 1 - orientation, one in
    six flipped), pairs between edges that share no node, pairs among the reads on many pairs by their number of common pairs (both id orders) and between them and
    ordinary reads, self pairs, a mate that is a node, a pair given twice.
    Where the graph has dense edges, the next library has only neighbours on them: valid, and upper + k - 2 arl <= 0, so the sweeps skip it (asserted).
    same_edge_share, cross_share: the share of edges, and of nodes and distant edge pairs, that get such mates (large graphs).
    Unless for_reference, the last library has one distance and a pair through a node: not valid (asserted) -- the reference divides by zero on it."""
    rng = np.random.default_rng(seed); arl = graph["header"][2]
    t = H.read_edge_table(graph); pr = H.by_read(t)
    nodes = {a["frm"] for _, a, b in graph["pairs"]} | {a["to"] for _, a, b in graph["pairs"]}
    E = {q: (a if a["frm"] < a["to"] else b) for q, a, b in graph["pairs"]}
    once = lambda r, q: len(t[(r, q)]["forward"]) == 1
    uniq = lambda r: r not in nodes and len(pr[r]) == 1
    out = {L: [] for L in range(1, libraries + 1)}
    strand = lambda: int(rng.integers(0, 2))
    # same edge, L entries apart
    for q in sorted(E):
        lst = [e[0] for e in E[q]["list"]]
        if _dense(E[q]) or rng.random() >= same_edge_share:
            continue
        for L in out:
            for i in range(len(lst) - L):
                a, b = (lst[i], lst[i + L]) if rng.integers(0, 2) else (lst[i + L], lst[i])
                out[L].append((a, strand(), b, strand()))
    leaving = {}
    for q, a, b in graph["pairs"]:
        for h in (a, b):
            if h["list"] and h["frm"] != h["to"]:
                leaving.setdefault(h["frm"], []).append(h)
    if cross_share > 0:
        # through a node
        for i in sorted(leaving):
            if rng.random() >= cross_share:
                continue
            for a in [h for h in leaving[i] if h["type"] in (0, 1)]:
                for b in [h for h in leaving[i] if h["type"] in (2, 3)]:
                    for j in range(min(3, len(a["list"]), len(b["list"]))):
                        ea, eb = a["list"][j], b["list"][j]; sa, sb = 1 - ea[1], 1 - eb[1]
                        if rng.integers(0, 6) == 0:
                            sa = 1 - sa
                        out[int(rng.integers(1, libraries + 1))].append((ea[0], sa, eb[0], sb))
        # between edges that share no node
        hs = [h for q, a, b in graph["pairs"] for h in (a, b) if h["list"]]
        for _ in range(int(len(hs) // 3 * cross_share)):
            x, y = hs[int(rng.integers(0, len(hs)))], hs[int(rng.integers(0, len(hs)))]
            if {x["frm"], x["to"]} & {y["frm"], y["to"]}:
                continue
            L = int(rng.integers(1, libraries + 1))
            for j in range(min(4, len(x["list"]), len(y["list"]))):
                ea, eb = x["list"][j], y["list"][j]
                out[L].append((ea[0], 1 - ea[1], eb[0], 1 - eb[1]))
    # the reads on many pairs
    many = sorted(r for r in pr if len(pr[r]) > 1 and r not in nodes)
    seen = {}
    for a in many:
        for b in many:
            if a < b:
                seen.setdefault(len(set(pr[a]) & set(pr[b])), []).append((a, b))
    for c in sorted(seen):
        ab = seen[c]; picks = [ab[0], ab[-1]]
        out[1].append((picks[0][0], strand(), picks[0][1], strand())); out[1].append((picks[1][1], strand(), picks[1][0], strand()))
    for a in many[:40]:
        q = pr[a][int(rng.integers(0, len(pr[a])))]; others = [e[0] for e in E[q]["list"] if e[0] != a]
        if others:
            b = others[int(rng.integers(0, len(others)))]
            out[1 + len(out[1]) % libraries].append((a, strand(), b, strand()) if rng.integers(0, 2) else (b, strand(), a, strand()))
    # self pairs, a node as a mate, a pair given twice
    on_lists = sorted(r for r in pr if r not in nodes)
    for L in out:
        if on_lists:
            r = on_lists[int(rng.integers(0, len(on_lists)))]; out[L].append((r, 0, r, 1))
            out[L].append((min(nodes), 1, on_lists[0], 1)); out[L].append((on_lists[-1], 0, max(nodes), 1))
        if out[L]:
            out[L].append(out[L][0])
    dist_of = lambda pl: H.mate_distances(t, H.mate_entries(pl))
    for L in out:
        assert H.valid_every_round(dist_of(out[L])), f"library {L}: a round with fewer than two distances"
    nxt = libraries + 1
    dense = [q for q in sorted(E) if _dense(E[q])]
    if dense:
        pl = []
        for q in dense:
            lst = [e[0] for e in E[q]["list"]]
            pl += [(lst[i], strand(), lst[i + 1], strand()) for i in range(len(lst) - 1) if once(lst[i], q) and once(lst[i + 1], q)]
        e = H.estimate(dist_of(pl), arl)
        assert H.valid_every_round(dist_of(pl)) and e["upper"] + k - 2 * arl <= 0, "the dense library is not one the sweeps skip"
        # mates through a node in this library too: they never count
        for i in sorted(leaving)[:20]:
            ins = [h for h in leaving[i] if h["type"] in (0, 1)]; outs = [h for h in leaving[i] if h["type"] in (2, 3)]
            if ins and outs and not _dense(ins[0]) and not _dense(outs[0]):
                ea, eb = ins[0]["list"][0], outs[0]["list"][0]; pl.append((ea[0], 1 - ea[1], eb[0], 1 - eb[1]))
        assert H.estimate(dist_of(pl), arl)["upper"] + k - 2 * arl <= 0
        out[nxt] = pl; nxt += 1
    if not for_reference:
        pl = []
        for q in sorted(E):
            lst = [e[0] for e in E[q]["list"]]
            if not _dense(E[q]) and len(lst) >= 2 and lst[0] != lst[1] and uniq(lst[0]) and uniq(lst[1]) and once(lst[0], q) and once(lst[1], q):
                pl.append((lst[0], 1, lst[1], 1)); break
        for i in sorted(leaving):
            ins = [h for h in leaving[i] if h["type"] in (0, 1)]; outs = [h for h in leaving[i] if h["type"] in (2, 3)]
            if ins and outs:
                ea, eb = ins[0]["list"][0], outs[0]["list"][0]
                if not set(pr[ea[0]]) & set(pr[eb[0]]):
                    pl.append((ea[0], 1 - ea[1], eb[0], 1 - eb[1])); break
        assert len(dist_of(pl)) == 1 and H.estimate(dist_of(pl), arl)["valid"] == 0
        out[nxt] = pl
    return out


def skipped_libraries(graph, pairs, k=40):
    """the valid libraries whose upper + k - 2 arl <= 0"""
    t = H.read_edge_table(graph); arl = graph["header"][2]; out = []
    for L, pl in pairs.items():
        e = H.estimate(H.mate_distances(t, H.mate_entries(pl)), arl)
        if e["valid"] and e["upper"] + k - 2 * arl <= 0:
            out.append(L)
    return out


# ------------------------------------------------------------------------------------------ the cases the test modules share
K = 40                                # of the read stores the graphs are loaded over (reads of 60 bases)
E_SEEDS = tuple(range(20))


def case_e(seed):
    """about 200 pairs over 2 000 reads with every knob on"""
    return composite_graph(1000 + seed, 200, n_reads=2000, hubs=1, loops_once=2, loops_twice=2, dense_edges=2, read_copies=(2, 2, 3, 5), twice_on_edge=0.08)


def mates_e(graph, seed, for_reference=False):
    return mates_for(graph, 2000 + seed, libraries=2, for_reference=for_reference, k=K)


# reads on many pairs: [start, start + m) of one order of the pairs.  17 / 33 from one start share 17 pairs (twice), 9 / 17 share 9, 8 / 17 share 8, 7 / 9 share 7,
# 2 / 17 share 1, 15 and 16 share none with 17
B_COPIES = ((33, 0), (17, 0), (9, 0), (7, 0), (8, 9), (2, 16), (16, 20), (7, 33), (15, 40), (33, 60), (17, 60), 2, 7, 8, 9, 15, 16)


def case_b(pairs=300, copies=B_COPIES):
    return composite_graph(77, pairs, n_reads=3000, hubs=1, read_copies=copies, twice_on_edge=0.1, list_len=(1, 5), empty_share=0.05)


def mates_b(graph, for_reference=False):
    return mates_for(graph, 78, libraries=2, for_reference=for_reference, k=K)


def case_a_pairs(pairs):
    """record pairs on both sides of 2^15 (half-edges on both sides of 2^16): lists of 1 .. 3 reads, short distances, no loops (ordinal = index of a pair)"""
    return composite_graph(5, pairs, node_share=0.75, hubs=4, list_len=(1, 3), empty_share=0.0, loops_once=0, loops_twice=0, dense_edges=0, flows=(1.0, 2.0, 1.0, 0.5),
                           dist=(1, 40), far_share=0.0)


def mates_a(graph):
    """-> (mates, triples).  The tables of the supports and of the links are put in order by the host; the device's sort only has to bring equal keys together.  A
    sort that leaves out the third digit of the second word shows only where one half a has records to the halves b and b + 65 536 IN TURNS: then b's records are
    not adjacent.  So, where the loaded text has more than 32 768 pairs, library 2 gets such mates: the first two reads of a (list order) each mated with the first
    read of half s of pair p and of pair p - 32 768, all close enough to their half's start to count.  triples = [((from, to) of a, of b, of b - 65 536)]"""
    pairs = mates_for(graph, 6, libraries=2, for_reference=True, k=K, same_edge_share=0.1, cross_share=0.15)
    P = graph["pairs"]; triples = []
    if len(P) <= 32768:
        return pairs, triples
    t = H.read_edge_table(graph); pr = H.by_read(t); arl = graph["header"][2]
    nodes = {a["frm"] for _, a, b in P} | {a["to"] for _, a, b in P}
    thr = H.estimate(H.mate_distances(t, H.mate_entries(pairs[2])), arl)["upper"] + K - 2 * arl
    good = lambda h, j: (len(h["list"]) > j and h["list"][j][0] not in nodes and len(pr[h["list"][j][0]]) == 1
                         and [e[0] for e in h["list"]].count(h["list"][j][0]) == 1)
    run = lambda h, j: sum(e[3] for e in h["list"][:j + 1])
    firsts = [(run(h, 1), p, s) for p, (_, a, b) in enumerate(P) for s, h in enumerate((a, b)) if good(h, 0) and good(h, 1)]
    firsts.sort()
    used = set()
    for p in range(32768, len(P)):
        for s in (0, 1):
            hb, hc = P[p][1 + s], P[p - 32768][1 + s]
            if len(triples) == 3 or not (good(hb, 0) and good(hc, 0)) or p in used:
                continue
            far = max(run(hb, 0), run(hc, 0))
            pick = next(((ra, pa, sa) for ra, pa, sa in firsts if pa not in used and pa not in (p, p - 32768) and ra + far < thr
                         and not {P[pa][1]["frm"], P[pa][1]["to"]} & {hb["frm"], hb["to"], hc["frm"], hc["to"]}), None)
            if pick is None:
                continue
            ha = P[pick[1]][1 + pick[2]]; used |= {p, p - 32768, pick[1]}
            for e in ha["list"][:2]:
                for h in (hb, hc):
                    r = h["list"][0]; pairs[2].append((e[0], 1 - e[1], r[0], 1 - r[1]))
            triples.append(((ha["frm"], ha["to"]), (hb["frm"], hb["to"]), (hc["frm"], hc["to"])))
    assert len(triples) == 3
    return pairs, triples


A_READS = (1, 255, 256, 65535, 65536)


def case_a_reads(N):
    return composite_graph(9, 300, n_reads=N, use_reads=[r for r in A_READS if r <= N], list_len=(1, 4), dense_edges=0)


A_LENGTH_PALETTE = (60, 61, 61, 99, 100, 100, 256, 257, 500, 500, 500, 1023, 1024, 2047, 2048, 3000, 3000, 4999, 5000, 5000)


def case_a_longest(longest, pairs=340):
    """pair 0 has `longest` bases and a consistent list; every other ordinary pair takes its length from a short palette: ties in the order key"""
    rng = np.random.default_rng(longest)
    lengths = {j: int(A_LENGTH_PALETTE[int(rng.integers(0, len(A_LENGTH_PALETTE)))]) for j in range(1, pairs)}; lengths[0] = longest
    return composite_graph(longest, pairs, n_reads=4000, hubs=1, loops_once=1, loops_twice=1, dense_edges=0, lengths=lengths, list_len=(0, 4))


def case_c():
    """one edge of 730 reads, distPrevious uniform in [1, 100]; library 1 = all 266 085 ordered pairs of its reads"""
    rng = np.random.default_rng(4); n = 730
    d = [int(x) for x in rng.integers(1, 101, size=n + 1)]
    r = H.rec(1, 2, 3, sum(d), [(3 + i, 1, 0, d[i], d[i + 1]) for i in range(n)])
    pairs = {1: [(3 + i, 1, 3 + j, 1) for i in range(n) for j in range(i + 1, n)]}
    return n + 2, (0, 2 * (n + 2), 60), [r, H.twin_of(r)], pairs


D_LONG, D_CYCLE = 700000, 4990


def case_d(n=D_LONG, cycle=D_CYCLE):
    """a list pool whose distPrevious add up to more than 2^32 (none of fewer than 2 098 177 entries does: the loader takes no distance above 2047):
    three edges 1 -> 2 -> 3 -> 4 of n entries 2046 or 2047 apart (each list's total stays below 2^31) over reads 11 .. 10 + cycle used cyclically, so every
    (read, pair) entry has about n / cycle locations; two short edges 5 -> 6 and 7 -> 8 of reads of their own, whose mates make library 1 valid and give a link.
    Every record leaves the smaller id, type 3, flow 0 (the caller sets flows), nodes ascending: the text is what the writer writes, and a pair's ordinal is its index.
    -> (N, header, text, long, short records, pairs); long = [(reads, orientations, the n + 1 distances)] as numpy arrays"""
    rng = np.random.default_rng(12); long_ = []; parts = []
    first = 11; short_first = first + cycle; N = short_first + 50
    header = (0, 2 * N, 60); parts.append("%d\n%d\n%d\n" % header)
    for e in range(3):
        reads = first + (np.arange(n, dtype=np.int64) + 17 * e) % cycle; o = rng.integers(0, 2, size=n); d = rng.integers(2046, 2048, size=n + 1)
        long_.append((reads, o, d)); length = int(d.sum()); assert length < 1 << 31
        parts.append("%d\t%d\t3\t1\t%d\t0\t%d\n" % (1 + e, 2 + e, length, n))
        parts.append("".join(["%d\t%d\t0\t%d\t%d\n" % x for x in zip(reads.tolist(), o.tolist(), d[:-1].tolist(), d[1:].tolist())])); parts.append("\n")
        parts.append("%d\t%d\t0\t1\t%d\t0\t%d\n" % (2 + e, 1 + e, length, n))
        parts.append("".join(["%d\t%d\t0\t%d\t%d\n" % x for x in zip(reads[::-1].tolist(), (1 - o[::-1]).tolist(), d[:0:-1].tolist(), d[-2::-1].tolist())])); parts.append("\n")
    short = []
    for (u, v, r0, m) in ((5, 6, short_first, 40), (7, 8, short_first + 40, 10)):
        d = [int(x) for x in rng.integers(200, 1201, size=m + 1)]                          # (an insert size of some thousands: the bound takes in a few entries of 2047)
        r = H.rec(u, v, 3, sum(d), [(r0 + i, 0, 0, d[i], d[i + 1]) for i in range(m)]); short += [r, H.twin_of(r)]
    parts.append(H.graph_text(header, short)[len(parts[0]):])
    a, b = [e[0] for e in short[0]["list"]], [e[0] for e in short[2]["list"]]
    pairs = {1: [(a[i], 1, a[i + 3], 1) for i in range(len(a) - 3)] + [(a[i], 1, b[i], 1) for i in range(4)] + [(int(long_[0][0][5]), 1, a[0], 1)]}
    return N, header, "".join(parts), long_, short, pairs


def case_d_table(header, long_, short):
    """the read-to-edge table of case_d by the contract, the long lists with numpy cumsum: (rows of (read, pair, from, to, type, n_forward, n_reverse, location),
    int32 locations).  Every list total is below 2^31, so no location wraps"""
    per_pair = []                                                                     # per pair: {read: (forward locations, reverse locations)}
    for reads, o, d in long_:
        run = np.cumsum(d[:-1]); fwd = np.where(o == 1, run, -run)                    # E is the record; its twin's list is the reverse, orientations flipped
        rrun = np.cumsum(d[:0:-1]); rev = np.where(o[::-1] == 0, rrun, -rrun); rreads = reads[::-1]
        assert int(run[-1]) < 1 << 31 and int(rrun[-1]) < 1 << 31
        halves = []
        for ids, vals in ((reads, fwd), (rreads, rev)):
            k = np.argsort(ids, kind="stable"); u, start = np.unique(ids[k], return_index=True)
            halves.append(dict(zip(u.tolist(), np.split(vals[k], start[1:]))))
        per_pair.append({i: (halves[0][i], halves[1][i]) for i in halves[0]})
    ts = H.read_edge_table(H.parse_graph(H.graph_text(header, short)))
    for q in range(len(short) // 2):
        per_pair.append({r: (np.asarray(w["forward"], dtype=np.int64), np.asarray(w["reverse"], dtype=np.int64)) for (r, qq), w in ts.items() if qq == q})
    ends = [(1 + e, 2 + e) for e in range(len(long_))] + [(short[2 * i]["frm"], short[2 * i]["to"]) for i in range(len(short) // 2)]
    ent = []; loc = []; at = 0
    for r in sorted(set().union(*per_pair)):
        for q, tab in enumerate(per_pair):
            if r in tab:
                f, v = tab[r]; ent.append((r, q, ends[q][0], ends[q][1], 3, len(f), len(v), at)); loc += [f, v]; at += len(f) + len(v)
    return np.asarray(ent, dtype=np.int64), np.concatenate(loc).astype(np.int32)


