"""CPU: the generator of composite graphs (tests/compgen.py) -- deterministic per seed, loadable by the parser, taken by all four restatements (read-to-edge table and
estimate, supports at a node, scaffold links, contigs) -- and the conditions that keep tests/test_gpu_compgen.py from being vacuous, shown from the restatements
alone.  Measured on the CPU for these tests: in all 13 golden P.graph4 files every read lies on exactly one record pair and exactly once on its edge; the graphs here
are what closes that gap."""
import numpy as np
import pytest
import sage2_amd as s2
import compgen as CG
import test_mate_estimate_host as H
import test_mate_support_host as MS
import test_links_host as LH
import test_contigs_host as CH


def store_reads(n, seed, L=60):
    """the reads of test_gpu_mate_estimate.random_store(n, seed): (bases, offsets)"""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n + n // 8, L))]
    reads = sorted({r.tobytes().decode() for r in a})[:n]
    assert len(reads) == n
    return np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(), np.arange(0, (n + 1) * L, L, dtype=np.uint64)


def host_store(n, seed, k=CG.K):
    ctx = s2.Context(k, device=-2); ctx.reads_add_ascii(*store_reads(n, seed)); ctx.reads_organize()
    assert ctx.reads_stats().unique_reads == n
    return ctx


def host_seqs(n, seed):
    ctx = host_store(n, seed); seqs = H.stored_reads(ctx); ctx.close()
    return seqs


def parsed(case):
    N, header, recs = case[:3]
    return H.parse_graph(H.graph_text(header, recs))


# ------------------------------------------------------------------------------------------ what the restatements say about a graph and its mates
def max_pairs_per_read(g):
    return max(len(v) for v in H.by_read(H.read_edge_table(g)).values())


def max_times_on_an_edge(g):
    return max(max(len(w["forward"]), len(w["reverse"])) for w in H.read_edge_table(g).values())


def distances_per_entry(g, pl):
    """{(a, b): (common pairs, distances)} of the mate entries with a < b"""
    t = H.read_edge_table(g); pr = H.by_read(t); out = {}
    for a, b in H.mate_entries(pl):
        if a < b:
            out[(a, b)] = (len(set(pr.get(a, [])) & set(pr.get(b, []))), len(H.mate_distances(t, [(a, b)])))
    return out


def links_owed_to_two_locations(g, pairs, k=CG.K):
    """link rows that change when the mates of reads with two forward locations on their (only) pair are left out, the estimates kept"""
    t, ests, (_, hi) = MS.support_inputs(g, pairs); arl = g["header"][2]
    two = {r for (r, q), w in t.items() if len(w["forward"]) == 2 or len(w["reverse"]) == 2}
    rest = {L: [p for p in pl if p[0] not in two and p[2] not in two] for L, pl in pairs.items()}
    full = LH.links(g, t, pairs, ests, hi, arl, k); less = LH.links(g, t, rest, ests, hi, arl, k)
    return [r for r in full if r not in less]


def conditions(g, pairs, seqs, k=CG.K):
    """the non-vacuity conditions of case E for one graph: {name: bool}"""
    sup = MS.all_supports(g, pairs, k); lk = LH.all_links(g, pairs, k); hv = LH.halves_of(g)
    _, st, _ = CH.contig_table(g, seqs, 20)
    return dict(support_2=any(r[3] >= 2 for r in sup), gap_negative=any(r[5] < 0 for r in lk), gap_positive=any(r[5] > 0 for r in lk),
                different_nodes=any(hv[(r[0], r[1])][0]["frm"] != hv[(r[2], r[3])][0]["frm"] for r in lk),
                two_locations_link=bool(links_owed_to_two_locations(g, pairs, k)),
                loop_with_reads=any(a["frm"] == a["to"] and a["list"] for _, a, _ in g["pairs"]),
                wrapped=st["wrapped"] > 0, gaps=st["gaps"] > 0, skipped_library=bool(CG.skipped_libraries(g, pairs, k)))


def sort_passes_by_rule(N, pairs):
    """the digits of (read:30 | pair:31 | side:1) that can be non-zero, from the contract's words alone"""
    b, bp = int(N).bit_length(), int(pairs).bit_length()
    return sum(1 for lo in range(0, 64, 8) if lo < 1 + bp or 32 <= lo < 32 + b)


# ------------------------------------------------------------------------------------------ tests
def test_deterministic_per_seed():
    a, b, c = CG.case_e(3), CG.case_e(3), CG.case_e(4)
    assert a == b and a != c
    g = parsed(a)
    assert CG.mates_e(g, 3) == CG.mates_e(g, 3) and CG.mates_e(g, 3) != CG.mates_e(g, 4)
    # the knobs that no shared case turns: inconsistent lengths, a length override without a list
    N, header, recs = CG.composite_graph(1, 40, inconsistent_share=0.5, lengths={0: 1}, hubs=1)
    bad = [r for r in recs if r["list"] and sum(e[3] for e in r["list"]) + r["list"][-1][4] != r["len"]]
    assert bad and recs[0]["len"] == 1 and not recs[0]["list"]


@pytest.fixture(scope="module")
def e_cases():
    return {s: CG.case_e(s) for s in CG.E_SEEDS}


def test_round_trip_through_the_parser(e_cases):
    cases = list(e_cases.values()) + [CG.case_b(), CG.case_a_reads(65535), CG.case_a_longest(65536), CG.case_c()[:3]]
    for N, header, recs in cases:
        text = H.graph_text(header, recs); g = H.parse_graph(text, fold=False)
        flat = [r for _, a, b in g["pairs"] for r in (a, b)]
        assert flat == recs and H.graph_text(header, flat) == text
        CG._assert_loadable(N, flat)


def test_every_knob_shows_in_case_e(e_cases):
    types, flows, orient, larger_first, hub = set(), set(), set(), 0, 0
    for N, header, recs in e_cases.values():
        g = parsed((N, header, recs)); assert 1900 <= N <= 2100 and 190 <= len(g["pairs"]) <= 210
        types |= {a["type"] for _, a, _ in g["pairs"]}; flows |= {a["flow"] for _, a, _ in g["pairs"]}
        orient |= {e[1] for _, a, _ in g["pairs"] for e in a["list"]}; larger_first += sum(a["frm"] > a["to"] for _, a, _ in g["pairs"])
        assert any(not a["list"] for _, a, _ in g["pairs"]) and max(max(e[3], e[4]) for _, a, _ in g["pairs"] for e in a["list"]) > 120
        assert len(H.parse_graph(H.graph_text(header, recs), fold=False)["pairs"]) == len(g["pairs"]) + 2      # the loops written twice
        assert max_pairs_per_read(g) >= 5 and max_times_on_an_edge(g) >= 2
        leaving = {}
        for _, a, b in g["pairs"]:
            for h in (a, b):
                leaving.setdefault(h["frm"], []).append(h["type"])
        hub += any(sum(t in (0, 1) for t in v) >= 4 and sum(t in (2, 3) for t in v) >= 4 for v in leaving.values())
        # consistent with the lists, both halves
        assert all(sum(e[3] for e in h["list"]) + h["list"][-1][4] == h["len"] for _, a, b in g["pairs"] for h in (a, b) if h["list"])
    assert types == {0, 1, 2, 3} and flows == {0.0, 0.5, 1.0, 2.0} and orient == {0, 1} and larger_first > 100 and hub == len(e_cases)
    assert max(max(e[3], e[4]) for N, header, recs in e_cases.values() for r in recs for e in r["list"]) == CG.MAX_DIST


def test_case_e_conditions_hold_across_the_seeds(e_cases):
    """all four restatements run on every seed; across the twenty seeds each condition holds somewhere"""
    seen = {}
    for s, case in e_cases.items():
        g = parsed(case); pairs = CG.mates_e(g, s); seqs = host_seqs(case[0], 100 + s)
        assert sorted(pairs) == [1, 2, 3, 4] and sorted(CG.mates_e(g, s, for_reference=True)) == [1, 2, 3]
        t, ests, _ = MS.support_inputs(g, pairs)
        assert [ests[L]["valid"] for L in (1, 2, 3, 4)] == [1, 1, 1, 0]
        for name, v in conditions(g, pairs, seqs).items():
            seen[name] = seen.get(name, 0) + bool(v)
    assert all(seen.values()), seen


def test_case_b_conditions():
    case = CG.case_b(); g = parsed(case); pairs = CG.mates_b(g)
    t = H.read_edge_table(g); pr = H.by_read(t)
    assert {len(v) for v in pr.values()} >= {1, 2, 7, 8, 9, 15, 16, 17, 33} and max_times_on_an_edge(g) == 2
    per = distances_per_entry(g, pairs[1])
    assert {c for c, _ in per.values()} >= {0, 1, 7, 8, 9, 17}
    nine = [e for e, (c, d) in per.items() if d >= 9]; fewer = [e for e, (c, d) in per.items() if c == 17 and 0 < d < 17]
    assert nine and fewer and len(set(nine) | set(fewer)) >= 2
    # reads on many pairs next to reads on one: among the ids within 8 of such a read there are single-pair reads
    many = [r for r in pr if len(pr[r]) >= 7]
    assert all(any(len(pr.get(x, [])) == 1 for x in range(r - 8, r + 9)) for r in many)
    # no support or link record comes from a read on many pairs: without their mates the tables are the same
    rest = {L: [p for p in pl if len(pr.get(p[0], [])) <= 1 and len(pr.get(p[2], [])) <= 1] for L, pl in pairs.items()}
    _, ests, (_, hi) = MS.support_inputs(g, pairs); arl = g["header"][2]
    assert MS.supports(g, t, pairs, ests, hi, arl, CG.K) == MS.supports(g, t, rest, ests, hi, arl, CG.K)
    assert LH.links(g, t, pairs, ests, hi, arl, CG.K) == LH.links(g, t, rest, ests, hi, arl, CG.K) and LH.all_links(g, pairs, CG.K)


def test_case_c_conditions():
    N, header, recs, pairs = CG.case_c(); g = H.parse_graph(H.graph_text(header, recs))
    d = H.mate_distances(H.read_edge_table(g), H.mate_entries(pairs[1])); e = H.estimate(d, header[2])
    assert len(d) == 266085 > 262144 and e["valid"] == 1 and e["rounds"] >= 3 and e["considered"][0] < e["considered"][-1] and H.valid_every_round(d)


def test_case_a_reads_and_longest_conditions():
    for N in (65535, 65536):
        g = parsed(CG.case_a_reads(N)); on = {e[0] for _, a, _ in g["pairs"] for e in a["list"]}
        assert on >= {r for r in CG.A_READS if r <= N} and sort_passes_by_rule(N, len(g["pairs"])) == (2 if N < 65536 else 3) + 2
    for longest in (65535, 65536, 70000):
        case = CG.case_a_longest(longest); g = parsed(case); seqs = host_seqs(case[0], 7)
        rows, st, thr = CH.contig_table(g, seqs)
        assert rows[0]["len"] == longest and len(rows) >= 301 and st["inconsistent"] == 0 and rows[0]["gaps"] > 0 and all(60 <= r["len"] <= 5000 for r in rows[1:])
        top = next(h for _, a, b in g["pairs"] for h in (a, b) if h["len"] == longest); assert len(top["list"]) >= 35
        lens = [r["len"] for r in rows[1:]]; assert len(set(lens)) < len(lens) // 4                       # ties
        assert ((longest - min(lens)) >> 16 != 0) == (longest == 70000)                                   # the key's third digit: selected from 65 536 on, non-zero at 70 000


def test_case_a_pairs_conditions():
    """33 024 record pairs: supported rows and link rows across half-edge 65 536 in both orders, and three halves whose link records go to b and b + 65 536 in turns"""
    case = CG.case_a_pairs(33024); g = parsed(case); pairs, triples = CG.mates_a(g)
    assert len(g["pairs"]) == 33024 and [q for q, _, _ in g["pairs"]] == list(range(33024)) and 65536 < case[0] < 1 << 17
    ix = {}
    for p, (_, a, b) in enumerate(g["pairs"]):
        ix[(a["frm"], a["to"])] = 2 * p; ix[(b["frm"], b["to"])] = 2 * p + 1
    across = lambda idx: any(a >= 65536 > b for a, b in idx) and any(b >= 65536 > a for a, b in idx)
    by_q = {q: (a, b) for q, a, b in g["pairs"]}; to = lambda q, i: next(h for h in by_q[q] if h["frm"] == i)["to"]
    sup = [r for r in MS.all_supports(g, pairs, CG.K) if r[3] >= 1]
    assert across([(ix[(i, to(qa, i))], ix[(i, to(qb, i))]) for i, qa, qb, s in sup]) and any(r[3] >= 2 for r in sup)
    hv = LH.halves_of(g); at = lambda q, s: ix[(hv[(q, s)][0]["frm"], hv[(q, s)][0]["to"])]
    lk = {(at(r[0], r[1]), at(r[2], r[3])): r[4] for r in LH.all_links(g, pairs, CG.K)}
    assert across(list(lk)) and len(triples) == 3
    assert all(ix[b] == ix[c] + 65536 and lk[(ix[a], ix[b])] == 2 and lk[(ix[a], ix[c])] == 2 for a, b, c in triples)
    assert CG.mates_a(parsed(CG.case_a_pairs(400)))[1] == []


def test_case_d_table_by_cumsum_is_the_restatement_s():
    """case D computes its expected table with numpy; on a small instance of the same construction that table is the per-entry restatement's"""
    N, header, text, long_, short, pairs = CG.case_d(n=3000, cycle=70)
    g = H.parse_graph(text); t = H.read_edge_table(g)
    assert len(g["pairs"]) == 5 and [q for q, _, _ in g["pairs"]] == [0, 1, 2, 3, 4] and all(a["frm"] < a["to"] for _, a, _ in g["pairs"])
    CG._assert_loadable(N, [r for _, a, b in g["pairs"] for r in (a, b)])
    ent, loc = CG.case_d_table(header, long_, short)
    assert [(int(e[0]), int(e[1])) for e in ent] == sorted(t)
    for e in ent:
        w = t[(int(e[0]), int(e[1]))]; at = int(e[7])
        assert (w["frm"], w["to"], w["type"], len(w["forward"]), len(w["reverse"])) == tuple(int(v) for v in e[2:7])
        assert loc[at:at + e[5]].tolist() == w["forward"] and loc[at + e[5]:at + e[5] + e[6]].tolist() == w["reverse"]
    d = H.mate_distances(t, H.mate_entries(pairs[1])); assert H.valid_every_round(d)
    assert LH.all_links(g, pairs, CG.K)                                              # the two short edges give a link
    # at full size: no pool of fewer than 2 098 177 entries wraps (2047 is the largest distance); three lists of 700 000 entries of 2046 or more pass 2^32, each
    # stays below 2^31
    assert 2098176 * 2047 < 1 << 32 and 3 * CG.D_LONG * 2046 > 1 << 32 and (CG.D_LONG + 1) * 2047 < 1 << 31


def test_sort_passes_rule():
    assert sort_passes_by_rule(8203, 2) == 3 and sort_passes_by_rule(65535, 300) == 4 and sort_passes_by_rule(65536, 300) == 5
    assert sort_passes_by_rule(99000, 32767) == 2 + 3 and sort_passes_by_rule(99000, 32768) == 3 + 3
