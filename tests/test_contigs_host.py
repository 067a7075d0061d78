"""CPU: the contract of sage2ov_contigs_* (include/sage2ov.h; OverlapGraph::printGraph and saveContigsToFile, overlapGraph.cpp:507-784) restated in Python over
parse_graph output and the stored reads, pinned on a hand-built graph with literal strings -- and what the reference and GPU tests of the contigs share: that
graph, the FASTA text, its parser and the comparison that allows the reference's open order among edges of equal length.  Also the C structs and the answer of
a device-less context."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import fixtures as fx
import sage2_amd as s2
import test_mate_estimate_host as H


# ------------------------------------------------------------------------------------------ the restatement
def default_threshold(arl):
    """contigLengthThreshold = (int)ceilf(100 * (averageReadLength / 100.0)), overlapGraph.cpp:32"""
    return int(math.ceil(np.float32(100 * (arl / 100.0))))


def halves_of(graph):
    """the half-edges in index order: pair p of parse_graph's list = halves 2p (the record) and 2p + 1 (its twin)"""
    return [h for _, a, b in graph["pairs"] for h in (a, b)]


def save_ordinals(hs):
    """pair -> ordinal of its record pair in sage2ov_graph4_save's order: per node ascending, the halves with from <= to by ascending index; a loop, which the
    writer visits from both halves, at its first writing (its second one takes an ordinal too)"""
    order = sorted((h["frm"], x) for x, h in enumerate(hs) if h["frm"] <= h["to"]); out = {}
    for rank, (_, x) in enumerate(order):
        out.setdefault(x >> 1, rank)
    return out


def spell(h, seqs):
    """(string, gaps, Ns, consistent) of half-edge h by overlapGraph.cpp:635-697"""
    rd = lambda i, fwd: seqs[i] if fwd else fx.revcomp(seqs[i])
    first = rd(h["frm"], h["type"] in (2, 3))
    s = ["N"] * (h["len"] + len(first)); at = 0; gaps = ns = 0

    def put(text):
        nonlocal at
        for ch in text:
            if at < len(s):
                s[at] = ch                                                            # (beyond the string: dropped; the reference writes out of bounds)
            at += 1
    put(first)
    nxt = h["len"]
    for (i, o, f, dp, dn) in h["list"]:
        r = rd(i, o == 1)
        if dp > len(r):
            gaps += 1; ns += dp - len(r); put("N" * (dp - len(r)) + r)
        else:
            put(r[len(r) - dp:])
        nxt = dn
    last = rd(h["to"], h["type"] in (1, 3))
    if nxt <= len(last):                                                              # else the unsigned loop start of :696 wraps and nothing is copied
        put(last[len(last) - nxt:])
    return "".join(s), gaps, ns, sum(e[3] for e in h["list"]) + nxt == h["len"]


def contig_table(graph, seqs, threshold=0, genome_size=0):
    """-> (rows, stats, threshold used); a row is dict(frm, to, pair, len, type, flow, string, string_length, contig_length, start, gaps, ns, wrapped)"""
    thr = threshold or default_threshold(graph["header"][2])
    hs = halves_of(graph); ordinal = save_ordinals(hs)
    deg = {}
    for h in hs:
        deg[h["frm"]] = deg.get(h["frm"], 0) + 1
    sel = [x for x, h in enumerate(hs) if h["frm"] >= h["to"] and h["len"] >= thr and (h["frm"] != h["to"] or x & 1)]
    sel.sort(key=lambda x: (hs[x]["frm"], -x))                                        # the enumeration of :529-531: nodes ascending, a node's list newest first
    sel.sort(key=lambda x: -hs[x]["len"])                                             # stable: ties keep it
    rows = []; st = dict(contigs=len(sel), written=0, bases=0, longest=0, n50=0, n50_ordinal=0, n90=0, n90_ordinal=0, covered=0, gaps=0, n_bases=0, inconsistent=0, wrapped=0)
    nx = 0
    for i, x in enumerate(sel):
        h = hs[x]; string, gaps, ns, ok = spell(h, seqs)
        Lf, Lt, ln = len(seqs[h["frm"]]), len(seqs[h["to"]]), h["len"]
        one_f, one_t = deg[h["frm"]] == 1, deg[h["to"]] == 1
        start = 0 if one_f else Lf - Lf // 2                                          # :699-724
        wrapped = not one_t and ln < Lt // 2
        cl = 0 if wrapped else (Lf if one_f else Lf - Lf // 2) + (ln if one_t else ln - Lt // 2)
        rows.append(dict(frm=h["frm"], to=h["to"], pair=ordinal[x >> 1], len=ln, type=h["type"], flow=h["flow"], string=string, string_length=len(string), contig_length=cl,
                         start=start, gaps=gaps, ns=ns, wrapped=wrapped, written=not wrapped and cl >= thr))
        st["covered"] += ln; st["gaps"] += gaps; st["n_bases"] += ns; st["inconsistent"] += not ok; st["wrapped"] += wrapped
        if rows[-1]["written"]:
            st["written"] += 1; st["bases"] += cl
        if i == 0:
            st["longest"] = cl
        nx += cl
        if not st["n50_ordinal"] and nx >= genome_size // 2:
            st["n50"], st["n50_ordinal"] = cl, i + 1
        if not st["n90_ordinal"] and nx >= genome_size * 9 // 10:
            st["n90"], st["n90_ordinal"] = cl, i + 1
    return rows, st, thr


def fasta_text(rows, scaffold=False):
    """the file of overlapGraph.cpp:726-742: running gap and N totals over all rows, ordinals with holes, lines of 60 cut at the string's end as substr cuts"""
    out = []; gaps = ns = 0
    for i, r in enumerate(rows):
        gaps += r["gaps"]; ns += r["ns"]
        if not r["written"]:
            continue
        out.append(">%s_%d flow=%g Edge length=%d String length: %d e(%d, %d) gapCount=%d nCount=%d\n" %
                   ("scaffold" if scaffold else "contig", i + 1, r["flow"], r["contig_length"], r["string_length"], r["frm"], r["to"], gaps, ns))
        for at in range(r["start"], r["start"] + r["contig_length"], 60):
            out.append(r["string"][at:min(at + 60, r["start"] + r["contig_length"])] + "\n")
    return "".join(out)


def table_tuples(rows):
    return [(r["frm"], r["to"], r["pair"], r["len"], r["string_length"], r["contig_length"], r["start"], r["gaps"], r["ns"], np.float32(r["flow"]), r["type"]) for r in rows]


def got_tuples(table):
    return [(int(t["from"]), int(t["to"]), int(t["pair"]), int(t["edge_length"]), int(t["string_length"]), int(t["contig_length"]), int(t["start"]), int(t["gap_count"]),
             int(t["n_count"]), np.float32(t["flow"]), int(t["type"])) for t in table]


STAT_NAMES = ("contigs", "written", "bases", "longest", "n50", "n50_ordinal", "n90", "n90_ordinal", "covered", "gaps", "n_bases", "inconsistent", "wrapped")


def same_stats(got: s2.ContigStats, want):
    assert {n: getattr(got, n) for n in STAT_NAMES} == {n: int(want[n]) for n in STAT_NAMES}


# ------------------------------------------------------------------------------------------ a FASTA against the restatement, the reference's open order allowed
def parse_fasta(text):
    """[dict(ordinal, flow, contig_length, string_length, frm, to, gaps, ns, lines)]"""
    import re
    recs = []
    for line in text.splitlines():
        if line.startswith(">"):
            m = re.fullmatch(r">(?:contig|scaffold)_(\d+) flow=(\S+) Edge length=(\d+) String length: (\d+) e\((\d+), (\d+)\) gapCount=(\d+) nCount=(\d+)", line)
            assert m, line
            recs.append(dict(ordinal=int(m[1]), flow=m[2], contig_length=int(m[3]), string_length=int(m[4]), frm=int(m[5]), to=int(m[6]), gaps=int(m[7]), ns=int(m[8]), lines=[]))
        else:
            recs[-1]["lines"].append(line)
    return recs


def same_fasta_up_to_ties(ref_text, rows):
    """the reference's file against the restatement's rows.  std::sort with a length-only comparator (overlapGraph.cpp:496-501, :588) leaves the order of rows of equal
    edge length open: such a group is compared as a set, its ordinals must be ordinals of the group, and the running counters are recomputed in the reference's own
    order (where every row of the group is in the file; else they must lie between the group's first and last possible values).  Everything else is equal.
    -> the number of groups with more than one row"""
    ref = parse_fasta(ref_text); want = parse_fasta(fasta_text(rows))
    assert len(ref) == len(want)
    by_ord = {r["ordinal"]: r for r in ref}; assert len(by_ord) == len(ref)
    body = lambda r: (r["flow"], r["contig_length"], r["string_length"], r["frm"], r["to"], tuple(r["lines"]))
    groups = 0; i = 0; g0 = n0 = 0                                                    # g0, n0: the running totals in front of the group
    while i < len(rows):
        j = i
        while j < len(rows) and rows[j]["len"] == rows[i]["len"]:
            j += 1
        mine = [w for w in want if i < w["ordinal"] <= j]; theirs = [by_ord[o] for o in range(i + 1, j + 1) if o in by_ord]
        assert sorted(body(r) for r in mine) == sorted(body(r) for r in theirs), (i, j)
        g1, n1 = g0 + sum(r["gaps"] for r in rows[i:j]), n0 + sum(r["ns"] for r in rows[i:j])
        if j - i == 1:
            assert [(r["ordinal"], r["gaps"], r["ns"]) for r in mine] == [(r["ordinal"], r["gaps"], r["ns"]) for r in theirs]
        else:
            groups += 1
            if len(theirs) == j - i:                                                  # the reference's order of the group is in its file
                own = {}
                for r in rows[i:j]:
                    own.setdefault((r["contig_length"], r["string_length"], r["frm"], r["to"]), []).append((r["gaps"], r["ns"]))
                g, n = g0, n0
                for t in theirs:
                    cands = own[(t["contig_length"], t["string_length"], t["frm"], t["to"])]
                    pick = next((c for c in cands if (t["gaps"], t["ns"]) == (g + c[0], n + c[1])), None)      # (parallel edges: the one the reference took here,
                    assert pick is not None, (t, g, n, cands)                                                  # and the running totals go on from that one)
                    cands.remove(pick); g += pick[0]; n += pick[1]
            else:
                assert all(g0 <= t["gaps"] <= g1 and n0 <= t["ns"] <= n1 for t in theirs)
        g0, n0 = g1, n1; i = j
    return groups


# ------------------------------------------------------------------------------------------ the hand-built graph
HAND_K = 21
HAND_HEADER = (0, 20, 50)                                                             # average read length 50: contigLengthThreshold = 50
READ_61, READ_37 = 18, 10                                                             # the ids the two odd reads get (asserted by hand_reads)


def hand_reads():
    """(bases, offsets): 18 random reads of 60 bases, one of 61 and one of 37"""
    rng = np.random.default_rng(7)
    reads = ["".join(rng.choice(list("ACGT"), size=n)) for n in [60] * 18 + [61, 37]]
    off = np.zeros(len(reads) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(), off


def hand_store(device=-2):
    ctx = s2.Context(HAND_K, device=device); ctx.reads_add_ascii(*hand_reads()); ctx.reads_organize()
    seqs = H.stored_reads(ctx)
    assert len(seqs) == 20 and len(seqs[READ_61]) == 61 and len(seqs[READ_37]) == 37 and all(len(s) == 60 for i, s in seqs.items() if i not in (READ_61, READ_37))
    return ctx, seqs


def hand_contig_graph():
    """the flat record list.  Rows (the halves with from >= to) at threshold 50, in table order:
      G  18 -> 16  2155  type 1  neither degree is 1; the 37-base read three times: distPrevious 37 (= L: the whole read, no gap), 38 (L + 1: one N), 2047 (2010 N)
      E  18 -> 9    140  type 3  only to's degree is 1: start 31 of the 61-base read, start + contig_length one past the string; both orientations; a gap of 5 N
      H  17 -> 16    91  type 0  only from's degree is 1; the last distNext is 61 > L(16): nothing of read 16 is copied, 61 N remain
      L  15 -> 15    70  type 3  a loop: the row is the twin (the half with the higher index)
      F  19 -> 18    64  type 2  only from's degree is 1, L(to) odd; 24 entries with distPrevious 1
      C   6 -> 5, D 8 -> 7, I 10 -> 5   55   three rows of equal length: `from` ascending; D: both degrees 1; I: trimmed to 44 < 50, in the table and not in the file
      J  10 -> 3     52  type 3  trimmed to 41: not in the file
      A   2 -> 1     50  type 0  len == threshold; both degrees 1
    not rows: B 4 -> 3 (49 = threshold - 1); K 20 -> 16 (20: below the threshold; at a threshold of 20 or less it is `wrapped`: 20 < L(16) / 2).
    Every row but A is the TWIN of the record the file holds first; A's pair is written row first (a record that leaves the larger id).
    The pieces of every row add up to len and every nextDistance but H's is <= L(to): the reference itself stays in bounds."""
    ids = [11, 12, 13, 14, 17, 19, 20, 1, 2, 3, 4, 5]
    f_list = [(ids[j % len(ids)], j % 2, 0, 1, 1) for j in range(23)] + [(16, 1, 0, 1, 40)]
    rows = dict(
        G=H.rec(18, 16, 1, 2155, [(10, 1, 0, 37, 38), (10, 0, 0, 38, 2047), (10, 1, 0, 2047, 33)]),
        E=H.rec(18, 9, 3, 140, [(11, 1, 0, 20, 65), (12, 0, 0, 65, 30), (13, 1, 0, 30, 25)]),
        H=H.rec(17, 16, 0, 91, [(14, 1, 0, 30, 61)]),
        L=H.rec(15, 15, 3, 70, [(12, 0, 0, 40, 30)]),
        F=H.rec(19, 18, 2, 64, f_list),
        C=H.rec(6, 5, 2, 55, []), D=H.rec(8, 7, 3, 55, []), I=H.rec(10, 5, 1, 55, []), J=H.rec(10, 3, 3, 52, []), A=H.rec(2, 1, 0, 50, []),
        B=H.rec(4, 3, 1, 49, []), K=H.rec(20, 16, 0, 20, []))
    flows = dict(G=2.0, E=1.0, H=0.0, L=1.5, F=3.0, C=1.0, D=0.5, I=1.0, J=0.0, A=1e6, B=1.0, K=1.0)
    recs = []
    for name in "CGBEAHLFDIJK":
        r = dict(rows[name], flow=flows[name]); t = dict(H.twin_of(r), flow=flows[name])
        recs += [r, t] if name == "A" else [t, r]
    return recs


def hand_graph_parsed():
    return H.parse_graph(H.graph_text(HAND_HEADER, hand_contig_graph()))


# ------------------------------------------------------------------------------------------ tests
def test_restatement_on_the_hand_built_graph():
    ctx, seqs = hand_store(); ctx.close()
    rows, st, thr = contig_table(hand_graph_parsed(), seqs)
    rc = fx.revcomp
    assert thr == 50
    assert [(r["frm"], r["to"], r["len"]) for r in rows] == [(18, 16, 2155), (18, 9, 140), (17, 16, 91), (15, 15, 70), (19, 18, 64), (6, 5, 55), (8, 7, 55), (10, 5, 55), (10, 3, 52), (2, 1, 50)]
    assert [(r["start"], r["contig_length"], r["string_length"]) for r in rows] == [(31, 2156, 2216), (31, 171, 201), (0, 121, 151), (30, 70, 130), (0, 94, 124), (0, 85, 115),
                                                                                    (0, 115, 115), (19, 44, 92), (19, 41, 89), (0, 110, 110)]
    assert [(r["gaps"], r["ns"]) for r in rows] == [(2, 2011), (1, 5)] + [(0, 0)] * 8 and [r["written"] for r in rows] == [True] * 7 + [False, False, True]
    # pairs in graph4_save's order: nodes ascending, a node's halves with from <= to oldest first -- 1->2, 3->4, 3->10, 5->6, 5->10, 7->8, 9->18, 15->15 (twice), 16->18,
    # 16->17, 16->20, 18->19
    assert [r["pair"] for r in rows] == [9, 6, 10, 7, 12, 3, 5, 4, 2, 0]
    assert {n: st[n] for n in STAT_NAMES} == dict(contigs=10, written=8, bases=2156 + 171 + 121 + 70 + 94 + 85 + 115 + 110, longest=2156, n50=2156, n50_ordinal=1, n90=2156, n90_ordinal=1,
                                                  covered=2155 + 140 + 91 + 70 + 64 + 55 * 3 + 52 + 50, gaps=3, n_bases=2016, inconsistent=0, wrapped=0)
    # A: both reads reverse-complemented (type 0), the last 50 bases of the second
    assert rows[9]["string"] == "TCACTCTGGAGCTAAGGTGCCCGGCAGAACTCGACTTGTCAAATTAGATAGAGTGCTCTT" + "CGTCTTATCACACAGTTTAAGTTAGGCCGTTATCCGTAGATCTTATTTTT"
    assert rows[9]["string"] == rc(seqs[2]) + rc(seqs[1])[10:]
    # H: the first read reverse-complemented, the last 30 bases of read 14, then 61 N (distNext 61 > L: nothing copied)
    assert rows[2]["string"] == rc(seqs[17]) + seqs[14][30:] + "N" * 61
    assert rows[2]["string"] == "GGTTGAAGGTCCAAAGGACGCCCGTCCCAGTGAAATCCTCACCAGCTTCGTAAAACTTCC" + "TACCGGAGGTGATAATCGAGCTGTTTATGC" + "N" * 61
    # E: forward 61-base read; last 20 of 11; a gap of 5 N and read 12 reverse-complemented; last 30 of 13; last 25 of read 9, forward (type 3)
    assert rows[1]["string"] == seqs[18] + seqs[11][40:] + "NNNNN" + rc(seqs[12]) + seqs[13][30:] + seqs[9][35:]
    assert rows[1]["string"][61:61 + 20 + 5 + 12] == "TTAACGTTCTCACAGTAAAA" + "NNNNN" + "TGGTGTTAACCT"
    # G: the 61-base read reverse-complemented (type 1), the 37-base read whole, N + it reverse-complemented, 2010 N + it, the last 33 of read 16 forward
    assert rows[0]["string"] == rc(seqs[18]) + seqs[10] + "N" + rc(seqs[10]) + "N" * 2010 + seqs[10] + seqs[16][27:]
    # F: 23 single bases, the last base of each entry's read as it is oriented, then the last base of read 16, then the last 40 of the 61-base read reverse-complemented
    ids = [11, 12, 13, 14, 17, 19, 20, 1, 2, 3, 4, 5]
    assert rows[4]["string"] == seqs[19] + "".join((seqs[ids[j % 12]] if j % 2 else rc(seqs[ids[j % 12]]))[-1] for j in range(23)) + seqs[16][-1] + rc(seqs[18])[21:]
    # L: the second half of the loop's pair, type 3 (both ends forward): the last 40 of read 12 reverse-complemented, the last 30 of read 15
    assert rows[3]["type"] == 3 and rows[3]["string"] == seqs[15] + rc(seqs[12])[20:] + seqs[15][30:]
    text = fasta_text(rows)
    assert text.count(">") == 8 and ">contig_8 " not in text and ">contig_9 " not in text
    assert ">contig_1 flow=2 Edge length=2156 String length: 2216 e(18, 16) gapCount=2 nCount=2011\n" in text
    assert ">contig_10 flow=1e+06 Edge length=110 String length: 110 e(2, 1) gapCount=3 nCount=2016\n" in text
    # E: start + contig_length = 202 is one past the string: its last line has 50 characters, not 51
    e = text[text.index(">contig_2 "):text.index(">contig_3 ")].splitlines()
    assert e[0].endswith("Edge length=171 String length: 201 e(18, 9) gapCount=3 nCount=2016") and [len(x) for x in e[1:]] == [60, 60, 50] and "".join(e[1:]) == rows[1]["string"][31:]
    assert same_fasta_up_to_ties(text, rows) == 1


def test_thresholds_and_genome_size_of_the_restatement():
    ctx, seqs = hand_store(); ctx.close()
    g = hand_graph_parsed()
    rows, st, thr = contig_table(g, seqs, threshold=20, genome_size=5000)
    assert len(rows) == 12 and (rows[-1]["frm"], rows[-1]["to"], rows[-1]["wrapped"], rows[-1]["contig_length"], rows[-1]["written"]) == (20, 16, True, 0, False)
    assert rows[-2]["len"] == 49 and st["wrapped"] == 1 and st["written"] == 11
    assert (st["n50"], st["n50_ordinal"]) == (70, 4) and (st["n90"], st["n90_ordinal"]) == (0, 0)      # 2156 + 171 + 121 = 2448 < 2500 <= 2448 + 70; all rows sum to 3086 < 4500
    assert default_threshold(100) == 100 and default_threshold(58) == 58 and default_threshold(151) == 151


def test_struct_layout_against_the_header(tmp_path):
    """sizeof(sage2ov_contig) == 48 and every field where the Python mirrors put it, asked of the C compiler"""
    fields = ["from", "to", "pair", "edge_length", "string_length", "contig_length", "start", "gap_count", "n_count", "flow", "type", "pad"]
    stats = [n for n, _ in s2.ContigStats._fields_]
    src = tmp_path / "layout.c"; exe = tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sage2ov.h"\nint main(void) {\n  printf("%zu %zu\\n", sizeof(sage2ov_contig), sizeof(sage2ov_contig_stats));\n' +
                   "".join('  printf("%%zu\\n", offsetof(sage2ov_contig, %s));\n' % f for f in fields) +
                   "".join('  printf("%%zu\\n", offsetof(sage2ov_contig_stats, %s));\n' % f for f in stats) + "  return 0;\n}\n")
    subprocess.run(["gcc", "-I", os.path.join(fx.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    assert out[:2] == ["48", str(C.sizeof(s2.ContigStats))] and C.sizeof(s2.Contig) == 48 and s2.CONTIG_DTYPE.itemsize == 48
    assert [int(x) for x in out[2:2 + len(fields)]] == [s2.CONTIG_DTYPE.fields[f][1] for f in fields]
    assert [int(x) for x in out[2:2 + len(fields)]] == [getattr(s2.Contig, "from_" if f == "from" else f).offset for f in fields]
    assert [int(x) for x in out[2 + len(fields):]] == [getattr(s2.ContigStats, f).offset for f in stats]


def test_device_less_context_is_refused(tmp_path):
    ctx, _ = hand_store()
    calls = [lambda: ctx.contigs_build(), lambda: ctx.contigs_build(50, 1000), ctx.contigs_count, ctx.contigs, lambda: ctx.contig_sequences(0, 0, np.zeros(0, dtype=np.uint32)),
             lambda: ctx.contigs_save(str(tmp_path / "x.fasta"))]
    for call in calls:
        with pytest.raises(s2.Sage2ovError) as e:
            call()
        assert e.value.code == -3                                                    # SAGE2OV_ERR_DEVICE
    assert not os.path.exists(tmp_path / "x.fasta")
    assert ctx.contig_stats().contigs == 0
    ctx.close()
