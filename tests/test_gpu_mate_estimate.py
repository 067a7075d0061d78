"""GPU: reads on edges, mate flags, distances and insert sizes on the device (sage2ov_mates_map_reads / _estimate, sage2ov_graph_load_composite)
against the restatement of tests/test_mate_estimate_host.py over the text sage2ov_graph4_save wrote."""
import ctypes as C, glob, gzip, os, subprocess
import numpy as np
import pytest
import fixtures as fx
import sage2_amd as s2
import test_mate_estimate_host as H

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("minimiser_groups_on")]
GOLDEN4 = sorted(os.path.basename(p)[:-len(".graph4.gz")] for p in glob.glob(os.path.join(fx.GOLDEN, "*.graph4.gz")))


def add_mates(ctx, pairs):
    seqs = H.stored_reads(ctx)
    for L, pl in pairs.items():
        b, o = H.mates_ascii(pl, seqs); ctx.mates_add_ascii(b, o, L)


def check_all(ctx, text, pairs, valid=None):
    """table, flags, distances, rounds and bounds of the context against the restatement over `text`; -> the read-to-edge table as exported"""
    g = H.parse_graph(text); t = H.read_edge_table(g); arl = g["header"][2]; N = ctx.reads_stats().unique_reads
    want_d = {L: H.mate_distances(t, H.mate_entries(pl)) for L, pl in pairs.items()}
    for L in (valid or []):
        assert H.valid_every_round(want_d[L]), f"library {L}: a round with fewer than two distances"       # before the library is asked anything
    ent, loc, off = ctx.read_edges()
    keys = sorted(t)
    assert len(ent) == len(keys) and [(int(e["read"]), int(e["pair"])) for e in ent] == keys
    at = 0
    for e, k in zip(ent, keys):
        w = t[k]
        assert (e["from"], e["to"], e["type"], e["n_forward"], e["n_reverse"], e["location"]) == (w["frm"], w["to"], w["type"], len(w["forward"]), len(w["reverse"]), at), k
        assert loc[at:at + len(w["forward"])].tolist() == w["forward"] and loc[at + len(w["forward"]):at + len(w["forward"]) + len(w["reverse"])].tolist() == w["reverse"], k
        at += len(w["forward"]) + len(w["reverse"])
    assert at == len(loc) and len(off) == N + 2 and int(off[N + 1]) == len(ent)
    reads = ent["read"].astype(np.int64)
    assert np.array_equal(off, np.searchsorted(reads, np.arange(N + 2)))
    st = ctx.readmap_stats()
    assert (st.entries, st.locations, st.records, st.route) == (len(ent), len(loc), len(loc), s2.MATE_ROUTE_DEVICE)
    ests = []
    for L, pl in pairs.items():
        m, _ = ctx.mates(L); mt = [(int(a), int(b)) for a, b in zip(m["from"], m["to"])]
        assert mt == H.mate_entries(pl)
        assert ctx.mates_flags(L).tolist() == H.mate_flags(t, mt)
        assert ctx.mates_distances(L).tolist() == want_d[L]
    ctx.mates_estimate()
    nlib = max(pairs) if pairs else 0
    for L in range(1, nlib + 1):
        w = H.estimate(want_d.get(L, []), arl); ests.append(w)
        H.same_estimate(ctx.mates_insert(L), w); assert ctx.mates_insert(L).library == L
        H.same_estimate(s2.insert_estimate(np.asarray(want_d.get(L, []), dtype=np.uint32), arl), w)
    for L in (valid or []):
        assert ests[L - 1]["valid"] == 1
    assert ctx.mates_bounds() == H.bounds(ests, arl)
    return ent, loc, off


@pytest.fixture(scope="module")
def goldens():
    """steps 1-4 on the device for a golden, its written P.graph4, mates from the graph: computed once per golden and shared"""
    cache = {}

    def get(name, tmp):
        if name not in cache:
            m = fx.golden(name); bases, off = fx.make_reads(m["synth"])
            ctx = s2.Context(m["k"]); ctx.reads_add_ascii(bases, off); ctx.reads_organize(); ctx.run_steps23(); ctx.graph_simplify()
            out = str(tmp / (name + ".graph4")); ctx.graph4_save(out); text = open(out, "rb").read()
            assert text == gzip.open(os.path.join(fx.GOLDEN, name + ".graph4.gz")).read()
            pairs = H.pairs_from_graph(H.parse_graph(text), 11, ctx.reads_stats().unique_reads)
            cache[name] = (ctx, text, pairs)
        return cache[name]
    yield get
    for ctx, _, _ in cache.values():
        ctx.close()


@pytest.mark.parametrize("name", ["g1_clean100_k21", "g3_noisy_rep_k21", "g4_highcopy_k21", "g7_palindrome_tandem_k21"])
def test_steps_1_to_4_then_mates_map_estimate(name, goldens, tmp_path_factory):
    """g1: one list of 15 632 entries (scan blocks of 2048, radix tiles of 2048); g7: a loop edge (E = the half with the higher index) and a read on two pairs"""
    ctx, text, pairs = goldens(name, tmp_path_factory.mktemp("g"))
    ctx.mates_clear(); add_mates(ctx, pairs)
    before = (text, ctx.edges().tobytes(), [ctx.mates(L)[0].tobytes() for L in pairs])
    ctx.mates_map_reads()
    ent, _, _ = check_all(ctx, text, pairs, valid=[1, 2])
    if name.startswith("g1"):
        assert max(len(a["list"]) for _, a, _ in H.parse_graph(text)["pairs"]) == 15632
    if name.startswith("g7"):
        g = H.parse_graph(text); loops = [q for q, a, _ in g["pairs"] if a["frm"] == a["to"]]
        assert len(loops) == 1 and len(H.parse_graph(text, fold=False)["pairs"]) == len(g["pairs"]) + 1
        assert any(int(e["pair"]) == loops[0] for e in ent)
    # nothing steps 2-4 or the mate table hold has changed
    out = str(tmp_path_factory.mktemp("s") / "again.graph4"); ctx.graph4_save(out)
    assert (open(out, "rb").read(), ctx.edges().tobytes(), [ctx.mates(L)[0].tobytes() for L in pairs]) == before


def random_store(n, seed, L=60, k=40):
    rng = np.random.default_rng(seed)
    a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n + n // 8, L))]
    reads = sorted({r.tobytes().decode() for r in a})[:n]
    assert len(reads) == n
    bases = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy(); off = np.arange(0, (n + 1) * L, L, dtype=np.uint64)
    ctx = s2.Context(k); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
    assert ctx.reads_stats().unique_reads == n
    return ctx


def load_text(ctx, text, tmp_path, name="h.graph4"):
    p = str(tmp_path / name); open(p, "w").write(text); ctx.graph_load_composite(p)
    return p


def test_hand_built_graph_through_the_loader(tmp_path):
    """a read on three pairs, a read twice on one edge, orientation 0, a record that leaves the larger id, loops written once and twice, two libraries"""
    N, header, recs = H.hand_graph(); text = H.graph_text(header, recs)
    ctx = random_store(N, 5); load_text(ctx, text, tmp_path)
    out = str(tmp_path / "o.graph4"); ctx.graph4_save(out)
    saved = open(out).read(); g = H.parse_graph(saved)
    assert len(g["pairs"]) == 6 and saved != text                                   # (the loop that was written once is written twice now; the record leaving 5 is its twin's twin)
    s4 = ctx.simplify_stats(); assert (s4.edges, s4.reads_on_edges) == (6, 5 + 6 + 3 + 2 + 3)
    pairs = {1: [(20, 1, 24, 1), (20, 0, 22, 1), (21, 1, 23, 0), (22, 1, 24, 1), (30, 1, 31, 1), (31, 1, 33, 1), (32, 0, 33, 1), (40, 1, 41, 1), (20, 1, 40, 0), (42, 1, 43, 1),
                 (44, 1, 46, 1), (45, 0, 46, 0), (1, 1, 20, 1), (50, 1, 51, 1), (30, 1, 30, 0), (20, 1, 24, 1)],
             2: [(44, 1, 45, 1), (31, 1, 32, 1), (23, 1, 24, 1), (24, 0, 23, 1), (52, 1, 20, 1)]}
    add_mates(ctx, pairs)
    ent, loc, off = check_all(ctx, saved, pairs, valid=[1, 2])
    assert off[21] - off[20] == 3 and ent[off[30]]["n_forward"] == 2 and (loc < 0).any()
    with pytest.raises(s2.Sage2ovError) as e:
        ctx.graph_simplify()
    assert e.value.code == -1
    ctx.close()


def test_long_list_invalid_library_and_empty_table(tmp_path):
    """a list of 8 193 entries (four scan blocks and radix tiles plus one entry); library 2 has one distance next to the valid library 1 and is left out of
    the bounds; library 3 lies beyond the libraries in use; before any mate is added the flags and distances are empty and nothing is valid"""
    n = 8193; N = n + 10; rng = np.random.default_rng(3)
    lst = [(i + 3, int(rng.integers(0, 2)), 0, int(rng.integers(1, 2048)), int(rng.integers(0, 2048))) for i in range(n)]
    long_ = H.rec(1, 2, 3, 1000, lst); short = H.rec(2, N, 3, 100, [(n + 5, 1, 0, 7, 8), (n + 6, 1, 0, 9, 10)])
    text = H.graph_text((0, 2 * N, 60), [long_, H.twin_of(long_), short, H.twin_of(short)])
    ctx = random_store(N, 9); load_text(ctx, text, tmp_path)
    out = str(tmp_path / "o.graph4"); ctx.graph4_save(out); assert open(out).read() == text
    ctx.mates_map_reads()
    assert ctx.mates_flags(1).size == 0 and ctx.mates_distances(1).size == 0
    ctx.mates_estimate(); assert ctx.mates_bounds() == (1000000, 0)
    pairs = {1: [(3 + i, 1, 3 + i + d, 0) for i, d in zip(range(0, 8000, 97), range(1, 100))] + [(3, 1, n + 2, 1)], 2: [(n + 5, 1, n + 6, 1), (5, 1, n + 5, 1)]}
    add_mates(ctx, pairs)
    check_all(ctx, text, pairs, valid=[1])
    assert ctx.mates_insert(2).valid == 0 and ctx.mates_insert(2).considered[0] == 1 and ctx.mates_insert(1).valid == 1
    assert ctx.mates_bounds()[0] == ctx.mates_insert(1).upper
    assert ctx.readmap_stats().distances[1] == len(pairs[1]) and ctx.readmap_stats().sort_passes == 2 + 1      # reads below 2^14: two digits; 2 pairs and the side: one
    ctx.close()


@pytest.mark.parametrize("name", GOLDEN4)
def test_load_then_save_is_byte_identical(name, tmp_path):
    assert len(GOLDEN4) == 13
    m = fx.golden(name); bases, off = fx.make_reads(m["synth"])
    ctx = s2.Context(m["k"]); ctx.reads_add_ascii(bases, off); ctx.reads_organize()
    text = gzip.open(os.path.join(fx.GOLDEN, name + ".graph4.gz")).read()
    assert all(a["flow"] == 0 and b["flow"] == 0 for _, a, b in H.parse_graph(text, fold=False)["pairs"])
    src = str(tmp_path / "in.graph4"); open(src, "wb").write(text)
    ctx.graph_load_composite(src)
    out = str(tmp_path / "out.graph4"); ctx.graph4_save(out)
    assert open(out, "rb").read() == text
    ctx.close()


def test_loader_refusals(tmp_path):
    N, header, recs = H.hand_graph(); ctx = random_store(N, 5)
    good = H.graph_text(header, recs)

    def refused(text, code, name):
        with pytest.raises(s2.Sage2ovError) as e:
            load_text(ctx, text, tmp_path, name)
        assert e.value.code == code, str(e.value)
    bad = [dict(r) for r in recs]; bad[1] = dict(bad[1], list=[bad[1]["list"][1], bad[1]["list"][0]] + bad[1]["list"][2:])
    refused(H.graph_text(header, bad), -1, "twin_order")
    bad = [dict(r) for r in recs]; bad[3] = dict(bad[3], list=bad[3]["list"][:-1])
    refused(H.graph_text(header, bad), -1, "twin_length")
    bad = [dict(r) for r in recs]; bad[0] = dict(bad[0], list=[(N + 1,) + bad[0]["list"][0][1:]] + bad[0]["list"][1:]); bad[1] = H.twin_of(bad[0])
    refused(H.graph_text(header, bad), -1, "read_above_n")
    bad = [dict(r) for r in recs]; bad[12] = H.rec(8, N + 1, 3, 40, []); bad[13] = H.twin_of(bad[12])
    refused(H.graph_text(header, bad), -1, "node_above_n")
    refused(good[:good.index("\n", good.index("21\t0\t0"))][:-2], -1, "cut_in_a_list")
    refused(H.graph_text(header, recs[:-1]), -1, "no_twin")
    for field in (3, 4):
        bad = [dict(r) for r in recs]; e0 = list(bad[0]["list"][0]); e0[field] = 2048; bad[0] = dict(bad[0], list=[tuple(e0)] + bad[0]["list"][1:]); bad[1] = H.twin_of(bad[0])
        refused(H.graph_text(header, bad), -5, "dist_%d" % field)
    refused("", -2, "empty")
    with pytest.raises(s2.Sage2ovError) as e:
        ctx.graph_load_composite(str(tmp_path / "missing"))
    assert e.value.code == -2
    load_text(ctx, good, tmp_path); ctx.mates_map_reads(); assert ctx.readmap_stats().entries > 0      # a refusal leaves the context usable
    ctx.close()
    c2 = s2.Context(40); p = str(tmp_path / "g"); open(p, "w").write(good)
    with pytest.raises(s2.Sage2ovError) as e:
        c2.graph_load_composite(p)
    assert e.value.code == -1 and "organise" in str(e.value)
    c2.close()


def test_call_order_staleness_and_device_less_context(tmp_path):
    m3 = fx.golden("g3_noisy_rep_k21"); bases, off = fx.make_reads(m3["synth"])
    ctx = s2.Context(m3["k"]); ctx.reads_add_ascii(bases, off); ctx.reads_organize(); ctx.run_steps23(); ctx.graph_simplify()      # (a context of its own: it loses its graph below)
    out = str(tmp_path / "t.graph4"); ctx.graph4_save(out); text = open(out, "rb").read()
    pairs = H.pairs_from_graph(H.parse_graph(text), 11, ctx.reads_stats().unique_reads)
    add_mates(ctx, {1: pairs[1]})
    ctx.mates_map_reads(); f1 = ctx.mates_flags(1); n1 = ctx.readmap_stats().entries; assert n1 > 0 and (f1 == 0).any()
    with pytest.raises(s2.Sage2ovError):
        ctx.mates_insert(1)                                                           # nothing estimated yet
    # mates added after a map: the next export has the flags of the larger table
    seqs = H.stored_reads(ctx); b, o = H.mates_ascii(pairs[2], seqs); ctx.mates_add_ascii(b, o, 1)
    t = H.read_edge_table(H.parse_graph(text)); m, _ = ctx.mates(1)
    f2 = ctx.mates_flags(1); assert len(f2) > len(f1) and f2.tolist() == H.mate_flags(t, list(zip(m["from"].tolist(), m["to"].tolist())))
    ctx.mates_estimate(); assert ctx.mates_insert(1).valid == 1
    # the table goes with the graph: graph_simplify and overlap_convert
    ctx.graph_simplify(); assert ctx.readmap_stats().entries == 0
    ctx.mates_map_reads(); assert ctx.readmap_stats().entries == n1
    ctx.overlap_convert(); assert ctx.readmap_stats().entries == 0
    with pytest.raises(s2.Sage2ovError):
        ctx.mates_insert(1)
    ctx.graph_simplify(); assert len(ctx.read_edges()[0]) == n1                        # (an export maps when the table is stale)
    # ... and with the read set
    rp = str(tmp_path / "t.reads"); ctx.reads_save(rp); ctx.reads_load(rp)
    for call in (ctx.mates_map_reads, ctx.mates_estimate, ctx.read_edges):
        with pytest.raises(s2.Sage2ovError) as e:
            call()
        assert e.value.code == -1
    ctx.close()
    # no graph at all; a device-less context
    c2 = random_store(50, 1)
    for call in (c2.mates_map_reads, c2.mates_estimate, c2.read_edges, lambda: c2.mates_flags(1), lambda: c2.mates_distances(1)):
        with pytest.raises(s2.Sage2ovError) as e:
            call()
        assert e.value.code == -1
    c2.close()
    c3 = s2.Context(40, device=-2); c3.reads_add_ascii(bases[:int(off[200])], off[:201]); c3.reads_organize()
    p = str(tmp_path / "g"); open(p, "wb").write(text)
    for call in (c3.mates_map_reads, c3.mates_estimate, c3.read_edges, lambda: c3.graph_load_composite(p)):
        with pytest.raises(s2.Sage2ovError) as e:
            call()
        assert e.value.code == -3
    c3.close()


def test_memory_diet_mode_gives_the_same_tables(monkeypatch, goldens, tmp_path_factory, tmp_path):
    ctx, text, pairs = goldens("g4_highcopy_k21", tmp_path_factory.mktemp("g"))
    ctx.mates_clear(); add_mates(ctx, pairs); ctx.mates_map_reads()
    want = [x.tobytes() for x in ctx.read_edges()] + [ctx.mates_flags(L).tobytes() + ctx.mates_distances(L).tobytes() for L in pairs]
    monkeypatch.setenv("SAGE2OV_MEMORY_DIET", "1")
    m = fx.golden("g4_highcopy_k21"); bases, off = fx.make_reads(m["synth"])
    c2 = s2.Context(m["k"]); c2.reads_add_ascii(bases, off); c2.reads_organize(); c2.run_steps23(); c2.graph_simplify()
    add_mates(c2, pairs)
    ent, loc, off2 = check_all(c2, text, pairs, valid=[1, 2])
    assert [x.tobytes() for x in (ent, loc, off2)] + [c2.mates_flags(L).tobytes() + c2.mates_distances(L).tobytes() for L in pairs] == want
    c2.close()


MIRROR_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include "sage2ov.hpp"
int main(int argc, char** argv) {
    using namespace sage2ov;
    Context ctx((uint16_t)atoi(argv[1]), atoi(argv[2]));
    ReadLoader loader(ctx); loader.readDatasetInBytes(argv[3]); loader.organizeReads();
    OverlapGraph graph(&loader); graph.loadCompositeGraphFromFile(argv[4]);
    MatePair mates(&loader); mates.mapMatePairs(argv[5], "", 1);
    mates.meanSdEstimation();
    for (uint64_t r = 0; r <= loader.numberOfUniqueReads; r++)
        for (const sage2ov_read_edge& e : mates.readToEdgeList(r)) {
            printf("e %u %u %u %u %u", e.read, e.pair, e.from, e.to, (unsigned)e.type);
            for (int32_t v : mates.locations(e, true)) printf(" f%d", v);
            for (int32_t v : mates.locations(e, false)) printf(" r%d", v);
            const std::vector<int32_t> d = mates.findDistanceOnEdge(e.pair, r);
            printf(" | %d\n", d[0]);
        }
    printf("not there %d\n", mates.findDistanceOnEdge(0, 59)[0]);
    printf("lib %u %u %d %d %llu %llu\n", mates.Mean[1], mates.standardDeviation[1], mates.lowerBoundOfInsert[1], mates.upperBoundOfInsert[1],
           (unsigned long long)mates.minimumUpperBoundOfInsert, (unsigned long long)mates.maximumUpperBoundOfInsert);
    return 0;
}
"""


def test_cpp_mirror(tmp_path):
    """sage2ov.hpp compiles, and MatePair's members print the restatement's table and insert size"""
    N, header, recs = H.hand_graph(); text = H.graph_text(header, recs)
    ctx = random_store(N, 5); seqs = H.stored_reads(ctx)
    load_text(ctx, text, tmp_path, "py.graph4"); sp = str(tmp_path / "saved.graph4"); ctx.graph4_save(sp); saved = open(sp).read(); ctx.close()      # (pair ordinals are those of the written file)
    fa, gp, mf = str(tmp_path / "r.fa"), str(tmp_path / "h.graph4"), str(tmp_path / "m.fa")
    open(fa, "w").write("".join(">r%d\n%s\n" % (i, seqs[i]) for i in sorted(seqs))); open(gp, "w").write(text)
    pl = [(20, 1, 24, 1), (21, 1, 23, 0), (22, 1, 24, 1), (31, 1, 33, 1), (40, 1, 41, 1), (44, 1, 46, 1)]
    b, o = H.mates_ascii(pl, seqs); open(mf, "w").write("".join(">m%d\n%s\n" % (i, b[int(o[i]):int(o[i + 1])].tobytes().decode()) for i in range(len(o) - 1)))
    src, exe = str(tmp_path / "mirror.cpp"), str(tmp_path / "mirror"); open(src, "w").write(MIRROR_CPP)
    libdir = os.path.join(fx.ROOT, "sage2_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(fx.ROOT, "include"), "-I", os.path.join(libdir, "csrc"), src, "-o", exe,
                    "-L", libdir, "-lsage2ov", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe, "40", "0", fa, gp, mf], check=True, stdout=subprocess.PIPE, text=True, timeout=120).stdout.splitlines()
    g = H.parse_graph(saved); t = H.read_edge_table(g)
    want = ["e %d %d %d %d %d" % (r, q, w["frm"], w["to"], w["type"]) + "".join(" f%d" % v for v in w["forward"]) + "".join(" r%d" % v for v in w["reverse"]) + " | %d" % len(w["forward"])
            for (r, q), w in sorted(t.items())]
    e = H.estimate(H.mate_distances(t, H.mate_entries(pl)), header[2]); lo, hi = H.bounds([e], header[2])
    assert e["valid"] == 1
    assert out == want + ["not there 0", "lib %d %d %d %d %d %d" % (e["mean"], e["deviation"], e["lower"], e["upper"], lo, hi)]
