"""The step-4 restatement (oracle/step4_oracle.cpp) against graphs dumped by the reference's own classes (tests/golden/*.graph4.gz,
made by oracle/make_golden_step4.py): byte identity of the whole file, i.e. the surviving edges, their read lists and their order."""
import ctypes, gzip, hashlib, json, os
import pytest
import fixtures as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    p = os.path.join(ROOT, "oracle", "liboracle_step4.so")
    if not os.path.exists(p):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "liboracle_step4.so"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(p)
    lib.orc4_run_files.argtypes = [ctypes.c_char_p, ctypes.c_ulonglong, ctypes.c_char_p, ctypes.POINTER(ctypes.c_ulonglong)]
    return lib


@pytest.mark.parametrize("name", fx.golden_names())
def test_step4_restatement_equals_reference_dump(name, tmp_path):
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", name + ".step4.json")))
    g3 = tmp_path / "t.graph3"; g3.write_bytes(fx.golden_graph3(name))
    out = tmp_path / "t.graph4"
    c = (ctypes.c_ulonglong * 5)()
    assert _lib().orc4_run_files(str(g3).encode(), meta["counters"]["unique_reads"], str(out).encode(), c) == 0
    want = gzip.open(os.path.join(ROOT, "tests", "golden", name + ".graph4.gz")).read()
    got = out.read_bytes()
    assert hashlib.md5(want).hexdigest() == meta["graph4_md5"]
    assert c[1] == meta["counters"]["loop_iterations"] and c[2] == meta["counters"]["nodes_contracted"] and c[3] == meta["counters"]["removed"]
    assert got == want


def _ref_driver():
    p = os.path.join(ROOT, "oracle", "_ref", "libsage2ref_driver.so")
    if not os.path.exists(p):
        pytest.skip("oracle/_ref not built (the reference is only present in the build container)")
    drv = ctypes.CDLL(p)
    if not hasattr(drv, "sage2ref_run_step4"):
        pytest.skip("oracle/_ref predates the step-4 driver")
    drv.sage2ref_run_step4.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_ulonglong)]
    return drv


@pytest.mark.parametrize("seed", range(24))
def test_step4_restatement_equals_reference_on_synthetic_graphs(seed, tmp_path):
    """cycles, closed and parallel chains, tips, multi-edges, nodes that do not combine -- ids scattered (tests/graphgen.py); the reference's
    classes run in process through oracle/_ref (build container only)"""
    import graphgen as gg
    drv = _ref_driver()
    N, e = gg.random_graph(seed, n_anchor=8 + 3 * seed, n_paths=20 + 6 * seed, max_len=3 + seed % 9, n_cycles=seed % 4, p_bad=0.02 * (seed % 3))
    pre = str(tmp_path / "t"); gg.write_graph3(pre + ".graph3", N, e); gg.write_reads(pre + ".reads", N, seed=seed)
    t = (ctypes.c_double * 2)(); c = (ctypes.c_ulonglong * 4)()
    assert drv.sage2ref_run_step4(pre.encode(), 40, 1, (pre + ".ref4").encode(), t, c) == 0
    c2 = (ctypes.c_ulonglong * 5)()
    assert _lib().orc4_run_files((pre + ".graph3").encode(), N, (pre + ".orc4").encode(), c2) == 0
    assert (c[1], c[2], c[3]) == (c2[1], c2[2], c2[3])
    assert open(pre + ".orc4", "rb").read() == open(pre + ".ref4", "rb").read()


# ---- the directed families of tests/graphgen.py: do they reach the branches they are built for (the restatement's own counters, no
# device), and is the restatement right on them (the reference's classes)
def _lib_ex():
    lib = _lib()
    lib.orc4_run_files_ex.argtypes = [ctypes.c_char_p, ctypes.c_ulonglong, ctypes.c_char_p, ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_ulonglong)]
    return lib


def _counted(N, e, tmp_path):
    import graphgen as gg
    g3 = str(tmp_path / "t.graph3"); gg.write_graph3(g3, N, e)
    c = (ctypes.c_ulonglong * 5)(); ex = (ctypes.c_ulonglong * 22)()
    assert _lib_ex().orc4_run_files_ex(g3.encode(), N, str(tmp_path / "t.graph4").encode(), c, ex) == 0
    return list(c), dict(zip(gg.COUNTERS, ex)), str(tmp_path / "t.graph4")


def _edge_ends(path):
    """the nodes that are an end of a surviving edge (not the reads lying on one)"""
    ends = set(); lines = open(path).read().split("\n")[3:]; x = 0
    while x < len(lines):
        if not lines[x]: x += 1; continue
        f = lines[x].split("\t"); ends.add(int(f[0])); ends.add(int(f[1])); x += 1 + int(f[6])
    return ends


# removals happen once per designed case, so their counters are known exactly; the others count visits (a kept node is judged again in
# every later sweep) and have the built count as their floor
EXACT = ("dead0", "dead1", "dead2", "dead3", "dec1", "dec2") + tuple(f"dec{s}_{c}" for s in (1, 2) for c in (10, 20, 30, 40, 50))
LOOP_ITERATIONS = {"B": 1, "BL": 6, "BM": 1, "BC": 4, "D": 5, "DC": 300, "TB": 1, "TL": 6}


def _check_floors(L, c, ex, g4):
    assert L.built, "a family that books nothing checks nothing"
    for k, v in L.built.items():
        assert (ex[k] == v) if k in EXACT else (ex[k] >= v), (k, ex[k], v)
    for k in EXACT:
        assert ex[k] == L.built.get(k, 0), (k, ex[k])
    assert c[3] == sum(ex[k] for k in ("dead0", "dead1", "dead2", "dead3", "dec1", "dec2"))
    ends = _edge_ends(g4)
    assert L.keep and not [v for v in L.keep if v not in ends]
    assert not [v for v in L.gone if v in ends]


@pytest.mark.parametrize("name", ["B", "BL", "BM", "BC", "D", "DC", "TB", "TL"])
@pytest.mark.parametrize("seed", [0, 1])
def test_directed_family_reaches_its_branches(name, seed, tmp_path):
    """every removal the generator designed happens, in the sweep it was designed for, and nothing else is removed; the nodes meant to stay
    are still ends of edges (tiers 50 and 51, the four-read tip, the nodes only a loop keeps, the node behind a far first edge, ...)"""
    import graphgen as gg
    L = gg.layout([name], seed, interleave=bool(seed))          # seed 0 in sequence, seed 1 interleaved: the graphs of the device test
    N, e = gg.compose([name], seed, interleave=bool(seed))
    assert N == L.N and e.tobytes() == L.edges.tobytes()
    c, ex, g4 = _counted(N, e, tmp_path)
    _check_floors(L, c, ex, g4)
    assert c[1] == LOOP_ITERATIONS[name]
    if name == "B":                                            # both sides, with odd and even halves on each: 7 cases each out of 56
        assert ex["dec1"] == 7 and ex["dec2"] == 7 and ex["undecided"] >= 42
    if name == "BL":
        assert all(ex[f"dec{s}_{t}"] == 2 for s in (1, 2) for t in gg.TIERS)
    if name in ("TB", "TL"):
        assert (e["length"] != e["length_twin"]).sum() > len(e) // 2
    if name == "D":
        assert all(ex[f"dead{t}"] >= 2 for t in range(4)) and ex["loop_keep"] >= 2


def test_composed_graph_reaches_every_branch(tmp_path):
    """all families over interleaved ids, three copies: every counter the families book is reached at least as often as built"""
    import graphgen as gg
    L = gg.composed_layout(seed=5, copies=3)
    c, ex, g4 = _counted(L.N, L.edges, tmp_path)
    _check_floors(L, c, ex, g4)
    assert all(L.built.get(k, 0) >= 3 for k in gg.COUNTERS), {k: L.built.get(k, 0) for k in gg.COUNTERS}


def test_random_graphs_hardly_reach_them(tmp_path):
    """the measurement behind the families: on the 40 random graphs of the device test no bubble node ever loses its own two edges, and few
    graphs get past threshold 0"""
    import graphgen as gg
    tot = {k: 0 for k in gg.COUNTERS}; past0 = 0
    for seed in range(40):
        N, e = gg.random_graph(seed, n_anchor=8 + 3 * seed, n_paths=20 + 6 * seed, max_len=3 + seed % 9, n_cycles=seed % 4, p_bad=0.02 * (seed % 3))
        c, ex, _ = _counted(N, e, tmp_path)
        for k in tot: tot[k] += ex[k]
        past0 += c[1] > 1
    print(tot, past0)
    assert tot["dec1"] == 0 and past0 <= 5


@pytest.mark.parametrize("name", ["B", "BL", "BM", "BC", "D", "DC", "TB", "TL", "ALL"])
def test_step4_restatement_equals_reference_on_directed_families(name, tmp_path):
    """the families reach branches on which the restatement was never pinned before; the reference's classes run in process through
    oracle/_ref (build container only).  No difference was found on any family."""
    import graphgen as gg
    drv = _ref_driver()
    L = gg.composed_layout(seed=3, copies=2) if name == "ALL" else gg.layout([name], 4, interleave=name not in ("DC",))
    pre = str(tmp_path / "t"); gg.write_graph3(pre + ".graph3", L.N, L.edges); gg.write_reads(pre + ".reads", L.N, seed=7)
    t = (ctypes.c_double * 2)(); c = (ctypes.c_ulonglong * 4)()
    assert drv.sage2ref_run_step4(pre.encode(), 40, 1, (pre + ".ref4").encode(), t, c) == 0
    c2 = (ctypes.c_ulonglong * 5)()
    assert _lib().orc4_run_files((pre + ".graph3").encode(), L.N, (pre + ".orc4").encode(), c2) == 0
    assert (c[1], c[2], c[3]) == (c2[1], c2[2], c2[3])
    assert open(pre + ".orc4", "rb").read() == open(pre + ".ref4", "rb").read()
