"""CPU: sage2ov_reads_find_ids (ReadLoader::getIdOfRead, readLoader.cpp:319-353, for a batch of queries) on a device-less context, which answers with the reference's
own method -- a binary search over the host copy of the sorted read list.  The expected value is a restatement of readLoader.cpp:319-353 written here
(`expected_ids`): a dictionary from the canonical string of every exported read to its id; a query that is not a good read (utils.cpp:144-166) gives 0, any other one
dict.get(min(q, revcomp(q))) with sign + iff q < revcomp(q), on upper-cased strings.  The cases are functions of the device ordinal: tests/test_gpu_find_ids.py runs
the same ones against the HIP path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fixtures as fx
import sage2_amd as s2

HOST = -2                                                                # SAGE2OV_DEVICE_NONE
LAYOUT_TOPS = [(123, 4), (251, 8), (504, 16), (1018, 32)]                # (longest read of the layout, words per read): the values of tests/test_gpu_edges.py
FIND_B_MIN, FIND_B_MAX = 4, 24                                           # kernels_find.inc


# ---------------------------------------------------------------------------------------------------------------- the expected value
def to_arrays(queries):
    bases = np.frombuffer("".join(queries).encode(), dtype=np.uint8).copy()
    off = np.zeros(len(queries) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(q) for q in queries])
    return bases, off


def input_reads(bases, off):
    return [bytes(bases[int(off[i]):int(off[i + 1])]).decode() for i in range(len(off) - 1)]


def stored_reads(ctx):
    """[None, read 1, read 2, ...]: the exported store (MSB-first 2-bit bytes, utils.cpp:96) as strings"""
    packed, length, _ = ctx.reads_export()
    codes = np.stack([(packed >> s) & 3 for s in (6, 4, 2, 0)], axis=2).reshape(packed.shape[0], -1)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    return [None] + [bytes(text[i, :int(length[i])]).decode() for i in range(1, packed.shape[0])]


def expected_ids(ctx, queries, k):
    """readLoader.cpp:319-353, restated"""
    table = {s: i for i, s in enumerate(stored_reads(ctx)) if i}
    out = np.zeros(len(queries), dtype=np.int64)
    for r, q in enumerate(queries):
        q = q.upper()
        if len(q) <= k or set(q) - set("ACGT"):
            continue                                                     # not a good read (utils.cpp:144-166)
        rc = fx.revcomp(q)
        out[r] = table.get(min(q, rc), 0) * (1 if q < rc else -1)        # :325: strictly smaller, else the reverse complement
    return out


def organised(k, reads, device):
    ctx = s2.Context(k, device=device)
    bases, off = reads if isinstance(reads, tuple) else to_arrays(reads)
    ctx.reads_add_ascii(bases, off); ctx.reads_organize()
    return ctx


def find(ctx, queries):
    return ctx.reads_find_ids(*to_arrays(queries))


def check(ctx, queries, k):
    """the call's answer is the restatement's; the stats add up; returns the ids"""
    got, want = find(ctx, queries), expected_ids(ctx, queries, k)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} of {len(queries)} ids differ, first: query {bad[0]} ({queries[bad[0]][:60]!r}, {len(queries[bad[0]])} bases) got {got[bad[0]]} want {want[bad[0]]}"
    st = ctx.reads_find_stats()
    good = sum(1 for q in queries if len(q) > k and not (set(q.upper()) - set("ACGT")))
    assert (st.queries, st.found, st.not_good, st.not_found) == (len(queries), int((want != 0).sum()), len(queries) - good, good - int((want != 0).sum()))
    return got


def rnd(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n))


def change_last(s):
    return s[:-1] + ("C" if s[-1] != "C" else "G")


# ---------------------------------------------------------------------------------------------------------------- the cases (device: a HIP ordinal, or HOST)
def case_every_input_read_finds_itself(device, L, k):
    bases, off = fx.make_reads(dict(recipe="tiling", seed=4100 + L, n_unique=3000, read_len=L, step=7, dup_every=7, dup_copies=2))
    ctx = organised(k, (bases, off), device)
    assert ctx.reads_stats().unique_reads == 3000
    queries = input_reads(bases, off)                                    # both strands (the tiling alternates) and the duplicates
    ids = check(ctx, queries, k)
    assert np.all(ids != 0) and ctx.reads_find_stats().found == len(queries)
    assert np.all((ids > 0) == np.array([q < fx.revcomp(q) for q in queries]))
    assert (ids > 0).sum() > 1000 and (ids < 0).sum() > 1000
    assert set(np.abs(ids)) == set(range(1, 3001))
    ctx.close()


def case_compare_is_bytes_then_length(device):
    k, top = 21, 123
    ctx = organised(k, fx.make_reads(dict(recipe="short_reads", seed=4200, k=k, top=top, step=5, n_reads=900)), device)
    store = stored_reads(ctx); rng = np.random.default_rng(4201)
    assert ctx.reads_stats().max_read_length == top
    short = [s for s in store[1:] if len(s) < top and len(s) % 4 != 0 and not s.startswith("T")]
    assert len(short) > 100
    queries = []
    for s in short[:150] + [s for s in store[1:] if len(s) == top][:50]:
        # s + "A": the packed bytes equal those of s with zero padding (A = 00), only the length differs -- unless the extra base flips the orientation
        queries += [s, s[:-1], s + "A", change_last(s), fx.revcomp(s[:-1]), fx.revcomp(s + "A"), "T" + fx.revcomp(s)]
    same_bytes = sum(1 for s in short[:150] if s + "A" < fx.revcomp(s + "A"))
    assert same_bytes > 100, "queries whose canonical form is a stored read plus one zero base"
    queries += [rnd(rng, top + 1), rnd(rng, 1018), rnd(rng, 1019), rnd(rng, 1100), rnd(rng, 5000), store[1] + rnd(rng, 1000)]      # longer than the store's longest read, than any layout
    ids = check(ctx, queries, k)
    assert np.all(ids[-6:] == 0) and (ids != 0).sum() >= 200
    ctx.close()


def case_bad_and_odd_queries(device):
    k, top = 21, 123
    ctx = organised(k, fx.make_reads(dict(recipe="short_reads", seed=4300, k=k, top=top, step=5, n_reads=900)), device)
    store = stored_reads(ctx)
    shortest = [s for s in store[1:] if len(s) == k + 1]; longest = [s for s in store[1:] if len(s) == top]
    assert len(shortest) >= 20 and len(longest) >= 20
    queries = []
    for s in shortest[:20] + longest[:20]:
        m = len(s) // 2
        queries += [s, fx.revcomp(s), s[:k], s[:k - 1], s[:1], "",                                    # exactly k + 1 (the shortest good read); length <= k; empty
                    "N" + s[1:], s[:m] + "N" + s[m + 1:], s[:-1] + "N", s[:m] + "n" + s[m + 1:], s[:m] + "-" + s[m + 1:],
                    s.lower(), fx.revcomp(s).lower(), "".join(c.lower() if i % 3 else c for i, c in enumerate(s))]
    ids = check(ctx, queries, k)
    per = ids.reshape(-1, 14)
    assert np.all(per[:, 0] > 0) and np.all(per[:, 1] == -per[:, 0])
    assert np.all(per[:, 2:11] == 0)
    assert np.all(per[:, 11] == per[:, 0]) and np.all(per[:, 12] == per[:, 1]) and np.all(per[:, 13] == per[:, 0])      # lower and mixed case: found like upper case
    st = ctx.reads_find_stats()
    assert st.not_good == 40 * 9 and st.found == 40 * 5
    ctx.close()


def case_self_reverse_complement(device):
    L, k = 100, 21
    bases, off = fx.make_reads(dict(recipe="low_complexity", seed=3000 + L, read_len=L, block=2 * L, flank=400, step=2))
    ctx = organised(k, (bases, off), device)
    queries = input_reads(bases, off) + ["AT" * (L // 2), "TA" * (L // 2), "A" * L, "T" * L]
    ids = check(ctx, queries, k)
    at, ta, pa, pt = (int(x) for x in ids[-4:])
    assert at < 0 and ta <= 0 and at != ta                               # (AT)n (in the store) and (TA)n (the block is tiled at even offsets: not in it) are each their own reverse complement: -id, 0
    assert pa > 0 and pt == -pa                                          # poly-A and poly-T: one id, opposite signs
    selfrc = [i for i, q in enumerate(queries) if q == fx.revcomp(q)]
    assert len(selfrc) > 10 and np.all(ids[selfrc] <= 0) and (ids[selfrc] < 0).sum() > 10
    assert np.all(ids[:-4] != 0)
    ctx.close()
    # a genome that is its own reverse complement around a centre: the reads across the centre equal their own reverse complement
    bases, off = fx.make_reads(dict(recipe="palindrome_tandem", seed=4400, half=600, flank=1500, tandem_units=60, read_len=L, step=2))
    ctx = organised(k, (bases, off), device)
    queries = input_reads(bases, off)
    ids = check(ctx, queries, k)
    selfrc = [i for i, q in enumerate(queries) if q == fx.revcomp(q)]
    assert len(selfrc) >= 1 and np.all(ids[selfrc] < 0) and np.all(ids != 0)
    ctx.close()


def case_layout(device, top, words, k):
    bases, off = fx.make_reads(dict(recipe="short_reads", seed=4500 + k + top, k=k, top=top, step=5, n_reads=600))
    ctx = organised(k, (bases, off), device)
    st = ctx.reads_stats()
    assert st.words_per_read == words and st.max_read_length == top
    reads = input_reads(bases, off); rng = np.random.default_rng(top + k)
    queries = reads + [fx.revcomp(r) for r in reads[::3]] + [change_last(r) for r in reads[::5]] + [r[:-1] for r in reads[1::5]] + [rnd(rng, top) for _ in range(20)]
    ids = check(ctx, queries, k)
    assert np.all(ids[:len(reads)] != 0) and len({len(r) for r in reads}) > 50
    ctx.close()


def case_heavy_bucket(device):
    L, k = 100, 21; rng = np.random.default_rng(4600)
    prefix = "A" * 8 + rnd(rng, 32)                                      # (a read that starts with AAAAAAAA is its own canonical form)
    heavy = [prefix + rnd(rng, L - 40) for _ in range(600)]
    ordinary = fx.recipe_reads(dict(recipe="tiling", seed=4601, n_unique=2000, read_len=L, step=7))
    ctx = organised(k, ordinary + heavy, device)
    assert ctx.reads_stats().unique_reads == 2600
    store = stored_reads(ctx)
    run = [i for i in range(1, 2601) if store[i].startswith(prefix)]
    assert len(run) == 600 and run == list(range(run[0], run[0] + 600))  # one run of ids: 600 reads inside one value of word 0
    near = []
    for h in heavy:                                                      # near misses: the tail differs in one base
        p = int(rng.integers(40, L)); near.append(h[:p] + ("C" if h[p] != "C" else "G") + h[p + 1:])
    queries = heavy + near + [fx.revcomp(h) for h in heavy[:100]] + ordinary[::4]
    ids = check(ctx, queries, k)
    assert np.all(ids[:600] > 0) and set(ids[:600]) == set(run) and np.all(ids[600:1200] == 0) and np.all(ids[1200:1300] < 0)
    ctx.close()


def directory_bits(n):
    return min(FIND_B_MAX, max(FIND_B_MIN, max(n - 1, 0).bit_length() - 1))                       # ceil(log2 n) - 1, clamped


def search_edge_counts():
    """N = 1, 2, 3 and both sides of every unique-read count in 2 .. 5000 at which the directory's bit count changes"""
    steps = [n for n in range(3, 5001) if directory_bits(n) != directory_bits(n - 1)]
    assert steps == [33, 65, 129, 257, 513, 1025, 2049, 4097]
    return [1, 2, 3] + [m for n in steps for m in (n - 1, n)]


def case_search_edges(device, n):
    L, k = 50, 21; rng = np.random.default_rng(4700 + n)
    reads = fx.recipe_reads(dict(recipe="tiling", seed=4700 + n, n_unique=n, read_len=L, step=7))
    ctx = organised(k, reads, device)
    assert ctx.reads_stats().unique_reads == n
    store = stored_reads(ctx)
    below, above = "A" * L, "T" * (L // 2) + "A" * (L // 2)             # smaller than read 1 (poly-A is its own canonical form); larger than read N (its own reverse complement)
    assert below < store[1] and above > store[n] and above == fx.revcomp(above)
    strangers = [rnd(rng, L) for _ in range(64)]                         # (N <= 3: nearly every one of the >= 16 buckets is empty)
    queries = reads + [fx.revcomp(r) for r in reads] + [below, above, "A" * (k + 1)] + strangers + [change_last(store[1]), change_last(store[n]), store[1][:-1], store[n] + "T"]
    ids = check(ctx, queries, k)
    assert np.all(ids[:2 * n] != 0) and np.all(ids[2 * n:2 * n + 3] == 0)
    bits = directory_bits(n); used = {top_bits(s, bits) for s in store[1:]}
    assert any(top_bits(min(q, fx.revcomp(q)), bits) not in used for q in strangers), "a query whose bucket is empty"
    if device != HOST:
        assert ctx.reads_find_stats().directory_bits == bits
    ctx.close()


def top_bits(s, b):
    """the top b bits of word 0 of a packed read"""
    v = 0
    for c in s[:32]:
        v = (v << 2) | "ACGT".index(c)
    v <<= 2 * (32 - min(len(s), 32))
    return v >> (64 - b)


def case_store_states(device, tmp_path):
    """after reads_organize, after reads_load of a P.reads we wrote, after reads_import_words: the same ids"""
    L, k = 100, 21
    bases, off = fx.make_reads(dict(recipe="tiling", seed=4800, n_unique=1500, read_len=L, step=7, dup_every=5, dup_copies=1))
    reads = input_reads(bases, off); rng = np.random.default_rng(4801)
    queries = reads + [rnd(rng, L) for _ in range(50)] + [r[:-1] for r in reads[:50]]
    a = organised(k, (bases, off), device)
    first = check(a, queries, k)
    p = str(tmp_path / "t.reads"); a.reads_save(p)
    b = s2.Context(k, device=device); b.reads_load(p)
    assert np.array_equal(check(b, queries, k), first)
    words, freq = a.reads_export_words(); st = a.reads_stats()
    c = s2.Context(k, device=device)
    c.reads_import_words(words, st.unique_reads, st.words_per_read, st.max_read_length, freq, st.good_reads, st.total_bp)
    assert np.array_equal(check(c, queries, k), first)
    for x in (a, b, c):
        x.close()
    return queries, first


MIRROR_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>
#include "sage2ov.hpp"
int main(int argc, char** argv) {      // <k> <device> <reads.fa> <queries.txt>: one id per line, single calls first, then the batch overload
    try {
        sage2ov::Context ctx((uint16_t)atoi(argv[1]), atoi(argv[2]));
        sage2ov::ReadLoader loader(ctx);
        loader.readDatasetInBytes(argv[3]);
        loader.organizeReads();
        std::vector<std::string> q; std::ifstream in(argv[4]); std::string line;
        while (std::getline(in, line)) q.push_back(line);
        for (const auto& s : q) printf("%lld\n", (long long)loader.getIdOfRead(s));
        for (int64_t id : loader.getIdOfRead(q)) printf("%lld\n", (long long)id);
    } catch (const sage2ov::Error& e) { fprintf(stderr, "error %d: %s\n", e.code, e.what()); return 1; }
    return 0;
}
"""


def case_cpp_mirror(device, tmp_path):
    """sage2ov.hpp compiles, and ReadLoader::getIdOfRead (one read, and the batch overload) returns what the C call returns"""
    L, k = 100, 21
    pd = dict(recipe="tiling", seed=4900, n_unique=300, read_len=L, step=7, dup_every=5, dup_copies=1)
    fa = str(tmp_path / "r.fa"); fx.write_recipe_fasta(pd, fa)
    reads = fx.recipe_reads(pd); rng = np.random.default_rng(4901)
    queries = reads[:60] + [fx.revcomp(r) for r in reads[60:90]] + [rnd(rng, L) for _ in range(5)] + [reads[0][:k], reads[1][:-1] + "N", reads[2].lower()]
    qf = str(tmp_path / "q.txt"); open(qf, "w").write("".join(q + "\n" for q in queries))
    src, exe = str(tmp_path / "mirror.cpp"), str(tmp_path / "mirror")
    open(src, "w").write(MIRROR_CPP)
    libdir = os.path.join(fx.ROOT, "sage2_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(fx.ROOT, "include"), "-I", os.path.join(libdir, "csrc"), src, "-o", exe,
                    "-L", libdir, "-lsage2ov", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe, str(k), str(device), fa, qf], check=True, stdout=subprocess.PIPE, text=True, timeout=120).stdout.split()
    got = np.array([int(x) for x in out], dtype=np.int64)
    ctx = s2.Context(k, device=device); ctx.reads_add_file(fa); ctx.reads_organize()
    want = check(ctx, queries, k)
    assert np.array_equal(got[:len(queries)], want) and np.array_equal(got[len(queries):], want)
    assert (want > 0).sum() >= 30 and (want < 0).sum() >= 30 and (want == 0).sum() >= 7
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- the host route
@pytest.mark.parametrize("L,k", [(100, 21), (150, 40)], ids=["L100k21", "L150k40"])
def test_every_input_read_finds_itself(L, k):
    case_every_input_read_finds_itself(HOST, L, k)


def test_compare_is_bytes_then_length():
    case_compare_is_bytes_then_length(HOST)


def test_bad_and_odd_queries():
    case_bad_and_odd_queries(HOST)


def test_self_reverse_complement_reads():
    case_self_reverse_complement(HOST)


@pytest.mark.parametrize("top,words", LAYOUT_TOPS, ids=[f"top{t}" for t, _ in LAYOUT_TOPS])
@pytest.mark.parametrize("k", [21, 64])
def test_every_layout(k, top, words):
    case_layout(HOST, top, words, k)


def test_heavy_bucket():
    case_heavy_bucket(HOST)


def test_edges_of_the_search():
    for n in search_edge_counts():
        case_search_edges(HOST, n)


def test_store_states(tmp_path):
    case_store_states(HOST, tmp_path)
    ctx = organised(21, ["ACGT" * 10], HOST)
    find(ctx, ["ACGT" * 10])
    st = ctx.reads_find_stats()
    assert (st.route, st.launches, st.directory_bits, st.device_ms) == (s2.FIND_ROUTE_HOST, 0, 0, 0.0)
    ctx.close()


def test_errors():
    L = s2.lib()
    ctx = s2.Context(21, device=HOST)
    bases, off = to_arrays(["ACGTACGTACGTACGTACGTACGTACGTAC"])
    ctx.reads_add_ascii(bases, off)
    with pytest.raises(s2.Sage2ovError) as e:                            # before the reads are organised
        ctx.reads_find_ids(bases, off)
    assert e.value.code == -1 and "organise" in str(e.value)
    ctx.reads_organize()
    assert ctx.reads_find_ids(np.zeros(0, np.uint8), np.zeros(1, np.uint64)).shape == (0,)       # n = 0
    assert L.sage2ov_reads_find_ids(ctx._h, None, None, C.c_uint64(0), None) == 0
    st = ctx.reads_find_stats()
    assert (st.queries, st.found, st.not_good, st.not_found) == (0, 0, 0, 0)
    ids = np.zeros(1, np.int64)
    for args in ((None, C.c_void_p(off.ctypes.data), C.c_void_p(ids.ctypes.data)), (C.c_void_p(bases.ctypes.data), None, C.c_void_p(ids.ctypes.data)),
                 (C.c_void_p(bases.ctypes.data), C.c_void_p(off.ctypes.data), None)):
        assert L.sage2ov_reads_find_ids(ctx._h, args[0], args[1], C.c_uint64(1), args[2]) == -1
        assert b"null" in L.sage2ov_last_error(ctx._h)
    assert L.sage2ov_reads_find_ids(None, C.c_void_p(bases.ctypes.data), C.c_void_p(off.ctypes.data), C.c_uint64(1), C.c_void_p(ids.ctypes.data)) == -1
    assert L.sage2ov_reads_find_stats_get(ctx._h, None) == -1
    backwards = np.array([5, 0], dtype=np.uint64)
    with pytest.raises(s2.Sage2ovError) as e:
        ctx.reads_find_ids(bases, backwards)
    assert e.value.code == -1
    assert check(ctx, ["ACGTACGTACGTACGTACGTACGTACGTAC", "GTACGTACGTACGTACGTACGTACGTACGT"], 21).tolist() == [1, -1]
    ctx.close()
    empty = s2.Context(21, device=HOST); empty.reads_organize()          # an empty store: nothing is found, nothing fails
    assert find(empty, ["ACGTACGTACGTACGTACGTACGTACGTAC", "ACGT"]).tolist() == [0, 0]
    empty.close()


def test_cpp_mirror(tmp_path):
    case_cpp_mirror(HOST, tmp_path)
