"""CPU: the mate table from step 1's own pass (sage2ov_reads_pair_library + sage2ov_mates_from_reads) on a device-less context, which builds it
from the host organiser's permutation.  The expected value is the route that exists: context B is organised from the same input with pairing off and given the
matching sequence of mates_add_* calls; context A stages with pairing on and calls mates_from_reads() once.  Compared are every library's export as a whole
(entries byte for byte, offsets) and the counters of mates_stats().  The cases are functions of the device ordinal: tests/test_gpu_pairing.py runs the same
ones against the HIP path."""
import gzip
import os

import numpy as np
import pytest

import fixtures as fx
import sage2_amd as s2
from test_find_ids_host import HOST, rnd, to_arrays

K = 21
COUNTERS = ("pairs_seen", "pairs_added", "pairs_not_good", "pairs_not_found", "records", "entries_before", "entries_after", "library", "libraries")


# ---------------------------------------------------------------------------------------------------------------- both routes
def stage(ctx, call, pairing):
    """one reads_add_* call; call = ("ascii", reads, library) | ("file", path1, path2 or None, library) | ("list", path)"""
    kind = call[0]
    if pairing:
        ctx.reads_pair_library(1 if kind == "list" else call[-1])
    if kind == "ascii":
        ctx.reads_add_ascii(*to_arrays(call[1]))
    elif kind == "file":
        ctx.reads_add_file(call[1], call[2])
    else:
        ctx.reads_add_list(call[1])


def mate(ctx, call):
    """the same call on the mates_add_* route"""
    kind = call[0]
    if kind == "ascii":
        ctx.mates_add_ascii(*to_arrays(call[1]), call[2])
    elif kind == "file":
        ctx.mates_add_file(call[1], call[2], call[3])
    else:
        ctx.mates_add_list(call[1])


def tables(ctx, libraries=(1, 2, 3)):
    return [ctx.mates(lib) for lib in libraries]


def same_tables(a, b):
    return all(ea.tobytes() == eb.tobytes() and np.array_equal(oa, ob) for (ea, oa), (eb, ob) in zip(a, b))


def counters(ctx):
    st = ctx.mates_stats()
    return tuple(int(getattr(st, f)) for f in COUNTERS)


def both_routes(device, calls, k=K, pre=None, between=None, libraries=(1, 2, 3)):
    """A: pairing on, mates_from_reads; B: pairing off, the matching mates_add_* calls.  pre: reads given to mates_add_ascii(library 1) on both before that
    (`first` has to continue from them); between(ctx): run on both after reads_organize.  Returns A's tables (B's are equal) and A's stats."""
    A, B = s2.Context(k, device=device), s2.Context(k, device=device)
    for c in calls:
        stage(A, c, True); stage(B, c, False)
    A.reads_organize(); B.reads_organize()
    pa, la, fa = A.reads_export(); pb, lb, fb = B.reads_export()
    assert np.array_equal(pa, pb) and np.array_equal(la, lb) and np.array_equal(fa, fb), "pairing must not change what step 1 makes"
    if between:
        between(A); between(B)
    if pre:
        A.mates_add_ascii(*to_arrays(pre), 1); B.mates_add_ascii(*to_arrays(pre), 1)
    A.mates_from_reads()
    for c in calls:
        mate(B, c)
    ta, tb = tables(A, libraries), tables(B, libraries)
    ca, cb = counters(A), counters(B)
    print(f"{len(calls)} calls: entries {[len(e) for e, _ in ta]} (expected {[len(e) for e, _ in tb]}); last call's counters {ca} (expected {cb})")
    assert same_tables(ta, tb), "a library's table differs from the mates_add_* route"
    assert ca == cb and ca[3] == 0, "the skip counters of the last call"
    st = A.mates_stats()
    B.close()
    return A, ta, st


# ---------------------------------------------------------------------------------------------------------------- the inputs
def random_reads(rng, n, lo=40, hi=150):
    return [rnd(rng, int(rng.integers(lo, hi + 1))) for _ in range(n)]


def palindrome(rng, half):
    s = rnd(rng, half)
    return s + fx.revcomp(s)                                               # equal to its own reverse complement


def with_n(s):
    return s[:7] + "N" + s[8:]


def ascii_calls(seed=8100):
    """three batches of odd size for library 1 that hold every kind of pair the rules name, and one batch for library 2 with the 255 / 256 / 257-fold pairs"""
    rng = np.random.default_rng(seed)
    r = random_reads(rng, 80)
    pal = palindrome(rng, 30)
    assert pal == fx.revcomp(pal)
    b1 = [r[0], r[1],
          with_n(r[2]), r[3],                                              # the first mate is not a good read
          r[4], with_n(r[5]),                                              # the second
          with_n(r[6]), with_n(r[7]),                                      # both
          r[8][:K], r[9],                                                  # a read of length k
          r[10], r[11][:K - 3],                                            # and shorter
          r[12], r[12],                                                    # both mates the same read
          pal, r[13], r[14], pal, pal, pal,                                # a read equal to its reverse complement
          r[15], r[16], fx.revcomp(r[16]), fx.revcomp(r[15]),              # (a, b) and (rc b, rc a): the same two entries
          r[17], fx.revcomp(r[17]),
          r[18]]                                                           # a trailing odd read
    b2 = [x for i in range(20, 40, 2) for x in (r[i], fx.revcomp(r[i + 1]) if i % 4 == 0 else r[i + 1])] + [r[0], r[1], r[1], r[0]] + [with_n(r[41])]
    b3 = [x for i in range(42, 60, 2) for x in (fx.revcomp(r[i]), r[i + 1])] + [r[15], r[16]] + [r[61]]
    assert len(b1) % 2 == len(b2) % 2 == len(b3) % 2 == 1
    dup = [r[62], r[63]] * 255 + [r[64], fx.revcomp(r[65])] * 256 + [fx.revcomp(r[66]), r[67]] * 257
    return [("ascii", b1, 1), ("ascii", b2, 1), ("ascii", b3, 1), ("ascii", dup, 2)], r


def file_reads(seed, n=8200, L=150):
    """n reads of L bases with bad ones (an N, or too short) spread out and in clusters around every sixteenth of the file, where the parallel reader cuts"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4, size=(n, L), dtype=np.uint8)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    reads = [bytes(row).decode() for row in text]
    for i in range(0, n, 400):                                             # duplicates and reverse complements of earlier reads: ids shared between records
        reads[i + 3] = reads[i]; reads[i + 5] = fx.revcomp(reads[i + 1])
    bad = set(range(0, n, 61))
    for x in range(1, 16):
        c = n * x // 16
        bad.update(range(c - 2, c + 3, 2)); bad.add(c + 1)
    for j, i in enumerate(sorted(bad)):
        reads[i] = with_n(reads[i]) if j % 3 else reads[i][:K - (j % 2)]
    return reads


def write_fasta(path, reads, opener=open):
    with opener(path, "wt") as f:
        f.write("".join(f">r{i}\n{s}\n" for i, s in enumerate(reads)))
    return path


def write_fastq(path, reads):
    with open(path, "w") as f:
        f.write("".join(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate(reads)))
    return path


# ---------------------------------------------------------------------------------------------------------------- the cases (device: a HIP ordinal, or HOST)
def case_ascii(device):
    calls, r = ascii_calls()
    A, t, st = both_routes(device, calls)
    e1, e2 = t[0][0], t[1][0]
    assert st.library == 2 and st.libraries == 2 and st.pairs_seen == 255 + 256 + 257 == st.pairs_added
    assert sorted(int(c) for c in e2["count"]) == [255, 255, 256, 256, 257, 257] and sorted(int(f) for f in e2["freq"]) == [0, 0, 1, 1, 255, 255]      # freq wraps to 0 at 256
    assert (e1["from"] == e1["to"]).sum() >= 2 and len(e1) > 40 and len(t[2][0]) == 0
    assert int(e1["count"].max()) >= 2                                     # (a, b) and (rc b, rc a), and the pairs given again in a later batch
    A.close()


def case_first_continues(device):
    """mates_add_ascii on library 1 before mates_from_reads: `first` of the new entries goes on from the pairs that call was given, skipped ones included"""
    calls, r = ascii_calls(8200)
    pre = [r[0], r[1], with_n(r[2]), r[3], r[20], r[21], r[15], r[16], r[70], r[71]]      # (r[70], r[71]: good reads that are not in the store)
    A, t, st = both_routes(device, calls[:3], pre=pre)
    e1 = t[0][0]
    assert int(e1["first"].min()) == 0 and int(e1["first"].max()) >= 2 * 5 + 2 * (len(calls[0][1]) // 2 + len(calls[1][1]) // 2)
    A.close()


def case_fasta(device, tmp_path, monkeypatch, sequential):
    monkeypatch.delenv("SAGE2OV_SEQUENTIAL_READER", raising=False)
    if sequential:
        monkeypatch.setenv("SAGE2OV_SEQUENTIAL_READER", "1")
    reads = file_reads(8300)
    p = write_fasta(str(tmp_path / "inter.fa"), reads)
    assert os.path.getsize(p) > (1 << 20)                                  # below that the parallel reader declines
    A, t, st = both_routes(device, [("file", p, None, 1)])
    assert st.pairs_seen == len(reads) // 2 and st.pairs_not_good > 100 and st.pairs_added > 3500
    A.close()


def case_fastq(device, tmp_path, monkeypatch):
    monkeypatch.delenv("SAGE2OV_SEQUENTIAL_READER", raising=False)
    reads = file_reads(8400, n=4301)                                       # (odd: the last record has no mate)
    p = write_fastq(str(tmp_path / "inter.fq"), reads)
    assert os.path.getsize(p) > (1 << 20)
    A, t, st = both_routes(device, [("file", p, None, 3)], libraries=(1, 2, 3))
    assert st.pairs_seen == 2150 and st.library == 3 and len(t[2][0]) > 3000
    A.close()


def case_gz(device, tmp_path, monkeypatch):
    monkeypatch.delenv("SAGE2OV_SEQUENTIAL_READER", raising=False)
    reads = file_reads(8500, n=1600)
    p = write_fasta(str(tmp_path / "inter.fa.gz"), reads, gzip.open)
    A, t, st = both_routes(device, [("file", p, None, 1)])
    assert st.pairs_seen == 800 and st.pairs_not_good > 20
    A.close()


def case_two_files(device, tmp_path, monkeypatch, extra):
    """f1 / f2 read in turn: record j of file 1 is record 2 j, record j of file 2 is 2 j + 1; extra = 1: file 1 has one record more"""
    monkeypatch.delenv("SAGE2OV_SEQUENTIAL_READER", raising=False)
    n = 7400
    a, b = file_reads(8600, n=n + 16), file_reads(8601, n=n)
    a = a[:n + extra]
    p1, p2 = write_fasta(str(tmp_path / "m1.fa"), a), write_fasta(str(tmp_path / "m2.fa"), b)
    assert os.path.getsize(p1) > (1 << 20) and os.path.getsize(p2) > (1 << 20)
    A, t, st = both_routes(device, [("file", p1, p2, 2)])
    assert st.pairs_seen == n and st.library == 2 and st.pairs_added > 6000
    A.close()


def case_list(device, tmp_path, monkeypatch):
    monkeypatch.delenv("SAGE2OV_SEQUENTIAL_READER", raising=False)
    r1, r2a, r2b = file_reads(8700, n=900), file_reads(8701, n=700), file_reads(8702, n=700)
    p1 = write_fasta(str(tmp_path / "d1.fa"), r1); pa = write_fasta(str(tmp_path / "d2_1.fa"), r2a); pb = write_fastq(str(tmp_path / "d2_2.fq"), r2b)
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        f.write(f"# two datasets\nf = {p1}\nf1 = {pa}\nf2 = {pb}\n")
    A, t, st = both_routes(device, [("list", lst)])
    assert st.library == 2 and st.libraries == 2 and st.pairs_seen == 700 and len(t[0][0]) > 700 and len(t[1][0]) > 1000
    A.close()


def case_errors(device):
    calls, r = ascii_calls(8800)
    ctx = s2.Context(K, device=device)
    ctx.reads_add_ascii(*to_arrays(calls[0][1])); ctx.reads_organize()     # no pairing
    ctx.mates_add_ascii(*to_arrays(calls[0][1]), 1)
    before = tables(ctx)

    def refused(f, *a):
        with pytest.raises(s2.Sage2ovError) as e:
            f(*a)
        assert e.value.code == -1
        assert same_tables(tables(ctx), before), "an error changed the mate tables"

    refused(ctx.mates_from_reads)                                          # staged without pairing
    refused(ctx.reads_pair_library, 1)                                     # after reads_organize
    ctx.close()
    ctx = s2.Context(K, device=device)
    with pytest.raises(s2.Sage2ovError) as e:
        ctx.reads_pair_library(128)
    assert e.value.code == -1
    ctx.reads_pair_library(1); ctx.reads_add_ascii(*to_arrays(calls[0][1]))
    ctx.reads_pair_library(0); ctx.reads_add_ascii(*to_arrays(calls[1][1]))      # (off again: this call is no mates call)
    with pytest.raises(s2.Sage2ovError) as e:
        ctx.mates_from_reads()                                             # before reads_organize
    assert e.value.code == -1
    ctx.reads_organize(); ctx.mates_from_reads()
    before = tables(ctx)
    assert len(before[0][0]) > 0
    B = s2.Context(K, device=device)
    B.reads_add_ascii(*to_arrays(calls[0][1] + calls[1][1])); B.reads_organize(); B.mates_add_ascii(*to_arrays(calls[0][1]), 1)
    assert same_tables(before, tables(B))
    B.close()
    refused(ctx.mates_from_reads)                                          # a second call
    ctx.mates_clear()
    before = tables(ctx)
    assert len(before[0][0]) == 0
    refused(ctx.mates_from_reads)
    ctx.close()
    ctx = s2.Context(K, device=device)                                     # mates_clear releases the remembered pairing
    ctx.reads_pair_library(1); ctx.reads_add_ascii(*to_arrays(calls[0][1])); ctx.reads_organize(); ctx.mates_clear()
    before = tables(ctx)
    refused(ctx.mates_from_reads)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- the tests
def test_ascii_rules():
    case_ascii(HOST)


def test_first_continues_from_earlier_calls():
    case_first_continues(HOST)


@pytest.mark.parametrize("sequential", [False, True], ids=["parallel_reader", "sequential_reader"])
def test_interleaved_fasta(tmp_path, monkeypatch, sequential):
    case_fasta(HOST, tmp_path, monkeypatch, sequential)


def test_four_line_fastq(tmp_path, monkeypatch):
    case_fastq(HOST, tmp_path, monkeypatch)


def test_gzip(tmp_path, monkeypatch):
    case_gz(HOST, tmp_path, monkeypatch)


@pytest.mark.parametrize("extra", [0, 1], ids=["n1_eq_n2", "n1_eq_n2_plus_1"])
def test_two_mate_files(tmp_path, monkeypatch, extra):
    case_two_files(HOST, tmp_path, monkeypatch, extra)


def test_list_of_two_datasets(tmp_path, monkeypatch):
    case_list(HOST, tmp_path, monkeypatch)


def test_errors():
    case_errors(HOST)
