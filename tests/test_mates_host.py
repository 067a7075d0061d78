"""CPU: the mate-pair table (sage2ov_mates_*: MatePair::mapMatePairs / processMatePairs, matePair.cpp:125-239) on a device-less context, which builds it with
find_ids_host, a sort of the records and a reduce.  The expected value is a restatement of matePair.cpp:161-239 as run with one thread, written here
(`Restated`): a serial loop over the pairs with per-read Python lists, head insertion, a search for an equal entry and `freq` as a uint8, over the ids of
`expected_ids` of tests/test_find_ids_host.py (not over the library's ids).  One rule differs from the reference, on purpose: a pair with a mate of id 0 (a good
read that is not in the store) is skipped instead of being filed under read 0.  From the restatement come, per read, the list in list order; compared with the
export are the set of entries, `count`, `freq`, the order that `first` implies, and `offsets`.  The cases are functions of the device ordinal:
tests/test_gpu_mates.py runs the same ones against the HIP path."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import fixtures as fx
import sage2_amd as s2
import test_find_ids_host as H
from test_find_ids_host import HOST, organised, rnd, stored_reads, to_arrays


# ---------------------------------------------------------------------------------------------------------------- the expected value
def good(q, k):
    return len(q) > k and not (set(q.upper()) - set("ACGT"))             # utils.cpp:144-166


class Restated:
    """matePair.cpp:161-239, one thread.  lists[a] = matePairList[a], head first; an entry is [ID, type1, type2, library, freq] as in MatePairInfo, plus the
    exact count and the ordinal of the record that inserted it (what the export calls `count` and `first`)."""

    def __init__(self):
        self.lists, self.pairs = {}, {}
        self.seen = self.added = self.not_good = self.not_found = 0      # of the last call

    def add(self, ctx, reads, k, library):
        ids = H.expected_ids(ctx, reads, k)
        self.seen = self.added = self.not_good = self.not_found = 0
        for i in range(0, len(reads) - 1, 2):                            # :172
            p = self.pairs.get(library, 0); self.pairs[library] = p + 1; self.seen += 1
            if not (good(reads[i], k) and good(reads[i + 1], k)):        # :176
                self.not_good += 1; continue
            id1, id2 = int(ids[i]), int(ids[i + 1])
            if id1 == 0 or id2 == 0:                                     # the deliberate difference: the reference goes on with id 0, type 0
                self.not_found += 1; continue
            type1, type2 = int(id1 > 0), int(id2 > 0)                    # :180-187
            id1, id2 = abs(id1), abs(id2)                                # :188-189
            self._insert(id1, id2, type1, type2, library, 2 * p)         # :190-212
            self._insert(id2, id1, type2, type1, library, 2 * p + 1)     # :213-235
            self.added += 1

    def _insert(self, a, b, t1, t2, library, ordinal):
        lst = self.lists.setdefault(a, [])
        for w in lst:
            if w[0] == b and w[1] == t1 and w[2] == t2 and w[3] == library:
                w[4] = (w[4] + 1) & 255; w[5] += 1                       # uint8_t freq
                return
        lst.insert(0, [b, t1, t2, library, 1, 1, ordinal])               # head insertion

    def list(self, a, library):
        return [tuple(w) for w in self.lists.get(a, []) if w[3] == library]

    def entries(self, library):
        return sum(len(self.list(a, library)) for a in self.lists)


def add(ctx, R, reads, k, library=1):
    """one call on both sides; the stats of the call are the restatement's"""
    before = ctx.mates_count(library)
    ctx.mates_add_ascii(*to_arrays(reads), library)
    R.add(ctx, reads, k, library)
    st = ctx.mates_stats()
    print(f"library {library}: {len(reads)} reads -> seen {st.pairs_seen} added {st.pairs_added} not good {st.pairs_not_good} not found {st.pairs_not_found}; "
          f"entries {st.entries_before} -> {st.entries_after}; route {st.route}, chunks {st.chunks}, passes {st.sort_passes}, flushes {st.flushes}")
    assert (st.pairs_seen, st.pairs_added, st.pairs_not_good, st.pairs_not_found) == (R.seen, R.added, R.not_good, R.not_found)
    assert st.pairs_seen == len(reads) // 2 == st.pairs_added + st.pairs_not_good + st.pairs_not_found and st.records == 2 * st.pairs_added
    assert (st.library, st.entries_before, st.entries_after) == (library, before, ctx.mates_count(library)) and st.entries_after == R.entries(library)
    return st


def compare(ctx, R, library=1):
    """the export of one library against the restatement: set, count, freq, the order `first` implies, offsets; returns the entries"""
    N = ctx.reads_stats().unique_reads
    ent, offs = ctx.mates(library)
    assert len(ent) == ctx.mates_count(library) == R.entries(library)
    key = (ent["from"].astype(np.uint64) << np.uint64(32)) | (ent["to"].astype(np.uint64) << np.uint64(2)) | (ent["type1"].astype(np.uint64) << np.uint64(1)) | ent["type2"].astype(np.uint64)
    assert np.all(key[1:] > key[:-1]), "ascending (from, to, type1, type2), every key once"
    assert np.all(ent["library"] == library) and np.all(ent["freq"] == (ent["count"] & np.uint64(255))) and np.all(ent["pad"] == 0)
    assert len(ent) == 0 or (ent["from"].min() >= 1 and ent["from"].max() <= N and ent["to"].min() >= 1 and ent["to"].max() <= N)
    assert offs.shape == (N + 2,) and np.array_equal(offs, np.searchsorted(ent["from"], np.arange(N + 2), side="left").astype(np.uint64))
    assert int(offs[N + 1]) == len(ent)
    assert len(np.unique(ent["first"])) == len(ent)                      # a record ordinal belongs to one key
    for a in sorted(set(R.lists) | set(int(x) for x in np.unique(ent["from"]))):
        seg = ent[int(offs[a]):int(offs[a + 1])]
        seg = seg[np.argsort(seg["first"])[::-1]]                        # the reference's list order: head insertion = descending first
        got = [(int(e["to"]), int(e["type1"]), int(e["type2"]), int(e["library"]), int(e["freq"]), int(e["count"]), int(e["first"])) for e in seg]
        assert got == R.list(a, library), f"list of read {a}"
    return ent


def tiling_store(device, n_unique, L, k, seed, **dup):
    bases, off = fx.make_reads(dict(recipe="tiling", seed=seed, n_unique=n_unique, read_len=L, step=7, **dup))
    ctx = organised(k, (bases, off), device)
    assert ctx.reads_stats().unique_reads == n_unique
    return ctx, H.input_reads(bases, off)


def ordinary_pairs(reads):
    """pairs of input reads (i, i + 37), mates flipped so that every type combination occurs, some pairs repeated 2-5 times"""
    out = []
    for i in range(len(reads) - 37):
        a, b = reads[i], reads[i + 37]
        if i % 3 == 0:
            a = fx.revcomp(a)
        if i % 4 == 1:
            b = fx.revcomp(b)
        out += [a, b] * (2 + (i // 11) % 4 if i % 11 == 0 else 1)
    return out


# ---------------------------------------------------------------------------------------------------------------- the cases (device: a HIP ordinal, or HOST)
def case_ordinary(device):
    k = 21
    ctx, reads = tiling_store(device, 3000, 100, k, 6100, dup_every=7, dup_copies=2)
    mates = ordinary_pairs(reads)
    assert 3800 <= len(mates) // 2 <= 4800
    R = Restated(); st = add(ctx, R, mates, k)
    assert st.pairs_added == len(mates) // 2
    ent = compare(ctx, R)
    for t1 in (0, 1):
        for t2 in (0, 1):
            assert ((ent["type1"] == t1) & (ent["type2"] == t2)).sum() > 100
    assert (ent["count"] > 1).sum() > 100 and ent["count"].sum() == 2 * st.pairs_added
    ctx.close()
    return mates


def case_freq_wrap(device):
    k = 21
    ctx, reads = tiling_store(device, 40, 100, k, 6200)
    mates = []
    for j, times in enumerate((255, 256, 257, 600)):
        mates += [reads[2 * j], fx.revcomp(reads[2 * j + 1])] * times
    R = Restated(); add(ctx, R, mates, k)
    ent = compare(ctx, R)
    assert len(ent) == 8 and sorted(ent["count"].tolist()) == [255, 255, 256, 256, 257, 257, 600, 600]
    by_count = {int(e["count"]): int(e["freq"]) for e in ent}
    assert by_count == {255: 255, 256: 0, 257: 1, 600: 88}
    pair = [reads[20], reads[21]]
    for _ in range(3):                                                   # the same pair 600 times over three calls, in a library of its own
        add(ctx, R, pair * 200, k, library=2)
    ent = compare(ctx, R, library=2)
    assert len(ent) == 2 and ent["count"].tolist() == [600, 600] and ent["freq"].tolist() == [88, 88] and sorted(ent["first"].tolist()) == [0, 1]
    compare(ctx, R)                                                      # library 1 is as it was
    ctx.close()


def case_self_pairs(device):
    k = 21
    ctx, reads = tiling_store(device, 60, 100, k, 6300)
    mates = []
    for r in reads[:20]:
        mates += [r, r]                                                  # one key: one entry of count 2 per pair
    for r in reads[20:40]:
        mates += [r, fx.revcomp(r)]                                      # two keys: two entries of count 1
    R = Restated(); add(ctx, R, mates, k)
    ent = compare(ctx, R)
    same = ent[ent["type1"] == ent["type2"]]; cross = ent[ent["type1"] != ent["type2"]]
    assert np.all(ent["from"] == ent["to"]) and len(same) == 20 and np.all(same["count"] == 2) and len(cross) == 40 and np.all(cross["count"] == 1)
    ctx.close()
    L = 100                                                              # a read equal to its own reverse complement: (AT)n, both types 0
    bases, off = fx.make_reads(dict(recipe="low_complexity", seed=3000 + L, read_len=L, block=2 * L, flank=400, step=2))
    ctx = organised(k, (bases, off), device)
    at = "AT" * (L // 2)
    assert at == fx.revcomp(at) and int(H.expected_ids(ctx, [at], k)[0]) < 0
    other = H.input_reads(bases, off)[3]
    R = Restated(); add(ctx, R, [at, at, at, other, other, at, at, at], k)
    ent = compare(ctx, R)
    me = ent[(ent["from"] == ent["to"])]
    assert len(me) == 1 and (int(me[0]["type1"]), int(me[0]["type2"]), int(me[0]["count"]), int(me[0]["first"])) == (0, 0, 4, 0)
    ctx.close()


def case_skipped_pairs(device):
    k, top = 21, 123
    ctx = organised(k, fx.make_reads(dict(recipe="short_reads", seed=6400, k=k, top=top, step=5, n_reads=600)), device)
    store = stored_reads(ctx); rng = np.random.default_rng(6401)
    assert ctx.reads_stats().max_read_length == top
    a, b, c = store[10], store[20], fx.revcomp(store[30])
    stranger, longer = rnd(rng, 80), rnd(rng, top + 1)
    assert int(H.expected_ids(ctx, [stranger], k)[0]) == 0
    mates = [a, b,                                                       # kept
             a[:5] + "N" + a[6:], b, a, b[:-1] + "N",                    # a mate with N, first or second
             a[:k], b, a, "",                                            # a mate of length k; an empty mate
             stranger, b, a, stranger,                                   # a good read that is not in the store
             longer, b, a, store[1] + rnd(rng, 1000),                    # mates longer than the store's longest read (good reads: not found)
             "N" + a[1:], stranger,                                      # one mate not good, the other not found: not good (:176 comes first)
             longer[:-1] + "N", b,                                       # too long AND not good
             c, a, b.lower(), c]                                         # kept; lower case is found like upper case
    R = Restated(); st = add(ctx, R, mates, k)
    assert (st.pairs_seen, st.pairs_added, st.pairs_not_good, st.pairs_not_found) == (13, 3, 6, 4)
    ent = compare(ctx, R)
    assert len(ent) == 6 and 0 not in ent["from"] and 0 not in ent["to"]
    for n, reads in ((0, []), (1, [a])):                                 # n = 0 and n = 1 are valid and add nothing
        st = add(ctx, R, reads, k)
        assert (st.pairs_seen, st.entries_after) == (0, 6)
    st = add(ctx, R, [a, c, b], k)                                       # odd n: the trailing read is dropped
    assert (st.pairs_seen, st.pairs_added) == (1, 1)
    compare(ctx, R)
    ctx.close()


def case_calls(device):
    k = 21
    ctx, reads = tiling_store(device, 500, 100, k, 6500, dup_every=5, dup_copies=1)
    mates = ordinary_pairs(reads) + [reads[0][:k], reads[1]] + ordinary_pairs(reads[:200])
    n = len(mates); cuts = [0, (n // 3) & ~1, (2 * n // 3) & ~1, n]
    R1 = Restated(); add(ctx, R1, mates, k, library=1)
    one = compare(ctx, R1, 1)
    R2 = Restated()
    for x in range(3):                                                   # cut at even positions: the same table, `first` included
        add(ctx, R2, mates[cuts[x]:cuts[x + 1]], k, library=2)
    three = compare(ctx, R2, 2)
    for f in ("from", "to", "type1", "type2", "count", "first", "freq"):
        assert np.array_equal(one[f], three[f]), f
    R3 = Restated(); odd = cuts[1] + 1                                   # a cut at an odd position drops that call's last read and shifts the pairing
    add(ctx, R3, mates[:odd], k, library=3); add(ctx, R3, mates[odd:], k, library=3)
    shifted = compare(ctx, R3, 3)
    assert len(shifted) != len(one) or not np.array_equal(shifted["first"], one["first"])
    compare(ctx, R1, 1)
    ctx.close()


DIGIT_EDGE_COUNTS = [1, 2, 3, 255, 256, 257, 65535, 65536]


def radix_passes(N):
    """8-bit digits of from:30 | to:30 | t:1 | t:1 (bits 61..32, 31..2, 1, 0) that can be non-zero for ids up to N"""
    b = int(N).bit_length()
    return sum(1 for lo in range(0, 64, 8) if lo < 2 + b or 32 <= lo < 32 + b)


def case_digit_edges(device, N):
    """ids 1 and N and the ids on both sides of every power of 256 below N, paired with each other on both strands: where a skipped radix pass would show"""
    k, L = 21, 50
    ctx, _ = tiling_store(device, N, L, k, 6600 + N)
    store = stored_reads(ctx)
    edge = sorted({1, N} | {x for p in (256, 65536) if p <= N for x in (p - 1, p, p + 1) if 1 <= x <= N} | {max(1, N // 2)})
    mates = []
    for x in edge:
        for y in edge:
            mates += [store[x], store[y], fx.revcomp(store[x]), store[y], store[x], fx.revcomp(store[y])]
    mates += mates[:40]
    R = Restated(); st = add(ctx, R, mates, k)
    ent = compare(ctx, R)
    assert set(ent["from"].tolist()) == set(edge) and st.pairs_added == len(mates) // 2
    if st.route == s2.MATE_ROUTE_DEVICE:
        assert st.sort_passes == radix_passes(N) and st.flushes == 1
        add(ctx, R, mates[:10], k)                                       # a second call: record sort and merge
        assert ctx.mates_stats().sort_passes == 2 * radix_passes(N)
        compare(ctx, R)
    ctx.close()


TILE_SEAM_PAIRS = [1023, 1024, 1025]


def case_tile_seams(device, P):
    """2 P = 2046 / 2048 / 2050 pending records, all with keys of their own, in one flush, then one more pair, whose merge sorts 2 P + 2 entries: the record
    counts on both sides of the 2048 items that a block of the scan and a tile of the radix sort take (SCAN_BLOCK, RS_TILE), in the sort, the heads and the merge"""
    k, n = 21, 300
    ctx, _ = tiling_store(device, n, 100, k, 7400)
    store = stored_reads(ctx)

    def pair(x):                                                         # reads i and i + d (mod n), d <= 5 < n / 2: no two x share their two reads, in either order
        i, d = x % n, 1 + x // n
        a, b = store[1 + i], store[1 + (i + d) % n]
        return [fx.revcomp(a) if x % 3 == 0 else a, fx.revcomp(b) if x % 4 == 1 else b]

    passes = radix_passes(n)
    on_device = device != HOST
    R = Restated(); st = add(ctx, R, [r for x in range(P) for r in pair(x)], k)
    assert (st.pairs_added, st.pairs_not_good, st.pairs_not_found, st.records, st.entries_after) == (P, 0, 0, 2 * P, 2 * P)      # every record an entry
    assert st.route == (s2.MATE_ROUTE_DEVICE if on_device else s2.MATE_ROUTE_HOST)
    assert (st.chunks, st.flushes, st.sort_passes) == ((1, 1, passes) if on_device else (0, 0, 0))                             # one sort of the records
    ent = compare(ctx, R)
    assert len(ent) == 2 * P and np.all(ent["count"] == 1)
    st = add(ctx, R, pair(4 * n), k)                                     # d = 5: a new pair
    assert (st.pairs_added, st.entries_before, st.entries_after) == (1, 2 * P, 2 * P + 2)
    assert (st.chunks, st.flushes, st.sort_passes) == ((1, 1, 2 * passes) if on_device else (0, 0, 0))                         # its two records, then the merge
    ent = compare(ctx, R)
    assert len(ent) == 2 * P + 2 and np.all(ent["count"] == 1)
    ctx.close()


def case_libraries(device, tmp_path):
    k = 21
    ctx, reads = tiling_store(device, 300, 100, k, 6700)
    mates = ordinary_pairs(reads)
    R = Restated()
    add(ctx, R, mates, k, library=1)
    assert ctx.mates_stats().libraries == 1
    add(ctx, R, mates[:200], k, library=2); add(ctx, R, mates[100:400], k, library=2)
    assert ctx.mates_stats().libraries == 2
    add(ctx, R, mates[:50], k, library=127)
    assert ctx.mates_stats().libraries == 127
    e1, e2, e127 = compare(ctx, R, 1), compare(ctx, R, 2), compare(ctx, R, 127)
    assert len(e1) > len(e2) > len(e127) > 0 and ctx.mates_count(5) == 0 and len(ctx.mates(5)[0]) == 0
    assert int(e1["count"].sum()) == len(mates) and int(e2["count"].sum()) == 500      # the same pairs under two libraries did not merge
    for library in (0, 128, -1, 1000):
        with pytest.raises(s2.Sage2ovError) as e:
            ctx.mates_add_ascii(*to_arrays(mates[:4]), library)
        assert e.value.code == -1 and "library" in str(e.value)
        with pytest.raises(s2.Sage2ovError):
            ctx.mates_count(library)
    compare(ctx, R, 1)
    ctx.mates_clear()
    assert [ctx.mates_count(x) for x in (1, 2, 127)] == [0, 0, 0] and ctx.mates_stats().libraries == 0
    R = Restated(); add(ctx, R, mates[:100], k, library=3)               # the ordinals start again
    assert int(compare(ctx, R, 3)["first"].min()) == 0
    p = str(tmp_path / "t.reads"); ctx.reads_save(p)
    ctx.reads_load(p)                                                    # a new read set drops the table
    assert ctx.mates_count(3) == 0 and ctx.mates_stats().libraries == 0
    R = Restated(); add(ctx, R, mates[:100], k, library=3); compare(ctx, R, 3)
    ctx.close()


def write_fasta(path, reads, opener=open):
    with opener(path, "wt") as f:
        for i, r in enumerate(reads):
            f.write(">m%d\n%s\n" % (i, r))


def write_fastq(path, reads):
    with open(path, "w") as f:
        for i, r in enumerate(reads):
            f.write("@m%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)))


def case_files(device, tmp_path, monkeypatch):
    k = 21
    monkeypatch.delenv("SAGE2OV_TEST_MATE_FILE_BATCH", raising=False)
    ctx, reads = tiling_store(device, 400, 100, k, 6800, dup_every=5, dup_copies=1)
    mates = ordinary_pairs(reads)[:801]                                  # an odd number of reads: the last one has no mate
    other = ordinary_pairs(reads[100:300])
    R = Restated(); add(ctx, R, mates, k, 1); add(ctx, R, other, k, 2)
    want1, want2 = compare(ctx, R, 1), compare(ctx, R, 2)
    fa, gz, q1, q2, lst = (str(tmp_path / n) for n in ("m.fa", "m.fa.gz", "m_1.fq", "m_2.fq", "mates.list"))
    write_fasta(fa, mates); write_fasta(gz, mates, gzip.open); write_fastq(q1, mates[0::2]); write_fastq(q2, mates[1::2])
    o1, o2 = str(tmp_path / "o_1.fa"), str(tmp_path / "o_2.fa")
    write_fasta(o1, other[0::2]); write_fasta(o2, other[1::2])

    def same(got, want):
        return all(np.array_equal(got[f], want[f]) for f in ("from", "to", "type1", "type2", "count", "first", "freq"))

    for batch in (None, "100", "7"):                                     # the default batch, and batches that cut the stream (an odd value is made even)
        if batch:
            monkeypatch.setenv("SAGE2OV_TEST_MATE_FILE_BATCH", batch); ctx.options_reload()
        for args in ((fa,), (gz,), (q1, q2)):
            ctx.mates_clear(); ctx.mates_add_file(*args, library=1)
            st = ctx.mates_stats()
            assert (st.pairs_seen, st.pairs_added, st.library) == (400, 400, 1)
            assert same(ctx.mates(1)[0], want1), (batch, args)
    open(lst, "w").write("# two datasets\nf = %s\n\nf1 = %s\nf2 = %s\n" % (fa, o1, o2))
    ctx.mates_clear(); ctx.mates_add_list(lst)
    assert same(ctx.mates(1)[0], want1) and same(ctx.mates(2)[0], want2)
    st = ctx.mates_stats()
    assert (st.library, st.libraries, st.pairs_seen) == (2, 2, len(other) // 2)
    for text in ("f1 = %s\nf = %s\n" % (o1, fa), "f2 = %s\n" % o2, "g = %s\n" % fa, "%s\n" % fa, "f1 = %s\n" % o1):
        open(lst, "w").write(text)                                       # wrong grammar (matePair.cpp:88-113)
        with pytest.raises(s2.Sage2ovError) as e:
            ctx.mates_add_list(lst)
        assert e.value.code == -2 and "format" in str(e.value)          # SAGE2OV_ERR_IO
    with pytest.raises(s2.Sage2ovError):
        ctx.mates_add_file(str(tmp_path / "absent.fa"), library=1)
    ctx.close()


MIRROR_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>
#include "sage2ov.hpp"
int main(int argc, char** argv) {      // <k> <device> <reads.fa> <mates.fa> <more.txt>: every list of library 1 and of library 2 in list order, then numberOfLibrary
    try {
        sage2ov::Context ctx((uint16_t)atoi(argv[1]), atoi(argv[2]));
        sage2ov::ReadLoader loader(ctx);
        loader.readDatasetInBytes(argv[3]);
        loader.organizeReads();
        sage2ov::MatePair mates(&loader);
        mates.mapMatePairs(argv[4], "", 1);
        std::vector<std::string> more; std::ifstream in(argv[5]); std::string line;
        while (std::getline(in, line)) more.push_back(line);
        mates.processMatePairs(more, 2);
        for (int library = 1; library <= 2; library++)
            for (uint64_t id = 0; id <= loader.numberOfUniqueReads + 1; id++)
                for (const sage2ov_mate& m : mates.list(id, library))
                    printf("%d %llu %u %u %u %u %llu\n", library, (unsigned long long)id, m.to, m.type1, m.type2, m.freq, (unsigned long long)m.count);
        printf("libraries %d\n", mates.numberOfLibrary());
    } catch (const sage2ov::Error& e) { fprintf(stderr, "error %d: %s\n", e.code, e.what()); return 1; }
    return 0;
}
"""


def case_cpp_mirror(device, tmp_path):
    """sage2ov.hpp compiles, and MatePair::list prints the restatement's lists in the restatement's order"""
    L, k = 100, 21
    pd = dict(recipe="tiling", seed=6900, n_unique=200, read_len=L, step=7, dup_every=5, dup_copies=1)
    fa = str(tmp_path / "r.fa"); fx.write_recipe_fasta(pd, fa)
    reads = fx.recipe_reads(pd)
    mates = ordinary_pairs(reads); more = ordinary_pairs(reads[:80]) + [reads[0]]
    mf, tf = str(tmp_path / "m.fa"), str(tmp_path / "more.txt")
    write_fasta(mf, mates); open(tf, "w").write("".join(q + "\n" for q in more))
    src, exe = str(tmp_path / "mirror.cpp"), str(tmp_path / "mirror")
    open(src, "w").write(MIRROR_CPP)
    libdir = os.path.join(fx.ROOT, "sage2_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(fx.ROOT, "include"), "-I", os.path.join(libdir, "csrc"), src, "-o", exe,
                    "-L", libdir, "-lsage2ov", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe, str(k), str(device), fa, mf, tf], check=True, stdout=subprocess.PIPE, text=True, timeout=120).stdout.splitlines()
    ctx = s2.Context(k, device=device); ctx.reads_add_file(fa); ctx.reads_organize()
    R = Restated(); R.add(ctx, mates, k, 1); R.add(ctx, more, k, 2)
    want = ["%d %d %d %d %d %d %d" % (library, a, w[0], w[1], w[2], w[4], w[5]) for library in (1, 2) for a in range(0, 202) for w in R.list(a, library)]
    assert out[-1] == "libraries 2" and out[:-1] == want and len(want) > 400
    ctx.close()


def case_errors(device):
    Lb = s2.lib(); k = 21
    ctx = s2.Context(k, device=device)
    reads = fx.recipe_reads(dict(recipe="tiling", seed=7000, n_unique=10, read_len=60, step=7))
    bases, off = to_arrays(reads)
    ctx.reads_add_ascii(bases, off)
    for call in (lambda: ctx.mates_add_ascii(bases, off, 1), lambda: ctx.mates_add_file("/nonexistent", library=1), lambda: ctx.mates_add_list("/nonexistent"),
                 lambda: ctx.mates_count(1), lambda: ctx.mates(1)):
        with pytest.raises(s2.Sage2ovError) as e:                        # before the reads are organised
            call()
        assert e.value.code == -1 and "organise" in str(e.value)
    ctx.reads_organize()
    pb, po = C.c_void_p(bases.ctypes.data), C.c_void_p(off.ctypes.data)
    assert Lb.sage2ov_mates_add_ascii(ctx._h, None, None, C.c_uint64(0), C.c_int(1)) == 0       # n = 0 needs no pointers
    for args in ((None, po), (pb, None)):
        assert Lb.sage2ov_mates_add_ascii(ctx._h, args[0], args[1], C.c_uint64(10), C.c_int(1)) == -1
        assert b"null" in Lb.sage2ov_last_error(ctx._h)
    assert Lb.sage2ov_mates_add_ascii(None, pb, po, C.c_uint64(10), C.c_int(1)) == -1
    assert Lb.sage2ov_mates_add_file(ctx._h, None, None, C.c_int(1)) == -1 and Lb.sage2ov_mates_add_list(ctx._h, None) == -1
    assert Lb.sage2ov_mates_count(ctx._h, C.c_int(1), None) == -1 and Lb.sage2ov_mates_stats_get(ctx._h, None) == -1
    with pytest.raises(s2.Sage2ovError):
        ctx.mates_add_ascii(bases, np.array([5, 0, 5], dtype=np.uint64), 1)
    assert ctx.mates_count(1) == 0
    R = Restated(); add(ctx, R, reads, k); ent = compare(ctx, R)
    n = len(ent); assert n == 10
    out = np.zeros(n, dtype=s2.MATE_DTYPE); po2 = C.c_void_p(out.ctypes.data)
    assert Lb.sage2ov_mates_export(ctx._h, C.c_int(1), po2, C.c_uint64(n - 1), None) == -1      # cap too small: nothing written
    assert b"fewer" in Lb.sage2ov_last_error(ctx._h) and not out["from"].any()
    assert Lb.sage2ov_mates_export(ctx._h, C.c_int(1), None, C.c_uint64(n), None) == -1
    assert Lb.sage2ov_mates_export(ctx._h, C.c_int(1), po2, C.c_uint64(n + 5), None) == 0 and np.array_equal(out, ent)      # without offsets
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- the host route
def test_ordinary_pairs():
    case_ordinary(HOST)


def test_freq_wraps_like_a_uint8():
    case_freq_wrap(HOST)


def test_self_pairs():
    case_self_pairs(HOST)


def test_skipped_pairs():
    case_skipped_pairs(HOST)


def test_calls():
    case_calls(HOST)


@pytest.mark.parametrize("N", DIGIT_EDGE_COUNTS)
def test_digit_edges(N):
    case_digit_edges(HOST, N)


@pytest.mark.parametrize("P", TILE_SEAM_PAIRS)
def test_tile_seams(P):
    case_tile_seams(HOST, P)


def test_radix_pass_count():
    assert [radix_passes(n) for n in DIGIT_EDGE_COUNTS] == [2, 2, 2, 3, 4, 4, 5, 6] and radix_passes(2 ** 30 - 1) == 8


def test_libraries(tmp_path):
    case_libraries(HOST, tmp_path)


def test_files(tmp_path, monkeypatch):
    case_files(HOST, tmp_path, monkeypatch)


def test_cpp_mirror(tmp_path):
    case_cpp_mirror(HOST, tmp_path)


def test_errors():
    case_errors(HOST)
    ctx = organised(21, ["ACGT" * 10], HOST)
    ctx.mates_add_ascii(*to_arrays(["ACGT" * 10] * 2), 1)
    st = ctx.mates_stats()
    assert (st.route, st.chunks, st.sort_passes, st.flushes, st.find_ms, st.sort_ms) == (s2.MATE_ROUTE_HOST, 0, 0, 0, 0.0, 0.0)
    ctx.close()
