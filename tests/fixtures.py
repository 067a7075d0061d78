"""Shared helpers: golden fixture metadata, synthetic reads, md5."""
import glob
import gzip
import hashlib
import json
import os

import sage2_amd as s2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def golden_names_all():
    """every fixture the reference binary produced (oracle/make_golden.py), including the ones pinned by md5 + size only"""
    return sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(GOLDEN, "*.json")) if not p.endswith(".step4.json") and not p.endswith("_digest.json") and not p.endswith(".hashtable.json"))


def golden_names():
    """the fixtures whose P.graph3 is committed (and that have a step-4 dump)"""
    return [n for n in golden_names_all() if os.path.exists(os.path.join(GOLDEN, n + ".graph3.gz"))]


def golden(name):
    return json.load(open(os.path.join(GOLDEN, name + ".json")))


def golden_graph3(name) -> bytes:
    return gzip.open(os.path.join(GOLDEN, name + ".graph3.gz"), "rb").read()


def graph3_matches(path, name):
    """the written P.graph3 against the reference's: byte for byte where the file is committed, md5 + size for the big fixtures"""
    gz = os.path.join(GOLDEN, name + ".graph3.gz")
    if os.path.exists(gz):
        return open(path, "rb").read() == gzip.open(gz, "rb").read()
    m = golden(name)
    return os.path.getsize(path) == m["graph3_size"] and md5_file(path) == m["graph3_md5"]


def md5_file(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()


def synth_params(d) -> s2.SynthParams:
    return s2.SynthParams(**d)


def recipe_reads(pd):
    """Hand-made inputs the generator never produces (dict with a "recipe" key) -> list of read strings, deterministic from the dict.
    tiling, low_complexity, short_reads, heavy_duplicates: see _RECIPES below.
    palindrome_tandem: a genome that is its own reverse complement around a centre (reads at mirrored positions share a canonical
    form; reads across the centre equal their own reverse complement), a tandem repeat of period 7 (several overlaps per read pair,
    a read's prefix equal to its own later windows), embedded in random sequence long enough for the reference (> 12.5 k unique reads)."""
    import numpy as np
    if pd["recipe"] in _RECIPES:
        return _RECIPES[pd["recipe"]](pd)
    assert pd["recipe"] == "palindrome_tandem"
    rng = np.random.default_rng(pd["seed"])
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    def rc(s): return "".join(comp[c] for c in reversed(s))
    def rnd(n): return "".join(rng.choice(list("ACGT"), size=n))
    half = rnd(pd["half"])
    genome = rnd(pd["flank"]) + half + rc(half) + rnd(200) + "ACGTTGA" * pd["tandem_units"] + rnd(pd["flank"])
    L, step, reads = pd["read_len"], pd["step"], []
    for i, p0 in enumerate(range(0, len(genome) - L + 1, step)):
        s = genome[p0:p0 + L]
        reads.append(s if i % 2 == 0 else rc(s))
    return reads


_COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def _rnd(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n))


def _tile(genome, L, step, n=None):
    """reads of L bases every `step` bases of the genome, odd ones reverse-complemented"""
    starts = range(0, len(genome) - L + 1, step)
    return [genome[p:p + L] if i % 2 == 0 else revcomp(genome[p:p + L]) for i, p in enumerate(starts) if n is None or i < n]


def _tiling(pd):
    """tiling: a random genome of (n_unique - 1) * step + read_len bases cut into reads at a fixed step, alternating strands: EXACTLY n_unique unique
    reads (two equal windows of a random genome of this size do not happen; the tests assert the count).  dup_every / dup_copies: every dup_every-th read
    is repeated dup_copies more times, on alternating strands."""
    import numpy as np
    rng = np.random.default_rng(pd["seed"])
    n, L, step = pd["n_unique"], pd["read_len"], pd["step"]
    reads = _tile(_rnd(rng, (n - 1) * step + L), L, step)
    assert len(reads) == n
    if pd.get("dup_every"):
        for i in range(0, n, pd["dup_every"]):
            reads += [reads[i] if c % 2 else revcomp(reads[i]) for c in range(pd.get("dup_copies", 1))]
    return reads


LOW_COMPLEXITY_UNITS = ("A", "AT", "CAG", "AACGTC", "T", "GA")          # periods 1, 2, 3, 6; (AT)n is its own reverse complement, poly-A / poly-T each other's


def _low_complexity(pd):
    """low_complexity: random flanks of `flank` bases around one block of `block` bases (> read_len) per unit of LOW_COMPLEXITY_UNITS: homopolymers
    (keys 0 and all-ones, forward and reverse key tie), (AT)n (reads equal to their own reverse complement), microsatellites of period 2, 3 and 6 (a key
    many times inside ONE read, overlaps at every multiple of the period).  Reads tiled at `step` (1 .. 3) on alternating strands."""
    import numpy as np
    rng = np.random.default_rng(pd["seed"])
    L, blk = pd["read_len"], pd["block"]
    assert blk > L and 1 <= pd["step"] <= 3
    genome = _rnd(rng, pd["flank"])
    for u in LOW_COMPLEXITY_UNITS:
        genome += (u * (blk // len(u) + 1))[:blk] + _rnd(rng, pd["flank"])
    return _tile(genome, L, pd["step"])


def _short_reads(pd):
    """short_reads: a random genome tiled at `step`; the read at every position is cut to k + 1, k + 2 or k + 3 bases (the shortest reads that are good: two to four
    windows), to a length anywhere up to `top`, or left at `top` (the longest read of a read-store layout) -- a third each, in that order, strands alternating."""
    import numpy as np
    rng = np.random.default_rng(pd["seed"])
    k, top, step, n = pd["k"], pd["top"], pd["step"], pd["n_reads"]
    assert top > k + 3
    genome = _rnd(rng, (n - 1) * step + top)
    mid = rng.integers(k + 4, top + 1, size=n)
    reads = []
    for i in range(n):
        L = (k + 1 + (i // 3) % 3) if i % 3 == 0 else (int(mid[i]) if i % 3 == 1 else top)
        p = i * step + (int(rng.integers(0, top - L + 1)) if i % 3 == 0 else 0)       # (the short ones anywhere inside the long read of their position)
        s = genome[p:p + L]
        reads.append(s if i % 2 == 0 else revcomp(s))
    return reads


HEAVY_COPIES = (65535, 65536, 65537)                                     # frequencies 65 535, 0 and 1 in the reference's uint16_t (readLoader.cpp:232)


def _heavy_duplicates(pd):
    """heavy_duplicates: a tiling of n_unique reads in which three reads (at 1/4, 1/2 and 3/4 of the genome) occur 65 535, 65 536 and 65 537 times in all,
    the copies on alternating strands and placed behind the tiling."""
    reads = _tiling(dict(pd, dup_every=0))
    n = len(reads)
    for q, copies in enumerate(HEAVY_COPIES):
        r = reads[(q + 1) * n // 4]
        twin = revcomp(r)
        reads += [r if c % 2 else twin for c in range(copies - 1)]
    return reads


_RECIPES = {"tiling": _tiling, "low_complexity": _low_complexity, "short_reads": _short_reads, "heavy_duplicates": _heavy_duplicates}


def write_recipe_fasta(pd, path):
    with open(path, "w") as f:
        for i, r in enumerate(recipe_reads(pd)):
            f.write(">r%d\n%s\n" % (i, r))


def make_reads(pd):
    """(bases u8 array, offsets u64 array) of the synthetic data set described by dict pd."""
    if "recipe" in pd:
        import numpy as np
        reads = recipe_reads(pd)
        bases = np.frombuffer("".join(reads).encode(), dtype=np.uint8).copy()
        off = np.zeros(len(reads) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(r) for r in reads])
        return bases, off
    p = synth_params(pd)
    g = s2.synth_genome(p)
    return s2.synth_reads_ascii(p, g)
