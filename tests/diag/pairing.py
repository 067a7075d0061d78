"""tests/diag/pairing.py [--reads N] [--runs R] [--fasta PATH] -- what the mate table costs beside step 1: the BASELINE configs[1] input
(10 M x 150 bp, k = 40, seed 2) as the interleaved FASTA synth_write_fasta writes, every quantity as wall time of a fresh GPU context, median and range of
R runs (default 3) after one warm-up context:
  A  step 1 with pairing off:  reads_add_file + reads_organize
  B  step 1 with pairing on + mates_from_reads  (the one-pass route)
  C  step 1 with pairing off + mates_add_file on the same file  (the two-pass route, the only one before)
With a library that has no pairing calls (SAGE2OV_LIB=<the parent commit's libsage2ov.so>) B is skipped: A of the two libraries must agree within the spread.
SAGE2OV_TIMING=1 adds the library's own laps on stderr.  A diagnostic, not a test."""
import argparse, json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import fixtures as fx, sage2_amd as s2

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000); ap.add_argument("--runs", type=int, default=3); ap.add_argument("--fasta", default=None)
args = ap.parse_args()
n, k = args.reads & ~1, 40
fa = args.fasta or os.path.join(tempfile.mkdtemp(prefix="pairing_"), "reads.fa")
if not os.path.exists(fa):
    t0 = time.perf_counter(); s2.synth_write_fasta(fx.synth_params(dict(seed=2, genome_len=3 * n, n_reads=n, read_len=150)), fa)
    print(f"input: {n} reads, {os.path.getsize(fa) / 1e9:.2f} GB of FASTA written in {time.perf_counter() - t0:.1f} s", flush=True)
has_pairing = hasattr(s2.lib(), "sage2ov_mates_from_reads")


def run(mode):
    """-> (milliseconds of step 1, of the mate table, entries of library 1)"""
    ctx = s2.Context(k, device=0)
    t0 = time.perf_counter()
    if mode == "B":
        ctx.reads_pair_library(1)
    ctx.reads_add_file(fa); ctx.reads_organize()
    t1 = time.perf_counter()
    if mode == "B":
        ctx.mates_from_reads()
    elif mode == "C":
        ctx.mates_add_file(fa, None, 1)
    t2 = time.perf_counter()
    entries = ctx.mates_count(1) if mode != "A" else 0
    st = ctx.mates_stats() if mode != "A" else None
    if st:
        assert st.pairs_seen == n // 2 and st.pairs_not_found == 0
    ctx.close()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, entries


run("A")                                                                 # warm-up: the device, the page cache
modes = ["A", "B", "C"] if has_pairing else ["A", "C"]
rows = {m: [] for m in modes}
for _ in range(args.runs):                                               # interleaved: a drift of the machine shows in all three
    for m in modes:
        rows[m].append(run(m))
entries = {m: rows[m][0][2] for m in modes}
assert not has_pairing or entries["B"] == entries["C"], entries
out = {}
for m in modes:
    s1 = [r[0] for r in rows[m]]; mt = [r[1] for r in rows[m]]; tot = [a + b for a, b in zip(s1, mt)]
    out[m] = dict(step1_ms=dict(median=statistics.median(s1), min=min(s1), max=max(s1)), mates_ms=dict(median=statistics.median(mt), min=min(mt), max=max(mt)),
                  total_ms=dict(median=statistics.median(tot), min=min(tot), max=max(tot)))
    print(f"{m}: step 1 {out[m]['step1_ms']['median']:8.1f} ms ({min(s1):.1f} .. {max(s1):.1f})   mate table {out[m]['mates_ms']['median']:8.1f} ms ({min(mt):.1f} .. {max(mt):.1f})   "
          f"together {out[m]['total_ms']['median']:8.1f} ms ({min(tot):.1f} .. {max(tot):.1f})", flush=True)
print(json.dumps(dict(reads=n, runs=args.runs, library="with pairing" if has_pairing else "without pairing", entries=entries, **out)))
