"""tests/diag/find_ids.py [--reads N] [--runs R] [--once] -- what a batched read-id look-up (sage2ov_reads_find_ids) costs: the BASELINE configs[1]
workload (10 M x 150 bp, k = 40), the queries are all input reads.  Prints, as the median of R runs (default 5) after one call that also builds the directory:
device milliseconds by HIP events for classify + pack, for the directory and for the search; the wall time of the call, transfers included; and the same call on a
device-less context with 16 host threads (the reference's method: a binary search per read over the host copy of the store).  A diagnostic, not a test.
--once: one look-up on the GPU context and nothing else (the run to put under `rocprofv3 --pmc`, counters in a run of their own)."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import fixtures as fx, sage2_amd as s2

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000); ap.add_argument("--runs", type=int, default=5); ap.add_argument("--once", action="store_true")
args = ap.parse_args()
n, k = args.reads, 40
p = fx.synth_params(dict(seed=2, genome_len=3 * n, n_reads=n, read_len=150))
t0 = time.perf_counter(); bases, off = s2.synth_reads_ascii(p, s2.synth_genome(p)); print(f"input: {n} reads, {bases.size / 1e9:.2f} GB of ASCII in {time.perf_counter() - t0:.1f} s", flush=True)


def timed(ctx, runs):
    rows = []
    for _ in range(runs):
        t = time.perf_counter(); ids = ctx.reads_find_ids(bases, off); wall = (time.perf_counter() - t) * 1e3
        st = ctx.reads_find_stats(); rows.append(dict(wall_ms=wall, pack_ms=st.pack_ms, search_ms=st.search_ms, directory_ms=st.directory_ms))
    return ids, st, {key: statistics.median(r[key] for r in rows) for key in rows[0]}, rows


g = s2.Context(k, device=0); g.reads_add_ascii(bases, off); g.reads_organize()
N = g.reads_stats().unique_reads
ids, st, _, first = timed(g, 1)                                          # builds the directory
assert st.found == n and np.all(ids != 0)
print(f"store: {N} unique reads, {g.reads_stats().words_per_read} words per read; directory: {st.directory_bits} bits, built in {first[0]['directory_ms']:.3f} ms; chunks per call: {st.launches}", flush=True)
if args.once:
    sys.exit(0)
gid, st, gm, grows = timed(g, args.runs)
print("device route, all runs:", json.dumps(grows), flush=True)
h = s2.Context(k, device=-2, host_threads=16)
words, freq = g.reads_export_words(); rs = g.reads_stats()
h.reads_import_words(words, rs.unique_reads, rs.words_per_read, rs.max_read_length, freq, rs.good_reads, rs.total_bp)
timed(h, 1)
hid, _, hm, hrows = timed(h, args.runs)
assert np.array_equal(gid, hid)
print("host route (16 threads), all runs:", json.dumps(hrows), flush=True)
print(json.dumps(dict(reads=n, unique=int(N), directory_bits=st.directory_bits, chunks=st.launches, device_pack_ms=gm["pack_ms"], device_search_ms=gm["search_ms"],
                      device_directory_ms=first[0]["directory_ms"], device_call_wall_ms=gm["wall_ms"], host16_call_wall_ms=hm["wall_ms"])))
