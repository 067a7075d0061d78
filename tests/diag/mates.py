"""tests/diag/mates.py [--reads N] [--runs R] [--once] -- what building the mate-pair table (sage2ov_mates_add_ascii) costs: the BASELINE configs[1]
workload (10 M x 150 bp, k = 40), all input reads as interleaved mates (5 M pairs, 10 M directed records).  Prints, as the median of R runs (default 5, each
into a cleared table, after one warm-up call that also builds the look-up directory): device milliseconds by HIP events per phase (find, records, sort, reduce,
merge) and the wall time of the call; beside them the route an integrator had before this call existed -- reads_find_ids on the device, the ids downloaded, the
record keys built, sorted and made unique on the host with 16 threads (numpy's sort is single-threaded: the keys are cut into 16 slices sorted by a thread pool
and merged by one final sort of the unique slices) -- and the host route of a device-less context with 16 host threads.  A diagnostic, not a test.
--once: one add call on the GPU context and nothing else (the run to put under `rocprofv3 --pmc`, counters in a run of their own)."""
import argparse, json, os, statistics, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import fixtures as fx, sage2_amd as s2

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000); ap.add_argument("--runs", type=int, default=5); ap.add_argument("--once", action="store_true")
args = ap.parse_args()
n, k = args.reads & ~1, 40
p = fx.synth_params(dict(seed=2, genome_len=3 * n, n_reads=n, read_len=150))
t0 = time.perf_counter(); bases, off = s2.synth_reads_ascii(p, s2.synth_genome(p)); print(f"input: {n} reads, {bases.size / 1e9:.2f} GB of ASCII in {time.perf_counter() - t0:.1f} s", flush=True)
PHASES = ("find_ms", "records_ms", "sort_ms", "reduce_ms", "merge_ms")


def timed(ctx, runs):
    rows = []
    for _ in range(runs):
        ctx.mates_clear()
        t = time.perf_counter(); ctx.mates_add_ascii(bases, off, 1); wall = (time.perf_counter() - t) * 1e3
        st = ctx.mates_stats(); rows.append(dict(wall_ms=wall, **{f: getattr(st, f) for f in PHASES}))
    return st, {key: statistics.median(r[key] for r in rows) for key in rows[0]}, rows


def parent_route(ctx):
    """reads_find_ids on the device + sort / unique of the record keys on the host, 16 threads"""
    t = time.perf_counter()
    ids = ctx.reads_find_ids(bases, off); t_find = time.perf_counter()
    a, b = ids[0::2], ids[1::2]; keep = (a != 0) & (b != 0); a, b = a[keep], b[keep]
    ia, ib, ta, tb = np.abs(a).astype(np.uint64), np.abs(b).astype(np.uint64), (a > 0).astype(np.uint64), (b > 0).astype(np.uint64)
    keys = np.concatenate([(ia << np.uint64(32)) | (ib << np.uint64(2)) | (ta << np.uint64(1)) | tb, (ib << np.uint64(32)) | (ia << np.uint64(2)) | (tb << np.uint64(1)) | ta])
    with ThreadPoolExecutor(16) as ex:
        parts = list(ex.map(lambda s: np.unique(s, return_counts=True), np.array_split(keys, 16)))
    allk = np.concatenate([x[0] for x in parts]); allc = np.concatenate([x[1] for x in parts])
    order = np.argsort(allk, kind="stable"); allk, allc = allk[order], allc[order]
    head = np.concatenate([[True], allk[1:] != allk[:-1]]); uk = allk[head]; uc = np.add.reduceat(allc, np.nonzero(head)[0])
    t_end = time.perf_counter()
    return uk, uc, dict(find_wall_ms=(t_find - t) * 1e3, host_sort_unique_ms=(t_end - t_find) * 1e3, wall_ms=(t_end - t) * 1e3)


g = s2.Context(k, device=0); g.reads_add_ascii(bases, off); g.reads_organize()
N = g.reads_stats().unique_reads
st, _, first = timed(g, 1)                                              # warm-up: builds the directory
assert st.pairs_added == n // 2 and st.route == s2.MATE_ROUTE_DEVICE
print(f"store: {N} unique reads; {st.pairs_added} pairs -> {st.entries_after} entries; chunks {st.chunks}, radix passes {st.sort_passes}, flushes {st.flushes}", flush=True)
if args.once:
    sys.exit(0)
st, gm, grows = timed(g, args.runs)
print("device route, all runs:", json.dumps(grows), flush=True)
ent, _ = g.mates(1)
prow = []
for _ in range(args.runs):
    uk, uc, row = parent_route(g); prow.append(row)
pm = {key: statistics.median(r[key] for r in prow) for key in prow[0]}
key = (ent["from"].astype(np.uint64) << np.uint64(32)) | (ent["to"].astype(np.uint64) << np.uint64(2)) | (ent["type1"].astype(np.uint64) << np.uint64(1)) | ent["type2"].astype(np.uint64)
assert np.array_equal(key, uk) and np.array_equal(ent["count"], uc.astype(np.uint64))
print("find_ids on the device + host sort/unique (16 threads), all runs:", json.dumps(prow), flush=True)
h = s2.Context(k, device=-2, host_threads=16)
words, freq = g.reads_export_words(); rs = g.reads_stats()
h.reads_import_words(words, rs.unique_reads, rs.words_per_read, rs.max_read_length, freq, rs.good_reads, rs.total_bp)
_, hm, hrows = timed(h, args.runs)
eh, _ = h.mates(1)
assert np.array_equal(ent, eh)
print("host route (16 threads), all runs:", json.dumps(hrows), flush=True)
# bytes the radix passes move per record: hist reads the key (8), scatter reads key + index (12) and writes them (12)
passes = st.sort_passes; sort_bytes = 32.0 * passes * st.records
print(json.dumps(dict(reads=n, unique=int(N), pairs=int(st.pairs_added), records=int(st.records), entries=int(st.entries_after), chunks=st.chunks, radix_passes=passes,
                      **{"device_" + f: gm[f] for f in PHASES}, device_call_wall_ms=gm["wall_ms"], sort_bytes_per_record=32 * passes,
                      sort_GBps=sort_bytes / (gm["sort_ms"] * 1e-3) / 1e9 if gm["sort_ms"] else None,
                      parent_route_wall_ms=pm["wall_ms"], parent_find_wall_ms=pm["find_wall_ms"], parent_host_sort_unique_ms=pm["host_sort_unique_ms"],
                      host16_call_wall_ms=hm["wall_ms"])))
