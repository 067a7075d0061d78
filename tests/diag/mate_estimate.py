"""tests/diag/mate_estimate.py [--reads N] [--runs R] [--once] -- what MatePair::meanSdEstimation costs on the device (sage2ov_mates_map_reads,
sage2ov_mates_estimate): the BASELINE configs[1] workload (10 M x 150 bp, k = 40) through steps 1-4, the generator's interleaved mates (read 2j
and 2j + 1 are a pair) as library 1.  Prints, as the median of R runs (default 5, after one warm-up call): device milliseconds by HIP events per stage (scan,
records, sort, reduce, join, rounds), the wall time of the two calls, the table's size and the estimate.  A diagnostic, not a test.
--once: one map + estimate on the GPU context and nothing else (the run to put under `rocprofv3 --pmc`, counters in a run of their own)."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import fixtures as fx, sage2_amd as s2

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000); ap.add_argument("--runs", type=int, default=5); ap.add_argument("--once", action="store_true")
args = ap.parse_args()
n, k = args.reads & ~1, 40
p = fx.synth_params(dict(seed=2, genome_len=3 * n, n_reads=n, read_len=150))
t0 = time.perf_counter(); bases, off = s2.synth_reads_ascii(p, s2.synth_genome(p)); print(f"input: {n} reads in {time.perf_counter() - t0:.1f} s", flush=True)
STAGES = ("scan_ms", "records_ms", "sort_ms", "reduce_ms", "join_ms", "round_ms")

g = s2.Context(k, device=0); g.reads_add_ascii(bases, off); g.reads_organize(); g.run_steps23(); g.graph_simplify()
s4 = g.simplify_stats(); g.mates_add_ascii(bases, off, 1)
print(f"graph: {s4.edges} edge pairs, {s4.reads_on_edges} reads on their lists; mates: {g.mates_count(1)} entries", flush=True)


def run():
    t = time.perf_counter(); g.mates_map_reads(); t1 = time.perf_counter(); g.mates_estimate(); t2 = time.perf_counter()
    st = g.readmap_stats()
    return st, dict(map_wall_ms=(t1 - t) * 1e3, estimate_wall_ms=(t2 - t1) * 1e3, **{f: getattr(st, f) for f in STAGES})


st, first = run()                                                       # warm-up
if args.once:
    sys.exit(0)
rows = [run()[1] for _ in range(args.runs)]
med = {key: statistics.median(r[key] for r in rows) for key in rows[0]}
print("all runs:", json.dumps(rows), flush=True)
ins = g.mates_insert(1); lo, hi = g.mates_bounds()
# bytes the radix passes move per record: hist reads the key (8), scatter reads key + index (12) and writes them (12)
print(json.dumps(dict(reads=n, unique=int(g.reads_stats().unique_reads), records=int(st.records), entries=int(st.entries), mate_entries=int(st.mate_entries), distances=int(st.distances[1]),
                      radix_passes=st.sort_passes, round_launches=st.rounds, sort_bytes_per_record=32 * st.sort_passes,
                      sort_GBps=32.0 * st.sort_passes * st.records / (med["sort_ms"] * 1e-3) / 1e9 if med["sort_ms"] else None, **med,
                      valid=ins.valid, rounds=ins.rounds, final=ins.final_round, mean=ins.mean, sd=ins.deviation, lower=ins.lower, upper=ins.upper, min_upper=lo, max_upper=hi)))
