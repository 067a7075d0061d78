"""tests/diag/links.py [--reads N] [--runs R] [--once] -- what the sweep that opens ScaffoldMaker::mergeFinal / mergeFinalSmall costs on the device (sage2ov_links;
DESIGN.md 5.14): the BASELINE configs[1] workload (10 M x 150 bp, k = 40) through steps 1-4, the generator's interleaved mates (read 2j and 2j + 1 are a pair) as
library 1.  Prints, as the median of R runs (default 5, after one warm-up call): device milliseconds by HIP events per stage (halves, scan, records, sort, reduce),
the wall time of the call, and the table's size under the three filters.  A diagnostic, not a test.
NOT RUN YET: no number from this script stands in any document.
--once: one links call on the GPU context and nothing else (the run to put under `rocprofv3 --pmc`, counters in a run of their own)."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import fixtures as fx, sage2_amd as s2

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000); ap.add_argument("--runs", type=int, default=5); ap.add_argument("--once", action="store_true")
args = ap.parse_args()
n, k = args.reads & ~1, 40
p = fx.synth_params(dict(seed=2, genome_len=3 * n, n_reads=n, read_len=150))
t0 = time.perf_counter(); bases, off = s2.synth_reads_ascii(p, s2.synth_genome(p)); print(f"input: {n} reads in {time.perf_counter() - t0:.1f} s", flush=True)
STAGES = ("halves_ms", "scan_ms", "records_ms", "sort_ms", "reduce_ms")

g = s2.Context(k, device=0); g.reads_add_ascii(bases, off); g.reads_organize(); g.run_steps23(); g.graph_simplify()
s4 = g.simplify_stats(); g.mates_add_ascii(bases, off, 1); g.mates_estimate()
print(f"graph: {s4.edges} edge pairs, {s4.reads_on_edges} reads on their lists; mates: {g.mates_count(1)} entries; max upper bound {g.mates_bounds()[1]}", flush=True)


def run():
    t = time.perf_counter(); g.links_build(); t1 = time.perf_counter()             # (links_build always builds)
    st = g.link_stats()
    return st, dict(wall_ms=(t1 - t) * 1e3, **{f: getattr(st, f) for f in STAGES})


st, first = run()                                                       # warm-up
if args.once:
    sys.exit(0)
rows = [run()[1] for _ in range(args.runs)]
med = {key: statistics.median(r[key] for r in rows) for key in rows[0]}
print("all runs:", json.dumps(rows), flush=True)
print(json.dumps(dict(reads=n, unique=int(g.reads_stats().unique_reads), halves=int(st.halves), entries_within=int(st.entries_within), unique_entries=int(st.unique_entries),
                      mate_entries=int(st.mate_entries), records=int(st.records), keys=int(st.keys), rows_final=len(g.links(s2.LINKS_FINAL)), rows_small=len(g.links(s2.LINKS_SMALL)),
                      radix_passes=st.sort_passes, **med)))
