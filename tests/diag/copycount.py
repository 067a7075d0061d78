"""tests/diag/copycount.py [--reads N] [--err-ppm E] [--runs R] -- what step 5 around its solver costs on the device (sage2ov_genome_size_estimate,
sage2ov_flow_network_*): a BASELINE-like workload (default configs[1]: 10 M x 150 bp, k = 40; --reads 50000000 is configs[2]) through steps 1-4,
then the estimate and the network R times (default 5, after one warm-up).  Prints the medians of the HIP-event times per stage (prepare = k of every pair and the
present reads, rounds, order = the two sorts and the node ranks, classes, arcs = arc records with the cost fold), the wall time of estimate + build and of the
export of the arc records, and the sizes.  No solver runs, so nothing is applied.  A diagnostic, not a test."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import fixtures as fx, sage2_amd as s2

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000); ap.add_argument("--runs", type=int, default=5); ap.add_argument("--err-ppm", type=int, default=0)
args = ap.parse_args()
n, k, L = args.reads, 40, 150
p = fx.synth_params(dict(seed=2, genome_len=3 * n, n_reads=n, read_len=L, err_ppm=args.err_ppm))
t0 = time.perf_counter(); bases, off = s2.synth_reads_ascii(p, s2.synth_genome(p)); print(f"input: {n} reads in {time.perf_counter() - t0:.1f} s", flush=True)
STAGES = ("prepare_ms", "rounds_ms", "order_ms", "classes_ms", "arcs_ms")

g = s2.Context(k, device=0); g.reads_add_ascii(bases, off); g.reads_organize(); g.run_steps23()


def run():
    g.graph_simplify()                                                  # (drops estimate and network: every run starts from the graph alone)
    t = time.perf_counter(); g.genome_size(); g.flow_network_build(); t1 = time.perf_counter()
    arcs = g.flow_network(); t2 = time.perf_counter()
    st = g.copycount_stats()
    return st, dict(estimate_and_build_wall_ms=(t1 - t) * 1e3, export_wall_ms=(t2 - t1) * 1e3, **{f: getattr(st, f) for f in STAGES}), len(arcs)


st, first, narcs = run()
s4 = g.simplify_stats()
print(f"graph: {s4.edges} edge pairs, {s4.reads_on_edges} reads on their lists", flush=True)
rows = [run()[1] for _ in range(args.runs)]
med = {key: statistics.median(r[key] for r in rows) for key in rows[0]}
print("all runs:", json.dumps(rows), flush=True)
print(json.dumps(dict(reads=n, err_ppm=args.err_ppm, unique=int(g.reads_stats().unique_reads), genome_size=int(st.genome_size), rounds=int(st.rounds), degenerate=int(st.degenerate),
                      reads_present=int(st.reads_present), nodes=int(st.nodes), edges=int(st.edges), simple=int(st.simple), once=int(st.once), many=int(st.many),
                      network_nodes=int(st.network_nodes), network_arcs=int(narcs), **med)))
