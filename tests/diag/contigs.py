"""tests/diag/contigs.py [--reads N] [--runs R] [--once] -- what the contig table and the spelling of the contig strings cost on the device (sage2ov_contigs_*;
DESIGN.md 5.13): the BASELINE configs[1] workload (10 M x 150 bp, k = 40) through steps 1-4, then contigs_build and the spelling of every string in one range.
Prints, as the median of R runs (default 5, after one warm-up call): device milliseconds by HIP events per stage (select, sort, layout, spell -- the spelling
kernel alone), the wall time of the build and of the sequences call (which includes the copy to the host and the compaction), the table's size, and the spell
kernel's own byte count: the characters written (every row rounded up to 16) plus the 64-byte lines of the read store it touches, counted on the host from the
graph -- one line per list entry and per end read at least, every line a read's used bases span at most: both bounds are printed.
A diagnostic, not a test.  NOT RUN YET: no number from this script stands in any document.
--once: one build and one spelling on the GPU context and nothing else (the run to put under `rocprofv3 --kernel-trace --stats`)."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import fixtures as fx, sage2_amd as s2

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000); ap.add_argument("--runs", type=int, default=5); ap.add_argument("--once", action="store_true")
args = ap.parse_args()
n, k, L = args.reads, 40, 150
p = fx.synth_params(dict(seed=2, genome_len=3 * n, n_reads=n, read_len=L))
t0 = time.perf_counter(); bases, off = s2.synth_reads_ascii(p, s2.synth_genome(p)); print(f"input: {n} reads in {time.perf_counter() - t0:.1f} s", flush=True)
STAGES = ("select_ms", "sort_ms", "layout_ms", "spell_ms")

g = s2.Context(k, device=0); g.reads_add_ascii(bases, off); g.reads_organize(); g.run_steps23(); g.graph_simplify()
s4 = g.simplify_stats()
print(f"graph: {s4.edges} edge pairs, {s4.reads_on_edges} reads on their lists", flush=True)


def run():
    t = time.perf_counter(); g.contigs_build(0, 3 * n); t1 = time.perf_counter()
    lens = g.contigs()["string_length"]
    t2 = time.perf_counter(); seq, offs = g.contig_sequences(0, len(lens), lens); t3 = time.perf_counter()
    st = g.contig_stats()
    return st, lens, dict(build_wall_ms=(t1 - t) * 1e3, sequences_wall_ms=(t3 - t2) * 1e3, **{f: getattr(st, f) for f in STAGES})


st, lens, first = run()                                                 # warm-up
if args.once:
    sys.exit(0)
rows = [run()[2] for _ in range(args.runs)]
med = {key: statistics.median(r[key] for r in rows) for key in rows[0]}
out_bytes = int(((lens.astype(np.int64) + 15) // 16 * 16).sum())
words = int(g.reads_stats().words_per_read); entries = int(s4.reads_on_edges)
# a spelled list entry touches the line that holds its last distPrevious bases (at least one 64-byte line, at most the read's ceil(2 L / 512) lines); so do the two end reads
lines_min = (entries // 2 + 2 * len(lens)) * 64                         # (reads_on_edges counts both halves of a pair; one half of each pair is spelled)
lines_max = lines_min * ((2 * L + 511) // 512)
print("all runs:", json.dumps(rows), flush=True)
print(json.dumps(dict(reads=n, unique=int(g.reads_stats().unique_reads), contigs=int(st.contigs), written=int(st.written), longest=int(st.longest), n50=int(st.n50),
                      string_bytes=int(lens.sum()), spell_output_bytes=out_bytes, spell_read_store_bytes=[lines_min, lines_max], words_per_read=words, **med)))
