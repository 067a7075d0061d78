import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import fixtures as fx, sage2_amd as s2
n = int(sys.argv[1])
p = fx.synth_params(dict(seed=3 if n == 50_000_000 else 2, genome_len=3 * n, n_reads=n, read_len=150))
ctx = s2.Context(40, device=0); ctx.reads_add_synth(p, s2.synth_genome(p)); ctx.reads_organize()
ctx.run_steps23()
for rep in range(2):
    t0 = time.perf_counter(); ctx.index_build(); t1 = time.perf_counter(); ctx.overlap_initial(); t2 = time.perf_counter(); ctx.overlap_reduce(); t3 = time.perf_counter(); ctx.overlap_convert(); t4 = time.perf_counter()
    tm = ctx.timings()
    print(f"wall: index {1e3*(t1-t0):.2f} initial {1e3*(t2-t1):.2f} reduce {1e3*(t3-t2):.2f} convert {1e3*(t4-t3):.2f} total {1e3*(t4-t0):.2f} | events: index {tm.index_ms:.2f} probe {tm.probe_ms:.2f} recip {tm.reciprocal_ms:.2f} reduce {tm.reduce_ms:.2f} convert {tm.convert_ms:.2f}")
    ctx.timings_reset()
