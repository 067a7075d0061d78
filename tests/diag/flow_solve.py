"""tests/diag/flow_solve.py [--goldens] [--reads N --err-ppm E] [--max-rounds R] -- what step 5's solver costs on the device (sage2ov_mcf_solve, sage2ov_flow_solve;
DESIGN.md 5.20).  --goldens (the default): the networks of tests/golden/g4_highcopy_k21 and g13_noisy300_k55 through mcf_solve, each held against the certificate
and its optimum.  --reads N: a BASELINE-like workload (N x 150 bp, k = 40, as tests/diag/copycount.py builds it) through steps 1-4 and the network, then
flow_solve with the round budget R (default: the library's); when the budget is spent the round and the phase it stopped in are printed.  Such a network is
timed, and held against the certificate when it finishes.  Per epsilon phase: rounds and HIP-event time; per solve: phases, rounds, pushes, relabels, price
updates.  A diagnostic, not a test."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import fixtures as fx, flow_model as fm, flowgen as fg, sage2_amd as s2

ap = argparse.ArgumentParser()
ap.add_argument("--goldens", action="store_true"); ap.add_argument("--reads", type=int, default=0); ap.add_argument("--err-ppm", type=int, default=0); ap.add_argument("--max-rounds", type=int, default=0)
args = ap.parse_args()
OPTIMA = {"g4_highcopy_k21": 2227089582, "g13_noisy300_k55": 19999938}


def report(name, st, wall, extra):
    ph = int(st.phases)
    print(json.dumps(dict(network=name, nodes=int(st.nodes), arcs=int(st.arcs), form=int(st.form), phases=ph, rounds=int(st.rounds), pushes=int(st.pushes), relabels=int(st.relabels),
                          price_updates=int(st.price_updates), total_cost=int(st.total_cost), build_ms=round(st.build_ms, 3), solve_ms=round(st.solve_ms, 3), wall_ms=round(wall * 1e3, 3),
                          refine_rounds=[int(x) for x in st.refine_rounds[:ph]], refine_ms=[round(x, 3) for x in st.refine_ms[:ph]], **extra)), flush=True)


if args.goldens or not args.reads:
    ctx = s2.Context(21, device=0)
    for name, opt in OPTIMA.items():
        n, fr, to, lo, up, co = fm.parse_input_cs2(os.path.join(fx.GOLDEN, name + ".input.cs2.gz"))
        a = np.zeros(len(fr), fg.ARC); a["from"], a["to"], a["lower"], a["upper"], a["cost"] = fr, to, lo, up, co
        ctx.mcf_solve(n, a)                                                           # warm-up
        t = time.perf_counter(); flow, price, st = ctx.mcf_solve(n, a, args.max_rounds); wall = time.perf_counter() - t
        cost = fm.certificate(n, fr, to, lo, up, co, flow, price, st.scale)
        report(name, st, wall, dict(certificate="ok", optimum=opt, reached=bool(cost == opt)))
    ctx.close()
if args.reads:
    n, k, L = args.reads, 40, 150
    p = fx.synth_params(dict(seed=2, genome_len=3 * n, n_reads=n, read_len=L, err_ppm=args.err_ppm))
    t0 = time.perf_counter(); bases, off = s2.synth_reads_ascii(p, s2.synth_genome(p)); print(f"input: {n} reads in {time.perf_counter() - t0:.1f} s", flush=True)
    g = s2.Context(k, device=0); g.reads_add_ascii(bases, off); g.reads_organize(); g.run_steps23(); g.graph_simplify(); g.genome_size(); g.flow_network_build()
    cs = g.copycount_stats(); print(f"network: {cs.network_nodes} nodes, {cs.network_arcs} arcs", flush=True)
    t = time.perf_counter()
    try:
        st = g.flow_solve(args.max_rounds); wall = time.perf_counter() - t
        arcs = g.flow_network(); flow, price, scale = g.flow_solution()
        cost = fm.certificate(int(cs.network_nodes), arcs["from"].astype(np.int64), arcs["to"].astype(np.int64), arcs["lower"], arcs["upper"],
                              np.trunc(arcs["cost"].astype(np.float64)).astype(np.int64), flow, price, scale)
        report(f"{n} reads, {args.err_ppm} ppm", st, wall, dict(certificate="ok", reached=bool(cost == st.total_cost)))
    except s2.Sage2ovError as e:
        wall = time.perf_counter() - t; st = g.mcf_stats()
        report(f"{n} reads, {args.err_ppm} ppm", st, wall, dict(stopped=str(e), stopped_in_phase=int(st.phases), stopped_at_round=int(st.rounds)))
    g.close()
