"""tests/diag/flow_solve_wide.py [--widths] [--reads N --err-ppm E] [--max-rounds R] [--twice] -- step 5's solver with 128-bit prices on the device
(sage2ov_mcf_solve_wide, the width sage2ov_flow_solve chooses).
--widths (the default): g4_highcopy_k21, g13_noisy300_k55 and the generated 1 602-node network through mcf_solve at both widths, side by side: the rounds (which
must be equal, as flows, prices and counters must) and the HIP-event time of the rounds, three solves each after a warm-up.
--reads N: a BASELINE-like noisy workload (N x 150 bp, k = 40, as tests/diag/flow_solve.py builds it) through steps 1-4 and the network; with
SAGE2OV_TEST_MCF_WIDE=0 the solve has to stop with SAGE2OV_ERR_LIMIT at round 0 where 64-bit prices do not carry the network; then, the variable unset, one
flow_solve with the round budget R (default: the library's).  When it finishes: price_words, the certificate in Python integers, total_cost against the
re-costed flows, and with --twice a second solve whose flows must be identical.  When the budget is spent: the phase and the round it stopped in.  Per epsilon
phase: rounds and HIP-event time.  The launches per price update are not in the statistics: run the script under a kernel trace and divide the calls of
k_mf_pu_relax by the price updates.  A diagnostic, not a test."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import fixtures as fx, flow_model as fm, flow_model_wide as fw, flowgen as fg, sage2_amd as s2

ap = argparse.ArgumentParser()
ap.add_argument("--widths", action="store_true"); ap.add_argument("--reads", type=int, default=0); ap.add_argument("--err-ppm", type=int, default=1000)
ap.add_argument("--max-rounds", type=int, default=0); ap.add_argument("--twice", action="store_true")
args = ap.parse_args()
OPTIMA = {"g4_highcopy_k21": 2227089582, "g13_noisy300_k55": 19999938, "shape_s3": json.load(open(os.path.join(fx.GOLDEN, "flow", "generated.json")))["shape_s3"]["optimum"]}
COUNTERS = ("phases", "rounds", "pushes", "relabels", "price_updates")


def report(name, st, wall, extra):
    ph = min(int(st.phases), s2.MCF_PHASES)
    print(json.dumps(dict(network=name, nodes=int(st.nodes), arcs=int(st.arcs), form=int(st.form), price_words=int(st.price_words), phases=int(st.phases), rounds=int(st.rounds),
                          pushes=int(st.pushes), relabels=int(st.relabels), price_updates=int(st.price_updates), total_cost=int(st.total_cost), build_ms=round(st.build_ms, 3),
                          solve_ms=round(st.solve_ms, 3), wall_ms=round(wall * 1e3, 3), refine_rounds=[int(x) for x in st.refine_rounds[:ph]],
                          refine_ms=[round(x, 3) for x in st.refine_ms[:ph]], **extra)), flush=True)


if args.widths or not args.reads:
    ctx = s2.Context(21, device=0)
    for name, opt in OPTIMA.items():
        if name in fg.GENERATED: n, a = fg.generated(name)
        else:
            n, fr, to, lo, up, co = fm.parse_input_cs2(os.path.join(fx.GOLDEN, name + ".input.cs2.gz"))
            a = np.zeros(len(fr), fg.ARC); a["from"], a["to"], a["lower"], a["upper"], a["cost"] = fr, to, lo, up, co
        out = {}
        for wide in (False, True):
            ctx.mcf_solve(n, a, wide=wide)                                              # warm-up
            ms = []
            for _ in range(3): flow, price, st = ctx.mcf_solve(n, a, args.max_rounds, wide=wide); ms.append(round(st.solve_ms, 2))
            out[wide] = (flow, [int(x) for x in price], [int(getattr(st, c)) for c in COUNTERS], ms)
        same = bool(np.array_equal(out[False][0], out[True][0]) and out[False][1] == out[True][1] and out[False][2] == out[True][2])
        cost = fw.certificate(n, *fg.split(a), out[True][0], out[True][1], n + 1)
        print(json.dumps(dict(network=name, nodes=n, arcs=len(a), rounds_64=out[False][2][1], rounds_128=out[True][2][1], solve_ms_64=out[False][3], solve_ms_128=out[True][3],
                              identical=same, certificate="ok", reached=bool(cost == opt))), flush=True)
        assert same and cost == opt
    ctx.close()
if args.reads:
    n, k, L = args.reads, 40, 150
    p = fx.synth_params(dict(seed=2, genome_len=3 * n, n_reads=n, read_len=L, err_ppm=args.err_ppm))
    t0 = time.perf_counter(); bases, off = s2.synth_reads_ascii(p, s2.synth_genome(p)); print(f"input: {n} reads in {time.perf_counter() - t0:.1f} s", flush=True)
    os.environ["SAGE2OV_TEST_MCF_WIDE"] = "0"
    g = s2.Context(k, device=0); g.reads_add_ascii(bases, off); g.reads_organize(); g.run_steps23(); g.graph_simplify(); g.genome_size(); g.flow_network_build()
    cs = g.copycount_stats(); nn = int(cs.network_nodes); print(f"network: {nn} nodes, {cs.network_arcs} arcs", flush=True)
    try:
        st = g.flow_solve(args.max_rounds); print(f"64-bit prices carry this network: solved in {st.rounds} rounds, {st.solve_ms:.1f} ms", flush=True)
    except s2.Sage2ovError as e:
        st = g.mcf_stats(); print(f"SAGE2OV_TEST_MCF_WIDE=0: code {e.code} at round {st.rounds}, price_words {st.price_words}: {e}", flush=True)
    del os.environ["SAGE2OV_TEST_MCF_WIDE"]; g.options_reload()
    t = time.perf_counter()
    try:
        st = g.flow_solve(args.max_rounds); wall = time.perf_counter() - t
        arcs = g.flow_network(); flow, price, scale = g.flow_solution_wide()
        cost = np.trunc(arcs["cost"].astype(np.float64)).astype(np.int64)
        c = fw.certificate(nn, arcs["from"], arcs["to"], arcs["lower"], arcs["upper"], cost, flow, price, scale)
        extra = dict(certificate="ok", reached=bool(c == st.total_cost), price_bits=max(abs(x) for x in price).bit_length())
        if args.twice: g.flow_solve(args.max_rounds); extra["second_solve_identical"] = bool(np.array_equal(flow, g.flow_solution_wide()[0]))
        report(f"{n} reads, {args.err_ppm} ppm", st, wall, extra)
    except s2.Sage2ovError as e:
        wall = time.perf_counter() - t; st = g.mcf_stats()
        report(f"{n} reads, {args.err_ppm} ppm", st, wall, dict(stopped=str(e), stopped_in_phase=int(st.phases), stopped_at_round=int(st.rounds)))
    g.close()
