"""tests/diag/flow_hubs.py [--small [--ab OTHER_LIB --runs K]] [--reads N --err-ppm E --max-rounds R [--hub-deg d1,d2,..] [--then-rounds R2]] -- what the hub form of
step 5's solver (k_mf_hub_*) costs and gains, beside a library without it.  The library is the one SAGE2OV_LIB names (default: this tree's); a
library without sage2ov_mcf_hub_stats_get (the parent commit's) reports hub: null and ignores SAGE2OV_TEST_MCF_HUB_DEG.
--small: g4_highcopy_k21, g13_noisy300_k55 and the generated 1 602-node network through mcf_solve, five solves each after a warm-up: counters, the HIP-event time of
the rounds (median and range), optimum and certificate.  None of them has a hub at the default threshold: the time is what the extra kernel argument costs.
With --ab OTHER_LIB the script runs itself in fresh child processes, OTHER_LIB and this library alternately, K times each, and prints the rows side by side; rounds,
pushes and relabels must be equal.
--reads N: a noisy synthetic workload (N x 150 bp, k = 40, as tests/diag/flow_solve_wide.py builds it) through steps 1-4 and the network, then one flow_solve per
threshold of --hub-deg (default: the library's own; 0 is the hub form off) with the round budget R.  The first finished solve is held against the certificate in
Python integers; the later ones must give the same flows and prices.  Per solve: counters, hub statistics, seconds per round, and per epsilon phase rounds and time.
--then-rounds R2: after the last threshold one more solve with the budget R2 (how far a longer budget gets).  A diagnostic, not a test."""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--small", action="store_true"); ap.add_argument("--ab", default=""); ap.add_argument("--runs", type=int, default=2)
ap.add_argument("--reads", type=int, default=0); ap.add_argument("--err-ppm", type=int, default=1000); ap.add_argument("--max-rounds", type=int, default=0)
ap.add_argument("--hub-deg", default=""); ap.add_argument("--then-rounds", type=int, default=0)
args = ap.parse_args()
HUB = "SAGE2OV_TEST_MCF_HUB_DEG"
COUNTERS = ("phases", "rounds", "pushes", "relabels", "price_updates")

if args.ab:                                                                            # children, one after the other: never two processes on the device
    rows = {}
    for run in range(args.runs):
        for tag, lib in (("other", args.ab), ("this", os.environ.get("SAGE2OV_LIB", ""))):
            env = dict(os.environ); env.pop("SAGE2OV_LIB", None)
            if lib: env["SAGE2OV_LIB"] = os.path.abspath(lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--small"], env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=300).stdout
            for line in out.splitlines():
                if line.startswith("{"): r = json.loads(line); rows.setdefault(r["network"], []).append((tag, run + 1, r))
    for name, got in rows.items():
        same = len({tuple(r["counters"]) for _, _, r in got}) == 1
        print(json.dumps(dict(network=name, counters=got[0][2]["counters"], counters_equal=same,
                              solve_ms={f"{tag} run {run}": [r["min_ms"], r["median_ms"], r["max_ms"]] for tag, run, r in got})), flush=True)
        assert same
    sys.exit(0)

import numpy as np
import fixtures as fx, flow_model as fm, flow_model_wide as fw, flowgen as fg, sage2_amd as s2


def hub_stats(ctx):
    try: return ctx.mcf_hub_stats()
    except AttributeError: return None                                                 # a library from before the hub form


if args.small or not args.reads:
    OPTIMA = {"g4_highcopy_k21": 2227089582, "g13_noisy300_k55": 19999938, "shape_s3": json.load(open(os.path.join(fx.GOLDEN, "flow", "generated.json")))["shape_s3"]["optimum"]}
    ctx = s2.Context(21, device=0)
    for name, opt in OPTIMA.items():
        if name in fg.GENERATED: n, a = fg.generated(name)
        else:
            n, fr, to, lo, up, co = fm.parse_input_cs2(os.path.join(fx.GOLDEN, name + ".input.cs2.gz"))
            a = np.zeros(len(fr), fg.ARC); a["from"], a["to"], a["lower"], a["upper"], a["cost"] = fr, to, lo, up, co
        ctx.mcf_solve(n, a)                                                            # warm-up
        ms = []
        for _ in range(5): flow, price, st = ctx.mcf_solve(n, a); ms.append(st.solve_ms)
        cost = fm.certificate(n, *fg.split(a), flow, price, st.scale)
        deg = np.bincount(np.concatenate([a["from"], a["to"]]).astype(np.int64), minlength=n + 1)
        print(json.dumps(dict(network=name, nodes=n, arcs=len(a), longest_list=int(deg.max()), counters=[int(getattr(st, c)) for c in COUNTERS], hub=hub_stats(ctx),
                              min_ms=round(min(ms), 2), median_ms=round(statistics.median(ms), 2), max_ms=round(max(ms), 2), certificate="ok", reached=bool(cost == opt))), flush=True)
        assert cost == opt
    ctx.close()

if args.reads:
    n, k, L = args.reads, 40, 150
    p = fx.synth_params(dict(seed=2, genome_len=3 * n, n_reads=n, read_len=L, err_ppm=args.err_ppm))
    t0 = time.perf_counter(); bases, off = s2.synth_reads_ascii(p, s2.synth_genome(p)); print(f"input: {n} reads in {time.perf_counter() - t0:.1f} s", flush=True)
    t0 = time.perf_counter()
    g = s2.Context(k, device=0); g.reads_add_ascii(bases, off); g.reads_organize(); g.run_steps23(); g.graph_simplify(); g.genome_size(); g.flow_network_build()
    del bases, off
    cs = g.copycount_stats(); nn = int(cs.network_nodes); print(f"network: {nn} nodes, {cs.network_arcs} arcs after {time.perf_counter() - t0:.1f} s", flush=True)
    arcs = g.flow_network()
    deg = np.bincount(np.concatenate([arcs["from"], arcs["to"]]).astype(np.int64), minlength=nn + 1); top = np.sort(deg)[::-1][:4]
    print(f"longest lists: {[int(x) for x in top]}", flush=True)
    first = None

    def one(setting, budget):
        global first
        if setting is None: os.environ.pop(HUB, None)
        else: os.environ[HUB] = setting
        g.options_reload()
        t = time.perf_counter(); extra = {}
        try:
            st = g.flow_solve(budget)
            flow, price, scale = g.flow_solution_wide()
            if first is None:
                cost = np.trunc(arcs["cost"].astype(np.float64)).astype(np.int64)
                c = fw.certificate(nn, arcs["from"], arcs["to"], arcs["lower"], arcs["upper"], cost, flow, price, scale)
                first = (flow, price); extra = dict(finished=True, certificate="ok", reached=bool(c == st.total_cost))
            else: extra = dict(finished=True, same_flows_and_prices_as_first=bool(np.array_equal(flow, first[0]) and price == first[1]))
        except s2.Sage2ovError as e:
            st = g.mcf_stats(); extra = dict(finished=False, stopped=str(e), stopped_in_phase=int(st.phases))
        wall = time.perf_counter() - t; ph = min(int(st.phases), s2.MCF_PHASES); rounds = max(1, int(st.rounds))
        print(json.dumps(dict(network=f"{n} reads, {args.err_ppm} ppm", hub_deg_setting=setting, budget=budget, price_words=int(st.price_words),
                              counters=[int(getattr(st, c)) for c in COUNTERS], hub=hub_stats(g), total_cost=int(st.total_cost), build_ms=round(st.build_ms, 2),
                              solve_ms=round(st.solve_ms, 1), ms_per_round=round(st.solve_ms / rounds, 4), wall_s=round(wall, 2), refine_rounds=[int(x) for x in st.refine_rounds[:ph]],
                              refine_ms=[round(x, 1) for x in st.refine_ms[:ph]], **extra)), flush=True)

    settings = [s for s in args.hub_deg.split(",") if s] or [None]
    for s in settings: one(s, args.max_rounds)
    if args.then_rounds: one(settings[-1], args.then_rounds)
    g.close()
