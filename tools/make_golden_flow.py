#!/usr/bin/env python3
"""Records the optima of the generated and hand-made min-cost-flow networks of tests/flowgen.py into tests/golden/flow/generated.json, so that the GPU tests need
neither scipy nor any solver: name -> {nodes, arcs, optimum}.  The optimum is scipy's (linprog, method="highs") on the LP of the circulation; an LP whose optimum
is not an integer within 1e-6 is an error, since every such network has integer data."""
import json
import os
import sys

import numpy as np
from scipy.optimize import linprog
from scipy.sparse import coo_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import flowgen as fg      # noqa: E402


def lp_optimum(n, arcs):
    fr, to, lo, up, co = fg.split(arcs); m = len(fr)
    A = coo_matrix((np.concatenate([np.ones(m), -np.ones(m)]), (np.concatenate([to - 1, fr - 1]), np.concatenate([np.arange(m), np.arange(m)]))), shape=(n, m))
    r = linprog(co.astype(float), A_eq=A.tocsr(), b_eq=np.zeros(n), bounds=list(zip(lo.tolist(), up.tolist())), method="highs")
    if r.status != 0: raise SystemExit(f"linprog: {r.message}")
    v = round(r.fun)
    if abs(r.fun - v) > 1e-6 * max(1.0, abs(r.fun)): raise SystemExit(f"optimum {r.fun} is no integer")
    return int(v)


def main():
    out = {}
    for name in fg.GENERATED:
        n, arcs = fg.generated(name); out[name] = {"nodes": int(n), "arcs": int(len(arcs)), "optimum": lp_optimum(n, arcs)}
    for name in fg.HAND:
        n, arcs = fg.hand(name); out[name] = {"nodes": int(n), "arcs": int(len(arcs)), "optimum": lp_optimum(n, arcs)}
    path = os.path.join(ROOT, "tests", "golden", "flow", "generated.json")
    with open(path, "w") as f: json.dump(out, f, indent=1, sort_keys=True); f.write("\n")
    print(f"{len(out)} networks -> {path}")


if __name__ == "__main__":
    main()
