"""Per-stage HIP-event times of one path-support sweep and one round (sage2ov_path_supports, sage2ov_extend_paths_round) on a generated composite
graph with mates: python tests/diag/paths.py [pairs=20000] [seed=1].  One process, one line of JSON; run it several times for a spread.  Scratch tooling, no test."""
import json
import os
import pathlib
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import compgen as CG
import test_mate_estimate_host as H
from test_gpu_mate_estimate import add_mates, random_store, load_text


def main():
    pairs_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000; seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    N, header, recs = CG.composite_graph(seed, pairs_n, n_reads=10 * pairs_n, hubs=4, loops_once=2, loops_twice=2, dense_edges=0, flows=(1.0, 2.0, 1.0, 0.5))
    text = H.graph_text(header, recs)
    mates = CG.mates_for(H.parse_graph(text), seed + 1, libraries=2, k=CG.K)
    with tempfile.TemporaryDirectory() as d:
        ctx = random_store(N, 9); load_text(ctx, text, pathlib.Path(d)); add_mates(ctx, mates)
        ctx.mates_estimate()
        ctx.path_supports_build()
        n = ctx.extend_paths_round(2); st = ctx.path_stats(); xs = ctx.extend_stats().last
        out = {k: getattr(st, k) for k in ("claimed_reads", "claiming_nodes", "start_nodes", "paths", "capped_nodes", "eligible_entries", "voting_entries", "records", "rows",
                                           "key_collisions", "mirrored", "order_dependent", "claim_ms", "starts_ms", "walk_ms", "vote_ms", "sort_ms", "reduce_ms")}
        out.update(pairs=pairs_n, list_entries=sum(len(r["list"]) for r in recs), merges=n, select_ms=xs.select_ms, lists_ms=xs.lists_ms, commit_ms=xs.commit_ms)
        print(json.dumps(out)); ctx.close()


if __name__ == "__main__":
    main()
