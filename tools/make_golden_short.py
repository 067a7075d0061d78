#!/usr/bin/env python3
"""tools/make_golden_short.py -- records what the reference does on the cases of tests/test_short_reference.py:GOLDEN_CASES, for the GPU tests (the reference does
not exist where they run): its own ContigExtender::mergeShortOverlap handed the rows of include/sage2ov.h (SHORT OVERLAPS) round after round until one joins
nothing, the joins per round (count, and from / to / support / gap of each), the graph it saves after every round (flag column of the list entries set to 0: the
reference leaves it uninitialised in the entries a join inserts) and the P_contig.fasta its printGraph(.., false) writes at the end.  Data only, gzip text, into
tests/golden/short/<case>.json.gz.  Needs the reference tree and oracle/_ref/ (oracle/Makefile).

The cases are the hand-built link graph with the components of tests/test_short_host.py, chosen so that (tests/test_short_reference.py checks all three on the CPU)
every recorded round has outside_reference == 0 and ties == 0 in the model, every case joins, and across the cases there is a blocked row, a row removed by
gapSum > 0 alone ("plus") and a join GAPPED with a gap of 0 ("minus", "zero").  The model's figures per recorded round, as (joins, rows, blocked, outside_reference, ties):
  short_cycle  high 1, the cycle's flows, components minus, zero, plus:     (2, 14, 12, 0, 0), (0, 12, 12, 0, 0)
  short_high1  high 1, every hand-graph flow 50, all seven components:      (2, 17, 15, 0, 0), (0, 15, 15, 0, 0)
  short_high2  high 2, every hand-graph flow 50, all seven components:      (3, 17, 2, 0, 0), (1, 12, 2, 0, 0), (0, 4, 2, 0, 0)"""
import gzip, json, os, sys, tempfile, pathlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_short_reference as R
import test_mate_estimate_host as H
import test_short_host as TH
from test_extend_reference import hand_store

out_dir = os.path.join(ROOT, "tests", "golden", "short"); os.makedirs(out_dir, exist_ok=True)
with tempfile.TemporaryDirectory() as d:
    driver = R.build_driver(d)
    for name in sorted(R.GOLDEN_CASES):
        N, header, recs, pairs, high = R.golden_case(name)
        work = pathlib.Path(d) / name; work.mkdir()
        ctx = hand_store(N)
        compared, joined, rs, op, g = R.ordered(driver, work, ctx, TH.K, H.graph_text(header, recs), pairs, high, fasta=True)
        assert joined >= 1 and not rs[-1]["merges"]
        rec = dict(case=name, high=high, joins=[len(r["merges"]) for r in rs],
                   merges=[[(m["frm"], m["to"], m["support"], m["gap"]) for m in r["merges"]] for r in rs],      # (the rows the reference was handed and joined: its count and graph confirm them)
                   graphs=[R.unflagged(open("%s.%d" % (op, rd)).read()) for rd in range(1, compared + 1)], fasta=open(op + "_contig.fasta").read())
        with gzip.GzipFile(os.path.join(out_dir, name + ".json.gz"), "wb", mtime=0) as f:
            f.write(json.dumps(rec, indent=0).encode())
        print(name, "high", high, [(len(r["merges"]), r["rows"], r["blocked"], int(r["outside_reference"]), int(r["ties"])) for r in rs], len(rec["fasta"]), "bytes of fasta")
        ctx.close()
