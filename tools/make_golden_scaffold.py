#!/usr/bin/env python3
"""tools/make_golden_scaffold.py -- records what the reference does on the cases of tests/test_scaffold_reference.py:GOLDEN_CASES, for the GPU tests (the reference
does not exist where they run): its own mergeAccordingToSupport / mergeAccordingToSupport2 handed the rows of include/sage2ov.h's rules (a) and (b) round after
round, the joins per round (count, and from / to / support / gap of each), the graph it saves after every round (flag column of the list entries set to 0: the reference leaves it uninitialised in the
entries a join inserts) and the P_scaffold.fasta its printGraph(.., true) writes at the end.  Data only, gzip text, into tests/golden/scaffold/<case>.json.gz.
Needs the reference tree and oracle/_ref/ (oracle/Makefile)."""
import gzip, json, os, sys, tempfile, pathlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_scaffold_reference as R
import test_mate_estimate_host as H
import test_links_host as LH
from test_extend_reference import hand_store

out_dir = os.path.join(ROOT, "tests", "golden", "scaffold"); os.makedirs(out_dir, exist_ok=True)
with tempfile.TemporaryDirectory() as d:
    driver = R.build_driver(d)
    for name in sorted(R.GOLDEN_CASES):
        N, header, recs, pairs, high, flag, small = R.golden_case(name)
        work = pathlib.Path(d) / name; work.mkdir()
        ctx = hand_store(N)
        compared, joined, rs, op, g = R.ordered(driver, work, ctx, LH.HAND_K, H.graph_text(header, recs), pairs, high, flag, small, fasta=True)
        rec = dict(case=name, high=high, flag=flag, small=small, joins=[len(r["merges"]) for r in rs],
                   merges=[[(m["frm"], m["to"], m["support"], m["gap"]) for m in r["merges"]] for r in rs],      # (the rows the reference was handed and joined: its count and graph confirm them)
                   graphs=[R.unflagged(open("%s.%d" % (op, rd)).read()) for rd in range(1, compared + 1)], fasta=open(op + "_scaffold.fasta").read())
        with gzip.open(os.path.join(out_dir, name + ".json.gz"), "wt") as f:
            json.dump(rec, f, indent=0)
        print(name, rec["joins"], len(rec["fasta"]), "bytes of fasta")
        ctx.close()
