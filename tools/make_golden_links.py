#!/usr/bin/env python3
"""tests/golden/<name>.links.txt.gz: the rows the reference's ScaffoldMaker::mergeFinal and mergeFinalSmall (matePair/scaffolding.cpp:786-935, :981-1130) hand to
quicksortListOfLongEdges for the golden's committed P.graph4 with the flows and mates of tests/test_links_reference.py (golden_case) -- results the reference
computed, recorded for the machines that have no reference tree.  Needs the reference tree and the objects oracle/Makefile builds from it
(oracle/_ref/libsage2ref_driver.so); the driver is the text of tests/test_links_reference.py.

    python tools/make_golden_links.py [name ...]          (default: g4, g9)

One line per row: mode (1 mergeFinal, 2 mergeFinalSmall), then from, to, type, length of half a (the twin of edge_1) and of half b (edge_2), support, gap; sorted."""
import gzip
import os
import pathlib
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
NAMES = ["g4_highcopy_k21", "g9_repeats160k_k40"]


def main(names):
    import fixtures as fx
    import test_links_reference as LR
    if not (os.path.isdir(LR.REF) and os.path.exists(LR.REF_LIB)):
        sys.exit("the reference tree or oracle/_ref/libsage2ref_driver.so is absent")
    with tempfile.TemporaryDirectory(prefix="goldenlinks_") as tmp:
        src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        open(src, "w").write(LR.DRIVER_CPP)
        subprocess.run(["g++", "-fopenmp", "-std=c++0x", "-O1", "-w", "-include", os.path.join(ROOT, "oracle", "ref_prelude.h"), "-I", LR.REF, src, "-o", exe,
                        "-L", LR.REF_DIR, "-lsage2ref_driver", "-Wl,-rpath," + LR.REF_DIR, "-lz"], check=True)
        for name in names:
            m, ctx, g, text, pairs = LR.golden_case(name)
            d = pathlib.Path(tmp) / name; d.mkdir()
            out, rows = LR.reference_rows(exe, d, ctx, m["k"], text, pairs)
            assert "r 1 0" in out and "r 2 0" in out
            lines = sorted("%d %s %s %d %d" % (mode, " ".join(map(str, a)), " ".join(map(str, b)), s, gap) for mode, t in rows.items() for (a, b), (s, gap) in t.items())
            path = os.path.join(fx.GOLDEN, name + ".links.txt.gz")
            with open(path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as z:
                z.write(("\n".join(lines) + "\n").encode())
            print(f"{path}: {len(rows[1])} rows of mergeFinal, {len(rows[2])} of mergeFinalSmall, {os.path.getsize(path)} bytes")
            ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:] or NAMES)
