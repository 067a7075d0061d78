#!/usr/bin/env python3
"""tests/golden/<name>.contig.fasta.gz: P_contig.fasta as the reference's OverlapGraph::printGraph writes it for the golden's committed P.graph4 -- data the
reference wrote.  Needs the reference tree and the objects oracle/Makefile builds from it (oracle/_ref/libsage2ref_driver.so); the driver below is our own text: it
includes the reference's headers, sets the globals main() would have set and calls the reference's own loader and printGraph with one thread.

    python tools/make_golden_contigs.py [name ...]          (default: g1, g5, g7, g10)

tests/test_contigs_reference.py uses the same driver to compare the reference with the tests' restatement."""
import gzip
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

REF = "/root/reference"
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
REF_LIB = os.path.join(REF_DIR, "libsage2ref_driver.so")
NAMES = ["g1_clean100_k21", "g5_mixedlen_k21", "g7_palindrome_tandem_k21", "g10_long900_k55"]

# loadReadsFromFile does not set averageReadLength, and the OverlapGraph constructor takes contigLengthThreshold from it (overlapGraph.cpp:52): it is set first.
# loadOverlapGraphFromFile overwrites genomeSize with the file's header (:382): it is set after the load.
DRIVER_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include "overlapGraph/overlapGraph.h"
extern ofstream logStream;
extern uint64_t genomeSize, averageReadLength;
int main(int argc, char** argv) {      // <k> <P.reads> <graph file> <log file> <output prefix> <averageReadLength> <genomeSize>
    if (argc < 8) return 2;
    omp_set_num_threads(1);
    logStream.open(argv[4]);
    averageReadLength = strtoull(argv[6], NULL, 10);
    ReadLoader* loader = new ReadLoader((uint16_t)atoi(argv[1]));
    loader->loadReadsFromFile(argv[2]);
    OverlapGraph* graph = new OverlapGraph(loader);
    graph->loadOverlapGraphFromFile(argv[3]);
    genomeSize = strtoull(argv[7], NULL, 10);
    graph->printGraph(argv[5], false);
    logStream.close();
    return 0;
}
"""


def available():
    return os.path.isdir(REF) and os.path.exists(REF_LIB)


def build_driver(workdir):
    src, exe = os.path.join(workdir, "contig_driver.cpp"), os.path.join(workdir, "contig_driver")
    open(src, "w").write(DRIVER_CPP)
    subprocess.run(["g++", "-fopenmp", "-std=c++0x", "-O1", "-w", "-include", os.path.join(ROOT, "oracle", "ref_prelude.h"), "-I", REF, src, "-o", exe,
                    "-L", REF_DIR, "-lsage2ref_driver", "-Wl,-rpath," + REF_DIR, "-lz"], check=True)
    return exe


def reference_contigs(driver, workdir, ctx, k, graph_text, genome_size):
    """-> (the text of P_contig.fasta, [longest, covered, N50, its ordinal, N90, its ordinal]) for the reads of `ctx` (any context with organised reads) and a graph file"""
    rp, gp, lp, op = (os.path.join(workdir, n) for n in ("P.reads", "P.graph", "P.log", "P_contig"))
    ctx.reads_save(rp)
    open(gp, "wb").write(graph_text if isinstance(graph_text, bytes) else graph_text.encode())
    arl = int((graph_text.decode() if isinstance(graph_text, bytes) else graph_text).split(None, 3)[2])      # the header's third value: what main() holds after a load
    subprocess.run([driver, str(k), rp, gp, lp, op, str(arl), str(genome_size)], check=True, timeout=600, env=dict(os.environ, OMP_NUM_THREADS="1"))
    log = open(lp).read()                                                             # the statistics are private members: taken from the log (overlapGraph.cpp:770-782)
    num = lambda label: [int(x) for x in re.search(label + r": (\d+)(?: BP \((\d+)\))?", log).groups() if x is not None]
    stats = num("Longest Contig") + num("Genome Covered")[:1] + num(r"N50") + num(r"N90")
    return open(op + ".fasta").read(), stats


def genome_len(manifest):
    return int(manifest["synth"].get("genome_len", 0))


def main(names):
    import fixtures as fx
    import sage2_amd as s2
    if not available():
        sys.exit("the reference tree or oracle/_ref/libsage2ref_driver.so is absent: run the build first")
    limit = max(os.path.getsize(os.path.join(fx.GOLDEN, f)) for f in os.listdir(fx.GOLDEN) if not f.endswith(".contig.fasta.gz"))
    with tempfile.TemporaryDirectory() as d:
        driver = build_driver(d)
        for name in names:
            m = fx.golden(name)
            ctx = s2.Context(m["k"], device=-2); ctx.reads_add_ascii(*fx.make_reads(m["synth"])); ctx.reads_organize()
            text = gzip.open(os.path.join(fx.GOLDEN, name + ".graph4.gz")).read()
            fasta, stats = reference_contigs(driver, d, ctx, m["k"], text, genome_len(m))
            ctx.close()
            out = os.path.join(fx.GOLDEN, name + ".contig.fasta.gz")
            with open(out, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as z:
                z.write(fasta.encode())
            size = os.path.getsize(out)
            print("%s: %d records, %d bytes of text, %d compressed, stats %s" % (name, fasta.count(">"), len(fasta), size, stats))
            if size > limit:
                os.remove(out); print("  larger than the largest fixture (%d): dropped" % limit)


if __name__ == "__main__":
    main(sys.argv[1:] or NAMES)
