"""The mate-pair table against the reference itself: MatePair::mapMatePairs (matePair.cpp:125-239) run by the reference's own objects under OMP_NUM_THREADS=1 (its
loop inserts into shared lists without a lock: with more threads its result is not defined), every matePairList[i] printed in list order, against
MatePair::list of sage2ov.hpp on the host route.  Runs only where the reference tree and the objects built from it (oracle/_ref/) are present.  The inputs are
upper case and every good read is in the store, so the one deliberate difference (a pair with a mate of id 0 is skipped here) plays no part.  The driver below
is our own text; it includes the reference's matePair/matePair.h and links oracle/_ref/libsage2ref_driver.so, which holds matePair.o and readLoader.o."""
import os
import subprocess

import pytest

import fixtures as fx
import sage2_amd as s2
import test_find_ids_host as H
import test_mates_host as M

REF = "/root/reference"
REF_DIR = os.path.join(fx.ROOT, "oracle", "_ref")
REF_LIB = os.path.join(REF_DIR, "libsage2ref_driver.so")
pytestmark = pytest.mark.skipif(not (os.path.isdir(REF) and os.path.exists(REF_LIB)), reason="the reference tree or oracle/_ref/libsage2ref_driver.so is absent")

DRIVER_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include "matePair/matePair.h"
extern ofstream logStream;
int main(int argc, char** argv) {      // <k> <P.reads> <mates.fa>: every matePairList[i] in list order
    omp_set_num_threads(1);
    logStream.open("/dev/null");
    ReadLoader* loader = new ReadLoader((uint16_t)atoi(argv[1]));
    loader->loadReadsFromFile(argv[2]);
    MatePair* mates = new MatePair(NULL, loader);
    mates->mapMatePairs(argv[3], "", 1);
    for (uint64_t i = 0; i <= loader->numberOfUniqueReads; i++)
        for (MatePairInfo* w = mates->matePairList[i]; w != NULL; w = w->next)
            printf("%llu %llu %d %d %d %d\n", (unsigned long long)i, (unsigned long long)w->ID, (int)w->type1, (int)w->type2, (int)w->freq, (int)w->library);
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("refmates")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(DRIVER_CPP)
    subprocess.run(["g++", "-fopenmp", "-std=c++0x", "-O1", "-w", "-include", os.path.join(fx.ROOT, "oracle", "ref_prelude.h"), "-I", REF, src, "-o", exe,
                    "-L", REF_DIR, "-lsage2ref_driver", "-Wl,-rpath," + REF_DIR, "-lz"], check=True)
    return exe


def ours_and_theirs(driver, tmp_path, ctx, mates, k):
    prefix, mf = str(tmp_path / "P.reads"), str(tmp_path / "mates.fa")
    ctx.reads_save(prefix); M.write_fasta(mf, mates)
    env = dict(os.environ, OMP_NUM_THREADS="1")
    theirs = subprocess.run([driver, str(k), prefix, mf], check=True, stdout=subprocess.PIPE, text=True, timeout=120, env=env).stdout.splitlines()
    ctx.mates_add_file(mf, library=1)
    ent, offs = ctx.mates(1)
    ours = []
    for a in range(ctx.reads_stats().unique_reads + 1):
        seg = ent[int(offs[a]):int(offs[a + 1])]
        for e in sorted(seg, key=lambda e: -int(e["first"])):            # MatePair::list: descending first
            ours.append("%d %d %d %d %d %d" % (a, e["to"], e["type1"], e["type2"], e["freq"], e["library"]))
    return ours, theirs


def test_ordinary_pairs_like_the_reference(driver, tmp_path):
    k = 21
    ctx, reads = M.tiling_store(H.HOST, 3000, 100, k, 6100, dup_every=7, dup_copies=2)
    ours, theirs = ours_and_theirs(driver, tmp_path, ctx, M.ordinary_pairs(reads), k)
    assert ours == theirs and len(ours) > 7000
    ctx.close()


def test_self_pairs_and_freq_wrap_like_the_reference(driver, tmp_path):
    k = 21
    ctx, reads = M.tiling_store(H.HOST, 60, 100, k, 6300)
    mates = []
    for r in reads[:20]:
        mates += [r, r]
    for r in reads[20:40]:
        mates += [r, fx.revcomp(r)]
    mates += [reads[40], reads[41]] * 256 + [reads[42], fx.revcomp(reads[43])] * 600
    ours, theirs = ours_and_theirs(driver, tmp_path, ctx, mates, k)
    assert ours == theirs and len(ours) == 20 + 40 + 4
    assert sorted(int(x.split()[4]) for x in ours)[:2] == [0, 0]        # 256 records: the uint8 wrapped to 0, there as here
    ctx.close()
