#!/usr/bin/env python3
"""tests/copycount_ref.py -- TEST INFRASTRUCTURE: step 5 of the golden fixtures, made by the REFERENCE binary (oracle/_ref/SAGE2).

For a fixture of oracle/make_golden.py, reference_step5() runs the four commands the step-5 goldens stand for:
  1. the FASTA is regenerated as oracle/make_golden_step4.py does;
  2. `SAGE2 -f x.fa -k K -o out -p t -M 3 -s` writes out/t.reads (and t.graph3);
  3. the committed tests/golden/<name>.graph4.gz is put in as out/t.graph4;
  4. `SAGE2 -f x.fa -k K -o out -i t -p t5 -m 5 -M 5 -s` writes out/input.cs2, out/output.cs2, out/t5.graph5 and out/t5.log.
Run as a script (where oracle/_ref/SAGE2 is built) it stores tests/golden/<name>.input.cs2.gz, .output.cs2.gz, .graph5.gz (mtime 0) and step5/<name>.step5.json:
    python tests/copycount_ref.py [name ...]
tests/test_copycount_reference.py calls reference_step5() again and finds the committed files.
"""
import ctypes, gzip, hashlib, json, os, re, shutil, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REF = os.path.join(ROOT, "oracle", "_ref", "SAGE2")
# what is committed of each fixture: the three files in full, the two .cs2 files, or md5 + size only
FULL = ("g1_clean100_k21", "g6_k70_150", "g7_palindrome_tandem_k21", "g12_lowcomplexity_k21", "g4_highcopy_k21")
CS2_ONLY = ("g13_noisy300_k55",)
MD5_ONLY = ("g3_noisy_rep_k21",)


def _mg():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import make_golden as mg
    return mg


def md5_bytes(b):
    return hashlib.md5(b).hexdigest()


def parse_log(text):
    """the lines genomeSizeEstimation and computeMinCostFlow log"""
    est = [int(v) for v in re.findall(r"Genome Size: (\d+) \((?:Estimation \d+|Final estimation)\)", text)]
    final = "(Final estimation)" in text
    num = lambda label: int(re.search(re.escape(label) + r"\s*:\s*(\d+)", text).group(1))
    return dict(estimates=est, agreed=final,
                nodes=num("Number of nodes"), edges=num("Number of edges"), simple=num("Simple edges"), once=num("Edges used exactly once"),
                many=num("Edges used more than once"), t_to_s_flow=num("Flow from T to S"), flow_different=num("Flow different in edges"))


def reference_step5(name, tmp):
    """-> (input.cs2 bytes, output.cs2 bytes, graph5 bytes, parsed log)"""
    mg = _mg()
    k, threads, pd = mg.FIXTURES[name]
    fa = os.path.join(tmp, "x.fa")
    if "recipe" in pd:
        sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
        import fixtures
        fixtures.write_recipe_fasta(pd, fa)
    else:
        lib = ctypes.CDLL(os.path.join(ROOT, "sage2_amd", "libsage2ov.so"))
        lib.sage2ov_synth_write_fasta.argtypes = [ctypes.POINTER(mg.SynthParams), ctypes.c_char_p]
        p = mg.SynthParams(**pd)
        assert lib.sage2ov_synth_write_fasta(ctypes.byref(p), fa.encode()) == 0
    env = dict(os.environ, OMP_NUM_THREADS=str(threads), LC_ALL="C")
    out = os.path.join(tmp, "out")
    subprocess.run([REF, "-f", fa, "-k", str(k), "-o", out, "-p", "t", "-M", "3", "-s"], check=True, env=env, stdout=subprocess.DEVNULL)
    with gzip.open(os.path.join(GOLD, name + ".graph4.gz"), "rb") as fi, open(os.path.join(out, "t.graph4"), "wb") as fo:
        shutil.copyfileobj(fi, fo)
    subprocess.run([REF, "-f", fa, "-k", str(k), "-o", out, "-i", "t", "-p", "t5", "-m", "5", "-M", "5", "-s"], check=True, env=env, stdout=subprocess.DEVNULL)
    rd = lambda n: open(os.path.join(out, n), "rb").read()
    return rd("input.cs2"), rd("output.cs2"), rd("t5.graph5"), parse_log(rd("t5.log").decode())


def step5_meta(name, inp, outp, g5, log):
    meta = dict(log)
    meta.update(name=name, genome_size=log["estimates"][-1], p_min=inp.split(b"\n", 1)[0].decode(),
                input_cs2_md5=md5_bytes(inp), input_cs2_size=len(inp), output_cs2_md5=md5_bytes(outp), output_cs2_size=len(outp),
                graph5_md5=md5_bytes(g5), graph5_size=len(g5),
                command="SAGE2 -f x.fa -k K -o out -p t -M 3 -s; tests/golden/<name>.graph4.gz as out/t.graph4; SAGE2 -f x.fa -k K -o out -i t -p t5 -m 5 -M 5 -s (tests/copycount_ref.py)")
    return meta


def main():
    only = set(sys.argv[1:])
    for name in FULL + CS2_ONLY + MD5_ONLY:
        if only and name not in only: continue
        tmp = tempfile.mkdtemp(prefix="sage2gold5_")
        try:
            inp, outp, g5, log = reference_step5(name, tmp)
            keep = []
            if name in FULL: keep = [(".input.cs2.gz", inp), (".output.cs2.gz", outp), (".graph5.gz", g5)]
            if name in CS2_ONLY: keep = [(".input.cs2.gz", inp), (".output.cs2.gz", outp)]
            for suffix, data in keep:
                with gzip.GzipFile(os.path.join(GOLD, name + suffix), "wb", compresslevel=9, mtime=0) as fo:
                    fo.write(data)
            os.makedirs(os.path.join(GOLD, "step5"), exist_ok=True)
            json.dump(step5_meta(name, inp, outp, g5, log), open(os.path.join(GOLD, "step5", name + ".step5.json"), "w"), indent=1, sort_keys=True)
            print(name, log, len(inp), len(outp), len(g5), [os.path.getsize(os.path.join(GOLD, name + s)) for s, _ in keep])
        finally:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
