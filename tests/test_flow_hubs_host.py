"""CPU: the binding of the hub form's statistics (sage2ov_mcf_hub_stats_get, Context.mcf_hub_stats, MCF_HUB_DEG) as far as it goes without a GPU.
tests/test_gpu_flow_hubs.py holds the form itself against the model."""
import ctypes as C
import os, subprocess

import pytest

import fixtures as fx
import sage2_amd as s2


def test_symbol_constant_and_device_less_context(tmp_path):
    L = s2.lib()
    assert hasattr(L, "sage2ov_mcf_hub_stats_get")
    src, exe = str(tmp_path / "hd.c"), str(tmp_path / "hd")
    open(src, "w").write('#include <stdio.h>\n#include "sage2ov.h"\nint main(void) { int (*f)(const sage2ov_ctx*, uint64_t*) = sage2ov_mcf_hub_stats_get; (void)f;\n'
                         'printf("%llu", (unsigned long long)SAGE2OV_MCF_HUB_DEG); return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(fx.ROOT, "include"), "-c", src, "-o", exe + ".o"], check=True)
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(fx.ROOT, "include"), "-E", "-dM", src, "-o", exe + ".defs"], check=True)
    defs = dict(l.split()[1:3] for l in open(exe + ".defs") if l.startswith("#define SAGE2OV_MCF_HUB_DEG "))
    assert int(defs["SAGE2OV_MCF_HUB_DEG"]) == s2.MCF_HUB_DEG and s2.MCF_HUB_DEG >= 64
    ctx = s2.Context(21, device=-2)
    with pytest.raises(s2.Sage2ovError) as e: ctx.mcf_hub_stats()
    assert e.value.code == -3
    out = (C.c_uint64 * 6)()
    assert L.sage2ov_mcf_hub_stats_get(None, out) == -1 and L.sage2ov_mcf_hub_stats_get(ctx._h, None) == -1 and L.sage2ov_mcf_hub_stats_get(ctx._h, out) == -3
    ctx.close()
