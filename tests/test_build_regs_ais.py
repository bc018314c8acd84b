"""The register allocation of the three kernels of annealed importance sampling (libstb_amd/csrc/seat_ais.hip), read from
the built library's gfx950 code objects as tests/test_build_regs_pf.py does: no scratch, no spills, no LDS; the counts
MEASUREMENTS.md section A1 was written with."""
import importlib.util
import os
import shutil

import pytest

from libstb_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(ROOT, "tools", "kernel_regs.py"))
kernel_regs = importlib.util.module_from_spec(spec)
spec.loader.exec_module(kernel_regs)

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(kernel_regs.LLVM, "llvm-readelf")) or shutil.which("c++filt") is None,
                                reason="llvm-readelf / c++filt not on this machine")

# (vgpr, sgpr) when section A1 was written; the bounds leave the compiler room, the zeros do not
RECORDED = {"k_ais_expand(": (42, 75), "k_ais_temper(": (19, 18), "k_ais_weight(": (58, 72)}


def test_the_three_kernels_have_no_scratch_and_no_spills():
    all_k = kernel_regs.kernels(capi.LIB_PATH)
    for prefix, (vgpr, sgpr) in RECORDED.items():
        ks = [k for n, k in all_k.items() if n.startswith(prefix)]
        assert len(ks) == 1, (prefix, [n for n in all_k if n.startswith("k_ais")])
        k = ks[0]
        print(prefix, "vgpr", k["vgpr"], "sgpr", k["sgpr"], "recorded", vgpr, sgpr)
        assert k["spill"] == 0 and k["scratch"] == 0 and k["lds"] == 0, (prefix, k)
        assert k["vgpr"] <= 128, (prefix, k)      # eight waves of 64 lanes a workgroup stay four to a SIMD
