"""The register allocation of the Gaussian-observation kernels (libstb_amd/csrc/gauss.hip), read from the built library's
gfx950 code objects as tests/test_build_regs_classgen.py does: each kernel once, no scratch, no spills."""
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

# launch bounds of 512: eight waves a workgroup, two a SIMD, 256 registers each at the most.  Every kernel whose waves hide
# memory latency behind one another gets half of that, so that two workgroups (at 256 threads: four) fit a compute unit;
# k_gs_logml, one small launch of two lgammas a cell, the whole 256
KERNELS = {"k_gs_sum_a": 128, "k_gs_sum_b": 128, "k_gs_fin_a": 128, "k_gs_fin_b": 128, "k_gs_draw": 128, "k_gs_prep": 128,
           "k_gs_lik_reg": 128, "k_gs_lik": 128, "k_gs_loglik": 128, "k_gs_logml": 256, "k_gs_init": 128}


@pytest.mark.parametrize("name", list(KERNELS))
def test_gauss_kernels_use_no_scratch(name):
    ks = {n: k for n, k in kernel_regs.kernels(capi.LIB_PATH).items() if n.startswith(name + "(")}
    assert len(ks) == 1, list(ks)
    k = next(iter(ks.values()))
    assert k["spill"] == 0 and k["scratch"] == 0, k
    assert k["vgpr"] + k.get("agpr", 0) <= KERNELS[name], k
