"""The register allocation of the held-out kernels under Gaussian observations (libstb_amd/csrc/gauss_heldout.hip, and
k_gh_sum of predict.hip), read from the built library's gfx950 code objects as tests/test_build_regs_gauss.py does: each
kernel once, no scratch, no spills."""
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

# launch bounds of 512: eight waves a workgroup, two a SIMD, 256 registers each at the most.  The point kernels hide the
# latency of their loads behind one another's waves and get half of that, so that two workgroups fit a compute unit; the
# sum is k_heldout_sum's body and gets what that has
KERNELS = {"k_gh_point_reg": 128, "k_gh_point": 128, "k_gh_reset": 128, "k_gh_sum": 128}


@pytest.mark.parametrize("name", list(KERNELS))
def test_heldout_kernels_use_no_scratch(name):
    ks = {n: k for n, k in kernel_regs.kernels(capi.LIB_PATH).items() if n.startswith(name + "(")}
    assert len(ks) == 1, list(ks)
    k = next(iter(ks.values()))
    assert k["spill"] == 0 and k["scratch"] == 0, k
    assert k["vgpr"] + k.get("agpr", 0) <= KERNELS[name], k


def test_the_shared_body_leaves_k_heldout_sum_its_lds():
    """one copy of the sum's LDS a kernel, whichever forms of the body it holds"""
    ks = kernel_regs.kernels(capi.LIB_PATH)
    a = next(k for n, k in ks.items() if n.startswith("k_heldout_sum("))
    b = next(k for n, k in ks.items() if n.startswith("k_gh_sum("))
    assert a["lds"] == b["lds"], (a, b)
