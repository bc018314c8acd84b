"""The register allocation of the class draw's kernels (libstb_amd/csrc/classgen.hip), read from the built library's
gfx950 code objects as tests/test_build_regs_pf.py does: no scratch, no spills."""
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


@pytest.mark.parametrize("name", ["k_cls_pre", "k_cls_base", "k_cls_draw"])
def test_class_draw_kernels_use_no_scratch(name):
    ks = {n: k for n, k in kernel_regs.kernels(capi.LIB_PATH).items() if n.startswith(name + "(")}
    assert len(ks) == 1, list(ks)
    k = next(iter(ks.values()))
    assert k["spill"] == 0 and k["scratch"] == 0, k
    assert k["vgpr"] <= 128, k     # launch bounds of 512: eight waves a workgroup, two a SIMD, and room for two workgroups
