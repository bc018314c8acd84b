"""The register and LDS allocation of the particle-filter kernel (libstb_amd/csrc/seat_pf.hip), read from the built
library's gfx950 code objects as tests/test_build_regs_partition.py does: MEASUREMENTS.md section F1 was measured with this
allocation."""
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


def test_filter_kernel_keeps_its_allocation():
    ks = {n: k for n, k in kernel_regs.kernels(capi.LIB_PATH).items() if n.startswith("k_seat_pf(")}
    assert len(ks) == 1, list(ks)
    k = next(iter(ks.values()))
    assert k["vgpr"] <= 256, k     # 172 when measured: eight waves a workgroup, two a SIMD, fit the launch bounds
    assert k["spill"] == 0 and k["scratch"] == 0, k
    assert k["lds"] == 3072, k     # T, N and the weights; the slots' pairs are dynamic, up to 61440 more
