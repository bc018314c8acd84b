"""Time the table-count sweep (stb_sample_tcounts, libstb_amd/csrc/tcounts.hip) on the GPU, against a single-core C
restatement of the same sweep on the host (tools/tcounts_host.c).

  python tools/time_tcounts.py [--sweeps 20] [--shapes A-realistic,A-wide,B] [--out FILE]

Shapes from synth.groups: A = 1000 restaurants x 1000 pairs, n_max 4000 ("realistic" / "wide"); B = 10^6 restaurants
x 1 pair ("realistic").  Table M = N = max n, filled once.  Device time from events around each sweep (after one warm-up
sweep), median.  Weights = sum over pairs of min(n, M); the bounds quoted are 8 B of table read per weight at HBM peak and
one log + one exp per weight.  The host baseline sweeps a slice of the restaurants once on one core (glibc log / exp,
h = 1) and is scaled to the whole shape; its draws are checked against the device's on that slice.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libstb_amd import capi, synth  # noqa: E402

SHAPES = {"A-realistic": (1000, 1000, "realistic"), "A-wide": (1000, 1000, "wide"), "B": (1000000, 1, "realistic")}


def host_lib():
    src = os.path.join(ROOT, "tools", "tcounts_host.c")
    out = os.path.join(ROOT, "tools", "build", "libtcounts_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", out, src, "-lm"], check=True)
    L = C.CDLL(out)
    vp, d, u64 = C.c_void_p, C.c_double, C.c_uint64
    L.tc_host_sweep.restype = d
    L.tc_host_sweep.argtypes = [vp, vp, C.c_uint, d, vp, C.c_int, C.c_int, vp, vp, vp, vp, u64, u64]
    return L


def run(name, sweeps, a=0.5, seed=2025):
    import torch

    I, K, prof = SHAPES[name]
    g = synth.groups(I, K, 4000, prof)
    N = M = int(g.n.max())
    L = capi.lib()
    tabs = capi.DeviceTables(N, M)
    tabs.fill(a)
    tabs.status()
    koff_h = np.concatenate([[0], np.cumsum(g.K)]).astype(np.uint64)
    koff = torch.as_tensor(koff_h.view(np.int64), device="cuda")
    d_n = torch.as_tensor(g.n.view(np.int32), device="cuda")
    d_t = torch.as_tensor(g.t.view(np.int16), device="cuda").clone()
    d_T = torch.as_tensor(g.T.view(np.int32), device="cuda").clone()
    d_b = torch.as_tensor(g.bpar, device="cuda")

    def sweep(s):
        capi.check(L.stb_sample_tcounts(tabs.tables.data_ptr(), tabs.S1.data_ptr(), N, M, a, d_b.data_ptr(), I,
                                        koff.data_ptr(), d_n.data_ptr(), d_t.data_ptr(), d_T.data_ptr(), None, seed, s,
                                        capi.stream_ptr()))

    # the host baseline's slice starts from the state the device's first sweep starts from
    nslice = max(1, I // 50)
    G0 = int(koff_h[nslice])
    t_host, T_host = g.t.copy(), g.T.copy()
    sweep(0)
    torch.cuda.synchronize()
    t_dev0 = d_t.cpu().numpy().view(np.uint16)[:G0].copy()
    ms = []
    for s in range(1, sweeps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sweep(s)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    weights = int(np.minimum(g.n.astype(np.int64), M).sum())
    med = float(np.median(ms))
    res = {"shape": name, "I": I, "K": K, "G": g.pairs, "N": N, "M": M, "a": a, "weights": weights,
           "ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)), "sweeps_timed": sweeps,
           "weights_per_s": weights / (med * 1e-3), "bound_table_8B_ms": weights * 8 / 8.0e12 * 1e3,
           "threads": int(os.environ.get("STB_TCOUNTS_THREADS", "256"))}
    # host: one core, the same sweep over the first restaurants, from the same state; scaled by the weights
    H = host_lib()
    S1 = tabs.S1[0].cpu().numpy().copy()
    tab = tabs.packed_host(0)
    sec = H.tc_host_sweep(S1.ctypes.data, tab.ctypes.data, M, a, g.bpar.ctypes.data, 0, nslice, koff_h.ctypes.data,
                          g.n.ctypes.data, t_host.ctypes.data, T_host.ctypes.data, seed, 0)
    w_slice = int(np.minimum(g.n[:G0].astype(np.int64), M).sum())
    res.update({"host_slice_restaurants": nslice, "host_slice_s": sec, "host_ms_scaled": sec * 1e3 * weights / w_slice,
                "host_same_draws_on_slice": int(np.sum(t_host[:G0] == t_dev0)), "host_slice_pairs": G0})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--shapes", default="A-realistic,A-wide,B")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert capi.lib().stb_device_count() > 0, "no GPU: " + capi.last_error()
    out = [run(s, args.sweeps) for s in args.shapes.split(",")]
    for r in out:
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
