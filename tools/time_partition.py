"""Time the table-size partition draw (stb_sample_partition, libstb_amd/csrc/partition.hip) on the GPU, against a
single-core C restatement of the same draw on the host (tools/partition_host.c).

  python tools/time_partition.py [--calls 20] [--shapes A-realistic,A-wide,B] [--out FILE]

Shapes as tools/time_tcounts.py: A = 1000 restaurants x 1000 pairs, n_max 4000 ("realistic" / "wide"); B = 10^6
restaurants x 1 pair ("realistic").  Table M = N = max n, filled once.  Device time from events around each call (the
histogram's zeroing and the kernel, histogram only, after one warm-up call), median.  Candidates = sum over pairs and
rounds of N - M (what the rounds with more than one candidate read).  The host baseline draws a slice of the pairs on one
core and is scaled to the whole shape by candidates; its draws are checked against the device's on that slice.
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
    src = os.path.join(ROOT, "tools", "partition_host.c")
    out = os.path.join(ROOT, "tools", "build", "libpartition_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", out, src, "-lm"], check=True)
    L = C.CDLL(out)
    vp, d, u64 = C.c_void_p, C.c_double, C.c_uint64
    L.pt_host.restype = d
    L.pt_host.argtypes = [vp, vp, C.c_uint, d, u64, u64, vp, vp, vp, vp, vp, u64, u64]
    return L


def candidates(n, t):
    """sum over rounds of L = N - M for the draws' expected path is data-dependent; bound it by (t-1)(n-t+1)"""
    n, t = n.astype(np.int64), t.astype(np.int64)
    d = (t > 1) & (t < n)
    return int(((t[d] - 1) * (n[d] - t[d] + 1)).sum())


def run(name, calls, a=0.5, seed=2025):
    import torch

    I, K, prof = SHAPES[name]
    g = synth.groups(I, K, 4000, prof)
    N = M = int(g.n.max())
    S = N + 1
    tabs = capi.DeviceTables(N, M)
    tabs.fill(a)
    tabs.status()
    d_n = torch.as_tensor(g.n.view(np.int32), device="cuda")
    d_t = torch.as_tensor(g.t.view(np.int16), device="cuda")
    cnt = torch.empty(S, dtype=torch.int32, device="cuda")
    soff = np.concatenate([[0], np.cumsum(g.t.astype(np.int64))]).astype(np.uint64)

    def call(s, sizes=None, d_soff=None):
        capi.sample_partition(tabs, a, d_n, d_t, S, seed, s, sizes=sizes, soff=d_soff, cnt=cnt)

    # the slice the host repeats: the device's sizes of call 0
    d_soff = torch.as_tensor(soff.view(np.int64), device="cuda")
    d_sz = torch.empty(int(soff[-1]), dtype=torch.int16, device="cuda")
    call(0, d_sz, d_soff)
    torch.cuda.synchronize()
    dev_sizes = d_sz.cpu().numpy().view(np.uint16)
    ms = []
    for s in range(1, calls + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call(s)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    cand = candidates(g.n, g.t)
    med = float(np.median(ms))
    res = {"shape": name, "I": I, "K": K, "G": g.pairs, "N": N, "M": M, "a": a, "tables": int(g.t.astype(np.int64).sum()),
           "candidates_bound": cand, "ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)),
           "calls_timed": calls, "waves": int(os.environ.get("STB_PARTITION_WAVES", "4"))}
    H = host_lib()
    G0 = max(1, g.pairs // 100)
    S1 = tabs.S1[0].cpu().numpy().copy()
    tab = tabs.packed_host(0)
    hs = np.zeros(int(soff[G0]) + 1, dtype=np.uint16)
    hc = np.zeros(S, dtype=np.uint32)
    sec = H.pt_host(S1.ctypes.data, tab.ctypes.data, M, a, 0, G0, g.n.ctypes.data, g.t.ctypes.data, soff.ctypes.data,
                    hs.ctypes.data, hc.ctypes.data, seed, 0)
    same = sum(int(np.array_equal(hs[soff[k]:soff[k + 1]], dev_sizes[soff[k]:soff[k + 1]])) for k in range(G0))
    c_slice = candidates(g.n[:G0], g.t[:G0])
    res.update({"host_slice_pairs": G0, "host_slice_s": sec,
                "host_ms_scaled": sec * 1e3 * cand / max(1, c_slice), "host_same_draws_on_slice": same})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--shapes", default="A-realistic,A-wide,B")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert capi.lib().stb_device_count() > 0, "no GPU: " + capi.last_error()
    out = [run(s, args.calls) for s in args.shapes.split(",")]
    for r in out:
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
