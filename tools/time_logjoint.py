"""Time the log joint of a sampler state on the device (stb_tcounts_logjoint, libstb_amd/csrc/logjoint.hip) against the
two routes a caller had before it, on the same machine and the same state:

  get+host    stb_tcounts_get (all of t and T read back) + the sum on one host core (tools/logjoint_host.c, the table a
              host copy of the device's slab made once, outside the timing)
  groups      stb_tcounts_to_groups + stb_groups_ssum + stb_tcounts_get of T alone + stb_joint_terms: W(a) + R(a, b),
              one shared b, no base-measure weights

  python tools/time_logjoint.py [--reps 20] [--restaurants 1000,100000] [--out FILE]

Shapes: I restaurants x 200 customers, spread over 20 dishes (multinomial), t = 1 + floor(u sqrt(n)); a = 0.5, b = 10.
Every figure is the wall-clock time of the whole call sequence as the caller sees it (launches, waits and copies
included), median of --reps after one warm-up.  The kernel's own duration comes from a profiler run of this tool
(rocprofv3 --kernel-trace --stats -- python tools/time_logjoint.py --reps 5): k_logjoint's row."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libstb_amd import capi  # noqa: E402

c_u16_p, c_u32_p = C.POINTER(C.c_uint16), C.POINTER(C.c_uint32)


def host_lib():
    src = os.path.join(ROOT, "tools", "logjoint_host.c")
    out = os.path.join(ROOT, "tools", "build", "liblogjoint_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", out, src, "-lm"], check=True)
    L = C.CDLL(out)
    vp = C.c_void_p
    L.lj_host_sum.restype = C.c_double
    L.lj_host_sum.argtypes = [vp, vp, C.c_uint, C.c_uint, C.c_double, vp, C.c_int, vp, vp, vp, vp, C.POINTER(C.c_double)]
    return L


def state(I, customers=200, dishes=20, seed=9):
    rng = np.random.default_rng(seed)
    n = rng.multinomial(customers, np.full(dishes, 1.0 / dishes), size=I).astype(np.uint32).reshape(-1)
    t = np.where(n > 0, np.minimum(1 + np.floor(rng.random(n.shape[0]) * np.sqrt(n)), n), 0).astype(np.uint16)
    return np.full(I, dishes, dtype=np.int32), n, t


def median_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(min(out))


def run(I, reps, a=0.5, b=10.0):
    import torch

    L = capi.lib()
    K, n, t = state(I)
    G = int(n.shape[0])
    bpar = np.full(I, b)
    koff = np.concatenate([[0], np.cumsum(K)]).astype(np.uint64)
    tc = capi.TableCounts(K, n, t)
    g = L.stb_groups_create(I, K.ctypes.data_as(C.POINTER(C.c_int)), None, None, None, None, 0, 0, 2)
    assert g, capi.last_error()
    res = {"I": I, "G": G, "customers": 200, "a": a, "b": b, "reps": reps}
    try:
        tc.sweep(a, bpar, 1, 0, 2)
        # ---- the device call
        box = {}

        def dev_call():
            box["dev"] = tc.logjoint(a, bpar, want_Li=False)

        res["device_ms"], res["device_ms_min"] = median_ms(dev_call, reps)
        tot, _, info = box["dev"]
        res["total"] = tot
        assert info.outside == 0 and info.impossible == 0 and info.t_mismatch == 0
        # ---- stb_tcounts_get + one host core
        H = host_lib()
        Nb = max(int(n.max()), 3)
        tabs = capi.DeviceTables(Nb, int(n.max()))
        tabs.fill(a)
        tabs.status()
        S1 = tabs.S1[0].cpu().numpy().copy()
        slab = tabs.tables[0].cpu().numpy().copy()
        t_out, T_out = np.zeros(G, dtype=np.uint16), np.zeros(I, dtype=np.uint32)
        sec = C.c_double(0.0)

        def host_call():
            capi.check(L.stb_tcounts_get(tc.h, t_out.ctypes.data_as(c_u16_p), T_out.ctypes.data_as(c_u32_p)))
            box["host"] = H.lj_host_sum(S1.ctypes.data, slab.ctypes.data, tabs.N, tabs.M, a, bpar.ctypes.data, I, koff.ctypes.data,
                                        n.ctypes.data, t_out.ctypes.data, None, C.byref(sec))

        res["get_host_ms"], res["get_host_ms_min"] = median_ms(host_call, reps)
        res["host_sum_alone_ms"] = sec.value * 1e3
        res["host_total_minus_device"] = box["host"] - tot
        # ---- to_groups + ssum + joint_terms
        Nd = torch.as_tensor(n.reshape(I, -1).sum(axis=1).astype(np.uint32).view(np.int32), device="cuda")

        def groups_call():
            tc.to_groups(g, bpar)
            W = capi.groups_ssum(g, [a])[0]
            capi.check(L.stb_tcounts_get(tc.h, None, T_out.ctypes.data_as(c_u32_p)))
            Td = torch.as_tensor(T_out.view(np.int32), device="cuda")
            R = float(capi.joint_terms([a], [b], Td, Nd).cpu().numpy()[0, 0])
            box["groups"] = W + R

        res["groups_ms"], res["groups_ms_min"] = median_ms(groups_call, reps)
        res["groups_total_minus_device"] = box["groups"] - tot
    finally:
        tc.free()
        L.stb_groups_free(g)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--restaurants", default="1000,100000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert capi.lib().stb_device_count() > 0, "no GPU: " + capi.last_error()
    out = [run(int(s), args.reps) for s in args.restaurants.split(",")]
    for r in out:
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
