"""Time the dish sweep (stb_tindic_sweep_dishes, libstb_amd/csrc/tdish.hip) on the GPU against a single-core C restatement
of the same sweep on the host (tools/tdish_host.c) and against the indicator sweep (stb_tindic_sweep) on the same state,
which does strictly less per visit and is the floor.

  python tools/time_tdish.py [--sweeps 20] [--shapes A,B,D] [--classes 4] [--no-host] [--out FILE]

Shapes (restaurants x dishes x customers per restaurant, as tools/time_tindic.py: customers spread over the dishes at
random, shuffled order, a = 0.5, b = 10, h = 1/50): A = 10^5 x 50 x 200, B = 1000 x 100 x 10^4, D = 1000 x 50 x 200.
Classes at random, likelihoods uniform on [0.5, 1.5).  Device time from events on the object's stream around each call
(after one warm-up sweep, which also grows the table): median (min, max).  The host baseline sweeps a slice of the
restaurants once on one core from the same state as the device's first sweep, is scaled by customers to the whole
shape, and its draws (n, t, cust) are checked against the device's on that slice.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from libstb_amd import capi  # noqa: E402
from time_tindic import make  # noqa: E402

SHAPES = {"A": (100000, 50, 200), "B": (1000, 100, 10000), "D": (1000, 50, 200)}


def host_lib():
    src = os.path.join(ROOT, "tools", "tdish_host.c")
    out = os.path.join(ROOT, "tools", "build", "libtdish_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, src, "-lm"], check=True)
    L = C.CDLL(out)
    vp, d, u, u64 = C.c_void_p, C.c_double, C.c_uint, C.c_uint64
    L.td_host_sweep.restype = d
    L.td_host_sweep.argtypes = [vp, u, u, d, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, u, vp, vp, vp, vp, u64, u64, u64, vp]
    return L


def timed(stream, f, reps):
    import torch

    ms = []
    for r in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        f(r)
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def run(name, sweeps, rows, host, a=0.5, b=10.0, seed=2025):
    import torch

    I, K, per = SHAPES[name]
    Kv, n, t, cust = make(I, K, per)
    rng = np.random.default_rng(7)
    h = np.full(n.shape[0], 1.0 / 50)
    cls = rng.integers(0, rows, size=cust.shape[0]).astype(np.uint32)
    lik = 0.5 + rng.random((rows, K))
    bpar = np.full(I, b)
    Ctot = I * per
    ti = capi.TableIndicators(Kv, n, t, h, cust)
    ti.set_classes(cls, rows)
    ti.set_lik(lik)
    stream = torch.cuda.ExternalStream(ti.lik_device()[3])
    info = ti.sweep_dishes(a, bpar, seed, 0)  # warm-up: grows the table to N = per
    n1, cust1 = ti.get_state()
    t1, _ = ti.get()
    dish = timed(stream, lambda r: ti.sweep_dishes(a, bpar, seed, 1 + r), sweeps)
    indic = timed(stream, lambda r: ti.sweep(a, bpar, seed + 1, r), sweeps)
    ti.free()
    res = {"shape": name, "I": I, "K": K, "customers_per_restaurant": per, "C": Ctot, "classes": rows, "a": a,
           "form": "registers" if K <= 64 else "LDS", "stuck_first_sweep": int(info.stuck), "sweeps_timed": sweeps,
           "dishes": dish, "indicators_same_state": indic,
           "ns_per_step_of_a_chain": dish["ms_median"] * 1e6 / per, "visits_per_s": Ctot / (dish["ms_median"] * 1e-3),
           "dishes_over_indicators": dish["ms_median"] / indic["ms_median"]}
    if host:
        H = host_lib()
        N = M = max(per, 3)
        vt = capi.DeviceVTables(N, M)
        vt.fill(a)
        capi.check(capi.lib().stb_fill_status())
        tab = vt.packed_host(0)
        nslice = max(1, min(I, I // 50, 2000000 // per))
        koff = np.concatenate([[0], np.cumsum(Kv)]).astype(np.uint64)
        coff = np.arange(I + 1, dtype=np.uint64) * np.uint64(per)
        G0, C0 = int(koff[nslice]), int(coff[nslice])
        nh, th, ch = n.copy(), t.copy(), cust.copy()
        Th = t.reshape(I, K).astype(np.uint32).sum(axis=1).astype(np.uint32)
        stuck = C.c_uint64(0)
        sec = H.td_host_sweep(tab.ctypes.data, N, M, a, bpar.ctypes.data, 0, nslice, koff.ctypes.data, coff.ctypes.data,
                              ch.ctypes.data, cls.ctypes.data, lik.ctypes.data, K, nh.ctypes.data, th.ctypes.data,
                              Th.ctypes.data, h.ctypes.data, Ctot, seed, 0, C.byref(stuck))
        same = bool(np.array_equal(nh[:G0], n1[:G0]) and np.array_equal(th[:G0], t1[:G0]) and np.array_equal(ch[:C0], cust1[:C0]))
        res.update({"host_slice_restaurants": nslice, "host_slice_s": sec, "host_ms_scaled": sec * 1e3 * I / nslice,
                    "host_ns_per_visit": sec * 1e9 / (nslice * per), "host_same_draws_on_slice": same,
                    "device_over_host": dish["ms_median"] / (sec * 1e3 * I / nslice)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--shapes", default="A,B,D")
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert capi.lib().stb_device_count() > 0, "no GPU: " + capi.last_error()
    out = []
    for s in args.shapes.split(","):
        r = run(s, args.sweeps, args.classes, host=not args.no_host)
        print(json.dumps(r), flush=True)
        out.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
