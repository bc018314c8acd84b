"""Time the table-indicator sweep (stb_sample_tindic, libstb_amd/csrc/tindic.hip) on the GPU under both kernel forms,
against a single-core C restatement of the same sweep on the host (tools/tindic_host.c).

  python tools/time_tindic.py [--sweeps 20] [--shapes A,B,C] [--forms lane,wave] [--no-host] [--out FILE]

Shapes (restaurants x dishes x customers per restaurant, customers spread over the dishes at random, shuffled order,
a = 0.5, b = 10, h = 1/50): A = 10^5 x 50 x 200, B = 1000 x 100 x 10^4, C = 3 x 50 x 2000 (demo.c's size); S<I> =
I x 50 x 200 (the crossover scan).  V table (max n, max n) filled once.  Device time from events around each sweep
(after one warm-up sweep): median (min, max).  The host baseline sweeps a slice of the restaurants once on one core
from the same state as the device's first sweep, is scaled by customers to the whole shape, and its draws are checked
against the device's on that slice.
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
from libstb_amd import capi  # noqa: E402

SHAPES = {"A": (100000, 50, 200), "B": (1000, 100, 10000), "C": (3, 50, 2000)}


def shape(name):
    if name in SHAPES:
        return SHAPES[name]
    assert name.startswith("S"), name
    return (int(name[1:]), 50, 200)


def host_lib():
    src = os.path.join(ROOT, "tools", "tindic_host.c")
    out = os.path.join(ROOT, "tools", "build", "libtindic_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, src, "-lm"], check=True)
    L = C.CDLL(out)
    vp, d, u, u64 = C.c_void_p, C.c_double, C.c_uint, C.c_uint64
    L.ti_host_sweep.restype = d
    L.ti_host_sweep.argtypes = [vp, u, u, d, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, u, u64, u64]
    return L


def make(I, K, per, seed=2025):
    """I restaurants of K dishes and `per` customers each: n multinomial, t = 1 + floor(u sqrt(n)), shuffled order"""
    rng = np.random.default_rng(seed)
    n = rng.multinomial(per, np.full(K, 1.0 / K), size=I).astype(np.uint32).reshape(-1)
    t = np.where(n > 0, 1 + np.floor(rng.random(n.shape[0]) * np.sqrt(n)), 0)
    t = np.minimum(t, n).astype(np.uint16)
    rest = np.repeat(np.arange(I), per)
    dish = np.repeat(np.tile(np.arange(K, dtype=np.uint32), I), n.astype(np.int64))
    cust = dish[np.lexsort((rng.random(rest.shape[0]), rest))].astype(np.uint32)
    return np.full(I, K, dtype=np.int32), n, t, cust


def run(name, form, sweeps, host, a=0.5, b=10.0, seed=2025):
    import torch

    I, K, per = shape(name)
    Kv, n, t, cust = make(I, K, per)
    h = np.full(n.shape[0], 1.0 / 50)
    N = M = max(int(n.max()), 3)
    L = capi.lib()
    os.environ["STB_TINDIC_FORM"] = form
    vt = capi.DeviceVTables(N, M)
    vt.fill(a)
    capi.check(L.stb_fill_status())
    koff_h = np.concatenate([[0], np.cumsum(Kv)]).astype(np.uint64)
    coff_h = np.arange(I + 1, dtype=np.uint64) * np.uint64(per)
    T0 = t.reshape(I, K).astype(np.uint32).sum(axis=1).astype(np.uint32)
    dev = "cuda"
    koff = torch.as_tensor(koff_h.view(np.int64), device=dev)
    coff = torch.as_tensor(coff_h.view(np.int64), device=dev)
    d_cust = torch.as_tensor(cust.view(np.int32), device=dev)
    d_n = torch.as_tensor(n.view(np.int32), device=dev)
    d_t = torch.as_tensor(t.view(np.int16), device=dev).clone()
    d_T = torch.as_tensor(T0.view(np.int32), device=dev).clone()
    d_h = torch.as_tensor(h, device=dev)
    d_b = torch.as_tensor(np.full(I, b), device=dev)

    def sweep(s):
        capi.check(L.stb_sample_tindic(vt.tables.data_ptr(), N, M, a, d_b.data_ptr(), I, koff.data_ptr(), d_n.data_ptr(),
                                       d_t.data_ptr(), d_T.data_ptr(), d_h.data_ptr(), coff.data_ptr(), d_cust.data_ptr(),
                                       0, seed, s, capi.stream_ptr()))

    nslice = max(1, min(I, I // 50, 2000000 // per))
    G0 = int(koff_h[nslice])
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
    Ctot = I * per
    med = float(np.median(ms))
    res = {"shape": name, "form": form, "I": I, "K": K, "customers_per_restaurant": per, "C": Ctot, "N": N, "a": a,
           "ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)), "sweeps_timed": sweeps,
           "ns_per_step_of_a_chain": med * 1e6 / per, "visits_per_s": Ctot / (med * 1e-3)}
    if host:
        H = host_lib()
        tab = vt.packed_host(0)
        t_host, T_host, b_host = t.copy(), T0.copy(), np.full(I, b)
        sec = H.ti_host_sweep(tab.ctypes.data, N, M, a, b_host.ctypes.data, 0, nslice, koff_h.ctypes.data,
                              coff_h.ctypes.data, cust.ctypes.data, n.ctypes.data, t_host.ctypes.data, T_host.ctypes.data,
                              h.ctypes.data, 0, seed, 0)
        res.update({"host_slice_restaurants": nslice, "host_slice_s": sec, "host_ms_scaled": sec * 1e3 * I / nslice,
                    "host_ns_per_visit": sec * 1e9 / (nslice * per),
                    "host_same_draws_on_slice": bool(np.array_equal(t_host[:G0], t_dev0)), "host_slice_pairs": G0})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--shapes", default="A,B,C")
    ap.add_argument("--forms", default="lane,wave")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert capi.lib().stb_device_count() > 0, "no GPU: " + capi.last_error()
    out = []
    for s in args.shapes.split(","):
        for j, f in enumerate(args.forms.split(",")):
            r = run(s, f, args.sweeps, host=not args.no_host and j == 0)
            print(json.dumps(r), flush=True)
            out.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
