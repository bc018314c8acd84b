"""Time the hyper-parameter half of the Gibbs loop from device-resident counts against the host path it replaces
(MEASUREMENTS.md section B1).

  python tools/hyper_bench.py [--reps 7] [--warmup 2] [--shapes A,S1000] [--out FILE]

On one stb_tindic object per shape (tools/time_tindic.py's shapes: A = 10^5 restaurants x 50 dishes x 200 customers,
S1000 = 1000 x 50 x 200; a = 0.5, b = 10, h = 1/50, shuffled customer order), the same N, T and pairs for both paths:

  device   (i)   b step: stb_tindic_sampleb
           (ii)  a step: stb_tindic_to_groups + stb_groups_samplea
           (iii) stb_tindic_sweep + (i) + (ii)
           (iv)  joint step: stb_tindic_samplejoint on [0.02, 0.97] x [0.05, 500], 24 x 24 cells (hyperj.hip), a set of its
                 own with Dmax = 25; and stb_tindic_sweep + (iv).  Over --joint-iters (50) iterations of sweep + joint, the
                 state moving with the draws: stages taken and acceptance rate.  k_joint_terms alone (device events around
                 stb_joint_terms) at 24 x 24 and 64 x 64.
  host     (i)   stb_tindic_get + sampleb(N, T)          (the parent's path: Beta draws on one core, T copied back up)
           (ii)  stb_tindic_get + samplea(ragged n, t)   (the pairs down and up again)
           (iii) stb_tindic_sweep + get + sampleb + samplea

and the split of the b step: the Q kernel alone (device events around stb_sample_logq), the evaluations' round trips
(the step minus the Q call; their number from the trace), and the host baseline's Beta loop (sampleb with a = 0: the
loop, a sum and one Gamma draw).  Wall clock around calls that wait for their results; `--warmup` untimed rounds, then
the median (min, max) of `--reps` rounds.  Every round starts both libc streams from the same seeds; the state is the
same for both paths (b and a steps do not write it; the sweeps of (iii) advance it alike for whichever path runs).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from libstb_amd import capi  # noqa: E402
import time_tindic  # noqa: E402

_libc = C.CDLL(None)
_libc.srand.argtypes = [C.c_uint]
_libc.srand48.argtypes = [C.c_long]


def seed_libc():
    _libc.srand(777)
    _libc.srand48(12345)


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}


def run(name, reps, warmup, a=0.5, b=10.0, shape=1.1, scale=20.0, joint_iters=50):
    import torch

    I, K, per = time_tindic.shape(name)
    Kv, n, t, cust = time_tindic.make(I, K, per)
    G = int(n.shape[0])
    h = np.full(G, 1.0 / 50)
    L = capi.lib()
    ti = capi.TableIndicators(Kv, n, t, h, cust)
    gs = L.stb_groups_create(I, Kv.ctypes.data_as(capi.c_int_p), None, None, None, None, 0, 0, 3)
    assert gs, capi.last_error()
    gj = L.stb_groups_create(I, Kv.ctypes.data_as(capi.c_int_p), None, None, None, None, 0, 0, 25)
    assert gj, capi.last_error()
    rect = (0.02, 0.97, 0.05, 500.0)
    joint_info = {}
    Nh = np.full(I, per, dtype=np.uint32)
    bvec = np.full(I, b)
    koff = np.concatenate([[0], np.cumsum(Kv)]).astype(np.uint64)
    th, Th = np.zeros(G, dtype=np.uint16), np.zeros(I, dtype=np.uint32)
    n_addr = (np.uint64(n.ctypes.data) + np.uint64(4) * koff[:-1]).astype(np.uint64)
    t_addr = (np.uint64(th.ctypes.data) + np.uint64(2) * koff[:-1]).astype(np.uint64)
    nn = (C.POINTER(C.c_uint32) * I).from_buffer(n_addr)
    tt = (C.POINTER(C.c_uint16) * I).from_buffer(t_addr)
    u32p, u16p, dp = capi.c_u32_p, capi.c_u16_p, capi.c_double_p
    sweep_no = [0]

    def sweep():
        ti.sweep(a, bvec, 2025, sweep_no[0], 1)
        sweep_no[0] += 1

    def get():
        capi.check(L.stb_tindic_get(ti.h, th.ctypes.data_as(u16p), Th.ctypes.data_as(u32p)))

    def dev_b():
        return ti.sampleb(b, shape, scale, a, seed=99, sweep=sweep_no[0])

    def dev_a():
        ti.to_groups(gs, bvec)
        return capi.groups_samplea(gs, a)

    def dev_joint():
        r = ti.samplejoint(gj, rect, a, b, shape, scale, seed=99, sweep=sweep_no[0])
        joint_info.update(stages=r["stages"], evals=r["evals"])
        return r

    def host_b(apar=a):
        get()
        return L.sampleb(b, I, shape, scale, Nh.ctypes.data_as(u32p), Th.ctypes.data_as(u32p), apar, None, 1, 0)

    def host_a():
        get()
        return L.samplea(a, I, Kv.ctypes.data_as(capi.c_int_p), Th.ctypes.data_as(u32p), nn, tt, None, bvec.ctypes.data_as(dp),
                         None, 1, 0)

    cases = {
        "device_b": dev_b, "host_b": host_b, "device_a": dev_a, "host_a": host_a,
        "device_iter": lambda: (sweep(), dev_b(), dev_a()), "host_iter": lambda: (sweep(), host_b(), host_a()),
        "host_beta_loop": lambda: host_b(0.0),
        "device_joint": dev_joint, "device_iter_joint": lambda: (sweep(), dev_joint()),
    }
    ms = {k: [] for k in cases}
    evals = {}
    for r in range(warmup + reps):
        for k, fn in cases.items():   # (in turn, so that drift hits every case alike)
            seed_libc()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                ms[k].append(dt)
            if k in ("device_b", "host_b", "device_a", "host_a"):
                evals[k] = int(L.stb_sampler_trace_count())
    # the Q kernel alone: device time between events, and the call's wall clock (one launch and one wait)
    Nd = torch.as_tensor(Nh.view(np.int32), device="cuda")
    qdev, qwall = [], []
    for r in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        capi.sample_logq(b, scale, Nd, seed=99, sweep=r, want_L=False, stream=torch.cuda.current_stream())
        e1.record()
        dt = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        if r >= warmup:
            qdev.append(e0.elapsed_time(e1))
            qwall.append(dt)
    # k_joint_terms alone
    Td = torch.as_tensor(Th.view(np.int32), device="cuda")
    get()
    Td.copy_(torch.as_tensor(Th.view(np.int32)))
    jt = {}
    for dj in (24, 64):
        av = 0.02 + 0.95 * (np.arange(dj) + 0.5) / dj
        bv = np.exp(np.log(0.05) + np.log(1e4) * (np.arange(dj) + 0.5) / dj)
        v = []
        for r in range(warmup + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            capi.joint_terms(av, bv, Td, Nd, stream=torch.cuda.current_stream())
            e1.record()
            torch.cuda.synchronize()
            if r >= warmup:
                v.append(e0.elapsed_time(e1))
        jt["%dx%d" % (dj, dj)] = stats(v)
    # a chain of sweep + joint: stages and acceptance with the state moving
    ca, cb, acc, stg = a, b, 0, []
    for it in range(joint_iters):
        ti.sweep(ca, np.full(I, cb), 2026, it, 1)
        r = ti.samplejoint(gj, rect, ca, cb, shape, scale, seed=2027, sweep=it)
        ca, cb = r["a"], r["b"]
        acc += r["accepted"]
        stg.append(r["stages"])
    res = {"shape": name, "joint_terms_device": jt, "joint_stages": joint_info,
           "joint_chain": {"iterations": joint_iters, "accepted": acc, "stages_min": int(min(stg)), "stages_max": int(max(stg)),
                           "stages_mean": float(np.mean(stg)), "a_last": ca, "b_last": cb}, "I": I, "K": K, "customers_per_restaurant": per, "G": G, "a": a, "b": b, "reps": reps, "warmup": warmup,
           "evaluations": evals, "q_kernel_device": stats(qdev), "q_call_wall": stats(qwall)}
    for k in cases:
        res[k] = stats(ms[k])
    res["device_b_round_trips_ms"] = res["device_b"]["median_ms"] - res["q_call_wall"]["median_ms"]
    ti.free()
    L.stb_groups_free(gs)
    L.stb_groups_free(gj)
    L.stb_sampler_cache_clear()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="A,S1000")
    ap.add_argument("--joint-iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = []
    for name in args.shapes.split(","):
        r = run(name, args.reps, args.warmup, joint_iters=args.joint_iters)
        out.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
