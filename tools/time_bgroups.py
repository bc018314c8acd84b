"""Time the per-group concentration step against the shared-b step it generalises (MEASUREMENTS.md section B2).

  python tools/time_bgroups.py [--reps 9] [--warmup 3] [--shapes A,S1000] [--out FILE]

On one stb_tindic object per shape (section B1's shapes: A = 10^5 restaurants x 50 dishes x 200 customers, S1000 =
1000 x 50 x 200; a = 0.5, b = 10, prior Gamma(1.1, 20)), after one sweep, in turn within every round so that drift hits
each alike:

  groups_one    stb_tindic_sampleb_groups with one range over all restaurants (G = 1)
  groups_each   the same with every restaurant its own group (G = I)
  shared_arms   stb_tindic_sampleb, the shared-b step: Q on the device, then ARMS over bterms round trips

The three steps are compared by wall clock, not by device events: the ARMS step is a series of host round trips on the
object's own stream, which no pair of device events brackets.  Each call waits for its result, so the wall clock around
it is the step; `--warmup` untimed rounds, then the median (min, max) of `--reps` rounds.  The two group layouts are switched outside the timed region (stb_tindic_set_bgroups), and b is
set back to 10 before each step (stb_tindic_set_bpar, also outside it).  Further rounds with the launches' device events
armed (stb_fill_profile_begin / _end) give the sum of the three kernels' durations and the span from the first kernel's
start to the last one's end.
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


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}


def run(name, reps, warmup, a=0.5, b=10.0, shape=1.1, scale=20.0):
    import torch

    I, K, per = time_tindic.shape(name)
    Kv, n, t, cust = time_tindic.make(I, K, per)
    L = capi.lib()
    ti = capi.TableIndicators(Kv, n, t, np.full(int(n.shape[0]), 1.0 / 50), cust)
    bvec = np.full(I, b)
    one = np.array([0, I], dtype=np.uint64)
    ti.sweep(a, bvec, 2025, 0, 1)
    ti.get()
    sweep_no = [1]

    def prepare(goff):
        ti.set_bgroups(goff)
        ti.set_bpar(bvec)
        ti.get()   # (waits for the upload)

    def groups_step():
        sweep_no[0] += 1
        return ti.sampleb_groups(a, shape, scale, seed=99, sweep=sweep_no[0], want_bgrp=False)[1]

    def arms_step():
        sweep_no[0] += 1
        _libc.srand(777)
        return ti.sampleb(b, shape, scale, a, seed=99, sweep=sweep_no[0])

    cases = {"groups_one": (lambda: prepare(one), groups_step), "groups_each": (lambda: prepare(None), groups_step),
             "shared_arms": (lambda: None, arms_step)}
    ms = {k: [] for k in cases}
    last = {}
    for r in range(warmup + reps):
        for k, (before, fn) in cases.items():
            before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                ms[k].append(dt)
    out = {"shape": name, "I": I, "reps": reps, "warmup": warmup, "wall": {k: stats(v) for k, v in ms.items()},
           "b_one": float(last["groups_one"].b), "b_arms": float(last["shared_arms"]),
           "kept_groups_each": int(last["groups_each"].kept_groups), "arms_evaluations": int(capi.sampler_trace()[0].shape[0])}
    kern = {}
    for k in ("groups_one", "groups_each"):
        tot, span = [], []
        for r in range(reps):
            cases[k][0]()
            torch.cuda.synchronize()
            L.stb_fill_profile_begin()
            groups_step()
            kms, nl = C.c_double(0.0), C.c_int(0)
            capi.check(L.stb_fill_profile_end(C.byref(kms), C.byref(nl)))
            tot.append(kms.value)
            span.append(float(L.stb_fill_profile_span()))
            assert nl.value == 3, nl.value
        kern[k] = {"kernels_sum_ms": stats(tot), "span_ms": stats(span)}
    out["kernels"] = kern
    ti.free()
    L.stb_sampler_cache_clear()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="A,S1000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = [run(s, args.reps, args.warmup) for s in args.shapes.split(",")]
    for r in res:
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
