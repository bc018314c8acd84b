"""Time the likelihood draw (stb_sample_lik, libstb_amd/csrc/tlik.hip) and the full uncollapsed step on an object
(stb_tindic_sample_lik + stb_tindic_sample_h, counts taken on the device) against the host round trip they replace:
stb_tindic_class_counts to the host, numpy's Generator.gamma on one core, a normalisation, stb_tindic_set_lik back.

  python tools/time_tlik.py [--reps 10] [--host-reps 2] [--shapes S,L] [--out FILE]

Shapes (classes x dishes): S = 10^4 x 256, L = 10^5 x 1024.  The object has 2000 restaurants of `dishes` dishes and 1000
customers each, dishes and classes at random; beta0 = 0.5, gamma0 = 1.  Device times are wall-clock around calls that
wait for their own answer (median, min, max after one warm-up call); the data term (stb_tindic_loglik) is timed too.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libstb_amd import capi  # noqa: E402

SHAPES = {"S": (10000, 256), "L": (100000, 1024)}


def timed(f, reps):
    f(0)
    ms = []
    for r in range(1, reps + 1):
        t0 = time.perf_counter()
        f(r)
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def run(name, reps, host_reps, I=2000, per=1000):
    import torch

    rows, stride = SHAPES[name]
    rng = np.random.default_rng(11)
    cust = rng.integers(0, stride, size=I * per).astype(np.uint32)
    cls = rng.integers(0, rows, size=I * per).astype(np.uint32)
    n = np.stack([np.bincount(cust[i * per:(i + 1) * per].astype(np.int64), minlength=stride) for i in range(I)])
    n = n.astype(np.uint32).reshape(-1)
    ti = capi.TableIndicators(np.full(I, stride, dtype=np.int32), n, (n > 0).astype(np.uint16), None, cust)
    ti.set_classes(cls, rows)
    ti.set_lik(None, rows, stride)
    cnt = ti.class_counts()
    d_cnt = torch.as_tensor(cnt.view(np.int32), device="cuda")
    d_lik = torch.empty((rows, stride), dtype=torch.float64, device="cuda")
    res = {"shape": name, "rows": rows, "stride": stride, "cells": rows * stride, "restaurants": I, "customers": I * per,
           "waves": int(os.environ.get("STB_TLIK_WAVES", "4"))}
    res["draw_raw"] = timed(lambda r: capi.sample_lik(d_cnt, 0.5, 1, r, out=d_lik), reps)
    res["ns_per_cell_raw"] = res["draw_raw"]["ms_median"] * 1e6 / (rows * stride)
    res["loglik_raw"] = timed(lambda r: capi.lik_loglik(d_cnt, d_lik), reps)
    res["object_sample_lik"] = timed(lambda r: ti.sample_lik(0.5, 2, r), reps)
    res["object_sample_h"] = timed(lambda r: ti.sample_h(1.0, 3, r), reps)
    res["object_loglik"] = timed(lambda r: ti.loglik(), reps)

    def full(r):
        ti.sample_lik(0.5, 2, r)
        ti.sample_h(1.0, 3, r)

    res["object_full_step"] = timed(full, reps)
    if host_reps > 0:
        gen = np.random.default_rng(5)
        parts = {"class_counts_ms": [], "gamma_ms": [], "set_lik_ms": []}

        def host(r):
            t0 = time.perf_counter()
            c = ti.class_counts()
            t1 = time.perf_counter()
            g = gen.gamma(0.5 + c.astype(np.float64))
            g /= g.sum(axis=0, keepdims=True)
            t2 = time.perf_counter()
            ti.set_lik(g)
            t3 = time.perf_counter()
            for k, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2)):
                parts[k].append(v * 1e3)

        res["host_round_trip"] = timed(host, host_reps)
        res["host_parts_ms_median"] = {k: float(np.median(v[1:])) for k, v in parts.items()}
        res["host_over_device_sample_lik"] = res["host_round_trip"]["ms_median"] / res["object_sample_lik"]["ms_median"]
    ti.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--shapes", default="S,L")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert capi.lib().stb_device_count() > 0, "no GPU: " + capi.last_error()
    out = []
    for s in args.shapes.split(","):
        r = run(s, args.reps, args.host_reps)
        print(json.dumps(r), flush=True)
        out.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
