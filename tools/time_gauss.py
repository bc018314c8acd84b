"""Times of the Gaussian-observation steps (libstb_amd/csrc/gauss.hip) on one GPU: the statistics, the draw and the matrix
through the raw calls at two corpus sizes, and on an object the dish sweep under the C x K matrix beside the same sweep
under a categorical matrix of equal K, and a whole iteration.  Every call waits for its result, so wall time is the call's.
Prints one JSON line; MEASUREMENTS.md, section GS1, records a run.

    python tools/time_gauss.py [--restaurants 1000] [--customers 200] [--K 64] [--D 16] [--reps 5] [--no-object]
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


def median_ms(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--restaurants", type=int, default=1000)
    ap.add_argument("--customers", type=int, default=200)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--D", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-object", action="store_true")
    a = ap.parse_args()
    I, per, K, D = a.restaurants, a.customers, a.K, a.D
    C = I * per
    g = torch.Generator(device="cuda").manual_seed(1)
    cust = torch.randint(0, K, (C,), device="cuda", dtype=torch.int32, generator=g)
    centre = 6.0 * torch.randn((K, D), device="cuda", dtype=torch.float64, generator=g)
    x = centre[cust.long()] + torch.randn((C, D), device="cuda", dtype=torch.float64, generator=g)
    prior = capi.gauss_prior(0.01, 1.0, 1.0)
    out = {"restaurants": I, "customers": per, "C": C, "K": K, "D": D, "matrix_bytes": 8 * C * K}
    n, mean, Q, _ = capi.gauss_stats(x, cust, K)
    mu, tau = capi.sample_gauss(n, mean, Q, prior, 1, 0)
    lik = torch.empty((C, K), dtype=torch.float64, device="cuda")
    out["stats_ms"] = median_ms(lambda: capi.gauss_stats(x, cust, K, out=(n, mean, Q)), a.reps)
    out["draw_ms"] = median_ms(lambda: capi.sample_gauss(n, mean, Q, prior, 1, 0), a.reps)
    out["matrix_ms"] = median_ms(lambda: capi.gauss_lik(x, mu, tau, out=lik), a.reps)
    out["loglik_ms"] = median_ms(lambda: capi.gauss_loglik(x, cust, mu, tau), a.reps)
    out["logml_ms"] = median_ms(lambda: capi.gauss_logml(n, mean, Q, prior), a.reps)
    # traffic the kernels cannot avoid: x twice and cust twice for the statistics; x once and the matrix once for the matrix
    out["stats_GBps"] = (2 * 8 * C * D + 2 * 4 * C) / out["stats_ms"] / 1e6
    out["matrix_GBps"] = (8 * C * D + 8 * C * K) / out["matrix_ms"] / 1e6
    if not a.no_object:
        rng = np.random.default_rng(2)
        cust_h = cust.cpu().numpy().view(np.uint32)
        pair = np.repeat(np.arange(I, dtype=np.int64), per) * K + cust_h
        nf = np.bincount(pair, minlength=I * K).astype(np.uint32).reshape(I, K)
        tf = (nf > 0).astype(np.uint16)
        Ks = np.full(I, K, dtype=np.int32)
        bpar = np.full(I, 1.0)
        ti = capi.TableIndicators(Ks, nf.reshape(-1), tf.reshape(-1), np.full(I * K, 1.0 / K), cust_h)
        try:
            ti.set_obs(x.cpu().numpy())
            ti.sample_gauss(prior, 3, 0)
            ti.sweep_dishes(0.1, bpar, 4, 0)
            ti.get()
            sw = [0]

            def sweep():
                sw[0] += 1
                ti.sweep_dishes(0.1, bpar, 4, sw[0])
                ti.get()

            def iteration():
                sweep()
                ti.sample_gauss(prior, 3, sw[0])
                ti.sample_h(1.0, 5, sw[0])

            out["sweep_gauss_ms"] = median_ms(sweep, a.reps)
            out["step_gauss_ms"] = median_ms(lambda: ti.sample_gauss(prior, 3, 1), a.reps)
            out["iteration_ms"] = median_ms(iteration, a.reps)
            ti.set_classes(rng.integers(0, 64, size=C).astype(np.uint32), 64)
            ti.set_lik(0.1 + rng.random((64, K)))
            out["sweep_categorical_ms"] = median_ms(sweep, a.reps)
        finally:
            ti.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
