"""Times of the held-out predictive density under Gaussian observations (libstb_amd/csrc/gauss_heldout.hip) on one GPU:
one stb_tindic_gauss_heldout call on an object (it waits for its answer: wall time), the raw stb_gauss_heldout alone
between device events (k_gs_prep and the point kernel; with and without the responsibilities and the accumulator), and
beside them stb_gauss_lik at the same (C, K, D), which does the same arithmetic a cell and writes 8 K bytes a row where the
point kernel writes 8.  Prints one JSON line; MEASUREMENTS.md, section GS2, records a run.  With --lik-only nothing of the
held-out interface is called, so the script also runs against a library that lacks it (STB_LIB_PATH).

    python tools/time_gauss_heldout.py [--points 100000] [--restaurants 1000] [--K 64] [--D 16] [--reps 20] [--lik-only]
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


def event_ms(f, reps):
    """median and minimum device time of f between two events on the current stream, after two warm calls"""
    import torch

    for _ in range(2):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(np.min(ts))


def wall_ms(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--restaurants", type=int, default=1000)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--D", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lik-only", action="store_true")
    a = ap.parse_args()
    I, Ch, K, D = a.restaurants, a.points, a.K, a.D
    per = Ch // I
    Ch = per * I
    g = torch.Generator(device="cuda").manual_seed(1)
    z = torch.randint(0, K, (Ch,), device="cuda", dtype=torch.int32, generator=g)
    mu = 6.0 * torch.randn((K, D), device="cuda", dtype=torch.float64, generator=g)
    tau = 0.5 + torch.rand((K, D), device="cuda", dtype=torch.float64, generator=g)
    y = mu[z.long()] + torch.randn((Ch, D), device="cuda", dtype=torch.float64, generator=g)
    out = {"points": Ch, "restaurants": I, "K": K, "D": D, "lib": os.path.basename(capi.LIB_PATH)}
    lik = torch.empty((Ch, K), dtype=torch.float64, device="cuda")
    # stb_gauss_lik waits for its info words: its device time is taken from the events around the whole call
    out["gauss_lik_ms"], out["gauss_lik_min_ms"] = event_ms(lambda: capi.gauss_lik(y, mu, tau, out=lik), a.reps)
    if not a.lik_only:
        hoff = torch.arange(I + 1, device="cuda", dtype=torch.int64) * per
        theta = torch.rand((I, K), device="cuda", dtype=torch.float64, generator=g)
        theta /= theta.sum(dim=1, keepdim=True)
        M = torch.full((Ch,), -float("inf"), dtype=torch.float64, device="cuda")
        A = torch.zeros(Ch, dtype=torch.float64, device="cuda")
        out["point_ms"], out["point_min_ms"] = event_ms(lambda: capi.gauss_heldout(theta, hoff, y, mu, tau), a.reps)
        out["point_acc_ms"], _ = event_ms(lambda: capi.gauss_heldout(theta, hoff, y, mu, tau, want_ell=False, acc=(M, A)), a.reps)
        out["point_resp_ms"], _ = event_ms(lambda: capi.gauss_heldout(theta, hoff, y, mu, tau, rstride=K), a.reps)
        ell, _ = capi.gauss_heldout(theta, hoff, y, mu, tau)
        out["sum_wall_ms"], _ = wall_ms(lambda: capi.gauss_heldout_loglik(hoff, ell=ell), a.reps)
        # the object: as many customers as held-out points, spread evenly over the dishes
        cust = z.cpu().numpy().view(np.uint32)
        pair = np.repeat(np.arange(I, dtype=np.int64), per) * K + cust
        nf = np.bincount(pair, minlength=I * K).astype(np.uint32)
        ti = capi.TableIndicators(np.full(I, K, dtype=np.int32), nf, (nf > 0).astype(np.uint16), np.full(I * K, 1.0 / K), cust)
        try:
            ti.set_obs(y.cpu().numpy())
            ti.set_gauss(mu.cpu().numpy(), tau.cpu().numpy())
            ti.set_heldout_obs(hoff.cpu().numpy(), y.cpu().numpy())
            bpar = np.full(I, 1.0)
            out["object_ms"], out["object_min_ms"] = wall_ms(lambda: ti.gauss_heldout(0.1, bpar, want_Hi=False), a.reps)
            out["object_acc_ms"], _ = wall_ms(lambda: ti.gauss_heldout(0.1, bpar, accumulate=True, want_Hi=False), a.reps)
        finally:
            ti.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
