"""Time the class draw of an object (stb_tindic_sample_classes, stb_tindic_generate; libstb_amd/csrc/classgen.hip) next to
stb_tindic_seat on the same object and a one-core numpy generation of the same corpus.

  python tools/time_classgen.py [--reps 7] [--out FILE] [--once]

Shape: 10^5 restaurants x 200 customers, K = 50 dishes, 1000 classes; a = 0.3, b = 2, h = 1 / K; every column of the
matrix a Dirichlet(0.5) draw.  Times are wall-clock around calls that wait for their own answer (median, min, max after
one warm-up call).  The numpy figure draws the classes alone, given the dishes the device seated: per dish a cumulative
sum of its column and one searchsorted over that dish's customers, on one core -- the seating has no vectorised host
form to put beside k_seat.  --once: one call of each, for a kernel trace.  Nothing here sets a threshold.
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

I, PER, K, ROWS = 100000, 200, 50, 1000
A_DISC, B_CONC = 0.3, 2.0


def timed(f, reps, warm=True):
    if warm:
        f(0)
    ms = []
    for r in range(1, reps + 1):
        t0 = time.perf_counter()
        f(r)
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def numpy_classes(lik, cust, rng):
    """the classes of the customers at dishes `cust`, one core"""
    cls = np.empty(len(cust), dtype=np.uint32)
    order = np.argsort(cust, kind="stable")
    edges = np.searchsorted(cust[order], np.arange(K + 1))
    for k in range(K):
        sel = order[edges[k]:edges[k + 1]]
        cum = np.cumsum(lik[:, k])
        cls[sel] = np.minimum(np.searchsorted(cum, rng.random(len(sel)) * cum[-1], side="right"), ROWS - 1)
    return cls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    assert capi.lib().stb_device_count() > 0, "no GPU: " + capi.last_error()
    reps, warm = (1, False) if args.once else (args.reps, True)
    rng = np.random.default_rng(23)
    bpar = np.full(I, B_CONC)
    n = np.zeros(I * K, dtype=np.uint32)
    n[::K] = PER                                    # (the customers' number is all the start state says: they are seated again)
    ti = capi.TableIndicators(np.full(I, K, dtype=np.int32), n, (n > 0).astype(np.uint16), np.full(I * K, 1.0 / K))
    lik = np.ascontiguousarray(rng.dirichlet(np.full(ROWS, 0.5), size=K).T)
    ti.set_lik(lik)
    res = {"restaurants": I, "customers": I * PER, "dishes": K, "classes": ROWS, "waves": int(os.environ.get("STB_CLS_WAVES", "4"))}
    out = {}

    def generate(r):
        out["seat"], out["cls"] = ti.generate(A_DISC, bpar, 5, r)

    res["generate"] = timed(generate, reps, warm)
    res["drawn"] = int(out["cls"].drawn)
    res["sample_classes"] = timed(lambda r: ti.sample_classes(6, r), reps, warm)
    res["sample_classes_ns_per_customer"] = res["sample_classes"]["ms_median"] * 1e6 / (I * PER)
    res["seat"] = timed(lambda r: ti.seat(A_DISC, bpar, 7, r), reps, warm)
    if not args.once:
        cust = ti.get_state()[1]
        res["numpy_classes"] = timed(lambda r: numpy_classes(lik, cust, rng), reps)
    ti.free()
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
