"""Time the held-out log likelihood and the predictive dish proportions of an object (stb_tindic_heldout,
stb_tindic_predict; libstb_amd/csrc/predict.hip) against the host round trip they replace: stb_tindic_get, _get_state and
_get_h, a copy of the likelihood matrix, and numpy on one core (theta, then sum_k theta[restaurant, k] lik[class, k] a
held-out customer, then the logs).

  python tools/time_predict.py [--reps 10] [--host-reps 2] [--shapes A,B] [--out FILE]

Shapes (restaurants x customers x dishes x classes, held-out customers a restaurant):
  A = 2000 x 1000 x 256 x 10^4, 200        B = 10^5 x 200 x 50 x 10^3, 40
Dishes and classes at random, a = 0.3, b = 2, h = 1 / dishes.  Device times are wall-clock around calls that wait for their
own answer (median, min, max after one warm-up call).  The host column agrees with the device's total to 1e-9 relative
(checked on every run).
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

SHAPES = {"A": (2000, 1000, 256, 10000, 200), "B": (100000, 200, 50, 1000, 40)}
A_DISC, B_CONC = 0.3, 2.0


def timed(f, reps):
    f(0)
    ms = []
    for r in range(1, reps + 1):
        t0 = time.perf_counter()
        f(r)
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def host_heldout(ti, I, K, hoff, hcls, bpar, parts):
    """the round trip: everything back, then numpy on one core; returns the total"""
    L = capi.lib()
    t0 = time.perf_counter()
    t, _ = ti.get()
    n, _ = ti.get_state()
    h = ti.get_h()
    p_, rows, stride, q = ti.lik_device()
    lik = np.empty((rows, stride), dtype=np.float64)
    capi.check(L.stb_memcpy_d2h(lik.ctypes.data, p_, lik.nbytes, q))
    capi.check(L.stb_stream_sync(q))
    t1 = time.perf_counter()
    n2, t2, h2 = n.reshape(I, K).astype(np.float64), t.reshape(I, K).astype(np.float64), h.reshape(I, K)
    T, N = t2.sum(axis=1), n2.sum(axis=1)
    theta = ((n2 - t2 * A_DISC) + (bpar + T * A_DISC)[:, None] * h2) / (bpar + N)[:, None]
    rest = np.repeat(np.arange(I), np.diff(hoff.astype(np.int64)))
    total = 0.0
    for c0 in range(0, len(hcls), 65536):
        sl = slice(c0, c0 + 65536)
        total += float(np.log(np.einsum("ck,ck->c", theta[rest[sl]], lik[hcls[sl], :K])).sum())
    t2_ = time.perf_counter()
    parts["copies_ms"].append((t1 - t0) * 1e3)
    parts["numpy_ms"].append((t2_ - t1) * 1e3)
    return total


def run(name, reps, host_reps):
    I, per, K, rows, held = SHAPES[name]
    rng = np.random.default_rng(13)
    cust = rng.integers(0, K, size=I * per).astype(np.uint32)
    cls = rng.integers(0, rows, size=I * per).astype(np.uint32)
    flat = np.repeat(np.arange(I, dtype=np.int64), per) * K + cust
    n = np.bincount(flat, minlength=I * K).astype(np.uint32)
    del flat
    ti = capi.TableIndicators(np.full(I, K, dtype=np.int32), n, (n > 0).astype(np.uint16), np.full(I * K, 1.0 / K), cust)
    ti.set_classes(cls, rows)
    ti.set_lik(0.05 + rng.random((rows, K)))
    hoff = np.arange(I + 1, dtype=np.uint64) * held
    hcls = rng.integers(0, rows, size=I * held).astype(np.uint32)
    ti.set_heldout(hoff, hcls)
    bpar = np.full(I, B_CONC)
    res = {"shape": name, "restaurants": I, "customers": I * per, "dishes": K, "classes": rows, "heldout": I * held,
           "gathered_bytes": I * held * K * 8, "waves": int(os.environ.get("STB_PREDICT_WAVES", "4"))}
    out = {}

    def single(r):
        out["single"] = ti.heldout(A_DISC, bpar, want_Hi=False)[0]

    res["heldout"] = timed(single, reps)
    res["heldout_accumulate"] = timed(lambda r: ti.heldout(A_DISC, bpar, accumulate=True, want_Hi=False), reps)
    res["heldout_with_Hi"] = timed(lambda r: ti.heldout(A_DISC, bpar), reps)
    res["predict"] = timed(lambda r: ti.predict(A_DISC, bpar), reps)
    res["ns_per_heldout_customer"] = res["heldout"]["ms_median"] * 1e6 / (I * held)
    res["gathered_GBps"] = res["gathered_bytes"] / (res["heldout"]["ms_median"] * 1e6)
    if host_reps > 0:
        parts = {"copies_ms": [], "numpy_ms": []}

        def host(r):
            out["host"] = host_heldout(ti, I, K, hoff, hcls, bpar, parts)

        res["host_round_trip"] = timed(host, host_reps)
        res["host_parts_ms_median"] = {k: float(np.median(v[1:])) for k, v in parts.items()}
        res["host_over_device"] = res["host_round_trip"]["ms_median"] / res["heldout"]["ms_median"]
        res["total_device"], res["total_host"] = out["single"], out["host"]
        assert abs(out["single"] - out["host"]) <= 1e-9 * abs(out["host"]), (out["single"], out["host"])
    ti.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--shapes", default="A,B")
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
