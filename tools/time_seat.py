"""Time the forward seating of an object (stb_tindic_seat, stb_tindic_heldout_seq; libstb_amd/csrc/seat.hip) next to one
dish sweep of the same object in the same run (stb_tindic_sweep_dishes).

  python tools/time_seat.py [--reps 5] [--shapes S,Q] [--out FILE]

Shapes (restaurants x customers x dishes, 1000 classes):
  S = 10^5 x 200 x 50: stb_tindic_seat on all customers, then one dish sweep on the state it left
  Q = 1000 x 200 x 50, every customer held out on an empty object: stb_tindic_heldout_seq at R = 1, 16 and 64 particles,
      then (the customers seated) one dish sweep
  L = 10^4 x 200 x 100: as S with more than 64 dishes a restaurant -- k_seat<false> and the LDS form of the visit and of
      the dish sweep (not among the defaults)
Classes at random, a = 0.3, b = 2, h = 1 / dishes, a random likelihood matrix.  Times are wall-clock around calls that
wait for their own answer (median, min, max after one warm-up call); the first stb_tindic_seat of an object also
materialises the customer sequence, so it is the warm-up.  Nothing here sets a threshold.
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

SHAPES = {"S": (100000, 200, 50, 1000), "Q": (1000, 200, 50, 1000), "L": (10000, 200, 100, 1000)}
A_DISC, B_CONC = 0.3, 2.0
PARTICLES = (1, 16, 64)


def timed(f, reps):
    f(0)
    ms = []
    for r in range(1, reps + 1):
        t0 = time.perf_counter()
        f(r)
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def make(I, per, K, rows, rng, seated: bool):
    cust = rng.integers(0, K, size=I * per).astype(np.uint32)
    cls = rng.integers(0, rows, size=I * per).astype(np.uint32)
    if seated:
        n = np.bincount(np.repeat(np.arange(I, dtype=np.int64), per) * K + cust, minlength=I * K).astype(np.uint32)
        ti = capi.TableIndicators(np.full(I, K, dtype=np.int32), n, (n > 0).astype(np.uint16), np.full(I * K, 1.0 / K), cust)
        ti.set_classes(cls, rows)
    else:
        ti = capi.TableIndicators(np.full(I, K, dtype=np.int32), np.zeros(I * K, dtype=np.uint32), np.zeros(I * K, dtype=np.uint16),
                                  np.full(I * K, 1.0 / K))
    ti.set_lik(0.05 + rng.random((rows, K)))
    return ti, cls


def run(name, reps):
    I, per, K, rows = SHAPES[name]
    rng = np.random.default_rng(17)
    bpar = np.full(I, B_CONC)
    res = {"shape": name, "restaurants": I, "customers": I * per, "dishes": K, "classes": rows,
           "waves": int(os.environ.get("STB_SEAT_WAVES", "4"))}
    ti, cls = make(I, per, K, rows, rng, seated=True)
    out = {}
    if name in ("S", "L"):
        def seat(r):
            out["total"], out["info"] = ti.seat(A_DISC, bpar, 5, r)

        res["seat"] = timed(seat, reps)
        res["seat_total"] = out["total"]
        res["seat_impossible"] = int(out["info"].impossible)
        res["ns_per_customer"] = res["seat"]["ms_median"] * 1e6 / (I * per)
    else:
        held, _ = make(I, per, K, rows, rng, seated=False)
        held.set_heldout(np.arange(I + 1, dtype=np.uint64) * per, cls)
        for R in PARTICLES:
            def seq(r, R=R):
                out[R] = held.heldout_seq(A_DISC, bpar, R, 7, 4096 * r, want_Hi=False)[0]

            res["heldout_seq_R%d" % R] = timed(seq, reps)
            res["heldout_seq_R%d_total" % R] = out[R]
            res["ns_per_customer_particle_R%d" % R] = res["heldout_seq_R%d" % R]["ms_median"] * 1e6 / (I * per * R)
        held.free()
    res["sweep_dishes"] = timed(lambda r: ti.sweep_dishes(A_DISC, bpar, 9, r), reps)
    ti.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="S,Q")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert capi.lib().stb_device_count() > 0, "no GPU: " + capi.last_error()
    out = []
    for s in args.shapes.split(","):
        r = run(s, args.reps)
        print(json.dumps(r), flush=True)
        out.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
