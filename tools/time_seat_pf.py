"""Time the particle filter of an object's held-out customers (stb_tindic_heldout_pf; libstb_amd/csrc/seat_pf.hip) next to
the sequential seating of the same customers (stb_tindic_heldout_seq) in the same run.

  python tools/time_seat_pf.py [--reps 7] [--restaurants 10000] [--particles 16] [--out FILE]

10^4 restaurants x 200 held-out customers x 50 dishes, 1000 classes, every customer held out on an empty object (the
shape Q of tools/time_seat.py, ten times the restaurants); a = 0.3, b = 2, h = 1 / dishes, a random likelihood matrix.
Times are wall-clock around calls that wait for their own answer (median, min, max after one warm-up call).  With a
library that has no stb_tindic_heldout_pf (STB_LIB_PATH at an older build) only the sequential call is timed: that is how
the parent's figure is taken.  Nothing here sets a threshold.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from libstb_amd import capi  # noqa: E402
from time_seat import A_DISC, B_CONC, make, timed  # noqa: E402

TAUS = (0.0, 0.5, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--restaurants", type=int, default=10000)
    ap.add_argument("--particles", type=int, default=16)
    ap.add_argument("--seq-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert capi.lib().stb_device_count() > 0, "no GPU: " + capi.last_error()
    I, per, K, rows, R = args.restaurants, 200, 50, 1000, args.particles
    rng = np.random.default_rng(17)
    bpar = np.full(I, B_CONC)
    held, _ = make(I, per, K, rows, rng, seated=False)
    held.set_heldout(np.arange(I + 1, dtype=np.uint64) * per, rng.integers(0, rows, size=I * per).astype(np.uint32))
    res = {"restaurants": I, "customers": I * per, "dishes": K, "classes": rows, "particles": R,
           "waves": os.environ.get("STB_SEAT_WAVES", "default"), "lib": os.path.basename(capi.LIB_PATH)}
    out = {}

    def seq(r):
        out["seq"] = held.heldout_seq(A_DISC, bpar, R, 7, 4096 * r, want_Hi=False)[0]

    res["heldout_seq"] = timed(seq, args.reps)
    res["heldout_seq_total"] = out["seq"]
    if not args.seq_only:
        for tau in TAUS:
            def pf(r, tau=tau):
                out[tau] = held.heldout_pf(A_DISC, bpar, R, tau, 7, 4096 * r, want_Hi=False)

            key = "heldout_pf_tau%g" % tau
            res[key] = timed(pf, args.reps)
            res[key + "_total"] = out[tau][0]
            res[key + "_resamplings_per_restaurant"] = out[tau][2].resamplings / I
            res[key + "_over_seq"] = res[key]["ms_median"] / res["heldout_seq"]["ms_median"]
    held.free()
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
