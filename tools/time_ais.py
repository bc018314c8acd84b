"""Time annealed importance sampling of an object's held-out customers (stb_tindic_heldout_ais; libstb_amd/csrc/
seat_ais.hip) next to the particle filter and the sequential seating of the same customers in the same run.

  python tools/time_ais.py [--reps 5] [--restaurants 10000] [--particles 16] [--temps 8,32] [--passes 1] [--out FILE]

tools/time_seat_pf.py's shape: 10^4 restaurants x 200 held-out customers x 50 dishes, 1000 classes, every customer held
out on an empty object; a = 0.3, b = 2, h = 1 / dishes, a random likelihood matrix.  Times are wall-clock around calls that
wait for their own answer (median, min, max after one warm-up call).  With --pieces the parts of one temperature step are
timed alone on the replicated shape: stb_lik_temper, and one dish sweep of restaurants x particles restaurants seated from
the prior (stb_sample_tdishes) -- what is left of a step is the weight increment.  With a library that has no
stb_tindic_heldout_ais (STB_LIB_PATH at an older build) only the two existing calls are timed: that is how the parent's
figures are taken.  Nothing here sets a threshold.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from libstb_amd import capi  # noqa: E402
from time_seat import A_DISC, B_CONC, make, timed  # noqa: E402


def pieces(I, per, K, rows, R, reps, rng):
    """stb_lik_temper and one dish sweep on the replicated shape, each alone behind a wait"""
    import torch

    lik = torch.as_tensor(0.05 + rng.random((rows, K)), device="cuda")
    out = torch.empty_like(lik)
    J = I * R
    koff = torch.arange(J + 1, dtype=torch.int64, device="cuda") * K
    coff = torch.arange(J + 1, dtype=torch.int64, device="cuda") * per
    n = torch.zeros(J * K, dtype=torch.int32, device="cuda")
    t = torch.zeros(J * K, dtype=torch.int16, device="cuda")
    h = torch.full((J * K,), 1.0 / K, dtype=torch.float64, device="cuda")
    bpar = torch.full((J,), B_CONC, dtype=torch.float64, device="cuda")
    cls = torch.as_tensor(rng.integers(0, rows, size=J * per).astype(np.int32), device="cuda")
    _, T, cust, _ = capi.seat_customers(A_DISC, bpar, koff, n, t, coff, h=h, commit=True, seed=7, want_p=False)
    tabs = capi.DeviceVTables(max(per, 3), max(per, 3))
    tabs.fill(A_DISC)
    capi.check(capi.lib().stb_fill_status())
    L = capi.lib()

    def temper(r):
        capi.lik_temper(lik, 0.5, out=out)
        torch.cuda.synchronize()

    def sweep(r):
        capi.check(L.stb_sample_tdishes(tabs.tables.data_ptr(), tabs.N, tabs.M, A_DISC, bpar.data_ptr(), J, koff.data_ptr(),
                                        n.data_ptr(), t.data_ptr(), T.data_ptr(), h.data_ptr(), coff.data_ptr(), cust.data_ptr(),
                                        cls.data_ptr(), lik.data_ptr(), rows, K, 7, 100 + r, None, None))
        torch.cuda.synchronize()

    return {"lik_temper": timed(temper, reps), "dish_sweep_replicated": timed(sweep, reps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--restaurants", type=int, default=10000)
    ap.add_argument("--particles", type=int, default=16)
    ap.add_argument("--temps", default="8,32")
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("--pieces", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert capi.lib().stb_device_count() > 0, "no GPU: " + capi.last_error()
    I, per, K, rows, R = args.restaurants, 200, 50, 1000, args.particles
    rng = np.random.default_rng(17)
    bpar = np.full(I, B_CONC)
    held, _ = make(I, per, K, rows, rng, seated=False)
    held.set_heldout(np.arange(I + 1, dtype=np.uint64) * per, rng.integers(0, rows, size=I * per).astype(np.uint32))
    res = {"restaurants": I, "customers": I * per, "dishes": K, "classes": rows, "particles": R, "passes": args.passes,
           "lib": os.path.basename(capi.LIB_PATH)}
    out = {}

    def seq(r):
        out["seq"] = held.heldout_seq(A_DISC, bpar, R, 7, 4096 * r, want_Hi=False)[0]

    def pf(r):
        out["pf"] = held.heldout_pf(A_DISC, bpar, R, 0.5, 7, 4096 * r, want_Hi=False)[0]

    res["heldout_seq"] = timed(seq, args.reps)
    res["heldout_seq_total"] = out["seq"]
    res["heldout_pf_tau0.5"] = timed(pf, args.reps)
    res["heldout_pf_total"] = out["pf"]
    if hasattr(capi.lib(), "stb_tindic_heldout_ais"):
        for S in (int(x) for x in args.temps.split(",")):
            def ais(r, S=S):
                out[S] = held.heldout_ais(A_DISC, bpar, R, S, 7, 4096 * r, passes=args.passes, want_Hi=False)

            key = "heldout_ais_S%d" % S
            res[key] = timed(ais, args.reps)
            res[key + "_total"] = out[S][0]
            res[key + "_dead"] = int(out[S][2].dead)
            res[key + "_over_pf"] = res[key]["ms_median"] / res["heldout_pf_tau0.5"]["ms_median"]
            res[key + "_ms_per_temperature"] = res[key]["ms_median"] / S
        if args.pieces:
            res["pieces"] = pieces(I, per, K, rows, R, args.reps, rng)
    held.free()
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
