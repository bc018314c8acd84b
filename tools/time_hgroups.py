"""Time the grouped base-weight step (stb_tindic_sample_hgroups; libstb_amd/csrc/hgroups.hip's kernels queued by htree.hip's step) against the flat draw it
generalises (stb_tindic_sample_h) on the same state.

  python tools/time_hgroups.py [--reps 5] [--restaurants 100000] [--customers 200] [--kmax 64,1024] [--groups 1,100,0]
                               [--out FILE]

The object has `restaurants` restaurants of Kmax dishes and `customers` customers each, dishes at random, one table a
pair with customers.  --groups: the numbers of equal contiguous ranges; 0 stands for every restaurant its own group.  The
step is the full one (auxiliary tables, root, concentration, groups; alpha = 5 going in, gamma0 = 1, a Gamma(1.1, 20)
prior) and, for comparison, the one that keeps root and concentration.  Times are wall-clock around calls that wait for
their own answer (median, min, max after one warm-up call).
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


def timed(f, reps):
    f(0)
    ms = []
    for r in range(1, reps + 1):
        t0 = time.perf_counter()
        f(r)
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def run(I, per, Kmax, groups, reps):
    rng = np.random.default_rng(13)
    cust = rng.integers(0, Kmax, size=(I, per))
    n = np.bincount((np.arange(I)[:, None] * Kmax + cust).reshape(-1), minlength=I * Kmax).astype(np.uint32)
    t = (n > 0).astype(np.uint16)
    ti = capi.TableIndicators(np.full(I, Kmax, dtype=np.int32), n, t)
    print("object of %d restaurants x %d dishes, %d tables" % (I, Kmax, int(t.sum())), file=sys.stderr, flush=True)
    out = []
    try:
        base = {"restaurants": I, "customers": I * per, "Kmax": Kmax, "tables": int(t.sum()),
                "waves": int(os.environ.get("STB_HGROUPS_WAVES", "4"))}
        flat = timed(lambda r: ti.sample_h(1.0, 3, r), reps)
        for G in groups:
            ti.set_hgroups(None if G == 0 else (np.arange(G + 1, dtype=np.uint64) * I) // G)
            ti.set_hroot(None)
            res = dict(base, groups=G if G else I, sample_h=flat)
            res["full_step"] = timed(lambda r: ti.sample_hgroups(5.0, 1.0, 4, r, flags=capi.HG_SAMPLE_ALPHA, shape=1.1, scale=20.0),
                                     reps)
            ti.set_hroot(None)
            res["groups_only"] = timed(lambda r: ti.sample_hgroups(5.0, 1.0, 4, r, flags=capi.HG_KEEP_ROOT), reps)
            res["ns_per_cell_full"] = res["full_step"]["ms_median"] * 1e6 / (res["groups"] * Kmax)
            print(json.dumps(res), flush=True)
            out.append(res)
    finally:
        ti.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--restaurants", type=int, default=100000)
    ap.add_argument("--customers", type=int, default=200)
    ap.add_argument("--kmax", default="64,1024")
    ap.add_argument("--groups", default="1,100,0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert capi.lib().stb_device_count() > 0, "no GPU: " + capi.last_error()
    out = []
    for k in args.kmax.split(","):
        out += run(args.restaurants, args.customers, int(k), [int(g) for g in args.groups.split(",")], args.reps)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
