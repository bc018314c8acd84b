"""Time the base-weight step on a tree of nested groups (stb_tindic_sample_htree, libstb_amd/csrc/htree.hip) against the
grouped step (stb_tindic_sample_hgroups), its one-level case behind another entry point, on the same state.

  python tools/time_htree.py [--reps 5] [--restaurants 100000] [--customers 200] [--kmax 64,1024]
                             [--trees 10000/10000:100/10000:100:4] [--out FILE]

The object is tools/time_hgroups.py's: `restaurants` restaurants of Kmax dishes and `customers` customers each, dishes at
random, one table a pair with customers.  --trees: the nodes of every level, level 1 first, levels cut into equal contiguous
ranges; a tree of one level is also run as the grouped step over the same ranges.  The step is the full one (auxiliary tables
upwards, root, every level's concentration, rows downwards; every alpha = 5 going in, gamma0 = 1, a Gamma(1.1, 20) prior)
and, for comparison, the one that keeps root and concentrations.  Times are wall-clock around calls that wait for their own
answer (median, min, max after one warm-up call).  `launches` counts the kernels of one full step: k_hg_count, a k_hg_aux
and a k_hg_rows a level, the root's k_hg_rows, k_ht_prep, the concentration step's three, the scatter and k_ht_finish.
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
from time_hgroups import timed  # noqa: E402


def even(n, G):
    return (np.arange(G + 1, dtype=np.uint64) * np.uint64(n)) // np.uint64(G)


def run(I, per, Kmax, trees, reps):
    rng = np.random.default_rng(13)
    cust = rng.integers(0, Kmax, size=(I, per))
    n = np.bincount((np.arange(I)[:, None] * Kmax + cust).reshape(-1), minlength=I * Kmax).astype(np.uint32)
    t = (n > 0).astype(np.uint16)
    ti = capi.TableIndicators(np.full(I, Kmax, dtype=np.int32), n, t)
    print("object of %d restaurants x %d dishes, %d tables" % (I, Kmax, int(t.sum())), file=sys.stderr, flush=True)
    out = []
    try:
        base = {"restaurants": I, "customers": I * per, "Kmax": Kmax, "tables": int(t.sum()),
                "waves": int(os.environ.get("STB_HTREE_WAVES", "4"))}
        for G in trees:
            L = len(G)
            below, offs = I, []
            for g in G:
                offs.append(even(below, g))
                below = g
            ti.set_hroot(None)
            ti.set_htree(offs)
            res = dict(base, nodes=list(G), launches=8 + 2 * L)
            res["full_step"] = timed(lambda r: ti.sample_htree([5.0] * L, 1.0, 4, r, flags=capi.HT_SAMPLE_ALPHA, shape=1.1, scale=20.0),
                                     reps)
            ti.set_hroot(None)
            ti.set_htree(offs)
            res["rows_only"] = timed(lambda r: ti.sample_htree([5.0] * L, 1.0, 4, r, flags=capi.HT_KEEP_ROOT), reps)
            if L == 1:
                ti.set_hgroups(offs[0])
                ti.set_hroot(None)
                res["hgroups_full_step"] = timed(lambda r: ti.sample_hgroups(5.0, 1.0, 4, r, flags=capi.HG_SAMPLE_ALPHA, shape=1.1,
                                                                             scale=20.0), reps)
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
    ap.add_argument("--trees", default="10000/10000:100/10000:100:4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert capi.lib().stb_device_count() > 0, "no GPU: " + capi.last_error()
    trees = [[int(g) for g in tree.split(":")] for tree in args.trees.split("/")]
    out = []
    for k in args.kmax.split(","):
        out += run(args.restaurants, args.customers, int(k), trees, args.reps)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
