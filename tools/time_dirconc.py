"""Time the Dirichlet concentration step (stb_sample_dirconc, libstb_amd/csrc/dirconc.hip) in the columns orientation,
beside the likelihood draw (stb_sample_lik) on the same count matrix: the step it sits next to in an iteration.

  python tools/time_dirconc.py [--reps 10] [--shapes D,Z] [--forms default,lane,wave] [--out FILE]

Shapes (classes x dishes):
  D  300 x 70: the (class, dish) counts of 10^5 restaurants x 200 customers, 2 x 10^7 customers at random cells
  Z  10^5 x 1024 with Zipf-distributed counts totalling 2 x 10^7: cell weights 1 / rank over a random order of the cells
Both calls wait for their own answer; times are wall-clock (median, min, max after one warm-up call), one process.  The
forms set STB_DIRCONC_FORM for the step's calls (who takes a cell's Bernoulli draws); they change no bit of s'.
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

TOTAL = 20_000_000


def matrix(name):
    rng = np.random.default_rng(23)
    if name == "D":
        rows, cols = 300, 70
        cells = rng.integers(0, rows * cols, size=TOTAL)
        return np.bincount(cells, minlength=rows * cols).astype(np.uint32).reshape(rows, cols)
    rows, cols = 100_000, 1024
    ncell = rows * cols
    k = 4_000_000                                    # cells that hold a count: ranks 1 .. k at random places
    p = 1.0 / np.arange(1, k + 1)
    c = rng.multinomial(TOTAL, p / p.sum()).astype(np.uint32)
    cnt = np.zeros(ncell, dtype=np.uint32)
    np.add.at(cnt, rng.integers(0, ncell, size=k), c)   # (two ranks may meet in a cell: their counts add)
    return cnt.reshape(rows, cols)


def timed(f, reps):
    f(0)
    ms = []
    for r in range(1, reps + 1):
        t0 = time.perf_counter()
        f(r)
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def run(name, reps, forms):
    import torch

    cnt = matrix(name)
    rows, cols = cnt.shape
    d_cnt = torch.as_tensor(cnt.view(np.int32), device="cuda")
    d_lik = torch.empty((rows, cols), dtype=torch.float64, device="cuda")
    res = {"shape": name, "rows": rows, "cols": cols, "count": int(cnt.sum(dtype=np.uint64)), "nonzero": int((cnt > 0).sum()),
           "largest_cell": int(cnt.max()), "past_twave": int((cnt > 257).sum())}
    res["sample_lik"] = timed(lambda r: capi.sample_lik(d_cnt, 0.5, 1, r, out=d_lik), reps)
    seen = set()
    for form in forms:
        if form == "default":
            os.environ.pop("STB_DIRCONC_FORM", None)
        else:
            os.environ["STB_DIRCONC_FORM"] = form
        out = []
        res["dirconc_" + form] = timed(lambda r: out.append(capi.sample_dirconc(d_cnt, 1.0, 0.5, 1.1, 1.0, 2, r, capi.DM_COLUMNS,
                                                                                want=())[2]), reps)
        res["aux_tables_" + form] = int(out[1].aux_tables)
        seen.add((out[1].s, out[1].aux_tables))
        res["over_sample_lik_" + form] = res["dirconc_" + form]["ms_median"] / res["sample_lik"]["ms_median"]
    os.environ.pop("STB_DIRCONC_FORM", None)
    res["forms_agree"] = len(seen) == 1
    torch.cuda.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="D,Z")
    ap.add_argument("--forms", default="default,lane,wave")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert capi.lib().stb_device_count() > 0, "no GPU: " + capi.last_error()
    out = []
    for s in args.shapes.split(","):
        r = run(s, args.reps, args.forms.split(","))
        print(json.dumps(r), flush=True)
        out.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
