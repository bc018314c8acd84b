"""Time the collapsed log joint (stb_tindic_logjoint_collapsed, libstb_amd/csrc/dirmult.hip) and its two integrated terms
as raw calls (stb_dirmult_logml) against the host route they replace -- the counts to the host (stb_tindic_get /
stb_tindic_class_counts), then scipy.special.gammaln on one core -- and against one read of the count matrix from HBM.

  python tools/time_collapsed.py [--reps 10] [--host-reps 3] [--tables 64:100,64:0,1024:100,1024:0] [--data S,L] [--out FILE]

--tables Kmax:G  the grouped tables' term on tools/time_hgroups.py's object: 10^5 restaurants of Kmax dishes and 200
                 customers each, dishes at random, one table a pair with customers; G equal contiguous ranges, 0 for every
                 restaurant its own group; alpha = 5, the root 1 / Kmax each.
--data S|L       the classes' term on tools/time_tlik.py's object: 2000 restaurants x 1000 customers, classes x dishes
                 S = 10^4 x 256, L = 10^5 x 1024; beta = 0.5, the flat model for the tables (gamma = 1).
Device times are wall-clock around calls that wait for their own answer, inputs resident (median, min, max after one
warm-up call).  hbm_floor_ms is the count matrix's bytes over 6.3 TB/s, the streaming rate measured on this part.
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

SHAPES = {"S": (10000, 256), "L": (100000, 1024)}
HBM_BYTES_PER_S = 6.3e12


def timed(f, reps):
    f(0)
    ms = []
    for r in range(1, reps + 1):
        t0 = time.perf_counter()
        f(r)
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def host_logml(c, w, axis):
    """the formula with gammaln: the multinomials run along `axis` of c; w broadcasts against c"""
    from scipy.special import gammaln

    c = c.astype(np.float64)
    W = float(np.sum(w)) if np.ndim(w) else float(w) * c.shape[axis]
    nz = c > 0
    wb = np.broadcast_to(w, c.shape)[nz]
    return float(np.sum(gammaln(W) - gammaln(W + c.sum(axis=axis))) + np.sum(gammaln(wb + c[nz]) - gammaln(wb)))


def run_tables(Kmax, G, reps, host_reps, I=100000, per=200):
    import torch

    rng = np.random.default_rng(13)
    cust = rng.integers(0, Kmax, size=(I, per))
    n = np.bincount((np.arange(I)[:, None] * Kmax + cust).reshape(-1), minlength=I * Kmax).astype(np.uint32)
    t = (n > 0).astype(np.uint16)
    ti = capi.TableIndicators(np.full(I, Kmax, dtype=np.int32), n, t)
    goff = np.arange(I + 1, dtype=np.uint64) if G == 0 else (np.arange(G + 1, dtype=np.uint64) * I) // G
    groups = len(goff) - 1
    alpha, bpar = 5.0, np.full(I, 2.0)
    res = {"term": "tables", "restaurants": I, "customers": I * per, "Kmax": Kmax, "groups": groups, "tables": int(t.sum()),
           "cells": groups * Kmax, "waves": int(os.environ.get("STB_DIRMULT_WAVES", "4"))}
    try:
        if G:
            ti.set_hgroups(goff)
        res["object_collapsed"] = timed(lambda r: ti.logjoint_collapsed(0.3, bpar, alpha), reps)
        res["object_logjoint"] = timed(lambda r: ti.logjoint(0.3, bpar, want_Li=False), reps)
        val, ci = ti.logjoint_collapsed(0.3, bpar, alpha)
        c = np.add.reduceat(t.reshape(I, Kmax).astype(np.uint32), goff[:-1].astype(np.int64), axis=0)
        d_c = torch.as_tensor(c.view(np.int32), device="cuda")
        rows_call = lambda r: capi.dirmult_logml(d_c, 1.0 / Kmax, capi.DM_ROWS, scale=alpha, want_each=False)
        res["raw_rows"] = timed(rows_call, reps)
        # the two forms of the rows kernel, forced in turn on the same inputs (the bits are equal; the default is one of them)
        kept = os.environ.get("STB_DIRMULT_FORM")
        for form in ("fused", "split"):
            os.environ["STB_DIRMULT_FORM"] = form
            res["raw_rows_" + form] = timed(rows_call, reps)
            res["value_" + form] = rows_call(0)[0]
        if kept is None:
            del os.environ["STB_DIRMULT_FORM"]
        else:
            os.environ["STB_DIRMULT_FORM"] = kept
        res["nonzero"] = int(ci.dm_tables.nonzero)
        res["hbm_floor_ms"] = 4.0 * groups * Kmax / HBM_BYTES_PER_S * 1e3
        res["tables_value"] = ci.tables
        if host_reps > 0:
            def host(r):
                tt, _ = ti.get()
                cc = np.add.reduceat(tt.reshape(I, Kmax).astype(np.uint32), goff[:-1].astype(np.int64), axis=0)
                res["host_value"] = host_logml(cc, alpha * (1.0 / Kmax), 1)

            res["host_route"] = timed(host, host_reps)
            res["host_over_raw"] = res["host_route"]["ms_median"] / res["raw_rows"]["ms_median"]
    finally:
        ti.free()
    return res


def run_data(name, reps, host_reps, I=2000, per=1000):
    import torch

    rows, stride = SHAPES[name]
    rng = np.random.default_rng(11)
    cust = rng.integers(0, stride, size=I * per).astype(np.uint32)
    cls = rng.integers(0, rows, size=I * per).astype(np.uint32)
    n = np.stack([np.bincount(cust[i * per:(i + 1) * per].astype(np.int64), minlength=stride) for i in range(I)])
    n = n.astype(np.uint32).reshape(-1)
    ti = capi.TableIndicators(np.full(I, stride, dtype=np.int32), n, (n > 0).astype(np.uint16), None, cust)
    bpar = np.full(I, 2.0)
    res = {"term": "data", "shape": name, "rows": rows, "stride": stride, "cells": rows * stride, "restaurants": I,
           "customers": I * per,  # (without STB_DIRMULT_WAVES the columns kernel takes 8 waves from 512 columns on)
           "waves": int(os.environ.get("STB_DIRMULT_WAVES", "8" if stride >= 512 else "4"))}
    try:
        ti.set_classes(cls, rows)
        ti.set_lik(None, rows, stride)
        flags = capi.CJ_FLAT | capi.CJ_DATA
        res["object_collapsed"] = timed(lambda r: ti.logjoint_collapsed(0.3, bpar, gamma=1.0, beta=0.5, flags=flags), reps)
        res["object_collapsed_without_data"] = timed(lambda r: ti.logjoint_collapsed(0.3, bpar, gamma=1.0, flags=capi.CJ_FLAT), reps)
        val, ci = ti.logjoint_collapsed(0.3, bpar, gamma=1.0, beta=0.5, flags=flags)
        cnt = ti.class_counts()
        d_cnt = torch.as_tensor(cnt.view(np.int32), device="cuda")
        res["raw_columns"] = timed(lambda r: capi.dirmult_logml(d_cnt, 0.5, capi.DM_COLUMNS, want_each=False), reps)
        res["nonzero"] = int(ci.dm_data.nonzero)
        res["hbm_floor_ms"] = 4.0 * rows * stride / HBM_BYTES_PER_S * 1e3
        res["data_value"] = ci.data
        if host_reps > 0:
            def host(r):
                res["host_value"] = host_logml(ti.class_counts(), 0.5, 0)

            res["host_route"] = timed(host, host_reps)
            res["host_over_raw"] = res["host_route"]["ms_median"] / res["raw_columns"]["ms_median"]
    finally:
        ti.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--tables", default="64:100,64:0,1024:100,1024:0")
    ap.add_argument("--data", default="S,L")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert capi.lib().stb_device_count() > 0, "no GPU: " + capi.last_error()
    out = []
    for spec in [s for s in args.tables.split(",") if s]:
        k, g = spec.split(":")
        out.append(run_tables(int(k), int(g), args.reps, args.host_reps))
        print(json.dumps(out[-1]), flush=True)
    for s in [s for s in args.data.split(",") if s]:
        out.append(run_data(s, args.reps, args.host_reps))
        print(json.dumps(out[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
