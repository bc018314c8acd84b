"""A numpy replay of the Dirichlet concentration step (libstb_amd/csrc/dirconc.hip; include/stb_hip.h stb_sample_dirconc),
written from the header's text on hh_oracle's auxiliary tables, hb_oracle's step and dm_oracle's weight total, and the law
it is checked against.

  key = mix(seed + (sweep+1) gamma); cell e = mu cols + j (rows) or j stride + mu (columns) owns mix(key + (e+1) gamma)
  n_mu   the multinomial's total;  V = sum v in dirmult's association (scale 1)
  m      hh_oracle.aux_tables with w = s v_j at the cell's own flat index;  M_mu = sum_j m
  B'     hb_oracle.replay(a = 0, shape, scale V, T = M, N = n, every b = s V, one group) on seed ^ SALT_A
  s'     B' / V
The replay reports the smallest margin of the Gamma acceptance tests and of the Bernoulli comparisons.  Three wrong laws
are kept for the tests of the law's power: "no_first" drops the [c >= 1] table, "no_q" leaves q undrawn (L = 0),
"no_V" leaves V out of the prior's scale.
"""
import math

import numpy as np

import dm_oracle as dmo
import hb_oracle as hbo
import hh_oracle as hho

ROWS, COLUMNS = 1, 2
LAWS = ("right", "no_first", "no_q", "no_V")
MASK = (1 << 64) - 1


def weights(v, ncat):
    """(v[ncat], V as k_dm_weights forms it with scale 1)"""
    return dmo.weights_of(v, ncat, 1.0)


def replay(cnt, v, s, shape, scale, seed, sweep, orientation, cols=None, law="right"):
    """the whole step on cnt (rows, stride), its first `cols` columns the matrix: dict with s (s'), m (rows, stride; 0 in
    the padding), M, n (one per multinomial), count, aux_tables, nonempty, V, margin_gamma, margin_y"""
    cnt = np.asarray(cnt).astype(np.int64)
    rows, stride = cnt.shape
    cols = stride if cols is None else cols
    c = cnt[:, :cols]
    by_rows = orientation == ROWS
    vv, V = weights(v, cols if by_rows else rows)
    w = float(s) * vv
    m = np.zeros((rows, stride), dtype=np.int64)
    if by_rows:
        mm, my = hho.aux_tables(c, w, seed, sweep, "no_first" if law == "no_first" else "right")
        m[:, :cols] = mm
        n, M = c.sum(axis=1), mm.sum(axis=1)
    else:
        cz = cnt.copy()
        cz[:, cols:] = 0                                  # (the flat index runs over the stride; the padding draws nothing)
        m, my = hho.aux_tables(cz, np.repeat(w[:, None], stride, axis=1), seed, sweep, "no_first" if law == "no_first" else "right")
        n, M = c.sum(axis=0), m[:, :cols].sum(axis=0)
    nm = len(n)
    B = float(s) * V
    scale_B = float(scale) if law == "no_V" else float(scale) * V
    N = np.zeros(nm, dtype=np.uint32) if law == "no_q" else n.astype(np.uint32)
    hb = hbo.replay(0.0, shape, scale_B, M.astype(np.uint32), N, np.full(nm, B), np.array([0, nm], dtype=np.int64),
                    (seed ^ hho.SALT_A) & MASK, sweep)
    return dict(s=float(hb["bgrp"][0]) / V, m=m, M=M, n=n, count=int(n.sum()), aux_tables=int(M.sum()),
                nonempty=int((n > 0).sum()), V=V, margin_gamma=hb["margin_gamma"], margin_y=min(my, hb["margin_y"]))


# ---- the law: p(s | c) ~ s^(shape-1) e^(-s/scale) prod_mu Gamma(sV) / Gamma(sV + n_mu) prod_j Gamma(s v_j + c) / Gamma(s v_j)

_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


class Posterior:
    """the posterior of s by quadrature in u = log s (trapezoid on a fine grid), with its CDF"""

    def __init__(self, c, v, shape, scale, points=60001):
        c = np.asarray(c, dtype=np.int64)                 # (multinomials, categories)
        v = np.broadcast_to(np.asarray(v, dtype=np.float64), (c.shape[1],))
        V = float(v.sum())
        u = np.linspace(-40.0, 12.0, points)
        s = np.exp(u)
        lp = shape * u - s / scale                        # (the Jacobian s of u = log s turns shape - 1 into shape)
        for row in c:
            if row.sum() > 0:
                lp = lp + _lgamma(s * V) - _lgamma(s * V + float(row.sum()))
            for vj, cj in zip(v, row):
                for i in range(int(cj)):                  # Gamma(w + c) / Gamma(w) = prod_i (w + i)
                    lp = lp + np.log(s * vj + i)
        lp -= lp.max()
        dens = np.exp(lp)
        cdf = np.concatenate([[0.0], np.cumsum(0.5 * (dens[1:] + dens[:-1]) * np.diff(u))])
        self.u, self.cdf = u, cdf / cdf[-1]

    def F(self, s):
        return np.interp(np.log(np.asarray(s, dtype=np.float64)), self.u, self.cdf)


# the fixtures of the law tests.  3 x 2: three multinomials (rows) over two categories, V = 1.5; one row over four, V = 4
LAW_FIX = {
    "3x2": dict(cnt=np.array([[5, 1], [0, 9], [2, 2]], dtype=np.uint32), v=np.array([0.5, 1.0]), shape=2.0, scale=1.5),
    "1row": dict(cnt=np.array([[4, 0, 7, 1]], dtype=np.uint32), v=1.0, shape=1.5, scale=2.0),
}
LAW_SEED = {"3x2": 5201, "1row": 5202}    # test_dirconc_host checks these chains on the CPU; test_gpu_dirconc runs 3x2's on the device
LAW_STEPS, LAW_BURN, LAW_THIN = 5900, 100, 5          # 6000 calls: the cap of the device test
WRONG_STEPS = 2000                                     # the wrong laws are far off: a shorter chain rejects them


def chain(fix, seed, law="right", steps=LAW_STEPS, burn=LAW_BURN, thin=LAW_THIN, step_fn=None):
    """s of the step iterated on a fixture from s = 1, sweeps 0, 1, ...: the kept values (after `burn`, every `thin`-th).
    step_fn(s, sweep) -> s' replaces the replay (the device)"""
    f = LAW_FIX[fix]
    s = 1.0
    kept = []
    for t in range(burn + steps):
        if step_fn is None:
            s = replay(f["cnt"], f["v"], s, f["shape"], f["scale"], seed, t, ROWS, law=law)["s"]
        else:
            s = step_fn(s, t)
        if t >= burn and (t - burn) % thin == 0:
            kept.append(s)
    return np.array(kept)


def law_pvalue(fix, kept):
    f = LAW_FIX[fix]
    return hbo.ks_pvalue(Posterior(f["cnt"], f["v"], f["shape"], f["scale"]).F(kept))


# ---- the replay cases of tests/test_gpu_dirconc.py; tests/test_dirconc_host.py checks every one's margins on the CPU ----

GARBAGE = 0xDEADBEEF
_COUNTS = np.array([0, 0, 0, 0, 1, 2, 3, 40, 300], dtype=np.uint32)      # (300: past HG_TWAVE, a wave's cell)
CASES = {
    # name: (orientation, rows, cols, stride, v: "vec" or a scalar, seed, sweep)
    "cols_3_2": (COLUMNS, 3, 2, 2, "vec", 6101, 0),
    "cols_257_7": (COLUMNS, 257, 7, 7, 0.5, 6102, 3),
    "cols_3_65": (COLUMNS, 3, 65, 65, "vec", 6103, 1),
    "cols_300_70_96": (COLUMNS, 300, 70, 96, "vec", 6104, 7),
    "cols_big": (COLUMNS, 2, 1, 1, "vec", 6105, 2),
    "cols_cells": (COLUMNS, 3, 6, 6, "vec", 6106, 4),
    "rows_1_5": (ROWS, 1, 5, 5, "vec", 6111, 0),
    "rows_3_2": (ROWS, 3, 2, 2, "vec", 6112, 5),
    "rows_513_3": (ROWS, 513, 3, 3, 0.25, 6113, 1),
    "rows_2_1024": (ROWS, 2, 1024, 1024, "vec", 6114, 2),
    "rows_big": (ROWS, 1, 1, 1, "vec", 6115, 9),
}
COL_CASES = [n for n in CASES if CASES[n][0] == COLUMNS]
ROW_CASES = [n for n in CASES if CASES[n][0] == ROWS]
CELL_C = (0, 1, 2, 257, 258, 65535)
CELL_V = (1e-3, 1.0, 1e3)


def case(name):
    """dict(cnt (rows, stride) uint32 with garbage in the padding, cols, v, s, shape, scale, seed, sweep, orientation)"""
    orientation, rows, cols, stride, v, seed, sweep = CASES[name]
    rng = np.random.default_rng(seed)
    cnt = np.full((rows, stride), GARBAGE, dtype=np.uint32)
    cnt[:, :cols] = rng.choice(_COUNTS, size=(rows, cols))
    ncat = cols if orientation == ROWS else rows
    if v == "vec":
        v = 0.2 + 2.0 * rng.random(ncat)
    if name == "cols_3_2":
        cnt[:, :] = LAW_FIX["3x2"]["cnt"]
    elif name == "cols_big":
        cnt[:, 0] = (100000, 3)
    elif name == "cols_cells":
        cnt[:, :] = np.array(CELL_C, dtype=np.uint32)[None, :]
        v = np.array(CELL_V)
    elif name == "rows_big":
        cnt[0, 0] = 300000
    elif name == "cols_300_70_96":
        cnt[:, 5] = 0                                   # an empty multinomial
    return dict(cnt=cnt, cols=cols, v=v, s=0.5 + 2.0 * rng.random(), shape=1.5, scale=4.0, seed=seed, sweep=sweep,
                orientation=orientation)


def replay_case(name, **kw):
    c = case(name)
    return replay(c["cnt"], c["v"], c["s"], c["shape"], c["scale"], c["seed"], c["sweep"], c["orientation"], c["cols"], **kw)
