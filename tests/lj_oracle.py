"""High-precision truth and error bar of the log joint probability of a sampler state (libstb_amd/csrc/logjoint.hip,
include/stb_hip.h stb_logjoint; test infrastructure only).

    log p(n, t | a, b, h) = sum_i L_i,     L_i = P_i + H_i + R_i (+ B_i: the table-indicator representation)
    P_i = sum_k S_S_a(n_ik, t_ik)        H_i = sum_k t_ik log h_ik        B_i = -sum_k log C(n_ik - 1, t_ik - 1)
    R_i = log (b_i|a)_{T_i} - log (b_i)_{N_i}                              (0 where N_i = 0)

Truth
-----
The cells S_S(n, t) from hp_oracle.tables (x87 long double, pinned by exact_rows: tests/test_logjoint_host.py); R_i,
t log h and the binomials by mpmath at 40 digits from the exact doubles a, b_i, h; everything summed in mpmath.  A pair
is classified as the kernel classifies it: impossible (t = 0 with n > 0, t > n; h not positive and finite), outside
(n > N; 1 < t < n with t > M or without a table) or in.

The bar (u = 2^-53), from the kernel's own operations -- nothing here is fitted to what the kernel returns
-------------------------------------------------------------------------------------------------------
  * a gathered cell: hp.bar(n, a, y) for 1 < t < n, hp.s1bar(n, a, y) for t = 1 < n (the table's cell, or the same
    expression evaluated in the kernel when there is no S1 vector), 0 for t = n (an exact 0).
  * t log h: the device's log to 1 ulp and one product: 2 u |t log h|.
  * a binomial -((lgamma(n) - lgamma(t)) - lgamma(n - t + 1)): the arguments are exact integers, each lgamma to
    hp.L_LGAMMA ulp of its value, the two subtractions round once each: u (L (|lg n| + |lg t| + |lg(n-t+1)|) + |lg n -
    lg t| + |c|).
  * a chunk of 64 terms is summed by a six-level tree of plain additions; each level rounds by at most u times the
    magnitude of its partial sums, which the magnitudes of the chunk's terms bound: 6 u sum |terms|, per component.
  * the chunk sums are added in double-double (no first-order term); P_i, H_i, B_i = hi + lo round once each.
  * R_i: hp.term_bar over its terms and lgamma arguments -- a > 0: T log a, lgamma(T + b/a), lgamma(b/a), lgamma(b + N),
    lgamma(b) with arguments T + b/a, b/a, b + N, b (five terms, four arguments); a = 0: T log b, lgamma(b + N), lgamma(b)
    with arguments b + N, b; a > 0 and b = 0: (T - 1) log a, lgamma(T), lgamma(N), exact arguments.
  * L_i = ((P_i + H_i) + R_i) + B_i: four hi + lo roundings (u/2 |component| each) and three plain additions (u/2 times a
    partial sum each, every partial sum at most the components' magnitudes together): 2 u (|P_i| + |H_i| + |R_i| + |B_i|),
    and 16 u absolute.
  * a component's total over restaurants: the bars of its per-restaurant values; the block tree of 256 values has eight
    levels of plain additions: 8 u sum_i |value_i|; the blocks are added in double-double and hi + lo rounds once, the
    truth is rounded to a double for the comparison: 2 u |total| + 16 u.
  * the total merges the four double-doubles and rounds once: the four components' bars without their own last
    2 u |.| + 16 u, and 2 u |total| + 16 u.
"""
from __future__ import annotations

import math
import os
import sys
from functools import lru_cache

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import hp_oracle as hp  # noqa: E402

LD = np.longdouble
U = hp.U
NEG_INF = -math.inf


def _mpf(x):
    """a long double (or double) as an mpf, exactly"""
    mp = hp._mp()
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(LD(x) - LD(hi)))


@lru_cache(maxsize=None)
def _lgi(k: int):
    return hp._mp().loggamma(k)


class Tables:
    """the truth's cells for discount a with bounds (N, M), hp_oracle's packed order; with_table False: no slab and no
    S1 vector are given to the kernel (S^n_1 is then evaluated in place, interior cells are outside)"""

    def __init__(self, a: float, N: int, M: int, with_table: bool = True, S1=None, S=None):
        self.a, self.N, self.M, self.with_table = float(a), int(N), int(M), with_table
        if S1 is None:
            S1, S, _ = hp.tables([a], max(N, 3), M)[0]
        self.S1, self.S = S1, S

    def cell(self, n: int, t: int):
        """(value, bar) of S_S(n, t) for 1 <= t <= n <= N, t <= M unless t = n"""
        if t == n:
            return LD(0), 0.0
        if t == 1:
            y = self.S1[n - 1]
            return y, float(hp.s1bar(n, self.a, float(y)))
        y = self.S[hp._s_rowoff(n, self.M) + t - 2]
        return y, float(hp.bar(n, self.a, float(y)))


def classify(n: int, t: int, h, tabs: Tables) -> str:
    """'zero' (n = 0, t = 0), 'imp_p', 'out', 'imp_h' or 'in' -- the kernel's order of tests"""
    if n == 0:
        return "zero" if t == 0 else "imp_p"
    if t == 0 or t > n:
        return "imp_p"
    if n > tabs.N:
        return "out"
    if 1 < t < n and (t > tabs.M or not tabs.with_table):
        return "out"
    if h is not None and not (h > 0.0 and math.isfinite(h)):
        return "imp_h"
    return "in"


def pair_terms(n: int, t: int, h, tabs: Tables, indicators: bool):
    """((p, q, c) as mpf, (bar_p, bar_q, bar_c)) of a pair that is 'in'"""
    mp = hp._mp()
    y, bp = tabs.cell(n, t)
    p = _mpf(y)
    q, bq = mp.mpf(0), 0.0
    if h is not None:
        q = t * mp.log(mp.mpf(float(h)))
        bq = 2.0 * U * abs(float(q))
    c, bc = mp.mpf(0), 0.0
    if indicators and t != n and t != 1:
        l1, l2, l3 = _lgi(n), _lgi(t), _lgi(n - t + 1)
        c = -((l1 - l2) - l3)
        bc = U * (hp.L_LGAMMA * (abs(float(l1)) + abs(float(l2)) + abs(float(l3))) + abs(float(l1 - l2)) + abs(float(c)))
    return (p, q, c), (bp, bq, bc)


def restaurant_term(a: float, b: float, T: int, N: int):
    """(R_i as mpf, bar)"""
    mp = hp._mp()
    if N == 0:
        return mp.mpf(0), 0.0
    am, bm = mp.mpf(float(a)), mp.mpf(float(b))
    if a > 0.0 and b != 0.0:
        z = bm / am
        t1 = T * mp.log(am)
        t2, t3 = mp.re(mp.loggamma(T + z)), mp.re(mp.loggamma(z))
        t4, t5 = mp.re(mp.loggamma(bm + N)), mp.re(mp.loggamma(bm))
        return (t1 + (t2 - t3)) - (t4 - t5), hp.term_bar([t1, t2, t3, t4, t5], [T + z, z, bm + N, bm])
    if a > 0.0:
        if T == 0:
            return mp.mpf(0), 0.0
        t1, t2, t3 = (T - 1) * mp.log(am), _lgi(T), _lgi(N)
        return (t1 + t2) - t3, hp.term_bar([t1, t2, t3], [])
    t1 = T * mp.log(bm)
    t4, t5 = mp.loggamma(bm + N), mp.loggamma(bm)
    return t1 - (t4 - t5), hp.term_bar([t1, t4, t5], [bm + N, bm])


def per_restaurant(K, n, t, h, a: float, bpar, tabs: Tables, indicators: bool = False):
    """what truth() sums, restaurant by restaurant: a dict of Li, Li_bar, T, Nc, P_ld, P_bar [I] as truth() returns them and
    comp, cbar [I][4] (P, H, R, B as mpf; their bars), out, imp_p, imp_h [I] (the restaurant's counts)"""
    mp = hp._mp()
    K = np.asarray(K, dtype=np.int64)
    I = K.shape[0]
    koff = np.concatenate([[0], np.cumsum(K)]).astype(np.int64)
    bpar = np.broadcast_to(np.asarray(bpar, dtype=np.float64), (I,))
    Li, Li_bar = np.zeros(I), np.zeros(I)
    Ts, Ns = np.zeros(I, dtype=np.int64), np.zeros(I, dtype=np.int64)
    P_ld, P_bar = np.zeros(I, dtype=LD), np.zeros(I)   # P_i in long double, and the sum of its cells' bars
    comps, cbars = [], []
    counts = np.zeros((3, I), dtype=np.int64)           # outside, impossible (S), impossible (h)
    for i in range(I):
        comp = [mp.mpf(0)] * 4
        cbar = [0.0] * 4
        for j0 in range(koff[i], koff[i + 1], 64):
            mags = [0.0, 0.0, 0.0]
            for g in range(j0, min(j0 + 64, koff[i + 1])):
                ng, tg = int(n[g]), int(t[g])
                hg = None if h is None else float(h[g])
                Ts[i] += tg
                Ns[i] += ng
                kind = classify(ng, tg, hg, tabs)
                if kind == "imp_p":
                    counts[1, i] += 1
                elif kind == "imp_h":
                    counts[2, i] += 1
                elif kind == "out":
                    counts[0, i] += 1
                elif kind == "in":
                    vals, bars = pair_terms(ng, tg, hg, tabs, indicators)
                    P_ld[i] += tabs.cell(ng, tg)[0]
                    P_bar[i] += bars[0]
                    for c, slot in enumerate((0, 1, 3)):
                        comp[slot] += vals[c]
                        cbar[slot] += bars[c]
                        mags[c] += abs(float(vals[c]))
            for c, slot in enumerate((0, 1, 3)):
                cbar[slot] += 6.0 * U * mags[c]
        comp[2], cbar[2] = restaurant_term(a, float(bpar[i]), int(Ts[i]), int(Ns[i]))
        absum = sum(abs(float(x)) for x in comp)
        bad = counts[1, i] + counts[2, i] > 0
        Li[i] = NEG_INF if bad else float(comp[0] + comp[1] + comp[2] + comp[3])
        Li_bar[i] = sum(cbar) + U * (2.0 * absum + 16.0)
        comps.append(comp)
        cbars.append(cbar)
    return {"Li": Li, "Li_bar": Li_bar, "T": Ts, "Nc": Ns, "P_ld": P_ld, "P_bar": P_bar, "comp": comps, "cbar": cbars,
            "out": counts[0], "imp_p": counts[1], "imp_h": counts[2]}


def tiled(per, mult=None):
    """the totals, their bars and the counts of a state in which restaurant i of `per` (per_restaurant's dict) occurs
    mult[i] times (None: once): sums over the types of multiplicity x value, bars sums of multiplicity x the type's bar --
    every per-restaurant term of the bar is linear in the restaurants, the block tree's 8 u sum_i |value_i| included; the
    double-double terms 2 u |total| + 16 u are taken once, on the tiled totals.  Returns truth()'s dict (Li, Li_bar, T,
    Nc, P_ld, P_bar stay per type)."""
    mp = hp._mp()
    I = len(per["comp"])
    mult = np.ones(I, dtype=np.int64) if mult is None else np.asarray(mult, dtype=np.int64)
    assert mult.shape == (I,) and (mult >= 0).all()
    tot = [mp.mpf(0)] * 4          # P, H, R, B
    tot_bar = [0.0] * 4            # the per-restaurant bars
    tot_abs = [0.0] * 4            # sum_i |value_i|: the block tree
    for i in range(I):
        m = int(mult[i])
        comp, cbar = per["comp"][i], per["cbar"][i]
        for c in range(4):
            tot[c] += m * comp[c]
            tot_bar[c] += m * (cbar[c] + U * abs(float(comp[c])))   # (hi + lo of the restaurant's sum, where it has one)
            tot_abs[c] += m * abs(float(comp[c]))
    outside, imp_p, imp_h = (int((mult * per[k]).sum()) for k in ("out", "imp_p", "imp_h"))
    out = {k: per[k] for k in ("Li", "Li_bar", "T", "Nc", "P_ld", "P_bar")}
    out.update({"outside": outside, "impossible": imp_p + imp_h})
    inner = [tot_bar[c] + 8.0 * U * tot_abs[c] for c in range(4)]
    for c, name in enumerate(("pairs", "base", "restaurants", "binom")):
        v = float(tot[c])
        if (name == "pairs" and imp_p) or (name == "base" and imp_h):
            v = NEG_INF
        out[name] = (v, inner[c] + U * (2.0 * abs(float(tot[c])) + 16.0))
    total = tot[0] + tot[1] + tot[2] + tot[3]
    out["total"] = (NEG_INF if imp_p or imp_h else float(total), sum(inner) + U * (2.0 * abs(float(total)) + 16.0))
    out["total_mp"] = total
    return out


def truth(K, n, t, h, a: float, bpar, tabs: Tables, indicators: bool = False, mult=None):
    """the truth and the bars of every output of stb_logjoint on the CSR state (K, n, t, h or None); mult (None: all 1):
    restaurant i stands for mult[i] restaurants with its pairs and its b_i (tiled()).  A dict:
      Li, Li_bar [I] (doubles; -inf where the restaurant holds an impossible pair), T, Nc [I] (the integer sums),
      P_ld, P_bar [I]: P_i summed in long double and the sum of its cells' bars,
      pairs, base, restaurants, binom, total: (value, bar) each (value -inf as the kernel defines it),
      outside, impossible: counts."""
    return tiled(per_restaurant(K, n, t, h, a, bpar, tabs, indicators), mult)


def within(got, want, bar) -> bool:
    """|got - want| <= bar, equal infinities agreeing; never true for a NaN"""
    if math.isinf(want) or math.isinf(got):
        return got == want
    return abs(got - want) <= bar
