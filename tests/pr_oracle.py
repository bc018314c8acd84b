"""Replay, high-precision truth and error bars of the predictive dish proportions and the held-out log likelihood
(libstb_amd/csrc/predict.hip; include/stb_hip.h "what a state predicts"; test infrastructure only).

    theta_ik = ((n_k - t_k a) + g_i h_k) / (b_i + N_i),  g_i = b_i + T_i a        p_c = sum_k theta_ik lik[cls_c, k]
    H_i = sum_c log(p_c / S)                                                       total = sum_i H_i

Replay (numpy float64, one ufunc an operation: no contraction) -- written from the header's text
------------------------------------------------------------------------------------------------
  T_i, N_i integer sums; g = b + T * a; den = b + N; x = n - t * a; theta = (x + g * h) / den; N_i = 0: theta = h.
  q_k = theta_k * L_k, L = 0 for a class >= rows, 1 without a matrix, +0.0 past K_i.  Dishes in blocks of 64 on an array
  padded to a multiple of 64; a block by the six explicit steps of the 64-lane tree (tree64); p = s_0, then p + s_j in
  block order.  x_c = log(p_c / S) (numpy's log: the device's is its own, so H_i and the total are compared within the bar,
  theta and p bit for bit); a restaurant's chunks of 64 through tree64, the chunk sums by dd_add in order, H_i = hi + lo;
  restaurants in blocks of 256 by block_tree, the block sums by dd_add in order.

Truth: mpmath at 40 digits from the exact doubles.

The bars (u = 2^-53), from the operations -- nothing here reads a device result
-------------------------------------------------------------------------------
  theta, absolutely, first order in u (times 1 + 2^-20 for the rest):
      x = n - fl(t a):      e_x = u (|t a| + |x|)          (the one cancellation: e_x / x <= u / (1 - a))
      g = b + fl(T a):      e_g = u (|T a| + |g|)          (b >= 0: <= 2 u g; -a < b < 0 cancels once more)
      g h:                  e_gh = e_g h + u |g h|
      x + g h:              e_num = e_x + e_gh + u |x + g h|
      den = b + N:          u |den|;    the division: u |theta|
      bar(theta) = |theta| (e_num / |num| + 2 u).  For b >= 0 this is at most u (4 + max(1 / (1 - a), 3)) |theta|.
  p: every product rounds once, a block's tree has six levels, the blocks are added one after another:
      bar(p) = sum_k bar(theta_k) L_k + u (1 + 6 + blocks) sum_k |q_k|
  an accumulator over S states: the states' bars and u (S - 1) acc.
  x = log(p / S): the quotient rounds once, the relative error of the argument is an absolute one of the log, and the
      log itself is good to one ulp (<= 2 u |x|):  bar(x) = bar(p) / p + u + 2 u |x|
  H_i: sum_c bar(x_c) + 6 u sum_c |x_c| (the chunk tree; the chunk sums are added in double-double) + u |H_i| (hi + lo).
  total: sum_i bar(H_i) + 8 u sum_i |H_i| (the block tree of 256: eight levels) + u (2 |total| + 16), as lj_oracle.tiled.
"""
from __future__ import annotations

import math
import os
import sys
from functools import lru_cache

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hp_oracle as hp  # noqa: E402

U = hp.U
NEG_INF = -math.inf
MAXK = 1024     # STB_TD_MAXK
SLACK = 1.0 + 2.0 ** -20


# ---------------------------------------------------------------------------------------------------- the pieces

def tree64(v, linear: bool = False):
    """the 64-lane shuffle tree on the last axis (length 64): v[l] += v[l + o], o = 32, 16, .. 1; lane 0.  linear: the
    wrong association, left to right (for the tests that show the replay can fail)"""
    v = np.array(v, dtype=np.float64)
    assert v.shape[-1] == 64
    if linear:
        s = v[..., 0].copy()
        for l in range(1, 64):
            s = s + v[..., l]
        return s
    v = v[..., 0:32] + v[..., 32:64]   # o = 32
    v = v[..., 0:16] + v[..., 16:32]   # o = 16
    v = v[..., 0:8] + v[..., 8:16]     # o = 8
    v = v[..., 0:4] + v[..., 4:8]      # o = 4
    v = v[..., 0:2] + v[..., 2:4]      # o = 2
    v = v[..., 0:1] + v[..., 1:2]      # o = 1
    return v[..., 0]


def dd_add(hi, lo, x):
    """stb_common.h's dd_add on arrays: (hi, lo) += x"""
    with np.errstate(invalid="ignore", over="ignore"):
        t = hi + x
        bb = t - hi
        corr = (hi - (t - bb)) + (x - bb)
    lo = np.where(np.isfinite(t), lo + np.where(np.isfinite(t), corr, 0.0), lo)
    return t, lo


def block_tree(x):
    """k_logjoint's tree over a block of 256 values (last axis): (x[l] + x[l+64]) + (x[l+128] + x[l+192]), then tree64"""
    x = np.asarray(x, dtype=np.float64)
    assert x.shape[-1] == 256
    return tree64((x[..., 0:64] + x[..., 64:128]) + (x[..., 128:192] + x[..., 192:256]))


def ordered_dd_sum(v):
    """the values of the last axis added in order in double-double; hi + lo"""
    v = np.asarray(v, dtype=np.float64)
    hi, lo = np.zeros(v.shape[:-1]), np.zeros(v.shape[:-1])
    for j in range(v.shape[-1]):
        hi, lo = dd_add(hi, lo, v[..., j])
    return hi + lo


# ---------------------------------------------------------------------------------------------------- the replay

def skipped_mask(K, stride=None, tstride=None):
    K = np.asarray(K, dtype=np.int64)
    m = K > MAXK
    if stride is not None:
        m |= K > stride
    if tstride is not None:
        m |= K > tstride
    return m


def theta_replay(K, n, t, h, a, bpar, tstride=None, stride=None, mut=None):
    """theta as an (I, KP) array, KP = the largest K padded to a multiple of 64 (and at least tstride): +0.0 past K_i and
    on skipped rows.  mut: 't+1' or 'noTa', the wrong replays"""
    K = np.asarray(K, dtype=np.int64)
    I = K.shape[0]
    koff = np.concatenate([[0], np.cumsum(K)]).astype(np.int64)
    bpar = np.broadcast_to(np.asarray(bpar, dtype=np.float64), (I,))
    skip = skipped_mask(K, stride, tstride)
    Kmax = int(K[~skip].max()) if (~skip).any() else 1
    KP = 64 * max(1, -(-max(Kmax, tstride or 0) // 64))
    col = np.arange(KP)
    live = (col[None, :] < K[:, None]) & ~skip[:, None]
    idx = np.where(live, koff[:-1, None] + col[None, :], 0)
    n64 = np.where(live, np.asarray(n, dtype=np.int64)[idx] if len(n) else 0, 0)
    t64 = np.where(live, np.asarray(t, dtype=np.int64)[idx] if len(t) else 0, 0)
    hh = np.where(live, np.asarray(h, dtype=np.float64)[idx], 1.0) if h is not None else np.ones((I, KP))
    Ti, Ni = t64.sum(axis=1), n64.sum(axis=1)          # the kernel's own integer sums
    if mut == "t+1":
        t64 = t64 + 1
    a = np.float64(a)
    T, N = Ti.astype(np.float64), Ni.astype(np.float64)
    g = bpar + T * a if mut != "noTa" else bpar + 0.0
    den = bpar + N
    x = n64.astype(np.float64) - t64.astype(np.float64) * a
    with np.errstate(divide="ignore", invalid="ignore"):
        th = (x + g[:, None] * hh) / den[:, None]
    th = np.where((Ni == 0)[:, None], hh, th)
    return np.where(live, th, 0.0), Ti, Ni


def p_replay(theta, K, hoff, hcls, lik, rows=None, stride=None, tstride=None, mut=None):
    """p[Hc] of one state from theta_replay's array; skipped restaurants' customers get 0.  mut: 'linear' (a block left to
    right) or 'reverse' (the block sums last to first)"""
    K = np.asarray(K, dtype=np.int64)
    hoff = np.asarray(hoff, dtype=np.int64)
    Hc = int(hoff[-1])
    KP = theta.shape[1]
    rest = np.repeat(np.arange(K.shape[0]), np.diff(hoff))
    hcls = np.asarray(hcls, dtype=np.int64)[:Hc]
    skip = skipped_mask(K, stride, tstride)
    col = np.arange(KP)
    live = (col[None, :] < K[rest][:, None]) & ~skip[rest][:, None]
    if lik is None:
        L = np.ones((Hc, KP))
    else:
        lik = np.asarray(lik, dtype=np.float64)
        rows = lik.shape[0] if rows is None else rows
        W = min(KP, lik.shape[1])
        L = np.zeros((Hc, KP))
        ok = hcls < rows
        L[ok, :W] = lik[hcls[ok], :W]
    q = np.where(live, theta[rest] * np.where(live, L, 0.0), 0.0)
    nb = KP // 64
    s = tree64(q.reshape(Hc, nb, 64), linear=(mut == "linear"))         # (Hc, nb)
    nbi = np.maximum(1, -(-K[rest] // 64))                               # the restaurant's own blocks
    if mut == "reverse":
        p = np.zeros(Hc)
        first = np.ones(Hc, dtype=bool)
        for j in range(nb - 1, -1, -1):
            use = j < nbi
            p = np.where(use, np.where(first, s[:, j], p + s[:, j]), p)
            first &= ~use
    else:
        p = s[:, 0].copy()
        for j in range(1, nb):
            p = np.where(j < nbi, p + s[:, j], p)
    return np.where(skip[rest], 0.0, p), q


def heldout_replay(p, hoff, samples=1):
    """(H_i [I] with -inf where a customer is impossible, total, impossible customers) from p as the kernel sums it"""
    hoff = np.asarray(hoff, dtype=np.int64)
    I = hoff.shape[0] - 1
    p = np.asarray(p, dtype=np.float64)
    cnt = np.diff(hoff)
    with np.errstate(divide="ignore", invalid="ignore"):
        qv = p / np.float64(samples)
        ok = (qv > 0.0) & np.isfinite(p)
        x = np.where(ok, np.log(np.where(ok, qv, 1.0)), 0.0)
    nch = max(1, int(-(-cnt.max() // 64))) if I else 1
    pad = np.zeros((I, nch * 64))
    rest = np.repeat(np.arange(I), cnt)
    pos = np.arange(p.shape[0]) - hoff[:-1][rest]
    pad[rest, pos] = x
    Hsum = ordered_dd_sum(tree64(pad.reshape(I, nch, 64)))      # extra chunks add +0.0 in double-double: nothing
    bad = np.zeros(I, dtype=bool)
    np.logical_or.at(bad, rest, ~ok)
    nblk = max(1, -(-I // 256))
    full = np.zeros(nblk * 256)
    full[:I] = Hsum
    total = float(ordered_dd_sum(block_tree(full.reshape(nblk, 256))))
    nimp = int((~ok).sum())
    return np.where(bad, NEG_INF, Hsum), (NEG_INF if nimp else total), nimp


def replay(K, n, t, h, a, bpar, hoff=None, hcls=None, lik=None, rows=None, stride=None, tstride=None, mut=None):
    """everything stb_predict_dishes + stb_heldout_loglik (samples = 1) give on one state: a dict of theta (I, KP), p, Hi,
    total, impossible, skipped"""
    theta, _, _ = theta_replay(K, n, t, h, a, bpar, tstride, stride if lik is not None else None, mut)
    out = {"theta": theta, "skipped": int(skipped_mask(K, stride if lik is not None else None, tstride).sum())}
    if hoff is not None:
        p, _ = p_replay(theta, K, hoff, hcls, lik, rows, stride if lik is not None else None, tstride, mut)
        Hi, total, nimp = heldout_replay(p, hoff, 1)
        out.update({"p": p, "Hi": Hi, "total": total, "impossible": nimp})
    return out


# ---------------------------------------------------------------------------------------------------- truth and bars

def truth(K, n, t, h, a, bpar, hoff=None, hcls=None, lik=None, samples_of=None):
    """mpmath truth and the bars of one state (no skipped restaurants; every class < rows).  A dict: theta, theta_bar as
    (I, Kmax) float arrays (the truth rounded), theta_sum [I] (mpf), and with hoff: p, p_bar [Hc], Hi, Hi_bar [I], total,
    total_bar.  Customers with p = 0 make H_i and the total -inf."""
    mp = hp._mp()
    K = np.asarray(K, dtype=np.int64)
    I = K.shape[0]
    koff = np.concatenate([[0], np.cumsum(K)]).astype(np.int64)
    bpar = np.broadcast_to(np.asarray(bpar, dtype=np.float64), (I,))
    am = mp.mpf(float(a))
    Kmax = int(K.max())
    th_f, th_bar = np.zeros((I, Kmax)), np.zeros((I, Kmax))
    th_mp, sums = [], []
    for i in range(I):
        k0, k1 = int(koff[i]), int(koff[i + 1])
        Ti, Ni = int(np.asarray(t[k0:k1], dtype=np.int64).sum()), int(np.asarray(n[k0:k1], dtype=np.int64).sum())
        bm = mp.mpf(float(bpar[i]))
        g, den = bm + Ti * am, bm + Ni
        row = []
        for k in range(k1 - k0):
            hk = mp.mpf(float(h[k0 + k])) if h is not None else mp.mpf(1)
            nk, tk = int(n[k0 + k]), int(t[k0 + k])
            if Ni == 0:
                th, bar = hk, 0.0
            else:
                x = nk - tk * am
                num = x + g * hk
                th = num / den
                e_x = U * (abs(float(tk * am)) + abs(float(x)))
                e_g = U * (abs(float(Ti * am)) + abs(float(g)))
                e_num = e_x + e_g * float(hk) + U * abs(float(g * hk)) + U * abs(float(num))
                bar = abs(float(th)) * (e_num / abs(float(num)) + 2.0 * U) * SLACK if num != 0 else 0.0
            row.append(th)
            th_f[i, k], th_bar[i, k] = float(th), bar
        th_mp.append(row)
        sums.append(mp.fsum(row))
    out = {"theta": th_f, "theta_bar": th_bar, "theta_sum": sums}
    if hoff is None:
        return out
    hoff = np.asarray(hoff, dtype=np.int64)
    Hc = int(hoff[-1])
    p_f, p_bar = np.zeros(Hc), np.zeros(Hc)
    Hi, Hi_bar = np.zeros(I), np.zeros(I)
    x_mp_tot, tot_bar, tot_abs, any_imp = mp.mpf(0), 0.0, 0.0, False
    likm = {}
    for i in range(I):
        Ki, nb = int(K[i]), max(1, -(-int(K[i]) // 64))
        Hm, bars, mags, imp = mp.mpf(0), 0.0, 0.0, False
        for c in range(int(hoff[i]), int(hoff[i + 1])):
            w = int(hcls[c])
            if lik is None:
                Lrow = None
                pm = sums[i]
                pb = float(th_bar[i, :Ki].sum()) + U * (7 + nb) * float(pm)
            else:
                if w not in likm:
                    likm[w] = [mp.mpf(float(v)) for v in lik[w]]
                Lrow = likm[w]
                pm = mp.fdot(th_mp[i], Lrow[:Ki])
                pb = float(np.dot(th_bar[i, :Ki], lik[w, :Ki])) + U * (7 + nb) * float(pm)   # (every q >= 0: sum |q| = p)
            p_f[c], p_bar[c] = float(pm), pb * SLACK
            if pm > 0:
                xm = mp.log(pm)
                Hm += xm
                bars += pb * SLACK / float(pm) + U + 2.0 * U * abs(float(xm))
                mags += abs(float(xm))
            else:
                imp = True
        Hi[i] = NEG_INF if imp else float(Hm)
        Hi_bar[i] = bars + 6.0 * U * mags + U * abs(float(Hm))
        x_mp_tot += Hm
        tot_bar += Hi_bar[i]
        tot_abs += abs(float(Hm))
        any_imp |= imp
    out.update({"p": p_f, "p_bar": p_bar, "Hi": Hi, "Hi_bar": Hi_bar,
                "total": NEG_INF if any_imp else float(x_mp_tot),
                "total_bar": tot_bar + 8.0 * U * tot_abs + U * (2.0 * abs(float(x_mp_tot)) + 16.0)})
    return out


def acc_bars(ps, pbars, hoff):
    """the bars of the running estimate over the states ps[s] (their bars pbars[s]): (acc_bar [Hc], Hi_bar [I], total_bar),
    the values taken from the arrays given -- S accumulating calls add in call order: u (S - 1) acc on top of the states'"""
    S = len(ps)
    acc = np.zeros_like(ps[0])
    for q in ps:
        acc = acc + q
    abar = sum(pbars) + U * (S - 1) * acc
    with np.errstate(divide="ignore"):
        x = np.log(acc / S)
    xbar = abar / acc + U + 2.0 * U * np.abs(x)
    hoff = np.asarray(hoff, dtype=np.int64)
    I = hoff.shape[0] - 1
    Hb, tot_abs, tot = np.zeros(I), 0.0, 0.0
    for i in range(I):
        sl = slice(int(hoff[i]), int(hoff[i + 1]))
        Hsum = math.fsum(x[sl])
        Hb[i] = float(xbar[sl].sum()) + 6.0 * U * float(np.abs(x[sl]).sum()) + U * abs(Hsum)
        tot_abs += abs(Hsum)
        tot += Hsum
    return abar, Hb, float(Hb.sum()) + 8.0 * U * tot_abs + U * (2.0 * abs(tot) + 16.0)


def within(got, want, bar) -> bool:
    """|got - want| <= bar, equal infinities agreeing; never true for a NaN"""
    if math.isinf(want) or math.isinf(got):
        return got == want
    return abs(got - want) <= bar


# ---------------------------------------------------------------------------------------------------- the cases

RAW_A = (0.0, 0.5, 0.999)
RAW_K = (1, 2, 63, 64, 65, 128, 130, 1024, 64, 65, 130, 2)
RAW_HC = (1, 63, 64, 300, 65, 129, 64, 63, 65, 1, 0, 129)
RAW_ROWS, RAW_STRIDE = 5, 1024
R_EMPTY, R_FULL, R_ONE, R_NEGB = 8, 9, 10, 6   # N_i = 0; every t = n; t = 1 everywhere; b in (-a, 0)


@lru_cache(maxsize=None)
def raw_case(a: float):
    """the 12 restaurants of the raw-layer replay test: (K, n, t, h, bpar, hoff, hcls, lik), read-only arrays"""
    rng = np.random.default_rng(4100 + int(round(a * 1000)))
    K = np.array(RAW_K, dtype=np.int32)
    G = int(K.sum())
    koff = np.concatenate([[0], np.cumsum(K)])
    n = rng.integers(0, 40, size=G).astype(np.uint32)
    n[rng.random(G) < 0.05] = 70000                 # (past a uint16: n is a uint32)
    t = np.where(n > 0, 1 + np.floor(rng.random(G) * np.minimum(n, 65535)), 0).astype(np.uint16)
    sl = lambda i: slice(int(koff[i]), int(koff[i + 1]))  # noqa: E731
    n[sl(R_EMPTY)] = 0
    t[sl(R_EMPTY)] = 0
    n[sl(R_FULL)] = np.minimum(n[sl(R_FULL)], 60000)
    n[sl(R_FULL)][:1] = 3
    t[sl(R_FULL)] = n[sl(R_FULL)].astype(np.uint16)
    n[sl(R_ONE)] = np.maximum(n[sl(R_ONE)], 1)
    t[sl(R_ONE)] = 1
    h = 0.01 + rng.random(G)
    bpar = 0.1 + 10.0 * rng.random(len(K))
    bpar[R_NEGB] = -0.5 * a if a > 0 else 2.0 ** -20
    bpar[3] = 1e6
    hoff = np.concatenate([[0], np.cumsum(RAW_HC)]).astype(np.uint64)
    hcls = rng.integers(0, RAW_ROWS, size=int(hoff[-1])).astype(np.uint32)
    lik = rng.random((RAW_ROWS, RAW_STRIDE)) ** 3
    lik[rng.random(lik.shape) < 0.02] = 0.0
    out = (K, n, t, h, bpar, hoff, hcls, lik)
    for x in out:
        x.setflags(write=False)
    return out


BIG_I, BIG_A = 70000, 0.5


@lru_cache(maxsize=None)
def big_case(I: int = BIG_I):
    """I restaurants of 2 dishes and 1 held-out customer each, a matrix of 5 x 2"""
    rng = np.random.default_rng(4200)
    K = np.full(I, 2, dtype=np.int32)
    n = rng.integers(0, 30, size=2 * I).astype(np.uint32)
    t = np.where(n > 0, 1 + np.floor(rng.random(2 * I) * n), 0).astype(np.uint16)
    h = 0.05 + rng.random(2 * I)
    bpar = 0.5 + rng.random(I)
    hoff = np.arange(I + 1, dtype=np.uint64)
    hcls = rng.integers(0, 5, size=I).astype(np.uint32)
    lik = 0.01 + rng.random((5, 2))
    out = (K, n, t, h, bpar, hoff, hcls, lik)
    for x in out:
        x.setflags(write=False)
    return out


def big_truth(case, a=BIG_A):
    """the truth's total and its bar for big_case, vectorised in long double where mpmath would take minutes: theta and p
    in long double (64-bit mantissa: 2^-11 of a double's rounding), the logs by mpmath.  (total, total_bar, sum |H_i|)"""
    mp = hp._mp()
    K, n, t, h, bpar, hoff, hcls, lik = case
    I = K.shape[0]
    LD = np.longdouble
    n2, t2, h2 = n.reshape(I, 2).astype(LD), t.reshape(I, 2).astype(LD), h.reshape(I, 2).astype(LD)
    T, N = t2.sum(axis=1), n2.sum(axis=1)
    b = bpar.astype(LD)
    g, den = b + T * LD(a), b + N
    x = n2 - t2 * LD(a)
    num = x + g[:, None] * h2
    th = np.where((N == 0)[:, None], h2, num / den[:, None])
    e_x = U * (np.abs(t2 * LD(a)) + np.abs(x))
    e_g = U * (np.abs(T * LD(a)) + np.abs(g))
    e_num = e_x + e_g[:, None] * h2 + U * np.abs(g[:, None] * h2) + U * np.abs(num)
    thb = np.where((N == 0)[:, None], 0.0, np.abs(th) * (e_num / np.abs(num) + 2.0 * U)).astype(np.float64) * SLACK
    L = lik[hcls.astype(np.int64)].astype(LD)
    p = (th * L).sum(axis=1)
    pb = ((thb * L.astype(np.float64)).sum(axis=1) + U * 8.0 * p.astype(np.float64)) * SLACK
    xs = [mp.log(mp.mpf(float(v)) + mp.mpf(float(v - LD(float(v))))) for v in p]
    tot = mp.fsum(xs)
    xa = np.array([abs(float(v)) for v in xs])
    xbar = pb / p.astype(np.float64) + U + 2.0 * U * xa + 2.0 ** -60   # (the long double's own rounding of p)
    Hb = xbar + 6.0 * U * xa + U * xa
    return float(tot), float(Hb.sum()) + 8.0 * U * float(xa.sum()) + U * (2.0 * abs(float(tot)) + 16.0), float(xa.sum())
