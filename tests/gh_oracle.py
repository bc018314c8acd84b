"""Replay, 40-digit truth and error bars of the held-out predictive density under Gaussian observations
(libstb_amd/csrc/gauss_heldout.hip, predict.hip's k_gh_sum; include/stb_hip.h "Held-out points under Gaussian observations";
test infrastructure only).

    ell_j = log sum_k theta_ik N(y_j | mu_k, 1 / tau_k)          r_jk = theta_ik N(y_j | mu_k, 1 / tau_k) / p_j
    total = sum_j ell_j,  or  sum_j log((1/S) sum_s p_j^(s))     over the S states of a chain

Replay (numpy float64, one ufunc an operation: no contraction) -- written from the header's text
------------------------------------------------------------------------------------------------
  theta: pr_oracle.theta_replay (stb_predict_dishes' theta, bit for bit).  l_jk: gs_oracle.log_density (stb_gauss_lik's
  values).  m_j: the maximum of l_jk over the k < K with theta_ik > 0, a NaN never greater; not finite: the point is
  impossible (ell = -inf, r = 0).  w_jk = theta_ik exp(l_jk - m_j), +0.0 where theta_ik is not > 0; s_j: blocks of 64 dishes
  through pr_oracle.tree64, the block sums added in block order; ell_j = (m_j + log s_j) + D (-0.9189385332046727);
  r_jk = w_jk / s_j.  The accumulator pair (M, A), empty (-inf, 0): ell = -inf leaves it; ell > M: A = A exp(M - ell) + 1
  (1 from the empty pair), M = ell; else A = A + exp(ell - M).  x_j = ell_j, or M_j + log(A_j / S), impossible when A_j / S
  is not positive and finite; the x_j in chunks of 64 in CSR order through tree64, the chunk sums in order in double-double,
  H_i = hi + lo; restaurants in blocks of 256 by pr_oracle.block_tree, the block sums in order in double-double
  (heldout_replay's association, with x given instead of log(p / S)).
  numpy's exp and log are not the device's: ell, r, A and x are compared within 1e-10, M with the ell it was taken from.

Truth: mpmath at 40 digits from the exact doubles (theta included).

The bars (u = 2^-53; one rounding per operation, E_LOG = 2 per log, E_EXP = 2 per exp, first order, times 1 + 2^-20)
-----------------------------------------------------------------------------------------------------------------
  theta_ik: pr_oracle.truth's bar, relative rt_k.
  l_jk, absolutely (gs_oracle.loglik_bar's per-term part): e_l = u ((E_LOG + 1 + D) hab_k + (3 + D) q / 2 + (hab_k + q / 2)),
      hab_k = sum_d |log(tau_kd) / 2|.
  ell is invariant under the pivot: log sum_k theta_k exp(l_k) = m + log sum_k theta_k exp(l_k - m) for any m, so the
  error of m itself does not enter.  The exponent l - m carries e_l and its own rounding u |l - m|, which the exp turns
  into a relative error; the exp E_EXP u, the product u:
      rw_k = rt_k + e_l + u |l_k - m| + (E_EXP + 1) u
  s, a sum of non-negative terms: the tree is six additions deep, the blocks are added one after another:
      rs = sum_k w_k rw_k / s + u (5 + blocks)
  ell: bar = rs + E_LOG u |log s| + u |m + log s| + u D c + u |ell|        (c = 0.9189...: the product and the addition)
  r_jk: bar = r (rw_k + rs + u).
  The accumulator, absolutely on A (the pivot M is exact by the same invariance; b_s the bar of the state's ell, which is
  a relative error of its term):
      ell > M:  bar' = bar x + A x (u |M - ell| + (E_EXP + 1) u) + b_s + u A',   x = exp(M - ell), A' = A x + 1
      else:     bar' = bar + x (u |ell - M| + E_EXP u + b_s) + u A',             x = exp(ell - M), A' = A + x
  x = M + log(A / S): bar = bar_A / A + u + E_LOG u |log(A / S)| + u |x|.
  H_i: sum_j bar(x_j) + 6 u sum_j |x_j| + u |H_i|; total: sum_i bar(H_i) + 8 u sum_i |H_i| + u (2 |total| + 16), as
  pr_oracle.truth.
Nothing here reads a device result.
"""
from __future__ import annotations

import math
import os
import sys
from functools import lru_cache

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gs_oracle as gso  # noqa: E402
import pr_oracle as pro  # noqa: E402

U = pro.U
E_LOG = gso.E_LOG
E_EXP = 2.0
SLACK = pro.SLACK
C_NORM = -0.9189385332046727
NEG_INF = -math.inf


# ---------------------------------------------------------------------------------------------------- the replay

def theta_of(K, n, t, h, a, bpar, mut=None):
    """theta (I, KP) of I restaurants of K dishes each; mut 'h': theta replaced by h (the wrong predictive)"""
    I = len(n) // K
    th, _, _ = pro.theta_replay(np.full(I, K), n, t, h, a, bpar, tstride=K)
    if mut == "h":
        hh = np.ones(I * K) if h is None else np.asarray(h, dtype=np.float64)
        th = np.zeros_like(th)
        th[:, :K] = hh.reshape(I, K)
    return th


def rest_of(hoff):
    hoff = np.asarray(hoff, dtype=np.int64)
    return np.repeat(np.arange(hoff.shape[0] - 1), np.diff(hoff))


def points(theta, K, hoff, y, mu, tau, rstride=None, mut=None):
    """one state's ell [Ch], resp (Ch, rstride), and the intermediate l, m, w, s, dead.  mut: 'noconst' the constant
    dropped, 'variance' tau read as a variance, 'maxall' the maximum over every k"""
    y, mu, tau = (np.asarray(v, dtype=np.float64) for v in (y, mu, tau))
    Ch, D = y.shape
    rest = rest_of(hoff)
    KP = 64 * max(1, -(-K // 64))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        l = gso.log_density(y, mu, tau) if Ch else np.zeros((0, K))
        if mut == "variance" and Ch:   # the exponent reads tau as a variance, the normaliser as the precision it is
            l = (gso.log_density(y, mu, 1.0 / tau) - gso.dish_H(1.0 / tau)[None, :]) + gso.dish_H(tau)[None, :]
        th = theta[rest, :K]
        pos = th > 0.0
        cand = np.where((pos | (mut == "maxall")) & ~np.isnan(l), l, NEG_INF)
        m = cand.max(axis=1) if Ch else np.zeros(0)
        dead = ~np.isfinite(m)
        ms = np.where(dead, 0.0, m)
        w = np.where(pos & ~dead[:, None], th * np.exp(l - ms[:, None]), 0.0)
        wp = np.zeros((Ch, KP))
        wp[:, :K] = w
        sb = pro.tree64(wp.reshape(Ch, KP // 64, 64))
        s = sb[:, 0].copy()
        for b in range(1, KP // 64):
            s = s + sb[:, b]
        ell = (ms + np.log(s)) + float(D) * (0.0 if mut == "noconst" else C_NORM)
        ell = np.where(dead, NEG_INF, ell)
        rs = K if rstride is None else rstride
        resp = np.zeros((Ch, rs))
        resp[:, :K] = np.where(dead[:, None], 0.0, w / np.where(dead, 1.0, s)[:, None])
    return {"ell": ell, "resp": resp, "l": l, "m": m, "w": w, "s": s, "dead": dead}


def acc_empty(Ch):
    return np.full(Ch, NEG_INF), np.zeros(Ch)


def acc_update(M, A, ell):
    """the pair after one state's ell"""
    M, A, ell = (np.asarray(v, dtype=np.float64) for v in (M, A, ell))
    with np.errstate(over="ignore", invalid="ignore"):
        live = ell != NEG_INF
        up = live & (ell > M)
        A_up = np.where(M == NEG_INF, 1.0, A * np.exp(np.where(up, M - ell, 0.0)) + 1.0)
        A_in = A + np.exp(np.where(live & ~up, ell - M, 0.0))
    return np.where(up, ell, M), np.where(up, A_up, np.where(live, A_in, A))


def acc_x(M, A, S):
    """(x_j = M_j + log(A_j / S), possible)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.asarray(A, dtype=np.float64) / np.float64(S)
        ok = (q > 0.0) & np.isfinite(q)
        x = np.where(ok, np.asarray(M, dtype=np.float64) + np.log(np.where(ok, q, 1.0)), 0.0)
    return x, ok


def sum_x(x, ok, hoff):
    """(H_i [I] with -inf where a point is impossible, total, impossible points): heldout_replay's association on x"""
    hoff = np.asarray(hoff, dtype=np.int64)
    I = hoff.shape[0] - 1
    cnt = np.diff(hoff)
    x = np.where(ok, np.asarray(x, dtype=np.float64), 0.0)
    nch = max(1, int(-(-cnt.max() // 64))) if I else 1
    pad = np.zeros((I, nch * 64))
    rest = rest_of(hoff)
    pad[rest, np.arange(x.shape[0]) - hoff[:-1][rest]] = x
    Hsum = pro.ordered_dd_sum(pro.tree64(pad.reshape(I, nch, 64)))
    bad = np.zeros(I, dtype=bool)
    np.logical_or.at(bad, rest, ~ok)
    nblk = max(1, -(-I // 256))
    full = np.zeros(nblk * 256)
    full[:I] = Hsum
    total = float(pro.ordered_dd_sum(pro.block_tree(full.reshape(nblk, 256))))
    nimp = int((~ok).sum())
    return np.where(bad, NEG_INF, Hsum), (NEG_INF if nimp else total), nimp


def total_of_ell(ell, hoff):
    ell = np.asarray(ell, dtype=np.float64)
    return sum_x(ell, np.isfinite(ell), hoff)


def naive_linear(ells):
    """what stb_tindic_heldout's accumulator would give on exp(ell): log((sum_s exp(ell_s)) / S)"""
    with np.errstate(divide="ignore"):
        acc = 0.0
        for e in ells:
            acc = acc + math.exp(e) if e > -1e308 else acc
        return math.log(acc / len(ells)) if acc > 0.0 else NEG_INF


# ---------------------------------------------------------------------------------------------------- truth and bars

def _mp():
    return gso._mp()


def mp_theta(K, n, t, h, a, bpar):
    mp = _mp()
    I = len(n) // K
    bpar = np.broadcast_to(np.asarray(bpar, dtype=np.float64), (I,))
    am, out = mp.mpf(float(a)), []
    for i in range(I):
        nn, tt = [int(v) for v in n[i * K:(i + 1) * K]], [int(v) for v in t[i * K:(i + 1) * K]]
        hh = [mp.mpf(1) if h is None else mp.mpf(float(h[i * K + k])) for k in range(K)]
        Ti, Ni, bm = sum(tt), sum(nn), mp.mpf(float(bpar[i]))
        out.append(hh if Ni == 0 else [((nn[k] - tt[k] * am) + (bm + Ti * am) * hh[k]) / (bm + Ni) for k in range(K)])
    return out


def mp_points(thm, hoff, y, mu, tau):
    """(ell as mpf or None for an impossible point, resp as lists of mpf) per point"""
    mp = _mp()
    K, D = mu.shape
    rest = rest_of(hoff)
    hl = [mp.fsum(mp.log(mp.mpf(float(tau[k, d]))) / 2 for d in range(D)) for k in range(K)]
    mum = [[mp.mpf(float(mu[k, d])) for d in range(D)] for k in range(K)]
    taum = [[mp.mpf(float(tau[k, d])) for d in range(D)] for k in range(K)]
    ells, resps = [], []
    for j in range(y.shape[0]):
        yj = [mp.mpf(float(v)) for v in y[j]]
        th = thm[rest[j]]
        ks = [k for k in range(K) if th[k] > 0]
        l = {k: hl[k] - mp.fsum((yj[d] - mum[k][d]) ** 2 * taum[k][d] for d in range(D)) / 2 for k in ks}
        top = max(l.values()) if ks else None
        if top is None or top < -1.7e308:
            ells.append(None)
            resps.append([mp.mpf(0)] * K)
            continue
        wk = {k: th[k] * mp.exp(l[k] - top) for k in ks}
        s = mp.fsum(wk.values())
        ells.append(top + mp.log(s) - D * mp.log(2 * mp.pi) / 2)
        resps.append([wk[k] / s if k in wk else mp.mpf(0) for k in range(K)])
    return ells, resps


def point_bars(theta, theta_bar, K, hoff, y, mu, tau, rep):
    """(ell_bar [Ch], resp_bar (Ch, K)) from the replay's own values"""
    y, mu, tau = (np.asarray(v, dtype=np.float64) for v in (y, mu, tau))
    Ch, D = y.shape
    rest = rest_of(hoff)
    nb = max(1, -(-K // 64))
    hab = np.abs(0.5 * np.log(tau)).sum(axis=1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        q = (((y[:, None, :] - mu[None, :, :]) ** 2) * tau[None, :, :]).sum(axis=2)
        e_l = U * ((E_LOG + 1.0 + D) * hab[None, :] + (3.0 + D) * 0.5 * q + (hab[None, :] + 0.5 * q))
        th = theta[rest, :K]
        rt = np.where(th > 0.0, theta_bar[rest, :K] / np.where(th > 0.0, th, 1.0), 0.0)
        m = np.where(rep["dead"], 0.0, rep["m"])
        live = rep["w"] > 0.0
        rw = np.where(live, rt + e_l + U * np.abs(rep["l"] - m[:, None]) + (E_EXP + 1.0) * U, 0.0)
        s = np.where(rep["dead"], 1.0, rep["s"])
        rs = (rep["w"] * rw).sum(axis=1) / s + U * (5.0 + nb)
        logs = np.log(s)
        ell = np.where(rep["dead"], 0.0, rep["ell"])
        ell_bar = (rs + E_LOG * U * np.abs(logs) + U * np.abs(m + logs) + U * D * abs(C_NORM) + U * np.abs(ell)) * SLACK
        resp_bar = rep["resp"][:, :K] * (rw + rs[:, None] + U) * SLACK
    return np.where(rep["dead"], 0.0, ell_bar), resp_bar


def total_bars(x, xbar, hoff):
    """(Hi_bar [I], total_bar) of the sums of x with the bars xbar (impossible points: x = 0, bar 0)"""
    hoff = np.asarray(hoff, dtype=np.int64)
    I = hoff.shape[0] - 1
    Hb, tot_abs, tot = np.zeros(I), 0.0, 0.0
    for i in range(I):
        sl = slice(int(hoff[i]), int(hoff[i + 1]))
        Hsum = math.fsum(x[sl])
        Hb[i] = float(xbar[sl].sum()) + 6.0 * U * float(np.abs(x[sl]).sum()) + U * abs(Hsum)
        tot_abs += abs(Hsum)
        tot += Hsum
    return Hb, float(Hb.sum()) + 8.0 * U * tot_abs + U * (2.0 * abs(tot) + 16.0)


def truth(K, n, t, h, a, bpar, hoff, y, mu, tau):
    """mpmath truth and bars of one state: ell, ell_bar [Ch] (-inf: impossible), ell_mp, resp, resp_bar (Ch, K), Hi, Hi_bar
    [I], total, total_bar"""
    I = len(n) // K
    theta = theta_of(K, n, t, h, a, bpar)
    tb = pro.truth(np.full(I, K), n, t, h, a, bpar)["theta_bar"]
    theta_bar = np.zeros_like(theta)
    theta_bar[:, :K] = tb
    rep = points(theta, K, hoff, y, mu, tau)
    ell_bar, resp_bar = point_bars(theta, theta_bar, K, hoff, y, mu, tau, rep)
    ells, resps = mp_points(mp_theta(K, n, t, h, a, bpar), hoff, y, mu, tau)
    ell = np.array([NEG_INF if e is None else float(e) for e in ells])
    resp = np.array([[float(v) for v in r] for r in resps]).reshape(len(ells), K)
    out = {"ell": ell, "ell_bar": ell_bar, "ell_mp": ells, "resp": resp, "resp_bar": resp_bar, "replay": rep}
    out.update(mp_totals(ells, ell_bar, hoff))
    return out


def mp_totals(xs, xbar, hoff):
    """Hi, Hi_bar, total, total_bar from per-point mpf values (None: impossible)"""
    mp = _mp()
    hoff = np.asarray(hoff, dtype=np.int64)
    I = hoff.shape[0] - 1
    Hi = np.zeros(I)
    tot, imp = mp.mpf(0), False
    for i in range(I):
        part = xs[int(hoff[i]):int(hoff[i + 1])]
        Hm = mp.fsum(v for v in part if v is not None)
        Hi[i] = NEG_INF if any(v is None for v in part) else float(Hm)
        imp |= any(v is None for v in part)
        tot += Hm
    xf = np.array([0.0 if v is None else float(v) for v in xs])
    Hb, tbar = total_bars(xf, np.asarray(xbar, dtype=np.float64), hoff)
    return {"Hi": Hi, "Hi_bar": Hb, "total": NEG_INF if imp else float(tot), "total_bar": tbar}


def acc_truth(ells_mp, ell_bars, hoff=None):
    """the running estimate over the states ells_mp[s][j] (mpf, or None), their bars ell_bars[s][j]: x [Ch] (-inf where no
    state is possible), x_mp, x_bar [Ch], and with hoff the totals.  The bar follows the replayed updates' own values."""
    mp = _mp()
    S, Ch = len(ells_mp), len(ells_mp[0])
    xs, xbar = [], np.zeros(Ch)
    for j in range(Ch):
        col = [ells_mp[s][j] for s in range(S)]
        live = [v for v in col if v is not None]
        if not live:
            xs.append(None)
            continue
        top = max(live)
        xs.append(top + mp.log(mp.fsum(mp.exp(v - top) for v in live) / S))
        M, A, bar = NEG_INF, 0.0, 0.0
        for s in range(S):
            if col[s] is None:
                continue
            e, b = float(col[s]), float(ell_bars[s][j])
            if e > M:
                xx = 0.0 if M == NEG_INF else math.exp(M - e)
                d = 0.0 if M == NEG_INF else abs(M - e)
                An = A * xx + 1.0
                bar = bar * xx + A * xx * (U * d + (E_EXP + 1.0) * U) + b + U * An
                M, A = e, An
            else:
                xx = math.exp(e - M)
                An = A + xx
                bar = bar + xx * (U * abs(e - M) + E_EXP * U + b) + U * An
                A = An
        lq = math.log(A / S)
        xbar[j] = (bar / A + U + E_LOG * U * abs(lq) + U * abs(M + lq)) * SLACK
    out = {"x": np.array([NEG_INF if v is None else float(v) for v in xs]), "x_mp": xs, "x_bar": xbar}
    if hoff is not None:
        out.update(mp_totals(xs, xbar, hoff))
    return out


def within(got, want, bar):
    return pro.within(float(got), float(want), float(bar))


# ---------------------------------------------------------------------------------------------------- the cases

# (K, D): the register / streamed boundary on both axes; one, two, sixteen blocks of dishes.  The points per restaurant
# {0, 1, 63, 64, 65, 300} (the chunk of 64, a trip count above one) concern the sum alone, which knows nothing of K and D:
# the small shapes carry them all, the large ones one chunk boundary, so that the 40-digit truth stays a matter of seconds
SHAPES = {
    "1x1": (1, 1, (1, 0, 63, 64, 65, 300)),
    "5x3": (5, 3, (300, 1, 0, 63, 64, 65)),
    "64x16": (64, 16, (2, 0, 65, 1)),
    "65x16": (65, 16, (2, 0, 65, 1)),
    "64x17": (64, 17, (2, 0, 65, 1)),
    "130x64": (130, 64, (2, 0, 5, 1)),
    "1024x2": (1024, 2, (2, 0, 5, 1)),
}
CASE_A, CASE_B = 0.4, 1.3


@lru_cache(maxsize=None)
def make_case(name, seed=0):
    """a state of len(counts) restaurants (the last with N_i = 0) and held-out points around the dishes' centres.  Where
    K > 1, dish 1 has n = 0 and h = 0 everywhere (theta = 0) and point 0 sits on its centre, far from every other dish;
    where there are more than three points, point 2 is impossible (1e200 in its last coordinate)"""
    K, D, counts = SHAPES[name]
    rng = np.random.default_rng(1000 + 7 * K + D + seed)
    I = len(counts)
    n = rng.integers(0, 6, size=(I, K))
    n[I - 1] = 0
    h = 0.1 + rng.random((I, K))
    if K > 1:
        n[:, 1] = 0
        h[:, 1] = 0.0
    if n[:I - 1].sum(axis=1).min() == 0:
        n[:I - 1, 0] += 1
    t = np.where(n > 0, rng.integers(1, 7, size=(I, K)).clip(max=np.maximum(n, 1)), 0)
    mu = rng.normal(0.0, 3.0, size=(K, D))
    tau = 0.3 + 2.0 * rng.random((K, D))
    if K > 1:
        mu[1] = 60.0
    hoff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    Ch = int(hoff[-1])
    z = rng.integers(0, K, size=Ch)
    y = mu[z] + rng.normal(0.0, 1.0, size=(Ch, D)) / np.sqrt(tau[z])
    if K > 1:
        y[0] = mu[1]
    if Ch > 3:
        y[2, D - 1] = 1e200
    return dict(K=K, D=D, I=I, n=n.reshape(-1).astype(np.uint32), t=t.reshape(-1).astype(np.uint16), h=h.reshape(-1),
                a=CASE_A, bpar=np.full(I, CASE_B), hoff=hoff, y=y, mu=mu, tau=tau)


@lru_cache(maxsize=None)
def case_truth(name):
    c = make_case(name)
    return truth(c["K"], c["n"], c["t"], c["h"], c["a"], c["bpar"], c["hoff"], c["y"], c["mu"], c["tau"])


def states_of(name, S=3):
    """S different (n, t, mu, tau) on one case's restaurants and points, for the accumulator"""
    base = make_case(name)
    out = []
    for s in range(S):
        c = dict(make_case(name, seed=s))
        c["hoff"], c["y"] = base["hoff"], base["y"]
        out.append(c)
    return out


# ---------------------------------------------------------------------------------------------------- the law

# gs_oracle's tiny chain with one held-out point per restaurant: p(y | x) = Z(x with y in restaurant i) / Z(x), each Z the
# prior of (z, t) times the evidence, summed over the states (chain_exact's enumeration, extended to the seventh customer)
LAW_Y = (0.4, -1.5)            # the point of restaurant 0, of restaurant 1
LAW_PRIOR = "weak"
LAW_ITER = 2020                # gs_oracle.CHAIN_PRIORS["weak"]'s length: no longer than the Gaussian chain test's
LAW_BATCHES = 20
LAW_Z = 4.5                    # the bar: this many batch-means standard errors of the replay chain's per-iteration p_j


def law_prior():
    k0, a0, b0 = gso.CHAIN_PRIORS[LAW_PRIOR][0]
    return gso.prior(k0, a0, b0, 1)


def _Z(xs_by_rest, pr):
    """sum over (z, t) of the PYP prior (h = 1/2) times the evidence of the customers xs_by_rest[i] of restaurant i"""
    import td_oracle as tdo
    import ti_oracle as tio

    K, a, b = (gso.CHAIN[k] for k in ("K", "a", "b"))
    S = {m: tio.stirling(m, a) for m in range(1, max(len(v) for v in xs_by_rest) + 1)}
    per = [tdo.states(len(v), K) for v in xs_by_rest]
    x = np.concatenate([np.asarray(v, dtype=np.float64) for v in xs_by_rest]).reshape(-1, 1)
    den = 1.0
    for v in xs_by_rest:
        den *= float(np.prod([b + j for j in range(len(v))]))
    tot = 0.0
    for s0 in per[0]:
        for s1 in per[1]:
            v = 1.0
            for z, ts in (s0, s1):
                v *= float(np.prod([b + j * a for j in range(sum(ts))]))
                for nk, tk in zip(tdo.counts(z, K), ts):
                    if nk:
                        v *= S[nk][tk] * 0.5 ** tk
            zz = np.array(s0[0] + s1[0])
            n, mean, Q, _ = gso.stats(x, zz, K)
            tot += v * math.exp(gso.logml(n, mean, Q, pr))
    return tot / den


@lru_cache(maxsize=None)
def law_exact():
    """(p(y_0 | x), p(y_1 | x))"""
    pr = law_prior()
    Nc = gso.CHAIN["Nc"]
    x = [list(gso.CHAIN["x"][:Nc]), list(gso.CHAIN["x"][Nc:])]
    Z0 = _Z(x, pr)
    return (_Z([x[0] + [LAW_Y[0]], x[1]], pr) / Z0, _Z([x[0], x[1] + [LAW_Y[1]]], pr) / Z0)


def law_points():
    return np.array([0, 1, 2], dtype=np.int64), np.array(LAW_Y).reshape(2, 1)


def law_chain(law="right", iterations=LAW_ITER, seed=gso.CHAIN_SEED):
    """gs_oracle.chain_run's right chain, scored after every iteration: p (iterations, 2), the per-iteration densities of
    the two held-out points under (n, t) after the sweep and the (mu, tau) the sweep ran under.  law: 'right'; 'h' theta
    replaced by h; 'stale' the parameters of the first draw kept for scoring while the chain moves on"""
    import td_oracle as tdo
    import ti_oracle as tio

    I, Nc, K, a, b = (gso.CHAIN[k] for k in ("I", "Nc", "K", "a", "b"))
    pr = law_prior()
    x = gso.chain_x()
    vt = tio.ExactV(list(range(1, Nc + 1)), a, Nc)
    Ks, bpar, h = np.full(I, K), np.full(I, b), np.full(I * K, 0.5)
    cust = np.array([0, 1, 0, 1, 0, 1])
    n = np.concatenate([tdo.counts(cust[:Nc], K), tdo.counts(cust[Nc:], K)]).astype(np.uint32)
    t = (n > 0).astype(np.uint16)
    hoff, y = law_points()
    out, first = np.zeros((iterations, 2)), None
    for s in range(iterations):
        nn, mean, Q, _ = gso.stats(x, cust, K)
        mu, tau, _ = gso.draw(nn, mean, Q, pr, seed + 1, s)
        L, _ = gso.lik(x, mu, tau)
        n, t, _, cust, _, _ = tdo.sweep(Ks, n, t, h, a, bpar, vt, Nc, Nc, seed, s, cust, np.arange(I * Nc), L)
        first = (mu, tau) if first is None else first
        pm, pt = first if law == "stale" else (mu, tau)
        th = theta_of(K, n, t, h, a, bpar, mut="h" if law == "h" else None)
        out[s] = np.exp(points(th, K, hoff, y, pm, pt)["ell"])
    return out


def batch_se(p, burn=None, batches=LAW_BATCHES):
    """(mean, batch-means standard error) of the columns of p past the burn-in"""
    burn = gso.CHAIN["burn"] if burn is None else burn
    v = p[burn:]
    m = v.shape[0] // batches
    bm = v[:m * batches].reshape(batches, m, -1).mean(axis=1)
    return v.mean(axis=0), bm.std(axis=0, ddof=1) / math.sqrt(batches)
