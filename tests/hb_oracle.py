"""A numpy replay of the per-group concentration step (libstb_amd/csrc/hyperb.hip, include/stb_hip.h stb_sample_bgroups),
built on hq_oracle's streams and log-Gamma variates, and the law it is checked against.

The step, as the header specifies it: key = mix(seed + (sweep+1) gamma); key_i = mix(key + (i+1) gamma).
  L_i    stb_sample_logq's draw on key_i with the restaurant's own b_i (0 where N_i = 0)
  Y_i    [T_i >= 1] + sum_{k=1}^{T_i-1} [u_k (b_i + k a) < b_i], u_k element k of the substream mix(key_i ^ SALT_Y)
  rate   1/scale + sum L over the group: blocks of 256 from the group's first restaurant, inside a block four quarters per
         lane and then the tree of a 64-lane wave, the block sums lane-strided in double-double, merged by the same tree,
         1/scale added last
  b_g    exp(log G - log rate), log G the log-Gamma variate of shape + sum Y on mix(mix(key ^ SALT_G) + (g+1) gamma)
The replay also reports the smallest margin of every accept / reject of the variates and of every Bernoulli comparison,
so that a test can pick seeds at which no decision hangs on the last bit of a transcendental.
"""
import math

import numpy as np

import hq_oracle as hq

SALT_Y = np.uint64(0x59B1D5A7C3E9F24D)
SALT_G = np.uint64(0x6A09E667F3BCC909)
LAWS = ("right", "no_k", "no_first")   # the step, and two wrong ones: k dropped from b + k a; the k = 0 factor dropped


# ---- the variates again, with margins (the decisions are hq_oracle's; test_bgroups_host checks the two agree)

def _log_gamma_ge1(alpha, key_i, k, dtype, margin):
    n = alpha.shape[0]
    out = np.full(n, np.nan)
    live = np.ones(n, dtype=bool)
    d = alpha - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    ld = np.log(hq._f(d, dtype)).astype(np.float64)
    for _ in range(hq.CAP):
        idx = np.nonzero(live)[0]
        if idx.size == 0:
            break
        ki = key_i[idx]
        k[idx] += np.uint64(1)
        u1 = hq.unit(ki, k[idx])
        k[idx] += np.uint64(1)
        u2 = hq.unit(ki, k[idx])
        lu1 = np.log(hq._f(u1, dtype)).astype(np.float64)
        cs = np.cos(hq._f(6.283185307179586 * u2, dtype)).astype(np.float64)
        x = np.sqrt(-2.0 * lu1) * cs
        w = 1.0 + c[idx] * x
        if w.size:
            margin[0] = min(margin[0], float(np.min(np.abs(w))))
        pos = w > 0.0
        idx, x, w = idx[pos], x[pos], w[pos]
        ki = key_i[idx]
        v = w * w * w
        k[idx] += np.uint64(1)
        u = hq.unit(ki, k[idx])
        lv = np.log(hq._f(v, dtype)).astype(np.float64)
        lu = np.log(hq._f(u, dtype)).astype(np.float64)
        di = d[idx]
        rhs = ((0.5 * (x * x) + di) - di * v) + di * lv
        if rhs.size:
            margin[0] = min(margin[0], float(np.min(np.abs(lu - rhs) / np.maximum(1.0, np.abs(rhs)))))
        acc = lu < rhs
        out[idx[acc]] = ld[idx[acc]] + lv[acc]
        live[idx[acc]] = False
    return out, live.any()


def _log_gamma(alpha, key_i, k, dtype, margin):
    small = alpha < 1.0
    lg, bad = _log_gamma_ge1(np.where(small, alpha + 1.0, alpha), key_i, k, dtype, margin)
    if small.any():
        idx = np.nonzero(small)[0]
        k[idx] += np.uint64(1)
        u = hq.unit(key_i[idx], k[idx])
        lg[idx] = lg[idx] + np.log(hq._f(u, dtype)).astype(np.float64) / alpha[idx]
    return lg, bad


def rest_keys(seed, sweep, I, first=0):
    key = hq.sweep_key(seed, sweep)
    with np.errstate(over="ignore"):
        return key, hq.mix(key + (np.arange(first, first + I, dtype=np.uint64) + np.uint64(1)) * hq.GAMMA)


def replay_L(bpar, N, seed, sweep, dtype=np.float64, margin=None):
    """L_i with every restaurant's own b_i (hq_oracle.replay_L takes one b)"""
    margin = [math.inf] if margin is None else margin
    N = np.asarray(N, dtype=np.uint64)
    bpar = np.asarray(bpar, dtype=np.float64)
    _, key_i = rest_keys(seed, sweep, N.shape[0])
    L = np.zeros(N.shape[0])
    idx = np.nonzero(N > 0)[0]
    if idx.size == 0:
        return L
    ki = key_i[idx]
    k = np.zeros(idx.size, dtype=np.uint64)
    lgb, bad1 = _log_gamma(bpar[idx], ki, k, dtype, margin)
    lgn, bad2 = _log_gamma(N[idx].astype(np.float64), ki, k, dtype, margin)
    if bad1 or bad2:
        raise RuntimeError("a Gamma draw was not accepted within %d attempts" % hq.CAP)
    D = lgn - lgb
    Dx = hq._f(D, dtype)
    with np.errstate(over="ignore"):
        Lpos = D + np.log1p(np.exp(-Dx)).astype(np.float64)
        Lneg = np.log1p(np.exp(np.minimum(Dx, 0))).astype(np.float64)
    L[idx] = np.where(D > 0.0, Lpos, Lneg)
    return L


def replay_Y(a, bpar, T, seed, sweep, law="right", margin=None):
    """Y_i (uint32): the Bernoulli sums, flat over all (i, k) pairs"""
    margin = [math.inf] if margin is None else margin
    T = np.asarray(T, dtype=np.int64)
    bpar = np.asarray(bpar, dtype=np.float64)
    I = T.shape[0]
    _, key_i = rest_keys(seed, sweep, I)
    ky = hq.mix(key_i ^ SALT_Y)
    cnt = np.maximum(T - 1, 0)
    Y = np.zeros(I, dtype=np.int64) if law == "no_first" else (T >= 1).astype(np.int64)
    tot = int(cnt.sum())
    if tot == 0:
        return Y.astype(np.uint32)
    owner = np.repeat(np.arange(I), cnt)
    start = np.cumsum(cnt) - cnt
    k = (np.arange(tot) - start[owner] + 1).astype(np.uint64)
    u = hq.unit(ky[owner], k)
    b = bpar[owner]
    kk = np.ones(tot) if law == "no_k" else k.astype(np.float64)
    lhs = u * (b + kk * a)
    margin[0] = min(margin[0], float(np.min(np.abs(lhs - b) / b)))
    Y += np.bincount(owner, weights=(lhs < b).astype(np.float64), minlength=I).astype(np.int64)
    return Y.astype(np.uint32)


# ---- the group sum in the kernel's association

def _dd_add(hi, lo, x):
    t = hi + x
    bb = t - hi
    lo = lo + ((hi - (t - bb)) + (x - bb))
    return t, lo


def group_rate(L, inv_scale):
    """1/scale + sum L as the kernels associate it"""
    L = np.asarray(L, dtype=np.float64)
    n = L.shape[0]
    nblk = (n + 255) // 256
    p = np.zeros(nblk * 256)
    p[:n] = L
    p = p.reshape(nblk, 4, 64)
    v = (p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3])     # [nblk, 64]
    w = 64
    while w > 1:
        w //= 2
        v = v[:, :w] + v[:, w:2 * w]
    blk = v[:, 0]
    rounds = (nblk + 63) // 64
    q = np.zeros(max(rounds, 1) * 64)
    q[:nblk] = blk
    q = q.reshape(max(rounds, 1), 64)
    live = (np.arange(max(rounds, 1) * 64) < nblk).reshape(max(rounds, 1), 64)
    hi, lo = np.zeros(64), np.zeros(64)
    for r in range(rounds):
        h2, l2 = _dd_add(hi, lo, q[r])
        hi, lo = np.where(live[r], h2, hi), np.where(live[r], l2, lo)
    w = 64
    while w > 1:
        w //= 2
        h2, l2 = _dd_add(hi[:w], lo[:w], hi[w:2 * w])
        hi, lo = h2, l2 + lo[w:2 * w]
    h, l = _dd_add(hi[0:1], lo[0:1], inv_scale)
    return float(h[0] + l[0])


def replay(a, shape, scale, T, N, bpar, goff, seed, sweep, dtype=np.float64, law="right"):
    """the whole step: dict with L, Y, rate [G], sumY [G], bgrp [G], bpar (new), kept, margin_gamma, margin_y"""
    T = np.asarray(T)
    N = np.asarray(N)
    bpar = np.asarray(bpar, dtype=np.float64)
    I = T.shape[0]
    mg, my = [math.inf], [math.inf]
    L = replay_L(bpar, N, seed, sweep, dtype, mg)
    Y = replay_Y(a, bpar, T, seed, sweep, law, my)
    key = hq.sweep_key(seed, sweep)
    keyG = hq.mix(key ^ SALT_G)
    inv_scale = 1.0 / scale
    if goff is None:
        G = I
        rate = L + inv_scale   # (a block of one restaurant: {L, 0} + 1/scale in double-double rounds to this)
        sumY = Y.astype(np.float64)
        lo_, hi_ = np.arange(I), np.arange(I) + 1
    else:
        goff = np.asarray(goff, dtype=np.int64)
        G = goff.shape[0] - 1
        lo_, hi_ = goff[:-1], goff[1:]
        rate = np.array([group_rate(L[lo_[g]:hi_[g]], inv_scale) for g in range(G)])
        cs = np.concatenate([[0], np.cumsum(Y.astype(np.int64))])
        sumY = (cs[hi_] - cs[lo_]).astype(np.float64)
    with np.errstate(over="ignore"):
        kg = hq.mix(keyG + (np.arange(G, dtype=np.uint64) + np.uint64(1)) * hq.GAMMA)
    k = np.zeros(G, dtype=np.uint64)
    lg, bad = _log_gamma(shape + sumY, kg, k, dtype, mg)
    with np.errstate(over="ignore", invalid="ignore"):
        b = np.exp(hq._f(lg, dtype) - np.log(hq._f(rate, dtype))).astype(np.float64)
    keep = ~((b > 0) & np.isfinite(b))
    new = bpar.copy()
    bg = b.copy()
    for g in np.nonzero(keep)[0]:
        bg[g] = bpar[lo_[g]] if hi_[g] > lo_[g] else np.nan
    size = hi_ - lo_
    owner = np.repeat(np.arange(G), size)
    ok = ~keep[owner]
    idx = np.arange(I)   # (the ranges are contiguous and cover 0 .. I-1)
    new[idx[ok]] = b[owner[ok]]
    return dict(L=L, Y=Y, rate=rate, sumY=sumY, bgrp=bg, bpar=new, kept=int(keep.sum()), margin_gamma=mg[0], margin_y=my[0])


# ---- the law: p(b | .) ~ b^(shape-1) e^(-b/scale) prod_i (b|a)_{T_i} Gamma(b) / Gamma(b + N_i)

_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


class Posterior:
    """the posterior of one group's b by quadrature in u = log b (trapezoid on a fine grid), with its CDF and inverse"""

    def __init__(self, a, shape, scale, T, N, points=60001):
        T = np.atleast_1d(np.asarray(T, dtype=np.int64))
        N = np.atleast_1d(np.asarray(N, dtype=np.int64))
        u = np.linspace(-40.0, 12.0, points)
        b = np.exp(u)
        lp = shape * u - b / scale                    # (the Jacobian b of u = log b turns shape - 1 into shape)
        for t, n in zip(T, N):
            for k in range(int(t)):
                lp = lp + np.log(b + k * a)
            if n > 0:
                lp = lp + _lgamma(b) - _lgamma(b + n)
        lp -= lp.max()
        dens = np.exp(lp)
        cdf = np.concatenate([[0.0], np.cumsum(0.5 * (dens[1:] + dens[:-1]) * np.diff(u))])
        self.u, self.cdf = u, cdf / cdf[-1]

    def F(self, b):
        return np.interp(np.log(np.asarray(b, dtype=np.float64)), self.u, self.cdf)

    def inverse(self, p):
        keep = np.concatenate([[True], np.diff(self.cdf) > 0])
        return np.exp(np.interp(p, self.cdf[keep], self.u[keep]))


def ks_pvalue(p):
    """the asymptotic Kolmogorov p-value of values that are uniform on (0, 1) under the hypothesis"""
    n = len(p)
    D = hq.ks_stat(p) / math.sqrt(n)
    lam = (math.sqrt(n) + 0.12 + 0.11 / math.sqrt(n)) * D
    if lam < 0.2:
        return 1.0
    s = sum((-1) ** (j - 1) * math.exp(-2.0 * j * j * lam * lam) for j in range(1, 101))
    return min(1.0, max(0.0, 2.0 * s))


CASES = [(12, 40, 0.5, 2.0, 3.0), (40, 200, 0.1, 1.0, 10.0), (6, 30, 0.9, 0.5, 5.0), (8, 25, 0.0, 1.5, 2.0)]   # (T, N, a, shape, scale)
GROUP4 = ([12, 3, 1, 0], [40, 5, 1, 0], 0.5, 2.0, 3.0)   # one group of four restaurants: (T, N, a, shape, scale)


def chain(case, n, steps, start_seed, seed, law="right", group=1, step_fn=None):
    """n groups of `group` identical-shaped restaurants started from the posterior by inverse CDF, `steps` steps with the
    sweeps 0 .. steps-1 of `seed`; returns (the final b per group, the posterior).  step_fn(a, shape, scale, T, N, bpar,
    goff, seed, sweep) -> new bpar replaces the replay (the device)"""
    Tg, Ng, a, shape, scale = case
    Tg, Ng = np.atleast_1d(Tg), np.atleast_1d(Ng)
    post = Posterior(a, shape, scale, Tg, Ng)
    rng = np.random.default_rng(start_seed)
    b0 = post.inverse(rng.random(n))
    T = np.tile(Tg, n).astype(np.uint32)
    N = np.tile(Ng, n).astype(np.uint32)
    bpar = np.repeat(b0, group)
    goff = None if group == 1 else np.arange(n + 1, dtype=np.int64) * group
    for s in range(steps):
        if step_fn is None:
            bpar = replay(a, shape, scale, T, N, bpar, goff, seed, s, law=law)["bpar"]
        else:
            bpar = step_fn(a, shape, scale, T, N, bpar, goff, seed, s)
    return bpar[::group], post


# ---- the restaurants of the replay tests (test_bgroups_host picks the seeds, test_gpu_bgroups replays on the device)

REPLAY_I = 3000
REPLAY_T = (0, 1, 2, 63, 64, 65, 129, 5000)
REPLAY_PRIOR = (1.5, 20.0)                       # shape, scale
REPLAY_SEEDS = {0.0: 7100, 0.3: 7101, 0.9: 7102}   # discount -> seed (sweep 5): margins checked in test_bgroups_host
REPLAY_SWEEP = 5
RAGGED_SIZES = (1, 255, 256, 257, 513, 0, 8)     # then the rest; the range of 8 holds only empty restaurants


def replay_case(grouping, I=REPLAY_I):
    """(T, N, bpar, goff) for grouping 'each' (every restaurant its own group, b_i log-uniform on [0.01, 2000]), 'one'
    (G = 1, one b) or 'ragged' (RAGGED_SIZES and the rest, b log-uniform per group)"""
    from libstb_amd import synth

    u = synth.unit(2 * I, 977)
    T = np.array(REPLAY_T, dtype=np.uint32)[np.arange(I) % len(REPLAY_T)]
    T = T[(np.arange(I) * 7 + 3) % I] if I % 7 else T          # (a fixed shuffle: the large T are not all in one lane)
    N = np.where(T == 0, 0, T + np.floor(u[:I] * 1000)).astype(np.uint32)
    blog = np.exp(math.log(0.01) + u[I:] * math.log(2000 / 0.01))
    if grouping == "each":
        return T, N, blog, None
    if grouping == "one":
        return T, N, np.full(I, 3.7), np.array([0, I], dtype=np.int64)
    assert grouping == "ragged"
    sizes = list(RAGGED_SIZES)
    sizes.append(I - sum(sizes))
    goff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    e0 = int(goff[6])
    T, N = T.copy(), N.copy()
    T[e0:e0 + 8] = 0
    N[e0:e0 + 8] = 0
    return T, N, np.repeat(blog[:len(sizes)], sizes), goff
