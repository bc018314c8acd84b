"""Replay, high-precision truth and error bar of the log marginal of multinomials under a Dirichlet prior
(libstb_amd/csrc/dirmult.hip, include/stb_hip.h stb_dirmult_logml; test infrastructure only).

    log ml = [lgamma(W) - lgamma(W + C)] + sum_j [lgamma(w_j + c_j) - lgamma(w_j)],   W = sum_j w_j, C = sum_j c_j

replay()  the kernel's stated operations and associations in numpy doubles (dirmult.hip's header): the cell terms by
          rise() for 1 <= c <= 8 and the lgamma difference above, W by chunks of 256 in the block tree and double-double,
          a row's cells by chunks of 64 in the shuffle tree and double-double, a column's by chunks of 256 rows added in
          row order and double-double, the multinomials by blocks of 256 in the block tree and double-double, the total by
          dd_merge.  The host's log and lgamma stand in for the device's, so it is a model of the operations, not a bit
          oracle of the device; `variant` makes the deliberately wrong replays the host tests tell apart.
truth()   mpmath at 40 digits from the exact doubles w_j = fl(scale * d_w[j]) -- the law is defined on those doubles -- with
          W their exact sum.

The bar (u = 2^-53), from the kernel's own operations -- nothing here is fitted to what the kernel returns
-------------------------------------------------------------------------------------------------------
  * a log is 1 ulp of its value, taken as 2 u |y|; an lgamma is hp.L_LGAMMA ulp of its value, taken as L u |y| as
    everywhere in these oracles, and 16 u absolute for the term it stands in.
  * rise(x, m): m logs; the arguments x + j (j >= 1) round once, which moves a log by u / 2; the m - 1 additions round by
    u / 2 times a partial sum each, every partial sum at most S = sum_j |log(x + j)|: 2 u S + (m - 1) u / 2 (1 + S).
  * c > 8: u (L (|lgamma(w + c)| + |lgamma(w)|) + slope(w + c) + |y| + 16): the argument w + c is formed with one
    rounding times lgamma's slope (hp._slope bounds |z psi(z)|), the subtraction rounds once.
  * W: d_w NULL, one product: dW = u W.  Else eight levels of the block tree, each rounding by at most u / 2 times sums
    of magnitudes that W bounds (the weights are >= 0), the double-double sum and hi + lo: dW = 5 u W.  The normaliser
    moves by |psi(W + C) - psi(W)| dW; its own operations as the cell's, on W.
  * a row's cells: a chunk of 64 by a six-level tree, 6 u / 2 sum |terms| (u / 2 a level on partial sums the magnitudes
    bound); the chunks in double-double; hi + lo rounds once.  A column's: a thread adds the n non-zero terms of a chunk
    one after another, (n - 1) u / 2 sum |terms|; then as the row's.  each = cells + normaliser rounds once.
  * a component over the multinomials: their own bars, eight levels of the block tree, 8 u / 2 sum |value_m|, the blocks
    in double-double, hi + lo and the truth's own rounding to a double: 2 u |sum| + 16 u.  The total: both components'
    bars without that last term, and 2 u |total| + 16 u.
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

U = hp.U
ROWS, COLUMNS = 1, 2
TINY = float(np.finfo(np.float64).tiny)   # the smallest normal double
NEG_INF = -math.inf
_lg = np.vectorize(math.lgamma, otypes=[np.float64])


# ---------------------------------------------------------------------------------------------------- the replay

def dd_add(hi, lo, x):
    """stb_common.h's dd_add on arrays (or scalars): returns (hi, lo)"""
    hi, lo, x = (np.asarray(v, dtype=np.float64) for v in (hi, lo, x))
    with np.errstate(invalid="ignore", over="ignore"):
        t = hi + x
        bb = t - hi
        lo = np.where(np.isfinite(t), lo + ((hi - (t - bb)) + (x - bb)), lo)
    return t, lo


def dd_sum(xs):
    """xs[n, ...] added along axis 0 in order in double-double: (hi, lo)"""
    xs = np.asarray(xs, dtype=np.float64)
    hi, lo = np.zeros(xs.shape[1:]), np.zeros(xs.shape[1:])
    for x in xs:
        hi, lo = dd_add(hi, lo, x)
    return hi, lo


def tree64(v):
    """the 64-lane shuffle tree along the last axis (64 long): lane 0's value"""
    v = np.array(v, dtype=np.float64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v[..., :off] + v[..., off:2 * off]
    return v[..., 0]


def block_tree(x, variant=None):
    """x[..., 256] -> the block's sum: (x[l] + x[l + 64]) + (x[l + 128] + x[l + 192]) per lane, then the shuffle tree"""
    x = np.asarray(x, dtype=np.float64)
    if variant == "block_order":      # a wrong replay: the block's values one after another
        s = np.zeros(x.shape[:-1])
        for j in range(x.shape[-1]):
            s = s + x[..., j]
        return s
    return tree64((x[..., 0:64] + x[..., 64:128]) + (x[..., 128:192] + x[..., 192:256]))


def blocks_of(x, size):
    """x[n] padded with 0.0 to a multiple of `size` (at least one block) and cut: [nblk, size]"""
    x = np.asarray(x, dtype=np.float64)
    nblk = max(1, -(-x.shape[0] // size))
    out = np.zeros(nblk * size)
    out[:x.shape[0]] = x
    return out.reshape(nblk, size)


def rise(x: float, m: int, variant=None) -> float:
    if variant == "short_rise":
        m -= 1
        if m == 0:
            return 0.0
    s = math.log(x + 0.0)
    for j in range(1, m):
        s = s + math.log(x + float(j))
    return s


def cell_term(w: float, c: int, variant=None) -> float:
    if c == 0:
        return 0.0
    if c <= 8:
        return rise(w, c, variant)
    arg = w + float(c)
    if variant == "arg_minus_one":
        arg = arg - 1.0
    return math.lgamma(arg) - math.lgamma(w)


def norm_term(W: float, C: int, variant=None) -> float:
    if C == 0 or variant == "no_norm":
        return 0.0
    if C <= 8:
        return -rise(W, C)
    return math.lgamma(W) - math.lgamma(W + float(C))


def weights_of(w, ncat: int, scale: float):
    """(the ncat doubles w_j, W as the kernel forms it); w a scalar (d_w NULL) or ncat values"""
    s = float(scale)
    if np.ndim(w) == 0:
        wc = s * float(w)
        return np.full(ncat, wc), float(ncat) * wc
    wv = s * np.asarray(w, dtype=np.float64)
    assert wv.shape == (ncat,)
    hi, lo = dd_sum(block_tree(blocks_of(wv, 256)))
    return wv, float(hi + lo)


def _terms(cnt, wcell, variant):
    """the matrix of cell terms (0.0 where c = 0 or the cell is impossible) through the unique (w, c) pairs"""
    out = np.zeros(cnt.shape)
    nz = (cnt > 0) & (wcell > 0.0)
    if nz.any():
        pairs = np.stack([wcell[nz], cnt[nz].astype(np.float64)], axis=1)
        uniq, inv = np.unique(pairs, axis=0, return_inverse=True)
        vals = np.array([cell_term(float(a), int(b), variant) for a, b in uniq])
        out[nz] = vals[np.asarray(inv).reshape(-1)]
    return out


def replay(cnt, w, orientation: int, scale: float = 1.0, variant=None):
    """the call on the matrix cnt[rows, cols] (the stride's padding already cut away): a dict of each [multinomials], cells,
    norms, total, nonzero, count, zero_weight, impossible"""
    cnt = np.asarray(cnt, dtype=np.uint64)
    rows, cols = cnt.shape
    by_rows = orientation == ROWS
    wv, W = weights_of(w, cols if by_rows else rows, scale)
    wcell = np.broadcast_to(wv[None, :] if by_rows else wv[:, None], cnt.shape)
    x = _terms(cnt, wcell, variant)
    bad = (cnt > 0) & (wcell == 0.0)
    if by_rows:
        nch = -(-cols // 64)
        pad = np.zeros((rows, nch * 64))
        pad[:, :cols] = x
        hi, lo = dd_sum(np.moveaxis(tree64(pad.reshape(rows, nch, 64)), 1, 0))
        C = cnt.sum(axis=1)
        imp_m = bad.any(axis=1)
    else:
        nch = max(1, -(-rows // 256))
        pad = np.zeros((nch * 256, cols))
        pad[:rows] = x
        pad = pad.reshape(nch, 256, cols)
        csum = np.zeros((nch, cols))
        for j in range(256):
            csum = csum + pad[:, j, :]
        hi, lo = dd_sum(csum)
        C = cnt.sum(axis=0)
        imp_m = bad.any(axis=0)
    cells_m = hi + lo
    uniqC, inv = np.unique(C, return_inverse=True)
    norm_m = np.array([norm_term(W, int(c), variant) for c in uniqC])[np.asarray(inv).reshape(-1)]
    each = np.where(imp_m, NEG_INF, cells_m + norm_m)
    ch, cl = dd_sum(block_tree(blocks_of(cells_m, 256), variant))
    nh, nl = dd_sum(block_tree(blocks_of(norm_m, 256), variant))
    th, tl = dd_add(0.0, 0.0, ch)
    tl = tl + cl
    th, tl = dd_add(th, tl, nh)
    tl = tl + nl
    imp = int(bad.sum())
    return {"each": each, "cells": NEG_INF if imp else float(ch + cl), "norms": float(nh + nl),
            "total": NEG_INF if imp else float(th + tl), "nonzero": int((cnt > 0).sum()), "count": int(cnt.sum()),
            "zero_weight": int(((cnt == 0) & (wcell == 0.0)).sum()), "impossible": imp, "W": W}


# ---------------------------------------------------------------------------------------------------- the truth and the bar

@lru_cache(maxsize=None)
def _rise_truth(x: float, m: int):
    """(sum_j log(x + j) as mpf, bar)"""
    mp = hp._mp()
    logs = [mp.log(mp.mpf(x) + j) for j in range(m)]
    S = sum(abs(float(v)) for v in logs)
    return sum(logs), U * (2.0 * S + 0.5 * (m - 1) * (1.0 + S))


@lru_cache(maxsize=None)
def cell_truth(w: float, c: int):
    """(the cell term as mpf, its bar) for w > 0, c >= 1"""
    mp = hp._mp()
    if c <= 8:
        return _rise_truth(w, c)
    l1, l0 = mp.loggamma(mp.mpf(w) + c), mp.loggamma(mp.mpf(w))
    y = l1 - l0
    return y, U * (hp.L_LGAMMA * (abs(float(l1)) + abs(float(l0))) + float(hp._slope(w + float(c))) + abs(float(y)) + 16.0)


def norm_truth(Wm, C: int, dW: float):
    """(the normaliser as mpf, its bar); Wm the exact sum of the weights, dW the bound of the kernel's W against it"""
    mp = hp._mp()
    if C == 0:
        return mp.mpf(0), 0.0
    move = abs(float(mp.digamma(Wm + C) - mp.digamma(Wm))) * dW
    Wd = float(Wm)
    if C <= 8:
        logs = [mp.log(Wm + j) for j in range(C)]
        S = sum(abs(float(v)) for v in logs)
        return -sum(logs), U * (2.0 * S + 0.5 * (C - 1) * (1.0 + S)) + move
    l0, l1 = mp.loggamma(Wm), mp.loggamma(Wm + C)
    y = l0 - l1
    return y, U * (hp.L_LGAMMA * (abs(float(l1)) + abs(float(l0))) + float(hp._slope(Wd + float(C))) + abs(float(y)) + 16.0) + move


def _multinomial_truth(c, wv, Wm, dW, by_rows):
    """one multinomial's (cells mpf, cells bar, norm mpf, norm bar, impossible) from its counts c[ncat]"""
    mp = hp._mp()
    nz = np.nonzero(c)[0]
    cells, bar = mp.mpf(0), 0.0
    imp = False
    group = 64 if by_rows else 256
    mags = {}
    for j in nz:
        if wv[j] == 0.0:
            imp = True
            continue
        y, b = cell_truth(float(wv[j]), int(c[j]))
        cells += y
        bar += b
        g = int(j) // group
        n, m = mags.get(g, (0, 0.0))
        mags[g] = (n + 1, m + abs(float(y)))
    for n, m in mags.values():
        bar += (3.0 if by_rows else 0.5 * (n - 1)) * U * m
    bar += U * abs(float(cells))
    nm, nbar = norm_truth(Wm, int(c.sum()), dW)
    return cells, bar, nm, nbar, imp


def truth(cnt, w, orientation: int, scale: float = 1.0):
    """the truth and the bars of every output on the matrix cnt[rows, cols]: each, each_bar [multinomials] (doubles; -inf
    where impossible), cells, norms, total as (value, bar), and the exact counters"""
    mp = hp._mp()
    cnt = np.asarray(cnt, dtype=np.uint64)
    rows, cols = cnt.shape
    by_rows = orientation == ROWS
    ncat = cols if by_rows else rows
    wv, _ = weights_of(w, ncat, scale)
    Wm = mp.fsum(mp.mpf(float(v)) for v in wv) if np.ndim(w) else mp.mpf(float(wv[0])) * ncat
    dW = (1.0 if np.ndim(w) == 0 else 5.0) * U * float(Wm)
    M = cnt if by_rows else cnt.T
    uniq, inv, mult = np.unique(M, axis=0, return_inverse=True, return_counts=True)
    inv = np.asarray(inv).reshape(-1)
    per = [_multinomial_truth(c, wv, Wm, dW, by_rows) for c in uniq]
    each = np.array([NEG_INF if p[4] else float(p[0] + p[2]) for p in per])[inv]
    each_bar = np.array([p[1] + p[3] + U * abs(float(p[0] + p[2])) for p in per])[inv]
    tot = [mp.mpf(0), mp.mpf(0)]
    inner = [0.0, 0.0]
    for p, m in zip(per, mult):
        m = int(m)
        for q, (v, b) in enumerate(((p[0], p[1]), (p[2], p[3]))):
            tot[q] += m * v
            inner[q] += m * (b + 4.0 * U * abs(float(v)))
    wcell = np.broadcast_to(wv[None, :] if by_rows else wv[:, None], cnt.shape)
    imp = int(((cnt > 0) & (wcell == 0.0)).sum())
    total = tot[0] + tot[1]
    last = lambda v: U * (2.0 * abs(float(v)) + 16.0)
    return {"each": each, "each_bar": each_bar,
            "cells": (NEG_INF if imp else float(tot[0]), inner[0] + last(tot[0])),
            "norms": (float(tot[1]), inner[1] + last(tot[1])),
            "total": (NEG_INF if imp else float(total), inner[0] + inner[1] + last(total)),
            "nonzero": int((cnt > 0).sum()), "count": int(cnt.sum()),
            "zero_weight": int(((cnt == 0) & (wcell == 0.0)).sum()), "impossible": imp}


def within(got, want, bar) -> bool:
    """|got - want| <= bar, equal infinities agreeing; never true for a NaN"""
    if math.isinf(want) or math.isinf(got):
        return got == want
    return abs(got - want) <= bar


def worst_ratio(got, want) -> float:
    """the largest |got - truth| / bar over each, cells, norms and total (inf where an infinity or a NaN disagrees)"""
    worst = 0.0
    for g, t, b in zip(np.asarray(got["each"]), want["each"], want["each_bar"]):
        if math.isinf(t) or math.isinf(g) or g != g:
            worst = max(worst, 0.0 if g == t else math.inf)
        elif g != t:
            worst = max(worst, abs(g - t) / b)
    for k in ("cells", "norms", "total"):
        g, (t, b) = got[k], want[k]
        if math.isinf(t) or math.isinf(g) or g != g:
            worst = max(worst, 0.0 if g == t else math.inf)
        elif g != t:
            worst = max(worst, abs(g - t) / b)
    return worst


# ---------------------------------------------------------------------------------------------------- the cases

CELL_C = (0, 1, 8, 9, 257, 65535, 2 ** 32 - 1)
CELL_W = (TINY, 1e-3, 1.0, 1e6)


def _sparse(rng, shape, zero, small=(1, 2, 3, 8, 9, 12, 40), big=()):
    c = rng.choice(np.array(small, dtype=np.uint64), size=shape)
    if big:
        hit = rng.random(shape) < 0.03
        c = np.where(hit, rng.choice(np.array(big, dtype=np.uint64), size=shape), c)
    return np.where(rng.random(shape) < zero, 0, c).astype(np.uint32)


def _case(name):
    """(cnt [rows, stride] uint32 with garbage in the padding, cols, w (a vector or a scalar), scale, orientation)"""
    rng = np.random.default_rng(abs(hash_name(name)))
    kind, *dims = name.split("_")
    if kind == "cellrows":      # every c against every w: a row a count, the weights along the columns
        cnt = np.repeat(np.array(CELL_C, dtype=np.uint64)[:, None], len(CELL_W), axis=1).astype(np.uint32)
        return cnt, len(CELL_W), np.array(CELL_W), 1.0, ROWS
    if kind == "cellcols":      # the same cells as columns: the weights along the rows
        cnt = np.repeat(np.array(CELL_C, dtype=np.uint64)[None, :], len(CELL_W), axis=0).astype(np.uint32)
        return cnt, len(CELL_C), np.array(CELL_W), 1.0, COLUMNS
    rows, cols = int(dims[0]), int(dims[1])
    stride = int(dims[2]) if len(dims) > 2 else cols
    if kind == "wide":          # one long sparse row: the weights' sum takes more than one stage of 512 chunks
        cnt = _sparse(rng, (rows, cols), 0.99, big=(257,))
        return cnt, cols, np.exp(rng.uniform(math.log(1e-3), math.log(10.0), size=cols)), 1.0, ROWS
    if kind == "rows":
        if rows > 100000:       # few distinct rows, so that the truth is a few hundred multinomials
            cnt = _sparse(rng, (rows, stride), 0.5, small=(1, 2, 9, 12))
            w = np.array([0.25, 1.0, 3.5])[:cols]
        else:
            cnt = _sparse(rng, (rows, stride), 0.6, big=(257, 65535, 2 ** 32 - 1))
            w = np.exp(rng.uniform(math.log(1e-3), math.log(10.0), size=cols))
        if stride > cols:
            cnt[:, cols:] = rng.integers(1, 2 ** 32, size=(rows, stride - cols), dtype=np.uint64).astype(np.uint32)
        return cnt, cols, w, 0.7, ROWS
    assert kind == "cols"
    cnt = _sparse(rng, (rows, stride), 0.8, big=(257, 65535))
    if stride > cols:
        cnt[:, cols:] = rng.integers(1, 2 ** 32, size=(rows, stride - cols), dtype=np.uint64).astype(np.uint32)
    w = np.exp(rng.uniform(math.log(1e-3), math.log(10.0), size=rows))
    return cnt, cols, w, 1.0, COLUMNS


def hash_name(name: str) -> int:
    h = 1469598103934665603
    for ch in name.encode():
        h = ((h ^ ch) * 1099511628211) % (1 << 61)
    return h


# rows past one trip of the rows kernel's workgroups (at most 8 x 256 compute units, a block of 256 rows a trip) and past
# one staging trip of its last workgroup (512 blocks)
ROWS_PAST_A_TRIP = 256 * 2048 + 257
# (wide: 512 x 256 + 257 categories, past one stage of the weights' chunk sums)
ROW_CASES = ["rows_3_2", "rows_5_64", "rows_5_65_80", "rows_2_1024", "rows_257_7", "rows_%d_3" % ROWS_PAST_A_TRIP,
             "wide_1_%d" % (512 * 256 + 257)]
# (257 and 513 columns: a second block of columns in the last workgroup, and the launch that many columns take)
COL_CASES = ["cols_%d_%d" % (r, c) for c in (3, 65) for r in (1, 255, 256, 257, 513)] + ["cols_257_65_70", "cols_3_257", "cols_300_513"]
CELL_CASES = ["cellrows", "cellcols"]
CASES = ROW_CASES + COL_CASES + CELL_CASES


@lru_cache(maxsize=None)
def case(name):
    return _case(name)


@lru_cache(maxsize=None)
def case_truth(name):
    cnt, cols, w, scale, orient = case(name)
    return truth(cnt[:, :cols], w, orient, scale)


@lru_cache(maxsize=None)
def case_replay(name, variant=None):
    cnt, cols, w, scale, orient = case(name)
    return replay(cnt[:, :cols], w, orient, scale, variant)
