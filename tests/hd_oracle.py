"""A high-precision reference for the slope of log S in the discount, g(n, m) = d log S^n_m / da (test infrastructure only).

It reads nothing from the reference tree and nothing from the device.

Truth
-----
* With E = -dS/da:  E^n_m = (n - 1 - m a) E^{n-1}_m + m S^{n-1}_m + E^{n-1}_{m-1}, E^1_1 = 0, next to hp_oracle's S recurrence,
  in x87 long double with ONE int64 exponent a cell shared by S and E (every term is non-negative and E / S <= n / (2 (1 - a)),
  so E fits S's exponent).  The S cells are hp_oracle.rows' own operations: the same bits.  A row step of E rounds four times
  at 2^-64 (two products, two sums) on top of the coefficient's one: the truth's g = -E / S is within 12 n 2^-64 relative.
* dS1[n-1] = d log S^n_1 / da = -sum_{k=1}^{n-1} 1 / (k - a): a long-double running sum (n 2^-64 relative).
* exact_da: S and E as exact rationals (fractions.Fraction); it pins the long-double truth (tests/test_da_host.py).
* the restaurant terms' derivative T / x - (b / x^2) (psi(T + b/x) - psi(b/x)) by mpmath.digamma at 40 digits.

Bar of a device g cell (derivation from fill_da.hip's roundings), u = 2^-53
---------------------------------------------------------------------------
k_fill_da walks (v, w) = (S, E) on block-floating cells.  Per row and cell:
    w <- fma(coef, w, fma(m, v, w_left));   v <- fma(coef, v, v_left);   coef += 1.0
with m = (double)column exact, left neighbours scaled by exact powers of two, renormalisations by ldexp (exact).
  * v is k_fill_pc's own step: hp_oracle's model, relative error after n rows <= u n (K1 + K2 / (1 - a)), K1 = K2 = 2
    (one fma rounding + the coefficient's error u (1 + 2 / (1 - a)) a row).
  * w: all three terms are non-negative, so the relative error of the new w is at most the largest relative error among its
    inputs (w above, w left: eps_{k-1}; v above: delta_{k-1} <= eps_{k-1}) plus what the row adds: the inner fma rounds once
    (u, on part of the sum), the coefficient carries its relative error u (1 + 2 / (1 - a)) (on part of the sum), the outer
    fma rounds once (u):  eps_k <= eps_{k-1} + u (3 + 2 / (1 - a)).  Kw = 3, Kw' = 2.
  * g = -w / v: one division, u; and one more u for what first order leaves out and the truth's own 12 n 2^-64.
    gbar(n, a, g) = u (Kv n + Kw n + (Kv' + Kw') n / (1 - a) + 2) |g|,   Kv = 2, Kw = 3, Kv' = 2, Kw' = 2.
The constants are read off the code, not fitted.

dS1 (k_ds1_da): every term 1 / ((double)k - a) rounds twice (2 u of the term; all terms positive: 2 u of the sum); the sum
runs over chunks of 64 terms: at most 64 additions inside a chunk and ceil(n / 64) over the chunk sums, u of the running
sum each:  ds1bar(n, y) = u (64 + n / 64 + 4) |y|.

Restaurant terms (sweep_terms.hip psi_diff, k_terms_da_partial), z = b / x formed with one rounding (it moves psi(T+z) - psi(z)
by at most u z sum 1/(z+k)^2 <= u times the difference itself):
  * T <= 64: P = sum_{k<T} 1 / (z + k): two roundings a term, T additions:                 bar_psi = u (T + 3) P.
  * T > 64: L = log1p((T - s) / (z + s)): the quotient's 3 roundings move L by at most 3 u L (q / (1 + q) <= log1p q), log1p
    itself is held to 2 u L; the two series tails A(y), |A(y)| <= 1/(2y) + 1/(12 y^2), about ten roundings each and y's own:
    13 u (|A1| + |A0|); the shift sum Q of s <= 16 terms: u (s + 3) Q; the final additions and z: 3 u of the difference;
    truncation of the series 2.4e-18:          bar_psi = u (5 L + 13 (|A1| + |A0|) + (s + 3) Q + 3 |diff|) + 2.4e-18.
  * the term T / x - c diff, c = b / (x x): T / x rounds once, c twice, the product and the subtraction once each:
    bar = u |T / x| + |c| bar_psi + 3 u |c diff| + u |term|.
Sums (double-double partials): the sum of the terms' bars + 4 u |sum|.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import hp_oracle as hp

LD = np.longdouble
U = hp.U
KV, KW, KV1, KW1, CDIV = 2.0, 3.0, 2.0, 2.0, 2.0
DS1_CHUNK = 64
PSI_CUT = 64


# ---------------------------------------------------------------------------------------------------- the truth

def rows(a, N: int, M: int):
    """yield (n, v, w, e) for n = 1 .. N: S^n_m = v[d, m] 2^e[d, m], E^n_m = w[d, m] 2^e[d, m], m = 0 .. min(n, M)"""
    hp.check_longdouble()
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    D = a.shape[0]
    hl = np.array([hp.split(x) for x in a], dtype=np.float64).reshape(D, 2)
    m = np.arange(M + 1, dtype=LD)
    mah = m[None, :] * hl[:, 0:1].astype(LD)
    mal = m[None, :] * hl[:, 1:2].astype(LD)
    v = np.zeros((D, M + 1), dtype=LD)
    w = np.zeros((D, M + 1), dtype=LD)
    e = np.full((D, M + 1), hp._NEG, dtype=np.int64)
    v[:, 1], e[:, 1] = LD(0.5), 1
    yield 1, v[:, :2], w[:, :2], e[:, :2]
    for n in range(2, N + 1):
        L = min(n, M)
        c = (LD(n - 1) - mah[:, 1:L + 1]) - mal[:, 1:L + 1]
        vu, wu, eu = v[:, 1:L + 1], w[:, 1:L + 1], e[:, 1:L + 1]
        vl, wl, el = v[:, 0:L], w[:, 0:L], e[:, 0:L]
        E = np.maximum(eu, el)
        su, sl = np.maximum(eu - E, hp._CLIP), np.maximum(el - E, hp._CLIP)
        x = np.ldexp(c * vu, su) + np.ldexp(vl, sl)
        y = np.ldexp(c * wu + m[None, 1:L + 1] * vu, su) + np.ldexp(wl, sl)
        f, de = np.frexp(x)
        v[:, 1:L + 1] = f
        w[:, 1:L + 1] = np.where(f == 0, LD(0), np.ldexp(y, -de))
        e[:, 1:L + 1] = np.where(f == 0, hp._NEG, E + de)
        yield n, v[:, :L + 1], w[:, :L + 1], e[:, :L + 1]


def slopes(v, w):
    """g = -E / S of a row's cells (NaN where S = 0)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return -w / v


def ds1(a: float, N: int):
    """dS1[n-1], n = 1 .. N (long double)"""
    hi, lo = hp.split(a)
    k = np.arange(1, N, dtype=LD)
    out = np.zeros(N, dtype=LD)
    out[1:] = -np.cumsum(LD(1) / ((k - LD(hi)) - LD(lo)))
    return out


def tables(a, N: int, M: int):
    """per discount (dS1[N], g[cells]) in the device's packed order, long double"""
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    D = a.shape[0]
    G = np.empty((D, hp.s_cells(N, M)), dtype=LD)
    for n, v, w, e in rows(a, N, M):
        if n >= 3:
            ln = min(n - 2, M - 1)
            o = hp._s_rowoff(n, M)
            G[:, o:o + ln] = slopes(v, w)[:, 2:2 + ln]
    return [(ds1(a[d], N), G[d]) for d in range(D)]


def lookup(a, n, t):
    """g_a(n, t) with stb_lookup_dS's cases for unbounded tables (n == t: 0; t == 1: dS1; t = 0 or t > n: NaN), for every
    discount of a: an array [D, pairs], long double"""
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    n = np.asarray(n, dtype=np.int64)
    t = np.asarray(t, dtype=np.int64)
    out = np.full((a.shape[0], n.shape[0]), LD("nan"), dtype=LD)
    out[:, n == t] = 0
    inner = (t >= 2) & (t < n)
    one = (t == 1) & (n > 1)
    if np.any(one):
        N1 = int(n[one].max())
        for d in range(a.shape[0]):
            out[d, one] = ds1(a[d], N1)[n[one] - 1]
    if np.any(inner):
        N, M = int(n[inner].max()), int(t[inner].max())
        by_row = {}
        for i in np.nonzero(inner)[0]:
            by_row.setdefault(int(n[i]), []).append(i)
        for nn, v, w, e in rows(a, N, M):
            idx = by_row.get(nn)
            if idx:
                out[:, idx] = slopes(v, w)[:, t[idx]]
    return out


# ---------------------------------------------------------------------------------------------------- exact rationals

def exact_da(a: float, N: int):
    """rows n = 1 .. N of (S, E) as exact rationals: a list of dicts m -> (S^n_m, E^n_m), m = 1 .. n"""
    af = Fraction(float(a))
    out = [{1: (Fraction(1), Fraction(0))}]
    for n in range(2, N + 1):
        prev, cur = out[-1], {}
        for m in range(1, n + 1):
            Su, Eu = prev.get(m, (0, 0))
            Sl, El = prev.get(m - 1, (0, 0))
            c = n - 1 - m * af
            cur[m] = (c * Su + Sl, c * Eu + m * Su + El)
        out.append(cur)
    return out


def frac_to_ld(x: Fraction) -> LD:
    """a rational as a long double, relative error < 2^-62"""
    if x == 0:
        return LD(0)
    s = 80 - (x.numerator.bit_length() - x.denominator.bit_length())
    q = (abs(x.numerator) << s) // x.denominator if s >= 0 else (abs(x.numerator) >> -s) // x.denominator
    f, b = hp._top64(q)
    r = np.ldexp(f, b - s)
    return -r if x < 0 else r


# ---------------------------------------------------------------------------------------------------- restaurant terms

def psi_diff(T: int, z):
    """psi(T + z) - psi(z) at 40 digits and the bar of the device's value (module docstring); z an mpmath number"""
    mp = hp._mp()
    if T == 0:
        return mp.mpf(0), 0.0
    d = mp.digamma(T + z) - mp.digamma(z)
    df = abs(float(d))
    if T <= PSI_CUT:
        return d, U * (T + 3) * df
    zf = float(z)
    s = 0 if zf >= 16.0 else int(np.ceil(16.0 - zf))
    tail = lambda y: 1.0 / (2.0 * y) + 1.0 / (12.0 * y * y)
    Lg = float(mp.log1p((T - s) / (z + s)))
    Q = float(sum(1 / (z + k) for k in range(s)))
    return d, U * (5 * Lg + 13 * (tail(T + zf) + tail(zf + s)) + (s + 3) * Q + 3 * df) + 2.4e-18


def restaurant_term_da(x: float, T: int, b: float):
    """T / x - (b / x^2) (psi(T + b/x) - psi(b/x)) from the exact doubles x, b: (value, bar)"""
    mp = hp._mp()
    xm, bm = mp.mpf(float(x)), mp.mpf(float(b))
    d, dbar = psi_diff(int(T), bm / xm)
    c = bm / (xm * xm)
    t1 = T / xm
    val = t1 - c * d
    return val, U * abs(float(t1)) + abs(float(c)) * dbar + 3 * U * abs(float(c * d)) + U * abs(float(val))


def restaurant_terms_da(x: float, T, bpar):
    """the sum over restaurants and its bar"""
    mp = hp._mp()
    val, bar = mp.mpf(0), 0.0
    for Ti, bi in zip(np.asarray(T, dtype=np.int64), np.asarray(bpar, dtype=np.float64)):
        v, b = restaurant_term_da(x, int(Ti), float(bi))
        val += v
        bar += b
    return val, bar + 4 * U * abs(float(val))


# ---------------------------------------------------------------------------------------------------- the rules

def gbar(n, a, g):
    n = np.asarray(n, dtype=np.float64)
    return U * ((KV + KW) * n + (KV1 + KW1) * n / (1.0 - float(a)) + CDIV) * np.abs(np.asarray(g, dtype=np.float64))


def ds1bar(n, y):
    n = np.asarray(n, dtype=np.float64)
    return U * (DS1_CHUNK + n / DS1_CHUNK + 4.0) * np.abs(np.asarray(y, dtype=np.float64))


def pair_sum(a: float, n, t):
    """sum over pairs with n > 1 of g_a(n, t) (long double; NaN with a log-0 pair) and its bar"""
    n = np.asarray(n, dtype=np.int64)
    t = np.asarray(t, dtype=np.int64)
    keep = n > 1
    n, t = n[keep], t[keep]
    g = lookup([a], n, t)[0]
    if np.any(np.isnan(g)):
        return LD("nan"), float("nan")
    gd = g.astype(np.float64)
    bars = np.where(t == 1, ds1bar(n, gd), gbar(n, a, gd))
    bars[n == t] = 0.0
    tot = g.sum()
    return tot, float(bars.sum() + 4 * U * abs(float(tot)))


def grad(a: float, n, t, T, bpar):
    """d aterms / da at a: (value as a double-double pair of floats summed in mpmath, bar)"""
    mp = hp._mp()
    ps, pb = pair_sum(a, n, t)
    rs, rb = restaurant_terms_da(a, T, bpar)
    if ps != ps:
        return float("nan"), float("nan")
    hi = float(ps)
    tot = rs + mp.mpf(hi) + mp.mpf(float(ps - LD(hi)))
    return float(tot), pb + rb + U * abs(float(tot))


# ---------------------------------------------------------------------------------------------------- the mode

def modea_replay(gradfn, a_lo, a_hi, tol, rounds_max, Dmax):
    """stb_groups_modea's control flow (groups_da.hip) on a gradient function of an array of abscissae: a dict with a_hat,
    the last bracket, its ends' gradients, rounds, evals, at_bound, delta, grad, curv"""
    k = min(Dmax, 8)
    lo, hi, glo, ghi = float(a_lo), float(a_hi), 0.0, 0.0
    rounds = evals = at_bound = 0
    while True:
        first = rounds == 0
        if first:
            px = [lo + i * (hi - lo) / (k - 1) for i in range(k)]
            px[k - 1] = hi
        else:
            px = [lo + (i + 1) * (hi - lo) / (k + 1) for i in range(k)]
        gr = [float(v) for v in gradfn(np.array(px))]
        rounds += 1
        evals += k
        assert not any(v != v for v in gr)
        if first:
            x = px
            if gr[0] <= 0.0:
                at_bound, hi, glo, ghi = -1, lo, gr[0], gr[0]
                break
            if gr[-1] >= 0.0:
                at_bound, lo, glo, ghi = 1, hi, gr[-1], gr[-1]
                break
        else:
            x = [lo] + px + [hi]
            gr = [glo] + gr + [ghi]
        i = 0
        while i + 2 < len(x) and not (gr[i] > 0.0 and gr[i + 1] <= 0.0):
            i += 1
        narrowed = (x[i + 1] - x[i]) < (hi - lo)
        lo, hi, glo, ghi = x[i], x[i + 1], gr[i], gr[i + 1]
        if hi - lo <= tol or rounds >= rounds_max or not narrowed:
            break
    ah = lo
    if not at_bound:
        ah = lo - glo * (hi - lo) / (ghi - glo)
        if not ah >= lo:
            ah = lo
        if ah > hi:
            ah = hi
    delta = tol if at_bound else hi - lo
    delta = min(delta, 0.5 * ah, 0.5 * (1.0 - ah))
    g3 = [float(v) for v in gradfn(np.array([ah - delta, ah, ah + delta]))]
    evals += 3
    return dict(a_hat=ah, lo=lo, hi=hi, g_lo=glo, g_hi=ghi, rounds=rounds, evals=evals, at_bound=at_bound, delta=delta,
                grad=g3[1], curv=(g3[2] - g3[0]) / (2.0 * delta), g3=g3)


def bisect_root(gradfn, lo, hi, tol=1e-12):
    """the root of a decreasing-through-zero gradient on [lo, hi] by plain bisection to width tol"""
    glo = float(gradfn(np.array([lo]))[0])
    assert glo > 0 > float(gradfn(np.array([hi]))[0])
    while hi - lo > tol:
        mid = 0.5 * (lo + hi)
        if float(gradfn(np.array([mid]))[0]) > 0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def grad_many(xs, n, t, T, bpar):
    """d aterms / da at every abscissa of xs (doubles), one pass over the truth's rows for all of them"""
    xs = np.atleast_1d(np.asarray(xs, dtype=np.float64))
    n = np.asarray(n, dtype=np.int64)
    t = np.asarray(t, dtype=np.int64)
    keep = n > 1
    ps = lookup(xs, n[keep], t[keep]).sum(axis=1)
    return np.array([float(restaurant_terms_da(x, T, bpar)[0]) + float(p) for x, p in zip(xs, ps)])
