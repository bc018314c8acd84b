"""A high-precision reference for the Stirling tables, written from the mathematics (test infrastructure only).

Every other numeric check of the tables compares with oracle/stb_oracle.c, which restates the reference's own
double-precision log-domain recurrence and is itself off by tens of units of 2^-53 * max(1, |y|).  This module gives the
true values to well below a double's rounding, and the error model the device's outputs are held to.

Truth
-----
* S^n_m = (n - 1 - m a) S^{n-1}_m + S^{n-1}_{m-1}, S^1_1 = 1, in the linear domain in x87 long double (64-bit
  significand), one int64 exponent per cell, every row normalised with frexp / ldexp; the log is taken only at output,
  log(v) + e ln2 with ln2 in long double.  The coefficient is formed with ONE rounding at 64 bits: a = a_hi + a_lo with
  a_hi the top 32 bits of a's significand, so m a_hi (m < 2^17) and m a_lo are exact and only the subtraction
  (n - 1 - m a_hi) - m a_lo rounds (for a >= 2^-14 the first subtraction is exact too).  Each row step then rounds three
  times at 2^-64 (coefficient, product, sum): the truth's relative error is <= 3 n 2^-64, 1/700 of the bar below.
* V^n_m = S^n_m / S^n_{m-1} and S^n_1 = Gamma(n - a) / Gamma(1 - a) from the same cells.
* exact_rows: every double a is p / 2^k, so Shat^n_m = 2^{k(n-m)} S^n_m is an integer with
  Shat^n_m = (2^k (n-1) - m p) Shat^{n-1}_m + Shat^{n-1}_{m-1}: Python ints, for N up to ~1500.  It pins the long-double
  truth (tests/test_hp_host.py).
* restaurant / bterms terms by mpmath.loggamma at 40 digits.

Error model of the device's linear-domain forms (derivation)
------------------------------------------------------------
u = 2^-53.  All forms but FILL_LOGDOMAIN run the recurrence on block-floating cells (v, e): per cell and row one fma
v <- fma(coef, v, left) (fill_hb.hip hb_row, fill_pc.hip, fill_chain.hip, grid_hb.hip gh_row, fill_rows.h cell_step),
the left neighbour scaled by a power of two, renormalisations by ldexp -- both exact (no cell comes near the subnormal
range: values are kept at 2^-PC_BIAS [0.5, 1) per lane, adjacent columns differ by less than n^C).  The coefficient
c = n - 1 - m a is formed once per strip / tile as (double)(n0 - 1) - (double)m * a (fill_hb.hip:378 and :1005,
fill_pc.hip:79/120, grid_hb.hip:293; fill_rows.h:169 and grid_hb.hip:144 use one fma, which only rounds less) and carried
down the rows by coef += 1.0.

Everything is positive, so the first-order relative error of S^n_m is at most the sum over rows k <= n of the largest
relative error made in row k (the cells of one row split the paths into S^n_m into disjoint sets).  In row k:
  * the fma rounds once: u;
  * the coefficient's absolute error is at most u m a (the product) + u max(c_k, m a) (the subtraction; the start value
    may lie below zero, right of the diagonal, where |c_0| <= m a) + 2 u c_k (coef += 1.0 is exact inside a binade; at a
    binade crossing it rounds by at most half an ulp of the new binade, and those half ulps sum to at most 2 u c_k).
    A coefficient multiplies a non-zero cell only where m <= k - 1, so c_k = k - 1 - m a >= m (1 - a) and
    m a / c_k <= a / (1 - a): relative error <= u (a/(1-a) + max(1, a/(1-a)) + 2) <= u (1 + 2/(1-a)).
Per row u (2 + 2/(1-a)), over n rows:  K1 = 2, K2 = 2.

The log is taken from the bits (hb_logs8 and its copies): exponent + 7 mantissa bits index a 128-entry {1/c, -log(1/c)}
table, a degree-5 Taylor polynomial in r = z/c - 1 (|r| <= 2^-8: truncation r^6/6 <= 2^-50.6 = 5.3 u absolute), then
fma(kf, ln2, ...): ln2's rounding times kf <= |y| / ln2 and the final roundings stay within 4 u |y|; 16 u absolute covers
the table entries, the polynomial and small cells.  So the bar of a log cell is

    bar(n, a, y) = u (K1 n + K2 n / (1 - a) + 4 |y| + 16).

A ratio V = S^n_m / S^n_{m-1} takes one division of two such cells: relative bar u (2 (K1 n + K2 n / (1 - a)) + 4).

S^n_1 does not come from the recurrence: every form writes lgamma((double)n - a) - lgamma(1.0 - a) (fill_pc.hip k_s1 and
k_prep).  Its budget, s1bar: each argument z is formed with one rounding (1 - a is exact for a >= 1/2), which moves
lgamma by at most u |z psi(z)| <= u (z (max(log z, 0) + gamma) + 1) (psi(z) lies in [-gamma, log z) for z >= 1 and in
[-1/z - gamma, -1/z] below); lgamma itself is held to L = 4 ulp of its value (the accuracy the HIP math library states
for double lgamma away from its negative zeros); the final subtraction rounds once, u |y|; and 16 u absolute.

    s1bar(n, a, y) = u (sum over z = n - a, 1 - a of [z (max(log z, 0) + gamma) + 1 + L |lgamma(z)|] + |y| + 16).

Other rules (the reference's order, where errors grow with |y| and no linear-domain model applies):
  * FILL_LOGDOMAIN and the reference's own V recurrence (stb_fill_V_exact, and stb_fill_V below 512 rows): the worst
    error against the truth at most 4x the oracle's worst error against the same truth on the same table, + 1e-15.
  * float outputs: each value equals float32(truth), except where the truth lies within the double bar of a float
    rounding boundary; there one float ulp is allowed and the cell is counted.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
K1 = 2.0
K2 = 2.0
LN2 = np.log(LD(2))
# fdlibm's split of ln2: e * LN2_HI is exact for |e| < 2^20
LN2_HI = LD(6.93147180369123816490e-01)
LN2_LO = LD(1.90821492927058770002e-10)
_NEG = np.int64(-(1 << 40))  # the exponent of a zero cell
_CLIP = -30000               # shifts below this make a term vanish at long-double precision anyway


def check_longdouble() -> None:
    """the truth needs x87 long double; a platform without it must not silently get a weaker truth"""
    nm = np.finfo(LD).nmant
    if nm < 63:
        raise RuntimeError(f"np.longdouble has a {nm}-bit mantissa here; the high-precision truth needs 63")


def split(a: float):
    """a = a_hi + a_lo, a_hi the top 32 bits of a's significand (both exact doubles)"""
    a = float(a)
    if a == 0.0:
        return 0.0, 0.0
    f, e = math.frexp(a)
    hi = math.ldexp(math.floor(math.ldexp(f, 32)), e - 32)
    return hi, a - hi


# ---------------------------------------------------------------------------------------------------- the truth

def rows(a, N: int, M: int):
    """yield (n, v, e) for n = 1 .. N: S^n_m = v[d, m] 2^e[d, m] for m = 0 .. min(n, M) (column 0 is zero), D discounts
    in one row loop.  The arrays are the generator's own state: use them before asking for the next row."""
    check_longdouble()
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    D = a.shape[0]
    hl = np.array([split(x) for x in a], dtype=np.float64).reshape(D, 2)
    m = np.arange(M + 1, dtype=LD)
    mah = m[None, :] * hl[:, 0:1].astype(LD)    # exact
    mal = m[None, :] * hl[:, 1:2].astype(LD)    # exact
    v = np.zeros((D, M + 1), dtype=LD)
    e = np.full((D, M + 1), _NEG, dtype=np.int64)
    v[:, 1], e[:, 1] = LD(0.5), 1               # S^1_1 = 1
    yield 1, v[:, :2], e[:, :2]
    for n in range(2, N + 1):
        L = min(n, M)
        c = (LD(n - 1) - mah[:, 1:L + 1]) - mal[:, 1:L + 1]
        vu, eu = v[:, 1:L + 1], e[:, 1:L + 1]
        vl, el = v[:, 0:L], e[:, 0:L]
        E = np.maximum(eu, el)
        x = np.ldexp(c * vu, np.maximum(eu - E, _CLIP)) + np.ldexp(vl, np.maximum(el - E, _CLIP))
        f, de = np.frexp(x)
        v[:, 1:L + 1] = f
        e[:, 1:L + 1] = np.where(f == 0, _NEG, E + de)
        yield n, v[:, :L + 1], e[:, :L + 1]


def logs(v, e):
    """log S (long double) of the cells (v, e); -inf for zero cells"""
    with np.errstate(divide="ignore"):
        return np.log(v) + e.astype(LD) * LN2


def ratios(v, e):
    """V^n_m = S^n_m / S^n_{m-1} for m = 1 .. L-1 of a row (v, e) with columns 0 .. L (V^n_1 = S^n_1 / 0: inf)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.ldexp(v[..., 1:] / v[..., :-1], np.maximum(e[..., 1:] - e[..., :-1], -16000))


def _s_rowoff(n, M):
    if n <= 3:
        return 0
    if n <= M + 1:
        k = n - 3
        return k * (k + 1) // 2
    return (M - 1) * M // 2 + (n - M - 2) * (M - 1)


def _v_rowoff(n, M):
    if n <= 2:
        return 0
    if n <= M:
        k = n - 2
        return k * (k + 1) // 2
    return (M - 1) * M // 2 + (n - M - 1) * (M - 1)


def s_cells(N, M):
    return _s_rowoff(N + 1, M) if N >= 3 else 0


def v_cells(N, M):
    return _v_rowoff(N + 1, M) if N >= 2 else 0


def tables(a, N: int, M: int, want_v: bool = False):
    """the truth in the device's packed orders, long double, per discount: a list of (S1[N], S[cells] or None,
    V[vcells] or None).  S row n (3..N) holds m = 2 .. min(n-1, M); V row n (2..N) holds m = 2 .. min(n, M)."""
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    D = a.shape[0]
    S1 = np.empty((D, N), dtype=LD)
    S = np.empty((D, s_cells(N, M)), dtype=LD)
    V = np.empty((D, v_cells(N, M)), dtype=LD) if want_v else None
    for n, v, e in rows(a, N, M):
        lg = logs(v, e)
        S1[:, n - 1] = lg[:, 1]
        if n >= 3:
            ln = min(n - 2, M - 1)
            o = _s_rowoff(n, M)
            S[:, o:o + ln] = lg[:, 2:2 + ln]
        if want_v and n >= 2:
            ln = min(n - 1, M - 1)
            o = _v_rowoff(n, M)
            V[:, o:o + ln] = ratios(v, e)[:, 1:1 + ln]
    return [(S1[d], S[d], None if V is None else V[d]) for d in range(D)]


def cell_coords(N, M):
    """(n, m) of every cell of the packed S order (int64 arrays)"""
    ns = np.arange(3, N + 1)
    ln = np.minimum(ns - 2, M - 1)
    n = np.repeat(ns, ln)
    start = np.repeat(np.cumsum(ln) - ln, ln)
    m = np.arange(n.shape[0]) - start + 2
    return n.astype(np.int64), m.astype(np.int64)


def vcell_coords(N, M):
    ns = np.arange(2, N + 1)
    ln = np.minimum(ns - 1, M - 1)
    n = np.repeat(ns, ln)
    start = np.repeat(np.cumsum(ln) - ln, ln)
    m = np.arange(n.shape[0]) - start + 2
    return n.astype(np.int64), m.astype(np.int64)


# ---------------------------------------------------------------------------------------------------- exact integers

def dyadic(a: float):
    """a = p / 2^k exactly"""
    fr = Fraction(float(a))
    k = fr.denominator.bit_length() - 1
    assert fr.denominator == 1 << k
    return fr.numerator, k


def exact_rows(a: float, N: int, M: int):
    """yield (n, k, [Shat^n_m for m = 0 .. min(n, M)]) with Shat^n_m = 2^{k(n-m)} S^n_m (Python ints)"""
    p, k = dyadic(a)
    two_k = 1 << k
    row = [0, 1]
    yield 1, k, row
    for n in range(2, N + 1):
        L = min(n, M)
        base = two_k * (n - 1)
        new = [0] * (L + 1)
        for m in range(1, L + 1):
            up = row[m] if m < len(row) else 0
            new[m] = (base - m * p) * up + row[m - 1]
        row = new
        yield n, k, row


def _top64(x: int):
    """x = f 2^b with f in [1/2, 1) as a long double (truncated to 64 bits) and b"""
    b = x.bit_length()
    t = x >> (b - 64) if b > 64 else x << (64 - b)
    f = (LD(t >> 32) * LD(2.0 ** 32) + LD(t & 0xFFFFFFFF)) * LD(2.0 ** -64)
    return f, b


def exact_log(x: int, pow2: int) -> LD:
    """log(x 2^pow2) for an integer x > 0, in long double: log(f) + b (LN2_HI + LN2_LO), f in [1/2, 1)"""
    f, b = _top64(x)
    E = LD(b + pow2)
    return np.log(f) + (E * LN2_HI + E * LN2_LO)


def exact_ratio(x: int, y: int, pow2: int) -> LD:
    """x / y * 2^pow2 in long double (relative error < 2^-63)"""
    s = 72 - (x.bit_length() - y.bit_length())
    q = (x << s) // y if s >= 0 else (x >> -s) // y
    f, b = _top64(q)
    return np.ldexp(f, b - s + pow2)


# ---------------------------------------------------------------------------------------------------- the terms

def _mp():
    import mpmath

    mpmath.mp.dps = 40
    return mpmath


def restaurant_term(x: float, T: int, b: float):
    """T log x + lgamma(T + b/x) - lgamma(b/x) and its bar (see term_bar) from the exact doubles x, b"""
    mp = _mp()
    xm, bm = mp.mpf(float(x)), mp.mpf(float(b))
    z = bm / xm
    t1 = T * mp.log(xm)
    t2 = mp.loggamma(T + z)
    t3 = mp.loggamma(z)
    val = t1 + t2 - t3
    return float(val), term_bar([t1, t2, t3], [T + z, z])


def bterms(x: float, Q: float, shape: float, T, apar: float):
    """-Q x + (shape - 1) log x + sum_i [lgamma(T_i + x/apar) - lgamma(x/apar)] and its bar"""
    mp = _mp()
    xm = mp.mpf(float(x))
    z = xm / mp.mpf(float(apar))
    lz = mp.loggamma(z)
    t0 = -mp.mpf(float(Q)) * xm
    t1 = (mp.mpf(float(shape)) - 1) * mp.log(xm)
    val = t0 + t1
    terms, args = [t0, t1], []
    for Ti in np.asarray(T, dtype=np.int64):
        g = mp.loggamma(int(Ti) + z)
        val += g - lz
        terms += [g, lz]
        args += [int(Ti) + z, z]
    return float(val), term_bar(terms, args)


def aterms2(x: float, cnt, T, bpar):
    """stb_hist_aterms2's value from the exact double x: the restaurant terms + sum over sizes s >= 2 of
    cnt[s] (loggamma(s - x) - loggamma(1 - x)), at 40 digits (returned as a long double), and its bar.

    The bar follows gcache_term's own operations (sweep_terms.hip), j = s - 1, u = 2^-53:
      * par = 1.0 - x is formed once on the host with one rounding, |d par| <= u/2 (par <= 1), exact for x >= 1/2.  The
        term's slope in par is psi(j + par) - psi(par) = sum_{i<j} 1/(par + i): d par moves the term by at most
        (u/2) sum_i 1/(par + i) -- taken as zero for x >= 1/2, where par is exact, so no 1/par enters for small par.
      * j <= 3: log(par (par+1) .. (par+j-1)) -- j-1 sums and j-1 products, each one relative rounding u, which move the
        log by u each: 2 (j-1) u; the log itself to 2 ulp of its value (what the HIP math library states for double log
        is 1 ulp): + 2 u |y|.
      * j >= 4: lgamma((double)j + par) - lgpar.  Both lgammas (the device's, and the host's for lgpar) at the stated
        L = 4 ulp of their values; the argument j + par is formed with one rounding, which moves lgamma by at most
        u |z psi(z)| (_slope); the subtraction rounds once, u |y|.
      * times the count -- exact as a double below 2^53 -- with one rounding of the product, u |c y|; the sums run in
        double-double (dd_add: no first-order term); the final hi + lo and the addition of the restaurant terms round
        once each: 2 u |total|; 16 u absolute.
    The restaurant terms carry term_bar as everywhere."""
    mp = _mp()
    xm = mp.mpf(float(x))
    par = 1.0 - float(x)
    dpar = 0.0 if float(x) >= 0.5 else U / 2
    lg1 = mp.loggamma(1 - xm)
    val, b = mp.mpf(0), 0.0
    for Ti, bi in zip(np.asarray(T, dtype=np.int64), np.asarray(bpar, dtype=np.float64)):
        v, tb = restaurant_term(x, int(Ti), float(bi))
        val += mp.mpf(v)
        b += tb
    cnt = np.asarray(cnt)
    for s in np.nonzero(cnt[2:])[0] + 2:
        c, j = int(cnt[s]), int(s) - 1
        lgz = mp.loggamma(int(s) - xm)
        y = lgz - lg1
        ya = abs(float(y))
        if j <= 3:
            e = 2.0 * (j - 1) * U + 2.0 * U * ya
        else:
            e = U * (L_LGAMMA * (abs(float(lgz)) + abs(float(lg1))) + float(_slope(j + par)) + ya)
        e += dpar * float(mp.digamma(j + par) - mp.digamma(par))
        val += c * y
        b += c * e + U * c * ya
    hi = float(val)
    return LD(hi) + LD(float(val - hi)), b + U * (2.0 * abs(hi) + 16.0)


def term_bar(terms, args):
    """8 u times the magnitudes of the terms, + 2 u |z psi(z)| for each lgamma argument z (z = b/x and T + z are formed
    with one rounding each: the argument's error times lgamma's slope), + 16 u"""
    mp = _mp()
    s = sum(abs(float(t)) for t in terms)
    g = sum(abs(float(z * mp.digamma(z))) for z in args)
    return U * (8 * s + 2 * g + 16)


# ---------------------------------------------------------------------------------------------------- the rules

def bar(n, a, y):
    """the model bar of a log cell (n, m) of discount a whose true value is y (see the module docstring)"""
    n = np.asarray(n, dtype=np.float64)
    y = np.abs(np.asarray(y, dtype=np.float64))
    return U * (K1 * n + K2 * n / (1.0 - float(a)) + 4.0 * y + 16.0)


L_LGAMMA = 4.0
_GAMMA = 0.5772156649015329


def _slope(z):
    """an upper bound of |z psi(z)| for z > 0 (see the module docstring)"""
    z = np.asarray(z, dtype=np.float64)
    return z * (np.maximum(np.log(z), 0.0) + _GAMMA) + 1.0


def s1bar(n, a, y):
    """the bar of S^n_1 = lgamma(n - a) - lgamma(1 - a) as the device forms it (see the module docstring)"""
    n = np.asarray(n, dtype=np.float64)
    a = float(a)
    z1, z0 = n - a, 1.0 - a
    lg = np.vectorize(math.lgamma, otypes=[np.float64])
    part = _slope(z1) + L_LGAMMA * np.abs(lg(z1)) + _slope(z0) + L_LGAMMA * abs(math.lgamma(z0))
    return U * (part + np.abs(np.asarray(y, dtype=np.float64)) + 16.0)


def vbar(n, a, v):
    """the model bar of a ratio cell V = S^n_m / S^n_{m-1} (absolute, v its true value)"""
    n = np.asarray(n, dtype=np.float64)
    return U * (2.0 * (K1 * n + K2 * n / (1.0 - float(a))) + 4.0) * np.abs(np.asarray(v, dtype=np.float64))


def err(got, truth):
    """|got - truth| in long double (equal infinities: 0)"""
    g = np.asarray(got).astype(LD)
    t = np.asarray(truth, dtype=LD)
    with np.errstate(invalid="ignore"):
        d = np.abs(g - t)
    same = (g == t)
    return np.where(same, LD(0), d)


def scaled_err(got, truth):
    """|got - truth| / max(1, |truth|), as a double"""
    t = np.asarray(truth, dtype=LD)
    return (err(got, truth) / np.maximum(LD(1), np.abs(t))).astype(np.float64)


def float_rule(got, truth, dbar):
    """float cells against float32(truth): (bad cells, cells that took the one-ulp allowance).  A cell differs legally only
    by one float ulp, and only when the truth lies within its double bar of the midpoint between the two floats."""
    got = np.asarray(got, dtype=np.float32)
    t = np.asarray(truth, dtype=LD)
    want = t.astype(np.float32)
    diff = got != want
    if not np.any(diff):
        return 0, 0
    idx = np.nonzero(diff)[0]
    g, w, tt = got[idx], want[idx], t[idx]
    adj = (g == np.nextafter(w, np.float32(np.inf))) | (g == np.nextafter(w, np.float32(-np.inf)))
    mid = (g.astype(LD) + w.astype(LD)) / 2
    near = np.abs(tt - mid) <= np.asarray(dbar, dtype=np.float64)[idx].astype(LD)
    ok = adj & near
    return int(np.count_nonzero(~ok)), int(np.count_nonzero(ok))
