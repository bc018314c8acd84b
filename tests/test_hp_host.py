"""The high-precision truth (tests/hp_oracle.py) pinned on the CPU: against exact integer tables, against mpmath's terms,
and the CPU oracle measured against it.  No GPU."""
import math

import numpy as np
import pytest

import hp_oracle as hp
import orc

U = hp.U
DYADIC = [0.0, 0.5, 0.375, 1 - 2.0 ** -20]
FULL = [0.01, 0.37, 0.98, 0.999, 0.99999, 3 * 2.0 ** -30]


def test_longdouble_is_x87():
    """a platform without a 64-bit long-double significand fails here, loudly, instead of getting a weaker truth"""
    hp.check_longdouble()
    assert np.finfo(np.longdouble).nmant >= 63


def test_split_is_exact():
    for a in DYADIC + FULL + [5e-324, 0.9999999999999999]:
        hi, lo = hp.split(a)
        assert hi + lo == a
        f, _ = math.frexp(hi) if hi else (0.0, 0)
        assert float(f * 2 ** 32).is_integer()


def _vs_exact(a, N, M, every):
    """worst |truth - exact| over the sampled rows, in units of 2^-53 max(1, |y|) (log S, S^n_1) and 2^-53 |V| (V)"""
    want = {}
    for n, k, row in hp.exact_rows(a, N, M):
        if n % every and n < N - 2:
            continue
        L = min(n, M)
        lg = [hp.exact_log(row[m], -k * (n - m)) for m in range(1, L + 1)]
        vv = [hp.exact_ratio(row[m], row[m - 1], k) for m in range(2, L + 1)]
        want[n] = (np.array(lg, dtype=hp.LD), np.array(vv, dtype=hp.LD))
    ws = wv = w1 = 0.0
    for n, v, e in hp.rows(a, N, M):
        if n not in want:
            continue
        lg, vv = want[n]
        got = hp.logs(v, e)[0, 1:]
        s = hp.scaled_err(got, lg) / U
        w1 = max(w1, float(s[0]))
        ws = max(ws, float(s.max()))
        if len(vv):
            gv = hp.ratios(v, e)[0, 1:]
            wv = max(wv, float(np.max(np.abs(gv / vv - 1))) / U)
    return ws, w1, wv


@pytest.mark.parametrize("a", DYADIC + FULL)
def test_long_double_truth_against_exact_integers(a):
    """log S, S^n_1 and V of the long-double truth against the exact tables Shat^n_m = 2^{k(n-m)} S^n_m: within 3 units
    of 2^-53 max(1, |y|) (measured: 0.003 -- both sides in long double)"""
    N, M, every = (1200, 1200, 97) if a in (0.37, 0.99999, 0.5) else (700, 500, 61)
    ws, w1, wv = _vs_exact(a, N, M, every)
    print(f"a={a!r}: log S {ws:.4f}, S1 {w1:.4f}, V {wv:.4f} units")
    assert ws <= 3 and w1 <= 3 and wv <= 3, (ws, w1, wv)


def test_S1_is_the_gamma_ratio():
    """S^n_1 of the truth = Gamma(n - a) / Gamma(1 - a) by mpmath"""
    mp = hp._mp()
    for a in (0.0, 0.37, 0.999, 1 - 2.0 ** -20):
        S1, _, _ = hp.tables([a], 3000, 3)[0]
        for n in (1, 2, 3, 17, 1000, 2999, 3000):
            y = mp.loggamma(n - mp.mpf(a)) - mp.loggamma(1 - mp.mpf(a))
            assert abs(float(S1[n - 1] - hp.LD(float(y)))) <= 2 * U * max(1.0, abs(float(y))), (a, n)


def test_mpmath_terms_against_math_lgamma():
    """the mpmath terms agree with libm's lgamma where both are accurate (arguments away from lgamma's zeros)"""
    for x, T, b in ((0.3, 5, 10.0), (0.7, 120, 3.5), (0.05, 1, 0.2), (0.9, 4000, 50.0)):
        want = T * math.log(x) + math.lgamma(T + b / x) - math.lgamma(b / x)
        got, bar = hp.restaurant_term(x, T, b)
        assert abs(got - want) <= 16 * U * max(1.0, abs(want)), (x, T, b, got, want)
        assert bar >= 8 * U * abs(want)
    T = np.array([3, 17, 200, 1])
    for x in (0.4, 7.0, 300.0):
        want = -2.0 * x + 0.1 * math.log(x) + sum(math.lgamma(t + x / 0.3) - math.lgamma(x / 0.3) for t in T)
        got, _ = hp.bterms(x, 2.0, 1.1, T, 0.3)
        assert abs(got - want) <= 64 * U * max(1.0, abs(want)), (x, got, want)


ORACLE_CASES = [(0.0, 3000), (0.01, 3000), (0.37, 10000), (0.5, 3000), (0.98, 3000),
                (0.999, 1500), (0.99999, 1500), (1 - 2.0 ** -20, 1500)]


@pytest.mark.parametrize("a,N", ORACLE_CASES)
def test_oracle_against_the_truth(a, N):
    """what the reference's algorithm delivers: the CPU oracle (orc.fill_S, orc.rows_stream, orc.fill_V) against the
    truth, in units of 2^-53 max(1, |y|).  At most 64 for a <= 0.98; the numbers near a = 1 are printed (MEASUREMENTS)"""
    if N <= 3000:
        M = N
        S1o, tab = orc.fill_S(a, N, M)
        V = orc.fill_V(a, N, M)
        S1t, St, Vt = hp.tables([a], N, M, want_v=True)[0]
        es = float(np.max(hp.scaled_err(tab, St))) / U
        e1 = float(np.max(hp.scaled_err(S1o, S1t))) / U
        ok = np.isfinite(Vt.astype(np.float64))
        ev = float(np.max(np.abs(V[ok].astype(hp.LD) / Vt[ok] - 1))) / U
        print(f"oracle vs truth a={a!r} N=M={N}: log S {es:.1f}, S1 {e1:.1f}, V {ev:.1f} units")
    else:
        M = N
        pick = [3, 4, 100, 1000, 2500, 5000, 7500, N - 1, N]
        got = orc.rows_stream(a, N, M, pick, threads=8)
        es = 0.0
        for n, v, e in hp.rows(a, N, M):
            if n in got:
                es = max(es, float(np.max(hp.scaled_err(got[n], hp.logs(v, e)[0, 2:2 + len(got[n])]))) / U)
        print(f"oracle vs truth a={a!r} N=M={N} (rows {pick}): log S {es:.1f} units")
    if a <= 0.98:
        assert es <= 64, es


def test_the_new_bar_sees_what_the_oracle_bar_does_not():
    """sensitivity of the checker: 1e-9 on a cell with |y| ~ 5e4 and 1e-11 on a cell with |y| ~ 1.  orc.close at 1e-10
    accepts both perturbed tables; the model bar rejects both (and accepts the truth itself, narrowed to double)"""
    a, N, M = 0.37, 6500, 6500
    want = {}
    for row, v, e in hp.rows(a, N, M):
        if row in (N, 5):
            lg = hp.logs(v, e)[0, 2:min(row - 1, M) + 1]       # the stored cells m = 2 .. n-1 of the row
            target, key = (5e4, "big") if row == N else (1.0, "small")
            j = int(np.argmin(np.abs(np.abs(lg.astype(np.float64)) - target)))
            want[key] = (row, j, lg.copy())
    for key, delta in (("big", 1e-9), ("small", 1e-11)):
        row, j, truth = want[key]
        exact = truth.astype(np.float64)
        bad = exact.copy()
        bad[j] += delta
        print(f"{key}: n={row} m={j + 2} y={float(truth[j]):.6g} delta={delta}")
        assert orc.close(bad, exact, 1e-10)                             # the old bar accepts the perturbed row
        b = hp.bar(row, a, truth.astype(np.float64))
        assert np.all(hp.err(exact, truth) <= b)                        # the new bar accepts the truth ...
        assert not np.all(hp.err(bad, truth) <= b)                      # ... and rejects the perturbation
        assert float(hp.err(bad, truth)[j]) > 4 * b[j]
