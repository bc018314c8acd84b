"""The truth of the slope of log S in the discount (tests/hd_oracle.py) pinned on the CPU: against exact rationals, against
hp_oracle's S cells, against the reference's S_approx_da goldens where that function is right -- and shown to disagree
where it is wrong (m = 4) -- and a replay of stb_groups_modea's control flow on truth gradients."""
import json
import os

import numpy as np
import pytest

import hd_oracle as hd
import hp_oracle as hp

LD = np.longdouble
HERE = os.path.dirname(os.path.abspath(__file__))
A_PIN = (0.0, 1.0 / 16, 0.5, 0.98)


@pytest.mark.parametrize("a", A_PIN)
def test_truth_against_exact_rationals(a):
    """g = -E / S of the long-double truth within 12 n 2^-64 of exact rationals for N <= 150, and dS1 against the exact sum"""
    N = 150
    ex = hd.exact_da(a, N)
    ds1 = hd.ds1(a, N)
    worst = 0.0
    for n, v, w, e in hd.rows([a], N, N):
        g = hd.slopes(v, w)[0]
        for m in range(1, n + 1):
            S, E = ex[n - 1][m]
            want = hd.frac_to_ld(-E / S)
            tol = LD(12 * n) * LD(2.0) ** -64 * max(abs(want), LD(0))
            err = abs(g[m] - want)
            assert err <= tol + LD(2.0) ** -62 * abs(want), (a, n, m, float(err), float(tol))
            if want != 0:
                worst = max(worst, float(err / abs(want)) / (12 * n * 2.0 ** -64))
        # column 1 is the closed form's derivative
        want1 = hd.frac_to_ld(-ex[n - 1][1][1] / ex[n - 1][1][0])
        assert abs(ds1[n - 1] - want1) <= LD(12 * n) * LD(2.0) ** -64 * abs(want1) + LD(2.0) ** -62 * abs(want1)
    print(f"a={a}: worst error / (12 n 2^-64) = {worst:.3f}")


def test_truth_S_cells_are_hp_oracles():
    a = np.array([0.0, 1.0 / 16, 0.3, 0.98])
    for (n, v, w, e), (n2, v2, e2) in zip(hd.rows(a, 300, 120), hp.rows(a, 300, 120)):
        assert n == n2 and np.array_equal(v, v2) and np.array_equal(e, e2)


def test_E_is_nonnegative_and_bounded():
    """what lets E share S's exponent: 0 <= E / S <= n / (2 (1 - a))"""
    for a in A_PIN:
        for n, v, w, e in hd.rows([a], 200, 200):
            r = -hd.slopes(v, w)[0][1:]
            assert np.all(r >= 0) and np.all(r <= LD(n) / (2 * (1 - LD(a))) * (1 + LD(1e-15)))


def _golden():
    rows = json.load(open(os.path.join(HERE, "golden", "sapprox.json")))["rows"]
    return [(float.fromhex(r["a"]), r["n"], r["m"], float.fromhex(r["S_approx_da"])) for r in rows]


def test_sapprox_da_goldens_m_le_3():
    """the reference's S_approx_da for a in {1/16, 1/8}, m <= 3 is the truth within 1e-11 max(1, |g|) -- n = 2000 included"""
    rows = [r for r in _golden() if r[0] in (1.0 / 16, 1.0 / 8) and r[2] <= 3 and r[1] >= r[2]]
    assert any(r[1] == 2000 for r in rows) and len(rows) >= 30
    for a in (1.0 / 16, 1.0 / 8):
        mine = [r for r in rows if r[0] == a]
        n = np.array([r[1] for r in mine])
        m = np.array([r[2] for r in mine])
        truth = hd.lookup([a], n, m)[0]
        for (aa, nn, mm, got), want in zip(mine, truth):
            err = abs(LD(got) - want)
            print(f"a={a} n={nn} m={mm}: golden {got:.15g} truth {float(want):.15g} err {float(err):.2e}")
            assert err <= 1e-11 * max(1.0, abs(float(want))), (a, nn, mm, got, float(want))


def test_sapprox_da_goldens_m4_are_wrong():
    """the deviation: at m = 4 the reference's S_approx_da is off by more than 1 (a = 1/16, n = 5: +45.87 against -1.0667)"""
    rows = [r for r in _golden() if r[0] in (1.0 / 16, 1.0 / 8) and r[2] == 4 and r[1] > 4]
    assert rows
    for a, n, m, got in rows:
        want = float(hd.lookup([a], [n], [m])[0, 0])
        assert abs(got - want) > 1.0, (a, n, m, got, want)
    ex = hd.exact_da(1.0 / 16, 5)[4][4]
    assert abs(float(-ex[1] / ex[0]) - (-1.0667)) < 1e-4
    got5 = [g for a, n, m, g in rows if a == 1.0 / 16 and n == 5][0]
    assert abs(got5 - 45.87) < 0.01


def small_set(seed=3, I=6, K=8, n_max=120):
    rng = np.random.default_rng(seed)
    n = rng.integers(2, n_max, size=I * K)
    t = np.minimum(n, 1 + rng.integers(0, np.maximum(1, (n ** 0.6).astype(np.int64))))
    T = t.reshape(I, K).sum(axis=1)
    return n, t, T, np.full(I, 5.0)


@pytest.fixture(scope="module")
def peaked():
    n, t, T, b = small_set()
    fn = lambda xs: hd.grad_many(xs, n, t, T, b)
    root = hd.bisect_root(fn, 0.02, 0.95, 1e-12)
    return fn, root


@pytest.mark.parametrize("Dmax", [8, 3])
def test_modea_replay_finds_the_root(peaked, Dmax):
    fn, root = peaked
    tol = 1e-6
    r = hd.modea_replay(fn, 0.02, 0.95, tol, 40, Dmax)
    assert r["at_bound"] == 0 and r["hi"] - r["lo"] <= tol
    assert r["lo"] <= root <= r["hi"] and abs(r["a_hat"] - root) <= tol
    assert r["g_lo"] > 0 >= r["g_hi"] and r["curv"] < 0
    if Dmax == 8:
        assert r["rounds"] <= 7   # a factor 7, then 9 a round


def test_modea_replay_on_each_bound(peaked):
    fn, root = peaked
    lo = hd.modea_replay(fn, root + 0.05, 0.9, 1e-6, 40, 8)
    assert lo["at_bound"] == -1 and lo["a_hat"] == root + 0.05 and lo["rounds"] == 1 and lo["evals"] == 11
    hi = hd.modea_replay(fn, 0.05, root - 0.05, 1e-6, 40, 8)
    assert hi["at_bound"] == 1 and hi["a_hat"] == root - 0.05 and hi["rounds"] == 1


def test_restaurant_term_derivative_is_the_terms_slope():
    """hd.restaurant_term_da against a central difference of hp.restaurant_term at 40 digits"""
    mp = hp._mp()
    for x, T, b in ((0.3, 5, 2.0), (0.7, 200, 0.01), (0.05, 1, 1e3), (0.5, 0, 4.0)):
        h = mp.mpf(10) ** -12
        f = lambda y: T * mp.log(y) + mp.loggamma(T + b / y) - mp.loggamma(b / y)
        num = (f(mp.mpf(x) + h) - f(mp.mpf(x) - h)) / (2 * h)
        val, bar = hd.restaurant_term_da(x, T, b)
        assert abs(val - num) <= mp.mpf(10) ** -15 * max(1, abs(num))
