"""tests/lj_oracle.py, the truth the device's log joint is held to (tests/test_gpu_logjoint.py), checked on the CPU: its
cells against exact integers, its differences against the conditionals the two t-samplers draw from (tc_oracle's weights,
ti_oracle's odds), and its total at a shared concentration against W + R of hj_oracle."""
import math

import numpy as np
import pytest

import hj_oracle as hj
import hp_oracle as hp
import lj_oracle as lj
import orc
import tc_oracle as tco
import ti_oracle as tio

LD = np.longdouble
U = hp.U
N48 = 48


def state(seed, I, Kmax, nmax, M):
    """a valid state: n in 0 .. nmax, t = 0 exactly when n = 0, else 1 <= t <= min(n, M); n = 1, t = 1, t = n among them"""
    rng = np.random.default_rng(seed)
    K = rng.integers(0, Kmax + 1, size=I).astype(np.int32)
    K[0] = Kmax
    G = int(K.sum())
    n = rng.integers(0, nmax + 1, size=G).astype(np.uint32)
    n[:4] = [0, 1, nmax, nmax]
    tm = np.minimum(n, M)
    t = np.where(n > 0, 1 + np.floor(rng.random(G) * tm), 0).astype(np.uint16)
    t[2], t[3] = 1, min(nmax, M)
    h = 0.05 + 0.95 * rng.random(G)
    return K, n, t, h


@pytest.mark.parametrize("M", [48, 7])
@pytest.mark.parametrize("a", [0.0, 0.125, 0.5, 0.9])
def test_long_double_pair_sums_equal_the_exact_integers(a, M):
    K, n, t, h = state(3, 6, 40, N48, M)
    tabs = lj.Tables(a, N48, M)
    tr = lj.truth(K, n, t, None, a, 1.0, tabs)
    exact = {}
    for r, k, row in hp.exact_rows(a, N48, M):
        for m in range(1, len(row)):
            if row[m] > 0:
                exact[(r, m)] = hp.exact_log(row[m], -k * (r - m))
    koff = np.concatenate([[0], np.cumsum(K)])
    worst = 0.0
    for i in range(len(K)):
        P = LD(0)
        for g in range(koff[i], koff[i + 1]):
            if n[g] >= 1 and t[g] != n[g]:
                P += exact[(int(n[g]), int(t[g]))]
        e = abs(float(P - tr["P_ld"][i]))
        assert e <= tr["P_bar"][i] / 100.0, (i, e, tr["P_bar"][i])
        worst = max(worst, e / max(tr["P_bar"][i], 1e-300))
    assert worst <= 0.01


def _float_tables(a, N, M):
    S1, S, _ = hp.tables([a], N, M)[0]
    assert all(orc.row_offset(r, M) == hp._s_rowoff(r, M) for r in range(3, N + 1))
    return S1.astype(np.float64), S.astype(np.float64)


@pytest.mark.parametrize("a,b", [(0.0, 2.0), (0.125, 1e-3), (0.5, -0.25), (0.9, 1e3)])
@pytest.mark.parametrize("M", [48, 7])
def test_one_pair_moves_the_joint_by_the_ratio_of_the_sweeps_weights(a, b, M):
    """L(t_k = tau') - L(t_k = tau) = log w(tau') - log w(tau), w the weights stb_sample_tcounts draws from.  Both sides
    see the same cells (the truth rounded to doubles); tc_oracle forms log w in doubles -- a cumulative sum of up to
    tmax log terms plus two more terms, every operation rounding by at most u times A = the sum of the terms'
    magnitudes -- so the two sides differ by at most 2 (tmax + 3) u A + 2 u |difference|."""
    K, n, t, h = state(5, 3, 9, N48, M)
    S1, S = _float_tables(a, N48, M)
    tabs = lj.Tables(a, N48, M, S1=S1.astype(LD), S=S.astype(LD))
    bpar = np.full(len(K), b)
    base = lj.truth(K, n, t, h, a, bpar, tabs)
    koff = np.concatenate([[0], np.cumsum(K)])
    checked = 0
    for i in range(len(K)):
        for g in range(koff[i], koff[i + 1]):
            tmax = min(int(n[g]), M)
            if tmax < 2:
                continue
            Tm = int(base["T"][i]) - int(t[g])
            lw = tco.log_weights(int(n[g]), Tm, a, b, float(h[g]), M, S1, S, M)
            A = (np.abs(np.log(b + (Tm + np.arange(1, tmax)) * a)).sum() + np.abs(S1[n[g] - 1]) + np.abs(lw).max()
                 + tmax * abs(math.log(h[g])))
            for tau in {1, tmax, 1 + (int(t[g]) + 2) % tmax}:
                t2 = t.copy()
                t2[g] = tau
                moved = lj.truth(K, n, t2, h, a, bpar, tabs)
                d = float(moved["total_mp"] - base["total_mp"])
                want = lw[tau - 1] - lw[int(t[g]) - 1]
                assert abs(d - want) <= 2 * (tmax + 3) * U * A + 2 * U * abs(want), (g, tau, d, want)
                checked += 1
    assert checked >= 20


@pytest.mark.parametrize("a,b", [(0.0, 2.0), (0.125, 1e-3), (0.5, -0.25), (0.9, 1e3)])
def test_one_indicator_moves_the_indicator_joint_by_the_sweeps_odds(a, b):
    """with the binomial part, L(t_k + 1) - L(t_k) = log of stb_sample_tindic's odds h (b + T a) t / (n - t) V^n_{t+1}.
    ti_oracle forms the odds in doubles from five operations (6 u relative with V's own rounding) and the log rounds
    once more: 16 u (1 + |log odds|) covers it."""
    M = N48
    K, n, t, h = state(7, 3, 9, N48, M)
    tabs = lj.Tables(a, N48, M)
    bpar = np.full(len(K), b)
    base = lj.truth(K, n, t, h, a, bpar, tabs, indicators=True)
    koff = np.concatenate([[0], np.cumsum(K)])
    checked = 0
    for i in range(len(K)):
        for g in range(koff[i], koff[i + 1]):
            ng, tg = int(n[g]), int(t[g])
            if ng < 2 or tg >= ng:
                continue
            V = float(np.exp(tabs.cell(ng, tg + 1)[0] - tabs.cell(ng, tg)[0]))
            o = tio.odds(ng, tg, int(base["T"][i]), float(h[g]), a, b, V, False)
            t2 = t.copy()
            t2[g] = tg + 1
            moved = lj.truth(K, n, t2, h, a, bpar, tabs, indicators=True)
            d = float(moved["total_mp"] - base["total_mp"])
            assert abs(d - math.log(o)) <= 16 * U * (1 + abs(d)), (g, d, math.log(o))
            checked += 1
    assert checked >= 10


@pytest.mark.parametrize("a,b", [(0.125, 1e-3), (0.5, 1.0), (0.9, 1e3)])
def test_total_at_a_shared_concentration_is_W_plus_R(a, b):
    """h = 1, one b: the total is hj_oracle's W(a) + R(a, b).  That side sums in long double: one rounding of 2^-64
    relative per addition and per log, G + sum T + sum N + 8 I operations on partial sums of at most the terms'
    magnitudes together."""
    K, n, t, _ = state(11, 40, 6, N48, N48)
    tabs = lj.Tables(a, N48, N48)
    tr = lj.truth(K, n, t, None, a, b, tabs)
    W = hj.W_truth([a], n, t)[0]
    R = hj.R_points([a], [b], tr["T"], tr["Nc"])[0]
    hi = float(tr["total_mp"])
    got = LD(hi) + LD(float(tr["total_mp"] - hi))
    ops = len(n) + int(tr["T"].sum()) + int(tr["Nc"].sum()) + 8 * len(K)
    mag = abs(float(tr["pairs"][0])) + sum(abs(float(lj.restaurant_term(a, b, int(T), int(Nc))[0])) + 2 * abs(
        float(hj._rise(LD(b), int(Nc)))) for T, Nc in zip(tr["T"], tr["Nc"]))
    assert abs(float(got - (W + R))) <= 2.0 ** -62 * ops * mag


def test_impossible_and_outside_pairs_are_classified_as_the_kernel_does():
    tabs = lj.Tables(0.5, 10, 4)
    K = np.array([6, 3], dtype=np.int32)
    n = np.array([5, 5, 0, 11, 9, 9, 4, 4, 0], dtype=np.uint32)
    t = np.array([0, 6, 2, 3, 5, 9, 2, 1, 0], dtype=np.uint16)
    h = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.5, 1.0])
    tr = lj.truth(K, n, t, h, 0.5, [1.0, 2.0], tabs)
    assert tr["impossible"] == 4 and tr["outside"] == 2
    assert tr["Li"][0] == -math.inf and tr["Li"][1] == -math.inf and tr["total"][0] == -math.inf
    assert tr["pairs"][0] == -math.inf and tr["base"][0] == -math.inf and math.isfinite(tr["restaurants"][0])
    assert list(tr["T"]) == [25, 3] and list(tr["Nc"]) == [39, 8]


def test_a_tiled_truth_equals_the_truth_of_the_state_written_out():
    """truth(mult=...) -- what the device's sums over 10^6 restaurants are held to -- against the same restaurants one by one"""
    a, M = 0.5, 7
    K, n, t, h = state(11, 7, 5, N48, M)
    n[5], t[5] = 60, 3      # outside
    n[9], t[9] = 4, 5       # impossible
    bpar = np.array([1e-3, 1.0, 1e3, -0.25, 2.0, 0.5, 7.0])
    tabs = lj.Tables(a, N48, M)
    mult = np.array([3, 0, 1, 4, 2, 1, 5])
    tiled = lj.truth(K, n, t, h, a, bpar, tabs, True, mult=mult)
    koff = np.concatenate([[0], np.cumsum(K)])
    idx = np.repeat(np.arange(len(K)), mult)
    pick = np.concatenate([np.arange(koff[i], koff[i + 1]) for i in idx]).astype(np.int64)
    full = lj.truth(K[idx], n[pick], t[pick], h[pick], a, bpar[idx], tabs, True)
    assert tiled["outside"] == full["outside"] and tiled["impossible"] == full["impossible"]
    assert tiled["outside"] + tiled["impossible"] > 0
    for name in ("pairs", "base", "restaurants", "binom", "total"):
        (v1, b1), (v2, b2) = tiled[name], full[name]
        assert (v1 == v2 or abs(v1 - v2) <= 4 * U * abs(v2)) and abs(b1 - b2) <= 1e-12 * b2, (name, tiled[name], full[name])
    assert abs(float(tiled["total_mp"] - full["total_mp"])) <= 1e-25 * abs(float(full["total_mp"]))
    # and without multiplicities nothing changed
    one = lj.truth(K, n, t, h, a, bpar, tabs, True, mult=np.ones(len(K), dtype=np.int64))
    ref = lj.truth(K, n, t, h, a, bpar, tabs, True)
    assert all(one[k] == ref[k] for k in ("pairs", "base", "restaurants", "binom", "total", "outside", "impossible"))
