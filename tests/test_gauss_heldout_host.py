"""The held-out predictive density under Gaussian observations, on the host: the numpy replay of the device's operations
(tests/gh_oracle.py) against the 40-digit truth within the derived bars, the log-domain accumulator where the linear one
returns -inf, the normalisation by quadrature with the mutations that break it, the empty restaurant, and the law of the
running estimate on gs_oracle's tiny chain against the enumerated p(y | x)."""
import math

import numpy as np
import pytest

import gh_oracle as gho
import gs_oracle as gso


# ---- 1. the replay within its bar of the truth ----

@pytest.mark.parametrize("name", list(gho.SHAPES))
def test_the_replay_lies_within_its_bar_of_the_truth(name):
    c, tr = gho.make_case(name), gho.case_truth(name)
    rep = tr["replay"]
    poss = np.isfinite(tr["ell"])
    assert np.array_equal(poss, ~rep["dead"]) and np.array_equal(poss, np.isfinite(rep["ell"]))
    if c["y"].shape[0] > 3:
        assert not poss[2] and np.all(rep["resp"][2] == 0.0)                 # the impossible point
    if c["K"] > 1:                                                          # the nearest dish has theta = 0
        assert poss[0] and np.argmax(rep["l"][0]) == 1 and rep["resp"][0, 1] == 0.0 and rep["m"][0] < rep["l"][0, 1]
    share = np.abs(rep["ell"][poss] - tr["ell"][poss]) / tr["ell_bar"][poss]
    rshare = np.abs(rep["resp"] - tr["resp"])[poss] / np.maximum(tr["resp_bar"][poss], 1e-320)
    assert np.all(np.abs(rep["resp"][poss].sum(axis=1) - 1.0) < 64 * c["K"] * gho.U + 1e-13)
    Hi, total, nimp = gho.total_of_ell(rep["ell"], c["hoff"])
    assert nimp == int((~poss).sum()) and np.array_equal(np.isinf(Hi), np.isinf(tr["Hi"]))
    # the sums of the possible points (an impossible one makes H_i and the total -inf: compared above)
    ell0 = np.where(poss, rep["ell"], 0.0)
    Hs, ts, _ = gho.sum_x(ell0, np.ones_like(poss), c["hoff"])
    mp = gho._mp()
    tot_true = float(mp.fsum(v for v in tr["ell_mp"] if v is not None))
    Hi_true = np.array([float(mp.fsum(v for v in tr["ell_mp"][int(c["hoff"][i]):int(c["hoff"][i + 1])] if v is not None))
                        for i in range(c["I"])])
    hshare = np.abs(Hs - Hi_true) / np.maximum(tr["Hi_bar"], 1e-320)      # (an empty restaurant: 0 of a bar of 0)
    tshare = abs(ts - tot_true) / tr["total_bar"]
    print(name, "largest share of the bar: ell", share.max(initial=0.0), "resp", rshare.max(initial=0.0), "H_i", hshare.max(),
          "total", tshare)
    assert share.max(initial=0.0) <= 1.0 and rshare.max(initial=0.0) <= 1.0 and hshare.max() <= 1.0 and tshare <= 1.0


# ---- 2. the accumulator ----

def _orders(S, base):
    rng = np.random.default_rng(S)
    v = base + np.sort(rng.normal(0.0, 30.0, size=S))
    mixed = v[rng.permutation(S)]
    return {"rising": v, "falling": v[::-1].copy(), "mixed": mixed}


@pytest.mark.parametrize("S", [1, 2, 7])
@pytest.mark.parametrize("base", [-5.0, -3000.0])
def test_the_accumulator_is_the_log_mean_exp(S, base):
    mp = gho._mp()
    worst = 0.0
    for order, v in _orders(S, base).items():
        for holes in (False, True):
            ells = v.copy()
            if holes and S > 1:
                ells[1] = -math.inf
            M, A = gho.acc_empty(1)
            for e in ells:
                M, A = gho.acc_update(M, A, np.array([e]))
            x, ok = gho.acc_x(M, A, S)
            col = [[None if e == -math.inf else mp.mpf(float(e))] for e in ells]
            tr = gho.acc_truth(col, [[0.0]] * S)
            assert ok[0] and M[0] == max(ells)
            share = abs(x[0] - tr["x"][0]) / tr["x_bar"][0]
            worst = max(worst, share)
            assert share <= 1.0, (order, holes, x[0], tr["x"][0], tr["x_bar"][0])
            if base < -1000.0:                                  # why the log domain: every exp(ell) is 0 in a double
                assert gho.naive_linear(ells) == -math.inf and math.isfinite(x[0])
    print("S", S, "base", base, "largest share of the bar", worst)


def test_an_accumulator_of_impossible_states_stays_empty():
    M, A = gho.acc_empty(2)
    M, A = gho.acc_update(M, A, np.array([-math.inf, -7.0]))
    M, A = gho.acc_update(M, A, np.array([-math.inf, -math.inf]))
    x, ok = gho.acc_x(M, A, 2)
    assert M[0] == -math.inf and A[0] == 0.0 and not ok[0] and ok[1] and (M[1], A[1]) == (-7.0, 1.0)
    Hi, total, nimp = gho.sum_x(x, ok, [0, 1, 2])
    assert nimp == 1 and Hi[0] == -math.inf and total == -math.inf and Hi[1] == -7.0 + math.log(0.5)


# ---- 3. the normalisation ----

def _quad_case():
    K = 3
    n = np.array([4, 0, 2], dtype=np.uint32)
    t = np.array([2, 0, 1], dtype=np.uint16)
    h = np.array([0.5, 0.2, 0.3])                      # sums to 1: theta does too
    mu = np.array([[-1.0], [0.7], [2.5]])
    tau = np.array([[4.0], [0.5], [9.0]])
    return K, n, t, h, 0.3, np.array([1.2]), mu, tau


def _integral(grid, **kw):
    K, n, t, h, a, bpar, mu, tau = _quad_case()
    th = gho.theta_of(K, n, t, h, a, bpar, mut=kw.get("theta"))
    hoff = np.array([0, grid.size])
    p = np.exp(gho.points(th, K, hoff, grid.reshape(-1, 1), mu, tau, mut=kw.get("mut"))["ell"])
    return float(((p[1:] + p[:-1]) * 0.5 * np.diff(grid)).sum())


def test_the_density_integrates_to_one_and_the_mutations_do_not():
    grid = np.linspace(-40.0, 40.0, 160001)
    # the trapezoid rule on an analytic integrand whose tails are below 1e-100 at the ends converges faster than any
    # power of the step; with step 5e-4 against a narrowest sigma of 1/3 its error is far below the rounding of the sum,
    # 160001 u: 1e-10 covers both with room
    tol = 1e-10
    right = _integral(grid)
    assert abs(right - 1.0) < tol, right
    wrong = {"noconst": _integral(grid, mut="noconst"), "variance": _integral(grid, mut="variance"),
             "h": _integral(grid, theta="h")}
    print(right, wrong)
    assert abs(wrong["noconst"] - math.sqrt(2.0 * math.pi)) < 1e-9
    assert abs(wrong["variance"] - 1.0) > 0.1
    assert abs(wrong["h"] - 1.0) < tol                  # h sums to 1 as well: the integral cannot tell theta from h ...
    K, n, t, h, a, bpar, mu, tau = _quad_case()
    y = np.array([[-1.0]])
    pt = [math.exp(gho.points(gho.theta_of(K, n, t, h, a, bpar, mut=m), K, [0, 1], y, mu, tau)["ell"][0]) for m in (None, "h")]
    assert abs(pt[0] - pt[1]) > 0.05 * pt[0]            # ... the density at a dish with customers does


def test_the_maximum_over_every_dish_loses_a_point_beside_a_dish_without_weight():
    # dish 0 has theta = 0 and sits on the point; the dishes with weight are 45 away: their l is 1000 below dish 0's, the
    # plain maximum underflows every term and the point comes out impossible.  (In D = 1 the mass there is e^-1000: no
    # quadrature can show it; the log density does.)
    K = 3
    n, t = np.array([0, 3, 2], dtype=np.uint32), np.array([0, 1, 1], dtype=np.uint16)
    h = np.array([0.0, 0.6, 0.4])
    mu, tau = np.array([[0.0], [45.0], [-45.0]]), np.ones((3, 1))
    th = gho.theta_of(K, n, t, h, 0.3, np.array([1.0]))
    y = np.array([[0.0]])
    right = gho.points(th, K, [0, 1], y, mu, tau)
    wrong = gho.points(th, K, [0, 1], y, mu, tau, mut="maxall")
    tr = gho.truth(K, n, t, h, 0.3, np.array([1.0]), [0, 1], y, mu, tau)
    assert abs(right["ell"][0] - tr["ell"][0]) <= tr["ell_bar"][0] and -1020.0 < tr["ell"][0] < -1000.0
    assert wrong["ell"][0] == -math.inf and right["resp"][0, 0] == 0.0 and abs(right["resp"][0].sum() - 1.0) < 1e-15


# ---- 4. an empty restaurant ----

def test_an_empty_restaurant_of_one_dish_scores_the_point_under_that_dish():
    rng = np.random.default_rng(8)
    D = 5
    mu, tau, y = rng.normal(size=(1, D)), 0.5 + rng.random((1, D)), rng.normal(size=(1, D))
    n, t = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint16)
    th = gho.theta_of(1, n, t, None, 0.3, np.array([1.0]))
    assert th[0, 0] == 1.0
    ell = gho.points(th, 1, [0, 1], y, mu, tau)["ell"][0]
    want, _ = gso.loglik(y, np.zeros(1, dtype=np.int64), mu, tau)
    tr = gho.truth(1, n, t, None, 0.3, np.array([1.0]), [0, 1], y, mu, tau)
    assert abs(ell - want) <= tr["ell_bar"][0] + gso.loglik_bar(y, np.zeros(1, dtype=np.int64), mu, tau)
    assert abs(ell - tr["ell"][0]) <= tr["ell_bar"][0]


# ---- 5. the law ----

@pytest.fixture(scope="module")
def right_chain():
    return gho.law_chain("right")


def test_the_running_estimate_has_the_enumerated_law(right_chain):
    exact = gho.law_exact()
    mean, se = gho.batch_se(right_chain)
    z = (mean - np.array(exact)) / se
    print("exact", exact, "mean", mean, "se", se, "z", z)
    assert np.all(np.abs(z) < gho.LAW_Z)
    # the log-domain accumulator over the same iterations is that mean
    M, A = gho.acc_empty(2)
    for s in range(gso.CHAIN["burn"], right_chain.shape[0]):
        M, A = gho.acc_update(M, A, np.log(right_chain[s]))
    x, ok = gho.acc_x(M, A, right_chain.shape[0] - gso.CHAIN["burn"])
    assert np.all(ok) and np.allclose(np.exp(x), mean, rtol=1e-9)


@pytest.mark.parametrize("law", ["h", "stale"])
def test_a_wrong_scoring_is_told_apart(law, right_chain):
    exact = np.array(gho.law_exact())
    _, se = gho.batch_se(right_chain)                    # the bar is the right chain's
    mean, _ = gho.batch_se(gho.law_chain(law))
    z = (mean - exact) / se
    print(law, "mean", mean, "z", z)
    assert np.max(np.abs(z)) > gho.LAW_Z
