"""The per-group concentration step on the CPU: the two identities its augmentation rests on (mpmath), the replay's own
pieces against hq_oracle, the replay's chain against the posterior by quadrature -- with the two wrong laws it must tell
apart --, and the seeds of the device tests (tests/test_gpu_bgroups.py), chosen here so that no decision of a replayed
draw hangs on a last bit."""
import itertools
import math

import numpy as np
import pytest

import hb_oracle as hb
import hq_oracle as hq

LAW_N, LAW_START, LAW_SEED = 20000, 1, 100   # restaurants, the start's generator, the steps' seed (the device test's too)


# ---- the identities

@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
def test_summing_out_y_gives_the_rising_factorial(T):
    import mpmath as mp
    mp.mp.dps = 40
    for a, b in ((mp.mpf("0.5"), mp.mpf("2.25")), (mp.mpf("0.9"), mp.mpf("0.01")), (mp.mpf(0), mp.mpf(7))):
        want = mp.mpf(1)
        for k in range(T):
            want *= b + k * a
        got = mp.mpf(0)
        for y in itertools.product((0, 1), repeat=T - 1):
            term = b ** (1 + sum(y))   # (the k = 0 factor is b itself)
            for k, yk in enumerate(y, start=1):
                term *= (k * a) ** (1 - yk)
            got += term
        assert abs(got - want) <= mp.mpf(10) ** -30 * abs(want)


@pytest.mark.parametrize("N", [1, 2, 7, 40])
def test_the_beta_integral(N):
    import mpmath as mp
    mp.mp.dps = 80
    for b in (mp.mpf("0.3"), mp.mpf("2.25"), mp.mpf(50)):
        # (1 - q)^(N-1) expanded and integrated term by term against q^(b-1): a finite sum, exact up to the working precision
        got = sum(mp.binomial(N - 1, j) * (-1) ** j / (b + j) for j in range(N))
        want = mp.gamma(b) * mp.gamma(N) / mp.gamma(b + N)
        assert abs(got - want) <= mp.mpf(10) ** -15 * want


# ---- the replay's pieces

def test_L_with_equal_b_is_hq_oracles():
    N = hq.mixed_restaurants(5000)
    for b in (0.01, 0.7, 10.0):
        assert np.array_equal(hb.replay_L(np.full(5000, b), N, 9001, 11), hq.replay_L(b, N, seed=9001, sweep=11))


@pytest.mark.parametrize("n", [1, 2, 63, 255, 256, 257, 513, 16384, 16385, 256 * 64 + 257, 512 * 256 + 257, 140001])
def test_the_group_sum(n):
    L = hq.replay_L(0.7, hq.mixed_restaurants(max(n, 8))[:n], seed=3, sweep=1)
    inv = 1.0 / 20.0
    got = hb.group_rate(L, inv)
    want = math.fsum(L) + inv
    assert abs(got - want) <= 4 * 2.0 ** -53 * n * abs(want)
    if n == 1:
        assert got == L[0] + inv


def test_a_zero_discount_counts_every_table():
    T, N, b, _ = hb.replay_case("each")
    assert np.array_equal(hb.replay_Y(0.0, b, T, 1, 0), T)
    Y = hb.replay_Y(0.9, b, T, 1, 0)
    assert ((Y <= T) & (Y >= (T >= 1))).all() and (Y < T).any()


# ---- the law

def _p(case, steps, law="right", group=1):
    b, post = hb.chain(case, LAW_N, steps, LAW_START, LAW_SEED, law=law, group=group)
    return hb.ks_pvalue(post.F(b))


@pytest.mark.parametrize("case", hb.CASES)
def test_the_chain_holds_the_posterior_and_the_wrong_laws_do_not(case):
    p1, p3 = _p(case, 1), _p(case, 3)
    print("%s: p = %.3g after one step, %.3g after three" % (case, p1, p3))
    assert p1 > 1e-3 and p3 > 1e-3
    pf = _p(case, 1, "no_first")
    print("  the k = 0 factor dropped: p = %.3g" % pf)
    assert pf < 1e-9
    if case[2] > 0:
        pk = _p(case, 1, "no_k")
        print("  k dropped from b + k a: p = %.3g" % pk)
        assert pk < 1e-9


def test_one_group_of_four_restaurants_holds_the_product_posterior():
    p1, p3 = _p(hb.GROUP4, 1, group=4), _p(hb.GROUP4, 3, group=4)
    print("group of four: p = %.3g after one step, %.3g after three" % (p1, p3))
    assert p1 > 1e-3 and p3 > 1e-3
    assert _p(hb.GROUP4, 1, "no_first", 4) < 1e-9 and _p(hb.GROUP4, 1, "no_k", 4) < 1e-9


# ---- the device tests' seeds

@pytest.mark.parametrize("a", sorted(hb.REPLAY_SEEDS))
@pytest.mark.parametrize("grouping", ["each", "one", "ragged"])
def test_the_replay_seeds_leave_every_decision_a_margin(a, grouping):
    T, N, b, goff = hb.replay_case(grouping)
    assert set(T.tolist()) == set(hb.REPLAY_T) and (N >= T).all() and ((N == 0) == (T == 0)).all()
    shape, scale = hb.REPLAY_PRIOR
    r = hb.replay(a, shape, scale, T, N, b, goff, hb.REPLAY_SEEDS[a], hb.REPLAY_SWEEP)
    print("a=%g %s: smallest margin %.2e (variates), %.2e (Bernoulli); kept %d" % (a, grouping, r["margin_gamma"], r["margin_y"], r["kept"]))
    assert r["margin_gamma"] > 1e-9 and r["margin_y"] > 1e-9 and r["kept"] == 0
    # the transcendentals in long double move no decision: the same Y, L within the device test's bar
    rl = hb.replay(a, shape, scale, T, N, b, goff, hb.REPLAY_SEEDS[a], hb.REPLAY_SWEEP, dtype=np.longdouble)
    assert np.array_equal(rl["Y"], r["Y"])
    assert (np.abs(rl["L"] - r["L"]) <= 1e-12 * np.maximum(1.0, r["L"])).all()
    assert (np.abs(rl["bgrp"] - r["bgrp"]) <= 1e-10 * r["bgrp"]).all()
