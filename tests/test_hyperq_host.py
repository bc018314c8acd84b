"""The law of the device draw of -log q_i (stb_sample_logq), checked on its numpy replay (tests/hq_oracle.py): closed-form
moments, Kolmogorov distances where the CDF is elementary, and the replay's own sensitivity to the last bit of its
transcendentals.  CPU only.  The seeds are fixed: a failure at a seed is a bug."""
import math

import numpy as np
import pytest

import hq_oracle as hq


def test_digamma_and_trigamma_are_pinned():
    assert abs(hq.digamma(1.0) + 0.5772156649015329) < 1e-14
    assert abs(hq.trigamma(1.0) - math.pi ** 2 / 6) < 1e-14
    # recurrences: psi(x+1) = psi(x) + 1/x, psi'(x+1) = psi'(x) - 1/x^2, also where only the series is used
    for x in (0.01, 0.5, 3.3, 12.5, 2000.0, 1e5):
        assert abs(hq.digamma(x + 1) - hq.digamma(x) - 1 / x) < 1e-13 * max(1.0, 1 / x)
        assert abs(hq.trigamma(x + 1) - hq.trigamma(x) + 1 / x ** 2) < 1e-13 * max(1.0, 1 / x ** 2)
    assert abs(hq.digamma(0.5) + 2 * math.log(2) + 0.5772156649015329) < 1e-14
    assert abs(hq.trigamma(0.5) - math.pi ** 2 / 2) < 1e-13


def test_uniforms_are_inside_the_open_interval_and_follow_the_projects_stream():
    from libstb_amd import synth

    key = hq.sweep_key(5, 0)
    ki = np.full(1000, hq.mix(np.array([key]) + hq.GAMMA)[0], dtype=np.uint64)
    u = hq.unit(ki, np.arange(1, 1001, dtype=np.uint64))
    assert (u > 0).all() and (u < 1).all()
    # restaurant 0's substream is splitmix64 seeded with key_0: the generator of synth.unit
    assert np.array_equal(u, synth.unit(1000, int(ki[0])))


@pytest.mark.parametrize("b", [0.01, 0.5, 1.0, 10.0, 2000.0])
@pytest.mark.parametrize("N", [1, 7, 200, 10 ** 5])
def test_moments_of_L_match_the_closed_forms(b, N):
    n = 10 ** 6
    L = hq.replay_L(b, np.full(n, N, dtype=np.uint64), seed=20240 + N, sweep=int(b * 100))
    assert np.isfinite(L).all() and (L > 0).all()
    ok, text = hq.moment_check(L, b, N)
    print(text)
    assert ok, text


@pytest.mark.parametrize("b", [0.01, 0.3, 0.9])
def test_kolmogorov_for_one_customer(b):
    """N = 1: P(q <= x) = x^b, so exp(-b L) is uniform; b < 1 takes the boosted branch"""
    n = 10 ** 5
    L = hq.replay_L(b, np.ones(n, dtype=np.uint64), seed=77, sweep=3)
    d = hq.ks_stat(np.exp(-b * L))
    print("b=%g N=1: sqrt(n) D = %.3f" % (b, d))
    assert d <= 2.2


@pytest.mark.parametrize("N", [1, 7, 200, 10 ** 5])
def test_kolmogorov_for_b_equal_one(N):
    """b = 1: P(q <= x) = 1 - (1 - x)^N"""
    n = 10 ** 5
    L = hq.replay_L(1.0, np.full(n, N, dtype=np.uint64), seed=78, sweep=N)
    p = -np.expm1(N * np.log(-np.expm1(-L)))
    d = hq.ks_stat(p)
    print("b=1 N=%d: sqrt(n) D = %.3f" % (N, d))
    assert d <= 2.2


@pytest.mark.parametrize("b", [0.01, 0.7, 10.0, 2000.0])
def test_the_replay_does_not_hinge_on_the_last_bit_of_its_transcendentals(b):
    """The device's log / cos may differ from numpy's in the last bit, which can flip an accept test and change a
    restaurant's value altogether.  The GPU test allows 1 restaurant in 10^5 for that; here the replay run with float64 and
    with longdouble transcendentals must itself stay inside that allowance on the same inputs (where longdouble is no wider
    than float64 the two runs coincide)."""
    I = 2 * 10 ** 5
    N = hq.mixed_restaurants(I)
    L64 = hq.replay_L(b, N, seed=9001, sweep=11)
    Lld = hq.replay_L(b, N, seed=9001, sweep=11, dtype=np.longdouble)
    assert (L64[N == 0] == 0).all() and (L64[N > 0] > 0).all()
    out = np.abs(L64 - Lld) > 1e-12 * np.maximum(1.0, np.abs(Lld))
    print("b=%g: %d of %d restaurants outside 1e-12" % (b, int(out.sum()), I))
    assert out.sum() <= I // 10 ** 5


def test_draws_depend_on_seed_sweep_and_index_alone():
    N = hq.mixed_restaurants(5000)
    whole = hq.replay_L(0.4, N, seed=5, sweep=2)
    part = hq.replay_L(0.4, N[1234:2000], seed=5, sweep=2, first=1234)
    assert np.array_equal(whole[1234:2000], part)
    assert not np.array_equal(whole, hq.replay_L(0.4, N, seed=5, sweep=3))
    assert not np.array_equal(whole, hq.replay_L(0.4, N, seed=6, sweep=2))
