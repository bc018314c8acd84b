"""The particle filter of the forward seating (stb_seat_filter, libstb_amd/csrc/seat_pf.hip) judged on the CPU: the
estimate is unbiased by exact enumeration, resampling triggered by the effective sample size included; a filter that
never resamples is the sequential seating; the numpy replay (tests/pf_oracle.py) lies within the derived bar of the
40-digit truth and wrong replays do not; the rescaling by powers of two is invisible.  The device is held to the replay
by bit-equality in tests/test_gpu_pf.py."""
import math

import numpy as np
import pytest

import pf_oracle as pf
import st_oracle as sto

# a rare dish 0 that the second customer's class all but demands: a slot whose first customer opened it outweighs one
# whose first customer did not by more than 10 to 1 (the trigger at tau = 0.6 and R = 2), two alike stay 1 to 1
HS = (0.02, 0.98)
LIK = ((0.9, 0.02), (0.9, 0.001))
CLS3 = (0, 1, 0)
PARAMS = ((0.3, 1.5, 4), (0.0, 2.0, 4), (0.9, -0.5, 4), (0.5, 1.0, 2))
A0, R0, TAU0 = 0.5, 3, 0.5


@pytest.mark.parametrize("tau", (0.0, 0.6, 1.0))
@pytest.mark.parametrize("a,b,M", PARAMS)
def test_the_estimate_is_unbiased_by_enumeration(a, b, M, tau):
    PZ, P, resampled, plain = pf.enumerate_filter(HS, a, b, CLS3, LIK, M, tau)
    want = float(sto.ujoint_states(3, 2, HS, a, b, CLS3, LIK, M).sum())
    assert abs(P - 1.0) <= 1e-12
    assert abs(PZ - want) <= 1e-12 * want, (PZ, want)
    if tau == 0.0:
        assert resampled == 0
    if tau == 0.6:                       # the trigger decides: some branches resample and some do not
        assert resampled > 0 and plain > 0, (resampled, plain)
    if tau == 1.0:
        assert resampled > 0


def test_a_filter_that_never_resamples_is_the_sequential_seating():
    K, n, t, h, bpar, coff, cls, lik = pf.host_case()
    koff = np.concatenate([[0], np.cumsum(K)])
    for R in (1, 3):
        rp = pf.replay(K, n, t, h, A0, bpar, coff, cls, lik, 0, pf.SEED, pf.SWEEP, R, 0.0)
        assert rp["resamplings"] == 0 and rp["skipped"] == 0
        for r in range(R):                # slot r is particle r of k_seat: the stream of sweep + r
            so = sto.replay(K, n, t, h, A0, bpar, coff, cls, lik, 0, pf.SEED, pf.SWEEP + r, 1)
            for i in range(len(K)):
                sl = slice(int(koff[i]) * R + r * int(K[i]), int(koff[i]) * R + (r + 1) * int(K[i]))
                assert np.array_equal(rp["pn"][sl], so["n"][koff[i]:koff[i + 1]]), (R, r, i)
                assert np.array_equal(rp["pt"][sl], so["t"][koff[i]:koff[i + 1]]), (R, r, i)
        sr = sto.replay(K, n, t, h, A0, bpar, coff, cls, lik, 0, pf.SEED, pf.SWEEP, R, bars=True)
        tr = sto.truth(K, n, t, h, A0, bpar, coff, cls, lik, 0, sr)
        tHi, tHb, _, _ = sto.loglik_truth(tr, range(len(K)), R)
        _, Ht, Hb = pf.truth(K, n, t, h, A0, bpar, coff, cls, lik, 0, pf.SEED, pf.SWEEP, R, 0.0)
        for i in range(len(K)):
            # both are estimates of the same log mean weight: each within its own bar of its truth, the truths equal
            assert sto.within(rp["H"][i], Ht[i], Hb[i]) and sto.within(rp["H"][i], tHi[i], tHb[i] + Hb[i]), (R, i)


def test_the_replay_lies_within_its_bar_of_the_truth():
    K, n, t, h, bpar, coff, cls, lik = pf.host_case()
    rep, Ht, Hb = pf.truth(K, n, t, h, A0, bpar, coff, cls, lik, 0, pf.SEED, pf.SWEEP, R0, TAU0)
    assert rep["resamplings"] >= 3 and rep["dead"] == 0
    worst = 0.0
    for i in range(len(K)):
        assert sto.within(rep["H"][i], Ht[i], Hb[i]), (i, rep["H"][i], Ht[i], Hb[i])
        if Hb[i] > 0:
            worst = max(worst, abs(rep["H"][i] - Ht[i]) / Hb[i])
            assert Hb[i] <= 1e-11 * max(1.0, abs(Ht[i]))        # the bar is a few hundred ulps, not a licence
    print("largest H error over its bar", worst)
    assert rep["H"][5] == 0.0 and Ht[5] == 0.0                 # no customers


def test_wrong_replays_are_told_apart():
    K, n, t, h, bpar, coff, cls, lik = pf.host_case()
    R, tau = 8, 0.8
    rep, Ht, Hb = pf.truth(K, n, t, h, A0, bpar, coff, cls, lik, 0, pf.SEED, pf.SWEEP, R, tau)
    assert rep["resamplings"] >= 5
    for mut in ("linear", "u4"):          # by bits: the weights' sums, or the states a resampling hands on
        rm = pf.replay(K, n, t, h, A0, bpar, coff, cls, lik, 0, pf.SEED, pf.SWEEP, R, tau, mut=mut)
        same = (np.array_equal(rm["pn"], rep["pn"]) and np.array_equal(rm["pt"], rep["pt"]) and
                np.array_equal(rm["w"].view(np.uint64), rep["w"].view(np.uint64)) and np.array_equal(rm["E"], rep["E"]) and
                np.array_equal(rm["Zm"].view(np.uint64), rep["Zm"].view(np.uint64)))
        assert not same, mut
    for mut in ("noE", "noS1"):           # by the bar
        rm = pf.replay(K, n, t, h, A0, bpar, coff, cls, lik, 0, pf.SEED, pf.SWEEP, R, tau, mut=mut)
        out = [i for i in range(len(K)) if rep["res"][i] > 0 and not sto.within(rm["H"][i], Ht[i], Hb[i])]
        assert len(out) == int((rep["res"] > 0).sum()) > 0, mut


def test_the_rescaling_is_invisible():
    # 400 customers with p about 1e-2: the product of the p underflows a double (1e-800); H stays finite, within the bar
    rng = np.random.default_rng(5)
    K = np.array([3], dtype=np.int32)
    lik = np.exp(rng.uniform(math.log(0.004), math.log(0.02), (4, 3)))
    h = np.array([0.2, 0.3, 0.5])
    coff = np.array([0, 400], dtype=np.uint64)
    cls = rng.integers(0, 4, 400).astype(np.uint32)
    n, t = np.zeros(3, dtype=np.uint32), np.zeros(3, dtype=np.uint16)
    for tau in (0.0, 0.5):
        rep, Ht, Hb = pf.truth(K, n, t, h, 0.3, [1.5], coff, cls, lik, 0, 9, 0, 4, tau)
        assert math.isfinite(rep["H"][0]) and rep["H"][0] < math.log(5e-324) and rep["dead"] == 0
        assert rep["E"][0] < -1100 and sto.within(rep["H"][0], Ht[0], Hb[0]), (rep["H"][0], Ht[0], Hb[0])
        so = sto.replay(K, n, t, h, 0.3, [1.5], coff, cls, lik, 0, 9, 0, 4)
        assert np.all(np.exp(so["lw"]) == 0.0)     # without step 2 every weight would be 0 in a double


def test_the_budget_is_the_headers():
    assert [pf.budget(K) for K in (0, 1, 64, 80, 81, 130, 1024)] == [64, 64, 64, 64, 62, 39, 5]
