"""The predictive dish proportions' law, and the replay of tests/pr_oracle.py against its own truth and bars -- on the CPU:
what tests/test_gpu_predict.py compares the device with is itself checked here, and shown to fail when it is wrong."""
import itertools
import math

import numpy as np
import pytest

import hp_oracle as hp
import pr_oracle as pro

U = pro.U


# ---- 1. the law: E_{t|n}[theta_k] = p(n + e_k) / p(n), by exact enumeration in mpmath

def stirling(a, nmax):
    """S[n][t] = S^n_{t,a} for n <= nmax by S^{n+1}_t = S^n_{t-1} + (n - t a) S^n_t, S^0_0 = 1"""
    mp = hp._mp()
    S = [[mp.mpf(0)] * (nmax + 2) for _ in range(nmax + 2)]
    S[0][0] = mp.mpf(1)
    for n in range(nmax + 1):
        for t in range(1, n + 2):
            S[n + 1][t] = S[n][t - 1] + (n - t * a) * S[n][t]
    return S


def p_joint(n, t, a, b, h, S):
    """p(n, t) = (b|a)_T / (b)_N prod_k S^{n_k}_{t_k} h_k^{t_k}"""
    mp = hp._mp()
    T, N = sum(t), sum(n)
    v = mp.mpf(1)
    for j in range(T):
        v *= b + j * a
    for j in range(N):
        v /= b + j
    for nk, tk, hk in zip(n, t, h):
        v *= S[nk][tk] * hk ** tk
    return v


def t_states(n):
    return itertools.product(*[range(1, nk + 1) if nk else (0,) for nk in n])


LAW = [((2, 1, 2), 1.5, (0.5, 0.125, 0.25)), ((5,), 0.75, (0.375,)), ((3, 0, 1), 4.0, (0.0625, 0.6875, 0.25))]


@pytest.mark.parametrize("a", [0.0, 0.3, 0.9])
@pytest.mark.parametrize("n, b, h", LAW)
def test_the_law(a, n, b, h):
    mp = hp._mp()
    am, bm, hm = mp.mpf(a), mp.mpf(b), [mp.mpf(x) for x in h]
    S = stirling(am, sum(n) + 1)
    pn = mp.fsum(p_joint(n, t, am, bm, hm, S) for t in t_states(n))
    K = len(n)
    want = []
    for k in range(K):
        n1 = tuple(nk + (j == k) for j, nk in enumerate(n))
        want.append(mp.fsum(p_joint(n1, t, am, bm, hm, S) for t in t_states(n1)) / pn)
    got = [mp.mpf(0)] * K
    for t in t_states(n):
        w = p_joint(n, t, am, bm, hm, S) / pn
        th, _, _ = pro.theta_replay([K], n, t, h, a, [b])
        for k in range(K):
            got[k] += w * mp.mpf(float(th[0, k]))
    for k in range(K):
        err = abs(float(got[k] - want[k]))
        print("a", a, "n", n, "dish", k, "E[theta]", float(got[k]), "p(n+e_k)/p(n)", float(want[k]), "difference", err)
        assert err <= 1e-12
    # the wrong replays miss the law
    for mut in ("t+1", "noTa"):
        bad = [mp.mpf(0)] * K
        for t in t_states(n):
            w = p_joint(n, t, am, bm, hm, S) / pn
            th, _, _ = pro.theta_replay([K], n, t, h, a, [b], mut=mut)
            for k in range(K):
                bad[k] += w * mp.mpf(float(th[0, k]))
        if a > 0:
            assert max(abs(float(bad[k] - want[k])) for k in range(K)) > 1e-6, mut


# ---- 2. sum_k theta = 1 when h sums to 1

@pytest.mark.parametrize("a", pro.RAW_A)
def test_theta_sums_to_one(a):
    K, n, t, _, bpar, *_ = pro.raw_case(a)
    koff = np.concatenate([[0], np.cumsum(K)])
    h = np.zeros(int(K.sum()))
    rng = np.random.default_rng(9)
    for i, k in enumerate(K):   # dyadic weights: the sum is exactly 1
        w = rng.multinomial(1 << 20, np.full(k, 1.0 / k)) + 1.0
        w[0] += (1 << 21) - w.sum()
        h[koff[i]:koff[i + 1]] = w / float(1 << 21)
        assert math.fsum(h[koff[i]:koff[i + 1]]) == 1.0
    tr = pro.truth(K, n, t, h, a, bpar)
    th, _, _ = pro.theta_replay(K, n, t, h, a, bpar)
    for i in range(len(K)):
        assert tr["theta_sum"][i] == 1
        got, bar = math.fsum(th[i]), float(tr["theta_bar"][i].sum())
        print("a", a, "restaurant", i, "K", int(K[i]), "sum theta - 1", got - 1.0, "bar", bar)
        assert abs(got - 1.0) <= bar


# ---- 3. the replay lies within its own bar of the truth on the cases the device is compared on

def worst(got, want, bar):
    """largest |got - want| / bar over the entries (bar 0 asks for equality)"""
    got, want, bar = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (got, want, bar))
    err = np.abs(got - want)
    assert np.all(err[bar == 0.0] == 0.0)
    nz = bar > 0.0
    return float((err[nz] / bar[nz]).max()) if nz.any() else 0.0


@pytest.mark.parametrize("a", pro.RAW_A)
def test_replay_within_bar_raw(a):
    K, n, t, h, bpar, hoff, hcls, lik = pro.raw_case(a)
    rp = pro.replay(K, n, t, h, a, bpar, hoff, hcls, lik, stride=pro.RAW_STRIDE)
    tr = pro.truth(K, n, t, h, a, bpar, hoff, hcls, lik)
    Kmax = int(K.max())
    # (the truth is rounded to a double for the comparison: u |value| more)
    w_th = worst(rp["theta"][:, :Kmax], tr["theta"], tr["theta_bar"] + U * np.abs(tr["theta"]))
    w_p = worst(rp["p"], tr["p"], tr["p_bar"] + U * np.abs(tr["p"]))
    fin = np.isfinite(tr["Hi"])
    assert np.array_equal(np.isfinite(rp["Hi"]), fin)
    w_H = worst(rp["Hi"][fin], tr["Hi"][fin], tr["Hi_bar"][fin])
    print("a", a, "largest error over bar: theta", w_th, "p", w_p, "H_i", w_H, "impossible", rp["impossible"])
    assert w_th <= 1.0 and w_p <= 1.0 and w_H <= 1.0
    assert rp["skipped"] == 0
    assert pro.within(rp["total"], tr["total"], tr["total_bar"])
    assert rp["impossible"] == int((tr["p"] == 0).sum())
    # the restaurant without customers: theta is h, bit for bit
    koff = np.concatenate([[0], np.cumsum(K)])
    e = pro.R_EMPTY
    assert np.array_equal(rp["theta"][e, :K[e]], h[koff[e]:koff[e + 1]])


def test_replay_within_bar_big():
    case = pro.big_case()
    K, n, t, h, bpar, hoff, hcls, lik = case
    rp = pro.replay(K, n, t, h, pro.BIG_A, bpar, hoff, hcls, lik, stride=2)
    tot, bar, mag = pro.big_truth(case)
    print("70 000 restaurants: total", rp["total"], "truth", tot, "difference", rp["total"] - tot, "bar", bar)
    assert rp["impossible"] == 0 and abs(rp["total"] - tot) <= bar


# ---- 4. the replay breaks when it is wrong

def test_wrong_replays_are_told_apart():
    a = 0.5
    K, n, t, h, bpar, hoff, hcls, lik = pro.raw_case(a)
    good = pro.replay(K, n, t, h, a, bpar, hoff, hcls, lik, stride=pro.RAW_STRIDE)
    tr = pro.truth(K, n, t, h, a, bpar, hoff, hcls, lik)
    Kmax = int(K.max())
    for mut in ("t+1", "noTa"):   # outside the bar
        bad = pro.replay(K, n, t, h, a, bpar, hoff, hcls, lik, stride=pro.RAW_STRIDE, mut=mut)
        err = np.abs(bad["theta"][:, :Kmax] - tr["theta"])
        over = err > tr["theta_bar"] + U * np.abs(tr["theta"])
        print(mut, "cells of theta outside the bar", int(over.sum()))
        assert over.any()
        fin = np.isfinite(tr["Hi"]) & (np.diff(hoff.astype(np.int64)) > 0) & (np.arange(len(K)) != pro.R_EMPTY)
        assert (np.abs(bad["Hi"][fin] - tr["Hi"][fin]) > tr["Hi_bar"][fin]).any(), mut
    for mut in ("linear", "reverse"):   # inside the bar, but other bits: what bit-equality is claimed for
        bad = pro.replay(K, n, t, h, a, bpar, hoff, hcls, lik, stride=pro.RAW_STRIDE, mut=mut)
        assert np.array_equal(bad["theta"], good["theta"])
        moved = bad["p"] != good["p"]
        print(mut, "values of p with other bits", int(moved.sum()), "of", moved.size)
        assert moved.any()
        assert np.all(np.abs(bad["p"] - tr["p"]) <= tr["p_bar"] + U * np.abs(tr["p"]))


def test_dd_add_keeps_what_a_plain_sum_loses():
    v = np.array([1.0, 2.0 ** -60, -1.0, 2.0 ** -61])
    assert pro.ordered_dd_sum(v) == 2.0 ** -60 + 2.0 ** -61
    assert pro.tree64(np.arange(64.0)) == 2016.0 and pro.block_tree(np.ones(256)) == 256.0
    x = np.zeros(64)
    x[[0, 1, 32]] = [2.0 ** -53, 2.0 ** -53, 1.0]   # the tree adds lanes 0 and 32 first: each half ulp is lost on its own
    assert pro.tree64(x) == 1.0 and pro.tree64(x, linear=True) == 1.0 + 2.0 ** -52
