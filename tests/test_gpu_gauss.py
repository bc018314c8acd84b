"""Gaussian observations on the device (libstb_amd/csrc/gauss.hip; include/stb_hip.h "Gaussian observations"): the raw
layer -- the statistics bit for bit against the numpy replay (tests/gs_oracle.py), the draw and the matrix cell for cell
within the project's standing bar, the data term and the evidence within their derived bars of the 40-digit truth, the
refusals, the bits across the waves of a workgroup -- and the object in observation mode: its step against the raw
composition, the dish sweep under its matrix, a failed draw, the refusals with the state compared, the law of the tiny
chain, and examples/pyp_resample -X."""
import hashlib
import math
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

import gs_oracle as gso
from libstb_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (C, K, D, offset of x): every C of {0, 1, 255, 256, 257, 513, 5000}, K of {1, 5, 64, 65, 130}, D of {1, 3, 16, 17, 64}
CASES = {
    "0x1x1": (0, 1, 1, 0.0),
    "1x5x3": (1, 5, 3, 0.0),
    "255x64x16": (255, 64, 16, 0.0),
    "256x65x17": (256, 65, 17, 0.0),
    "257x130x64": (257, 130, 64, 0.0),
    "513x5x3_1e8": (513, 5, 3, 1e8),
    "5000x64x16": (5000, 64, 16, 0.0),
    "5000x130x1": (5000, 130, 1, 0.0),
    # the matrix's three forms (gauss.hip, gs_queue_lik): K <= 64 with D = 16 keeps mu and tau in registers at stride <= 64;
    # D = 17 reads the transposed copies, in one block of dishes at K = 64 and K = 40, in several at stride > 64
    "260x64x17": (260, 64, 17, 0.0),
    "300x40x17": (300, 40, 17, 0.0),
    "300x10x32": (300, 10, 32, 0.0),
}
# the strided axes of the grids are capped at 1024 workgroups: the sums take 1024 x 4 waves x 256 customers a step at the
# default four waves, the matrix 4096 rows, the data term's blocks 1024 x 256 at most
PAST_ONE_STEP = 1024 * 4 * 256 + 300


def dev(x, dtype):
    import torch

    a = np.ascontiguousarray(x, dtype=dtype)
    if dtype == np.uint32:
        a = a.view(np.int32)
    return torch.as_tensor(a, device="cuda")


def make_case(C, K, D, offset, seed):
    """x (C, D) around a centre per dish, cust with entries >= K; dish 1 empty and dish 2 of one customer where K allows"""
    rng = np.random.default_rng(seed)
    cust = rng.integers(0, K + 2, size=C).astype(np.uint32)
    if K > 2 and C > 4:
        cust[cust == 1] = 0
        cust[cust == 2] = 3 % K
        cust[C // 2] = 2
        cust[C // 3] = K + 1
    centre = rng.normal(0.0, 3.0, size=(K + 2, D))
    x = offset + centre[cust] + rng.normal(0.0, 1.0, size=(C, D))
    return x, cust


PRIORS = {
    "boost": lambda D: gso.prior(0.7, 0.4, 0.5 + np.arange(D) / 7.0, D, m0=np.linspace(-1.0, 1.0, D)),
    "plain": lambda D: gso.prior(2.0, 2.5, 1.5, D),
}


def c_prior(pr, scalar_beta=False):
    return capi.gauss_prior(pr["kappa0"], pr["alpha0"], float(pr["beta0"][0]) if scalar_beta else pr["beta0"],
                            None if not pr["m0"].any() else pr["m0"])


@lru_cache(maxsize=None)
def stats_of(name):
    """(x, cust, the replay's (n, mean, Q, skipped), the device's) of a case, computed once"""
    import torch

    C, K, D, offset = CASES[name]
    x, cust = make_case(C, K, D, offset, 100 + len(name))
    want = gso.stats(x, cust, K)
    out = (torch.full((K,), -7, dtype=torch.int32, device="cuda"),
           torch.full((K, D), float("nan"), dtype=torch.float64, device="cuda"),
           torch.full((K, D), -1e300, dtype=torch.float64, device="cuda"))       # garbage beforehand
    n, mean, Q, info = capi.gauss_stats(dev(x.reshape(C, D), np.float64), dev(cust, np.uint32), K, out=out)
    torch.cuda.synchronize()
    got = (n.cpu().numpy().view(np.uint32).astype(np.int64), mean.cpu().numpy(), Q.cpu().numpy(), int(info.skipped))
    return x, cust, want, got


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- 1. statistics ----

@pytest.mark.parametrize("name", list(CASES))
def test_statistics_equal_the_replay_bit_for_bit(name):
    x, cust, want, got = stats_of(name)
    C, K, D, _ = CASES[name]
    assert np.array_equal(got[0], want[0]) and got[3] == want[3]
    assert same_bits(got[1], want[1]), "mean"
    assert same_bits(got[2], want[2]), "Q"
    assert int(want[0].sum()) + want[3] == C
    if K > 2 and C > 4:
        assert want[0][1] == 0 and same_bits(got[1][1], np.zeros(D)) and same_bits(got[2][1], np.zeros(D))   # an empty dish: +0.0
        assert want[0][2] == 1 and same_bits(got[2][2], np.zeros(D))                 # one customer: Q = +0.0
        assert want[3] > 0


def test_statistics_past_one_grid_step():
    import torch

    C, K, D = PAST_ONE_STEP, 2, 1
    rng = np.random.default_rng(5)
    cust = rng.integers(0, 3, size=C).astype(np.uint32)
    x = rng.normal(0.0, 1.0, size=(C, D)) + cust[:, None]
    want = gso.stats(x, cust, K)
    d_x, d_cust = dev(x, np.float64), dev(cust, np.uint32)
    n, mean, Q, info = capi.gauss_stats(d_x, d_cust, K)
    torch.cuda.synchronize()
    assert np.array_equal(n.cpu().numpy().view(np.uint32), want[0]) and info.skipped == want[3] > 0
    assert same_bits(mean.cpu().numpy(), want[1]) and same_bits(Q.cpu().numpy(), want[2])
    # the matrix and the data term past their steps too: the last rows against the replay, the total against its own
    pr = PRIORS["plain"](D)
    mu, tau = capi.sample_gauss(n, mean, Q, c_prior(pr), 3, 0)
    lik, linfo = capi.gauss_lik(d_x, mu, tau)
    mu_h, tau_h = mu.cpu().numpy(), tau.cpu().numpy()
    wl, _ = gso.lik(x[C - 600:], mu_h, tau_h)
    from test_gpu_tlik import assert_replayed

    assert_replayed(lik[C - 600:].cpu().numpy(), wl, "the last rows")
    assert linfo.dead == 0
    tot, tinfo = capi.gauss_loglik(d_x, d_cust, mu, tau)
    want_tot, want_skip = gso.loglik(x, cust, mu_h, tau_h)
    # (the device and the replay differ in H's logs alone; each lies within the derived bar of the truth)
    assert tinfo.skipped == want_skip and abs(tot - want_tot) <= 2.0 * gso.loglik_bar(x, cust, mu_h, tau_h)


# ---- 2. the draw ----

@lru_cache(maxsize=None)
def draw_of(name, prior_name):
    """(the prior, the replay's (mu, tau, margin), the device's (mu, tau) as device tensors and on the host)"""
    import torch

    x, cust, want, got = stats_of(name)
    C, K, D, _ = CASES[name]
    pr = PRIORS[prior_name](D)
    seed, sweep = 4000 + len(name), 2
    n, mean, Q = dev(got[0], np.uint32), dev(got[1], np.float64), dev(got[2], np.float64)
    mu, tau = capi.sample_gauss(n, mean, Q, c_prior(pr, scalar_beta=prior_name == "plain"), seed, sweep)
    torch.cuda.synchronize()
    return pr, gso.draw(got[0], got[1], got[2], pr, seed, sweep), (mu, tau), (mu.cpu().numpy(), tau.cpu().numpy())


@pytest.mark.parametrize("prior_name", list(PRIORS))
@pytest.mark.parametrize("name", list(CASES))
def test_every_drawn_cell_equals_the_replay(name, prior_name):
    x, cust, want, got = stats_of(name)
    pr, (wmu, wtau, margin), _, (mu, tau) = draw_of(name, prior_name)
    kn, mn, an, bn = gso.posterior(got[0], got[1], got[2], pr)
    assert np.all(np.isfinite(mu)) and np.all(tau > 0.0) and np.all(np.isfinite(tau))
    rel_tau = float((np.abs(tau - wtau) / wtau).max())
    scale = np.maximum(np.abs(mn), 1.0 / np.sqrt(kn * wtau))
    rel_mu = float((np.abs(mu - wmu) / scale).max())
    print(name, prior_name, "cells", mu.size, "margin", margin, "tau", rel_tau, "mu", rel_mu)
    assert rel_tau <= 1e-10 and rel_mu <= 1e-10
    if prior_name == "boost":
        assert (an < 1.0).any() or not (got[0] == 0).any()     # the boost branch, at the dishes drawn from the prior


def test_a_draw_depends_on_seed_and_sweep_alone():
    x, cust, want, got = stats_of("255x64x16")
    pr = PRIORS["plain"](16)
    n, mean, Q = dev(got[0], np.uint32), dev(got[1], np.float64), dev(got[2], np.float64)
    a = capi.sample_gauss(n, mean, Q, c_prior(pr), 9, 1)
    b = capi.sample_gauss(n, mean, Q, c_prior(pr), 9, 1)
    c = capi.sample_gauss(n, mean, Q, c_prior(pr), 9, 2)
    assert same_bits(a[0].cpu().numpy(), b[0].cpu().numpy()) and same_bits(a[1].cpu().numpy(), b[1].cpu().numpy())
    assert not same_bits(a[1].cpu().numpy(), c[1].cpu().numpy())


# ---- 3. the matrix ----

@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_every_cell_of_the_matrix_equals_the_replay(name, pad):
    """pad = 0: stride = K, the object's own shape -- at K <= 64 one block of dishes, in registers up to D = 16; pad = 3:
    padding columns, and at K = 64 a second block that holds nothing but padding"""
    import torch
    from test_gpu_tlik import assert_replayed

    x, cust, _, _ = stats_of(name)
    C, K, D, _ = CASES[name]
    _, _, (d_mu, d_tau), (mu, tau) = draw_of(name, "plain")
    x = x.copy()
    if C > 10:
        x[7] = 1e200     # every l of this row is -inf: a dead row
    stride = K + pad
    lik, info = capi.gauss_lik(dev(x, np.float64), d_mu, d_tau, stride=stride,
                               out=torch.full((C, stride), float("nan"), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    got = lik.cpu().numpy()
    want, dead = gso.lik(x, mu, tau, stride)
    assert info.dead == dead == (1 if C > 10 else 0)
    if C == 0:
        return
    assert_replayed(got, want, "%s stride %d" % (name, stride))
    assert np.all(got[:, K:] == 0.0)
    live = np.ones(C, dtype=bool)
    if C > 10:
        live[7] = False
        assert np.all(got[7] == 0.0)
    assert np.all(got[live].max(axis=1) == 1.0) and np.all(got >= 0.0)
    assert np.array_equal(got[live, :K].argmax(axis=1), want[live, :K].argmax(axis=1))


# ---- 4. the data term and the evidence ----

@pytest.mark.parametrize("name", ["1x5x3", "255x64x16", "257x130x64", "513x5x3_1e8"])
def test_the_totals_lie_within_their_bars_of_the_truth(name):
    x, cust, _, got = stats_of(name)
    C, K, D, _ = CASES[name]
    pr, _, (d_mu, d_tau), (mu, tau) = draw_of(name, "boost")
    d_x, d_cust = dev(x, np.float64), dev(cust, np.uint32)
    tot, info = capi.gauss_loglik(d_x, d_cust, d_mu, d_tau)
    truth, bar = gso.mp_loglik(x, cust, mu, tau), gso.loglik_bar(x, cust, mu, tau)
    err = abs(float(gso._mp().mpf(tot) - truth))
    print(name, "data term", tot, "error", err, "bar", bar, "share", err / bar)
    assert math.isfinite(tot) and info.skipped == int((cust >= K).sum()) and err <= bar
    n, mean, Q = dev(got[0], np.uint32), dev(got[1], np.float64), dev(got[2], np.float64)
    for pname in PRIORS:
        p = PRIORS[pname](D)
        ml = capi.gauss_logml(n, mean, Q, c_prior(p))
        truth, bar = gso.mp_logml(got[0], got[1], got[2], p), gso.logml_bar(got[0], got[1], got[2], p)
        err = abs(float(gso._mp().mpf(ml) - truth))
        print(name, pname, "evidence", ml, "error", err, "bar", bar, "share", err / bar)
        assert math.isfinite(ml) and err <= bar


def test_the_data_term_is_minus_infinity_or_finite_never_a_nan():
    x, cust, _, _ = stats_of("255x64x16")
    _, _, (d_mu, d_tau), _ = draw_of("255x64x16", "plain")
    x = x.copy()
    inside = np.nonzero(cust < 64)[0]
    x[inside[3]] = 1e200
    tot, _ = capi.gauss_loglik(dev(x, np.float64), dev(cust, np.uint32), d_mu, d_tau)
    assert tot == -math.inf
    # nobody seated: the evidence is exactly 0, the data term the constant's 0
    import torch

    z = torch.zeros((3, 2), dtype=torch.float64, device="cuda")
    assert capi.gauss_logml(dev(np.zeros(3), np.uint32), z, z, c_prior(PRIORS["plain"](2))) == 0.0
    tot, _ = capi.gauss_loglik(torch.zeros((0, 2), dtype=torch.float64, device="cuda"), dev(np.zeros(0), np.uint32), z + 1.0, z + 1.0)
    assert tot == 0.0


# ---- 5. refusals ----

def test_what_the_raw_calls_refuse():
    import torch

    L = capi.lib()
    x, cust = dev(np.zeros((4, 2)), np.float64), dev(np.zeros(4), np.uint32)
    n, m, q = dev(np.zeros(3), np.uint32), dev(np.zeros((3, 2)), np.float64), dev(np.zeros((3, 2)), np.float64)
    mu, tau = dev(np.zeros((3, 2)), np.float64), dev(np.ones((3, 2)), np.float64)
    lik = dev(np.zeros((4, 3)), np.float64)
    P = [p.data_ptr() for p in (x, cust, n, m, q, mu, tau, lik)]
    px, pc, pn, pm, pq, pmu, ptau, plik = P
    import ctypes as C

    for args in ((px, 0, pc, 4, 3, pn, pm, pq, None, None), (px, 65, pc, 4, 3, pn, pm, pq, None, None),
                 (px, 2, pc, 4, 0, pn, pm, pq, None, None), (px, 2, pc, 4, 1025, pn, pm, pq, None, None),
                 (None, 2, pc, 4, 3, pn, pm, pq, None, None), (px, 2, pc, 4, 3, None, pm, pq, None, None)):
        assert L.stb_gauss_stats(*args) != 0 and capi.last_error()
    assert L.stb_gauss_lik(px, 2, 4, pmu, ptau, 3, plik, 2, None, None) != 0 and "stride" in capi.last_error()
    for kw in (dict(kappa0=0.0), dict(alpha0=math.inf), dict(beta0=-1.0), dict(beta0=[1.0, math.nan]), dict(m0=[0.0, math.inf])):
        a = dict(kappa0=1.0, alpha0=1.0, beta0=1.0, m0=None)
        a.update(kw)
        p, keep = capi.gauss_prior(a["kappa0"], a["alpha0"], a["beta0"], a["m0"])
        tot = C.c_double(0.0)
        assert L.stb_sample_gauss(pn, pm, pq, 3, 2, C.byref(p), 1, 0, pmu, ptau, None) != 0 and capi.last_error(), kw
        assert L.stb_gauss_logml(pn, pm, pq, 3, 2, C.byref(p), C.byref(tot), None) != 0, kw
    torch.cuda.synchronize()
    assert np.all(tau.cpu().numpy() == 1.0)


# ---- 6. geometry ----

def _digest():
    """every output of the raw layer on three cases: more than one block of dishes and D past 16; K = 64, D = 16 (the
    matrix at stride = K from registers); one block of dishes at D = 17"""
    import torch

    h = hashlib.sha256()
    for name in ("257x130x64", "5000x64x16", "300x40x17"):
        C, K, D, offset = CASES[name]
        x, cust = make_case(C, K, D, offset, 100 + len(name))
        d_x, d_cust = dev(x, np.float64), dev(cust, np.uint32)
        n, mean, Q, info = capi.gauss_stats(d_x, d_cust, K)
        pr = c_prior(PRIORS["boost"](D))
        mu, tau = capi.sample_gauss(n, mean, Q, pr, 11, 3)
        lik, linfo = capi.gauss_lik(d_x, mu, tau, stride=K + 1)
        lik0, linfo0 = capi.gauss_lik(d_x, mu, tau)          # stride = K: at K = 64, D = 16 the register form
        tot, tinfo = capi.gauss_loglik(d_x, d_cust, mu, tau)
        ml = capi.gauss_logml(n, mean, Q, pr)
        torch.cuda.synchronize()
        for t in (n, mean, Q, mu, tau, lik, lik0):
            h.update(t.cpu().numpy().tobytes())
        h.update(np.array([tot, ml], dtype=np.float64).tobytes())
        h.update(np.array([info.skipped, linfo.dead, linfo0.dead, tinfo.skipped], dtype=np.uint64).tobytes())
    return h.hexdigest()


def test_the_bits_do_not_depend_on_the_waves_of_a_workgroup():
    # a fresh process per setting, the four at once
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    procs = {w: subprocess.Popen([sys.executable, os.path.abspath(__file__), "--digest"], env=dict(env, STB_GAUSS_WAVES=str(w)),
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for w in (1, 2, 4, 8)}
    out = {}
    for w, p in procs.items():
        so, se = p.communicate(timeout=120)
        assert p.returncode == 0, (w, se[-2000:])
        out[w] = so.strip().splitlines()[-1]
    assert len(out[4]) == 64 and len(set(out.values())) == 1, out
    assert out[4] == _digest()                                  # and this process, at the default


# ---- 7. the object in observation mode ----

def obs_object(seed=61, I=6, K=5, D=3, nmax=7):
    import test_gpu_tdish as tdt

    rng = np.random.default_rng(seed)
    Ks, n, t, h = tdt.random_state(rng, [K] * I, nmax)
    cust = tdt.shuffled_order(rng, Ks, n)
    x = rng.normal(0.0, 4.0, size=(K, D))[cust] + rng.normal(0.0, 1.0, size=(len(cust), D))
    return capi.TableIndicators(Ks, n, t, h, cust), Ks, n, t, h, cust, x


def read_lik(ti):
    from test_gpu_tlik import read_lik as rl

    return rl(ti)


def obs_state(ti, params=True):
    t, T = ti.get()
    n, cust = ti.get_state()
    return (n, t, T, cust, ti.get_h(), read_lik(ti), ti.get_classes()[0]) + (ti.get_gauss() if params else ())


def assert_same(got, want):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        if isinstance(g, tuple):
            assert_same(g, w)
        else:
            assert np.array_equal(g, w), j


def test_the_object_step_is_the_raw_composition_and_the_sweep_reads_its_matrix():
    import td_oracle as tdo
    import test_gpu_tdish as tdt

    ti, Ks, n, t, h, cust, x = obs_object()
    C, K, D = len(cust), 5, 3
    pr = c_prior(PRIORS["boost"](D))
    a, bpar = 0.3, np.full(len(Ks), 1.5)
    try:
        ti.set_obs(x)
        cls, rows = ti.get_classes()
        assert rows == C and np.array_equal(cls, np.arange(C)) and np.all(read_lik(ti) == 1.0) and read_lik(ti).shape == (C, K)
        before = obs_state(ti, params=False)
        info = ti.sample_gauss(pr, 71, 2)
        after = obs_state(ti, params=False)
        assert_same(after[:5], before[:5])                    # n, t, T, cust and h are not written
        d_x, d_cust = dev(x, np.float64), dev(before[3], np.uint32)
        rn, rmean, rQ, rinfo = capi.gauss_stats(d_x, d_cust, K)
        rmu, rtau = capi.sample_gauss(rn, rmean, rQ, pr, 71, 2)
        rlik, rl = capi.gauss_lik(d_x, rmu, rtau)
        mu, tau = ti.get_gauss()
        assert same_bits(mu, rmu.cpu().numpy()) and same_bits(tau, rtau.cpu().numpy()) and same_bits(after[5], rlik.cpu().numpy())
        assert (info.skipped, info.dead) == (0, 0) == (rinfo.skipped, rl.dead)
        assert np.all(after[5].max(axis=1) == 1.0)
        # the evidence and the data term are the raw calls' on the object's state
        assert ti.gauss_logml(pr) == capi.gauss_logml(rn, rmean, rQ, pr)
        assert ti.gauss_loglik() == capi.gauss_loglik(d_x, d_cust, rmu, rtau)[0]
        # a dish sweep under the matrix read back from the device
        vt, N, M = tdt.grown_vtab(a, tdt.max_Ni(Ks, n))
        ti.sweep_dishes(a, bpar, 72, 0)
        want = tdo.sweep(Ks, n, t, h, a, bpar, vt, N, M, 72, 0, cust, np.arange(C), after[5])
        tdt.assert_state(tdt.fetch(ti), want[:4])
        assert not np.array_equal(want[3], cust)
        # parameters from the caller: the round trip, and the matrix rewritten
        rng = np.random.default_rng(3)
        mu2, tau2 = rng.normal(0.0, 3.0, size=(K, D)), 0.2 + rng.random((K, D))
        ti.set_gauss(mu2, tau2)
        g = ti.get_gauss()
        assert same_bits(g[0], mu2) and same_bits(g[1], tau2)
        assert same_bits(read_lik(ti), capi.gauss_lik(d_x, dev(mu2, np.float64), dev(tau2, np.float64))[0].cpu().numpy())
    finally:
        ti.free()


def test_the_start_of_observation_mode_past_one_grid_step():
    # k_gs_init's grid is capped at 1024 workgroups of 256 cells: C x K past 262144 takes a second step
    ti, Ks, n, t, h, cust, x = obs_object(seed=64, I=24, K=64, D=1, nmax=6)
    C = len(cust)
    assert C * 64 > 1024 * 256 + 64
    try:
        ti.set_obs(x)
        cls, rows = ti.get_classes()
        lik = read_lik(ti)
        assert rows == C and np.array_equal(cls, np.arange(C)) and lik.shape == (C, 64) and np.all(lik == 1.0)
    finally:
        ti.free()


def test_a_failed_draw_blocks_the_sweeps_until_repaired():
    ti, Ks, n, t, h, cust, x = obs_object(seed=62)
    pr = c_prior(PRIORS["plain"](3))
    a, bpar = 0.3, np.full(len(Ks), 1.5)
    try:
        x = x.copy()
        x[0] = 1e200              # finite, and its dish's Q overflows: beta_n = inf, tau = 0
        ti.set_obs(x)
        with pytest.raises(capi.StbError, match="precision"):
            ti.sample_gauss(pr, 5, 0)
        for call in (lambda: ti.sweep_dishes(a, bpar, 6, 0), ti.get_gauss, ti.gauss_loglik):
            with pytest.raises(capi.StbError, match="failed"):
                call()
        ti.set_gauss(np.zeros((5, 3)), np.ones((5, 3)))
        ti.sweep_dishes(a, bpar, 6, 0)
        assert ti.gauss_loglik() == -math.inf
    finally:
        ti.free()


def test_what_observation_mode_refuses_and_what_leaving_it_restores():
    ti, Ks, n, t, h, cust, x = obs_object(seed=63)
    C = len(cust)
    pr = c_prior(PRIORS["plain"](3))
    a, bpar = 0.3, np.full(len(Ks), 1.5)
    hoff = np.arange(len(Ks) + 1, dtype=np.uint64)
    try:
        with pytest.raises(capi.StbError, match="no observations"):
            ti.sample_gauss(pr, 1, 0)
        with pytest.raises(capi.StbError, match="finite"):
            ti.set_obs(np.where(np.arange(x.size).reshape(x.shape) == 4, np.nan, x))
        ti.set_obs(x)
        ti.sample_gauss(pr, 1, 0)
        ti.set_heldout(hoff, np.zeros(len(Ks), dtype=np.uint32))
        before = obs_state(ti)
        refused = {
            "sample_lik": lambda: ti.sample_lik(0.5, 2, 0),
            "loglik": ti.loglik,
            "class_counts": ti.class_counts,
            "sample_beta": lambda: ti.sample_beta(1.0, 2.0, 1.0, 2, 0),
            "logjoint_collapsed": lambda: ti.logjoint_collapsed(a, bpar, flags=capi.CJ_FLAT | capi.CJ_DATA),
            "sample_classes": lambda: ti.sample_classes(2, 0),
            "generate": lambda: ti.generate(a, bpar, 2, 0),
            "heldout": lambda: ti.heldout(a, bpar),
            "heldout_seq": lambda: ti.heldout_seq(a, bpar, 2, 2, 0),
            "heldout_pf": lambda: ti.heldout_pf(a, bpar, 2, 0.5, 2, 0),
            "heldout_ais": lambda: ti.heldout_ais(a, bpar, 2, 2, 2, 0),
        }
        for name, call in refused.items():
            with pytest.raises(capi.StbError, match="Gaussian observations"):
                call()
            assert_same(obs_state(ti), before)
        # what works as it stands: the log joint, the collapsed one without the data term, the prediction
        ti.logjoint(a, bpar)
        ti.logjoint_collapsed(a, bpar, flags=capi.CJ_FLAT)
        # leaving the mode: neither classes nor a matrix; the categorical calls come back with the caller's own
        ti.set_obs(None)
        assert ti.lik_device()[0] is None
        with pytest.raises(capi.StbError, match="classes"):
            ti.get_classes()
        with pytest.raises(capi.StbError, match="no observations"):
            ti.gauss_logml(pr)
        ti.set_classes(np.arange(C, dtype=np.uint32) % 2, 2)
        ti.set_lik(np.full((2, 5), 0.5))
        assert int(ti.class_counts().sum()) == C and math.isfinite(ti.loglik()[0])
        # the caller's matrix ends the mode too
        ti.set_obs(x)
        ti.set_lik(np.full((2, 5), 0.5))
        with pytest.raises(capi.StbError, match="no observations"):
            ti.sample_gauss(pr, 1, 0)
    finally:
        ti.free()
    # restaurants of differing K_i are refused
    rng = np.random.default_rng(9)
    import test_gpu_tdish as tdt

    Ks, n, t, h = tdt.random_state(rng, [3, 4], 5)
    tj = capi.TableIndicators(Ks, n, t, h)
    try:
        with pytest.raises(capi.StbError, match="every K_i equal"):
            tj.set_obs(np.zeros((int(n.sum()), 2)))
        assert tj.lik_device()[0] is None
    finally:
        tj.free()


def test_the_example_mixture_runs_and_its_evidence_rises():
    exe = os.path.join(ROOT, "examples", "bin", "pyp_resample")
    r = subprocess.run([exe, "-X", "2", "-J", "4", "-n", "300", "-c", "12"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("iter")]
    ev = [float(ln.split("log p(x | z) = ")[1].split()[0]) for ln in lines]
    start = float(r.stdout.split("start: log p(x | z) = ")[1].split()[0])
    print(start, ev)
    assert len(ev) == 12 and all(math.isfinite(v) for v in ev) and ev[-1] > start + 100.0 and "rose" in r.stdout


def test_the_device_chain_has_the_enumerated_law():
    """the host test's tiny chain through the object: sample_gauss and the dish sweep alternated, the partitions of the six
    customers against the exact p(z | x) under the chain test's bar.  2020 iterations: 5050 calls, within the law tests' 6000"""
    import ch_oracle as ch
    import td_oracle as tdo

    (k0, a0, b0), iterations = gso.CHAIN_PRIORS["weak"]
    I, Nc, K, a, b = (gso.CHAIN[k] for k in ("I", "Nc", "K", "a", "b"))
    pr = gso.prior(k0, a0, b0, 1)
    index, probs = ch.merge_cells(gso.chain_exact(pr), (iterations - gso.CHAIN["burn"]) // gso.CHAIN["thin"])
    cust = np.array([0, 1, 0, 1, 0, 1], dtype=np.uint32)
    n = np.concatenate([tdo.counts(cust[:Nc], K), tdo.counts(cust[Nc:], K)]).astype(np.uint32)
    ti = capi.TableIndicators(np.full(I, K, dtype=np.int32), n, (n > 0).astype(np.uint16), np.full(I * K, 0.5), cust)
    cp, bpar, kept = c_prior(pr), np.full(I, b), []
    try:
        ti.set_obs(gso.chain_x())
        for s in range(iterations):
            ti.sample_gauss(cp, gso.CHAIN_SEED + 1, s)
            ti.sweep_dishes(a, bpar, gso.CHAIN_SEED, s)
            if s >= gso.CHAIN["burn"] and s % gso.CHAIN["thin"] == 0:
                kept.append(gso.chain_cell(ti.get_state()[1]))
    finally:
        ti.free()
    p = ch.chi2_pvalue(ch.cell_counts(kept, index, len(probs)), probs)
    print("bins", len(probs), "kept", len(kept), "p", p)
    assert p > 1e-3


if __name__ == "__main__" and sys.argv[1:] == ["--digest"]:
    print(_digest())
