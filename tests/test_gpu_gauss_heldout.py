"""Held-out points under Gaussian observations on the device (libstb_amd/csrc/gauss_heldout.hip, predict.hip's k_gh_sum;
include/stb_hip.h "Held-out points under Gaussian observations"): ell, the responsibilities, the accumulator pairs and
the totals against the numpy replay (tests/gh_oracle.py) within the project's standing bar for device libm, the totals
within their derived bars of the 40-digit truth, the counters exactly; the bits across the waves of a workgroup; the object
against the raw composition, its refusals with the state compared; the law of the running estimate on the tiny chain; and
examples/pyp_resample -X 2 -P."""
import hashlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import gh_oracle as gho
import gs_oracle as gso
from libstb_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-10   # the project's standing bar for values that pass through the device's exp and log


def dev(x, dtype):
    import torch

    a = np.ascontiguousarray(x, dtype=dtype)
    if dtype == np.uint32:
        a = a.view(np.int32)
    if dtype == np.uint16:
        a = a.view(np.int16)
    return torch.as_tensor(a, device="cuda")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def close(got, want, rel=REL, floor=1.0):
    """|got - want| <= rel max(floor, |want|) entry by entry, equal infinities agreeing, no NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    inf = np.isinf(want) | np.isinf(got)
    if np.isnan(got).any() or not np.array_equal(got[inf], want[inf]):
        return False
    return bool(np.all(np.abs(got[~inf] - want[~inf]) <= rel * np.maximum(floor, np.abs(want[~inf]))))


def device_theta(c):
    K, I = c["K"], c["I"]
    koff = dev(np.arange(I + 1) * K, np.int64)
    theta, _ = capi.predict_dishes(c["a"], dev(c["bpar"], np.float64), koff, dev(c["n"], np.uint32), dev(c["t"], np.uint16),
                                   h=dev(c["h"], np.float64), tstride=K)
    return theta


def raw(c, rstride=0, acc=None, hoff=None, y=None):
    """the raw composition on a case: (theta, ell, resp) as device tensors"""
    hoff = c["hoff"] if hoff is None else hoff
    y = c["y"] if y is None else y
    theta = device_theta(c)
    ell, resp = capi.gauss_heldout(theta, dev(hoff, np.int64), dev(y, np.float64), dev(c["mu"], np.float64),
                                   dev(c["tau"], np.float64), rstride=rstride, acc=acc)
    return theta, ell, resp


def without_point(c, j):
    """(hoff, y) with flat point j taken out"""
    hoff = np.asarray(c["hoff"]).copy()
    hoff[1:] -= (np.arange(1, hoff.size) > gho.rest_of(c["hoff"])[j]).astype(np.int64)
    return hoff, np.delete(c["y"], j, axis=0)


# ---- 1, 2. the raw calls against the replay and the truth, shape by shape ----

@pytest.mark.parametrize("name", list(gho.SHAPES))
def test_every_output_against_the_replay_and_the_truth(name):
    import torch

    c, tr = gho.make_case(name), gho.case_truth(name)
    K, Ch = c["K"], c["y"].shape[0]
    rstride = K + 3 if len(name) % 2 else K
    theta, ell, resp = raw(c, rstride=rstride)
    tot, Hi, info = capi.gauss_heldout_loglik(dev(c["hoff"], np.int64), ell=ell)
    torch.cuda.synchronize()
    want_theta = gho.theta_of(K, c["n"], c["t"], c["h"], c["a"], c["bpar"])
    assert same_bits(theta.cpu().numpy(), want_theta[:, :K])
    rep = gho.points(want_theta, K, c["hoff"], c["y"], c["mu"], c["tau"], rstride=rstride)
    ell_h, resp_h = ell.cpu().numpy(), resp.cpu().numpy()
    assert close(ell_h, rep["ell"])
    assert resp_h.shape == (Ch, rstride) and close(resp_h, rep["resp"], floor=0.0) and np.all(resp_h[:, K:] == 0.0)
    poss = np.isfinite(rep["ell"])
    assert np.all(resp_h[~poss] == 0.0) and np.all(np.abs(resp_h[poss].sum(axis=1) - 1.0) < 1e-12)
    if K > 1:
        assert resp_h[0, 1] == 0.0 and poss[0]                   # the nearest dish has theta = 0: the point is still scored
    wHi, wtot, nimp = gho.total_of_ell(rep["ell"], c["hoff"])
    assert (info.impossible, info.customers, info.skipped) == (nimp, Ch, 0)
    assert close(Hi.cpu().numpy(), wHi) and close([tot], [wtot])
    # the totals of the possible points within the derived bar of the truth: the same call without the impossible point
    if nimp:
        assert nimp == 1 and not poss[2] and tot == -math.inf
        hoff2, y2 = without_point(c, 2)
        _, ell2, _ = raw(c, hoff=hoff2, y=y2)
        tot, Hi, info = capi.gauss_heldout_loglik(dev(hoff2, np.int64), ell=ell2)
        assert (info.impossible, info.customers) == (0, Ch - 1)
        xs = [v for j, v in enumerate(tr["ell_mp"]) if j != 2]
        want = gho.mp_totals(xs, np.delete(tr["ell_bar"], 2), hoff2)
        assert close(np.delete(ell_h, 2), ell2.cpu().numpy(), rel=0.0, floor=0.0)      # a point's bits do not depend on its neighbours
    else:
        want = tr
    Hi_h = Hi.cpu().numpy()
    hshare = np.abs(Hi_h - want["Hi"]) / np.maximum(want["Hi_bar"], 1e-320)
    tshare = abs(tot - want["total"]) / want["total_bar"]
    eshare = (np.abs(ell_h - tr["ell"])[poss] / tr["ell_bar"][poss]).max(initial=0.0)
    print(name, "largest share of the bar on the device: ell", eshare, "H_i", hshare.max(), "total", tshare)
    assert eshare <= 1.0 and hshare.max() <= 1.0 and tshare <= 1.0


def test_more_points_than_one_grid_step():
    """the grid is capped at 1024 workgroups: at the default four waves a step takes 4096 points, at one wave 1024"""
    import torch

    K, D, I = 2, 1, 3
    Ch = 1024 * 4 + 300
    rng = np.random.default_rng(12)
    c = dict(K=K, D=D, I=I, n=np.array([3, 1, 0, 2, 0, 0], dtype=np.uint32), t=np.array([1, 1, 0, 2, 0, 0], dtype=np.uint16),
             h=np.array([0.4, 0.6, 0.5, 0.5, 0.3, 0.7]), a=0.25, bpar=np.full(I, 0.8),
             hoff=np.array([0, 700, 700 + 3000, Ch], dtype=np.int64), y=rng.normal(0.0, 2.0, size=(Ch, D)),
             mu=np.array([[-1.0], [1.5]]), tau=np.array([[1.0], [2.0]]))
    theta, ell, resp = raw(c, rstride=K)
    M, A = (dev(v, np.float64) for v in gho.acc_empty(Ch))
    raw(c, acc=(M, A))
    tot, Hi, info = capi.gauss_heldout_loglik(dev(c["hoff"], np.int64), ell=ell)
    tot2, Hi2, _ = capi.gauss_heldout_loglik(dev(c["hoff"], np.int64), acc=(M, A), samples=1)
    torch.cuda.synchronize()
    rep = gho.points(gho.theta_of(K, c["n"], c["t"], c["h"], c["a"], c["bpar"]), K, c["hoff"], c["y"], c["mu"], c["tau"])
    ell_h = ell.cpu().numpy()
    assert close(ell_h, rep["ell"]) and close(resp.cpu().numpy(), rep["resp"], floor=0.0)
    assert same_bits(M.cpu().numpy(), ell_h) and np.all(A.cpu().numpy() == 1.0)
    wHi, wtot, _ = gho.total_of_ell(rep["ell"], c["hoff"])
    assert (info.impossible, info.customers) == (0, Ch) and close(Hi.cpu().numpy(), wHi) and close([tot], [wtot])
    # one state: M + log(1 / 1) is ell, and the same sum
    assert tot2 == tot and same_bits(Hi2.cpu().numpy(), Hi.cpu().numpy())
    # and the total within the sum's own part of the bar of the exact sum of the device's ell
    exact = math.fsum(ell_h)
    assert abs(tot - exact) <= gho.U * (6.0 * np.abs(ell_h).sum() + 8.0 * abs(exact) + 3.0 * abs(exact) + 16.0)


# ---- 3. the accumulator over three states ----

@pytest.mark.parametrize("name", ["5x3", "65x16", "1024x2"])
def test_three_accumulating_calls_equal_the_replayed_stream(name):
    import torch

    states = gho.states_of(name, 3)
    base = states[0]
    K = base["K"]
    hoff, y = without_point(base, 2)
    Ch = y.shape[0]
    M, A = (dev(v, np.float64) for v in gho.acc_empty(Ch))
    ells, wM, wA = [], *gho.acc_empty(Ch)
    reps, mps, bars = [], [], []
    for c in states:
        _, ell, _ = raw(c, hoff=hoff, y=y)                     # the state alone ...
        raw(c, acc=(M, A), hoff=hoff, y=y)                     # ... and into the accumulator
        ells.append(ell.cpu().numpy())
        th = gho.theta_of(K, c["n"], c["t"], c["h"], c["a"], c["bpar"])
        rep = gho.points(th, K, hoff, y, c["mu"], c["tau"])
        wM, wA = gho.acc_update(wM, wA, rep["ell"])
        tr = gho.truth(K, c["n"], c["t"], c["h"], c["a"], c["bpar"], hoff, y, c["mu"], c["tau"])
        reps.append(rep)
        mps.append(tr["ell_mp"])
        bars.append(tr["ell_bar"])
    tot, Hi, info = capi.gauss_heldout_loglik(dev(hoff, np.int64), acc=(M, A), samples=3)
    torch.cuda.synchronize()
    M_h, A_h = M.cpu().numpy(), A.cpu().numpy()
    assert same_bits(M_h, np.max(np.stack(ells), axis=0))                   # M is the ell it was taken from
    assert close(M_h, wM) and close(A_h, wA, floor=0.0)
    # the stream replayed on the device's own ell: what the updates alone add
    sM, sA = gho.acc_empty(Ch)
    for e in ells:
        sM, sA = gho.acc_update(sM, sA, e)
    assert same_bits(sM, M_h) and close(A_h, sA, floor=0.0)
    x, ok = gho.acc_x(wM, wA, 3)
    wHi, wtot, nimp = gho.sum_x(x, ok, hoff)
    assert (info.impossible, info.customers) == (nimp, Ch) == (0, Ch)
    assert close(Hi.cpu().numpy(), wHi) and close([tot], [wtot])
    want = gho.acc_truth(mps, bars, hoff)
    tshare = abs(tot - want["total"]) / want["total_bar"]
    hshare = np.abs(Hi.cpu().numpy() - want["Hi"]) / np.maximum(want["Hi_bar"], 1e-320)
    print(name, "largest share of the bar on the device over three states: H_i", hshare.max(), "total", tshare)
    assert tshare <= 1.0 and hshare.max() <= 1.0


def test_what_the_raw_calls_refuse():
    import torch

    C = capi.C
    L = capi.lib()
    f = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device="cuda")   # noqa: E731
    theta, y, mu, tau, ell, resp, M, A = f(2, 3), f(4, 2), f(3, 2), f(3, 2), f(4), f(4, 3), f(4), f(4)
    hoff = dev([0, 2, 4], np.int64)
    p = lambda t: None if t is None else t.data_ptr()                       # noqa: E731

    def call(**kw):
        a = dict(theta=theta, tstride=3, I=2, hoff=hoff, y=y, D=2, mu=mu, tau=tau, K=3, ell=ell, resp=resp, rstride=3, M=M, A=A,
                 flags=capi.GH_ACCUMULATE)
        a.update(kw)
        return L.stb_gauss_heldout(p(a["theta"]), a["tstride"], a["I"], p(a["hoff"]), p(a["y"]), a["D"], p(a["mu"]), p(a["tau"]),
                                   a["K"], p(a["ell"]), p(a["resp"]), a["rstride"], p(a["M"]), p(a["A"]), a["flags"], None)

    for kw, match in (({"theta": None}, "required"), ({"hoff": None}, "required"), ({"y": None}, "required"),
                      ({"mu": None}, "required"), ({"tau": None}, "required"), ({"D": 0}, "D=0"), ({"D": 65}, "D=65"),
                      ({"K": 0}, "K=0"), ({"K": 1025, "tstride": 2000, "rstride": 2000}, "K=1025"), ({"tstride": 2}, "tstride"),
                      ({"rstride": 2}, "rstride"), ({"M": None}, "accumulator"), ({"A": None}, "accumulator"),
                      ({"flags": 2}, "flags"), ({"I": -1}, "I=-1")):
        assert call(**kw) != 0, kw
        assert match in capi.last_error(), (kw, capi.last_error())
    tot = C.c_double(5.0)

    def lcall(**kw):
        a = dict(ell=ell, M=None, A=None, samples=1, hoff=hoff, I=2, tot=C.byref(tot))
        a.update(kw)
        return L.stb_gauss_heldout_loglik(p(a["ell"]), p(a["M"]), p(a["A"]), a["samples"], p(a["hoff"]), a["I"], None, a["tot"],
                                          None, None)

    for kw, match in (({"ell": None}, "required"), ({"M": M}, "pair"), ({"M": M, "A": A, "samples": 0}, "samples=0"),
                      ({"hoff": None}, "required"), ({"tot": None}, "total_host"), ({"I": -1}, "I=-1")):
        assert lcall(**kw) != 0, kw
        assert match in capi.last_error(), (kw, capi.last_error())
    torch.cuda.synchronize()
    for t in (ell, resp, M, A):                                              # nothing was queued
        assert torch.all(t == 7.0)
    assert tot.value == 5.0


# ---- 4. geometry ----

def _digest():
    """every output of the raw layer: the register form, two blocks of dishes, D past 16, sixteen blocks; with and without
    the accumulator"""
    import torch

    h = hashlib.sha256()
    for name in ("5x3", "64x16", "65x16", "64x17", "130x64", "1024x2"):
        states = gho.states_of(name, 2)
        K, Ch = states[0]["K"], states[0]["y"].shape[0]
        M, A = (dev(v, np.float64) for v in gho.acc_empty(Ch))
        hoff = dev(states[0]["hoff"], np.int64)
        for c in states:
            _, ell, resp = raw(c, rstride=K + 1)
            raw(c, acc=(M, A))
            tot, Hi, info = capi.gauss_heldout_loglik(hoff, ell=ell)
            for t in (ell, resp, Hi):
                h.update(t.cpu().numpy().tobytes())
            h.update(np.array([tot], dtype=np.float64).tobytes())
            h.update(np.array([info.impossible, info.customers], dtype=np.uint64).tobytes())
        tot, Hi, info = capi.gauss_heldout_loglik(hoff, acc=(M, A), samples=2)
        torch.cuda.synchronize()
        for t in (M, A, Hi):
            h.update(t.cpu().numpy().tobytes())
        h.update(np.array([tot], dtype=np.float64).tobytes())
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


# ---- 5. the object ----

def obs_object(seed=71, I=6, K=5, D=3):
    import test_gpu_gauss as tgg

    ti, Ks, n, t, h, cust, x = tgg.obs_object(seed=seed, I=I, K=K, D=D)
    rng = np.random.default_rng(seed + 1)
    counts = np.array([3, 0, 70, 1, 2, 5][:I] + [1] * max(0, I - 6))
    hoff = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    y = rng.normal(0.0, 4.0, size=(int(hoff[-1]), D))
    return ti, Ks, x, hoff, y


def raw_of_object(ti, a, bpar, hoff, y, acc=None, rstride=0):
    """the raw composition on the state read back from the object"""
    K, I = ti.maxK, ti.I
    t, _ = ti.get()
    n, _ = ti.get_state()
    mu, tau = ti.get_gauss()
    c = dict(K=K, I=I, n=n, t=t, h=ti.get_h(), a=a, bpar=np.broadcast_to(np.asarray(bpar, dtype=np.float64), (I,)),
             hoff=np.asarray(hoff, dtype=np.int64), y=y, mu=mu, tau=tau)
    theta, ell, resp = raw(c, rstride=rstride, acc=acc)
    return c, ell, resp


def test_the_object_call_is_the_raw_composition_and_writes_nothing():
    import test_gpu_gauss as tgg

    ti, Ks, x, hoff, y = obs_object()
    K = 5
    a, bpar = 0.3, np.full(len(Ks), 1.5)
    pr = tgg.c_prior(tgg.PRIORS["boost"](3))
    try:
        ti.set_obs(x)
        ti.sample_gauss(pr, 71, 2)
        ti.set_heldout_obs(hoff, y)
        before = tgg.obs_state(ti)
        tot, Hi, resp, info = ti.gauss_heldout(a, bpar, want_resp=True)
        tgg.assert_same(tgg.obs_state(ti), before)
        c, ell, rresp = raw_of_object(ti, a, bpar, hoff, y, rstride=K)
        rtot, rHi, rinfo = capi.gauss_heldout_loglik(dev(c["hoff"], np.int64), ell=ell)
        assert tot == rtot and same_bits(Hi, rHi.cpu().numpy()) and same_bits(resp, rresp.cpu().numpy())
        assert (info.impossible, info.customers, info.skipped) == (rinfo.impossible, rinfo.customers, 0) == (0, int(hoff[-1]), 0)
        assert math.isfinite(tot) and Hi[1] == 0.0
        M, A, S = ti.gauss_heldout_get()
        assert S == 0 and np.all(M == -math.inf) and np.all(A == 0.0)            # scoring a state leaves the accumulator alone
        # a short chain with accumulation: the running estimate against the oracle's on the fetched states
        wM, wA = gho.acc_empty(int(hoff[-1]))
        rM, rA = (dev(v, np.float64) for v in gho.acc_empty(int(hoff[-1])))
        for s in range(4):
            ti.sample_gauss(pr, 72, s)
            ti.sweep_dishes(a, bpar, 73, s)
            run, rHi_o, _, info = ti.gauss_heldout(a, bpar, accumulate=True)
            c, _, _ = raw_of_object(ti, a, bpar, hoff, y, acc=(rM, rA))
            rrun, rrHi, _ = capi.gauss_heldout_loglik(dev(c["hoff"], np.int64), acc=(rM, rA), samples=s + 1)
            assert run == rrun and same_bits(rHi_o, rrHi.cpu().numpy())            # the raw composition again, bit for bit
            th = gho.theta_of(K, c["n"], c["t"], c["h"], a, c["bpar"])
            wM, wA = gho.acc_update(wM, wA, gho.points(th, K, c["hoff"], y, c["mu"], c["tau"])["ell"])
            xw, ok = gho.acc_x(wM, wA, s + 1)
            wHi, wtot, _ = gho.sum_x(xw, ok, c["hoff"])
            assert close([run], [wtot]) and close(rHi_o, wHi)
        M, A, S = ti.gauss_heldout_get()
        assert S == 4 and close(M, wM) and close(A, wA, floor=0.0)
        assert same_bits(M, rM.cpu().numpy()) and same_bits(A, rA.cpu().numpy())
        # STB_BPAR_RESIDENT works as for predict
        ti.set_bpar(bpar)
        assert ti.gauss_heldout(a, capi.BPAR_RESIDENT)[0] == ti.gauss_heldout(a, bpar)[0]
        ti.gauss_heldout_reset()
        M, A, S = ti.gauss_heldout_get()
        assert S == 0 and np.all(M == -math.inf) and np.all(A == 0.0)
        # the class held-out set is storage of its own, and its estimator stays refused
        ti.set_heldout(np.arange(len(Ks) + 1, dtype=np.uint64), np.zeros(len(Ks), dtype=np.uint32))
        with pytest.raises(capi.StbError, match="Gaussian observations"):
            ti.heldout(a, bpar)
        assert ti.gauss_heldout(a, bpar)[0] == ti.gauss_heldout(a, bpar)[0]
        # new observations of the same D keep the set; another D drops it; so does leaving the mode
        ti.set_obs(x + 1.0)
        ti.sample_gauss(pr, 74, 0)
        assert math.isfinite(ti.gauss_heldout(a, bpar)[0])
        ti.set_obs(x[:, :2])
        ti.sample_gauss(tgg.c_prior(tgg.PRIORS["plain"](2)), 74, 0)
        with pytest.raises(capi.StbError, match="no held-out points"):
            ti.gauss_heldout(a, bpar)
        ti.set_heldout_obs(hoff, y[:, :2])
        ti.set_obs(None)
        with pytest.raises(capi.StbError, match="no observations"):
            ti.gauss_heldout(a, bpar)
        ti.set_obs(x)
        ti.set_gauss(np.zeros((K, 3)), np.ones((K, 3)))
        with pytest.raises(capi.StbError, match="no held-out points"):
            ti.gauss_heldout(a, bpar)
        for leave in (lambda: ti.set_lik(np.full((2, K), 0.5)), lambda: ti.set_classes(np.zeros(ti.C, dtype=np.uint32), 2)):
            ti.set_obs(x)
            ti.set_heldout_obs(hoff, y)
            leave()
            with pytest.raises(capi.StbError, match="no observations"):
                ti.set_heldout_obs(hoff, y)
    finally:
        ti.free()


def test_what_the_object_refuses_with_state_and_accumulator_as_they_were():
    import test_gpu_gauss as tgg

    ti, Ks, x, hoff, y = obs_object(seed=75, I=2, K=3, D=2)
    hoff, y = hoff[:3], y[:int(hoff[2])]
    a, bpar = 0.3, np.full(len(Ks), 1.5)
    pr = tgg.c_prior(tgg.PRIORS["plain"](2))
    try:
        for call in (lambda: ti.set_heldout_obs(hoff, y), lambda: ti.gauss_heldout(a, bpar), ti.gauss_heldout_reset,
                     ti.gauss_heldout_get):
            with pytest.raises(capi.StbError, match="no observations"):
                call()
        ti.set_obs(x)
        with pytest.raises(capi.StbError, match="no parameters"):
            ti.gauss_heldout(a, bpar)
        ti.sample_gauss(pr, 1, 0)
        for call in (lambda: ti.gauss_heldout(a, bpar), ti.gauss_heldout_reset, ti.gauss_heldout_get):
            with pytest.raises(capi.StbError, match="no held-out points"):
                call()
        ti.set_heldout_obs(hoff, y)
        ti.gauss_heldout(a, bpar, accumulate=True)
        state, acc = tgg.obs_state(ti), ti.gauss_heldout_get()

        def unchanged():
            tgg.assert_same(tgg.obs_state(ti), state)
            got = ti.gauss_heldout_get()
            assert same_bits(got[0], acc[0]) and same_bits(got[1], acc[1]) and got[2] == acc[2] == 1

        bad_y = y.copy()
        bad_y[1, 0] = np.inf
        for call, match in ((lambda: ti.set_heldout_obs(hoff, bad_y), "finite"),
                            (lambda: ti.set_heldout_obs(np.array([1, 2, 3], dtype=np.uint64), y), r"hoff\[0\]"),
                            (lambda: ti.set_heldout_obs(np.array([0, 3, 2], dtype=np.uint64), y[:2]), r"hoff\[2\] < hoff\[1\]"),
                            (lambda: ti.gauss_heldout(1.0, bpar), "discount"),
                            (lambda: ti.gauss_heldout(a, np.full(len(Ks), -0.5)), "bpar"),
                            (lambda: ti.gauss_heldout(a, bpar, flags=2), "flags"),
                            (lambda: ti.gauss_heldout(a, bpar, flags=capi.GH_ACCUMULATE | 4), "flags")):
            with pytest.raises(capi.StbError, match=match):
                call()
            unchanged()
        L = capi.lib()
        assert L.stb_tindic_gauss_heldout(ti.h, a, capi.dp(bpar), 0, None, None, None, None) != 0 and "total" in capi.last_error()
        assert L.stb_tindic_gauss_heldout(ti.h, a, None, 0, capi.C.byref(capi.C.c_double()), None, None, None) != 0
        assert "bpar" in capi.last_error()
        unchanged()
        # h undefined after a failed draw of the base weights
        ti.set_hroot(np.array([0.3, 1e308, 0.3]))
        with pytest.raises(capi.StbError, match="error word 0x"):
            ti.sample_hgroups(1e10, 1.0, 9, 0, flags=capi.HG_KEEP_ROOT)
        with pytest.raises(capi.StbError, match="undefined"):
            ti.gauss_heldout(a, bpar, accumulate=True)
        got = ti.gauss_heldout_get()
        assert same_bits(got[0], acc[0]) and same_bits(got[1], acc[1]) and got[2] == 1
        ti.set_h(np.full(6, 0.5))
        ti.gauss_heldout(a, bpar)
        # parameters undefined after a failed draw of (mu, tau)
        x2 = x.copy()
        x2[0] = 1e200
        ti.set_obs(x2)
        with pytest.raises(capi.StbError, match="precision"):
            ti.sample_gauss(pr, 5, 0)
        with pytest.raises(capi.StbError, match="failed"):
            ti.gauss_heldout(a, bpar, accumulate=True)
        got = ti.gauss_heldout_get()                             # (the same D: the set and its accumulator were kept)
        assert same_bits(got[0], acc[0]) and same_bits(got[1], acc[1]) and got[2] == 1
    finally:
        ti.free()


# ---- 6. the law ----

def test_the_device_chain_scores_the_enumerated_predictive():
    """host test 5's chain through the object: sample_gauss, the dish sweep, and the two held-out points into the
    accumulator after every iteration past the burn-in; the estimate against the exact p(y | x) under the host test's bar
    (a multiple of the batch-means standard error of the oracle's own chain, never the device's)"""
    import td_oracle as tdo
    import test_gpu_gauss as tgg

    I, Nc, K, a, b = (gso.CHAIN[k] for k in ("I", "Nc", "K", "a", "b"))
    pr = gho.law_prior()
    exact = np.array(gho.law_exact())
    _, se = gho.batch_se(gho.law_chain("right"))
    cust = np.array([0, 1, 0, 1, 0, 1], dtype=np.uint32)
    n = np.concatenate([tdo.counts(cust[:Nc], K), tdo.counts(cust[Nc:], K)]).astype(np.uint32)
    ti = capi.TableIndicators(np.full(I, K, dtype=np.int32), n, (n > 0).astype(np.uint16), np.full(I * K, 0.5), cust)
    cp, bpar = tgg.c_prior(pr), np.full(I, b)
    hoff, y = gho.law_points()
    try:
        ti.set_obs(gso.chain_x())
        ti.set_heldout_obs(hoff, y)
        for s in range(gho.LAW_ITER):
            ti.sample_gauss(cp, gso.CHAIN_SEED + 1, s)
            ti.sweep_dishes(a, bpar, gso.CHAIN_SEED, s)
            if s >= gso.CHAIN["burn"]:
                ti.gauss_heldout(a, bpar, accumulate=True, want_Hi=False)
        M, A, S = ti.gauss_heldout_get()
    finally:
        ti.free()
    mean = A * np.exp(M) / S
    z = (mean - exact) / se
    print("exact", exact, "device", mean, "se", se, "z", z)
    assert S == gho.LAW_ITER - gso.CHAIN["burn"] and np.all(np.abs(z) < gho.LAW_Z)


# ---- 7. the example ----

def test_the_example_scores_its_held_out_points():
    exe = os.path.join(ROOT, "examples", "bin", "pyp_resample")
    r = subprocess.run([exe, "-X", "2", "-P", "-J", "4", "-n", "300", "-c", "8"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("iter")]
    held = [float(ln.split("heldout = ")[1].split()[0]) for ln in lines]
    avg = [float(ln.split("avg = ")[1].split()[0]) for ln in lines]
    share = [ln for ln in r.stdout.splitlines() if "held-out points classified" in ln]
    print(held, avg, share)
    assert len(held) == 8 and all(math.isfinite(v) for v in held + avg) and len(share) == 1


if __name__ == "__main__" and sys.argv[1:] == ["--digest"]:
    print(_digest())
