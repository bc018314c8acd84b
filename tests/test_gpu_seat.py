"""Customers seated one by one on the device (stb_seat_customers / stb_seat_loglik, stb_tindic_seat / _heldout_seq): the
state, every p_c and the counters bit for bit against the numpy replay (tests/st_oracle.py), the log weights and their
log-mean-exp within the derived bars of the high-precision truth, and the object's calls on the state a seating left.
The law itself is judged on the CPU (tests/test_seat_host.py); the device is held to that replay by bit-equality."""
import hashlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import lj_oracle as lj
import pr_oracle as pro
import st_oracle as sto
import td_oracle as tdo
from libstb_amd import capi
from test_gpu_predict import dev, same_bits
from test_gpu_tdish import assert_state, fetch, grown_vtab, random_lik, random_state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def run_raw(case, a, M=0, particles=1, commit=False, seed=sto.SEED, sweep=sto.RAW_SWEEP, with_info=True):
    """stb_seat_customers on host arrays: a dict of lw (I, particles), the arrays after the call (n, t, and with commit T,
    cust, p), info (skipped, impossible, stuck) and the device lw"""
    import torch

    K, n, t, h, bpar, coff, cls, lik = case
    koff = np.concatenate([[0], np.cumsum(np.asarray(K, dtype=np.int64))])
    d_n, d_t = dev(n, np.uint32), dev(t, np.uint16)
    info = torch.zeros(3, dtype=torch.int64, device="cuda") if with_info else None
    cust0 = np.full(int(coff[-1]), 0xABCD, dtype=np.uint32)
    d_cust = dev(cust0, np.uint32)
    lw, T, cust, p = capi.seat_customers(a, dev(bpar, np.float64), dev(koff, np.uint64), d_n, d_t, dev(coff, np.uint64),
                                         None if h is None else dev(h, np.float64), M, None if cls is None else dev(cls, np.uint32),
                                         None if lik is None else dev(lik, np.float64), particles, commit, seed, sweep,
                                         cust=d_cust, info=info)
    torch.cuda.synchronize()
    out = {"lw": lw.cpu().numpy(), "d_lw": lw, "n": d_n.cpu().numpy().view(np.uint32), "t": d_t.cpu().numpy().view(np.uint16),
           "cust": d_cust.cpu().numpy().view(np.uint32), "cust0": cust0}
    if commit:
        out.update({"T": T.cpu().numpy().view(np.uint32), "p": p.cpu().numpy()})
    if with_info:
        out["info"] = tuple(int(v) for v in info.cpu().numpy())
    return out


def loglik(d_lw):
    tot, Hi, info = capi.seat_loglik(d_lw)
    return tot, Hi.cpu().numpy(), info


# ---- 1. the raw case: bit for bit against the replay, within the bars of the truth

@pytest.mark.parametrize("a,M", sto.RAW_CONFIGS)
def test_the_committed_seating_equals_the_replay(a, M):
    case = sto.raw_case(a)
    K, n, t, h, bpar, coff, cls, lik = case
    assert sorted(set(K)) == [0, 1, 2, 63, 64, 65, 128, 130, 1024] and (bpar[pro.R_NEGB] < 0) == (a > 0)
    rp = sto.raw_replay(a, M, 1, True)
    got = run_raw(case, a, M, 1, commit=True)
    for f in ("n", "t", "T"):
        assert np.array_equal(got[f], rp[f]), f
    skipped_c = slice(int(coff[sto.R_NOK]), int(coff[sto.R_NOK + 1]))
    want_cust = rp["cust"].copy()
    want_cust[skipped_c] = got["cust0"][skipped_c]          # a skipped restaurant is left untouched
    assert np.array_equal(got["cust"], want_cust), "cust"
    assert same_bits(got["p"], rp["p"]), "p"
    assert got["info"] == (rp["skipped"], rp["impossible"], rp["stuck"]) and rp["skipped"] == rp["stuck"] == 1
    assert rp["impossible"] >= 2                              # the stuck visit and the class outside the matrix
    tr = sto.raw_truth(a, M, 1)
    for i in range(len(K)):
        assert sto.within(got["lw"][i, 0], tr["lw"][i, 0], tr["lw_bar"][i, 0]), (i, got["lw"][i, 0], tr["lw"][i, 0])
    # the truncation binds where M = 2 and nowhere else
    grown = rp["t"].astype(np.int64) - t
    assert grown.sum() > 0 and (M != 2 or np.all(grown <= np.maximum(0, 2 - t.astype(np.int64))))


@pytest.mark.parametrize("a,M", sto.RAW_CONFIGS)
def test_log_weights_and_their_mean_lie_within_the_bars(a, M):
    case = sto.raw_case(a)
    K, n, t, h, bpar, coff, cls, lik = case
    import torch

    rp, tr = sto.raw_replay(a, M, 64, True), sto.raw_truth(a, M, 64)
    seated = int(coff[sto.R_NOK])                    # (the customers of the skipped restaurant come last)
    alive = [i for i in range(12) if np.all(np.isfinite(tr["lw"][i]))]
    assert sto.R_STUCK not in alive and sto.R_CLASS not in alive and len(alive) >= 8
    d_alive = torch.as_tensor(alive, device="cuda")
    lw64 = None
    for R in sorted(sto.R_SET, reverse=True):
        got = run_raw(case, a, M, R)
        # nothing but lw is written
        assert np.array_equal(got["n"], n) and np.array_equal(got["t"], t) and np.array_equal(got["cust"], got["cust0"])
        lw = got["lw"]
        assert lw.shape == (13, R) and not np.isnan(lw).any()
        worst = 0.0
        for i in range(13):
            for r in range(R):
                assert sto.within(lw[i, r], tr["lw"][i, r], tr["lw_bar"][i, r]), (R, i, r, lw[i, r], tr["lw"][i, r])
                if tr["lw_bar"][i, r] > 0:
                    worst = max(worst, abs(lw[i, r] - tr["lw"][i, r]) / tr["lw_bar"][i, r])
        # particle r's stream is sweep + r whatever R is
        lw64 = lw if lw64 is None else lw64
        assert same_bits(lw, lw64[:, :R])
        assert got["info"] == (1, int((rp["pall"][:seated, :R] == 0.0).sum()), R)
        # H_i and the total over the restaurants every particle of which lives; then with the dead ones
        tot, Hi, info = loglik(got["d_lw"][d_alive].contiguous())
        tHi, tHb, ttot, ttb = sto.loglik_truth(tr, alive, R)
        assert all(sto.within(Hi[j], tHi[j], tHb[j]) for j in range(len(alive))), (R, Hi, tHi, tHb)
        assert sto.within(tot, ttot, ttb) and info.impossible == 0, (R, tot, ttot, ttb)
        print("a", a, "M", M, "R", R, "total", tot, "truth", ttot, "bar", ttb, "largest lw error over bar", worst)
        tot, Hi, info = loglik(got["d_lw"])
        assert tot == -math.inf and info.impossible == 12 - len(alive) and not np.isnan(Hi).any()
        assert Hi[0] == Hi[1] == -math.inf and Hi[12] == 0.0 and np.all(np.isfinite(Hi[alive]))


def _digest(case, a, M):
    c = run_raw(case, a, M, 1, commit=True)
    f = run_raw(case, a, M, 7)
    tot, Hi, _ = loglik(f["d_lw"][2:12].contiguous())
    hsh = hashlib.sha256()
    for x in (c["n"], c["t"], c["T"], c["cust"], c["p"], c["lw"], f["lw"], Hi, np.float64(tot)):
        hsh.update(np.ascontiguousarray(x).tobytes())
    return hsh.hexdigest()


def test_the_bits_do_not_depend_on_the_waves_of_a_workgroup():
    # a fresh process per setting, the four at once
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    procs = {w: subprocess.Popen([sys.executable, os.path.abspath(__file__), "--digest"], env=dict(env, STB_SEAT_WAVES=str(w)),
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for w in (1, 2, 4, 8)}
    out = {}
    for w, p in procs.items():
        so, se = p.communicate(timeout=120)
        assert p.returncode == 0, (w, se[-2000:])
        out[w] = so.strip().splitlines()[-1]
    assert len(out[4]) == 64 and len(set(out.values())) == 1, out
    assert out[4] == _digest(sto.raw_case(0.5), 0.5, 0)      # and this process, at the default


def test_small_restaurants_do_not_feel_the_large_ones():
    # the same call with every restaurant of more than 64 dishes turned into one without dishes (skipped): the flat
    # customer indices and C stay, so the others' streams do
    a, M = 0.5, 0
    K, n, t, h, bpar, coff, cls, lik = sto.raw_case(a)
    koff = np.concatenate([[0], np.cumsum(K)])
    small = [i for i in range(len(K)) if K[i] <= 64]
    keep = np.concatenate([np.arange(koff[i], koff[i + 1]) for i in small]).astype(np.int64)
    K2 = np.where(K <= 64, K, 0).astype(np.int32)
    case2 = (K2, n[keep], t[keep], h[keep], bpar, coff, cls, lik)
    full, part = run_raw(sto.raw_case(a), a, M, 1, commit=True), run_raw(case2, a, M, 1, commit=True)
    assert part["info"][0] == 1 + sum(1 for i in range(len(K)) if K[i] > 64 and coff[i + 1] > coff[i])
    assert np.array_equal(full["n"][keep], part["n"]) and np.array_equal(full["t"][keep], part["t"])
    for i in small:
        sl = slice(int(coff[i]), int(coff[i + 1]))
        assert np.array_equal(full["cust"][sl], part["cust"][sl]) and same_bits(full["p"][sl], part["p"][sl]), i
        assert same_bits(full["lw"][i], part["lw"][i]) and full["T"][i] == part["T"][i], i
    f7, p7 = run_raw(sto.raw_case(a), a, M, 7), run_raw(case2, a, M, 7)
    assert same_bits(f7["lw"][small], p7["lw"][small])


def test_without_a_matrix_and_without_h():
    a = 0.5
    K, n, t, h, bpar, coff, cls, lik = sto.raw_case(a)
    case = (K, n, t, None, bpar, coff, None, None)
    rp = sto.replay(K, n, t, None, a, bpar, coff, None, None, seed=sto.SEED, sweep=sto.RAW_SWEEP)
    got = run_raw(case, a, 0, 1, commit=True)
    for f in ("n", "t", "T"):
        assert np.array_equal(got[f], rp[f]), f
    assert same_bits(got["p"], rp["p"]) and got["info"] == (1, 0, 0)


def test_refusals_of_the_raw_layer():
    import torch

    case = sto.raw_case(0.5)
    for kw in (dict(a=1.0), dict(a=-0.1), dict(particles=0), dict(particles=4097), dict(particles=2, commit=True), dict(M=65536)):
        args = dict(a=0.5, M=0, particles=1, commit=False)
        args.update(kw)
        with pytest.raises(capi.StbError):
            run_raw(case, args["a"], args["M"], args["particles"], args["commit"])
    K, n, t, h, bpar, coff, cls, lik = case
    koff = dev(np.concatenate([[0], np.cumsum(K)]), np.uint64)
    with pytest.raises(capi.StbError, match="unknown flags"):
        capi.seat_customers(0.5, dev(bpar, np.float64), koff, dev(n, np.uint32), dev(t, np.uint16), dev(coff, np.uint64), flags=2)
    with pytest.raises(capi.StbError, match="d_cls"):
        capi.seat_customers(0.5, dev(bpar, np.float64), koff, dev(n, np.uint32), dev(t, np.uint16), dev(coff, np.uint64),
                            lik=dev(lik, np.float64))
    L = capi.lib()
    assert L.stb_seat_customers(0.5, None, 13, koff.data_ptr(), None, None, None, None, 0, None, None, None, None, 0, 0, 1, 0, 0, 0,
                                None, None, None, None) != 0
    lw = torch.zeros((3, 2), dtype=torch.float64, device="cuda")
    assert L.stb_seat_loglik(lw.data_ptr(), 3, 0, None, None, None, None) != 0
    assert L.stb_seat_loglik(lw.data_ptr(), 3, 2, None, None, None, None) != 0       # total_host is required
    tot, Hi, info = capi.seat_loglik(lw)
    assert tot == 0.0 and np.array_equal(Hi.cpu().numpy(), np.zeros(3)) and info.impossible == 0


# ---- 2. the law case: the replay the host test judged, bit for bit

def test_the_law_case_equals_the_replay_the_host_judged():
    case = sto.law_case()
    rp = sto.law_replay()
    got = run_raw(case, sto.LAW_A, 0, 1, commit=True, seed=sto.LAW_SEED, sweep=sto.LAW_SWEEP)
    for f in ("n", "t", "T", "cust"):
        assert np.array_equal(got[f], rp[f]), f
    assert same_bits(got["p"], rp["p"]) and got["info"] == (0, 0, 0)
    # three customers: the replay's numpy logs and the device's may differ by an ulp each
    assert np.abs(got["lw"][:, 0] - rp["lw"][:, 0]).max() <= 3 * 4.0 * U * np.abs(rp["lw"]).max()
    tot, Hi, info = loglik(got["d_lw"])
    assert same_bits(Hi, got["lw"][:, 0]) and info.impossible == 0          # one particle: H_i = lw_i + log(1)
    assert abs(tot - math.fsum(got["lw"][:, 0])) <= 16.0 * U * abs(tot)


# ---- 3. the object

def object_case(big: bool, M: int = 0, seed: int = 5):
    rng = np.random.default_rng(seed)
    Ks = list(rng.integers(1, 10, size=30)) + ([70, 64, 65] if big else [64, 33])
    K, n, t, h = random_state(rng, Ks, 6)
    if M:
        t = np.minimum(t, M).astype(np.uint16)
    coff = np.concatenate([[0], np.cumsum([x.sum() for x in np.split(n.astype(np.int64), np.cumsum(K)[:-1])])]).astype(np.uint64)
    cls = rng.integers(0, 3, size=int(coff[-1])).astype(np.uint32)
    lik = random_lik(rng, 3, int(K.max()) + 3)
    bpar = 0.3 + 4.0 * rng.random(len(K))
    return K, n, t, h, bpar, coff, cls, lik


def make_object(case, M=0, flags=0, with_lik=True):
    K, n, t, h, bpar, coff, cls, lik = case
    ti = capi.TableIndicators(K, n, t, h, None, M, flags)
    if with_lik:
        ti.set_classes(cls, lik.shape[0])
        ti.set_lik(lik)
    return ti


@pytest.mark.parametrize("big,M", [(False, 0), (True, 0), (True, 2)])
def test_the_object_seats_its_customers_and_goes_on(big, M):
    a = 0.45
    case = object_case(big, M)
    K, n, t, h, bpar, coff, cls, lik = case
    zn, zt = np.zeros_like(n), np.zeros_like(t)
    rp = sto.replay(K, zn, zt, h, a, bpar, coff, cls, lik, M=M, seed=77, sweep=4, bars=True)
    tr = sto.truth(K, zn, zt, h, a, bpar, coff, cls, lik, M, rp)
    maxNi = int(np.diff(coff.astype(np.int64)).max())
    ti = make_object(case, M)
    try:
        total, info = ti.seat(a, bpar, 77, 4)
        assert_state(fetch(ti), (rp["n"], rp["t"], rp["T"], rp["cust"]))
        assert (info.skipped, info.impossible, info.stuck, info.customers) == (0, rp["impossible"], 0, int(coff[-1]))
        if rp["impossible"] == 0:
            want = math.fsum(tr["lw"][:, 0])
            bar = float(tr["lw_bar"].sum()) + 8.0 * U * float(np.abs(tr["lw"]).sum()) + U * (2.0 * abs(want) + 16.0)
            assert abs(total - want) <= bar, (total, want, bar)
        else:
            assert total == -math.inf
        cnt = np.zeros((3, lik.shape[1]), dtype=np.uint32)
        np.add.at(cnt, (cls, rp["cust"]), 1)
        assert np.array_equal(ti.class_counts(), cnt)
        # the log joint of that state, then a dish sweep on it: the bounds are the first dish sweep's
        vt, N, Mt = grown_vtab(a, maxNi, M)
        ltr = lj.truth(K, rp["n"], rp["t"], h, a, bpar, lj.Tables(a, N, Mt), True)
        tot, Li, linfo = ti.logjoint(a, bpar, True)
        assert lj.within(tot, *ltr["total"]) and linfo.outside == 0 and linfo.impossible == 0 and linfo.t_mismatch == 0
        assert all(lj.within(float(Li[i]), float(ltr["Li"][i]), float(ltr["Li_bar"][i])) for i in range(len(K)))
        dinfo = ti.sweep_dishes(a, bpar, 78, 0)
        n2, t2, T2, c2, skipped, stuck = tdo.sweep(K, rp["n"], rp["t"], h, a, bpar, vt, N, Mt, 78, 0, rp["cust"], cls, lik)
        assert_state(fetch(ti), (n2, t2, T2, c2))
        assert (dinfo.skipped, dinfo.stuck) == (skipped, stuck) and not np.array_equal(c2, rp["cust"])
        # seated again from the model: the same stream gives the same seating, another one another
        ti.seat(a, bpar, 77, 4)
        assert_state(fetch(ti), (rp["n"], rp["t"], rp["T"], rp["cust"]))
        ti.seat(a, bpar, 77, 5)
        assert not np.array_equal(ti.get_state()[1], rp["cust"])
    finally:
        ti.free()


def test_the_prior_seating_of_an_object_without_a_matrix():
    a = 0.3
    case = object_case(False)
    K, n, t, h, bpar, coff, cls, lik = case
    rp = sto.replay(K, np.zeros_like(n), np.zeros_like(t), h, a, bpar, coff, None, None, seed=3, sweep=0)
    ti = make_object(case, with_lik=False)
    try:
        total, info = ti.seat(a, bpar, 3, 0)
        assert_state(fetch(ti), (rp["n"], rp["t"], rp["T"], rp["cust"]))
        assert info.impossible == 0 and math.isfinite(total)
    finally:
        ti.free()


def test_one_held_out_customer_is_the_one_step_predictive():
    a = 0.45
    case = object_case(True)
    K, n, t, h, bpar, coff, cls, lik = case
    I = len(K)
    rng = np.random.default_rng(9)
    hoff = np.arange(I + 1, dtype=np.uint64)
    hcls = rng.integers(0, 3, size=I).astype(np.uint32)
    ptr = pro.truth(K, n, t, h, a, bpar, hoff, hcls, lik)
    ti = make_object(case)
    try:
        ti.set_heldout(hoff, hcls)
        ti.heldout(a, bpar, accumulate=True)
        before, acc0, h0 = fetch(ti), ti.heldout_get(), ti.get_h()
        tot_h, Hi_h, _ = ti.heldout(a, bpar)
        tot_s, Hi_s, info = ti.heldout_seq(a, bpar, 1, 21, 0)
        assert info.customers == I and info.skipped == 0 and info.stuck == 0
        for i in range(I):
            assert pro.within(Hi_s[i], ptr["Hi"][i], ptr["Hi_bar"][i]), (i, Hi_s[i], ptr["Hi"][i], ptr["Hi_bar"][i])
            if math.isfinite(ptr["Hi"][i]):                  # both lie within one bar of the truth
                assert abs(Hi_s[i] - Hi_h[i]) <= 2.0 * ptr["Hi_bar"][i], i
        assert pro.within(tot_s, ptr["total"], ptr["total_bar"])
        assert info.impossible == int(np.sum(~np.isfinite(ptr["Hi"])))
        # nothing of the object was written
        assert_state(fetch(ti), before)
        acc1 = ti.heldout_get()
        assert same_bits(acc1[0], acc0[0]) and acc1[1] == acc0[1] and same_bits(ti.get_h(), h0)
    finally:
        ti.free()


def test_an_empty_object_scores_unseen_documents_as_the_raw_call():
    a = 0.45
    K, n, t, h, bpar, coff, cls, lik = object_case(True)
    zn, zt = np.zeros_like(n), np.zeros_like(t)
    R = 7
    raw = run_raw((K, zn, zt, h, bpar, coff, cls, lik), a, 0, R, seed=31, sweep=2)
    tot_r, Hi_r, _ = loglik(raw["d_lw"])
    ti = capi.TableIndicators(K, zn, zt, h)
    try:
        ti.set_lik(lik)
        ti.set_heldout(coff, cls)
        tot, Hi, info = ti.heldout_seq(a, bpar, R, 31, 2)
        assert same_bits(Hi, Hi_r) and same_bits(tot, tot_r)
        assert (info.skipped, info.impossible, info.stuck, info.customers) == (0,) + raw["info"][1:] + (int(coff[-1]),)
        n1, _ = ti.get_state()
        assert not n1.any()
        # more particles: the estimate's spread shrinks, the stream of the first R is the same
        raw64 = run_raw((K, zn, zt, h, bpar, coff, cls, lik), a, 0, 64, seed=31, sweep=2)
        assert same_bits(raw64["lw"][:, :R], raw["lw"])
    finally:
        ti.free()


def test_refusals_leave_the_object_as_it_was():
    a = 0.45
    case = object_case(False)
    K, n, t, h, bpar, coff, cls, lik = case
    I = len(K)
    hoff = np.arange(I + 1, dtype=np.uint64)
    hcls = np.zeros(I, dtype=np.uint32)
    ti = make_object(case)
    ref = make_object(case, flags=capi.TI_REF_ODDS)
    nolik = make_object(case, with_lik=False)
    try:
        ti.set_heldout(hoff, hcls)
        ti.heldout(a, bpar, accumulate=True)
        before, acc0, h0 = fetch(ti), ti.heldout_get(), ti.get_h()
        bad_b = bpar.copy()
        bad_b[3] = -a
        for call in (lambda: ti.seat(1.0, bpar, 1, 0), lambda: ti.seat(-0.5, bpar, 1, 0), lambda: ti.seat(a, bad_b, 1, 0),
                     lambda: ti.heldout_seq(1.0, bpar, 4, 1, 0), lambda: ti.heldout_seq(a, bad_b, 4, 1, 0),
                     lambda: ti.heldout_seq(a, bpar, 0, 1, 0), lambda: ti.heldout_seq(a, bpar, 4097, 1, 0),
                     lambda: nolik.heldout_seq(a, bpar, 1, 1, 0), lambda: ref.seat(a, bpar, 1, 0)):
            with pytest.raises(capi.StbError):
                call()
        L = capi.lib()
        assert L.stb_tindic_seat(None, a, None, 1, 0, None, None) != 0
        assert L.stb_tindic_seat(ti.h, a, None, 1, 0, None, None) != 0
        assert L.stb_tindic_heldout_seq(ti.h, a, capi.dp(bpar), 1, 1, 0, None, None, None) != 0     # total is required
        # a matrix without classes
        nolik.set_lik(lik)
        with pytest.raises(capi.StbError, match="classes"):
            nolik.seat(a, bpar, 1, 0)
        assert_state(fetch(ti), before)
        acc1 = ti.heldout_get()
        assert same_bits(acc1[0], acc0[0]) and acc1[1] == acc0[1] and same_bits(ti.get_h(), h0)
        assert_state(fetch(ref), before)
        assert_state(fetch(nolik), before)
    finally:
        for o in (ti, ref, nolik):
            o.free()


# ---- 4. the example

EXE = os.path.join(ROOT, "examples", "bin", "pyp_resample")


def test_example_starts_from_the_device_and_scores_whole_documents():
    import re

    assert os.path.exists(EXE), "examples/bin/pyp_resample not built (make -C libstb_amd/csrc)"
    base = [EXE, "-J", "3", "-n", "400", "-c", "4", "-s", "5", "-d", "-z", "-P"]
    p = subprocess.run(base + ["-S", "-Q", "8"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    m = re.search(r"^start state seated on the device: 1200 customers, log weight (\S+), 0 impossible visits$", p.stdout, re.M)
    assert m and math.isfinite(float(m.group(1))) and float(m.group(1)) < 0.0, p.stdout
    rows = re.findall(r"^iteration (\d+): heldout (\S+) avg (\S+) seq (\S+)$", p.stdout, re.M)
    assert [int(r[0]) for r in rows] == [0, 1, 2, 3] and all(math.isfinite(float(r[3])) and float(r[3]) < 0.0 for r in rows), p.stdout
    # without the new flags the lines are the old ones; the flags alone are refused
    q = subprocess.run(base, capture_output=True, text=True, timeout=60)
    assert q.returncode == 0 and "seq" not in q.stdout and "seated on the device" not in q.stdout
    assert len(re.findall(r"^iteration \d+: heldout \S+ avg \S+$", q.stdout, re.M)) == 4
    for args in (["-S"], ["-d", "-z", "-Q", "4"], ["-d", "-z", "-P", "-Q", "0"], ["-d", "-z", "-P", "-Q", "5000"]):
        assert subprocess.run([EXE] + args, capture_output=True, text=True, timeout=60).returncode == 2, args


if __name__ == "__main__":
    if sys.argv[1:] == ["--digest"]:
        print(_digest(sto.raw_case(0.5), 0.5, 0))
