"""What a sampler state predicts (libstb_amd/csrc/predict.hip; include/stb_hip.h "what a state predicts"): the dish
proportions and every held-out probability bit for bit against the numpy replay (tests/pr_oracle.py), the sums within the
oracle's bars of the replay and of the mpmath truth, launch geometries, accumulation over states, impossible and skipped
customers, the object layer end to end, the refusals and examples/pyp_resample -P."""
import math
import os
import re
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import pr_oracle as pro
from libstb_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def dev(x, dtype):
    """a host array on the device; unsigned types travel as the signed type of the same width"""
    import torch

    view = {np.uint64: np.int64, np.uint32: np.int32, np.uint16: np.int16}.get(dtype)
    x = np.array(x, dtype=dtype, order="C")   # (a copy: the cases' arrays are read-only)
    return torch.as_tensor(x.view(view) if view else x, device="cuda")


def run_raw(K, n, t, h, a, bpar, hoff=None, hcls=None, lik=None, tstride=0, rows=None):
    """stb_predict_dishes + stb_heldout_loglik on host arrays: a dict of theta, p, Hi, total, info, skipped (numpy)"""
    import torch

    koff = np.concatenate([[0], np.cumsum(np.asarray(K, dtype=np.int64))])
    d_lik = None if lik is None else dev(lik, np.float64)
    if d_lik is not None and rows is not None:
        d_lik = d_lik[:rows]
    d_hoff = None if hoff is None else dev(hoff, np.uint64)
    skipped = torch.zeros(1, dtype=torch.int64, device="cuda")
    theta, p = capi.predict_dishes(a, dev(bpar, np.float64), dev(koff, np.uint64), dev(n, np.uint32), dev(t, np.uint16),
                                   None if h is None else dev(h, np.float64), tstride, d_hoff,
                                   None if hoff is None else dev(hcls, np.uint32), d_lik, skipped=skipped)
    out = {"theta": None if theta is None else theta.cpu().numpy()}
    if hoff is not None:
        tot, Hi, info = capi.heldout_loglik(p, d_hoff)
        out.update({"p": p.cpu().numpy(), "Hi": Hi.cpu().numpy(), "total": tot, "info": info})
    torch.cuda.synchronize()
    out["skipped"] = int(skipped.item())
    return out


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def over_bar(got, want, bar):
    """largest |got - want| / bar over finite entries; infinities must agree, and a bar of 0 asks for equality"""
    got, want, bar = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (got, want, bar))
    assert not np.isnan(got).any()
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin])
    exact = fin & (bar == 0.0)
    assert np.array_equal(got[exact], want[exact])
    fin &= bar > 0.0
    return float((np.abs(got[fin] - want[fin]) / bar[fin]).max()) if fin.any() else 0.0


# ---- 1. replay, raw layer

@lru_cache(maxsize=None)
def raw_reference(a):
    """(the replay, the truth) of the raw case for discount a, computed once"""
    K, n, t, h, bpar, hoff, hcls, lik = pro.raw_case(a)
    rp = pro.replay(K, n, t, h, a, bpar, hoff, hcls, lik, stride=pro.RAW_STRIDE, tstride=pro.RAW_STRIDE)
    return rp, pro.truth(K, n, t, h, a, bpar, hoff, hcls, lik)


@pytest.mark.parametrize("a", pro.RAW_A)
def test_every_value_equals_the_replay(a):
    K, n, t, h, bpar, hoff, hcls, lik = pro.raw_case(a)
    assert sorted(set(K)) == [1, 2, 63, 64, 65, 128, 130, 1024] and sorted(set(pro.RAW_HC)) == [0, 1, 63, 64, 65, 129, 300]
    assert len(K) == 12 and lik.shape == (5, 1024) and (bpar[pro.R_NEGB] < 0) == (a > 0)
    rp, tr = raw_reference(a)
    got = run_raw(K, n, t, h, a, bpar, hoff, hcls, lik, tstride=pro.RAW_STRIDE)
    assert got["skipped"] == 0 and got["info"].skipped == 0
    assert got["info"].customers == int(hoff[-1]) and got["info"].impossible == rp["impossible"]
    assert same_bits(got["theta"], rp["theta"][:, :pro.RAW_STRIDE]), "theta"
    assert same_bits(got["p"], rp["p"]), "p"
    w_rp = max(over_bar(got["Hi"], rp["Hi"], tr["Hi_bar"]), over_bar(got["total"], rp["total"], tr["total_bar"]))
    w_tr = max(over_bar(got["Hi"], tr["Hi"], tr["Hi_bar"]), over_bar(got["total"], tr["total"], tr["total_bar"]))
    print("a", a, "total", got["total"], "replay", rp["total"], "truth", tr["total"], "bar", tr["total_bar"],
          "largest error over bar: against the replay", w_rp, "against the truth", w_tr)
    assert w_rp <= 1.0 and w_tr <= 1.0
    # without h and without a matrix: h = 1, L = 1
    rp1 = pro.replay(K, n, t, None, a, bpar, hoff, hcls, None, tstride=pro.RAW_STRIDE)
    got1 = run_raw(K, n, t, None, a, bpar, hoff, hcls, None, tstride=pro.RAW_STRIDE)
    assert same_bits(got1["theta"], rp1["theta"][:, :pro.RAW_STRIDE]) and same_bits(got1["p"], rp1["p"])


# ---- 2. register and LDS forms

def test_register_and_lds_forms_agree():
    # The kernel chooses per restaurant (wave-uniformly): K_i <= 64 keeps theta in a register, K_i > 64 in LDS.  So a
    # small restaurant's bits must not depend on who shares the call -- with or without a 65-dish restaurant.
    a = 0.5
    K, n, t, h, bpar, hoff, hcls, lik = pro.raw_case(a)
    full = run_raw(K, n, t, h, a, bpar, hoff, hcls, lik, tstride=64 * 16)
    koff = np.concatenate([[0], np.cumsum(K)])
    ho = hoff.astype(np.int64)
    small = [i for i in range(len(K)) if K[i] <= 64]
    assert len(small) >= 6 and (K > 64).any()
    pick = lambda arr, off: np.concatenate([arr[off[i]:off[i + 1]] for i in small])  # noqa: E731
    hoff_s = np.concatenate([[0], np.cumsum([ho[i + 1] - ho[i] for i in small])]).astype(np.uint64)
    alone = run_raw(K[small], pick(n, koff), pick(t, koff), pick(h, koff), a, bpar[small], hoff_s, pick(hcls, ho), lik, tstride=64)
    assert same_bits(alone["theta"], full["theta"][small][:, :64])
    assert same_bits(alone["p"], pick(full["p"], ho))
    assert same_bits(alone["Hi"], full["Hi"][small])


# ---- 3. geometry

def pr_geom(I, wv=0):
    return capi.reduce_geometry(capi.GEOM_LOGJOINT, I, waves=wv)


def geometry_case(I):
    """big_case(I) and its replay, the restaurants taken 16384 at a time (the replay pads every restaurant to 64 lanes)"""
    case = pro.big_case(I)
    K, n, t, h, bpar, hoff, hcls, lik = case
    thetas, ps = [], []
    for i0 in range(0, I, 16384):
        i1 = min(I, i0 + 16384)
        theta, _, _ = pro.theta_replay(K[i0:i1], n[2 * i0:2 * i1], t[2 * i0:2 * i1], h[2 * i0:2 * i1], pro.BIG_A, bpar[i0:i1])
        p, _ = pro.p_replay(theta, K[i0:i1], np.arange(i1 - i0 + 1), hcls[i0:i1], lik, stride=2)
        thetas.append(theta[:, :2])
        ps.append(p)
    p = np.concatenate(ps)
    Hi, total, nimp = pro.heldout_replay(p, hoff)
    assert nimp == 0
    return case, np.concatenate(thetas), p, Hi, total


def check_big(I, monkeypatch):
    (K, n, t, h, bpar, hoff, hcls, lik), theta, p, Hi, total = geometry_case(I)
    first = None
    for waves in (1, 2, 4, 8):
        monkeypatch.setenv("STB_PREDICT_WAVES", str(waves))  # (read at every call)
        assert pr_geom(I, waves).waves == waves
        got = run_raw(K, n, t, h, pro.BIG_A, bpar, hoff, hcls, lik, tstride=2)
        if first is None:
            first = got
            assert same_bits(got["theta"], theta) and same_bits(got["p"], p)
            assert got["info"].impossible == 0 and got["info"].customers == I
            # every H_i is one logarithm: against numpy's to the last bits of either, the total within the sums' bar
            assert np.all(np.abs(got["Hi"] - Hi) <= 4.0 * U * np.abs(Hi))
            mag = float(np.abs(Hi).sum())
            bar = 4.0 * U * mag + 8.0 * U * mag + U * (2.0 * abs(total) + 16.0)
            print("I", I, "total", got["total"], "replay", total, "difference", got["total"] - total, "bar", bar)
            assert abs(got["total"] - total) <= bar
        else:
            for k in ("theta", "p", "Hi"):
                assert same_bits(got[k], first[k]), (waves, k)
            assert got["total"] == first["total"], waves


def test_the_bits_do_not_depend_on_the_workgroup(monkeypatch):
    a = 0.5
    K, n, t, h, bpar, hoff, hcls, lik = pro.raw_case(a)
    rp, _ = raw_reference(a)
    first = None
    for waves in (1, 2, 4, 8):
        monkeypatch.setenv("STB_PREDICT_WAVES", str(waves))
        got = run_raw(K, n, t, h, a, bpar, hoff, hcls, lik, tstride=pro.RAW_STRIDE)
        assert same_bits(got["theta"], rp["theta"][:, :pro.RAW_STRIDE]) and same_bits(got["p"], rp["p"]), waves
        first = first or got
        assert same_bits(got["Hi"], first["Hi"]) and got["total"] == first["total"], waves


def test_seventy_thousand_restaurants(monkeypatch):
    # 274 blocks of 256 restaurants: many workgroups, the ticket, a last block of 112.  Whether a workgroup takes more
    # than one block here depends on the device's width (the query says); the next test makes sure of it.
    g = pr_geom(pro.BIG_I)
    assert g.blocks == 274 and g.chunks == 1
    print("70 000 restaurants:", g.blocks, "blocks on", g.grid_x, "workgroups,", g.steps, "steps")
    check_big(pro.BIG_I, monkeypatch)


def test_past_one_block_per_workgroup(monkeypatch):
    # the same restaurants, as many as put a second block on a workgroup of the device at hand
    W = pr_geom(1 << 30).grid_x
    I = max(pro.BIG_I, W * 256 + 1)
    g = pr_geom(I)
    assert g.steps > g.grid_x and g.chunks == 1, (g.steps, g.grid_x)
    check_big(I, monkeypatch)


def test_heldout_outgrows_the_block_sums_and_the_calls_after_it():
    """stb_heldout_loglik one block sum past what its first buffer holds, a call of two blocks in the larger buffer, and the
    large call again.  One held-out customer a restaurant, so H_i = log p_i and the kernel's value for a customer depends
    on p_i alone; the p are 257 values tiled, restaurant i of value i mod 257.  The 257 alone are held to the replay as
    check_big holds them (one logarithm: numpy's to the last bits of either), and every H_i of the large call has the
    bits of its customer's value there.  The totals: the replay's block trees and ordered double-double sum of the
    replayed H_i, within check_big's bar."""
    cap0 = int(pr_geom(1).cap0)
    big, small = cap0 * 256 + 1, 257
    gb, gs = pr_geom(big), pr_geom(small)
    assert gb.need == gb.cap0 + 1 and gb.need == gb.blocks and gs.need == 2 <= gs.cap0
    p_types = 0.001 + np.random.default_rng(4300).random(small)

    def case(I):
        """(p and hoff on the device, the replayed H_i, the replayed total, its bar)"""
        Hi_types, _, nimp = pro.heldout_replay(p_types, np.arange(small + 1))
        assert nimp == 0
        Hi = np.resize(Hi_types, I)
        full = np.zeros(-(-I // 256) * 256)
        full[:I] = Hi
        total = float(pro.ordered_dd_sum(pro.block_tree(full.reshape(-1, 256))))
        mag = float(np.abs(Hi).sum())
        bar = 4.0 * U * mag + 8.0 * U * mag + U * (2.0 * abs(total) + 16.0)
        return dev(np.resize(p_types, I), np.float64), dev(np.arange(I + 1), np.uint64), Hi, total, bar

    def run(p, hoff, Hi, total, bar, what):
        import torch

        tot, Hd, info = capi.heldout_loglik(p, hoff)
        torch.cuda.synchronize()
        Hd = Hd.cpu().numpy()
        print(what, "total", tot, "replay", total, "difference", tot - total, "bar", bar)
        assert abs(tot - total) <= bar and np.all(np.abs(Hd - Hi) <= 4.0 * U * np.abs(Hi))
        assert info.impossible == 0 and info.skipped == 0 and info.customers == Hi.shape[0]
        return Hd, (np.float64(tot).tobytes(), Hd.tobytes(), bytes(info))

    cs, cb = case(small), case(big)
    H_types, _ = run(*cs, "the 257 alone")
    capi.lib().stb_sampler_cache_clear()   # (this thread's buffer of block sums: the next call allocates afresh)
    try:
        Hb, ref_b = run(*cb, "regrow")         # more than the first buffer would hold
        assert same_bits(Hb, np.resize(H_types, big)) and Hb[-1] != 0.0
        Hs, ref_s = run(*cs, "after the larger call")   # a smaller call in the larger buffer
        assert same_bits(Hs, H_types)
        Hb2, ref_b2 = run(*cb, "the large call again")
        assert ref_b2 == ref_b
    finally:
        capi.lib().stb_sampler_cache_clear()


# ---- 4. accumulation over states

def small_object(seed=21):
    """6 restaurants of up to 70 dishes, 3 classes, a matrix of 4 rows x 72, and 0 .. 70 held-out customers each"""
    rng = np.random.default_rng(seed)
    K = np.array([70, 9, 64, 1, 65, 30], dtype=np.int32)
    G = int(K.sum())
    n = rng.integers(0, 9, size=G).astype(np.uint32)
    t = np.where(n > 0, 1 + np.floor(rng.random(G) * n), 0).astype(np.uint16)
    h = 0.05 + rng.random(G)
    cust = np.concatenate([rng.permutation(np.repeat(np.arange(k, dtype=np.uint32), n[o:o + k].astype(np.int64)))
                           for k, o in zip(K, np.concatenate([[0], np.cumsum(K)[:-1]]))]).astype(np.uint32)
    cls = rng.integers(0, 3, size=len(cust)).astype(np.uint32)
    hoff = np.concatenate([[0], np.cumsum([70, 0, 5, 64, 65, 1])]).astype(np.uint64)
    hcls = rng.integers(0, 3, size=int(hoff[-1])).astype(np.uint32)
    ti = capi.TableIndicators(K, n, t, h, cust, 0)
    ti.set_classes(cls, 3)
    ti.set_lik(0.1 + rng.random((4, 72)))
    ti.set_heldout(hoff, hcls)
    return ti, K, hoff, hcls


def read_lik(ti):
    L = capi.lib()
    p, rows, stride, q = ti.lik_device()
    out = np.empty((rows, stride), dtype=np.float64)
    capi.check(L.stb_memcpy_d2h(out.ctypes.data, p, out.nbytes, q))
    capi.check(L.stb_stream_sync(q))
    return out


def full_state(ti):
    t, T = ti.get()
    n, cust = ti.get_state()
    return n, t, T, cust, read_lik(ti), ti.get_h()


def assert_same_state(got, want):
    for name, g, w in zip(("n", "t", "T", "cust", "lik", "h"), got, want):
        assert np.array_equal(g, w), name


def state_reference(ti, K, a, bpar, hoff, hcls):
    """(the replay's theta and p, the truth's p_bar) of the object's current state"""
    n, t, _, _, lik, h = full_state(ti)
    theta, _, _ = pro.theta_replay(K, n, t, h, a, bpar)
    p, _ = pro.p_replay(theta, K, hoff, hcls, lik, stride=lik.shape[1])
    return theta, p, pro.truth(K, n, t, h, a, bpar, hoff, hcls, lik)


def test_accumulation_over_states():
    ti, K, hoff, hcls = small_object()
    a, bpar = 0.4, np.array([1.5, 0.7, 3.0, 0.2, 9.0, 1.0])
    try:
        ps, bars, singles = [], [], []
        assert ti.heldout_get()[1] == 0 and not ti.heldout_get()[0].any()
        for s in range(3):
            ti.sweep_dishes(a, bpar, 77, s)
            theta, p, tr = state_reference(ti, K, a, bpar, hoff, hcls)
            assert same_bits(ti.predict(a, bpar, 72), theta[:, :72])
            ps.append(p)
            bars.append(tr["p_bar"])
            tot1, Hi1, info1 = ti.heldout(a, bpar)           # the state alone: the accumulator is left as it is
            assert info1.impossible == 0 and info1.customers == int(hoff[-1]) and info1.skipped == 0
            assert over_bar(Hi1, tr["Hi"], tr["Hi_bar"]) <= 1.0 and pro.within(tot1, tr["total"], tr["total_bar"])
            singles.append(tot1)
            run, Hi, info = ti.heldout(a, bpar, accumulate=True)
            acc, S = ti.heldout_get()
            want = ps[0] if s == 0 else (ps[0] + ps[1] if s == 1 else (ps[0] + ps[1]) + ps[2])
            assert S == s + 1 and same_bits(acc, want), s
            assert ti.heldout(a, bpar)[0] == tot1 and same_bits(ti.heldout_get()[0], want)
            Hi_rp, tot_rp, nimp = pro.heldout_replay(want, hoff, s + 1)
            _, Hb, tb = pro.acc_bars(ps, bars, hoff)
            print("states", s + 1, "running estimate", run, "replay", tot_rp, "difference", run - tot_rp, "bar", tb,
                  "this state alone", tot1)
            assert nimp == 0 and over_bar(Hi, Hi_rp, Hb) <= 1.0 and abs(run - tot_rp) <= tb
        assert not (ps[0] == ps[1]).all() and not (ps[1] == ps[2]).all()   # three states indeed
        ti.heldout_reset()
        acc, S = ti.heldout_get()
        assert S == 0 and acc.shape == (int(hoff[-1]),) and not acc.any()
        run, _, _ = ti.heldout(a, bpar, accumulate=True)    # one state after the reset: the state's own value
        assert run == singles[2] and ti.heldout_get()[1] == 1
    finally:
        ti.free()


# ---- 5. impossible and skipped

def test_impossible_and_skipped():
    import torch

    rng = np.random.default_rng(5)
    K = np.array([3, 70, 5, 3, 4], dtype=np.int32)
    G = int(K.sum())
    n = rng.integers(1, 9, size=G).astype(np.uint32)
    t = (1 + np.floor(rng.random(G) * n)).astype(np.uint16)
    h = 0.05 + rng.random(G)
    a, bpar = 0.5, np.array([1.0, 2.0, 0.5, 3.0, 1.5])
    lik = 0.1 + rng.random((4, 64))          # stride 64 < 70: restaurant 1 is skipped
    lik[2] = 0.0                             # class 2: no dish serves it
    counts = [2, 2, 3, 2, 3]
    hoff = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    hcls = np.array([0, 1, 0, 1, 0, 2, 1, 1, 7, 0, 0, 1], dtype=np.uint32)   # class 7 >= rows
    got = run_raw(K, n, t, h, a, bpar, hoff, hcls, lik, tstride=64)
    assert got["skipped"] == 1 and got["info"].impossible == 4 and got["info"].customers == 12
    assert got["total"] == -math.inf
    assert list(np.isneginf(got["Hi"])) == [False, True, True, True, False]
    for k in ("theta", "p", "Hi"):
        assert not np.isnan(got[k]).any(), k
    assert not got["theta"][1].any() and list(got["p"][[2, 3, 5, 8]]) == [0.0] * 4 and np.all(np.delete(got["p"], [2, 3, 5, 8]) > 0)
    rp = pro.replay(K, n, t, h, a, bpar, hoff, hcls, lik, stride=64, tstride=64)
    assert same_bits(got["theta"], rp["theta"][:, :64]) and same_bits(got["p"], rp["p"])
    assert rp["skipped"] == 1 and rp["impossible"] == 4 and np.array_equal(np.isneginf(rp["Hi"]), np.isneginf(got["Hi"]))
    # every other restaurant's H_i is what it is without them
    koff = np.concatenate([[0], np.cumsum(K)])
    keep = [0, 4]
    pick = lambda arr, off: np.concatenate([arr[off[i]:off[i + 1]] for i in keep])  # noqa: E731
    ho = hoff.astype(np.int64)
    alone = run_raw(K[keep], pick(n, koff), pick(t, koff), pick(h, koff), a, bpar[keep], np.array([0, 2, 5], dtype=np.uint64),
                    pick(hcls, ho), lik, tstride=64)
    assert alone["info"].impossible == 0 and math.isfinite(alone["total"]) and same_bits(alone["Hi"], got["Hi"][keep])
    # accumulating: nothing is added for a skipped restaurant's customers; negative, infinite and NaN p are impossible too
    p = torch.full((12,), 7.0, dtype=torch.float64, device="cuda")
    kd = dev(koff, np.uint64)
    capi.predict_dishes(a, dev(bpar, np.float64), kd, dev(n, np.uint32), dev(t, np.uint16), dev(h, np.float64), 0,
                        dev(hoff, np.uint64), dev(hcls, np.uint32), dev(lik, np.float64), p=p, accumulate=True)
    ph = p.cpu().numpy()
    assert list(ph[[2, 3, 5, 8]]) == [7.0] * 4 and same_bits(ph, 7.0 + rp["p"])
    for bad in (-1.0, math.inf, math.nan, 5e-324):
        p[0] = bad
        tot, Hi, info = capi.heldout_loglik(p, dev(hoff, np.uint64), samples=3)
        Hh = Hi.cpu().numpy()
        assert tot == -math.inf and info.impossible == 1 and Hh[0] == -math.inf and np.isfinite(Hh[1:]).all(), bad
    torch.cuda.synchronize()


# ---- 6. the state is not written

def test_the_state_is_untouched():
    ti, K, hoff, hcls = small_object()
    a, bpar = 0.4, np.full(6, 1.5)
    try:
        ti.sweep_dishes(a, bpar, 3, 0)
        before = full_state(ti)
        theta, p, tr = state_reference(ti, K, a, bpar, hoff, hcls)
        got = ti.predict(a, bpar, 72)
        assert got.shape == (6, 72) and same_bits(got, theta[:, :72]) and not got[1, 9:].any()
        assert over_bar(got[:, :70], tr["theta"], tr["theta_bar"] + U * tr["theta"]) <= 1.0
        ti.heldout(a, bpar)
        ti.heldout(a, bpar, accumulate=True)
        ti.heldout_reset()
        assert_same_state(full_state(ti), before)
    finally:
        ti.free()


# ---- 7. end to end

def planted(I=200, Nc=50, Nh=10, Kd=8, rows=20, seed=81):
    """restaurants that serve three dishes each; dish k's customers come from classes 2k, 2k+1 (0.45 each) and the rest.
    Nc training and Nh held-out customers a restaurant, from the same dishes"""
    rng = np.random.default_rng(seed)
    phi = np.full((rows, Kd), 0.1 / (rows - 2))
    for k in range(Kd):
        phi[2 * k, k] = phi[2 * k + 1, k] = 0.45
    cls, hcls = [], []
    for _ in range(I):
        menu = rng.choice(Kd, size=3, replace=False)
        for out, cnt in ((cls, Nc), (hcls, Nh)):
            out.extend(rng.choice(rows, p=phi[:, k]) for k in rng.choice(menu, size=cnt))
    return np.array(cls, dtype=np.uint32), np.array(hcls, dtype=np.uint32)


def test_the_chain_end_to_end():
    I, Nc, Nh, Kd, rows = 200, 50, 10, 8, 20
    cls, hcls = planted(I, Nc, Nh, Kd, rows)
    a, bpar = 0.3, np.full(I, 2.0)
    start = np.random.default_rng(82).integers(0, Kd, size=I * Nc).astype(np.uint32)
    n = np.stack([np.bincount(start[i * Nc:(i + 1) * Nc].astype(np.int64), minlength=Kd) for i in range(I)]).astype(np.uint32)
    ti = capi.TableIndicators(np.full(I, Kd, dtype=np.int32), n.reshape(-1), (n > 0).astype(np.uint16).reshape(-1), None, start)
    try:
        ti.set_classes(cls, rows)
        ti.set_lik(None, rows, Kd)
        ti.set_heldout(np.arange(I + 1, dtype=np.uint64) * Nh, hcls)
        ti.sample_lik(0.5, 83, 1000)
        ti.sample_h(1.0, 84, 1000)
        first = ti.heldout(a, bpar)[0]
        singles, avg = [], None
        for it in range(30):
            info = ti.sweep_dishes(a, bpar, 85, it)
            ti.sample_lik(0.5, 83, it)
            ti.sample_h(1.0, 84, it)
            ti.sweep(a, bpar, 86, it)
            assert info.stuck + info.skipped == 0
            if it >= 20:
                singles.append(ti.heldout(a, bpar)[0])
                avg, _, pinfo = ti.heldout(a, bpar, accumulate=True)
                assert pinfo.impossible == 0 and pinfo.customers == I * Nh
        assert ti.heldout_get()[1] == 10
        mean = math.fsum(singles) / 10
        # Jensen: log of the mean >= mean of the logs, customer by customer, in exact arithmetic.  In doubles a customer's
        # x = log(p) carries at most u (4 + 1/(1-a) + 8) relative on p (pr_oracle's bars, one block of dishes), 10 u for
        # the accumulation, u for the quotient and 2 u |x| for the log; the sums add 14 u |x| more at most: per side
        # u (40 Hc + 16 sum |x|), and every x < 0 so sum |x| = |total|.
        bar = U * (40.0 * I * Nh + 16.0 * abs(avg)) + U * (40.0 * I * Nh + 16.0 * abs(mean))
        print("held-out log likelihood: start", first, "mean of the last 10 states", mean, "averaged over them", avg,
              "perplexity", math.exp(-avg / (I * Nh)))
        assert math.isfinite(avg) and math.isfinite(first)
        assert avg > first
        assert avg >= mean - bar
    finally:
        ti.free()


# ---- 8. refusals

def test_refusals_leave_the_object():
    import torch

    L = capi.lib()
    ti, K, hoff, hcls = small_object()
    bare = capi.TableIndicators(np.array([2], dtype=np.int32), np.array([3, 1], dtype=np.uint32), np.array([1, 1], dtype=np.uint16))
    a, good = 0.4, np.full(6, 1.5)
    try:
        ti.heldout(a, good, accumulate=True)
        before, acc0 = full_state(ti), ti.heldout_get()
        for call in (lambda b_, a_: ti.heldout(a_, b_), lambda b_, a_: ti.heldout(a_, b_, accumulate=True),
                     lambda b_, a_: ti.predict(a_, b_, 72)):
            for aa, bb, match in ((1.0, good, "discount"), (-0.1, good, "discount"), (math.nan, good, "discount"),
                                  (a, np.full(6, -0.4), "bpar"), (a, np.full(6, math.inf), "bpar")):
                with pytest.raises(capi.StbError, match=match):
                    call(bb, aa)
        with pytest.raises(capi.StbError, match="flags"):
            ti.heldout(a, good, flags=2)
        with pytest.raises(capi.StbError, match="tstride"):
            ti.predict(a, good, 69)
        for call in (lambda: bare.heldout(0.4, [1.0]), bare.heldout_reset, bare.heldout_get):
            with pytest.raises(capi.StbError, match="no held-out customers"):
                call()
        assert bare.predict(0.4, [1.0]).shape == (1, 2)            # (theta needs no held-out set)
        wide = capi.TableIndicators(np.array([1025], dtype=np.int32), np.ones(1025, dtype=np.uint32), np.ones(1025, dtype=np.uint16))
        try:
            wide.set_heldout(np.array([0, 1], dtype=np.uint64), np.zeros(1, dtype=np.uint32))
            for call in (lambda: wide.predict(0.4, [1.0]), lambda: wide.heldout(0.4, [1.0])):
                with pytest.raises(capi.StbError, match="STB_TD_MAXK"):
                    call()
        finally:
            wide.free()
        with pytest.raises(capi.StbError, match="hoff"):
            ti.set_heldout(np.array([0, 3, 2, 2, 2, 2, 2], dtype=np.uint64), np.zeros(2, dtype=np.uint32))
        with pytest.raises(capi.StbError, match="hoff"):
            ti.set_heldout(np.array([1, 1, 1, 1, 1, 1, 1], dtype=np.uint64), np.zeros(1, dtype=np.uint32))
        with pytest.raises(capi.StbError, match="rows"):
            ti.set_heldout(hoff, np.full(int(hoff[-1]), 4, dtype=np.uint32))    # the matrix has 4 rows
        # a matrix with fewer rows set afterwards: found at use
        lik = read_lik(ti)
        ti.set_lik(lik[:2])
        with pytest.raises(capi.StbError, match="rows"):
            ti.heldout(a, good)
        ti.set_lik(lik)
        # null objects and arguments
        tot = capi.C.c_double(0.0)
        assert L.stb_tindic_heldout(None, a, capi.dp(good), 0, capi.C.byref(tot), None, None) != 0 and "null object" in capi.last_error()
        assert L.stb_tindic_heldout(ti.h, a, capi.dp(good), 0, None, None, None) != 0 and "total" in capi.last_error()
        assert L.stb_tindic_heldout(ti.h, a, None, 0, capi.C.byref(tot), None, None) != 0 and "bpar" in capi.last_error()
        assert L.stb_tindic_predict(ti.h, a, capi.dp(good), None, 72) != 0 and "theta_host" in capi.last_error()
        assert L.stb_tindic_predict(None, a, capi.dp(good), None, 72) != 0 and "null object" in capi.last_error()
        assert L.stb_tindic_set_heldout(None, None, None) != 0 and "null object" in capi.last_error()
        assert L.stb_tindic_heldout_reset(None) != 0 and "null object" in capi.last_error()
        # the raw layer
        koff = dev(np.concatenate([[0], np.cumsum(K)]), np.uint64)
        n, t, _, _, _, h = before
        dn, dt, dh, db = dev(n, np.uint32), dev(t, np.uint16), dev(h, np.float64), dev(good, np.float64)
        dho, dhc, dl = dev(hoff, np.uint64), dev(hcls, np.uint32), dev(lik, np.float64)
        p = torch.full((int(hoff[-1]),), 3.0, dtype=torch.float64, device="cuda")
        th = torch.full((6, 72), 3.0, dtype=torch.float64, device="cuda")
        sp, P = capi.stream_ptr(), (lambda x: None if x is None else x.data_ptr())
        ok = dict(a=a, b=db, I=6, koff=koff, n=dn, t=dt, h=dh, th=th, ts=72, ho=dho, hc=dhc, lik=dl, rows=4, stride=72, p=p, fl=0)
        for change, match in ((dict(a=1.0), "discount"), (dict(a=-0.5), "discount"), (dict(koff=None), "required"),
                              (dict(n=None), "required"), (dict(t=None), "required"), (dict(b=None), "bpar"),
                              (dict(p=None), "d_p"), (dict(hc=None), "d_hcls"), (dict(rows=0), "rows=0"),
                              (dict(stride=0), "stride=0"), (dict(ts=0), "tstride=0"), (dict(fl=4), "flags"), (dict(I=-1), "I=-1")):
            c = dict(ok, **change)
            rc = L.stb_predict_dishes(c["a"], P(c["b"]), c["I"], P(c["koff"]), P(c["n"]), P(c["t"]), P(c["h"]), P(c["th"]), c["ts"],
                                      P(c["ho"]), P(c["hc"]), P(c["lik"]), c["rows"], c["stride"], P(c["p"]), c["fl"], None, sp)
            assert rc != 0 and re.search(match, capi.last_error()), (change, capi.last_error())
        for args, match in (((None, P(dho), 6, 1, None, capi.C.byref(tot), None, sp), "required"),
                            ((P(p), None, 6, 1, None, capi.C.byref(tot), None, sp), "required"),
                            ((P(p), P(dho), 6, 0, None, capi.C.byref(tot), None, sp), "samples=0"),
                            ((P(p), P(dho), 6, 1, None, None, None, sp), "total_host"),
                            ((P(p), P(dho), -2, 1, None, capi.C.byref(tot), None, sp), "I=-2")):
            assert L.stb_heldout_loglik(*args) != 0 and re.search(match, capi.last_error()), (match, capi.last_error())
        assert capi.heldout_loglik(p[:0], dho[:1])[0] == 0.0          # I = 0
        torch.cuda.synchronize()
        assert torch.all(p == 3.0) and torch.all(th == 3.0)
        # nothing above changed the object, its accumulator or what the calls do
        assert_same_state(full_state(ti), before)
        acc1 = ti.heldout_get()
        assert acc1[1] == acc0[1] == 1 and same_bits(acc1[0], acc0[0])
        ref, *_ = small_object()
        try:
            ref.heldout(a, good, accumulate=True)
            assert ti.heldout(a, good, accumulate=True)[0] == ref.heldout(a, good, accumulate=True)[0]
            assert same_bits(ti.heldout_get()[0], ref.heldout_get()[0])
        finally:
            ref.free()
        ti.set_heldout(None)
        with pytest.raises(capi.StbError, match="no held-out customers"):
            ti.heldout(a, good)
    finally:
        ti.free()
        bare.free()


# ---- 9. example

EXE = os.path.join(ROOT, "examples", "bin", "pyp_resample")
ARGS = ["-J", "3", "-n", "400", "-c", "9", "-s", "5", "-d", "-z", "-L"]


def test_example_reports_the_held_out_likelihood():
    assert os.path.exists(EXE), "examples/bin/pyp_resample not built (make -C libstb_amd/csrc)"
    for extra in (["-P"], ["-P", "-w"]):
        p = subprocess.run([EXE] + ARGS + extra, capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr[-2000:]
        rows = re.findall(r"^iteration (\d+): log joint .* heldout (\S+) avg (\S+)$", p.stdout, re.M)
        assert [int(r[0]) for r in rows] == list(range(9)), p.stdout
        for _, ho, avg in rows:
            assert math.isfinite(float(ho)) and math.isfinite(float(avg)) and float(ho) < 0.0 and float(avg) < 0.0
        assert rows[0][1] == rows[0][2]          # one state: the estimate is the state's
        m = re.search(r"^held-out: 240 customers, log likelihood (\S+) averaged over 9 states, perplexity (\S+)$", p.stdout, re.M)
        assert m and float(m.group(1)) == float(rows[-1][2])
        assert abs(float(m.group(2)) - math.exp(-float(m.group(1)) / 240)) <= 1e-5 * float(m.group(2))
    # without -L the line is the held-out one alone
    p = subprocess.run([EXE, "-J", "3", "-n", "400", "-c", "4", "-s", "5", "-d", "-z", "-P"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and len(re.findall(r"^iteration \d+: heldout \S+ avg \S+$", p.stdout, re.M)) == 4, p.stdout
    # -P without -d -z is refused
    for args in (["-P"], ["-d", "-P"], ["-z", "-P"]):
        assert subprocess.run([EXE] + args, capture_output=True, text=True, timeout=60).returncode == 2, args


def test_example_without_the_flag_prints_what_it_printed(golden_dir):
    # tests/golden/pyp_resample_dzL.txt is the output of the build before -w and -P existed, for these arguments
    # (tests/test_gpu_tlik.py says how it was recorded)
    assert os.path.exists(EXE), "examples/bin/pyp_resample not built (make -C libstb_amd/csrc)"
    p = subprocess.run([EXE] + ARGS, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "heldout" not in p.stdout and "held-out" not in p.stdout
    assert p.stdout == open(os.path.join(golden_dir, "pyp_resample_dzL.txt")).read()
