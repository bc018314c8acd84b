"""The windowed table-count sweep on the device (stb_tcounts_sweep_window / stb_sample_tcounts_window): draw for draw
against the numpy oracle (tests/tcw_oracle.py) in both modes, in distribution against the exact joint (and the reference
chain's own law), interleaved with full sweeps, handed to a group set, and with rejected inputs."""
import math
import os

import numpy as np
import pytest

import orc
import tc_oracle as tco
import tcw_oracle as tcw
from libstb_amd import capi, synth

pytestmark = pytest.mark.gpu


def device_table(a, N, M):
    """the slab stb_tcounts fills for (a, N, M), in the oracle's packed layout: the draws see the same cells"""
    tabs = capi.DeviceTables(N, M)
    tabs.fill(a)
    tabs.status()
    return tabs.S1[0].cpu().numpy(), tabs.packed_host(0)


def random_state(rng, I, K, nmax):
    n = rng.integers(0, nmax + 1, size=I * K).astype(np.uint32)
    t = np.where(n > 0, 1 + np.floor(rng.random(I * K) * n), 0).astype(np.uint16)
    h = 0.05 + 0.95 * rng.random(I * K)
    return np.full(I, K, dtype=np.int32), n, t, h


def chi2_sf(x, k):
    try:
        from scipy.stats import chi2

        return float(chi2.sf(x, k))
    except ImportError:  # Wilson-Hilferty
        z = ((x / k) ** (1.0 / 3.0) - (1.0 - 2.0 / (9.0 * k))) / math.sqrt(2.0 / (9.0 * k))
        return 0.5 * math.erfc(z / math.sqrt(2.0))


def chi2_p(counts, p):
    exp = p * counts.sum()
    keep = exp >= 5
    obs = np.append(counts[keep], counts[~keep].sum())
    ex = np.append(exp[keep], exp[~keep].sum())
    if ex[-1] < 5:  # fold the tail bin into the last kept one
        obs, ex = np.append(obs[:-2], obs[-2:].sum()), np.append(ex[:-2], ex[-2:].sum())
    return chi2_sf(float(np.sum((obs - ex) ** 2 / ex)), len(obs) - 1)


def check_sweeps(tc, K, n, t, h, a, bpar, M, S1, tab, W, seed, sweeps, ref=False):
    for s in sweeps:
        tc.sweep_window(a, bpar, W, seed, s, ref=ref)
        got_t, got_T = tc.get()
        t, T, ties = tcw.sweep(K, n, t, h, a, bpar, M, S1, tab, M, W, seed, s, ref=ref)
        assert ties == 0, "pick a seed without near-ties"
        assert np.array_equal(got_t, t), np.flatnonzero(got_t != t)[:10]
        assert np.array_equal(got_T, T)
    return t


@pytest.mark.parametrize("W", [1, 10, 30, 300, 65535])
@pytest.mark.parametrize("ref", [False, True])
@pytest.mark.parametrize("a,b,seed", [(0.0, 2.0, 11), (0.5, 0.5, 12), (0.75, 20.0, 13)])
def test_exact_agreement_with_the_oracle(a, b, seed, ref, W):
    rng = np.random.default_rng(seed)
    K, n, t, h = random_state(rng, 48, 40, 300)
    bpar = np.full(48, b)
    N = M = int(n.max())
    S1, tab = device_table(a, N, M)
    tc = capi.TableCounts(K, n, t, h)
    try:
        check_sweeps(tc, K, n, t, h, a, bpar, M, S1, tab, W, seed, range(3), ref)
    finally:
        tc.free()


@pytest.mark.parametrize("W", [16, 40, 200, 65535])
def test_long_spans(W):
    # spans above 64 tau values: the chunked path (4W+1 > 64), rows up to 5000
    a, b, seed = 0.5, 3.0, 21
    K = np.array([3, 2, 1, 4], dtype=np.int32)
    n = np.array([5000, 4000, 3777, 5000, 65, 4999, 1, 0, 2500, 5000], dtype=np.uint32)
    t = np.array([1, 300, 3777, 50, 60, 2000, 1, 0, 2, 100], dtype=np.uint16)
    h = np.array([1.0, 0.5, 0.9, 0.2, 1.0, 0.7, 1.0, 1.0, 0.3, 0.8])
    bpar = np.array([b, 0.1, 40.0, b])
    N = M = 5000
    S1, tab = device_table(a, N, M)
    tc = capi.TableCounts(K, n, t, h, M)
    try:
        for ref in (False, True):
            t = check_sweeps(tc, K, n, t, h, a, bpar, M, S1, tab, W, seed, range(2 * ref, 2 * ref + 2), ref)
    finally:
        tc.free()


@pytest.mark.parametrize("W", [1, 2, 5])
def test_edge_pairs_against_the_oracle(W):
    # n = 0, n = 1, M < n (truncated at M = 25), t at 1 and at min(n, M), a pair with n = 2
    a, M = 0.3, 25
    K = np.array([5, 3, 2], dtype=np.int32)
    n = np.array([0, 1, 40, 12, 12, 30, 2, 1, 25, 25], dtype=np.uint32)
    t = np.array([0, 1, 1, 12, 5, 25, 2, 1, 25, 1], dtype=np.uint16)
    bpar = np.array([1.0, 2.0, 0.2])
    S1, tab = device_table(a, 40, M)
    tc = capi.TableCounts(K, n, t, None, M)
    try:
        t = check_sweeps(tc, K, n, t, None, a, bpar, M, S1, tab, W, 5, range(8))
        assert t[0] == 0 and t[1] == 1 and t[7] == 1 and t.max() <= M
    finally:
        tc.free()


def test_raw_pairs_outside_the_table_keep_t():
    import torch

    a, N, M, W = 0.5, 40, 100, 3
    tabs = capi.DeviceTables(N, M)
    tabs.fill(a)
    tabs.status()
    S1, tab = tabs.S1[0].cpu().numpy(), tabs.packed_host(0)
    K = np.array([4, 1], dtype=np.int32)
    n = np.array([60, 30, 41, 40, 200], dtype=np.uint32)    # n > N, with M >= n (60, 41) and M < n (200)
    t = np.array([7, 4, 41, 40, 9], dtype=np.uint16)
    dev = "cuda"
    koff = torch.as_tensor(np.array([0, 4, 5], dtype=np.int64), device=dev)
    d_n = torch.as_tensor(n.view(np.int32), device=dev)
    d_t = torch.as_tensor(t.view(np.int16), device=dev).clone()
    d_T = torch.as_tensor(np.array([92, 9], dtype=np.int32), device=dev)
    d_b = torch.as_tensor(np.array([1.0, 1.0]), device=dev)
    want = t.copy()
    for s in range(4):
        capi.sample_tcounts_window(tabs, a, d_b, koff, d_n, d_t, d_T, None, W, 8, s)
        want, T, ties = tcw.sweep(K, n, want, None, a, [1.0, 1.0], M, S1, tab, M, W, 8, s, N=N)
        assert ties == 0
    torch.cuda.synchronize()
    got = d_t.cpu().numpy().view(np.uint16)
    assert np.array_equal(got, want) and got[0] == 7 and got[2] == 41 and got[4] == 9
    assert np.array_equal(d_T.cpu().numpy().view(np.uint32), T)


def sample_states(rng, p, states, I):
    idx = rng.choice(len(states), size=I, p=p)
    return np.array(states, dtype=np.uint16)[idx].reshape(-1)


@pytest.mark.parametrize("ref", [False, True])
def test_distribution_one_dish(ref):
    # started from the chain's own stationary law, three sweeps keep it: the exact joint (exact mode), the reference
    # chain's stationary law, 0.054 away from it (reference mode)
    n, a, b, h, W, I = 10, 0.5, 1.0, 1.0, 1, 200000
    S1, tab = orc.fill_S(a, n, n)
    pi = tcw.joint((n,), (h,), a, b, S1, tab, n)
    law = tcw.stationary(tcw.sweep_matrix((n,), (h,), a, b, W, S1, tab, n, ref=True)) if ref else pi
    law = np.clip(law, 0.0, None) / np.clip(law, 0.0, None).sum()
    rng = np.random.default_rng(4 + ref)
    t0 = sample_states(rng, law, tcw.states((n,)), I)
    tc = capi.TableCounts(np.ones(I, dtype=np.int32), np.full(I, n, dtype=np.uint32), t0)
    try:
        tc.sweep_window(a, np.full(I, b), W, 99, 0, 3, ref=ref)
        got, T = tc.get()
    finally:
        tc.free()
    assert np.array_equal(T, got.astype(np.uint32))
    counts = np.bincount(got.astype(np.int64) - 1, minlength=n).astype(np.float64)
    assert chi2_p(counts, law) > 1e-6
    if ref:
        assert chi2_p(counts, pi) < 1e-12  # the reference's chain is not the joint's


@pytest.mark.parametrize("W", [1, 2])
def test_distribution_coupled(W):
    a, b = 0.4, 1.5
    ns, hs = (6, 4), (1.0, 0.5)
    I = 100000
    S1, tab = orc.fill_S(a, 6, 6)
    pi = tcw.joint(ns, hs, a, b, S1, tab, 6)
    st = tcw.states(ns)
    rng = np.random.default_rng(W)
    t0 = sample_states(rng, pi, st, I)
    K = np.full(I, 2, dtype=np.int32)
    n = np.tile(np.array(ns, dtype=np.uint32), I)
    tc = capi.TableCounts(K, n, t0, np.tile(np.array(hs), I))
    try:
        tc.sweep_window(a, np.full(I, b), W, 4242, 0, 5)
        got, T = tc.get()
    finally:
        tc.free()
    g = got.reshape(I, 2).astype(np.int64)
    assert np.array_equal(T, g.sum(axis=1).astype(np.uint32))
    counts = np.bincount((g[:, 0] - 1) * 4 + (g[:, 1] - 1), minlength=len(st)).astype(np.float64)
    assert chi2_p(counts, pi) > 1e-6


def test_long_chain_reaches_the_joint():
    # from t = 1 everywhere, W = 1 chains reach the joint: the acceptance test is what makes that law the target
    n, a, b, h, W, I = 12, 0.0, 1.0, 1.0, 2, 100000
    S1, tab = orc.fill_S(a, n, n)
    pi = tcw.joint((n,), (h,), a, b, S1, tab, n)
    tc = capi.TableCounts(np.ones(I, dtype=np.int32), np.full(I, n, dtype=np.uint32), np.ones(I, dtype=np.uint16))
    try:
        tc.sweep_window(a, np.full(I, b), W, 7, 0, 200)
        got, _ = tc.get()
    finally:
        tc.free()
    counts = np.bincount(got.astype(np.int64) - 1, minlength=n).astype(np.float64)
    assert chi2_p(counts, pi) > 1e-6


def test_queued_sweeps_equal_single_calls():
    g = synth.groups(30, 20, 400, "realistic", seed=3)
    q = capi.TableCounts(g.K, g.n, g.t)
    r = capi.TableCounts(g.K, g.n, g.t)
    try:
        q.sweep_window(0.4, g.bpar, 10, 17, 2, 5)
        for s in range(2, 7):
            r.sweep_window(0.4, g.bpar, 10, 17, s)
        assert all(np.array_equal(x, y) for x, y in zip(q.get(), r.get()))
    finally:
        q.free()
        r.free()


def test_interleaved_with_full_sweeps():
    a, seed = 0.6, 31
    rng = np.random.default_rng(seed)
    K, n, t, h = random_state(rng, 20, 30, 200)
    bpar = 0.5 + rng.random(20)
    N = M = int(n.max())
    S1, tab = device_table(a, N, M)
    tc = capi.TableCounts(K, n, t, h)
    try:
        for s, kind in enumerate(("full", "win", "win", "full", "ref", "win")):
            if kind == "full":
                tc.sweep(a, bpar, seed, s)
                t, T, ties = tco.sweep(K, n, t, h, a, bpar, M, S1, tab, M, seed, s)
            else:
                tc.sweep_window(a, bpar, 4, seed, s, ref=kind == "ref")
                t, T, ties = tcw.sweep(K, n, t, h, a, bpar, M, S1, tab, M, 4, seed, s, ref=kind == "ref")
            assert ties == 0
            got_t, got_T = tc.get()
            assert np.array_equal(got_t, t) and np.array_equal(got_T, T), (s, kind)
    finally:
        tc.free()


def test_launch_geometry_does_not_change_the_bits():
    g = synth.groups(301, 25, 3000, "realistic", seed=12)
    outs = []
    old = os.environ.get("STB_TCWIN_WAVES")
    try:
        for wv in ("1", "2", "4", "8"):
            os.environ["STB_TCWIN_WAVES"] = wv
            tc = capi.TableCounts(g.K, g.n, g.t)
            tc.sweep_window(0.45, g.bpar, 10, 5, 0, 2)
            tc.sweep_window(0.45, g.bpar, 40, 5, 2, 1)
            tc.sweep_window(0.45, g.bpar, 3, 5, 3, 1, ref=True)
            outs.append(tc.get())
            tc.free()
    finally:
        if old is None:
            os.environ.pop("STB_TCWIN_WAVES", None)
        else:
            os.environ["STB_TCWIN_WAVES"] = old
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1])
    assert not np.array_equal(outs[0][0], g.t)


def test_hand_over_to_a_group_set():
    L = capi.lib()
    g = synth.groups(100, 20, 300, "realistic", seed=77)
    N = M = int(g.n.max())
    x = synth.discount_grid(8)
    tc = capi.TableCounts(g.K, g.n, g.t)
    A = L.stb_groups_create(g.I, orc.i32p(g.K), orc.u32p(g.T), orc.u32p(g.n), orc.u16p(g.t), orc.dp(g.bpar), N, M, 8)
    B = L.stb_groups_create(g.I, orc.i32p(g.K), orc.u32p(g.T), orc.u32p(g.n), orc.u16p(g.t), orc.dp(g.bpar), N, M, 8)
    assert A and B, capi.last_error()
    try:
        bnew = g.bpar * 0.5
        for it in range(2):
            tc.sweep_window(0.45, bnew, 10, 2024, 3 * it, 3)
            tc.to_groups(A, bnew)
            t, T = tc.get()
            capi.check(L.stb_groups_update_pairs(B, orc.u32p(g.n), orc.u16p(t)))
            capi.check(L.stb_groups_update_restaurants(B, orc.u32p(T), orc.dp(bnew)))
            outA, outB = np.zeros(8), np.zeros(8)
            capi.check(L.stb_groups_aterms(A, capi.dp(x), 8, capi.dp(outA)))
            capi.check(L.stb_groups_aterms(B, capi.dp(x), 8, capi.dp(outB)))
            assert np.array_equal(outA, outB), (outA, outB)
            assert not np.array_equal(t, g.t)
    finally:
        tc.free()
        L.stb_groups_free(A)
        L.stb_groups_free(B)


def test_invalid_inputs_leave_the_state():
    g = synth.groups(6, 5, 40, "realistic", seed=9)
    L = capi.lib()
    tc = capi.TableCounts(g.K, g.n, g.t)
    ref = capi.TableCounts(g.K, g.n, g.t)
    try:
        for a, b, W, match in ((1.0, 1.0, 3, "outside"), (-0.1, 1.0, 3, "outside"), (0.5, -0.5, 3, "bpar"),
                               (0.0, 0.0, 3, "bpar"), (0.3, np.nan, 3, "bpar"), (0.5, 1.0, 0, "W=0")):
            with pytest.raises(capi.StbError, match=match):
                tc.sweep_window(a, np.full(g.I, b), W, 1, 0)
            t, T = tc.get()
            assert np.array_equal(t, g.t) and np.array_equal(T, g.T)
        bp = np.ascontiguousarray(g.bpar)
        for flags, nsw, match in ((2, 1, "unknown flags"), (0x80000001, 1, "unknown flags"), (0, -1, "nsweeps=-1")):
            assert L.stb_tcounts_sweep_window(tc.h, 0.5, capi.dp(bp), 3, flags, 1, 0, nsw) != 0
            assert match in capi.last_error()
            t, T = tc.get()
            assert np.array_equal(t, g.t) and np.array_equal(T, g.T)
        assert L.stb_tcounts_sweep_window(tc.h, 0.5, None, 3, 0, 1, 0, 1) != 0
        # nothing above changed what a sweep does
        tc.sweep_window(0.5, g.bpar, 3, 1, 0)
        ref.sweep_window(0.5, g.bpar, 3, 1, 0)
        assert all(np.array_equal(x, y) for x, y in zip(tc.get(), ref.get()))
    finally:
        tc.free()
        ref.free()
