"""The hyper-parameter half of the Gibbs loop from device-resident counts: stb_sample_logq (hyperq.hip) against its
numpy replay and its law, Q's reduction -- also past one trip per workgroup and past the block sums first allocated, on
sizes taken from stb_reduce_geometry --, the b step on the tcounts / tindic objects, stb_groups_samplea on sets the
device filled, the refusals, and examples/pyp_resample -d."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from devarr import dev_coff, dev_u32
import hq_oracle as hq
import orc
from libstb_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


class waves:
    """STB_HYPERQ_WAVES for the calls inside"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        self.old = os.environ.get("STB_HYPERQ_WAVES")
        os.environ["STB_HYPERQ_WAVES"] = str(self.v)

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("STB_HYPERQ_WAVES", None)
        else:
            os.environ["STB_HYPERQ_WAVES"] = self.old


# ---- replay

@pytest.mark.parametrize("b", [0.01, 0.7, 10.0, 2000.0])
def test_L_equals_the_replay(b):
    I = 2 * 10 ** 5
    N = hq.mixed_restaurants(I)
    assert (N == 0).any() and (N == 1).any() and N.max() == 10 ** 7
    Q, Lt = capi.sample_logq(b, 20.0, dev_u32(N), seed=9001, sweep=11)
    L = Lt.cpu().numpy()
    want = hq.replay_L(b, N, seed=9001, sweep=11)
    assert (L[N == 0] == 0).all()
    assert np.isfinite(L).all() and (L[N > 0] > 0).all()
    out = np.abs(L - want) > 1e-12 * np.maximum(1.0, want)
    worst = float(np.max(np.abs(L - want)[~out] / np.maximum(1.0, want[~out])))
    print("b=%g: %d of %d restaurants outside 1e-12; worst of the rest %.2e" % (b, int(out.sum()), I, worst))
    assert out.sum() <= I // 10 ** 5, np.nonzero(out)[0][:10]


# ---- reduction

@pytest.mark.parametrize("I", [1, 255, 256, 257, 1000, 200000])
def test_Q_has_the_same_bits_for_every_geometry_and_equals_the_sum(I):
    N = hq.mixed_restaurants(max(I, 8))[:I]
    if I == 1:
        N[:] = 5
    Nd = dev_u32(N)
    scale = 20.0
    qs = []
    L0 = None
    for wv in (1, 2, 4, 8, 4):
        with waves(wv):
            Q, Lt = capi.sample_logq(0.7, scale, Nd, seed=31, sweep=2)
        qs.append(Q)
        L = Lt.cpu().numpy()
        if L0 is None:
            L0 = L
        assert np.array_equal(L, L0)
    assert all(q == qs[0] for q in qs), [q.hex() for q in qs]
    want = 1.0 / scale + math.fsum(L0)
    print("I=%d: Q=%.17g, |Q - fsum| = %.3e (bar %.3e)" % (I, qs[0], abs(qs[0] - want), 4 * U * I * abs(qs[0])))
    assert abs(qs[0] - want) <= 4 * U * I * abs(qs[0])
    Q2, none = capi.sample_logq(0.7, scale, Nd, seed=31, sweep=2, want_L=False)   # (d_L = NULL)
    assert none is None and Q2 == qs[0]


def test_Q_without_restaurants_is_one_over_scale():
    import torch

    Q, _ = capi.sample_logq(1.0, 4.0, torch.zeros(0, dtype=torch.int32, device="cuda"), seed=1, sweep=0)
    assert Q == 0.25
    Q, Lt = capi.sample_logq(1.0, 4.0, dev_u32(np.zeros(300)), seed=1, sweep=0)
    assert Q == 0.25 and (Lt.cpu().numpy() == 0).all()


# ---- past one trip per workgroup

HQ_CASES = ["second trip, four waves", "second trip, eight waves", "third trip, four waves", "third trip, eight waves",
            "odd chunks, eight waves"]


def hq_geom(I, wv=0):
    return capi.reduce_geometry(capi.GEOM_LOGQ, I, waves=wv)


def hq_case(label):
    """I and the case's premise, asserted through the query -- every size from the device at hand"""
    wv = 8 if "eight" in label else 4
    W = hq_geom(1 << 30, wv).grid_x
    span = 256 * hq_geom(1, wv).chunks
    assert span == (512 if wv == 8 else 256)
    if label.startswith("second"):
        I = span * W + 1
        g = hq_geom(I, wv)
        assert g.grid_x == W and g.steps == g.grid_x + 1
    elif label.startswith("third"):
        I = 2 * span * W + 257 + 64
        g = hq_geom(I, wv)
        assert g.grid_x == W and g.steps > 2 * g.grid_x and g.blocks == 2 * g.chunks * W + 2
    else:   # the last step of a workgroup of eight waves holds one block, not two
        I = 2 * span * W + 64
        g = hq_geom(I, wv)
        assert g.chunks == 2 and g.blocks % 2 == 1 and g.steps > 2 * g.grid_x
    return I


def trip_windows(I):
    """the first 512 restaurants, the 512 either side of every trip boundary (at four and at eight waves), the last 512"""
    starts = {0, max(I - 512, 0)}
    for wv in (4, 8):
        g = hq_geom(I, wv)
        trip = g.grid_x * g.chunks * 256
        starts |= {k - 512 for k in range(trip, I, trip)}
        assert g.steps <= g.grid_x or any(k for k in range(trip, I, trip))
    return sorted(starts)


def check_L_on_windows(L, N, b, seed, sweep, what):
    """test_L_equals_the_replay's criterion on the windows: outside 1e-12 at most one restaurant in 10^5, rounded down --
    none, the windows holding fewer than 10^5"""
    I = len(N)
    nout = ntot = 0
    for w0 in trip_windows(I):
        w1 = min(w0 + 1024, I) if 0 < w0 < I - 512 else min(w0 + 512, I)
        want = hq.replay_L(b, N[w0:w1], seed=seed, sweep=sweep, first=w0)
        got = L[w0:w1]
        assert (got[N[w0:w1] == 0] == 0).all() and np.isfinite(got).all() and (got[N[w0:w1] > 0] > 0).all()
        out = np.abs(got - want) > 1e-12 * np.maximum(1.0, want)
        nout += int(out.sum())
        ntot += w1 - w0
    print("%s: %d of %d restaurants on the windows outside 1e-12" % (what, nout, ntot))
    assert ntot >= 1024 and nout <= ntot // 10 ** 5


def all_geometries(I, N, b, scale, seed, sweep):
    """(Q, L) for 1, 2, 4, 8 waves and again 4: the same bits each time; and with the customers as prefix sums"""
    Nd = dev_u32(N)
    Q0 = L0 = None
    for wv in (1, 2, 4, 8, 4):
        with waves(wv):
            assert hq_geom(I).waves == wv
            Q, Lt = capi.sample_logq(b, scale, Nd, seed=seed, sweep=sweep)
        L = Lt.cpu().numpy()
        if L0 is None:
            Q0, L0 = Q, L
        assert np.array_equal(L, L0) and Q == Q0, (wv, Q.hex(), Q0.hex())
    Q2, none = capi.sample_logq(b, scale, Nd, seed=seed, sweep=sweep, want_L=False)
    assert none is None and Q2 == Q0
    Q3, Lt = capi.sample_logq(b, scale, None, seed=seed, sweep=sweep, coff=dev_coff(N))
    assert Q3 == Q0 and np.array_equal(Lt.cpu().numpy(), L0)
    return Q0, L0


def check_Q(Q, L, I, scale, what):
    want = 1.0 / scale + math.fsum(L)
    print("%s I=%d: Q=%.17g, |Q - fsum| = %.3e (bar %.3e)" % (what, I, Q, abs(Q - want), 4 * U * I * abs(Q)))
    assert abs(Q - want) <= 4 * U * I * abs(Q)


@pytest.mark.parametrize("label", HQ_CASES)
def test_L_and_Q_past_one_trip_per_workgroup(label):
    I = hq_case(label)
    N = hq.mixed_restaurants(I)
    b, scale = 0.7, 20.0
    Q, L = all_geometries(I, N, b, scale, seed=4711, sweep=3)
    check_L_on_windows(L, N, b, 4711, 3, label)
    assert (L[N == 0] == 0).all() and np.isfinite(L).all() and (L[N > 0] > 0).all()
    check_Q(Q, L, I, scale, label)


def test_a_call_that_outgrows_the_block_sums_and_the_calls_after_it():
    cap0 = int(hq_geom(1).cap0)
    big, small = cap0 * 256 + 1, 1000
    gb, gs = hq_geom(big), hq_geom(small)
    assert gb.need == gb.cap0 + 1 and gs.need <= gs.cap0
    b, scale = 0.7, 20.0
    Nb, Ns = hq.mixed_restaurants(big), hq.mixed_restaurants(small)
    capi.lib().stb_sampler_cache_clear()   # (this thread's buffer of block sums: the next call allocates cap0 afresh)
    Qs, Lts = capi.sample_logq(b, scale, dev_u32(Ns), seed=31, sweep=2)
    Ls = Lts.cpu().numpy()
    Q, L = all_geometries(big, Nb, b, scale, seed=31, sweep=2)   # replaces the buffer
    check_L_on_windows(L, Nb, b, 31, 2, "regrow")
    check_Q(Q, L, big, scale, "regrow")
    Qs2, Lts2 = capi.sample_logq(b, scale, dev_u32(Ns), seed=31, sweep=2)   # a smaller call in the larger buffer
    assert Qs2 == Qs and np.array_equal(Lts2.cpu().numpy(), Ls)
    check_Q(Qs, Ls, small, scale, "after the larger call")
    Q2, Lt2 = capi.sample_logq(b, scale, dev_u32(Nb), seed=31, sweep=2)    # ... and the large one again
    assert Q2 == Q and np.array_equal(Lt2.cpu().numpy(), L)


# ---- law

@pytest.mark.parametrize("b", [0.01, 0.5, 1.0, 10.0, 2000.0])
@pytest.mark.parametrize("N", [1, 7, 200, 10 ** 5])
def test_moments_of_the_devices_L(b, N):
    n = 10 ** 6
    _, Lt = capi.sample_logq(b, 20.0, dev_u32(np.full(n, N)), seed=20240 + N, sweep=int(b * 100))
    L = Lt.cpu().numpy()
    assert np.isfinite(L).all() and (L > 0).all()
    ok, text = hq.moment_check(L, b, N)
    print(text)
    assert ok, text


# ---- b step

def objects(g, M=0):
    tc = capi.TableCounts(g.K, g.n, g.t, None, M)
    ti = capi.TableIndicators(g.K, g.n, g.t, None, None, M)
    return tc, ti


@pytest.mark.parametrize("sampler", ["ars", "slice"])
def test_b_step_on_the_objects(sampler, monkeypatch):
    monkeypatch.setenv("STB_SAMPLER", sampler)
    L, O = capi.lib(), orc.oracle()
    g = synth.groups(3000, 20, 300, "realistic", seed=5)
    tc, ti = objects(g)
    a, b = 0.4, 12.0
    try:
        # sweeps are queued, nothing is read back before the b step
        tc.sweep(a, np.full(g.I, b), 77, 0, 2)
        got = []
        for obj in (tc, ti):
            if obj is ti:   # the same state in the other object: the pairs the first one holds now
                t_now, T_now = tc.get()
                ti.free()
                ti = obj = capi.TableIndicators(g.K, g.n, t_now, None, None, 0)
            orc.seed_libc(777, 4242)
            bn = obj.sampleb(b, g.shape, g.scale, a, seed=123, sweep=9, loops=2)
            xs, ys, code = capi.sampler_trace()
            got.append((bn, xs, ys, L.stb_sampleb_last_Q()))
        t_now, T_now = tc.get()
        (b1, x1, y1, Q1), (b2, x2, y2, Q2) = got
        assert Q1 == Q2 and b1 == b2 and np.array_equal(x1, x2) and np.array_equal(y1, y2)
        assert 0.01 <= b1 <= 2000 and b1 != b
        # Q is the replay's sum (N_i the sum of n over restaurant i's pairs): every L within 1e-12 relative of the replay's
        # (test_L_equals_the_replay) plus the reduction's 4 u I |Q| = 1.4e-12 |Q| at I = 3000
        Lw = hq.replay_L(b, g.N, seed=123, sweep=9)
        assert abs(Q1 - (1 / g.scale + math.fsum(Lw))) <= (1e-12 + 4 * U * g.I) * Q1
        assert len(x1) >= 1
        if sampler == "ars":
            lo, hi = 0.01, 2000.0
            assert np.array_equal(x1[:3], np.array([lo + (k + 1.0) * (hi - lo) / 4.0 for k in range(3)]))
        want = np.array([O.orc_bterms(float(x), Q1, g.shape, g.I, orc.u32p(T_now), a) for x in x1])
        err = np.max(np.abs(y1 - want) / np.maximum(1.0, np.abs(want)))
        print("%s: %d evaluations, b %.6g -> %.6g, worst y error %.2e" % (sampler, len(x1), b, b1, err))
        assert err <= 1e-10
        # t and T are not written by the step
        t2, T2 = ti.get()
        assert np.array_equal(t2, t_now) and np.array_equal(T2, T_now)
    finally:
        tc.free()
        ti.free()
        L.stb_sampler_cache_clear()


def test_b_step_raw_entry_point_matches_the_object():
    L = capi.lib()
    g = synth.groups(500, 10, 100, "realistic", seed=8)
    tc = capi.TableCounts(g.K, g.n, g.t)
    try:
        orc.seed_libc(5, 6)
        want = tc.sampleb(3.0, g.shape, g.scale, 0.3, seed=4, sweep=1)
        orc.seed_libc(5, 6)
        got = capi.sampleb_device(3.0, g.shape, g.scale, dev_u32(g.N), dev_u32(g.T), 0.3, seed=4, sweep=1)
        assert got == want
    finally:
        tc.free()
        L.stb_sampler_cache_clear()


def test_b_step_with_zero_discount_is_the_gamma_draw():
    """a = 0: b Q ~ Gamma(shape + sum T) exactly (sum T <= 400: lib/sampleb.c:101-118 draws the Gamma itself)"""
    L = capi.lib()
    g = synth.groups(6, 4, 30, "realistic", seed=3)
    tc = capi.TableCounts(g.K, g.n, g.t)
    k = g.shape + float(g.T.sum())
    assert k < 400
    try:
        orc.seed_libc(1, 2024)
        vals = []
        for c in range(4000):
            bn = tc.sampleb(5.0, g.shape, g.scale, 0.0, seed=1000 + c // 100, sweep=c)
            assert 0.01 < bn < 2000   # (the clamps do not bite here)
            vals.append(bn * L.stb_sampleb_last_Q())
        vals = np.array(vals)
        z = (vals.mean() - k) / math.sqrt(k / len(vals))
        print("a=0: mean of b Q %.4f, exact %.4f, z=%+.2f" % (vals.mean(), k, z))
        assert abs(z) <= 5
        t2, T2 = tc.get()
        assert np.array_equal(t2, g.t) and np.array_equal(T2, g.T)
    finally:
        tc.free()
        L.stb_sampler_cache_clear()


# ---- a step

def test_a_step_on_sets_the_device_filled():
    L, O = capi.lib(), orc.oracle()
    g = synth.groups(400, 25, 600, "realistic", seed=21)
    a, b = 0.45, 8.0
    bpar = np.full(g.I, b)
    tc = capi.TableCounts(g.K, g.n, g.t)
    h1 = L.stb_groups_create(g.I, orc.i32p(g.K), None, None, None, None, 0, 0, 3)
    h2 = None
    assert h1, capi.last_error()
    try:
        tc.sweep(a, bpar, 55, 0, 2)
        tc.to_groups(h1, bpar)
        orc.seed_libc(4321, 99)
        a1 = capi.groups_samplea(h1, a)
        x1, y1, c1 = capi.sampler_trace()
        # the same pairs through the host, the same bounds
        t_now, T_now = tc.get()
        Nb, Mb = C.c_uint(), C.c_uint()
        assert L.stb_groups_shape(h1, None, None, C.byref(Nb), C.byref(Mb), None) == 0
        h2 = L.stb_groups_create(g.I, orc.i32p(g.K), orc.u32p(T_now), orc.u32p(g.n), orc.u16p(t_now), orc.dp(bpar), Nb.value,
                                 Mb.value, 3)
        assert h2, capi.last_error()
        orc.seed_libc(4321, 99)
        a2 = capi.groups_samplea(h2, a)
        x2, y2, c2 = capi.sampler_trace()
        assert a1 == a2 and c1 == c2 and np.array_equal(x1, x2) and np.array_equal(y1, y2)
        assert max(0.01, a - 0.2) <= a1 <= min(0.98, a + 0.2) and a1 != a
        scratch = np.zeros(Nb.value + int(O.orc_cells(Nb.value, Mb.value)))
        want = np.array([O.orc_aterms(float(x), g.I, orc.i32p(g.K), orc.u32p(T_now), orc.u32p(g.n), orc.u16p(t_now),
                                      orc.dp(bpar), Nb.value, Mb.value, orc.dp(scratch)) for x in x1])
        err = np.max(np.abs(y1 - want) / np.maximum(1.0, np.abs(want)))
        print("a step: %d evaluations, a %.4f -> %.6f, worst y error %.2e" % (len(x1), a, a1, err))
        assert err <= 1e-10
        # the host samplea() on the same pairs: the same bracket, hence the same three starting abscissae
        gg = synth.Groups(I=g.I, K=g.K, n=g.n, t=t_now, T=T_now, N=g.N, bpar=bpar)
        NP, TP = C.POINTER(C.c_uint32) * g.I, C.POINTER(C.c_uint16) * g.I
        nn, tt = NP(), TP()
        off = 0
        for i in range(g.I):
            nn[i] = C.cast(gg.n.ctypes.data + 4 * off, C.POINTER(C.c_uint32))
            tt[i] = C.cast(gg.t.ctypes.data + 2 * off, C.POINTER(C.c_uint16))
            off += int(g.K[i])
        orc.seed_libc(4321, 99)
        a3 = L.samplea(a, g.I, orc.i32p(g.K), orc.u32p(T_now), nn, tt, None, orc.dp(bpar), None, 1, 0)
        x3, y3, c3 = capi.sampler_trace()
        lo, hi = a - 0.2, a + 0.2
        assert np.array_equal(x3[:3], x1[:3])
        assert np.array_equal(x1[:3], np.array([lo + (k + 1.0) * (hi - lo) / 4.0 for k in range(3)]))
        assert lo <= a3 <= hi
    finally:
        tc.free()
        L.stb_groups_free(h1)
        if h2:
            L.stb_groups_free(h2)
        L.stb_sampler_cache_clear()


def test_a_step_after_the_indicator_sweep():
    """the loop of examples/pyp_resample -d: sweep -> b -> to_groups -> a, nothing read back in between"""
    L = capi.lib()
    g = synth.groups(200, 10, 200, "realistic", seed=2)
    ti = capi.TableIndicators(g.K, g.n, g.t)
    h = L.stb_groups_create(g.I, orc.i32p(g.K), None, None, None, None, 0, 0, 3)
    assert h, capi.last_error()
    try:
        a, b = 0.3, 5.0
        orc.seed_libc(11, 12)
        for it in range(3):
            ti.sweep(a, np.full(g.I, b), 900, it, 1)
            b = ti.sampleb(b, 1.1, 20.0, a, seed=901, sweep=it)
            ti.to_groups(h, np.full(g.I, b))
            a = capi.groups_samplea(h, a)
            assert 0.01 <= a <= 0.98 and 0.01 <= b <= 2000
    finally:
        ti.free()
        L.stb_groups_free(h)
        L.stb_sampler_cache_clear()


# ---- refusals

def test_refused_inputs_leave_the_state_as_it_was():
    import torch

    L = capi.lib()
    g = synth.groups(50, 5, 50, "realistic", seed=1)
    tc, ti = objects(g)
    Nd = dev_u32(g.N)
    Q = C.c_double(-1.0)
    try:
        for bad_b, bad_scale in ((0.0, 1.0), (-1.0, 1.0), (float("nan"), 1.0), (float("inf"), 1.0), (1.0, 0.0), (1.0, -2.0)):
            assert L.stb_sample_logq(bad_b, bad_scale, g.I, Nd.data_ptr(), None, C.byref(Q), 1, 0, None) != 0
            assert "stb_sample_logq" in capi.last_error() and Q.value == -1.0
        assert L.stb_sample_logq(1.0, 1.0, g.I, None, None, C.byref(Q), 1, 0, None) != 0
        assert L.stb_sample_logq(1.0, 1.0, -1, Nd.data_ptr(), None, C.byref(Q), 1, 0, None) != 0
        for obj, fn in ((tc, L.stb_tcounts_sampleb), (ti, L.stb_tindic_sampleb)):
            for b_in, scale, a in ((1.0, 20.0, -0.1), (1.0, 20.0, 1.0), (-0.5, 20.0, 0.3), (float("nan"), 20.0, 0.3),
                                   (float("inf"), 20.0, 0.3), (1.0, 0.0, 0.3), (1.0, -1.0, 0.3), (0.0, 20.0, 0.0)):
                r = fn(obj.h, b_in, 1.1, scale, a, None, 1, 0, 1, 0)
                assert r != r and capi.last_error(), (b_in, scale, a)
            r = fn(None, 1.0, 1.1, 20.0, 0.3, None, 1, 0, 1, 0)
            assert r != r and "null object" in capi.last_error()
            t2, T2 = obj.get()
            assert np.array_equal(t2, g.t) and np.array_equal(T2, g.T)
        r = L.stb_sampleb_device(1.0, g.I, 1.1, 20.0, None, dev_u32(g.T).data_ptr(), 0.3, None, 1, 0, 1, 0, None)
        assert r != r and "d_N" in capi.last_error()
        r = L.stb_groups_samplea(None, 0.5, None, 1, 0)
        assert r != r and "null" in capi.last_error()
        h = L.stb_groups_create(g.I, orc.i32p(g.K), None, None, None, None, 0, 0, 3)   # no pairs yet
        assert h
        r = L.stb_groups_samplea(h, 0.5, None, 1, 0)
        assert r != r and capi.last_error()
        tc.to_groups(h, g.bpar)
        for bad_a in (0.0, 1.0, -0.2, float("nan")):
            r = L.stb_groups_samplea(h, bad_a, None, 1, 0)
            assert r != r and "outside" in capi.last_error()
        orc.seed_libc(1, 1)
        assert 0.01 <= capi.groups_samplea(h, 0.5) <= 0.98   # (and the set still works)
        L.stb_groups_free(h)
        # the objects still work
        assert 0.01 <= tc.sampleb(2.0, 1.1, 20.0, 0.3, 1, 0) <= 2000
    finally:
        tc.free()
        ti.free()
        L.stb_sampler_cache_clear()
    del torch


# ---- example

def test_example_runs_its_loop_on_the_device():
    exe = os.path.join(ROOT, "examples", "bin", "pyp_resample")
    assert os.path.exists(exe), "examples/bin/pyp_resample not built (make -C libstb_amd/csrc)"
    p = subprocess.run([exe, "-d", "-J", "3", "-n", "2000", "-a", "0.4", "-b", "15", "-c", "45", "-s", "3"], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert re.search(r"^data: 3 restaurants x 2000 customers", p.stdout, re.M), p.stdout
    m = re.search(r"posterior means after 45 sweeps: a=([0-9.]+) b=([0-9.]+); tables:", p.stdout)
    assert m, p.stdout
    a, b = float(m.group(1)), float(m.group(2))
    print(p.stdout)
    assert math.isfinite(a) and math.isfinite(b)
    assert 0.01 <= a <= 0.98 and 0.01 <= b <= 2000
