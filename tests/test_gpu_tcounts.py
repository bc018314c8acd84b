"""Table counts resampled on the device (stb_tcounts_* / stb_sample_tcounts): draw for draw against the numpy oracle
(tests/tc_oracle.py), in distribution against the exact conditional laws, and handed to a group set for aterms."""
import math

import numpy as np
import pytest

import orc
import tc_oracle as tco
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


@pytest.mark.parametrize("a,b,seed", [(0.0, 2.0, 11), (0.3, 0.5, 12), (0.75, 20.0, 13)])
def test_exact_agreement_with_the_oracle(a, b, seed):
    rng = np.random.default_rng(seed)
    K, n, t, h = random_state(rng, 64, 50, 300)
    bpar = np.full(64, b)
    N = M = int(n.max())
    S1, tab = device_table(a, N, M)
    tc = capi.TableCounts(K, n, t, h)
    try:
        for s in range(3):
            tc.sweep(a, bpar, seed, s)
            got_t, got_T = tc.get()
            t, T, ties = tco.sweep(K, n, t, h, a, bpar, M, S1, tab, M, seed, s)
            assert ties == 0, "pick a seed without near-ties"
            assert np.array_equal(got_t, t), np.flatnonzero(got_t != t)[:10]
            assert np.array_equal(got_T, T)
    finally:
        tc.free()


def test_long_rows():
    a, b, seed = 0.5, 3.0, 21
    K = np.array([3, 2, 1, 4], dtype=np.int32)
    n = np.array([10000, 9000, 7777, 10000, 65, 9999, 1, 0, 5000, 10000], dtype=np.uint32)
    t = np.array([1, 300, 4000, 50, 60, 9999, 1, 0, 2, 100], dtype=np.uint16)
    h = np.array([1.0, 0.5, 0.9, 0.2, 1.0, 0.7, 1.0, 1.0, 0.3, 0.8])
    bpar = np.array([b, 0.1, 40.0, b])
    N = M = 10000
    S1, tab = device_table(a, N, M)
    tc = capi.TableCounts(K, n, t, h, M)
    try:
        for s in range(2):
            tc.sweep(a, bpar, seed, s)
            got_t, got_T = tc.get()
            t, T, ties = tco.sweep(K, n, t, h, a, bpar, M, S1, tab, M, seed, s)
            assert ties == 0
            assert np.array_equal(got_t, t) and np.array_equal(got_T, T)
    finally:
        tc.free()


@pytest.mark.parametrize("a,b,h,M", [(0.5, 10.0, 1.0, 200), (0.0, 3.0, 0.25, 200), (0.9, 0.5, 1.0, 20)])
def test_distribution_one_dish(a, b, h, M):
    I, n = 200000, 200
    K = np.ones(I, dtype=np.int32)
    nv = np.full(I, n, dtype=np.uint32)
    tv = np.ones(I, dtype=np.uint16)
    S1, tab = orc.fill_S(a, n, M)
    lw = tco.log_weights(n, 0, a, b, h, M, S1, tab, M)
    p = np.exp(lw - lw.max())
    p /= p.sum()
    tc = capi.TableCounts(K, nv, tv, np.full(I, h), M)
    try:
        tc.sweep(a, np.full(I, b), 777, 0)
        got, T = tc.get()
    finally:
        tc.free()
    assert got.min() >= 1 and got.max() <= min(n, M)
    assert np.array_equal(T, got.astype(np.uint32))
    counts = np.bincount(got.astype(np.int64) - 1, minlength=len(p)).astype(np.float64)
    assert chi2_p(counts, p) > 1e-6


def test_distribution_coupled():
    a, b = 0.4, 1.5
    ns = (6, 4)
    I = 100000
    S1, tab = orc.fill_S(a, 6, 6)
    cells = [(t1, t2) for t1 in range(1, 7) for t2 in range(1, 5)]
    lj = np.array([tco.log_joint(ns, c, a, b, (1.0, 1.0), S1, tab, 6) for c in cells])
    p = np.exp(lj - lj.max())
    p /= p.sum()
    K = np.full(I, 2, dtype=np.int32)
    n = np.tile(np.array(ns, dtype=np.uint32), I)
    t = np.tile(np.array([1, 4], dtype=np.uint16), I)
    tc = capi.TableCounts(K, n, t)
    try:
        tc.sweep(a, np.full(I, b), 4242, 0, 30)
        got, T = tc.get()
    finally:
        tc.free()
    g = got.reshape(I, 2).astype(np.int64)
    assert np.array_equal(T, g.sum(axis=1).astype(np.uint32))
    counts = np.bincount((g[:, 0] - 1) * 4 + (g[:, 1] - 1), minlength=24).astype(np.float64)
    assert chi2_p(counts, p) > 1e-6


def test_determinism_streams_and_sweeps():
    import torch

    g = synth.groups(40, 30, 600, "realistic", seed=5)
    a, N, M = 0.6, int(g.n.max()), int(g.n.max())
    tabs = capi.DeviceTables(N, M)
    tabs.fill(a)
    tabs.status()
    dev = "cuda"
    koff = torch.as_tensor(np.concatenate([[0], np.cumsum(g.K)]).astype(np.int64), device=dev)
    d_n = torch.as_tensor(g.n.view(np.int32), device=dev)
    d_b = torch.as_tensor(g.bpar, device=dev)
    outs = []
    for st in (torch.cuda.Stream(), torch.cuda.Stream(), None):
        d_t = torch.as_tensor(g.t.view(np.int16), device=dev).clone()
        d_T = torch.as_tensor(g.T.view(np.int32), device=dev).clone()
        torch.cuda.synchronize()
        for s in range(2):
            capi.check(capi.lib().stb_sample_tcounts(tabs.tables.data_ptr(), tabs.S1.data_ptr(), N, M, a, d_b.data_ptr(),
                                                     g.I, koff.data_ptr(), d_n.data_ptr(), d_t.data_ptr(), d_T.data_ptr(),
                                                     None, 31, s, capi.stream_ptr(st)))
        torch.cuda.synchronize()
        outs.append((d_t.cpu().numpy().view(np.uint16).copy(), d_T.cpu().numpy().view(np.uint32).copy()))
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1])
    # the object gives the same draws as the raw layer on the same table
    tc = capi.TableCounts(g.K, g.n, g.t)
    tc.sweep(a, g.bpar, 31, 0, 2)
    t2, T2 = tc.get()
    assert np.array_equal(t2, outs[0][0]) and np.array_equal(T2, outs[0][1])
    assert np.array_equal(T2, np.add.reduceat(t2.astype(np.uint32), np.concatenate([[0], np.cumsum(g.K)[:-1]])))
    tc.free()
    # another sweep index (or seed) draws differently
    tc = capi.TableCounts(g.K, g.n, g.t)
    tc.sweep(a, g.bpar, 31, 1, 2)
    t3, _ = tc.get()
    tc.free()
    assert not np.array_equal(t3, t2)


def test_edge_pairs_and_totals():
    K = np.array([5, 1, 2], dtype=np.int32)
    n = np.array([0, 1, 40, 0, 1, 1, 0, 0], dtype=np.uint32)
    t = np.array([0, 1, 7, 0, 1, 1, 0, 0], dtype=np.uint16)
    tc = capi.TableCounts(K, n, t)
    try:
        for s in range(5):
            tc.sweep(0.3, [1.0, 2.0, 3.0], 5, s)
            got, T = tc.get()
            assert got[[0, 3, 6, 7]].tolist() == [0, 0, 0, 0] and got[[1, 4, 5]].tolist() == [1, 1, 1]
            assert 1 <= got[2] <= 40
            assert T.tolist() == [int(got[:5].sum()), int(got[5]), 0]
    finally:
        tc.free()


def test_invalid_inputs_leave_the_state():
    g = synth.groups(6, 5, 40, "realistic", seed=9)
    L = capi.lib()
    bad_t = g.t.copy()
    bad_t[3] = 0
    with pytest.raises(capi.StbError, match="t = 0 exactly when n = 0"):
        capi.TableCounts(g.K, g.n, bad_t)
    bad_t = g.t.copy()
    bad_t[3] = g.n[3] + 1
    with pytest.raises(capi.StbError, match="pair 3"):
        capi.TableCounts(g.K, g.n, bad_t)
    with pytest.raises(capi.StbError, match="min\\(n, M=2\\)"):
        capi.TableCounts(g.K, g.n, np.maximum(g.t, 3).astype(np.uint16), None, 2)
    n0 = g.n.copy()
    n0[0] = 0
    with pytest.raises(capi.StbError, match="t = 0 exactly"):
        capi.TableCounts(g.K, n0, g.t)
    h = np.ones(g.pairs)
    h[2] = 0.0
    with pytest.raises(capi.StbError, match="h\\[2\\]"):
        capi.TableCounts(g.K, g.n, g.t, h)
    h[2] = np.inf
    with pytest.raises(capi.StbError, match="h\\[2\\]"):
        capi.TableCounts(g.K, g.n, g.t, h)
    tc = capi.TableCounts(g.K, g.n, g.t)
    ref = capi.TableCounts(g.K, g.n, g.t)
    try:
        for a, b, match in ((1.0, 1.0, "outside"), (-0.1, 1.0, "outside"), (0.5, -0.5, "bpar"), (0.0, 0.0, "bpar"),
                            (0.3, np.nan, "bpar")):
            with pytest.raises(capi.StbError, match=match):
                tc.sweep(a, np.full(g.I, b), 1, 0)
            t, T = tc.get()
            assert np.array_equal(t, g.t) and np.array_equal(T, g.T)
        with pytest.raises(capi.StbError, match="h\\[2\\]"):
            tc.set_h(h)
        assert L.stb_tcounts_sweep(tc.h, 0.5, None, 1, 0, 1) != 0
        # nothing above changed what a sweep does
        tc.sweep(0.5, g.bpar, 1, 0)
        ref.sweep(0.5, g.bpar, 1, 0)
        assert all(np.array_equal(x, y) for x, y in zip(tc.get(), ref.get()))
    finally:
        tc.free()
        ref.free()


def make_set(g, t, T, N, M, D):
    L = capi.lib()
    h = L.stb_groups_create(g.I, orc.i32p(g.K), orc.u32p(T), orc.u32p(g.n), orc.u16p(t), orc.dp(g.bpar), N, M, D)
    assert h, capi.last_error()
    return h


def test_hand_over_to_a_group_set():
    L = capi.lib()
    g = synth.groups(200, 20, 300, "realistic", seed=77)
    N = M = int(g.n.max())
    x = synth.discount_grid(8)
    a = 0.45
    tc = capi.TableCounts(g.K, g.n, g.t)
    A = make_set(g, g.t, g.T, N, M, 8)
    B = make_set(g, g.t, g.T, N, M, 8)
    C = make_set(g, np.minimum(g.t, 3).astype(np.uint16), g.T, N, 3, 8)  # bounds too small for the new t: they grow
    try:
        bnew = g.bpar * 0.5
        for it in range(2):
            tc.sweep(a, bnew, 2024, 3 * it, 3)
            tc.to_groups(A, bnew)                                # no host copy of the pairs
            tc.to_groups(C, bnew)
            outA, outC = np.zeros(8), np.zeros(8)
            capi.check(L.stb_groups_aterms(A, capi.dp(x), 8, capi.dp(outA)))
            t, T = tc.get()                                      # the host way, for comparison
            capi.check(L.stb_groups_update_pairs(B, orc.u32p(g.n), orc.u16p(t)))
            capi.check(L.stb_groups_update_restaurants(B, orc.u32p(T), orc.dp(bnew)))
            outB = np.zeros(8)
            capi.check(L.stb_groups_aterms(B, capi.dp(x), 8, capi.dp(outB)))
            assert np.array_equal(outA, outB), (outA, outB)
            capi.check(L.stb_groups_aterms(C, capi.dp(x), 8, capi.dp(outC)))
            Nc, Mc = capi.C.c_uint(), capi.C.c_uint()
            capi.check(L.stb_groups_shape(C, None, None, capi.C.byref(Nc), capi.C.byref(Mc), None))
            assert Mc.value == N and Nc.value == N                # min(max n, M): no count read back
            scratch = np.zeros(N + int(orc.oracle().orc_cells(N, M)))
            scratch_c = np.zeros(Nc.value + int(orc.oracle().orc_cells(Nc.value, Mc.value)))
            for d in range(8):
                want = orc.oracle().orc_aterms(float(x[d]), g.I, orc.i32p(g.K), orc.u32p(T), orc.u32p(g.n), orc.u16p(t),
                                               orc.dp(bnew), N, M, orc.dp(scratch))
                assert orc.close(outA[d], want, 1e-10), (d, outA[d], want)
                want_c = orc.oracle().orc_aterms(float(x[d]), g.I, orc.i32p(g.K), orc.u32p(T), orc.u32p(g.n),
                                                 orc.u16p(t), orc.dp(bnew), Nc.value, Mc.value, orc.dp(scratch_c))
                assert orc.close(outC[d], want_c, 1e-10), (d, outC[d], want_c)
        # a set of another shape is refused
        g2 = synth.groups(10, 5, 50, "realistic")
        D2 = make_set(g2, g2.t, g2.T, 50, 50, 1)
        with pytest.raises(capi.StbError, match="I=10"):
            tc.to_groups(D2)
        L.stb_groups_free(D2)
    finally:
        tc.free()
        for s in (A, B, C):
            L.stb_groups_free(s)


@pytest.mark.parametrize("M", [0, 1])
def test_objects_without_a_table(M):
    # every pair n <= 1 (M = 0: the largest n), or M = 1 whatever n: every draw is t = 1 and no table is filled
    if M == 0:
        K = np.array([3, 1, 2], dtype=np.int32)
        n = np.array([1, 0, 1, 1, 0, 0], dtype=np.uint32)
        t = np.array([1, 0, 1, 1, 0, 0], dtype=np.uint16)
    else:
        K = np.array([2, 3], dtype=np.int32)
        n = np.array([50, 0, 7, 1, 300], dtype=np.uint32)
        t = np.array([1, 0, 1, 1, 1], dtype=np.uint16)
    tc = capi.TableCounts(K, n, t, None, M)
    try:
        for s, a in enumerate((0.5, 0.0, 0.9)):
            tc.sweep(a, np.full(len(K), 2.0), 3, s)
            got, T = tc.get()
            assert np.array_equal(got, (n > 0).astype(np.uint16))
            assert T.tolist() == [int(x.sum()) for x in np.split(got.astype(np.int64), np.cumsum(K)[:-1])]
    finally:
        tc.free()


def test_largest_n_beyond_uint16_needs_an_explicit_M():
    K = np.array([2], dtype=np.int32)
    n = np.array([70000, 5], dtype=np.uint32)
    t = np.array([3, 2], dtype=np.uint16)
    with pytest.raises(capi.StbError, match="pass M <= 65535"):
        capi.TableCounts(K, n, t)


def test_raw_pairs_outside_the_table_keep_t():
    import torch

    a, N, M = 0.5, 40, 100
    tabs = capi.DeviceTables(N, M)
    tabs.fill(a)
    tabs.status()
    K = np.array([3, 1], dtype=np.int32)
    n = np.array([60, 30, 41, 200], dtype=np.uint32)    # n > N, with M >= n (60, 41) and M < n (200)
    t = np.array([7, 4, 41, 9], dtype=np.uint16)
    dev = "cuda"
    koff = torch.as_tensor(np.array([0, 3, 4], dtype=np.int64), device=dev)
    d_n = torch.as_tensor(n.view(np.int32), device=dev)
    d_t = torch.as_tensor(t.view(np.int16), device=dev).clone()
    d_T = torch.as_tensor(np.array([52, 9], dtype=np.int32), device=dev)
    d_b = torch.as_tensor(np.array([1.0, 1.0]), device=dev)
    for s in range(4):
        capi.check(capi.lib().stb_sample_tcounts(tabs.tables.data_ptr(), tabs.S1.data_ptr(), N, M, a, d_b.data_ptr(), 2,
                                                 koff.data_ptr(), d_n.data_ptr(), d_t.data_ptr(), d_T.data_ptr(), None,
                                                 8, s, capi.stream_ptr()))
    torch.cuda.synchronize()
    got = d_t.cpu().numpy().view(np.uint16)
    T = d_T.cpu().numpy().view(np.uint32)
    assert got[0] == 7 and got[2] == 41 and got[3] == 9
    assert 1 <= got[1] <= 30
    assert T.tolist() == [7 + int(got[1]) + 41, 9]


def test_queued_sweeps_with_changing_concentrations():
    # sweeps queued back to back, each with new b (the staging buffers are used in turn), against one sweep at a time
    g = synth.groups(30, 20, 400, "realistic", seed=3)
    bs = [g.bpar * f for f in (1.0, 0.3, 2.5, 0.3, 0.3, 7.0)]
    q = capi.TableCounts(g.K, g.n, g.t)
    r = capi.TableCounts(g.K, g.n, g.t)
    try:
        for s, b in enumerate(bs):
            q.sweep(0.4, b, 17, s)
        for s, b in enumerate(bs):
            r.sweep(0.4, b, 17, s)
            r.get()
        tq, Tq = q.get()
        tr, Tr = r.get()
        assert np.array_equal(tq, tr) and np.array_equal(Tq, Tr)
    finally:
        q.free()
        r.free()


# ---- the hand-over to a group set, for both resident-count objects (stb_groups_take_counts)

X3 = np.array([0.2, 0.4, 0.7])


def make(kind, g, t=None, M=0):
    t = g.t if t is None else t
    return capi.TableCounts(g.K, g.n, t, None, M) if kind == "tcounts" else capi.TableIndicators(g.K, g.n, t, None, None, M)


def aterms3(h):
    out = np.zeros(3)
    capi.check(capi.lib().stb_groups_aterms(h, capi.dp(X3), 3, capi.dp(out)))
    return out


def same_bits(x, y):
    return np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64))


@pytest.mark.parametrize("kind", ["tcounts", "tindic"])
def test_refused_hand_overs_leave_both_sides_as_they_were(kind):
    L = capi.lib()
    g = synth.groups(6, 5, 40, "realistic")
    N = M = int(g.n.max())
    obj = make(kind, g)
    A = make_set(g, g.t, g.T, N, M, 3)

    def unchanged(before, t0, T0):
        assert same_bits(aterms3(A), before)
        t, T = obj.get()
        assert np.array_equal(t, t0) and np.array_equal(T, T0)
        obj.to_groups(A, g.bpar)                                  # a valid hand-over still goes through
        assert np.isfinite(aterms3(A)).all()

    try:
        t0, T0 = obj.get()
        # the sentinel from an object that was never given concentrations
        before = aterms3(A)
        with pytest.raises(capi.StbError, match="holds no concentrations"):
            obj.to_groups(A, capi.BPAR_RESIDENT)
        unchanged(before, t0, T0)
        # an evaluation queued and not waited for
        before = aterms3(A)
        out = np.zeros(3)
        capi.check(L.stb_groups_aterms_async(A, capi.dp(X3), 3, capi.dp(out), None))
        with pytest.raises(capi.StbError, match="has not been waited for"):
            obj.to_groups(A, g.bpar)
        capi.check(L.stb_groups_wait(A))
        assert same_bits(out, before)
        unchanged(before, t0, T0)
        # a set between pairs_begin and _commit
        before = aterms3(A)
        capi.check(L.stb_groups_pairs_begin(A))
        with pytest.raises(capi.StbError, match="pairs_begin and"):
            obj.to_groups(A, g.bpar)
        capi.check(L.stb_groups_pairs_put(A, orc.u32p(g.n), orc.u16p(t0), len(g.n), None, None))
        capi.check(L.stb_groups_pairs_commit(A, orc.u32p(T0), orc.dp(g.bpar), 0, 0))
        unchanged(before, t0, T0)
    finally:
        obj.free()
        L.stb_groups_free(A)


@pytest.mark.parametrize("way", ["host", "resident", "none"])
def test_the_two_objects_hand_over_the_same_thing(way):
    L = capi.lib()
    g = synth.groups(6, 5, 40, "realistic")
    N = int(g.n.max())
    assert N > 4
    t4 = np.minimum(g.t, 4).astype(np.uint16)                     # column bound 4, below the largest n
    t3 = np.minimum(g.t, 3).astype(np.uint16)
    off = np.concatenate([[0], np.cumsum(g.K)])
    T4 = np.array([t4[off[i]:off[i + 1]].sum() for i in range(g.I)], dtype=np.uint32)
    T3 = np.array([t3[off[i]:off[i + 1]].sum() for i in range(g.I)], dtype=np.uint32)
    bnew = g.bpar * 0.5
    objs = [make(kind, g, t4, 4) for kind in ("tcounts", "tindic")]
    sets = [make_set(g, t3, T3, N, 3, 3) for _ in objs]           # bounds too small for t = 4: they grow
    H = make_set(g, t3, T3, N, 4, 3)                              # the host route, at the grown bounds
    try:
        outs = []
        for obj, h in zip(objs, sets):
            if way == "host":
                obj.to_groups(h, bnew)
            elif way == "resident":
                obj.set_bpar(bnew)
                obj.to_groups(h, capi.BPAR_RESIDENT)
            else:
                obj.to_groups(h)                                  # the set keeps the bpar it was created with
            Ns, Ms = capi.C.c_uint(), capi.C.c_uint()
            capi.check(L.stb_groups_shape(h, None, None, capi.C.byref(Ns), capi.C.byref(Ms), None))
            assert (Ns.value, Ms.value) == (N, 4)
            outs.append(aterms3(h))
        capi.check(L.stb_groups_update_pairs(H, orc.u32p(g.n), orc.u16p(t4)))
        capi.check(L.stb_groups_update_restaurants(H, orc.u32p(T4), orc.dp(g.bpar if way == "none" else bnew)))
        want = aterms3(H)
        assert np.isfinite(want).all()
        assert same_bits(outs[0], outs[1]) and same_bits(outs[0], want), (outs, want)
    finally:
        for obj in objs:
            obj.free()
        for h in sets + [H]:
            L.stb_groups_free(h)


@pytest.mark.parametrize("kind", ["tcounts", "tindic"])
def test_the_hand_over_holds_later_sweeps_back(kind):
    L = capi.lib()
    g = synth.groups(200, 20, 300, "realistic", seed=77)
    N = M = int(g.n.max())
    a, b, seed = 0.45, g.bpar * 0.5, 2024
    o1, o2, o3 = make(kind, g), make(kind, g), make(kind, g)
    A = make_set(g, g.t, g.T, N, M, 3)
    B = make_set(g, g.t, g.T, N, M, 3)
    try:
        o1.sweep(a, b, seed, 0, 1)
        o1.to_groups(A, b)
        o1.sweep(a, b, seed, 1, 3)                                # at once: the set's copy is still queued
        outA = aterms3(A)
        o2.sweep(a, b, seed, 0, 1)
        t2, T2 = o2.get()
        capi.check(L.stb_groups_update_pairs(B, orc.u32p(g.n), orc.u16p(t2)))
        capi.check(L.stb_groups_update_restaurants(B, orc.u32p(T2), orc.dp(b)))
        assert same_bits(outA, aterms3(B))
        o3.sweep(a, b, seed, 0, 4)
        t1, T1 = o1.get()
        t3, T3 = o3.get()
        assert np.array_equal(t1, t3) and np.array_equal(T1, T3) and not np.array_equal(t1, t2)
    finally:
        for o in (o1, o2, o3):
            o.free()
        for h in (A, B):
            L.stb_groups_free(h)
