"""Table indicators resampled on the device (stb_tindic_* / stb_sample_tindic): draw for draw against the numpy oracle
(tests/ti_oracle.py), the two kernel forms against each other, in distribution against the exact laws, and handed to a
group set for aterms."""
import math

import numpy as np
import pytest

import orc
import ti_oracle as tio
from libstb_amd import capi, synth

pytestmark = pytest.mark.gpu

FORMS = ("lane", "wave")


def device_vtab(a, maxn, M=0):
    """the slab an stb_tindic object fills for (a, the largest n, M), as an oracle VTab: the draws see the same cells"""
    N = max(maxn, 3)
    M = N if M == 0 else min(M, N)
    v = capi.DeviceVTables(N, M)
    v.fill(a)
    capi.check(capi.lib().stb_fill_status())
    return tio.VTab(v.packed_host(0), N, M), N


def random_state(rng, I, K, nmax):
    n = rng.integers(0, nmax + 1, size=I * K).astype(np.uint32)
    t = np.where(n > 0, 1 + np.floor(rng.random(I * K) * n), 0).astype(np.uint16)
    h = 0.05 + 1.95 * rng.random(I * K)
    return np.full(I, K, dtype=np.int32), n, t, h


def shuffled_order(rng, K, n):
    """every restaurant's customers (local pair indices) in a random order"""
    out, g = [], 0
    for Ki in K:
        seq = np.repeat(np.arange(Ki, dtype=np.uint32), n[g:g + Ki].astype(np.int64))
        rng.shuffle(seq)
        out.append(seq)
        g += Ki
    return np.concatenate(out).astype(np.uint32)


def run(K, n, t, h, cust, M, flags, a, bpar, seed, sweeps, form=None, monkeypatch=None):
    if form:
        monkeypatch.setenv("STB_TINDIC_FORM", form)
    ti = capi.TableIndicators(K, n, t, h, cust, M, flags)
    try:
        ti.sweep(a, bpar, seed, 0, sweeps)
        return ti.get()
    finally:
        ti.free()


# ---- helpers of tests/test_gpu_tcounts.py (copied) ----

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


# ---- draw for draw ----

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("a,b,seed,order,flags,M", [
    (0.0, 2.0, 11, "pair", 0, 0), (0.3, 0.5, 12, "shuffled", 0, 0), (0.75, 20.0, 13, "shuffled", 0, 0),
    (0.3, 5.0, 14, "pair", capi.TI_REF_ODDS, 0), (0.75, 1.0, 15, "shuffled", capi.TI_REF_ODDS, 0),
    (0.5, 3.0, 16, "shuffled", 0, 7), (0.5, 3.0, 17, "pair", capi.TI_REF_ODDS, 7)])
def test_exact_agreement_with_the_oracle(monkeypatch, form, a, b, seed, order, flags, M):
    monkeypatch.setenv("STB_TINDIC_FORM", form)
    rng = np.random.default_rng(seed)
    K, n, t, h = random_state(rng, 24, 9, 60)
    if M:
        t = np.minimum(t, M).astype(np.uint16)
    cust = shuffled_order(rng, K, n) if order == "shuffled" else None
    bpar = b * (0.5 + rng.random(24))
    vt, N = device_vtab(a, int(n.max()), M)
    ti = capi.TableIndicators(K, n, t, h, cust, M, flags)
    try:
        for s in range(3):
            ti.sweep(a, bpar, seed, s)
            got_t, got_T = ti.get()
            t, T = tio.sweep(K, n, t, h, a, bpar, vt, N, seed, s, cust, bool(flags))
            assert np.array_equal(got_t, t), np.flatnonzero(got_t != t)[:10]
            assert np.array_equal(got_T, T)
    finally:
        ti.free()


def test_forms_are_bit_equal(monkeypatch):
    rng = np.random.default_rng(5)
    # short and long restaurants, one with more dishes than a wave keeps in LDS (4096)
    Ks = [3, 40, 1, 5000, 200, 64, 65]
    n = np.concatenate([rng.integers(0, 300 if Ki < 100 else 6, size=Ki) for Ki in Ks]).astype(np.uint32)
    K = np.array(Ks, dtype=np.int32)
    t = np.where(n > 0, 1 + np.floor(rng.random(len(n)) * n), 0).astype(np.uint16)
    h = 0.1 + rng.random(len(n))
    bpar = 0.5 + 10 * rng.random(len(K))
    for cust in (None, shuffled_order(rng, K, n)):
        for flags in (0, capi.TI_REF_ODDS):
            out = [run(K, n, t, h, cust, 0, flags, 0.6, bpar, 99, 4, f, monkeypatch) for f in FORMS]
            assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
            assert not np.array_equal(out[0][0], t)
    # and the oracle agrees on the restaurant above the LDS cap (one sweep)
    cust = shuffled_order(rng, K, n)
    vt, N = device_vtab(0.6, int(n.max()))
    want_t, want_T = tio.sweep(K, n, t, h, 0.6, bpar, vt, N, 7, 0, cust)
    got_t, got_T = run(K, n, t, h, cust, 0, 0, 0.6, bpar, 7, 1, "wave", monkeypatch)
    assert np.array_equal(got_t, want_t) and np.array_equal(got_T, want_T)


@pytest.mark.parametrize("form", FORMS)
def test_queued_sweeps_equal_single_calls(monkeypatch, form):
    monkeypatch.setenv("STB_TINDIC_FORM", form)
    rng = np.random.default_rng(8)
    K, n, t, h = random_state(rng, 50, 6, 120)
    cust = shuffled_order(rng, K, n)
    a, bpar = 0.4, np.full(50, 3.0)
    q = capi.TableIndicators(K, n, t, h, cust)
    r = capi.TableIndicators(K, n, t, h, cust)
    try:
        q.sweep(a, bpar, 21, 4, 3)
        for s in (4, 5, 6):
            r.sweep(a, bpar, 21, s)
            r.get()
        assert all(np.array_equal(x, y) for x, y in zip(q.get(), r.get()))
    finally:
        q.free()
        r.free()


# ---- in distribution ----

def one_dish(n, a, b, h, flags, I, sweeps, seed, start):
    """I one-pair restaurants, t drawn from `start` (a law over t = 1 .. n), `sweeps` sweeps: the t histogram"""
    K = np.ones(I, dtype=np.int32)
    rng = np.random.default_rng(seed)
    t0 = (1 + rng.choice(n, size=I, p=start)).astype(np.uint16)
    got, T = run(K, np.full(I, n, dtype=np.uint32), t0, np.full(I, h), None, 0, flags, a, np.full(I, b), seed, sweeps)
    assert np.array_equal(T, got.astype(np.uint32))
    return np.bincount(got.astype(np.int64) - 1, minlength=n).astype(np.float64)


# (a one-dish chain mixes slowly -- 50 sweeps from t = 1 leave it 0.1 from its law at n = 9, a = 0.9 -- so the
# restaurants start from the joint: then every sweep leaves their law at the joint, exactly when the step is right)
@pytest.mark.parametrize("n,a,b,h", [(9, 0.0, 1.0, 1.0), (9, 0.3, 1.5, 0.5), (12, 0.5, 10.0, 1 / 50), (9, 0.9, 0.5, 2.0)])
def test_distribution_one_dish(n, a, b, h):
    sweeps = 50
    P = tio.sweep_matrix((n,), (h,), a, b, [0], tio.ExactV([n], a))
    joint = tio.joint((n,), (h,), a, b)
    assert np.max(np.abs(joint @ np.linalg.matrix_power(P, sweeps) - joint)) < 1e-12
    counts = one_dish(n, a, b, h, 0, 20000, sweeps, 777, joint)
    assert chi2_p(counts, joint) > 1e-3


def test_distribution_coupled():
    # three dishes that share T_i, customers in a random order per restaurant, from one state: 50 sweeps mix this chain
    a, b = 0.4, 1.5
    ns, hs = (4, 3, 5), (0.5, 1.3, 2.0)
    I, sweeps = 20000, 50
    cells = tio.states(ns)
    p = tio.joint(ns, hs, a, b)
    P = tio.sweep_matrix(ns, hs, a, b, [0] * 4 + [1] * 3 + [2] * 5, tio.ExactV(ns, a))
    assert np.max(np.abs(np.linalg.matrix_power(P, sweeps)[cells.index((4, 1, 2))] - p)) < 1e-9
    rng = np.random.default_rng(3)
    K = np.full(I, 3, dtype=np.int32)
    n = np.tile(np.array(ns, dtype=np.uint32), I)
    t = np.tile(np.array([4, 1, 2], dtype=np.uint16), I)
    cust = shuffled_order(rng, K, n)
    got, T = run(K, n, t, np.tile(hs, I), cust, 0, 0, a, np.full(I, b), 4242, sweeps)
    g = got.reshape(I, 3).astype(np.int64)
    assert np.array_equal(T, g.sum(axis=1).astype(np.uint32))
    idx = {c: j for j, c in enumerate(cells)}
    counts = np.bincount([idx[tuple(r)] for r in g], minlength=len(cells)).astype(np.float64)
    assert chi2_p(counts, p) > 1e-3


def test_distribution_with_the_reference_factor():
    # the reference's chain, started from the joint: its law after 50 sweeps is what its own transition matrix says,
    # and that is not the PYP joint
    n, a, b, h = 9, 0.9, 0.5, 2.0
    sweeps = 50
    P = tio.sweep_matrix((n,), (h,), a, b, [0], tio.ExactV([n], a), ref=True)
    joint = tio.joint((n,), (h,), a, b)
    want = joint @ np.linalg.matrix_power(P, sweeps)
    assert np.max(np.abs(want - joint)) > 0.05
    counts = one_dish(n, a, b, h, capi.TI_REF_ODDS, 20000, sweeps, 778, joint)
    assert chi2_p(counts, want) > 1e-3
    assert chi2_p(counts, joint) < 1e-9


# ---- edges, errors, queues, hand-over ----

@pytest.mark.parametrize("M", [0, 1])
@pytest.mark.parametrize("form", FORMS)
def test_objects_without_a_table(monkeypatch, M, form):
    # every pair n <= 1 (M = 0: the largest n), or M = 1 whatever n: no indicator is ever added, no table is filled
    monkeypatch.setenv("STB_TINDIC_FORM", form)
    if M == 0:
        K = np.array([3, 1, 2], dtype=np.int32)
        n = np.array([1, 0, 1, 1, 0, 0], dtype=np.uint32)
        t = np.array([1, 0, 1, 1, 0, 0], dtype=np.uint16)
    else:
        K = np.array([2, 3], dtype=np.int32)
        n = np.array([50, 0, 7, 1, 300], dtype=np.uint32)
        t = np.array([1, 0, 1, 1, 1], dtype=np.uint16)
    cust = shuffled_order(np.random.default_rng(1), K, n)
    for c in (None, cust):
        ti = capi.TableIndicators(K, n, t, None, c, M)
        try:
            for s, a in enumerate((0.5, 0.0, 0.9)):
                ti.sweep(a, np.full(len(K), 2.0), 3, s)
                got, T = ti.get()
                assert np.array_equal(got, (n > 0).astype(np.uint16))
                assert T.tolist() == [int(x.sum()) for x in np.split(got.astype(np.int64), np.cumsum(K)[:-1])]
        finally:
            ti.free()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pair_order", [True, False])
def test_raw_pairs_outside_the_table_keep_t(monkeypatch, form, pair_order):
    import torch

    monkeypatch.setenv("STB_TINDIC_FORM", form)
    a, N, M = 0.5, 40, 40
    v = capi.DeviceVTables(N, M)
    v.fill(a)
    capi.check(capi.lib().stb_fill_status())
    vt = tio.VTab(v.packed_host(0), N, M)
    K = np.array([3, 1], dtype=np.int32)
    n = np.array([60, 30, 41, 200], dtype=np.uint32)  # n > N but for pair 1
    t = np.array([7, 4, 41, 9], dtype=np.uint16)
    T0 = np.array([52, 9], dtype=np.uint32)
    cust = None if pair_order else shuffled_order(np.random.default_rng(2), K, n)
    coff = np.array([0, 131, 331], dtype=np.uint64)
    dev = "cuda"
    koff = torch.as_tensor(np.array([0, 3, 4], dtype=np.int64), device=dev)
    d_coff = torch.as_tensor(coff.view(np.int64), device=dev)
    d_cust = None if cust is None else torch.as_tensor(cust.view(np.int32), device=dev)
    d_n = torch.as_tensor(n.view(np.int32), device=dev)
    d_t = torch.as_tensor(t.view(np.int16), device=dev).clone()
    d_T = torch.as_tensor(T0.view(np.int32), device=dev).clone()
    d_b = torch.as_tensor(np.array([1.0, 1.0]), device=dev)
    want_t = t
    for s in range(4):
        capi.check(capi.lib().stb_sample_tindic(v.tables.data_ptr(), N, M, a, d_b.data_ptr(), 2, koff.data_ptr(),
                                                d_n.data_ptr(), d_t.data_ptr(), d_T.data_ptr(), None, d_coff.data_ptr(),
                                                None if d_cust is None else d_cust.data_ptr(), 0, 8, s, capi.stream_ptr()))
        want_t, want_T = tio.sweep(K, n, want_t, None, a, [1.0, 1.0], vt, N, 8, s, cust)
    torch.cuda.synchronize()
    got = d_t.cpu().numpy().view(np.uint16)
    T = d_T.cpu().numpy().view(np.uint32)
    assert got[0] == 7 and got[2] == 41 and got[3] == 9 and 1 <= got[1] <= 30
    assert np.array_equal(got, want_t) and np.array_equal(T, want_T)
    assert T.tolist() == [7 + int(got[1]) + 41, 9]


def test_truncation_at_M():
    rng = np.random.default_rng(4)
    K, n, t, h = random_state(rng, 200, 5, 40)
    M = 3
    t = np.minimum(t, M).astype(np.uint16)
    got, _ = run(K, n, t, h, shuffled_order(rng, K, n), M, 0, 0.7, np.full(200, 30.0), 5, 10)
    assert got.max() == M and np.all(got[n > 0] >= 1)


def test_invalid_inputs_leave_the_state():
    g = synth.groups(6, 5, 40, "realistic", seed=9)
    L = capi.lib()
    cust = shuffled_order(np.random.default_rng(0), g.K, g.n)
    with pytest.raises(capi.StbError, match="sum K"):
        capi.TableIndicators(g.K, g.n[:-1], g.t[:-1])
    bad_t = g.t.copy()
    bad_t[3] = 0
    with pytest.raises(capi.StbError, match="t = 0 exactly when n = 0"):
        capi.TableIndicators(g.K, g.n, bad_t)
    bad_t[3] = g.n[3] + 1
    with pytest.raises(capi.StbError, match="pair 3"):
        capi.TableIndicators(g.K, g.n, bad_t)
    with pytest.raises(capi.StbError, match="min\\(n, M=2\\)"):
        capi.TableIndicators(g.K, g.n, np.maximum(g.t, 3).astype(np.uint16), None, None, 2)
    h = np.ones(g.pairs)
    for x in (0.0, np.inf, np.nan, -1.0):
        h[2] = x
        with pytest.raises(capi.StbError, match="h\\[2\\]"):
            capi.TableIndicators(g.K, g.n, g.t, h)
    bad_c = cust.copy()
    bad_c[7] = g.K[0]  # not a pair of restaurant 0
    with pytest.raises(capi.StbError, match="is not a pair of restaurant 0"):
        capi.TableIndicators(g.K, g.n, g.t, None, bad_c)
    bad_c = cust.copy()
    bad_c[1] = (bad_c[0] + 1) % g.K[0] if bad_c[1] == bad_c[0] else bad_c[0]  # one pair visited once too often
    with pytest.raises(capi.StbError, match="visits pair"):
        capi.TableIndicators(g.K, g.n, g.t, None, bad_c)
    with pytest.raises(capi.StbError, match="customers in cust"):
        capi.TableIndicators(g.K, g.n, g.t, None, cust[:-1])
    with pytest.raises(capi.StbError, match="unknown flags"):
        capi.TableIndicators(g.K, g.n, g.t, None, cust, 0, 2)
    with pytest.raises(capi.StbError, match="pass M <= 65535"):
        capi.TableIndicators(np.array([2], dtype=np.int32), np.array([70000, 5], dtype=np.uint32),
                             np.array([3, 2], dtype=np.uint16))
    ti = capi.TableIndicators(g.K, g.n, g.t, None, cust)
    ref = capi.TableIndicators(g.K, g.n, g.t, None, cust)
    try:
        for a, b, match in ((1.0, 1.0, "outside"), (-0.1, 1.0, "outside"), (0.5, -0.5, "bpar"), (0.0, 0.0, "bpar"),
                            (0.3, np.nan, "bpar")):
            with pytest.raises(capi.StbError, match=match):
                ti.sweep(a, np.full(g.I, b), 1, 0)
            t, T = ti.get()
            assert np.array_equal(t, g.t) and np.array_equal(T, g.T)
        h[2] = 0.0
        with pytest.raises(capi.StbError, match="h\\[2\\]"):
            ti.set_h(h)
        assert L.stb_tindic_sweep(ti.h, 0.5, None, 1, 0, 1) != 0
        # nothing above changed what a sweep does
        ti.sweep(0.5, g.bpar, 1, 0)
        ref.sweep(0.5, g.bpar, 1, 0)
        assert all(np.array_equal(x, y) for x, y in zip(ti.get(), ref.get()))
    finally:
        ti.free()
        ref.free()


def test_queued_sweeps_with_a_changing_discount():
    # a new a refills the table behind the sweeps already queued: the same bits as a fresh object at that a
    rng = np.random.default_rng(6)
    K, n, t, h = random_state(rng, 30, 8, 200)
    cust = shuffled_order(rng, K, n)
    bpar = np.full(30, 4.0)
    plan = [(0.2, 0), (0.7, 1), (0.7, 2), (0.0, 3), (0.2, 4)]
    q = capi.TableIndicators(K, n, t, h, cust)
    try:
        for a, s in plan:
            q.sweep(a, bpar, 19, s)
        got = q.get()
    finally:
        q.free()
    cur = t
    for a, s in plan:
        r = capi.TableIndicators(K, n, cur, h, cust)
        try:
            r.sweep(a, bpar, 19, s)
            cur, T = r.get()
        finally:
            r.free()
    assert np.array_equal(got[0], cur) and np.array_equal(got[1], T)


def test_queued_sweeps_with_changing_concentrations():
    g = synth.groups(30, 20, 400, "realistic", seed=3)
    bs = [g.bpar * f for f in (1.0, 0.3, 2.5, 0.3, 0.3, 7.0)]
    q = capi.TableIndicators(g.K, g.n, g.t)
    r = capi.TableIndicators(g.K, g.n, g.t)
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


def make_set(g, t, T, N, M, D):
    L = capi.lib()
    h = L.stb_groups_create(g.I, orc.i32p(g.K), orc.u32p(T), orc.u32p(g.n), orc.u16p(t), orc.dp(g.bpar), N, M, D)
    assert h, capi.last_error()
    return h


def test_hand_over_to_a_group_set():
    L = capi.lib()
    g = synth.groups(100, 10, 200, "realistic", seed=77)
    N = M = int(g.n.max())
    x = synth.discount_grid(8)
    cust = shuffled_order(np.random.default_rng(9), g.K, g.n)
    ti = capi.TableIndicators(g.K, g.n, g.t, None, cust)
    A = make_set(g, g.t, g.T, N, M, 8)
    try:
        bnew = g.bpar * 0.5
        ti.sweep(0.45, bnew, 2024, 0, 3)
        ti.to_groups(A, bnew)
        t, T = ti.get()
        assert not np.array_equal(t, g.t)
        B = make_set(g, t, T, N, M, 8)
        capi.check(L.stb_groups_update_restaurants(B, orc.u32p(T), orc.dp(bnew)))
        outA, outB = np.zeros(8), np.zeros(8)
        capi.check(L.stb_groups_aterms(A, capi.dp(x), 8, capi.dp(outA)))
        capi.check(L.stb_groups_aterms(B, capi.dp(x), 8, capi.dp(outB)))
        L.stb_groups_free(B)
        assert np.allclose(outA, outB, rtol=1e-12, atol=0.0), (outA, outB)
        g2 = synth.groups(10, 5, 50, "realistic")
        D2 = make_set(g2, g2.t, g2.T, 50, 50, 1)
        with pytest.raises(capi.StbError, match="I=10"):
            ti.to_groups(D2)
        L.stb_groups_free(D2)
    finally:
        ti.free()
        L.stb_groups_free(A)
