"""Customers' dishes resampled on the device (stb_tindic_sweep_dishes / stb_sample_tdishes): draw for draw against the numpy
oracle (tests/td_oracle.py), against the indicator sweep where no customer can move, in distribution against the exact
joint, and mixed with the object's other calls."""
import math

import numpy as np
import pytest

import orc
import td_oracle as tdo
import ti_oracle as tio
from libstb_amd import capi, synth

pytestmark = pytest.mark.gpu


def grown_vtab(a, maxNi, Mgiven=0):
    """the slab an stb_tindic object holds after its first dish sweep, as an oracle VTab: (vt, N, M)"""
    N = max(maxNi, 3)
    M = min(Mgiven if Mgiven else max(maxNi, 1), N)
    v = capi.DeviceVTables(N, M)
    v.fill(a)
    capi.check(capi.lib().stb_fill_status())
    return tio.VTab(v.packed_host(0), N, M), N, M


def max_Ni(K, n):
    return int(max(x.sum() for x in np.split(np.asarray(n, dtype=np.int64), np.cumsum(K)[:-1])))


def random_state(rng, Ks, nmax):
    K = np.array(Ks, dtype=np.int32)
    G = int(K.sum())
    n = rng.integers(0, nmax + 1, size=G).astype(np.uint32)
    t = np.where(n > 0, 1 + np.floor(rng.random(G) * n), 0).astype(np.uint16)
    h = 0.05 + 1.95 * rng.random(G)
    return K, n, t, h


def shuffled_order(rng, K, n):
    out, g = [np.zeros(0, dtype=np.uint32)], 0
    for Ki in K:
        seq = np.repeat(np.arange(Ki, dtype=np.uint32), n[g:g + Ki].astype(np.int64))
        rng.shuffle(seq)
        out.append(seq)
        g += Ki
    return np.concatenate(out).astype(np.uint32)


def random_lik(rng, rows, stride, zeros=0.15):
    lik = 0.05 + 3.0 * rng.random((rows, stride))
    lik[rng.random((rows, stride)) < zeros] = 0.0
    return lik


def fetch(ti):
    t, T = ti.get()
    n, cust = ti.get_state()
    return n, t, T, cust


def assert_state(got, want):
    for name, g, w in zip(("n", "t", "T", "cust"), got, want):
        assert np.array_equal(g, w), (name, np.flatnonzero(np.asarray(g) != np.asarray(w))[:10])


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

def replay(K, n, t, h, cust, cls, lik, Mgiven, a, bpar, seed, sweeps=3):
    """`sweeps` dish sweeps on an object and in the oracle, compared after every one"""
    vt, N, M = grown_vtab(a, max_Ni(K, n), Mgiven)
    ti = capi.TableIndicators(K, n, t, h, cust, Mgiven)
    try:
        if cls is not None:
            ti.set_classes(cls, lik.shape[0])
            ti.set_lik(lik)
        moved = 0
        for s in range(sweeps):
            info = ti.sweep_dishes(a, bpar, seed, s)
            n, t, T, new, skipped, stuck = tdo.sweep(K, n, t, h, a, bpar, vt, N, M, seed, s, cust, cls, lik)
            moved += int(np.sum(new != cust))
            cust = new
            assert_state(fetch(ti), (n, t, T, cust))
            assert (info.skipped, info.stuck) == (skipped, stuck)
        assert moved > 0
    finally:
        ti.free()


@pytest.mark.parametrize("a,b,seed,rows,M", [(0.0, 2.0, 31, 2, 0), (0.3, 0.5, 32, 3, 0), (0.75, 20.0, 33, 4, 0),
                                             (0.5, 3.0, 34, 3, 7)])
def test_exact_agreement_with_the_oracle(a, b, seed, rows, M):
    rng = np.random.default_rng(seed)
    K, n, t, h = random_state(rng, [9] * 24, 60)
    if M:
        t = np.minimum(t, M).astype(np.uint16)
    cust = shuffled_order(rng, K, n)
    cls = rng.integers(0, rows, size=len(cust)).astype(np.uint32)
    replay(K, n, t, h, cust, cls, random_lik(rng, rows, 9), M, a, b * (0.5 + rng.random(24)), seed)


@pytest.mark.parametrize("Ks", [[1, 64, 65, 130], [1, 64, 7, 63]])
def test_exact_agreement_across_the_scan_blocks(Ks):
    # 64 | 65: the block boundary; 130: two full blocks and padded lanes; the second set stays in the register form
    rng = np.random.default_rng(41)
    K, n, t, h = random_state(rng, Ks, 5)
    cust = shuffled_order(rng, K, n)
    cls = rng.integers(0, 3, size=len(cust)).astype(np.uint32)
    replay(K, n, t, h, cust, cls, random_lik(rng, 3, 136), 0, 0.4, 1.0 + rng.random(len(Ks)), 42)


def test_exact_agreement_without_a_likelihood():
    rng = np.random.default_rng(51)
    K, n, t, h = random_state(rng, [9] * 24, 60)
    cust = shuffled_order(rng, K, n)
    replay(K, n, t, h, cust, None, None, 0, 0.3, 2.0 * (0.5 + rng.random(24)), 52)


# ---- equality with the indicator sweep ----

def with_a_full_restaurant(K, n, t, h):
    """one more restaurant of one dish holding max_i N_i customers: an indicator object of these pairs has the bounds a
    dish object grows to, so the two read the same V cells"""
    big = max_Ni(K, n)
    return (np.append(K, 1).astype(np.int32), np.append(n, big).astype(np.uint32), np.append(t, 1).astype(np.uint16),
            np.append(h, 1.0))


@pytest.mark.parametrize("case", ["one_dish", "one_hot"])
def test_a_customer_that_cannot_move_gets_the_indicator_sweeps_bits(case):
    rng = np.random.default_rng(61)
    if case == "one_dish":
        K, n, t, h = random_state(rng, [1] * 200, 50)
        cust = shuffled_order(rng, K, n)
        cls = lik = None
    else:
        K, n, t, h = with_a_full_restaurant(*random_state(rng, [9] * 24, 60))
        cust = shuffled_order(rng, K, n)
        cls, lik = cust.copy(), np.eye(9)  # every row one-hot on the customer's own dish
    bpar = 0.5 + 3.0 * rng.random(len(K))
    d = capi.TableIndicators(K, n, t, h, cust)
    r = capi.TableIndicators(K, n, t, h, cust)
    try:
        if cls is not None:
            d.set_classes(cls, 9)
            d.set_lik(lik)
        for s, a in enumerate((0.6, 0.6, 0.2)):
            info = d.sweep_dishes(a, bpar, 62, s)
            r.sweep(a, bpar, 62, s)
            assert (info.skipped, info.stuck) == (0, 0)
        got = fetch(d)
        assert_state(got, (n, r.get()[0], r.get()[1], cust))
        assert not np.array_equal(got[1], t)
    finally:
        d.free()
        r.free()


# ---- invariants ----

def test_invariants_on_random_shapes():
    import torch

    rng = np.random.default_rng(71)
    K, n, t, h = random_state(rng, list(rng.integers(1, 41, size=40)) + [70, 100], 12)
    M = 6
    t = np.minimum(t, M).astype(np.uint16)
    cust = shuffled_order(rng, K, n)
    cls = rng.integers(0, 3, size=len(cust)).astype(np.uint32)
    lik = random_lik(rng, 3, 104)
    a, bpar = 0.45, 0.3 + 4.0 * rng.random(len(K))
    Ni = np.array([x.sum() for x in np.split(n.astype(np.int64), np.cumsum(K)[:-1])])
    ti = capi.TableIndicators(K, n, t, h, cust, M)
    try:
        ti.set_classes(cls, 3)
        ti.set_lik(lik)
        ti.sweep_dishes(a, bpar, 72, 0, 4)
        n1, t1, T1, c1 = fetch(ti)
        assert not np.array_equal(n1, n)
        koff = np.concatenate([[0], np.cumsum(K)]).astype(np.int64)
        coff = np.concatenate([[0], np.cumsum(Ni)]).astype(np.int64)
        for i in range(len(K)):
            ni, tt = n1[koff[i]:koff[i + 1]].astype(np.int64), t1[koff[i]:koff[i + 1]].astype(np.int64)
            assert ni.sum() == Ni[i] and T1[i] == tt.sum()
            assert np.array_equal(np.bincount(c1[coff[i]:coff[i + 1]].astype(np.int64), minlength=K[i]), ni)
            assert np.all((tt == 0) == (ni == 0)) and np.all(tt[ni > 0] >= 1) and np.all(tt <= np.minimum(ni, M))
        want = np.zeros((3, 104), dtype=np.int64)
        np.add.at(want, (cls.astype(np.int64), c1.astype(np.int64)), 1)
        assert np.array_equal(ti.class_counts(), want)
        # the object's log joint is the raw call's on the fetched state, on a table of the grown bounds
        N = max(int(Ni.max()), 3)
        tabs = capi.DeviceTables(N, min(M, N))
        tabs.fill(a)
        tabs.status()
        dev = lambda x, ty, sty: torch.as_tensor(np.ascontiguousarray(x, dtype=ty).view(sty), device="cuda")
        for ind in (False, True):
            tot, Li, info = ti.logjoint(a, bpar, ind)
            tot_r, Li_r, info_r = capi.logjoint(tabs, a, dev(bpar, np.float64, np.float64), dev(koff, np.int64, np.int64),
                                                dev(n1, np.uint32, np.int32), dev(t1, np.uint16, np.int16),
                                                dev(T1, np.uint32, np.int32), dev(h, np.float64, np.float64), ind)
            torch.cuda.synchronize()
            assert tot == tot_r and np.array_equal(Li, Li_r.cpu().numpy())
            assert info.t_mismatch == 0 and info.outside == 0 and info.impossible == 0
    finally:
        ti.free()


# ---- in distribution ----

def test_distribution_from_the_exact_joint():
    # 20000 restaurants of 4 customers, 3 dishes, two classes with a zero entry, started from the joint over (z, t):
    # when the step is right every sweep leaves their law there
    Nc, K, I, sweeps = 4, 3, 20000, 20
    hs, a, b = (0.5, 1.3, 2.0), 0.3, 0.8
    cls1, lik = (0, 1, 0, 1), np.array([[0.9, 0.0, 2.5], [0.2, 1.1, 0.6]])
    st = tdo.states(Nc, K)
    p = tdo.joint(Nc, K, hs, a, b, cls1, lik)
    assert np.max(np.abs(p @ tdo.sweep_matrix(Nc, K, hs, a, b, cls1, lik) - p)) < 1e-12
    rng = np.random.default_rng(81)
    pick = rng.choice(len(st), size=I, p=p)
    z0 = np.array([st[j][0] for j in pick], dtype=np.uint32)
    t0 = np.array([st[j][1] for j in pick], dtype=np.uint16)
    n0 = np.stack([np.bincount(z.astype(np.int64), minlength=K) for z in z0]).astype(np.uint32)
    ti = capi.TableIndicators(np.full(I, K, dtype=np.int32), n0.reshape(-1), t0.reshape(-1), np.tile(hs, I), z0.reshape(-1))
    try:
        ti.set_classes(np.tile(np.array(cls1, dtype=np.uint32), I), 2)
        ti.set_lik(lik)
        info = ti.sweep_dishes(a, np.full(I, b), 82, 0, sweeps)
        assert (info.skipped, info.stuck) == (0, 0)
        n1, t1, T1, c1 = fetch(ti)
    finally:
        ti.free()
    cells, q = tdo.marginal_nt(p, Nc, K)
    idx = {c: j for j, c in enumerate(cells)}
    keys = [(tuple(int(x) for x in nn), tuple(int(x) for x in tt)) for nn, tt in zip(n1.reshape(I, K), t1.reshape(I, K))]
    counts = np.bincount([idx[k] for k in keys], minlength=len(cells)).astype(np.float64)
    pv = chi2_p(counts, q)
    print("p against the joint", pv)
    assert pv > 1e-3
    # the same counts against the law of a chain that ignores u3 (always the first dish): the test can fail
    Pbad = tdo.sweep_matrix(Nc, K, hs, a, b, cls1, lik, first_dish=True)
    _, qbad = tdo.marginal_nt(p @ np.linalg.matrix_power(Pbad, sweeps), Nc, K)
    pbad = chi2_p(counts, qbad)
    print("p against the first-dish law", pbad)
    assert pbad < 1e-9


# ---- queues and mixing ----

def test_queued_sweeps_equal_single_calls():
    rng = np.random.default_rng(91)
    K, n, t, h = random_state(rng, [6] * 50, 30)
    cust = shuffled_order(rng, K, n)
    cls = rng.integers(0, 2, size=len(cust)).astype(np.uint32)
    lik = random_lik(rng, 2, 6)
    a, bpar = 0.4, np.full(50, 3.0)
    q = capi.TableIndicators(K, n, t, h, cust)
    r = capi.TableIndicators(K, n, t, h, cust)
    try:
        for o in (q, r):
            o.set_classes(cls, 2)
            o.set_lik(lik)
        iq = q.sweep_dishes(a, bpar, 92, 4, 3)
        stuck = 0
        for s in (4, 5, 6):
            stuck += r.sweep_dishes(a, bpar, 92, s).stuck
        assert_state(fetch(q), fetch(r))
        assert iq.stuck == stuck
    finally:
        q.free()
        r.free()


def test_dish_sweeps_follow_the_discount():
    # three dish sweeps at a = 0.2, 0.7 and 0.2 again: each reads the V table of its own discount
    rng = np.random.default_rng(93)
    K, n, t, h = random_state(rng, [6] * 50, 30)
    cust = shuffled_order(rng, K, n)
    cls = rng.integers(0, 2, size=len(cust)).astype(np.uint32)
    lik = random_lik(rng, 2, 6)
    bpar = np.full(50, 3.0)
    tabs = {a: grown_vtab(a, max_Ni(K, n)) for a in (0.2, 0.7)}
    ti = capi.TableIndicators(K, n, t, h, cust)
    try:
        ti.set_classes(cls, 2)
        ti.set_lik(lik)
        for s, a in enumerate((0.2, 0.7, 0.2)):
            vt, N, M = tabs[a]
            ti.sweep_dishes(a, bpar, 94, s)
            n, t, T, cust, _, _ = tdo.sweep(K, n, t, h, a, bpar, vt, N, M, 94, s, cust, cls, lik)
            assert_state(fetch(ti), (n, t, T, cust))
    finally:
        ti.free()


def test_dish_and_indicator_sweeps_alternate():
    rng = np.random.default_rng(101)
    K, n, t, h = random_state(rng, [5, 9, 70, 3], 8)
    cust = None  # pair order: the first dish sweep writes the sequence out
    C = int(n.sum())
    cls = rng.integers(0, 2, size=C).astype(np.uint32)
    lik = random_lik(rng, 2, 70)
    a, bpar = 0.35, 1.0 + rng.random(4)
    vt, N, M = grown_vtab(a, max_Ni(K, n))
    ti = capi.TableIndicators(K, n, t, h, cust)
    try:
        ti.set_classes(cls, 2)
        ti.set_lik(lik)
        cust = tio.pair_order(K, n)
        for s in range(3):
            ti.sweep_dishes(a, bpar, 102, s)
            n, t, T, cust, _, _ = tdo.sweep(K, n, t, h, a, bpar, vt, N, M, 102, s, cust, cls, lik)
            ti.sweep(a, bpar, 103, s)
            t, T = tio.sweep(K, n, t, h, a, bpar, vt, N, 103, s, cust)
            assert_state(fetch(ti), (n, t, T, cust))
    finally:
        ti.free()


# ---- stuck and skipped ----

def test_a_class_without_likelihood_stays():
    rng = np.random.default_rng(111)
    K, n, t, h = random_state(rng, [7] * 30, 20)
    cust = shuffled_order(rng, K, n)
    cls = rng.integers(0, 3, size=len(cust)).astype(np.uint32)
    lik = random_lik(rng, 3, 7, zeros=0.0)
    lik[1] = 0.0
    a, bpar = 0.5, np.full(30, 2.0)
    vt, N, M = grown_vtab(a, max_Ni(K, n))
    ti = capi.TableIndicators(K, n, t, h, cust)
    try:
        ti.set_classes(cls, 3)
        ti.set_lik(lik)
        info = ti.sweep_dishes(a, bpar, 112, 0, 2)
        assert info.stuck == 2 * int(np.sum(cls == 1)) and info.skipped == 0
        want = (n, t, None, cust)
        for s in range(2):
            want = tdo.sweep(K, want[0], want[1], h, a, bpar, vt, N, M, 112, s, want[3], cls, lik)
        got = fetch(ti)
        assert_state(got, want[:4])
        assert np.array_equal(got[3][cls == 1], cust[cls == 1]) and not np.array_equal(got[3], cust)
    finally:
        ti.free()
    # every class without likelihood: nothing at all changes
    ti = capi.TableIndicators(K, n, t, h, cust)
    try:
        ti.set_classes(cls, 3)
        ti.set_lik(np.zeros((3, 7)))
        info = ti.sweep_dishes(a, bpar, 112, 0)
        assert info.stuck == len(cust)
        assert_state(fetch(ti), (n, t, ti.get()[1], cust))
        assert np.array_equal(ti.get()[1], [x.sum() for x in np.split(t.astype(np.int64), np.cumsum(K)[:-1])])
    finally:
        ti.free()


def test_raw_restaurants_outside_the_bounds_are_skipped():
    import torch

    a, N, M = 0.5, 40, 40
    v = capi.DeviceVTables(N, M)
    v.fill(a)
    capi.check(capi.lib().stb_fill_status())
    vt = tio.VTab(v.packed_host(0), N, M)
    rng = np.random.default_rng(121)
    # restaurant 0 fits; 1 has 50 customers > N; 2 has 1030 dishes > STB_TD_MAXK
    K = np.array([4, 3, capi.TD_MAXK + 6], dtype=np.int32)
    n = np.concatenate([[10, 0, 25, 5], [20, 20, 10], rng.integers(0, 2, size=capi.TD_MAXK + 6)]).astype(np.uint32)
    n[7] = 1
    t = np.concatenate([[3, 0, 9, 1], [4, 2, 10], (n[7:] > 0)]).astype(np.uint16)
    cust = shuffled_order(rng, K, n)
    Ni = np.array([x.sum() for x in np.split(n.astype(np.int64), np.cumsum(K)[:-1])])
    T0 = np.array([x.sum() for x in np.split(t.astype(np.int64), np.cumsum(K)[:-1])]).astype(np.uint32)
    bpar = np.array([1.0, 2.0, 3.0])
    dev = lambda x, ty, sty: torch.as_tensor(np.ascontiguousarray(x, dtype=ty).view(sty), device="cuda").clone()
    koff = dev(np.concatenate([[0], np.cumsum(K)]), np.int64, np.int64)
    coff = dev(np.concatenate([[0], np.cumsum(Ni)]), np.int64, np.int64)
    d_n, d_t, d_T = dev(n, np.uint32, np.int32), dev(t, np.uint16, np.int16), dev(T0, np.uint32, np.int32)
    d_c, d_b = dev(cust, np.uint32, np.int32), dev(bpar, np.float64, np.float64)
    d_info = torch.zeros(2, dtype=torch.int64, device="cuda")
    L = capi.lib()
    want = (n, t, T0, cust)
    for s in range(2):
        capi.check(L.stb_sample_tdishes(v.tables.data_ptr(), N, M, a, d_b.data_ptr(), 3, koff.data_ptr(), d_n.data_ptr(),
                                        d_t.data_ptr(), d_T.data_ptr(), None, coff.data_ptr(), d_c.data_ptr(), None, None,
                                        0, 0, 122, s, d_info.data_ptr(), capi.stream_ptr()))
        want = tdo.sweep(K, want[0], want[1], None, a, bpar, vt, N, M, 122, s, want[3])
    torch.cuda.synchronize()
    got = (d_n.cpu().numpy().view(np.uint32), d_t.cpu().numpy().view(np.uint16), d_T.cpu().numpy().view(np.uint32),
           d_c.cpu().numpy().view(np.uint32))
    assert d_info.cpu().tolist() == [4, 0]  # two restaurants skipped in each of two sweeps
    assert_state(got, want[:4])
    assert np.array_equal(got[0][4:], n[4:]) and np.array_equal(got[1][4:], t[4:]) and np.array_equal(got[3][40:], cust[40:])
    assert not np.array_equal(got[3][:40], cust[:40])
    # refused before anything is queued
    with pytest.raises(capi.StbError, match="d_cust"):
        capi.check(L.stb_sample_tdishes(v.tables.data_ptr(), N, M, a, d_b.data_ptr(), 3, koff.data_ptr(), d_n.data_ptr(),
                                        d_t.data_ptr(), d_T.data_ptr(), None, coff.data_ptr(), None, None, None, 0, 0, 1, 0,
                                        None, capi.stream_ptr()))
    with pytest.raises(capi.StbError, match="likelihood"):
        capi.check(L.stb_sample_tdishes(v.tables.data_ptr(), N, M, a, d_b.data_ptr(), 3, koff.data_ptr(), d_n.data_ptr(),
                                        d_t.data_ptr(), d_T.data_ptr(), None, coff.data_ptr(), d_c.data_ptr(), None,
                                        d_b.data_ptr(), 1, 0, 1, 0, None, capi.stream_ptr()))


def test_too_many_dishes_are_refused_on_the_object():
    K = np.array([2, capi.TD_MAXK + 1], dtype=np.int32)
    n = np.zeros(capi.TD_MAXK + 3, dtype=np.uint32)
    n[:4] = [3, 2, 1, 4]
    t = (n > 0).astype(np.uint16)
    ti = capi.TableIndicators(K, n, t)
    try:
        with pytest.raises(capi.StbError, match="STB_TD_MAXK"):
            ti.sweep_dishes(0.5, np.full(2, 1.0), 1, 0)
        assert np.array_equal(ti.get()[0], t) and np.array_equal(ti.get_state()[0], n)
        ti.sweep(0.5, np.full(2, 1.0), 1, 0)  # the indicator sweep has no such bound
    finally:
        ti.free()


# ---- table growth, hand-over, refusals ----

def test_the_first_dish_sweep_grows_the_table():
    rng = np.random.default_rng(131)
    K = np.array([10, 10], dtype=np.int32)
    n = np.array([5, 4, 4, 4, 4, 4, 4, 4, 4, 3] * 2, dtype=np.uint32)  # max n = 5, N_i = 40
    t = np.where(n > 0, 1 + np.floor(rng.random(20) * n), 0).astype(np.uint16)
    h = 0.2 + rng.random(20)
    cust = shuffled_order(rng, K, n)
    a, bpar = 0.55, np.array([0.5, 8.0])
    lik = np.tile(np.array([1.0, 1.0, 0.2, 0.1, 0.1, 0.1, 0.05, 0.05, 0.02, 0.02]), (1, 1))  # customers pile up in a few dishes
    vt, N, M = grown_vtab(a, 40)
    assert (N, M) == (40, 40)
    ti = capi.TableIndicators(K, n, t, h, cust)
    try:
        ti.sweep(a, bpar, 132, 0)  # on the table as created (5 x 5)
        v5, N5, _ = grown_vtab(a, 5)
        t, T = tio.sweep(K, n, t, h, a, bpar, v5, N5, 132, 0, cust)
        assert np.array_equal(ti.get()[0], t)
        ti.logjoint(a, bpar)  # (an S slab at the old bounds, to be replaced)
        ti.set_classes(np.zeros(80, dtype=np.uint32), 1)
        ti.set_lik(lik)
        for s in range(3):
            ti.sweep_dishes(a, bpar, 133, s)
            n, t, T, cust, _, _ = tdo.sweep(K, n, t, h, a, bpar, vt, N, M, 133, s, cust, np.zeros(80, dtype=np.int64), lik)
        assert_state(fetch(ti), (n, t, T, cust))
        assert n.max() > 5
        ti.sweep(a, bpar, 134, 0)
        t, T = tio.sweep(K, n, t, h, a, bpar, vt, N, 134, 0, cust)
        assert_state(fetch(ti), (n, t, T, cust))
        tot, Li, info = ti.logjoint(a, bpar)
        assert info.outside == 0 and info.impossible == 0 and info.t_mismatch == 0
        S = {m: tio.stirling(m, a) for m in range(1, 41)}
        for i in range(2):
            ni, tt, hh = n[10 * i:10 * i + 10], t[10 * i:10 * i + 10], h[10 * i:10 * i + 10]
            want = sum(math.log(S[int(x)][int(y)]) + int(y) * math.log(z) for x, y, z in zip(ni, tt, hh) if x)
            want += sum(math.log(bpar[i] + j * a) for j in range(int(T[i]))) - sum(math.log(bpar[i] + j) for j in range(40))
            assert abs(Li[i] - want) < 1e-9 * max(1.0, abs(want)), (i, Li[i], want)
    finally:
        ti.free()


def make_set(K, n, t, T, bpar, N, M, D):
    L = capi.lib()
    g = L.stb_groups_create(len(K), orc.i32p(K), orc.u32p(T), orc.u32p(n), orc.u16p(t), orc.dp(bpar), N, M, D)
    assert g, capi.last_error()
    return g


def test_hand_over_to_a_group_set():
    L = capi.lib()
    g = synth.groups(60, 8, 30, "realistic", seed=141)
    rng = np.random.default_rng(142)
    cust = shuffled_order(rng, g.K, g.n)
    x = synth.discount_grid(8)
    N0 = int(g.n.max())
    ti = capi.TableIndicators(g.K, g.n, g.t, None, cust)
    A = make_set(g.K, g.n, g.t, g.T, g.bpar, N0, N0, 8)  # bounds of the state as created: the hand-over grows them
    try:
        ti.sweep_dishes(0.45, g.bpar, 143, 0, 3)
        ti.to_groups(A, g.bpar)
        n, t, T, _ = fetch(ti)
        assert not np.array_equal(n, g.n)
        Nb = int(g.N.max())
        B = make_set(g.K, n, t, T, g.bpar, Nb, Nb, 8)
        outA, outB = np.zeros(8), np.zeros(8)
        capi.check(L.stb_groups_aterms(A, capi.dp(x), 8, capi.dp(outA)))
        capi.check(L.stb_groups_aterms(B, capi.dp(x), 8, capi.dp(outB)))
        L.stb_groups_free(B)
        assert np.allclose(outA, outB, rtol=1e-12, atol=0.0), (outA, outB)
    finally:
        ti.free()
        L.stb_groups_free(A)


def test_refusals_leave_the_state():
    rng = np.random.default_rng(151)
    K, n, t, h = random_state(rng, [5] * 6, 15)
    cust = shuffled_order(rng, K, n)
    C = len(cust)
    cls = rng.integers(0, 2, size=C).astype(np.uint32)
    lik = random_lik(rng, 2, 5)
    bpar = np.full(6, 1.5)
    ti = capi.TableIndicators(K, n, t, h, cust)
    ref = capi.TableIndicators(K, n, t, h, cust)
    odd = capi.TableIndicators(K, n, t, h, cust, 0, capi.TI_REF_ODDS)
    try:
        for o in (ti, ref):
            o.set_classes(cls, 2)
            o.set_lik(lik)
        bad = cls.copy()
        bad[3] = 2
        with pytest.raises(capi.StbError, match="cls\\[3\\]"):
            ti.set_classes(bad, 2)
        for x in (-1.0, np.nan, np.inf):
            badl = lik.copy()
            badl[1, 2] = x
            with pytest.raises(capi.StbError, match="lik\\[7\\]"):
                ti.set_lik(badl)
        with pytest.raises(capi.StbError, match="stride"):
            ti.set_lik(lik[:, :4])
        with pytest.raises(capi.StbError, match="STB_TI_REF_ODDS"):
            odd.sweep_dishes(0.5, bpar, 1, 0)
        for a, b, match in ((1.0, 1.0, "outside"), (-0.1, 1.0, "outside"), (0.5, -0.5, "bpar"), (0.0, 0.0, "bpar"),
                            (0.3, np.nan, "bpar")):
            with pytest.raises(capi.StbError, match=match):
                ti.sweep_dishes(a, np.full(6, b), 1, 0)
        T0 = np.array([x.sum() for x in np.split(t.astype(np.int64), np.cumsum(K)[:-1])])
        for o in (ti, odd):
            assert_state(fetch(o), (n, t, T0, cust))
        # classes set for more rows than the matrix has
        ti.set_classes(np.full(C, 2, dtype=np.uint32), 3)
        with pytest.raises(capi.StbError, match="rows"):
            ti.sweep_dishes(0.5, bpar, 1, 0)
        ti.set_classes(cls, 2)
        # nothing above changed what a sweep does
        ti.sweep_dishes(0.5, bpar, 1, 0)
        ref.sweep_dishes(0.5, bpar, 1, 0)
        assert_state(fetch(ti), fetch(ref))
    finally:
        ti.free()
        ref.free()
        odd.free()
