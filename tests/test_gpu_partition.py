"""The table-size partition draw on the device (stb_sample_partition / stb_tcounts_partition): draw for draw against the
numpy replay (tests/pt_oracle.py), the reference walk against the oracle's orc_partition, in law against the truth
enumerated from the definition and against an unbiasedness identity at working sizes, handed over from a table-count
object into a device histogram, and as half of an S-free discount chain."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import orc
import pt_oracle as pto
import tc_oracle as tco
from libstb_amd import capi, synth

pytestmark = pytest.mark.gpu


def torch():
    import torch as _t

    return _t


def device_table(a, N, M):
    tabs = capi.DeviceTables(N, M)
    tabs.fill(a)
    tabs.status()
    return tabs, tabs.S1[0].cpu().numpy(), tabs.packed_host(0)


def run_device(tabs, a, n, t, S, seed, sweep, ref=False, sizes=True):
    """(cnt, per-pair sizes in draw order (None where nothing was written)) of one raw call"""
    T = torch()
    n = np.ascontiguousarray(n, dtype=np.uint32)
    t = np.ascontiguousarray(t, dtype=np.uint16)
    d_n = T.as_tensor(n.view(np.int32), device="cuda")
    d_t = T.as_tensor(t.view(np.int16), device="cuda")
    soff = np.concatenate([[0], np.cumsum(t.astype(np.int64))]).astype(np.int64)
    d_soff = T.as_tensor(soff, device="cuda") if sizes else None
    d_sz = T.full((max(1, int(soff[-1])),), -1, dtype=T.int16, device="cuda") if sizes else None
    cnt = capi.sample_partition(tabs, a, d_n, d_t, S, seed, sweep, sizes=d_sz, soff=d_soff, ref=ref)
    T.cuda.synchronize()
    cnt = cnt.cpu().numpy().view(np.uint32).astype(np.int64)
    if not sizes:
        return cnt, None
    sz = d_sz.cpu().numpy().view(np.uint16)
    out = []
    for g in range(len(n)):
        v = sz[soff[g]:soff[g + 1]]
        out.append(None if len(v) and v[0] == 0xFFFF else [int(x) for x in v])
    return cnt, out


def special_pairs(N, M):
    """t = 1, t = n, n = 0, n > N, t > M, t = 0, t > n, and short pairs"""
    n = [5, 7, 0, N + 3, min(N, M + 5), 9, 4, 3, 2, 1, N, N]
    t = [1, 7, 0, 2, M + 1, 0, 6, 2, 1, 1, 2, min(N - 1, M)]
    return np.array(n, dtype=np.uint32), np.array(t, dtype=np.uint16)


def set_pairs(I, K, nmax, prof, N, M, seed=3):
    g = synth.groups(I, K, nmax, prof, seed=seed)
    t = np.minimum(g.t, M).astype(np.uint16)
    sn, st = special_pairs(N, M)
    return np.concatenate([g.n, sn]), np.concatenate([t, st])


def check_exact(a, n, t, N, M, S, seed, sweep):
    tabs, S1, tab = device_table(a, N, M)
    cnt, sizes = run_device(tabs, a, n, t, S, seed, sweep)
    want, wsz, ties = pto.replay(n, t, a, S1, tab, N, M, S, seed, sweep)
    assert ties == 0, "pick a seed without near-ties"
    for g in range(len(n)):
        if wsz[g] is None:
            assert sizes[g] is None or len(sizes[g]) == 0, g
        else:
            assert sizes[g] == wsz[g], (g, int(n[g]), int(t[g]), sizes[g], wsz[g])
    assert np.array_equal(cnt, want), np.flatnonzero(cnt != want)[:10]
    return cnt, sizes


@pytest.mark.parametrize("a", [0.0, 0.3, 0.75, 0.999])
def test_exact_agreement_realistic(a):
    N = M = 400
    n, t = set_pairs(30, 40, 400, "realistic", N, M)
    check_exact(a, n, t, N, M, N + 1, 21, 2)


@pytest.mark.parametrize("a", [0.0, 0.5, 0.999])
def test_exact_agreement_wide(a):
    N = M = 160
    n, t = set_pairs(8, 25, 160, "wide", N, M)
    check_exact(a, n, t, N, M, N + 1, 22, 5)


def test_exact_agreement_truncated_and_small_histogram():
    """M below the largest n (pairs with t > M left out), N below some n, and S with sizes past the LDS copy"""
    N, M = 1500, 30
    n, t = set_pairs(6, 30, 1600, "realistic", N, M, seed=9)
    cnt, _ = check_exact(0.4, n, t, N, M, 1550, 23, 1)
    assert cnt[0] > 0 and cnt[1024:].sum() > 0


def test_reference_walk_is_the_oracles():
    """STB_PT_REF_WALK against orc_partition with the same per-pair uniforms (r = 0's)"""
    a, N, M = 0.35, 300, 40
    g = synth.groups(20, 30, 300, "realistic", seed=4)
    n, t = g.n, np.minimum(g.t, M).astype(np.uint16)
    tabs, S1, tab = device_table(a, N, M)
    cnt, sizes = run_device(tabs, a, n, t, N + 1, 31, 7, ref=True)
    key = tco.sweep_key(31, 7)
    draws = np.flatnonzero((t > 1) & (t < n))
    u = np.array([pto.round_u(key, int(g_), 0) for g_ in draws])
    m = np.zeros(int((t[draws].astype(np.int64) - 1).sum()) + 1, dtype=np.uint16)
    L = orc.oracle()
    K = np.full(20, 30, dtype=np.int32)
    got = L.orc_partition(a, orc.dp(tab), orc.dp(np.ascontiguousarray(S1)), N, M, 20, orc.i32p(K), orc.u32p(n),
                          orc.u16p(t), orc.dp(u), orc.u16p(m))
    assert got == m.shape[0] - 1
    off = 0
    for g_ in draws:
        k = int(t[g_]) - 1
        assert sizes[g_][:k] == [int(x) for x in m[off:off + k][::-1]], g_
        assert sum(sizes[g_]) == n[g_]
        off += k


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


@pytest.mark.parametrize("n,t,a", [(8, 3, 0.5), (12, 4, 0.2), (10, 5, 0.8), (16, 6, 0.0), (14, 3, 0.999)])
def test_law_against_the_truth(n, t, a):
    copies = 100000
    tabs, _, _ = device_table(a, n, n)
    cnt, sizes = run_device(tabs, a, np.full(copies, n), np.full(copies, t), n + 1, 41, 0)
    truth = pto.truth(n, t, a)
    keys = sorted(truth)
    idx = {k: j for j, k in enumerate(keys)}
    obs = np.zeros(len(keys))
    for sz in sizes:
        obs[idx[tuple(sorted(sz, reverse=True))]] += 1
    p = np.array([truth[k] for k in keys])
    assert chi2_p(obs, p) > 1e-4
    assert cnt[2:].sum() + cnt[1] == copies * t


def log_rising(x, k):
    return math.lgamma(x + k) - math.lgamma(x)


def ratio_stat(sizes, a, ap):
    """X = prod_j (1-a')_{s_j-1} / (1-a)_{s_j-1} for every drawn partition"""
    out = np.empty(len(sizes))
    for i, sz in enumerate(sizes):
        out[i] = math.exp(sum(log_rising(1 - ap, s - 1) - log_rising(1 - a, s - 1) for s in sz))
    return out


@pytest.mark.parametrize("n,t,copies", [(100, 10, 20000), (300, 20, 20000), (4000, 60, 4000)])
def test_unbiased_at_working_sizes(n, t, copies):
    """E_a[prod (1-a')_{s-1} / (1-a)_{s-1}] = S^n_t(a') / S^n_t(a): exact draws meet it, the reference walk does not"""
    a = 0.5
    tabs, S1, tab = device_table(a, n, t)
    _, sizes = run_device(tabs, a, np.full(copies, n), np.full(copies, t), n + 1, 51, 3)
    for ap in (0.47, 0.53):
        S1p, tabp = orc.fill_S(ap, n, t)
        want = math.exp(pto.S_at(S1p, tabp, t, n, t) - pto.S_at(S1, tab, t, n, t))
        X = ratio_stat(sizes, a, ap)
        se = X.std(ddof=1) / math.sqrt(len(X))
        assert abs(X.mean() - want) <= 5 * se + 1e-12 * want, (ap, X.mean(), want, se)
    if n <= 300:
        _, rs = run_device(tabs, a, np.full(2000, n), np.full(2000, t), n + 1, 51, 3, ref=True)
        S1p, tabp = orc.fill_S(0.47, n, t)
        want = math.exp(pto.S_at(S1p, tabp, t, n, t) - pto.S_at(S1, tab, t, n, t))
        X = ratio_stat(rs, a, 0.47)
        se = max(X.std(ddof=1) / math.sqrt(len(X)), 1e-3 * want)
        assert abs(X.mean() - want) > 10 * se, (X.mean(), want, se)


def test_determinism_across_geometry():
    a, N, M = 0.6, 500, 500
    n, t = set_pairs(20, 50, 500, "realistic", N, M, seed=12)
    tabs, _, _ = device_table(a, N, M)
    old = os.environ.get("STB_PARTITION_WAVES")
    try:
        res = []
        for w in ("1", "2", "8"):
            os.environ["STB_PARTITION_WAVES"] = w
            res.append(run_device(tabs, a, n, t, N + 1, 61, 9))
    finally:
        if old is None:
            os.environ.pop("STB_PARTITION_WAVES", None)
        else:
            os.environ["STB_PARTITION_WAVES"] = old
    for c, s in res[1:]:
        assert np.array_equal(c, res[0][0]) and s == res[0][1]
    c2, s2 = run_device(tabs, a, n, t, N + 1, 61, 10)
    assert s2 != res[0][1]
    # the histogram alone is the same histogram
    c3, _ = run_device(tabs, a, n, t, N + 1, 61, 9, sizes=False)
    assert np.array_equal(c3, res[0][0])


def test_hand_over_from_table_counts():
    a, b = 0.45, 3.0
    g = synth.groups(12, 20, 200, "realistic", seed=5)
    N = M = max(int(g.n.max()), 3)
    tc = capi.TableCounts(g.K, g.n, g.t)
    h = capi.Histogram(N + 1, g.I)
    try:
        tc.sweep(a, np.full(g.I, b), 71, 0, nsweeps=3)
        tc.partition(a, h, np.full(g.I, b), 72, 4)
        got = h.counts().astype(np.int64)
        t_now, T_now = tc.get()
        tabs, S1, tab = device_table(a, N, M)
        raw, _ = run_device(tabs, a, g.n, t_now, N + 1, 72, 4)
        assert np.array_equal(got, raw)
        want, _, ties = pto.replay(g.n, t_now, a, S1, tab, N, M, N + 1, 72, 4)
        assert ties == 0 and np.array_equal(got, want)
        # aterms2 on the device-built histogram = stb_hist_create on the replay's counts, bit for bit
        host = capi.Histogram(N + 1, g.I, cnt=want.astype(np.uint32), T=T_now, bpar=np.full(g.I, b))
        xs = np.array([0.1, 0.3, 0.45, 0.6, 0.9])
        assert np.array_equal(h.aterms2(xs), host.aterms2(xs))
        host.free()
        # rejected inputs leave the state as it was
        small = capi.Histogram(int(g.n.max()), g.I)
        other = capi.Histogram(N + 1, g.I + 1)
        for bad in (lambda: tc.partition(1.0, h, np.full(g.I, b), 1, 1),
                    lambda: tc.partition(a, h, np.full(g.I, -a - 1), 1, 1),
                    lambda: tc.partition(a, small, np.full(g.I, b), 1, 1),
                    lambda: tc.partition(a, other, np.full(g.I, b), 1, 1)):
            with pytest.raises(capi.StbError):
                bad()
        assert np.array_equal(h.counts().astype(np.int64), got)
        t2, T2 = tc.get()
        assert np.array_equal(t2, t_now) and np.array_equal(T2, T_now)
        small.free()
        other.free()
    finally:
        h.free()
        tc.free()


def test_empty_histogram_and_restaurants():
    h = capi.Histogram(50, 3)
    try:
        assert not h.counts().any()
        cnt = np.zeros(50, dtype=np.uint32)
        cnt[[2, 5, 7]] = [3, 1, 2]
        p, _ = h.device_counts()
        torch().cuda.synchronize()
        capi.check(capi.lib().stb_memcpy_h2d(C.c_void_p(p), cnt.ctypes.data_as(C.c_void_p), 200, None))
        capi.check(capi.lib().stb_stream_sync(None))
        T, b = np.array([4, 6, 3], dtype=np.uint32), np.array([1.0, 2.0, 0.5])
        h.restaurants(T, b)
        host = capi.Histogram(50, 3, cnt=cnt, T=T, bpar=b)
        xs = np.array([0.2, 0.7])
        assert np.array_equal(h.counts(), cnt) and np.array_equal(h.aterms2(xs), host.aterms2(xs))
        host.free()
    finally:
        h.free()


def ks_stat(x, cdf_grid, grid):
    x = np.sort(x)
    F = np.interp(x, grid, cdf_grid)
    n = len(x)
    return max(np.max(np.arange(1, n + 1) / n - F), np.max(F - np.arange(n) / n))


def test_discount_chain_end_to_end():
    """partition | a (device) and a | partition (stb_samplea2_hist) alternated: the a-marginal is the collapsed posterior
    exp(aterms(a)) of stb_groups_aterms, judged by a KS test on the thinned chain"""
    L = capi.lib()
    g = synth.groups(6, 40, 60, "realistic", seed=8, bpar=2.0)
    N = M = int(g.n.max())
    tc = capi.TableCounts(g.K, g.n, g.t)
    h = capi.Histogram(N + 1, g.I)
    old = os.environ.get("STB_SAMPLER")
    os.environ["STB_SAMPLER"] = "slice"
    try:
        orc.seed_libc(777, 4242)
        a, chain = 0.5, []
        for k in range(3000):
            tc.partition(a, h, g.bpar, 81, k)
            a = L.stb_samplea2_hist(a, h.h, None, 1, 0)
            chain.append(a)
    finally:
        if old is None:
            os.environ.pop("STB_SAMPLER", None)
        else:
            os.environ["STB_SAMPLER"] = old
        h.free()
        tc.free()
    grid = np.linspace(0.01, 0.98, 389)
    hg = L.stb_groups_create(g.I, orc.i32p(g.K), orc.u32p(g.T), orc.u32p(g.n), orc.u16p(g.t), orc.dp(g.bpar), N, M, 1)
    lp = np.zeros(len(grid))
    out = np.zeros(1)
    for j, x in enumerate(grid):
        capi.check(L.stb_groups_aterms(hg, capi.dp(np.array([x])), 1, capi.dp(out)))
        lp[j] = out[0]
    L.stb_groups_free(hg)
    p = np.exp(lp - lp.max())
    cdf = np.concatenate([[0.0], np.cumsum((p[1:] + p[:-1]) / 2 * np.diff(grid))])
    cdf /= cdf[-1]
    x = np.array(chain[200::10])
    D = ks_stat(x, cdf, grid)
    assert D < 1.63 / math.sqrt(len(x)) * 1.5, D  # (a loose bar: the thinned chain is still correlated)
