"""The table-size partition draw's oracle (tests/pt_oracle.py) against the law it is meant to sample, enumerated from
the definition: the exact draw has it, the reference's walk (lib/samplea.c:295-320, the drop-in samplea2's) does not.
And the C entry points without a GPU."""
import ctypes as C

import numpy as np
import pytest

import orc
import pt_oracle as pto
from libstb_amd import capi, synth

PAIRS = [(5, 2), (6, 3), (8, 3), (9, 4), (10, 5), (12, 4), (14, 7), (16, 3), (16, 12)]
AS = [0.0, 0.2, 0.5, 0.9]

# (n, t, a) -> total variation of the reference walk's law from the truth (deviation 12)
REF_ROWS = [((8, 3, 0.5), 0.57), ((12, 4, 0.2), 0.88), ((10, 5, 0.8), 0.54)]


def law_diff(p, q):
    return max(abs(p.get(k, 0.0) - q.get(k, 0.0)) for k in set(p) | set(q))


@pytest.mark.parametrize("a", AS)
def test_the_recursion_is_the_definition(a):
    for n, t in PAIRS:
        T = pto.truth(n, t, a)
        assert abs(sum(T.values()) - 1.0) < 1e-14
        assert law_diff(pto.recursion_law(n, t, a), T) <= 1e-13, (n, t, a)


@pytest.mark.parametrize("a", AS)
def test_the_replay_draws_the_definition(a):
    """the kernel's arithmetic on a table of logs, integrated exactly over u"""
    S1, tab = orc.fill_S(a, 16, 16)
    for n, t in PAIRS:
        assert law_diff(pto.replay_law(n, t, a, S1, tab, 16), pto.truth(n, t, a)) <= 1e-13, (n, t, a)


@pytest.mark.parametrize("row", REF_ROWS)
def test_the_reference_walk_does_not(row):
    (n, t, a), want = row
    S1, tab = orc.fill_S(a, n, n)
    d = pto.tv(pto.ref_walk_law(n, t, a, S1, tab, n), pto.truth(n, t, a))
    assert abs(d - want) < 0.01, d
    # its singletons: t-1 tables of one customer almost always
    law = pto.ref_walk_law(n, t, a, S1, tab, n, K=2000)
    assert law.get((n - t + 1,) + (1,) * (t - 1), 0.0) > 0.9


def _drand48(count):
    libc = C.CDLL(None)
    libc.drand48.restype = C.c_double
    orc.seed_libc(777, 12345)
    return np.array([libc.drand48() for _ in range(count)])


def test_the_restated_walk_is_the_oracles():
    """pto.ref_walk against orc_partition on samplea2's golden set and uniforms (the first pairs that draw)"""
    L = orc.oracle()
    g = synth.groups(20, 30, 300, "realistic")
    a0 = 0.3
    N = int(g.n.max())
    M = max(int(g.t.max()), 10)
    S1, tab = orc.fill_S(a0, N, M)
    draws = (g.t > 1) & (g.t < g.n)
    u = _drand48(int(draws.sum()))
    m = np.zeros(int((g.t[draws].astype(np.int64) - 1).sum()) + 1, dtype=np.uint16)
    cnt = L.orc_partition(a0, orc.dp(tab), orc.dp(S1), N, M, g.I, orc.i32p(g.K), orc.u32p(g.n), orc.u16p(g.t), orc.dp(u),
                          orc.u16p(m))
    assert cnt == m.shape[0] - 1
    D = pto.dense(S1, tab, N, M)
    off = k = 0
    for g_ in np.flatnonzero(draws)[:60]:
        n, t = int(g.n[g_]), int(g.t[g_])
        sz = pto.ref_walk(n, t, a0, float(u[k]), D)
        # the reference lays the drawn sizes out as m[M-1] for M = t-1 .. 1, the remainder implied
        assert list(m[off:off + t - 1]) == sz[:t - 1][::-1], g_
        assert sum(sz) == n
        off += t - 1
        k += 1
    assert k == 60


def test_bookkeeping():
    """the replay's histogram is its sizes binned; cnt[0] counts the pairs left out, cnt[1] the singletons; every pair
    that draws has t sizes summing to n"""
    a, N, M, S = 0.4, 40, 12, 45
    S1, tab = orc.fill_S(a, N, M)
    n = np.array([0, 5, 7, 1, 9, 30, 41, 44, 20, 3, 6, 13, 40, 50], dtype=np.uint32)
    t = np.array([0, 5, 1, 1, 0, 13, 2, 1, 21, 2, 4, 12, 12, 1], dtype=np.uint16)
    cnt, sizes, ties = pto.replay(n, t, a, S1, tab, N, M, S, 7, 3)
    assert ties == 0
    # left out: t = 0 (n = 9), t > M (30, 13), n > N (41, 2), t > n (20, 21), n >= S (50, 1)
    assert cnt[0] == 5
    assert [sizes[g] is None for g in range(len(n))] == [False, False, False, False, True, True, True, False, True, False,
                                                         False, False, False, True]
    assert sizes[0] == [] and sizes[1] == [1] * 5 and sizes[2] == [7] and sizes[3] == [1] and sizes[7] == [44]
    for g in (9, 10, 11, 12):
        assert len(sizes[g]) == t[g] and sum(sizes[g]) == n[g] and min(sizes[g]) >= 1
    # t = n (pairs 1 and 3) counts nothing; everything else is binned
    counted = [sizes[g] for g in range(len(n)) if g not in (1, 3)]
    assert np.array_equal(cnt, pto.bin_sizes(counted, S, left_out=5))
    assert cnt[1] == sum(s == 1 for sz in counted for s in (sz or [])) >= 1
    # the draws depend on the sweep
    cnt2, sizes2, _ = pto.replay(n, t, a, S1, tab, N, M, S, 7, 4)
    assert any(sizes2[g] != sizes[g] for g in (10, 11, 12))


def test_uniform_index():
    """round r of pair g reads element g 65536 + r + 1 of the sweep's stream (synth.unit's element)"""
    import tc_oracle as tco

    key = tco.sweep_key(5, 2)
    u = synth.unit(70000, key)
    assert pto.round_u(key, 0, 0) == u[0]
    assert pto.round_u(key, 1, 3) == u[65536 + 3]


def test_entry_points_without_a_gpu():
    L = capi.lib()
    for name in ("stb_sample_partition", "stb_tcounts_partition", "stb_hist_create_empty", "stb_hist_restaurants",
                 "stb_hist_counts_device", "stb_hist_get", "stb_samplea2_hist"):
        assert hasattr(L, name), name
    # the raw call refuses bad arguments before it reaches a device
    vp = C.c_void_p(1)
    rc = L.stb_sample_partition(None, None, 10, 10, 1.5, 0, None, None, vp, 11, None, None, 0, 1, 0, None)
    assert rc != 0 and "discount" in capi.last_error()
    rc = L.stb_sample_partition(None, None, 10, 10, 0.5, 0, None, None, vp, 11, None, None, 4, 1, 0, None)
    assert rc != 0 and "flags" in capi.last_error()
    rc = L.stb_sample_partition(None, None, 10, 10, 0.5, 0, None, None, vp, 1, None, None, 0, 1, 0, None)
    assert rc != 0 and "S=1" in capi.last_error()
    rc = L.stb_sample_partition(None, None, 10, 10, 0.5, 0, None, None, vp, 11, vp, None, 0, 1, 0, None)
    assert rc != 0 and "together" in capi.last_error()
