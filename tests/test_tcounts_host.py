"""The table-count sweep's oracle (tests/tc_oracle.py) against brute-force enumeration of the PYP joint, and the C entry
points of stb_tcounts_* / stb_sample_tcounts without a GPU."""
import itertools

import numpy as np
import pytest

import orc
import tc_oracle as tco
from libstb_amd import capi, synth


def enum_conditionals(ns, hs, a, b, S1, tab, M):
    """for every t vector of a restaurant and every pair k: the conditional p(t_k | t_-k) from the joint"""
    ranges = [range(1, n + 1) for n in ns]
    lj = {ts: tco.log_joint(ns, ts, a, b, hs, S1, tab, M) for ts in itertools.product(*ranges)}
    for ts in lj:
        for k in range(len(ns)):
            vals = np.array([lj[ts[:k] + (tau,) + ts[k + 1:]] for tau in ranges[k]])
            p = np.exp(vals - vals.max())
            yield ts, k, p / p.sum()


@pytest.mark.parametrize("a", [0.0, 0.4, 0.8])
@pytest.mark.parametrize("ns,hs,b", [((5, 3), (1.0, 1.0), 1.5), ((8, 2, 4), (0.3, 1.0, 0.7), 0.2), ((7, 6), (0.05, 2.0), 12.0)])
def test_conditional_is_the_joints(a, ns, hs, b):
    S1, tab = orc.fill_S(a, 8, 8)
    worst = 0.0
    for ts, k, p in enum_conditionals(ns, hs, a, b, S1, tab, 8):
        Tm = sum(ts) - ts[k]
        lw = tco.log_weights(ns[k], Tm, a, b, hs[k], 8, S1, tab, 8)
        q = np.exp(lw - lw.max())
        worst = max(worst, float(np.max(np.abs(q / q.sum() - p))))
    assert worst < 1e-12, worst


def test_truncated_conditional():
    # M < n: the conditional restricted to tau <= M, renormalised
    a, b = 0.6, 2.0
    S1, tab = orc.fill_S(a, 8, 8)
    full = tco.log_weights(8, 3, a, b, 0.5, 8, S1, tab, 8)
    S1m, tabm = orc.fill_S(a, 8, 5)
    trunc = tco.log_weights(8, 3, a, b, 0.5, 5, S1m, tabm, 5)
    assert trunc.shape == (5,)
    p, q = np.exp(full[:5] - full[:5].max()), np.exp(trunc - trunc.max())
    assert np.max(np.abs(p / p.sum() - q / q.sum())) < 1e-12


def test_uniforms_are_splitmix():
    seed, s = 0x1234, 5
    key = tco.sweep_key(seed, s)
    gamma, mask = 0x9E3779B97F4A7C15, (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        return z ^ (z >> 31)

    assert key == mix((seed + (s + 1) * gamma) & mask)
    u = tco.uniforms(seed, s, 10)
    for g in range(10):
        assert u[g] == (mix((key + (g + 1) * gamma) & mask) >> 11) / 2.0**53


def test_oracle_sweep_edge_cases():
    a, M = 0.5, 12
    S1, tab = orc.fill_S(a, 12, M)
    K = np.array([4, 3], dtype=np.int32)
    n = np.array([0, 1, 12, 5, 9, 0, 1], dtype=np.uint32)
    t = np.array([0, 1, 3, 2, 9, 0, 1], dtype=np.uint16)
    for s in range(5):
        t, T, _ = tco.sweep(K, n, t, None, a, [1.0, 3.0], M, S1, tab, M, 99, s)
        assert t[0] == 0 and t[5] == 0 and t[1] == 1 and t[6] == 1
        assert np.all((t[n > 0] >= 1) & (t[n > 0] <= n[n > 0]))
        assert T.tolist() == [int(t[:4].sum()), int(t[4:].sum())]


def test_entry_points_exist():
    L = capi.lib()
    for name in ("stb_sample_tcounts", "stb_tcounts_create", "stb_tcounts_set_h", "stb_tcounts_sweep", "stb_tcounts_get",
                 "stb_tcounts_to_groups", "stb_tcounts_free"):
        assert hasattr(L, name), name


def test_create_without_or_with_a_device():
    L = capi.lib()
    g = synth.groups(4, 3, 50, "realistic")
    if L.stb_device_count() == 0:
        with pytest.raises(capi.StbError, match="no HIP device"):
            capi.TableCounts(g.K, g.n, g.t)
        assert L.stb_sample_tcounts(None, None, 10, 10, 0.5, None, 0, None, None, None, None, None, 1, 0, None) == 0
    else:
        tc = capi.TableCounts(g.K, g.n, g.t)
        t, T = tc.get()
        assert np.array_equal(t, g.t) and np.array_equal(T, g.T)
        tc.free()
    # invalid discounts are refused before any device is touched
    assert L.stb_sample_tcounts(None, None, 10, 10, 1.0, None, 1, None, None, None, None, None, 1, 0, None) != 0
    assert "outside [0, 1)" in capi.last_error()
