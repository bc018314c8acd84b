"""The windowed table-count sweep's oracle (tests/tcw_oracle.py) against the PYP joint, exactly: the corrected chain
leaves it invariant, the reference's (test/check.c's SampleCTW) does not.  And the C entry points without a GPU."""
import numpy as np
import pytest

import orc
import tc_oracle as tco
import tcw_oracle as tcw
from libstb_amd import capi

# (n, a, b, h, W) -> the reference chain's max |pi_CTW - pi| (deviation 11)
REF_ROWS = [((10, 0.5, 1.0, 1.0, 1), 0.054), ((12, 0.0, 1.0, 1.0, 2), 0.042), ((9, 0.9, 0.5, 2.0, 1), 0.035),
            ((20, 0.5, 10.0, 1 / 50, 1), 0.037), ((40, 0.5, 10.0, 1.0, 3), 0.033), ((60, 0.3, 1.0, 1.0, 10), 0.005)]


def tables(a, N):
    return orc.fill_S(a, N, N)


@pytest.mark.parametrize("row", [r for r, _ in REF_ROWS] + [(30, 0.5, 10.0, 1 / 50, 10), (7, 0.8, 3.0, 0.3, 2)])
def test_exact_mode_is_invariant_one_pair(row):
    n, a, b, h, W = row
    S1, tab = tables(a, n)
    pi = tcw.joint((n,), (h,), a, b, S1, tab, n)
    P = tcw.sweep_matrix((n,), (h,), a, b, W, S1, tab, n)
    assert np.allclose(P.sum(axis=1), 1.0, atol=1e-13) and P.min() >= 0.0
    assert np.max(np.abs(pi @ P - pi)) <= 1e-12


@pytest.mark.parametrize("a", [0.0, 0.45, 0.8])
@pytest.mark.parametrize("ns,hs,b,W", [((6, 4), (1.0, 0.5), 1.5, 1), ((8, 3, 5), (0.3, 1.0, 2.0), 0.4, 2),
                                       ((9, 7), (0.05, 1.0), 12.0, 3)])
def test_exact_mode_is_invariant_restaurants(a, ns, hs, b, W):
    # pairs that share T: every pair's step (and so the sweep) leaves the joint invariant
    S1, tab = tables(a, max(ns))
    pi = tcw.joint(ns, hs, a, b, S1, tab, max(ns))
    P = tcw.sweep_matrix(ns, hs, a, b, W, S1, tab, max(ns))
    assert np.max(np.abs(pi @ P - pi)) <= 1e-12


def test_exact_mode_truncated():
    # M < n: invariant for the joint restricted to t <= M
    n, a, b, h, W, M = 12, 0.6, 2.0, 0.7, 1, 5
    S1, tab = orc.fill_S(a, n, M)
    pi = tcw.joint((n,), (h,), a, b, S1, tab, M)
    P = tcw.sweep_matrix((n,), (h,), a, b, W, S1, tab, M)
    assert P.shape == (M, M)
    assert np.max(np.abs(pi @ P - pi)) <= 1e-12


@pytest.mark.parametrize("row,gap", REF_ROWS)
def test_reference_mode_is_biased(row, gap):
    n, a, b, h, W = row
    S1, tab = tables(a, n)
    pi = tcw.joint((n,), (h,), a, b, S1, tab, n)
    P = tcw.sweep_matrix((n,), (h,), a, b, W, S1, tab, n, ref=True)
    assert np.max(np.abs(pi @ P - pi)) > 1e-4
    d = float(np.max(np.abs(tcw.stationary(P) - pi)))
    assert abs(d - gap) < 1e-3, d


def test_reference_mode_is_biased_in_a_restaurant():
    ns, hs, a, b, W = (8, 5), (1.0, 1.0), 0.5, 1.0, 1
    S1, tab = tables(a, 8)
    pi = tcw.joint(ns, hs, a, b, S1, tab, 8)
    P = tcw.sweep_matrix(ns, hs, a, b, W, S1, tab, 8, ref=True)
    assert np.max(np.abs(tcw.stationary(P) - pi)) > 1e-3


@pytest.mark.parametrize("ref", [False, True])
@pytest.mark.parametrize("W", [11, 12, 100])
def test_wide_window_is_the_full_conditional(W, ref):
    # W >= Mt - 1: every proposal is the full conditional and is accepted -- stb_tcounts' kernel, in law
    n, a, b, h = 12, 0.4, 1.5, 0.6
    S1, tab = tables(a, n)
    lw = tco.log_weights(n, 3, a, b, h, n, S1, tab, n)
    p = np.exp(lw - lw.max())
    p /= p.sum()
    P = tcw.pair_kernel(lw, W, ref)
    assert np.max(np.abs(P - p[None, :])) < 1e-14
    # and draw for draw: the same uniform u1 gives the full sweep's tau
    rng = np.random.default_rng(W)
    for u in rng.random(200):
        for t in (1, 6, 12):
            got, _, _ = tcw.step(lw, t, W, float(u), 0.5, ref)
            assert got == tco.draw(lw, float(u))[0]


def test_oracle_sweep_edge_cases():
    a, M, W = 0.5, 12, 2
    S1, tab = orc.fill_S(a, 12, M)
    K = np.array([4, 3], dtype=np.int32)
    n = np.array([0, 1, 12, 5, 9, 0, 1], dtype=np.uint32)
    t = np.array([0, 1, 3, 2, 9, 0, 1], dtype=np.uint16)
    for s in range(6):
        prev = t.copy()
        t, T, _ = tcw.sweep(K, n, t, None, a, [1.0, 3.0], M, S1, tab, M, W, 99, s)
        assert t[0] == 0 and t[5] == 0 and t[1] == 1 and t[6] == 1
        assert np.all((t[n > 0] >= 1) & (t[n > 0] <= n[n > 0]))
        assert np.all(np.abs(t.astype(int) - prev.astype(int)) <= W)
        assert T.tolist() == [int(t[:4].sum()), int(t[4:].sum())]


def test_uniforms_follow_the_indicator_convention():
    import ti_oracle as tio

    u1, u2 = tcw.uniforms(0x77, 3, 20)
    v1, v2 = tio.uniforms(0x77, 3, 20)
    assert np.array_equal(u1, v1) and np.array_equal(u2, v2)
    # the same stream as stb_tcounts': u1 of pair g is element 2g+1
    full = tco.uniforms(0x77, 3, 40)
    assert np.array_equal(u1, full[0::2]) and np.array_equal(u2, full[1::2])


def test_entry_points_exist():
    L = capi.lib()
    for name in ("stb_sample_tcounts_window", "stb_tcounts_sweep_window"):
        assert hasattr(L, name), name


def test_inputs_are_checked_before_any_device():
    L = capi.lib()
    args = dict(N=10, M=10, a=0.5, W=3, flags=0)

    def call(**kw):
        p = {**args, **kw}
        return L.stb_sample_tcounts_window(None, None, p["N"], p["M"], p["a"], None, 1, None, None, None, None, None,
                                           p["W"], p["flags"], 1, 0, None)

    for kw, msg in ((dict(a=1.0), "outside [0, 1)"), (dict(W=0), "W=0"), (dict(flags=2), "unknown flags"),
                    (dict(M=70000), "M=70000")):
        assert call(**kw) != 0
        assert msg in capi.last_error()
    assert L.stb_tcounts_sweep_window(None, 0.5, None, 3, 0, 1, 0, 1) != 0
    assert "null object" in capi.last_error()
    # no restaurants: nothing to do, no device needed
    assert L.stb_sample_tcounts_window(None, None, 10, 10, 0.5, None, 0, None, None, None, None, None, 3, 0, 1, 0, None) == 0
