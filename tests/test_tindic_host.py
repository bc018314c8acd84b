"""The table-indicator sweep's oracle (tests/ti_oracle.py) against the PYP joint, exactly, and the C entry points of
stb_tindic_* / stb_sample_tindic without a GPU."""
import importlib.util
import os
import shutil

import numpy as np
import pytest

import orc
import ti_oracle as tio
from libstb_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, a, b, h) -> the reference factor's max |pi - joint|
ROWS = [((5, 0.0, 1.0, 1.0), 0.069), ((7, 0.3, 1.5, 0.5), 0.051), ((12, 0.5, 10.0, 1 / 50), 0.024), ((9, 0.9, 0.5, 2.0), 0.191)]


@pytest.mark.parametrize("row,gap", ROWS)
def test_one_dish_stationary_law(row, gap):
    n, a, b, h = row
    vt = tio.ExactV([n], a)
    want = tio.joint((n,), (h,), a, b)
    exact = tio.stationary(tio.sweep_matrix((n,), (h,), a, b, [0], vt))
    assert np.max(np.abs(exact - want)) < 1e-12
    ref = tio.stationary(tio.sweep_matrix((n,), (h,), a, b, [0], vt, ref=True))
    d = float(np.max(np.abs(ref - want)))
    assert d > 1e-3 and abs(d - gap) < 1e-3, d


@pytest.mark.parametrize("a", [0.0, 0.45, 0.8])
def test_coupled_stationary_law(a):
    # three dishes that share T, customers in a mixed order: the sweep leaves the joint invariant
    ns, hs, b = (4, 3, 5), (0.5, 1.3, 2.0), 1.5
    order = [0, 1, 2, 0, 2, 1, 0, 2, 0, 1, 2, 2]
    vt = tio.ExactV(ns, a)
    pi = tio.stationary(tio.sweep_matrix(ns, hs, a, b, order, vt))
    assert np.max(np.abs(pi - tio.joint(ns, hs, a, b))) < 1e-12


def test_truncated_law():
    # M < n: the joint restricted to t <= M
    n, a, b, h, M = 9, 0.4, 2.0, 0.7, 4
    vt = tio.ExactV([n], a, M)
    pi = tio.stationary(tio.sweep_matrix((n,), (h,), a, b, [0], vt, M=M))
    assert pi.shape == (M,)
    assert np.max(np.abs(pi - tio.joint((n,), (h,), a, b, M))) < 1e-12


def test_exact_V_against_the_oracle_table():
    a, N = 0.35, 30
    vt = tio.VTab(orc.fill_V(a, N, N), N, N)
    ev = tio.ExactV(list(range(2, N + 1)), a)
    for n in range(2, N + 1):
        for m in range(2, n + 1):
            assert orc.close(vt.V(n, m), ev.V(n, m), 1e-10), (n, m)


def test_uniforms_are_splitmix():
    seed, s = 0x1234, 5
    key = tio.sweep_key(seed, s)
    gamma, mask = 0x9E3779B97F4A7C15, (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        return z ^ (z >> 31)

    assert key == mix((seed + (s + 1) * gamma) & mask)
    u1, u2 = tio.uniforms(seed, s, 10)
    u = synth.unit(20, key)
    for c in range(10):
        assert u1[c] == (mix((key + (2 * c + 1) * gamma) & mask) >> 11) / 2.0**53 == u[2 * c]
        assert u2[c] == (mix((key + (2 * c + 2) * gamma) & mask) >> 11) / 2.0**53 == u[2 * c + 1]


def test_oracle_edge_cases():
    a, N, M = 0.5, 12, 4
    vt = tio.VTab(orc.fill_V(a, N, M), N, M)
    K = np.array([5, 2], dtype=np.int32)
    # n = 0, n = 1, t at M (t+1 > M: no indicator added), n > N (outside the table), an ordinary pair
    n = np.array([0, 1, 9, 20, 6, 1, 12], dtype=np.uint32)
    t = np.array([0, 1, 4, 7, 2, 1, 1], dtype=np.uint16)
    bpar = [1.0, 3.0]
    seen_at_M = False
    for s in range(20):
        t, T = tio.sweep(K, n, t, None, a, bpar, vt, N, 99, s)
        assert t[0] == 0 and t[1] == 1 and t[5] == 1 and t[3] == 7
        assert np.all(t[[2, 4, 6]] >= 1) and np.all(t[[2, 4, 6]] <= M)
        seen_at_M |= t[2] == M
        assert T.tolist() == [int(t[:5].sum()), int(t[5:].sum())]
    assert seen_at_M
    # a pair never moves above M, even from odds that would add one
    assert tio.visit(9, 4, 4, 1e300, a, 1.0, vt, 0.99, 0.0, False, N) == (4, 4)
    # with infinite odds the indicator is always added
    big = tio.VTab(np.full(len(vt.v), np.inf), N, M)
    assert tio.visit(9, 2, 2, 1.0, a, 1.0, big, 0.99, 0.999999, False, N) == (3, 3)


def test_pair_order_is_an_explicit_order():
    a, N = 0.3, 40
    vt = tio.VTab(orc.fill_V(a, N, N), N, N)
    g = synth.groups(5, 4, N, "realistic", seed=7)
    cust = tio.pair_order(g.K, g.n)
    assert len(cust) == int(g.n.sum())
    x = tio.sweep(g.K, g.n, g.t, None, a, g.bpar, vt, N, 3, 0)
    y = tio.sweep(g.K, g.n, g.t, None, a, g.bpar, vt, N, 3, 0, cust=cust)
    assert all(np.array_equal(p, q) for p, q in zip(x, y))


def test_entry_points_exist():
    L = capi.lib()
    for name in ("stb_sample_tindic", "stb_tindic_create", "stb_tindic_set_h", "stb_tindic_sweep", "stb_tindic_get",
                 "stb_tindic_to_groups", "stb_tindic_free"):
        assert hasattr(L, name), name
    assert capi.TI_REF_ODDS == 1


def test_create_without_or_with_a_device():
    L = capi.lib()
    g = synth.groups(4, 3, 50, "realistic")
    if L.stb_device_count() == 0:
        with pytest.raises(capi.StbError, match="no HIP device"):
            capi.TableIndicators(g.K, g.n, g.t)
    # invalid discounts and flags are refused before any device is touched
    args = [None, 10, 10, 1.0, None, 1, None, None, None, None, None, None, None, 0, 1, 0, None]
    assert L.stb_sample_tindic(*args) != 0
    assert "outside [0, 1)" in capi.last_error()
    args[3], args[13] = 0.5, 2
    assert L.stb_sample_tindic(*args) != 0
    assert "unknown flags" in capi.last_error()


_spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(ROOT, "tools", "kernel_regs.py"))
kernel_regs = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kernel_regs)


@pytest.mark.skipif(not os.path.exists(os.path.join(kernel_regs.LLVM, "llvm-readelf")) or shutil.which("c++filt") is None,
                    reason="llvm-readelf / c++filt not on this machine")
def test_kernels_do_not_spill():
    ks = {n: k for n, k in kernel_regs.kernels(capi.LIB_PATH).items() if n.startswith("k_tindic")}
    assert {n.split("(")[0] for n in ks} == {"k_tindic_lane", "k_tindic_wave"}, sorted(ks)
    bad = {n: k for n, k in ks.items() if k["spill"] or k["scratch"]}
    assert not bad, bad
