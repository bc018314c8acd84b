"""The dish sweep's law, without a GPU: the exact one-sweep transition matrix of tests/td_oracle.py leaves the joint
pi(z, t) ~ (b|a)_T prod_k S^{n_k}_{t_k} h_k^{t_k} prod_c L[cls_c][z_c] invariant, and with a one-hot likelihood it is the
indicator sweep's matrix."""
import ctypes as C
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

import orc
import td_oracle as tdo
import ti_oracle as tio
from libstb_amd import capi

CASES = {
    "4x2": dict(Nc=4, K=2, hs=(0.7, 1.6), a=0.4, b=1.5, cls=None, lik=None, M=None),
    "4x3_two_classes_zero_entry": dict(Nc=4, K=3, hs=(0.5, 1.3, 2.0), a=0.3, b=0.8, cls=(0, 1, 0, 1),
                                       lik=((0.9, 0.0, 2.5), (0.2, 1.1, 0.6)), M=None),
    "5x2_a0": dict(Nc=5, K=2, hs=(1.2, 0.4), a=0.0, b=2.0, cls=None, lik=None, M=None),
    "5x2_M2": dict(Nc=5, K=2, hs=(0.6, 1.9), a=0.6, b=0.7, cls=(0, 0, 1, 1, 0), lik=((1.0, 0.5), (0.3, 2.0)), M=2),
}


@pytest.mark.parametrize("name", list(CASES))
def test_one_sweep_leaves_the_joint_invariant(name):
    c = CASES[name]
    p = tdo.joint(**c)
    assert np.all(p >= 0) and abs(p.sum() - 1.0) < 1e-14
    P = tdo.sweep_matrix(**c)
    assert np.max(np.abs(P.sum(axis=1) - 1.0)) < 1e-13
    # every visit on its own, and the sweep
    for cc in range(c["Nc"]):
        assert np.max(np.abs(p @ tdo.visit_matrix(cc, **c) - p)) < 1e-12
    assert np.max(np.abs(p @ P - p)) < 1e-12


def test_the_wrong_law_is_seen():
    # u3 ignored (always the first dish of positive weight): the joint is not invariant, so the check above can fail
    c = CASES["4x3_two_classes_zero_entry"]
    p = tdo.joint(**c)
    assert np.max(np.abs(p @ tdo.sweep_matrix(first_dish=True, **c) - p)) > 1e-2


@pytest.mark.parametrize("a,M", [(0.4, None), (0.0, None), (0.7, 2)])
def test_one_hot_likelihood_is_the_indicator_sweep(a, M):
    # every customer's row is one-hot on its own dish: z never changes, and t moves as under ti_oracle.sweep_matrix
    z0 = (0, 1, 1, 0, 1)
    hs, b, K, Nc = (0.8, 1.7), 1.3, 2, 5
    P = tdo.sweep_matrix(Nc, K, hs, a, b, cls=z0, lik=np.eye(2), M=M)
    st = tdo.states(Nc, K, M)
    rows = [j for j, (z, _) in enumerate(st) if z == z0]
    assert np.max(np.abs(P[rows][:, rows].sum(axis=1) - 1.0)) < 1e-14  # nothing leaves z0
    ns = tdo.counts(z0, K)
    assert [st[j][1] for j in rows] == tio.states(ns, M)
    want = tio.sweep_matrix(ns, hs, a, b, list(z0), tio.ExactV(list(range(1, Nc + 1)), a, M), M=M)
    assert np.max(np.abs(P[rows][:, rows] - want)) < 1e-14


def test_cumsum64_association():
    rng = np.random.default_rng(1)
    for K in (1, 9, 64, 65, 130):
        z = rng.random(K) * 10.0 ** rng.integers(-3, 4, size=K)
        cum = tdo.cumsum64(z)
        assert len(cum) % 64 == 0 and abs(cum[-1] - z.sum()) <= 1e-12 * z.sum()
        # the scan by its definition, lane by lane
        nb = len(cum) // 64
        x = np.zeros(nb * 64)
        x[:K] = z
        base = 0.0
        for j in range(nb):
            blk = list(x[j * 64:(j + 1) * 64])
            d = 1
            while d < 64:
                blk = [blk[l] + blk[l - d] if l >= d else blk[l] for l in range(64)]
                d *= 2
            blk = [base + v for v in blk]
            assert np.array_equal(cum[j * 64:(j + 1) * 64], np.array(blk))
            base = blk[63]


def test_choose_skips_dishes_without_weight():
    z = np.array([0.0, 1.0, 0.0, 1.0, 0.0])
    assert tdo.choose(z, 0.0) == 1 and tdo.choose(z, 0.49) == 1 and tdo.choose(z, 0.5) == 3
    assert tdo.choose(z, 1.0) == 3  # (no cum above thr: the largest k with weight)
    assert tdo.choose(np.zeros(3), 0.3) is None and tdo.choose(np.array([1.0, np.inf]), 0.3) is None


# ---- the host restatement (tools/tdish_host.c) and the C entry points, without a GPU ----

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_sweep(tmp_path):
    out = str(tmp_path / "libtdish_host.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, os.path.join(ROOT, "tools", "tdish_host.c"),
                    "-lm"], check=True)
    L = C.CDLL(out)
    vp, d, u, u64 = C.c_void_p, C.c_double, C.c_uint, C.c_uint64
    L.td_host_sweep.restype = d
    L.td_host_sweep.argtypes = [vp, u, u, d, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, u, vp, vp, vp, vp, u64, u64, u64, vp]
    return L.td_host_sweep


@pytest.mark.parametrize("a,M,with_lik", [(0.4, 40, True), (0.0, 40, False), (0.7, 5, True)])
def test_the_host_restatement_draws_what_the_oracle_draws(tmp_path, a, M, with_lik):
    f = host_sweep(tmp_path)
    rng = np.random.default_rng(3)
    N = 40
    packed = np.ascontiguousarray(orc.fill_V(a, N, M), dtype=np.float64)
    vt = tio.VTab(packed, N, M)
    K = np.array([1, 7, 70, 3], dtype=np.int32)  # 70: two blocks of the scan
    w = [rng.dirichlet(np.ones(k)) for k in K]
    n = np.concatenate([rng.multinomial(c, p) for c, p in zip((40, 40, 38, 0), w)]).astype(np.uint32)
    t = np.where(n > 0, 1 + np.floor(rng.random(len(n)) * np.minimum(n, M)), 0).astype(np.uint16)
    h = 0.1 + rng.random(len(n))
    cust = np.concatenate([rng.permutation(np.repeat(np.arange(k), n[o:o + k].astype(np.int64)))
                           for k, o in zip(K, np.concatenate([[0], np.cumsum(K)[:-1]]))]).astype(np.uint32)
    Ctot = len(cust)
    cls = rng.integers(0, 3, size=Ctot).astype(np.uint32)
    lik = 0.1 + rng.random((3, 72))
    lik[rng.random((3, 72)) < 0.2] = 0.0
    lik[2, :] = 0.0  # a class that is stuck
    bpar = np.array([0.5, 2.0, 7.0, 1.0])
    koff = np.concatenate([[0], np.cumsum(K)]).astype(np.uint64)
    Ni = np.array([x.sum() for x in np.split(n.astype(np.int64), np.cumsum(K)[:-1])])
    coff = np.concatenate([[0], np.cumsum(Ni)]).astype(np.uint64)
    nh, th, ch = n.copy(), t.copy(), cust.copy()
    Th = np.array([x.sum() for x in np.split(t.astype(np.int64), np.cumsum(K)[:-1])]).astype(np.uint32)
    want = (n, t, None, cust)
    total_stuck = 0
    for s in range(3):
        stuck = C.c_uint64(0)
        f(packed.ctypes.data, N, M, a, bpar.ctypes.data, 0, 4, koff.ctypes.data, coff.ctypes.data, ch.ctypes.data,
          cls.ctypes.data if with_lik else None, lik.ctypes.data if with_lik else None, 72, nh.ctypes.data, th.ctypes.data,
          Th.ctypes.data, h.ctypes.data, Ctot, 17, s, C.byref(stuck))
        want = tdo.sweep(K, want[0], want[1], h, a, bpar, vt, N, M, 17, s, want[3], cls if with_lik else None,
                         lik if with_lik else None)
        for name, g, x in zip(("n", "t", "T", "cust"), (nh, th, Th, ch), want[:4]):
            assert np.array_equal(g, x), (s, name)
        assert stuck.value == want[5] and want[4] == 0
        total_stuck += want[5]
    assert not np.array_equal(ch, cust)
    assert (total_stuck > 0) == with_lik


def test_entry_points_exist():
    L = capi.lib()
    for name in ("stb_sample_tdishes", "stb_tindic_set_classes", "stb_tindic_set_lik", "stb_tindic_lik_device",
                 "stb_tindic_sweep_dishes", "stb_tindic_get_state", "stb_tindic_class_counts"):
        assert hasattr(L, name), name
    assert capi.TD_MAXK == 1024
    # refused before any device is touched
    args = [None, 10, 10, 1.0] + [None] * 2 + [None] * 9 + [0, 0, 1, 0, None, None]
    args[5] = 1
    assert L.stb_sample_tdishes(*args) != 0 and "outside [0, 1)" in capi.last_error()
    args[3] = 0.5
    assert L.stb_sample_tdishes(*args) != 0 and "d_cust" in capi.last_error()
    assert L.stb_tindic_sweep_dishes(None, 0.5, None, 1, 0, 1, None) != 0 and "null object" in capi.last_error()


_spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(ROOT, "tools", "kernel_regs.py"))
kernel_regs = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kernel_regs)


@pytest.mark.skipif(not os.path.exists(os.path.join(kernel_regs.LLVM, "llvm-readelf")) or shutil.which("c++filt") is None,
                    reason="llvm-readelf / c++filt not on this machine")
def test_kernels_do_not_spill():
    ks = {n: k for n, k in kernel_regs.kernels(capi.LIB_PATH).items() if n.startswith("void k_tdish") or n.startswith("k_tdish")}
    assert len(ks) == 2, sorted(ks)
    bad = {n: k for n, k in ks.items() if k["spill"] or k["scratch"]}
    assert not bad, bad
    print(ks)
