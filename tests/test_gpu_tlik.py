"""The likelihood and the base weights drawn on the device, and the data term (libstb_amd/csrc/tlik.hip; include/stb_hip.h
"the likelihood and the base weights"): cell for cell against the numpy replay (tests/tl_oracle.py), the normalisation,
launch geometries, the law, the object layer end to end, the refusals and examples/pyp_resample -w."""
import math
import os
import re
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import hq_oracle as hqo
import lj_oracle as lj
import ti_oracle as tio
import tl_oracle as tlo
from libstb_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def dev_u32(x):
    import torch

    return torch.as_tensor(np.array(x, dtype=np.uint32).view(np.int32), device="cuda")


def dev_f64(x):
    import torch

    return torch.as_tensor(np.array(x, dtype=np.float64), device="cuda")


def device_lik(cnt, beta, seed, sweep):
    import torch

    out = capi.sample_lik(dev_u32(cnt), beta, seed, sweep)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@lru_cache(maxsize=None)
def case(name):
    """(cnt, beta, seed, sweep, the replay's matrix, the device's matrix) of a replay case, computed once"""
    cnt, beta, seed, sweep = tlo.lik_case(name)
    want, _ = tlo.sample_lik(cnt, beta, seed, sweep)
    got = device_lik(cnt, beta, seed, sweep)
    for a in (cnt, want, got):
        a.setflags(write=False)
    return cnt, beta, seed, sweep, want, got


def assert_replayed(got, want, what):
    """the project's standing 1e-10 relative where the replay's value is >= 1e-280, 1e-290 absolute below; no cell left out"""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    assert got.shape == want.shape and not np.isnan(got).any()
    big = want >= 1e-280
    err = np.abs(got - want)
    rel = float((err[big] / want[big]).max()) if big.any() else 0.0
    small = float(err[~big].max()) if (~big).any() else 0.0
    print(what, "cells", got.size, "largest relative error", rel, "largest absolute error below 1e-280", small,
          "cells below", int((~big).sum()))
    assert rel <= 1e-10, (what, rel)
    assert small <= 1e-290, (what, small)


def read_lik(ti):
    L = capi.lib()
    p, rows, stride, q = ti.lik_device()
    out = np.empty((rows, stride), dtype=np.float64)
    capi.check(L.stb_memcpy_d2h(out.ctypes.data, p, out.nbytes, q))
    capi.check(L.stb_stream_sync(q))
    return out


def full_state(ti):
    t, T = ti.get()
    n, cust = ti.get_state()
    return n, t, T, cust, read_lik(ti), ti.get_h()


def assert_same_state(got, want):
    for name, g, w in zip(("n", "t", "T", "cust", "lik", "h"), got, want):
        assert np.array_equal(g, w), name


# ---- 1. replay, raw layer ----

@pytest.mark.parametrize("name", list(tlo.LIK_CASES))
def test_every_cell_equals_the_replay(name):
    cnt, beta, seed, sweep, want, got = case(name)
    assert_replayed(got, want, name)
    if cnt.shape[0] == 1:
        assert np.all(got == 1.0)


# ---- 2. normalisation ----

@pytest.mark.parametrize("name", list(tlo.LIK_CASES))
def test_columns_sum_to_one(name):
    cnt, _, _, _, _, got = case(name)
    rows = cnt.shape[0]
    assert np.all(np.isfinite(got)) and got.min() >= 0.0 and got.max() <= 1.0
    worst = max(abs(math.fsum(got[:, k]) - 1.0) for k in range(got.shape[1]))
    print(name, "largest |column sum - 1|", worst, "bar", 2.0 * U * rows)
    assert worst <= 2.0 * U * rows


# ---- 3. geometry ----

def small_object(with_lik=True, flags=0, seed=21):
    """6 restaurants of up to 70 dishes, 3 classes, a matrix of 4 rows x 72"""
    rng = np.random.default_rng(seed)
    K = np.array([70, 9, 64, 1, 65, 30], dtype=np.int32)
    G = int(K.sum())
    n = rng.integers(0, 9, size=G).astype(np.uint32)
    t = np.where(n > 0, 1 + np.floor(rng.random(G) * n), 0).astype(np.uint16)
    h = 0.05 + rng.random(G)
    cust = np.concatenate([rng.permutation(np.repeat(np.arange(k, dtype=np.uint32), n[o:o + k].astype(np.int64)))
                           for k, o in zip(K, np.concatenate([[0], np.cumsum(K)[:-1]]))]).astype(np.uint32)
    cls = rng.integers(0, 3, size=len(cust)).astype(np.uint32)
    ti = capi.TableIndicators(K, n, t, h, cust, 0, flags)
    if with_lik:
        ti.set_classes(cls, 3)
        ti.set_lik(0.1 + rng.random((4, 72)))
    return ti, K, n, t, h, cust, cls


def test_the_bits_do_not_depend_on_the_workgroup(monkeypatch):
    cnt, beta, seed, sweep, _, got = case("600x70_vec")
    d_cnt, d_lik = dev_u32(cnt), dev_f64(got)
    ll0 = capi.lik_loglik(d_cnt, d_lik)
    ti, K, n, t, h, cust, cls = small_object()
    try:
        gamma = 0.2 + np.arange(70) / 35.0
        ti.sample_h(gamma, 31, 2)
        h0 = ti.get_h()
        assert not np.array_equal(h0, h)
        for waves in (1, 2, 4, 8, 4):
            monkeypatch.setenv("STB_TLIK_WAVES", str(waves))
            assert np.array_equal(device_lik(cnt, beta, seed, sweep), got), waves
            assert capi.lik_loglik(d_cnt, d_lik) == ll0, waves
            ti.sample_h(gamma, 31, 2)
            assert np.array_equal(ti.get_h(), h0), waves
    finally:
        ti.free()


# ---- 4. law ----

def test_the_law_of_the_likelihood_draw():
    base, beta0 = np.array([3, 0, 17, 1], dtype=np.uint32), 0.3
    cnt = np.tile(base.reshape(4, 1), (1, 4096))
    lik = device_lik(cnt, beta0, 41, 0)
    alpha = beta0 + base.astype(np.float64)
    assert np.all(lik > 0.0)
    for w in range(4):  # p_w ~ Beta(alpha_w, alpha_0 - alpha_w), and moment_check takes -log of such a variable
        ok, text = hqo.moment_check(-np.log(lik[w]), float(alpha[w]), float(alpha.sum() - alpha[w]))
        print("class", w, text)
        assert ok, text
    # it can fail: the same draws against a prior of 0.6
    ok, text = hqo.moment_check(-np.log(lik[1]), 0.6, float(alpha.sum() - alpha[1]))
    assert not ok, text


def test_the_law_of_the_base_weights():
    K = np.array([5, 5, 5], dtype=np.int32)
    n = np.array([4, 9, 1, 0, 6, 2, 2, 0, 3, 8, 5, 0, 7, 1, 1], dtype=np.uint32)
    t = np.array([2, 3, 1, 0, 1, 1, 2, 0, 3, 2, 4, 0, 1, 1, 1], dtype=np.uint16)
    gamma = 0.7
    c = tlo.table_counts(K, t)
    alpha = gamma + c.astype(np.float64)
    ti = capi.TableIndicators(K, n, t)
    try:
        hs = np.empty((2000, 5))
        for s in range(2000):
            ti.sample_h(gamma, 51, s)
            hs[s] = ti.get_h()[:5]
    finally:
        ti.free()
    for k in range(5):
        ok, text = hqo.moment_check(-np.log(hs[:, k]), float(alpha[k]), float(alpha.sum() - alpha[k]))
        print("dish", k, text)
        assert ok, text


# ---- 5. base weights ----

def test_base_weights_equal_the_replay():
    c = tlo.H_CASE
    K, n, t = np.array(c["K"], dtype=np.int32), np.array(c["n"], dtype=np.uint32), np.array(c["t"], dtype=np.uint16)
    hk, _ = tlo.sample_h(c["K"], c["t"], c["gamma"], c["seed"], c["sweep"])
    want = tlo.spread_h(c["K"], hk)
    a, bpar = 0.4, np.array([1.5, 0.7, 3.0])
    ti = capi.TableIndicators(K, n, t, 0.3 + np.arange(9) / 10.0)
    try:
        t0, T0 = ti.get()
        ti.sample_h(c["gamma"], c["seed"], c["sweep"])
        got = ti.get_h()
        assert_replayed(got, want, "h")
        assert got[0] == got[5] == got[8] and got[1] == got[6] and got[2] == got[7]  # one double a dish
        t1, T1 = ti.get()
        assert np.array_equal(t0, t1) and np.array_equal(T0, T1) and np.array_equal(t1, t)
        tot, Li, info = ti.logjoint(a, bpar)
        tr = lj.truth(K, n, t, want, a, bpar, lj.Tables(a, 9, 9))
        base, bar = tr["base"]
        host = math.fsum(int(x) * math.log(y) for x, y in zip(t, want) if x)
        print("base", info.base, "truth", base, "bar", bar, "sum t log h", host)
        assert abs(host - base) <= bar
        assert lj.within(info.base, base, bar), (info.base, base, bar)
        # a scalar prior, and the draw replaces h again
        g2, seed2, sweep2 = tlo.H_CASE_SCALAR
        ti.sample_h(g2, seed2, sweep2)
        hk2, _ = tlo.sample_h(c["K"], c["t"], g2, seed2, sweep2)
        assert_replayed(ti.get_h(), tlo.spread_h(c["K"], hk2), "h, scalar gamma")
    finally:
        ti.free()


# ---- 6. data term ----

def exact_loglik(cnt, lik):
    """(sum cnt log lik, sum |cnt log lik|) with the log in mpmath, or in long double where it is absent"""
    nz = cnt > 0
    c, l = cnt[nz].astype(np.float64), lik[nz]
    try:
        import mpmath as mp

        x = [mp.mpf(float(a)) * mp.log(mp.mpf(float(b))) for a, b in zip(c, l)]
        return float(mp.fsum(x)), float(mp.fsum(abs(v) for v in x))
    except ImportError:
        x = c.astype(np.longdouble) * np.log(l.astype(np.longdouble))
        return float(x.sum()), float(np.abs(x).sum())


def test_the_data_term():
    import torch

    cnt, _, _, _, _, lik = case("600x70_b1.5")
    rows, stride = cnt.shape
    assert lik[cnt > 0].min() > 0.0
    tot, imp = capi.lik_loglik(dev_u32(cnt), dev_f64(lik))
    want, mag = exact_loglik(cnt, lik)
    bar = U * (258 + math.ceil(rows / 256) + stride) * mag
    print("data term", tot, "exact", want, "difference", tot - want, "bar", bar)
    assert imp == 0 and abs(tot - want) <= bar
    # a zero under a positive count: -inf, counted, no NaN; a zero under a zero count changes nothing
    z = lik.copy()
    w, k = np.argwhere(cnt > 0)[137]
    z[w, k] = 0.0
    tot_z, imp_z = capi.lik_loglik(dev_u32(cnt), dev_f64(z))
    assert tot_z == -math.inf and imp_z == 1
    z = lik.copy()
    w, k = np.argwhere(cnt == 0)[59]
    z[w, k] = 0.0
    assert capi.lik_loglik(dev_u32(cnt), dev_f64(z)) == (tot, 0)
    torch.cuda.synchronize()


# ---- 7. object layer end to end ----

def planted(I=200, Nc=50, Kd=8, rows=20, seed=61):
    """restaurants that serve three dishes each; dish k's customers come from classes 2k, 2k+1 (0.45 each) and the rest"""
    rng = np.random.default_rng(seed)
    phi = np.full((rows, Kd), 0.1 / (rows - 2))
    for k in range(Kd):
        phi[2 * k, k] = phi[2 * k + 1, k] = 0.45
    z = np.concatenate([rng.choice(rng.choice(Kd, size=3, replace=False), size=Nc) for _ in range(I)]).astype(np.uint32)
    cls = np.array([rng.choice(rows, p=phi[:, k]) for k in z], dtype=np.uint32)
    return z, cls


def object_of(cust, I, Nc, Kd):
    n = np.stack([np.bincount(cust[i * Nc:(i + 1) * Nc].astype(np.int64), minlength=Kd) for i in range(I)]).astype(np.uint32)
    t = (n > 0).astype(np.uint16)
    return capi.TableIndicators(np.full(I, Kd, dtype=np.int32), n.reshape(-1), t.reshape(-1), None, cust)


def test_the_chain_end_to_end():
    I, Nc, Kd, rows = 200, 50, 8, 20
    z, cls = planted(I, Nc, Kd, rows)
    C_ = I * Nc
    a, bpar = 0.3, np.full(I, 2.0)
    start = np.random.default_rng(62).integers(0, Kd, size=C_).astype(np.uint32)
    ti = object_of(start, I, Nc, Kd)
    try:
        ti.set_classes(cls, rows)
        ti.set_lik(None, rows, Kd)
        # iteration 0: the random start, with a likelihood and base weights drawn given it
        ti.sample_lik(0.5, 63, 1000)
        ti.sample_h(1.0, 64, 1000)
        first = ti.logjoint(a, bpar, True)[0] + ti.loglik()[0]
        for it in range(30):
            info = ti.sweep_dishes(a, bpar, 65, it)
            ti.sample_lik(0.5, 63, it)
            ti.sample_h(1.0, 64, it)
            ti.sweep(a, bpar, 66, it)
            assert info.stuck + info.skipped == 0
            assert int(ti.class_counts().sum()) == C_
            lik = read_lik(ti)
            assert lik.shape == (rows, Kd) and all(abs(math.fsum(lik[:, k]) - 1.0) <= 2.0 * U * rows for k in range(Kd))
        dt, imp = ti.loglik()
        last = ti.logjoint(a, bpar, True)[0] + dt
        print("complete-data log joint: start", first, "after 30 iterations", last)
        assert imp == 0 and math.isfinite(first) and math.isfinite(last) and last > first
        h = ti.get_h().reshape(I, Kd)
        assert np.all(h == h[0]) and abs(math.fsum(h[0]) - 1.0) <= 2.0 * U * Kd
    finally:
        ti.free()


def test_a_planted_likelihood_comes_back():
    I, Nc, Kd, rows = 200, 50, 8, 20
    z, _ = planted(I, Nc, Kd, rows)
    cls = (2 * z).astype(np.uint32)  # one-hot: dish k's customers are all of class 2k
    onehot = np.zeros((rows, Kd))
    onehot[2 * np.arange(Kd), np.arange(Kd)] = 1.0
    ti = object_of(z, I, Nc, Kd)
    try:
        ti.set_classes(cls, rows)
        ti.set_lik(onehot)
        assert ti.loglik() == (0.0, 0)
        ti.sample_lik(1e-3, 71, 0)
        lik = read_lik(ti)
        assert np.array_equal(lik.argmax(axis=0), 2 * np.arange(Kd))
        assert all(abs(math.fsum(lik[:, k]) - 1.0) <= 2.0 * U * rows for k in range(Kd))
    finally:
        ti.free()


# ---- 8. refusals ----

def test_refusals_leave_the_state():
    L = capi.lib()
    ti, K, n, t, h, cust, cls = small_object()
    bare, *_ = small_object(with_lik=False)
    odd, *_ = small_object(flags=capi.TI_REF_ODDS)
    try:
        before = full_state(ti)
        odd_h = odd.get_h()
        bad_vec = np.full(4, 0.5)
        bad_vec[2] = 0.0
        for beta in (0.0, -1.0, math.nan, math.inf, bad_vec):
            with pytest.raises(capi.StbError, match="beta"):
                ti.sample_lik(beta, 1, 0)
        bad_g = np.full(70, 1.0)
        bad_g[69] = math.inf
        for gamma in (0.0, -2.0, math.nan, math.inf, bad_g):
            with pytest.raises(capi.StbError, match="gamma"):
                ti.sample_h(gamma, 1, 0)
        with pytest.raises(capi.StbError, match="STB_TI_REF_ODDS"):
            odd.sample_h(1.0, 1, 0)
        assert np.array_equal(odd.get_h(), odd_h)
        # no classes, no matrix
        for call in (lambda: bare.sample_lik(0.5, 1, 0), bare.loglik):
            with pytest.raises(capi.StbError, match="classes are not set"):
                call()
        bare.set_classes(cls, 3)
        for call in (lambda: bare.sample_lik(0.5, 1, 0), bare.loglik):
            with pytest.raises(capi.StbError, match="no likelihood matrix"):
                call()
        ti.set_classes(np.full(len(cust), 4, dtype=np.uint32), 5)  # more classes than the matrix has rows
        with pytest.raises(capi.StbError, match="rows"):
            ti.sample_lik(0.5, 1, 0)
        ti.set_classes(cls, 3)
        # null objects and arrays, empty shapes
        assert L.stb_tindic_sample_lik(None, None, 0.5, 1, 0) != 0 and "null object" in capi.last_error()
        assert L.stb_tindic_sample_h(None, None, 0.5, 1, 0) != 0 and "null object" in capi.last_error()
        assert L.stb_tindic_loglik(None, None, None) != 0 and "null object" in capi.last_error()
        assert L.stb_tindic_loglik(ti.h, None, None) != 0 and "total" in capi.last_error()
        d_cnt, d_lik = dev_u32(np.zeros((4, 72))), dev_f64(np.ones((4, 72)))
        keep = d_lik.clone()
        sp = capi.stream_ptr()
        tot = capi.C.c_double(0.0)
        for args, match in (((None, 4, 72, None, 0.5, d_lik.data_ptr(), 1, 0, sp), "required"),
                            ((d_cnt.data_ptr(), 4, 72, None, 0.5, None, 1, 0, sp), "required"),
                            ((d_cnt.data_ptr(), 0, 72, None, 0.5, d_lik.data_ptr(), 1, 0, sp), "rows=0"),
                            ((d_cnt.data_ptr(), 4, 0, None, 0.5, d_lik.data_ptr(), 1, 0, sp), "stride=0"),
                            ((d_cnt.data_ptr(), 4, 72, None, 0.0, d_lik.data_ptr(), 1, 0, sp), "beta"),
                            ((d_cnt.data_ptr(), 4, 72, capi.dp(bad_vec), 0.0, d_lik.data_ptr(), 1, 0, sp), "beta\\[2\\]")):
            assert L.stb_sample_lik(*args) != 0 and re.search(match, capi.last_error()), (match, capi.last_error())
        for args, match in (((None, d_lik.data_ptr(), 4, 72, capi.C.byref(tot), None, sp), "required"),
                            ((d_cnt.data_ptr(), d_lik.data_ptr(), 4, 72, None, None, sp), "required"),
                            ((d_cnt.data_ptr(), d_lik.data_ptr(), 0, 72, capi.C.byref(tot), None, sp), "rows=0"),
                            ((d_cnt.data_ptr(), d_lik.data_ptr(), 4, 0, capi.C.byref(tot), None, sp), "stride=0")):
            assert L.stb_lik_loglik(*args) != 0 and re.search(match, capi.last_error()), (match, capi.last_error())
        import torch

        torch.cuda.synchronize()
        assert torch.equal(d_lik, keep)
        assert_same_state(full_state(ti), before)
        # nothing above changed what the calls do
        ref, *_ = small_object()
        try:
            for o in (ti, ref):
                o.sample_lik(0.5, 5, 1)
                o.sample_h(1.0, 6, 1)
                o.sweep_dishes(0.4, np.full(6, 1.5), 7, 0)
            assert_same_state(full_state(ti), full_state(ref))
        finally:
            ref.free()
    finally:
        ti.free()
        bare.free()
        odd.free()


def test_a_refused_draw_leaves_an_object_without_h():
    c = tlo.H_CASE
    K, n, t = np.array(c["K"], dtype=np.int32), np.array(c["n"], dtype=np.uint32), np.array(c["t"], dtype=np.uint16)
    a, bpar = 0.4, np.array([1.5, 0.7, 3.0])
    v = capi.DeviceVTables(9, 9)  # the object's own bounds: max n = 9
    v.fill(a)
    capi.check(capi.lib().stb_fill_status())
    vt = tio.VTab(v.packed_host(0), 9, 9)
    ti = capi.TableIndicators(K, n, t)  # created without h
    try:
        for gamma in (0.0, math.nan):
            with pytest.raises(capi.StbError, match="gamma"):
                ti.sample_h(gamma, c["seed"], c["sweep"])
        assert np.array_equal(ti.get_h(), np.ones(9))
        ti.sweep(a, bpar, 11, 0)
        t1, T1 = tio.sweep(K, n, t, None, a, bpar, vt, 9, 11, 0)  # (h None: every h is 1)
        got_t, got_T = ti.get()
        assert np.array_equal(got_t, t1) and np.array_equal(got_T, T1)
        # a draw that goes through gives the object its h
        ti.sample_h(c["gamma"], c["seed"], c["sweep"])
        hk, _ = tlo.sample_h(c["K"], t1, c["gamma"], c["seed"], c["sweep"])
        assert_replayed(ti.get_h(), tlo.spread_h(c["K"], hk), "h of an object created without one")
    finally:
        ti.free()


# ---- 9. example ----

EXE = os.path.join(ROOT, "examples", "bin", "pyp_resample")
ARGS = ["-J", "3", "-n", "400", "-c", "9", "-s", "5", "-d", "-z", "-L"]


def test_example_redraws_the_likelihood():
    assert os.path.exists(EXE), "examples/bin/pyp_resample not built (make -C libstb_amd/csrc)"
    p = subprocess.run([EXE] + ARGS + ["-w"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = re.findall(r"^iteration (\d+): log joint (\S+) \(.*\) data (\S+) complete (\S+) a=", p.stdout, re.M)
    assert [int(r[0]) for r in rows] == list(range(9)), p.stdout
    for _, ljv, dt, comp in rows:
        assert math.isfinite(float(dt)) and float(dt) < 0.0
        assert abs(float(ljv) + float(dt) - float(comp)) <= 1e-5
    # -w alone, or without the dish sweep, is refused
    assert subprocess.run([EXE, "-d", "-w"], capture_output=True, text=True, timeout=60).returncode == 2


def test_example_without_the_flag_prints_what_it_printed(golden_dir):
    # tests/golden/pyp_resample_dzL.txt: the output of the build before -w existed, for these arguments.  To record it
    # again: check out the commit before the one that added -w ("Resample customers' dishes on the device under a fixed
    # likelihood"), make -C libstb_amd/csrc, and on an MI355X
    #     examples/bin/pyp_resample -J 3 -n 400 -c 9 -s 5 -d -z -L > tests/golden/pyp_resample_dzL.txt
    assert os.path.exists(EXE), "examples/bin/pyp_resample not built (make -C libstb_amd/csrc)"
    p = subprocess.run([EXE] + ARGS, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    want = open(os.path.join(golden_dir, "pyp_resample_dzL.txt")).read()
    assert "data " not in p.stdout.split("\n", 1)[1]
    assert p.stdout == want
