"""The log marginal of multinomials under a Dirichlet prior on the device (libstb_amd/csrc/dirmult.hip; include/stb_hip.h
stb_dirmult_logml) and the collapsed log joint built on it (stb_tindic_logjoint_collapsed): the raw call in both
orientations against the 40-digit truth within the bar of tests/dm_oracle.py, the bits across launch geometries and
across the ways to pass weights and scale, the edge rules and refusals, the object layer against the raw call, against
stb_tindic_logjoint and against the uncollapsed densities in mpmath, and examples/pyp_resample -C."""
import math
import os
import re
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import dm_oracle as dmo
import hp_oracle as hp
from libstb_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def dev(x, dtype):
    import torch

    a = np.ascontiguousarray(x, dtype=dtype)
    view = {np.uint16: np.int16, np.uint32: np.int32, np.uint64: np.int64}.get(dtype)
    return torch.as_tensor(a.view(view) if view else a, device="cuda")


def raw(cnt, cols, w, scale, orient, want_each=True):
    """the raw call on a host matrix cnt[rows, stride]: a dict shaped like dm_oracle.replay's"""
    wd = w if np.ndim(w) == 0 else dev(w, np.float64)
    tot, each, info = capi.dirmult_logml(dev(cnt, np.uint32), wd, orient, cols, scale, want_each)
    return {"total": tot, "each": None if each is None else each.cpu().numpy(), "cells": info.cells, "norms": info.norms,
            "nonzero": info.nonzero, "count": info.count, "zero_weight": info.zero_weight, "impossible": info.impossible}


@lru_cache(maxsize=None)
def ran(name):
    return raw(*dmo.case(name))


def same_bits(x, y):
    keys = ("total", "cells", "norms", "nonzero", "count", "zero_weight", "impossible")
    return all(np.float64(x[k]).tobytes() == np.float64(y[k]).tobytes() for k in keys) and \
        np.array_equal(np.asarray(x["each"]).view(np.uint64), np.asarray(y["each"]).view(np.uint64))


# ---- 1. against the oracle ----

@pytest.mark.parametrize("name", dmo.CASES)
def test_the_call_lies_within_the_bar_of_the_truth(name):
    got, want = ran(name), dmo.case_truth(name)
    for k in ("nonzero", "count", "zero_weight", "impossible"):
        assert got[k] == want[k], k
    assert got["each"].shape == want["each"].shape and not np.isnan(got["each"]).any()
    ratio = dmo.worst_ratio(got, want)
    print(name, "multinomials", got["each"].size, "worst |device - truth| / bar", ratio, "total", got["total"], "bar", want["total"][1])
    for k in ("cells", "norms", "total"):
        assert dmo.within(got[k], *want[k]), (k, got[k], want[k])
    assert ratio <= 1.0


@pytest.mark.parametrize("name", dmo.CASES)
def test_the_bits_do_not_depend_on_the_launch(name, monkeypatch):
    """1, 2, 4, 8 waves a workgroup; for the rows orientation also both forms (blocks of rows a workgroup; rows a wave
    over the grid, which few rows take by default)"""
    got = ran(name)
    for form in ("fused", "split") if name in dmo.ROW_CASES + ["cellrows"] else ("",):
        monkeypatch.setenv("STB_DIRMULT_FORM", form)
        for waves in (1, 2, 4, 8):
            monkeypatch.setenv("STB_DIRMULT_WAVES", str(waves))
            assert same_bits(raw(*dmo.case(name)), got), (form, waves)


# ---- 2. the ways to pass weights and scale, bit for bit ----

@pytest.mark.parametrize("orient", [dmo.ROWS, dmo.COLUMNS])
def test_weights_and_scale_however_passed_give_the_same_bits(orient):
    import torch

    cnt, cols, w, _, _ = dmo.case("rows_5_65_80" if orient == dmo.ROWS else "cols_257_65_70")
    ncat = cols if orient == dmo.ROWS else cnt.shape[0]
    # a scalar against the constant vector: 0.5 and a dyadic scale, so that both forms of W are exact
    assert same_bits(raw(cnt, cols, 0.5, 0.25, orient), raw(cnt, cols, np.full(ncat, 0.5), 0.25, orient))
    # the scale as a device word against the argument
    s = 0.7
    by_arg = raw(cnt, cols, w, s, orient)
    tot, each, info = capi.dirmult_logml(dev(cnt, np.uint32), dev(w, np.float64), orient, cols, dev(np.array([s]), np.float64))
    torch.cuda.synchronize()
    assert same_bits(dict(total=tot, each=each.cpu().numpy(), cells=info.cells, norms=info.norms, nonzero=info.nonzero,
                          count=info.count, zero_weight=info.zero_weight, impossible=info.impossible), by_arg)
    # scale 1.0 on weights multiplied ahead
    assert same_bits(raw(cnt, cols, s * np.asarray(w), 1.0, orient), by_arg)
    # d_each is optional
    assert raw(cnt, cols, w, s, orient, want_each=False)["total"] == by_arg["total"]


# ---- 3. the edge rules ----

@pytest.mark.parametrize("orient", [dmo.ROWS, dmo.COLUMNS])
def test_zero_weights_and_zero_matrices(orient):
    w = np.array([0.0, 1.5, 2.0])
    ok_m, bad_m = np.array([[0, 3, 9], [0, 0, 0], [0, 1, 0]]), np.array([[1, 3, 9], [0, 1, 0], [0, 0, 2]])
    if orient == dmo.COLUMNS:
        ok_m, bad_m = ok_m.T.copy(), bad_m.T.copy()
    ok, want = raw(ok_m, 3, w, 1.0, orient), dmo.truth(ok_m, w, orient)
    assert ok["zero_weight"] == 3 and ok["impossible"] == 0 and math.isfinite(ok["total"]) and dmo.worst_ratio(ok, want) <= 1.0
    bad, want = raw(bad_m, 3, w, 1.0, orient), dmo.truth(bad_m, w, orient)
    assert bad["impossible"] == 1 and bad["total"] == -math.inf and bad["cells"] == -math.inf and math.isfinite(bad["norms"])
    assert bad["each"][0] == -math.inf and np.isfinite(bad["each"][1:]).all() and dmo.worst_ratio(bad, want) <= 1.0
    zero = raw(np.zeros((300, 70), dtype=np.uint32), 65, np.full(65 if orient == dmo.ROWS else 300, 0.3), 1.0, orient)
    assert zero["total"] == 0.0 and zero["cells"] == 0.0 and zero["norms"] == 0.0 and not zero["each"].any()
    assert zero["nonzero"] == 0 and zero["count"] == 0
    some, tot, info = dev(np.ones((1, 4)), np.uint32), capi.C.c_double(-3.0), capi.DirMultInfo()      # rows = 0 gives 0
    info.nonzero = 9
    assert capi.lib().stb_dirmult_logml(some.data_ptr(), 0, 4, 4, orient, None, 1.0, 1.0, None, None, capi.C.byref(tot),
                                        capi.C.byref(info), capi.stream_ptr()) == 0
    assert tot.value == 0.0 and info.nonzero == 0


def test_unusable_weights_fail_after_the_wait():
    cnt = np.array([[1, 2, 3], [0, 4, 0]], dtype=np.uint32)
    for w, scale, bit in ((np.array([1.0, -1.0, 2.0]), 1.0, 1), (np.array([1.0, math.nan, 2.0]), 1.0, 1),
                          (np.array([1.0, math.inf, 2.0]), 1.0, 1), (np.zeros(3), 1.0, 2),
                          (np.ones(3), dev(np.array([-2.0]), np.float64), 1), (np.ones(3), dev(np.array([math.nan]), np.float64), 1)):
        with pytest.raises(capi.StbError, match="error word 0x") as e:
            capi.dirmult_logml(dev(cnt, np.uint32), dev(w, np.float64), dmo.ROWS, 3, scale)
        assert e.value.info.error_word & bit, (w, scale)
    assert math.isfinite(capi.dirmult_logml(dev(cnt, np.uint32), dev(np.ones(3), np.float64), dmo.ROWS)[0])


def test_refusals_leave_the_outputs_untouched():
    import torch

    L, C = capi.lib(), capi.C
    cnt, w, each = dev(np.ones((4, 8)), np.uint32), dev(np.ones(8), np.float64), dev(np.full(8, 7.0), np.float64)
    sc = dev(np.array([1.0]), np.float64)
    tot, info = C.c_double(-3.0), capi.DirMultInfo()
    info.cells, info.nonzero = 5.0, 9
    p = lambda t: t.data_ptr()
    ok = dict(cnt=p(cnt), rows=4, cols=8, stride=8, flags=capi.DM_ROWS, w=p(w), w0=0.0, scale=1.0, d_scale=None, tot=C.byref(tot))
    for kw, match in ((dict(cnt=None), "required"), (dict(tot=None), "required"), (dict(cols=0), "cols=0"),
                      (dict(cols=9), "cols=9"), (dict(flags=0), "flags"), (dict(flags=3), "flags"), (dict(flags=4), "flags"),
                      (dict(flags=capi.DM_COLUMNS | 8), "flags"), (dict(w=None, w0=0.0), "w0"), (dict(w=None, w0=-1.0), "w0"),
                      (dict(w=None, w0=math.nan), "w0"), (dict(w=None, w0=math.inf), "w0"), (dict(scale=0.0), "scale"),
                      (dict(scale=-1.0), "scale"), (dict(scale=math.nan), "scale"), (dict(scale=math.inf), "scale")):
        a = dict(ok, **kw)
        rc = L.stb_dirmult_logml(a["cnt"], a["rows"], a["cols"], a["stride"], a["flags"], a["w"], a["w0"], a["scale"], a["d_scale"],
                                 p(each), a["tot"], C.byref(info), capi.stream_ptr())
        assert rc != 0 and re.search(match, capi.last_error()), (kw, capi.last_error())
    torch.cuda.synchronize()
    assert tot.value == -3.0 and info.cells == 5.0 and info.nonzero == 9 and torch.all(each == 7.0)
    # a bad scale argument is not read when the device word replaces it
    assert L.stb_dirmult_logml(p(cnt), 4, 8, 8, capi.DM_ROWS, p(w), 0.0, -1.0, p(sc), p(each), C.byref(tot), C.byref(info),
                               capi.stream_ptr()) == 0


# ---- 4. the object layer ----

I_OBJ, ROWS_OBJ = 40, 300
RANGES = {1: [0, 40], 3: [0, 10, 25, 40], None: None}


def chain(Kd, G, seed=83, sweeps=3, empty_last=False):
    """40 restaurants of Kd dishes, 30 customers each of 300 classes, after a few sweeps and a grouped step with the root
    held at 1 / Kd and alpha = 2 Kd (so alpha r_k = 2 and no h cell underflows)"""
    rng = np.random.default_rng(seed + Kd)
    I, Nc = I_OBJ, 30
    cust = rng.integers(0, Kd - 1 if empty_last else Kd, size=I * Nc).astype(np.uint32)
    cls = rng.integers(0, ROWS_OBJ, size=I * Nc).astype(np.uint32)
    n = np.stack([np.bincount(cust[i * Nc:(i + 1) * Nc].astype(np.int64), minlength=Kd) for i in range(I)]).astype(np.uint32)
    ti = capi.TableIndicators(np.full(I, Kd, dtype=np.int32), n.reshape(-1), (n > 0).astype(np.uint16).reshape(-1), None, cust)
    ti.set_classes(cls, ROWS_OBJ)
    ti.set_lik(None, ROWS_OBJ, Kd)
    if RANGES[G] is not None:
        ti.set_hgroups(np.array(RANGES[G], dtype=np.uint64))
    a, bpar = 0.3, np.full(I, 2.0)
    for it in range(sweeps):
        ti.sample_lik(0.5, 63, it)
        ti.set_hroot(np.full(Kd, 1.0 / Kd))
        ti.sample_hgroups(2.0 * Kd, 1.0, 64, it, flags=capi.HG_KEEP_ROOT)
        assert ti.sweep_dishes(a, bpar, 65, it).stuck == 0
        ti.sweep(a, bpar, 66, it)
    return ti, a, bpar


def group_counts(ti, Kd, G):
    t, _ = ti.get()
    t = t.reshape(I_OBJ, Kd).astype(np.int64)
    goff = RANGES[G] if RANGES[G] is not None else list(range(I_OBJ + 1))
    return np.stack([t[goff[g]:goff[g + 1]].sum(axis=0) for g in range(len(goff) - 1)]).astype(np.uint32), goff


def log_dir_mp(h, w):
    mp = hp._mp()
    return mp.loggamma(mp.fsum(w)) - mp.fsum(mp.loggamma(x) for x in w) + mp.fsum((x - 1) * mp.log(p) for x, p in zip(w, h))


def state_of(ti):
    n, cust = ti.get_state()
    t, T = ti.get()
    return n, cust, t, T, ti.get_h(), ti.get_hroot(), ti.class_counts()


@pytest.mark.parametrize("Kd", [5, 70])
@pytest.mark.parametrize("G", [1, 3, None])
def test_the_collapsed_joint_of_an_object(Kd, G):
    mp = hp._mp()
    ti, a, bpar = chain(Kd, G)
    try:
        info_h = ti.sample_hgroups(0.0, 1.0, 64, 9, flags=capi.HG_KEEP_ROOT)     # h for the final counts
        alpha = info_h.alpha
        before = state_of(ti)
        beta = 0.25 + (np.arange(ROWS_OBJ) % 7) / 8.0
        gamma = 0.5 + np.arange(Kd) / Kd
        tot, ci = ti.logjoint_collapsed(a, bpar, 0.0, gamma, beta, capi.CJ_INDICATORS | capi.CJ_DATA | capi.CJ_ROOT)
        after = state_of(ti)
        assert all(np.array_equal(x, y) for x, y in zip(before, after)), "the call changed the state"
        # the base: stb_tindic_logjoint's components, bit for bit
        _, _, lj = ti.logjoint(a, bpar, indicators=True, want_Li=False)
        assert (ci.pairs, ci.restaurants, ci.binom) == (lj.pairs, lj.restaurants, lj.binom) and ci.lj.base == 0.0
        assert ci.lj.impossible == 0 and ci.lj.outside == lj.outside
        # the integrated terms: the raw call on counts rebuilt on the host, bit for bit
        c, goff = group_counts(ti, Kd, G)
        root, h = before[5], before[4].reshape(I_OBJ, Kd)
        rt = raw(c, Kd, root, alpha, dmo.ROWS)
        rd = raw(before[6], Kd, beta, 1.0, dmo.COLUMNS)
        assert ci.tables == rt["total"] and ci.dm_tables.count == int(c.sum()) == int(before[3].sum())
        assert ci.data == rd["total"] and ci.dm_data.count == I_OBJ * 30
        assert (ci.dm_tables.cells, ci.dm_tables.norms, ci.dm_data.cells, ci.dm_data.norms) == (rt["cells"], rt["norms"], rd["cells"], rd["norms"])
        # tables against the uncollapsed densities at the drawn h: sum c log h + log Dir(h; alpha r) - log Dir(h; alpha r + c)
        assert (h > 0.0).all(), "an h cell underflowed"
        wm = [mp.mpf(alpha * float(r)) for r in root]                      # (alpha r_k as the kernel forms it: one product)
        want = mp.mpf(0)
        for g in range(len(goff) - 1):
            if goff[g] == goff[g + 1]:
                continue
            hg = [mp.mpf(float(x)) for x in h[goff[g]]]
            want += mp.fsum(int(cc) * mp.log(p) for cc, p in zip(c[g], hg)) + log_dir_mp(hg, wm) \
                - log_dir_mp(hg, [x + int(cc) for x, cc in zip(wm, c[g])])
        bar_t = dmo.truth(c, root, dmo.ROWS, alpha)["total"]
        print("Kd", Kd, "G", G, "tables", ci.tables, "mpmath", float(want), "bar", bar_t[1], "oracle", bar_t[0])
        assert abs(ci.tables - float(want)) <= bar_t[1] and dmo.within(ci.tables, *bar_t)
        assert dmo.within(ci.data, *dmo.truth(before[6], beta, dmo.COLUMNS)["total"])
        # the root term and the total
        R = mp.fsum(mp.mpf(float(r)) for r in root)
        gm = [mp.mpf(float(x)) for x in gamma]
        root_mp = mp.loggamma(mp.fsum(gm)) - mp.fsum(mp.loggamma(x) for x in gm) \
            + mp.fsum((x - 1) * mp.log(mp.mpf(float(r)) / R) for x, r in zip(gm, root))
        mags = float(abs(mp.loggamma(mp.fsum(gm))) + mp.fsum(abs(mp.loggamma(x)) for x in gm)
                     + mp.fsum(abs((x - 1) * mp.log(mp.mpf(float(r)) / R)) for x, r in zip(gm, root)))
        # every term to L_LGAMMA ulp (the logs and their argument r / R, formed with Kd roundings, among them), three roundings
        root_bar = U * ((hp.L_LGAMMA + 3.0) * mags + float(sum(abs(float(x) - 1.0) for x in gamma)) * (Kd + 2.0) + 16.0)
        print("root", ci.root, "mpmath", float(root_mp), "bar", root_bar)
        assert abs(ci.root - float(root_mp)) <= root_bar and ci.root_left_out == 0
        # the total: the components added in order (without the flags, data and root are exact zeros)
        only = ti.logjoint_collapsed(a, bpar, alpha, 1.0, 1.0, capi.CJ_INDICATORS)
        assert only[1].tables == ci.tables and only[1].data == 0.0 and only[1].root == 0.0
        assert math.isfinite(tot) and tot == ((only[0] + ci.data) + ci.root)
    finally:
        ti.free()


@pytest.mark.parametrize("Kd", [5, 70])
def test_the_flat_model_is_sample_hs(Kd):
    mp = hp._mp()
    ti, a, bpar = chain(Kd, None, sweeps=2)
    try:
        gamma = 0.5 + np.arange(Kd) / Kd
        ti.sample_h(gamma, 67, 0)
        t, T = ti.get()
        c = t.reshape(I_OBJ, Kd).astype(np.int64).sum(axis=0, keepdims=True).astype(np.uint32)
        h = ti.get_h().reshape(I_OBJ, Kd)
        assert (h == h[0]).all() and (h > 0.0).all()
        tot, ci = ti.logjoint_collapsed(a, bpar, gamma=gamma, flags=capi.CJ_FLAT)
        rt = raw(c, Kd, gamma, 1.0, dmo.ROWS)
        assert ci.tables == rt["total"] and ci.dm_tables.count == int(T.sum()) and ci.binom == 0.0 and ci.data == 0.0
        hm, gm = [mp.mpf(float(x)) for x in h[0]], [mp.mpf(float(x)) for x in gamma]
        want = mp.fsum(int(cc) * mp.log(p) for cc, p in zip(c[0], hm)) + log_dir_mp(hm, gm) \
            - log_dir_mp(hm, [x + int(cc) for x, cc in zip(gm, c[0])])
        bar = dmo.truth(c, gamma, dmo.ROWS)["total"]
        print("Kd", Kd, "flat tables", ci.tables, "mpmath", float(want), "bar", bar[1])
        assert abs(ci.tables - float(want)) <= bar[1]
        # a scalar gamma, and the grouped model on an object that holds no root: 1 / Kd each, scaled by alpha
        assert ti.logjoint_collapsed(a, bpar, gamma=0.5, flags=capi.CJ_FLAT)[1].tables == raw(c, Kd, 0.5, 1.0, dmo.ROWS)["total"]
    finally:
        ti.free()
    rng = np.random.default_rng(3)
    n = rng.integers(0, 6, size=(I_OBJ, Kd)).astype(np.uint32)
    fresh = capi.TableIndicators(np.full(I_OBJ, Kd, dtype=np.int32), n.reshape(-1), (n > 0).astype(np.uint16).reshape(-1))
    try:
        ci = fresh.logjoint_collapsed(0.3, np.full(I_OBJ, 2.0), alpha=3.0)[1]
        assert ci.tables == raw((n > 0).astype(np.uint32), Kd, 1.0 / Kd, 3.0, dmo.ROWS)["total"]
    finally:
        fresh.free()


def test_a_root_cell_that_underflowed_is_left_out():
    """a dish nobody sits at under a tiny gamma: the root's draw underflows to 0 there, the grouped step gives the shape
    alpha 0 + 0 the weight 0 in every group and leaves that root; the collapsed joint stays finite"""
    mp = hp._mp()
    Kd = 5
    ti, a, bpar = chain(Kd, 3, sweeps=0, empty_last=True)
    try:
        ti.sample_hgroups(4.0, 1e-5, 64, 0)
        root = ti.get_hroot()
        assert root[Kd - 1] == 0.0 and (root[:Kd - 1] > 0.0).all(), root
        h = ti.get_h().reshape(I_OBJ, Kd)
        assert (h[:, Kd - 1] == 0.0).all() and (h[:, :Kd - 1] > 0.0).all() and np.all(np.abs(h.sum(axis=1) - 1.0) <= 2.0 * U * Kd)
        gamma = np.array([0.5, 1.0, 1.5, 2.0, 0.75])
        tot, ci = ti.logjoint_collapsed(a, bpar, 4.0, gamma, 1.0, capi.CJ_ROOT)
        assert math.isfinite(tot) and ci.root_left_out == 1 and ci.dm_tables.zero_weight == 3 and ci.dm_tables.impossible == 0
        R = mp.fsum(mp.mpf(float(r)) for r in root)
        gm = [mp.mpf(float(x)) for x in gamma]
        terms = [mp.loggamma(mp.fsum(gm))] + [mp.loggamma(x) for x in gm] + \
            [(x - 1) * mp.log(mp.mpf(float(r)) / R) for x, r in zip(gm[:-1], root[:-1])]
        want = terms[0] - mp.fsum(terms[1:1 + Kd]) + mp.fsum(terms[1 + Kd:])
        bar = U * ((hp.L_LGAMMA + 3.0) * float(mp.fsum(abs(x) for x in terms)) + float(np.abs(gamma - 1.0).sum()) * (Kd + 2.0) + 16.0)
        print("root", ci.root, "mpmath", float(want), "bar", bar)
        assert abs(ci.root - float(want)) <= bar
        c, _ = group_counts(ti, Kd, 3)
        assert ci.tables == raw(c, Kd, root, 4.0, dmo.ROWS)["total"]
    finally:
        ti.free()
    # a table at a dish without weight: impossible, -inf, not NaN
    n = np.ones((2, 2), dtype=np.uint32)
    two = capi.TableIndicators(np.full(2, 2, dtype=np.int32), n.reshape(-1), np.ones(4, dtype=np.uint16))
    try:
        two.set_hroot(np.array([1.0, 5e-324]))
        tot, ci = two.logjoint_collapsed(0.3, np.full(2, 2.0), alpha=0.25)      # 0.25 x 5e-324 rounds to 0
        assert tot == -math.inf and ci.tables == -math.inf and ci.dm_tables.impossible == 2 and math.isfinite(ci.pairs + ci.restaurants)
    finally:
        two.free()


def test_the_object_refuses_and_leaves_the_state():
    L, C = capi.lib(), capi.C
    Kd = 5
    ti, a, bpar = chain(Kd, 3, sweeps=1)
    bare = capi.TableIndicators(np.full(2, 2, dtype=np.int32), np.ones(4, dtype=np.uint32), np.ones(4, dtype=np.uint16))
    odd = capi.TableIndicators(np.full(2, 2, dtype=np.int32), np.ones(4, dtype=np.uint32), np.ones(4, dtype=np.uint16), None, None, 0,
                               capi.TI_REF_ODDS)
    try:
        before = state_of(ti)
        bad_g, bad_b = np.ones(Kd), np.ones(ROWS_OBJ)
        bad_g[2], bad_b[7] = math.inf, 0.0
        for kw, match in ((dict(flags=16), "flags"), (dict(flags=capi.CJ_ROOT | capi.CJ_FLAT), "STB_CJ_ROOT"),
                          (dict(alpha=-1.0), "alpha"), (dict(alpha=math.nan), "alpha"), (dict(alpha=math.inf), "alpha"),
                          (dict(flags=capi.CJ_FLAT, gamma=0.0), "gamma0"), (dict(flags=capi.CJ_ROOT, gamma=bad_g), r"gamma\[2\]"),
                          (dict(flags=capi.CJ_DATA, beta=-1.0), "beta0"), (dict(flags=capi.CJ_DATA, beta=bad_b), r"beta\[7\]"),
                          (dict(a=1.0), "discount"), (dict(bpar=np.full(I_OBJ, -1.0)), "bpar"),
                          (dict(bpar=np.full(I_OBJ, math.nan)), "bpar")):
            args = dict(a=a, bpar=bpar, alpha=2.0, gamma=1.0, beta=1.0, flags=0)
            args.update(kw)
            with pytest.raises(capi.StbError, match=match):
                ti.logjoint_collapsed(**args)
        # gamma and beta are not looked at when they are not read
        assert math.isfinite(ti.logjoint_collapsed(a, bpar, 2.0, 0.0, -1.0)[0])
        with pytest.raises(capi.StbError, match="none yet"):
            bare.logjoint_collapsed(0.3, np.full(2, 2.0))
        with pytest.raises(capi.StbError, match="classes"):
            bare.logjoint_collapsed(0.3, np.full(2, 2.0), 1.0, flags=capi.CJ_DATA)
        bare.set_classes(np.array([0, 1, 2, 0], dtype=np.uint32), 3)
        with pytest.raises(capi.StbError, match="matrix"):
            bare.logjoint_collapsed(0.3, np.full(2, 2.0), 1.0, flags=capi.CJ_DATA)
        bare.set_lik(None, 2, 2)
        with pytest.raises(capi.StbError, match="rows"):
            bare.logjoint_collapsed(0.3, np.full(2, 2.0), 1.0, flags=capi.CJ_DATA)
        with pytest.raises(capi.StbError, match="STB_TI_REF_ODDS"):
            odd.logjoint_collapsed(0.3, np.full(2, 2.0), 1.0)
        opts, tot = capi.CJOpts(1.0, 1.0, 1.0, None, None), C.c_double(-3.0)
        bp = capi.dp(np.ascontiguousarray(bpar))
        assert L.stb_tindic_logjoint_collapsed(None, a, bp, 0, C.byref(opts), C.byref(tot), None) != 0 and "null object" in capi.last_error()
        assert L.stb_tindic_logjoint_collapsed(ti.h, a, bp, 0, None, C.byref(tot), None) != 0 and "opts" in capi.last_error()
        assert L.stb_tindic_logjoint_collapsed(ti.h, a, bp, 0, C.byref(opts), None, None) != 0 and "total" in capi.last_error()
        assert L.stb_tindic_logjoint_collapsed(ti.h, a, None, 0, C.byref(opts), C.byref(tot), None) != 0 and "bpar" in capi.last_error()
        assert tot.value == -3.0
        # a refused a or bpar leaves info as it was too
        info = capi.CJInfo()
        info.tables, info.root_left_out = 5.0, 9
        assert L.stb_tindic_logjoint_collapsed(ti.h, 1.0, bp, 0, C.byref(opts), C.byref(tot), C.byref(info)) != 0
        assert L.stb_tindic_logjoint_collapsed(ti.h, a, capi.dp(np.full(I_OBJ, -1.0)), 0, C.byref(opts), C.byref(tot), C.byref(info)) != 0
        assert tot.value == -3.0 and info.tables == 5.0 and info.root_left_out == 9
        # more dishes in a restaurant than STB_TD_MAXK: every flag combination is refused, the outputs untouched
        wide = capi.TableIndicators(np.array([1025], dtype=np.int32), np.ones(1025, dtype=np.uint32), np.ones(1025, dtype=np.uint16))
        try:
            for fl in (0, capi.CJ_FLAT, capi.CJ_ROOT, capi.CJ_INDICATORS):
                with pytest.raises(capi.StbError, match="STB_TD_MAXK"):
                    wide.logjoint_collapsed(0.3, np.full(1, 2.0), 1.0, flags=fl)
            assert L.stb_tindic_logjoint_collapsed(wide.h, 0.3, capi.dp(np.full(1, 2.0)), capi.CJ_ROOT, C.byref(opts), C.byref(tot),
                                                   C.byref(info)) != 0 and "STB_TD_MAXK" in capi.last_error()
            assert tot.value == -3.0 and info.tables == 5.0 and info.root_left_out == 9
        finally:
            wide.free()
        assert all(np.array_equal(x, y) for x, y in zip(before, state_of(ti)))
        # the concentrations where they live
        ti.set_bpar(bpar)
        assert ti.logjoint_collapsed(a, capi.BPAR_RESIDENT, 2.0)[0] == ti.logjoint_collapsed(a, bpar, 2.0)[0]
    finally:
        ti.free()
        bare.free()
        odd.free()


# ---- 5. the example ----

EXE = os.path.join(ROOT, "examples", "bin", "pyp_resample")


def test_example_prints_the_collapsed_joint():
    assert os.path.exists(EXE), "examples/bin/pyp_resample not built (make -C libstb_amd/csrc)"
    p = subprocess.run([EXE, "-J", "8", "-n", "400", "-c", "6", "-s", "5", "-d", "-z", "-w", "-H", "4", "-C"], capture_output=True,
                       text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = re.findall(r"^iteration (\d+): collapsed log joint (\S+) \(pairs (\S+), restaurants (\S+), indicators (\S+), tables (\S+), "
                      r"data (\S+), root (\S+)\)$", p.stdout, re.M)
    assert [int(r[0]) for r in rows] == list(range(6)), p.stdout[-2000:]
    for r in rows:
        vals = [float(x) for x in r[1:]]
        assert all(math.isfinite(v) for v in vals) and abs(vals[0] - sum(vals[1:])) <= 1e-6 * abs(vals[0])
    assert subprocess.run([EXE, "-d", "-z", "-C"], capture_output=True, text=True, timeout=60).returncode == 2
