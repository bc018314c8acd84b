"""Base weights per group of restaurants under a shared root, drawn on the device (libstb_amd/csrc/hgroups.hip;
include/stb_hip.h stb_sample_hgroups): the step against the numpy replay (tests/hh_oracle.py), the row sums, the anchors
to stb_tindic_sample_h and stb_sample_bgroups, launch geometries, the law, the object layer and examples/pyp_resample -H."""
import hashlib
import json
import math
import os
import re
import struct
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import hb_oracle as hbo
import hh_oracle as hho
import hq_oracle as hqo
from libstb_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def dev(x, dtype):
    import torch

    a = np.ascontiguousarray(x, dtype=dtype)
    view = {np.uint16: np.int16, np.uint32: np.int32, np.uint64: np.int64}.get(dtype)
    return torch.as_tensor(a.view(view) if view else a, device="cuda")


def koff_of(K):
    return np.concatenate([[0], np.cumsum(np.asarray(K, dtype=np.int64))])


def device_step(c, **kw):
    """the raw call on a case dict (hh_oracle.case); kw overrides its entries.  Returns dict of numpy arrays + info"""
    import torch

    c = dict(c, **kw)
    root = dev(c["root"], np.float64)
    goff = None if c["goff"] is None else dev(c["goff"], np.uint64)
    h, out, info = capi.sample_hgroups(dev(koff_of(c["K"]), np.uint64), dev(c["t"], np.uint16), c["Kmax"], root, c["alpha"],
                                       c["gamma"], c["seed"], c["sweep"], goff=goff, flags=c["flags"], shape=c["shape"],
                                       scale=c["scale"])
    torch.cuda.synchronize()
    return dict(h=h.cpu().numpy(), root=root.cpu().numpy(), hgrp=out["hgrp"].cpu().numpy(),
                c=out["c"].cpu().numpy().view(np.uint32).astype(np.int64), m=out["m"].cpu().numpy().view(np.uint32).astype(np.int64),
                alpha=info.alpha, tables=info.tables, aux_tables=info.aux_tables)


BITS = os.path.join(ROOT, "tests", "golden", "hstep_bits.json")


def step_bits(h, root, rows, c, m, alpha, tables, aux_tables):
    """what tests/golden/hstep_bits.json keeps of a step (tools/record_hstep_bits.py): SHA-256 of the arrays' bytes (rows, c
    and m a list a level; the counts as uint32), the concentrations' bit patterns, the totals"""
    def sha(x, dtype):
        return hashlib.sha256(np.ascontiguousarray(x, dtype=dtype).tobytes()).hexdigest()

    return dict(h=sha(h, np.float64), root=sha(root, np.float64), rows=[sha(x, np.float64) for x in rows],
                c=[sha(x, np.uint32) for x in c], m=[sha(x, np.uint32) for x in m],
                alpha=[struct.pack(">d", float(a)).hex() for a in alpha], tables=[int(x) for x in tables],
                aux_tables=[int(x) for x in aux_tables])


def bits_of(got):
    return step_bits(got["h"], got["root"], [got["hgrp"]], [got["c"]], [got["m"]], [got["alpha"]], [got["tables"]],
                     [got["aux_tables"]])


@lru_cache(maxsize=None)
def recorded():
    with open(BITS) as f:
        return json.load(f)


@lru_cache(maxsize=None)
def stepped(name):
    """(the case, the device's step, the replay fed the device's own r' and alpha' where the step draws them)"""
    c = hho.case(name)
    got = device_step(c)
    fed = {}
    if not c["flags"] & hho.KEEP_ROOT:
        fed["root_new"] = got["root"]
    if c["flags"] & hho.SAMPLE_ALPHA:
        fed["alpha_new"] = got["alpha"]
    want = hho.replay_case(name, **fed)
    return c, got, want


def assert_replayed(got, want, what):
    """test_gpu_tlik's standing bar: 1e-10 relative where the replay's value is >= 1e-280, 1e-290 absolute below; no cell
    left out"""
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


# ---- 1. the step against the replay ----

@pytest.mark.parametrize("name", list(hho.CASES))
def test_the_step_equals_the_replay(name):
    c, got, want = stepped(name)
    assert np.array_equal(got["c"], want["c"]), "c"
    assert np.array_equal(got["m"], want["m"]), "m"
    assert got["tables"] == want["tables"] and got["aux_tables"] == want["aux_tables"]
    if c["flags"] & hho.KEEP_ROOT:
        assert np.array_equal(got["root"], c["root"])
    else:
        assert_replayed(got["root"], want["root"], name + " root")
    if c["flags"] & hho.SAMPLE_ALPHA:
        print(name, "alpha'", got["alpha"], "replay", want["alpha"])
        assert abs(got["alpha"] - want["alpha"]) <= 1e-10 * want["alpha"] and got["alpha"] != c["alpha"]
    else:
        assert got["alpha"] == c["alpha"]
    assert_replayed(got["hgrp"], want["hgrp"], name + " hgrp")
    assert_replayed(got["h"], want["h"], name + " h")


@pytest.mark.parametrize("name", list(hho.CASES))
def test_the_step_keeps_the_recorded_bits(name):
    """every output bit is what the library gave before the grouped step became the one-level tree"""
    _, got, _ = stepped(name)
    assert bits_of(got) == recorded()["hgroups"][name]


# ---- 2. row sums, and the pairs ----

@pytest.mark.parametrize("name", list(hho.CASES))
def test_rows_sum_to_one_and_pairs_hold_their_groups_weights(name):
    c, got, want = stepped(name)
    Kmax = c["Kmax"]
    assert np.all(np.isfinite(got["hgrp"])) and got["hgrp"].min() >= 0.0 and got["hgrp"].max() <= 1.0
    worst = max(abs(math.fsum(row) - 1.0) for row in got["hgrp"])
    print(name, "largest |row sum - 1|", worst, "bar", 2.0 * U * Kmax)
    assert worst <= 2.0 * U * Kmax
    if not c["flags"] & hho.KEEP_ROOT:
        assert abs(math.fsum(got["root"]) - 1.0) <= 2.0 * U * Kmax
    assert np.array_equal(got["h"], hho.spread(c["K"], want["owner"], got["hgrp"]))


# ---- 3. anchors, bit for bit ----

def test_one_group_with_the_root_kept_is_sample_h():
    c = hho.case("ragged_keep")
    K, t = c["K"], c["t"]
    gamma = c["gamma"]
    got = device_step(c, goff=np.array([0, len(K)], dtype=np.uint64), alpha=1.0, root=gamma, flags=hho.KEEP_ROOT)
    ti = capi.TableIndicators(K, t.astype(np.uint32), t)
    try:
        ti.sample_h(gamma, c["seed"], c["sweep"])
        h = ti.get_h()
    finally:
        ti.free()
    assert np.array_equal(got["h"], h)
    assert got["hgrp"].shape == (1, c["Kmax"]) and got["m"].sum() == got["aux_tables"] and got["c"].sum() == got["tables"]


def test_the_concentration_is_sample_bgroups():
    import torch

    c, got, _ = stepped("ragged_full")
    C_g, M_g = got["c"].sum(axis=1), got["m"].sum(axis=1)
    G = len(C_g)
    bd = dev(np.full(G, c["alpha"]), np.float64)
    bg, _, _, _, info = capi.sample_bgroups(0.0, c["shape"], c["scale"], dev(M_g, np.uint32), bd, (c["seed"] ^ hho.SALT_A) & (2 ** 64 - 1),
                                            c["sweep"], N=dev(C_g, np.uint32), goff=dev(np.array([0, G]), np.uint64))
    torch.cuda.synchronize()
    assert info.b == got["alpha"] and float(bg.cpu().numpy()[0]) == got["alpha"]


# ---- 4. geometry ----

def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("h", "root", "hgrp", "c", "m")) and a["alpha"] == b["alpha"]


@pytest.mark.parametrize("name", ["ragged_full", "k1024_alpha", "each_keep"])
def test_the_bits_do_not_depend_on_the_launch(name, monkeypatch):
    c, got, _ = stepped(name)
    for waves, form in ((1, "lane"), (2, "wave"), (4, "lane"), (8, "wave"), (8, ""), (4, "wave")):
        monkeypatch.setenv("STB_HGROUPS_WAVES", str(waves))
        monkeypatch.setenv("STB_HGROUPS_FORM", form)
        assert same_bits(device_step(c), got), (waves, form)


def test_ranges_of_one_restaurant_are_no_ranges():
    c, got, _ = stepped("each_keep")
    assert c["goff"] is None
    assert same_bits(device_step(c, goff=np.arange(len(c["K"]) + 1, dtype=np.uint64)), got)


# ---- 5. the law on the device: the root's chain ----

def test_the_roots_chain_keeps_its_posterior():
    K, n, t, goff = hho.law_object()
    ti = capi.TableIndicators(K, n, t)
    try:
        ti.set_hgroups(goff)

        def step(r, s):
            ti.sample_hgroups(hho.LAW_ALPHA, hho.LAW_GAMMA, hho.LAW_SEED, s)
            return ti.get_hroot()

        r0 = hho.root_chain(hho.LAW_SEED, step_fn=step)
    finally:
        ti.free()
    assert len(r0) == hho.LAW_STEPS // hho.LAW_THIN and np.all((r0 > 0) & (r0 < 1))
    pv = hho.law_pvalue(r0)
    print("KS p-value of r_0 on the device", pv, "mean", r0.mean())
    assert pv > 1e-3


# ---- 6. the law on the device: the groups' draw ----

def test_the_law_of_the_group_draw():
    G = 4096
    K = np.full(G, 4, dtype=np.int32)
    base = np.array([3, 0, 17, 1], dtype=np.uint16)
    root, alpha = np.array([0.9, 0.6, 1.5, 2.0]), 1.25
    c = dict(K=K, t=np.tile(base, G), goff=None, root=root, alpha=alpha, gamma=1.0, flags=hho.KEEP_ROOT, seed=41, sweep=0,
             shape=1.0, scale=1.0, Kmax=4)
    got = device_step(c)
    shape = alpha * root + base
    assert np.all(got["hgrp"] > 0.0) and np.array_equal(got["c"], np.tile(base, (G, 1)))
    for k in range(4):  # h_gk ~ Beta(shape_k, rest), and moment_check takes -log of such a variable
        ok, text = hqo.moment_check(-np.log(got["hgrp"][:, k]), float(shape[k]), float(shape.sum() - shape[k]))
        print("dish", k, text)
        assert ok, text
    # it can fail: the same draws against the shape without its tables
    ok, text = hqo.moment_check(-np.log(got["hgrp"][:, 0]), float(alpha * root[0]), float(shape.sum() - shape[0]))
    assert not ok, text


# ---- 7. the object ----

def small_chain(seed=71):
    """64 restaurants of 6 dishes in 4 groups (one empty), 3 classes"""
    rng = np.random.default_rng(seed)
    I, Kd, Nc, rows = 64, 6, 30, 3
    cust = rng.integers(0, Kd, size=I * Nc).astype(np.uint32)
    cls = rng.integers(0, rows, size=I * Nc).astype(np.uint32)
    n = np.stack([np.bincount(cust[i * Nc:(i + 1) * Nc].astype(np.int64), minlength=Kd) for i in range(I)]).astype(np.uint32)
    t = (n > 0).astype(np.uint16)
    ti = capi.TableIndicators(np.full(I, Kd, dtype=np.int32), n.reshape(-1), t.reshape(-1), None, cust)
    ti.set_classes(cls, rows)
    ti.set_lik(None, rows, Kd)
    ti.set_hgroups(np.array([0, 10, 10, 40, 64], dtype=np.uint64))
    return ti, I, Kd


def run_chain():
    ti, I, Kd = small_chain()
    a, bpar = 0.3, np.full(I, 2.0)
    try:
        alphas = []
        for it in range(30):
            ti.sample_lik(0.5, 63, it)
            info = ti.sample_hgroups(1.5 if it == 0 else 0.0, 1.0, 64, it, flags=capi.HG_SAMPLE_ALPHA, shape=1.1, scale=20.0)
            alphas.append(info.alpha)
            di = ti.sweep_dishes(a, bpar, 65, it)
            ti.sweep(a, bpar, 66, it)
            assert di.stuck + di.skipped == 0 and info.tables >= info.aux_tables >= Kd
        h = ti.get_h().reshape(I, Kd)
        lj = ti.logjoint(a, bpar, True)[0]
        theta = ti.predict(a, bpar)
        t, T = ti.get()
        return h, ti.get_hroot(), np.array(alphas), lj, theta, t
    finally:
        ti.free()


def test_the_object_chain_repeats_itself():
    h1, r1, al1, lj1, th1, t1 = run_chain()
    h2, r2, al2, lj2, th2, t2 = run_chain()
    assert np.array_equal(h1, h2) and np.array_equal(r1, r2) and np.array_equal(al1, al2) and lj1 == lj2 and np.array_equal(t1, t2)
    assert math.isfinite(lj1) and np.all(np.isfinite(al1)) and np.all(al1 > 0) and len(set(al1)) == 30
    assert np.all(np.isfinite(th1)) and np.array_equal(th1, th2) and np.all(np.abs(th1.sum(axis=1) - 1.0) < 1e-12)
    # one h a group: restaurants 0..9, 10..39, 40..63
    for lo, hi in ((0, 10), (10, 40), (40, 64)):
        assert np.all(h1[lo:hi] == h1[lo]) and abs(math.fsum(h1[lo]) - 1.0) <= 2.0 * U * h1.shape[1]
    assert not np.array_equal(h1[0], h1[10]) and not np.array_equal(h1[10], h1[40])
    assert abs(math.fsum(r1) - 1.0) <= 2.0 * U * len(r1)


def test_refusals_leave_the_state_and_failures_block_the_dish_sweep():
    L = capi.lib()
    ti, I, Kd = small_chain()
    odd = capi.TableIndicators(np.full(2, 2, dtype=np.int32), np.ones(4, dtype=np.uint32), np.ones(4, dtype=np.uint16), None, None, 0,
                               capi.TI_REF_ODDS)
    a, bpar = 0.3, np.full(I, 2.0)
    try:
        with pytest.raises(capi.StbError, match="none yet"):
            ti.sample_hgroups(0.0, 1.0, 1, 0)                       # no concentration to take up
        ti.set_hroot(0.2 + np.arange(Kd) / 10.0)
        info = ti.sample_hgroups(2.0, 1.0, 5, 0, flags=capi.HG_SAMPLE_ALPHA, shape=2.0, scale=3.0)
        before = (ti.get_h(), ti.get_hroot())
        alpha = info.alpha
        bad_g = np.full(Kd, 1.0)
        bad_g[Kd - 1] = math.inf
        both = capi.HG_SAMPLE_ALPHA
        for kw, match in ((dict(alpha=-1.0), "alpha"), (dict(alpha=math.nan), "alpha"), (dict(alpha=math.inf), "alpha"),
                          (dict(gamma=0.0), "gamma0"), (dict(gamma=bad_g), r"gamma\[%d\]" % (Kd - 1)),
                          (dict(flags=both, shape=0.0), "shape"), (dict(flags=both, shape=math.nan), "shape"),
                          (dict(flags=both, scale=-1.0), "scale"), (dict(flags=both, scale=math.inf), "scale"),
                          (dict(flags=4), "flags")):
            args = dict(alpha=2.0, gamma=1.0, seed=1, sweep=0, flags=0, shape=1.0, scale=1.0)
            args.update(kw)
            with pytest.raises(capi.StbError, match=match):
                ti.sample_hgroups(**args)
        for goff, match in (([0, 10, 63], "ranges run"), ([1, 10, 64], "ranges run"), ([0, 40, 10, 64], "goff")):
            with pytest.raises(capi.StbError, match=match):
                ti.set_hgroups(np.array(goff, dtype=np.uint64))
        for root in (np.zeros(Kd), np.full(Kd, math.nan), -np.ones(Kd)):
            with pytest.raises(capi.StbError, match="root"):
                ti.set_hroot(root)
        with pytest.raises(capi.StbError, match="STB_TI_REF_ODDS"):
            odd.sample_hgroups(1.0, 1.0, 1, 0)
        assert L.stb_tindic_sample_hgroups(ti.h, None, 1, 0, None) != 0 and "opts" in capi.last_error()
        assert np.array_equal(ti.get_h(), before[0]) and np.array_equal(ti.get_hroot(), before[1])
        # ranges and alpha as they were: the step the object would have taken anyway, against a twin that saw no refusal
        twin, _, _ = small_chain()
        try:
            twin.set_hroot(0.2 + np.arange(Kd) / 10.0)
            twin.sample_hgroups(2.0, 1.0, 5, 0, flags=capi.HG_SAMPLE_ALPHA, shape=2.0, scale=3.0)
            for o in (ti, twin):
                i2 = o.sample_hgroups(0.0, 1.0, 6, 1)
                assert i2.alpha == alpha
            assert np.array_equal(ti.get_h(), twin.get_h()) and np.array_equal(ti.get_hroot(), twin.get_hroot())
        finally:
            twin.free()
        # the raw layer's refusals write nothing
        import torch

        koff, td = dev(koff_of(np.full(I, Kd)), np.uint64), dev(np.ones(I * Kd), np.uint16)
        root, h = dev(np.full(Kd, 0.5), np.float64), dev(np.full(I * Kd, 7.0), np.float64)
        goff = dev(np.array([0, 10, 64]), np.uint64)
        badg = dev(np.array([0, 70, 64]), np.uint64)
        shortg = dev(np.array([0, 10, 63]), np.uint64)
        keep, opts = capi.hgroups_opts(1.0, 1.0)
        _, bad_alpha = capi.hgroups_opts(0.0, 1.0)
        sp, ob = capi.stream_ptr(), capi.C.byref(opts)
        for args, match in (((I, None, td.data_ptr(), Kd, 2, goff.data_ptr(), ob, root.data_ptr(), h.data_ptr()), "required"),
                            ((I, koff.data_ptr(), None, Kd, 2, goff.data_ptr(), ob, root.data_ptr(), h.data_ptr()), "required"),
                            ((I, koff.data_ptr(), td.data_ptr(), Kd, 2, goff.data_ptr(), ob, None, h.data_ptr()), "required"),
                            ((I, koff.data_ptr(), td.data_ptr(), Kd, 2, goff.data_ptr(), ob, root.data_ptr(), None), "required"),
                            ((I, koff.data_ptr(), td.data_ptr(), Kd, 2, goff.data_ptr(), None, root.data_ptr(), h.data_ptr()), "opts"),
                            ((I, koff.data_ptr(), td.data_ptr(), 0, 2, goff.data_ptr(), ob, root.data_ptr(), h.data_ptr()), "Kmax=0"),
                            ((I, koff.data_ptr(), td.data_ptr(), 1025, 2, goff.data_ptr(), ob, root.data_ptr(), h.data_ptr()), "Kmax=1025"),
                            ((I, koff.data_ptr(), td.data_ptr(), Kd, 0, goff.data_ptr(), ob, root.data_ptr(), h.data_ptr()), "G=0"),
                            ((I, koff.data_ptr(), td.data_ptr(), Kd, 2, None, ob, root.data_ptr(), h.data_ptr()), "its own group"),
                            ((I, koff.data_ptr(), td.data_ptr(), Kd, 2, badg.data_ptr(), ob, root.data_ptr(), h.data_ptr()), "goff"),
                            ((I, koff.data_ptr(), td.data_ptr(), Kd, 2, shortg.data_ptr(), ob, root.data_ptr(), h.data_ptr()), "ranges run"),
                            ((I, koff.data_ptr(), td.data_ptr(), Kd, 2, goff.data_ptr(), capi.C.byref(bad_alpha), root.data_ptr(),
                              h.data_ptr()), "alpha")):
            assert L.stb_sample_hgroups(*args, None, None, None, 1, 0, sp, None) != 0, match
            assert re.search(match, capi.last_error()), (match, capi.last_error())
        torch.cuda.synchronize()
        assert torch.all(h == 7.0) and torch.all(root == 0.5)
        # a root so small that alpha r_k + 0 is exactly 0 is no failure: the coordinate is 0 where the group has no table
        # and a draw of shape c where it has.  A failure after the wait: a root so large that alpha r_k is infinite.  h is then
        # undefined and the dish sweep refused, as after a failed sample_h, until a draw succeeds
        cust = np.array([0, 0, 2, 0, 1], dtype=np.uint32)          # two restaurants of three dishes; c_01 = c_12 = 0
        n2 = np.array([2, 0, 1, 1, 1, 0], dtype=np.uint32)
        two = capi.TableIndicators(np.full(2, 3, dtype=np.int32), n2, (n2 > 0).astype(np.uint16), None, cust)
        try:
            two.set_hroot(np.array([0.3, 5e-324, 0.3]))
            two.sample_hgroups(0.25, 1.0, 9, 0, flags=capi.HG_KEEP_ROOT)
            h2 = two.get_h().reshape(2, 3)
            assert h2[0, 1] == 0.0 and h2[1, 1] > 0.0 and np.all(h2[:, [0, 2]] > 0.0)
            assert np.all(np.abs(h2.sum(axis=1) - 1.0) <= 6.0 * 2.0 ** -53)
            two.set_hroot(np.array([0.3, 1e308, 0.3]))
            with pytest.raises(capi.StbError, match="error word 0x") as e:
                two.sample_hgroups(1e10, 1.0, 9, 0, flags=capi.HG_KEEP_ROOT)
            assert e.value.info.error_word & 4
            with pytest.raises(capi.StbError, match="undefined"):
                two.sweep_dishes(a, np.full(2, 2.0), 65, 0)
            two.set_hroot(None)
            two.sample_hgroups(0.25, 1.0, 9, 0)
            assert two.sweep_dishes(a, np.full(2, 2.0), 65, 0).stuck == 0
        finally:
            two.free()
    finally:
        ti.free()
        odd.free()


# ---- 8. the example ----

EXE = os.path.join(ROOT, "examples", "bin", "pyp_resample")
ARGS = ["-J", "8", "-n", "400", "-c", "6", "-s", "5", "-d", "-z", "-L", "-w"]


def test_example_with_grouped_base_weights():
    assert os.path.exists(EXE), "examples/bin/pyp_resample not built (make -C libstb_amd/csrc)"
    p = subprocess.run([EXE] + ARGS + ["-H", "4"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = re.findall(r"^iteration (\d+): base weights in 4 groups, alpha (\S+), (\d+) tables, (\d+) auxiliary, largest \|sum h - 1\| (\S+)$",
                      p.stdout, re.M)
    assert [int(r[0]) for r in rows] == list(range(6)), p.stdout
    for _, alpha, tables, aux, worst in rows:
        assert math.isfinite(float(alpha)) and float(alpha) > 0 and int(tables) >= int(aux) > 0
        assert 0.0 <= float(worst) <= 2.0 * U * 50 * 2           # (the example adds the 50 weights once more itself)
    joint = re.findall(r"^iteration \d+: log joint (\S+) .* complete (\S+) a=", p.stdout, re.M)
    assert len(joint) == 6 and all(math.isfinite(float(x)) for pair in joint for x in pair)
    # without -H the lines of the grouped step are absent and the rest is what -w printed before
    q = subprocess.run([EXE] + ARGS, capture_output=True, text=True, timeout=60)
    assert q.returncode == 0 and "base weights in" not in q.stdout and len(re.findall(r"^iteration \d+: log joint", q.stdout, re.M)) == 6
    # -H without -d -z -w is refused
    assert subprocess.run([EXE, "-d", "-z", "-H", "4"], capture_output=True, text=True, timeout=60).returncode == 2
