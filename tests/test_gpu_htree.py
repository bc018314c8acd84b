"""Base weights on a tree of nested groups, drawn on the device (libstb_amd/csrc/htree.hip; include/stb_hip.h
stb_sample_htree): one level against stb_sample_hgroups bit for bit, the step against the numpy replay (tests/ht_oracle.py),
launch geometries, the law of the chain and of the downward draw, the object layer and examples/pyp_resample -T."""
import math
import os
import re
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import hb_oracle as hbo
import hh_oracle as hho
import ht_oracle as hto
import test_gpu_hgroups as tgh
from libstb_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
dev, koff_of, assert_replayed = tgh.dev, tgh.koff_of, tgh.assert_replayed


def u32(x):
    return x.cpu().numpy().view(np.uint32).astype(np.int64)


def device_step(c, **kw):
    """the raw call on a case dict (ht_oracle.case); kw overrides its entries.  Returns dict of numpy arrays, lists a level"""
    import torch

    c = dict(c, **kw)
    L = len(c["offs"])
    G = [len(o) - 1 for o in c["offs"]]
    root = dev(c["root"], np.float64)
    hnode = [None] + [dev(c["rows"][l], np.float64) for l in range(1, L)]
    off = [dev(o, np.uint64) for o in c["offs"]]
    h, out, info = capi.sample_htree(dev(koff_of(c["K"]), np.uint64), dev(c["t"], np.uint16), c["Kmax"], G, off, root, hnode,
                                     c["alpha"], c["gamma"], c["seed"], c["sweep"], flags=c["flags"], shape=c["shape"],
                                     scale=c["scale"])
    torch.cuda.synchronize()
    return dict(h=h.cpu().numpy(), root=root.cpu().numpy(), rows=[r.cpu().numpy() for r in out["rows"]],
                c=[u32(x) for x in out["c"]], m=[u32(x) for x in out["m"]], alpha=list(info.alpha)[:L],
                tables=list(info.tables)[:L], aux_tables=list(info.aux_tables)[:L], rest=(list(info.alpha)[L:], list(info.tables)[L:]))


@lru_cache(maxsize=None)
def stepped(name, flags):
    """(the case, the device's step, the replay fed the device's own r', alpha' and upper rows)"""
    c = hto.case(name, flags)
    got = device_step(c)
    fed = dict(rows_new=[None] + got["rows"][1:])
    if not flags & hto.KEEP_ROOT:
        fed["root_new"] = got["root"]
    if flags & hto.SAMPLE_ALPHA:
        fed["alpha_new"] = got["alpha"]
    return c, got, hto.replay_case(name, flags, **fed)


# ---- 1. one level is stb_sample_hgroups, bit for bit ----

@pytest.mark.parametrize("name", ["ragged_full", "k1024_alpha"])
def test_one_level_is_sample_hgroups(name):
    c = hho.case(name)
    want = tgh.device_step(c)
    got = device_step(dict(c, offs=[c["goff"]], rows=[None], alpha=[c["alpha"]]))
    for key in ("h", "root"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["rows"][0], want["hgrp"]) and np.array_equal(got["c"][0], want["c"])
    assert np.array_equal(got["m"][0], want["m"])
    assert got["alpha"] == [want["alpha"]] and got["tables"] == [want["tables"]] and got["aux_tables"] == [want["aux_tables"]]
    assert all(math.isnan(a) for a in got["rest"][0]) and not any(got["rest"][1])


# ---- 2. the step against the replay ----

@pytest.mark.parametrize("name,flags", hto.STEPS)
def test_the_step_equals_the_replay(name, flags):
    c, got, want = stepped(name, flags)
    L, Kmax = len(c["G"]), c["Kmax"]
    for l in range(L):
        assert np.array_equal(got["c"][l], want["c"][l]), ("c", l)
        assert np.array_equal(got["m"][l], want["m"][l]), ("m", l)
    assert got["tables"] == want["tables"] and got["aux_tables"] == want["aux_tables"]
    if flags & hto.KEEP_ROOT:
        assert np.array_equal(got["root"], c["root"])
    else:
        assert_replayed(got["root"], want["root"], name + " root")
        assert abs(math.fsum(got["root"]) - 1.0) <= 2.0 * U * Kmax
    for l in range(L):
        if flags & hto.SAMPLE_ALPHA:
            print(name, "level", l + 1, "alpha'", got["alpha"][l], "replay", want["alpha"][l])
            assert abs(got["alpha"][l] - want["alpha"][l]) <= 1e-10 * want["alpha"][l] and got["alpha"][l] != c["alpha"][l]
        else:
            assert got["alpha"][l] == c["alpha"][l]
        assert_replayed(got["rows"][l], want["rows"][l], "%s rows of level %d" % (name, l + 1))
        assert np.all(np.isfinite(got["rows"][l])) and got["rows"][l].min() >= 0.0 and got["rows"][l].max() <= 1.0
        worst = max(abs(math.fsum(row) - 1.0) for row in got["rows"][l])
        print(name, "level", l + 1, "largest |row sum - 1|", worst, "bar", 2.0 * U * Kmax)
        assert worst <= 2.0 * U * Kmax
    assert_replayed(got["h"], want["h"], name + " h")
    assert np.array_equal(got["h"], hho.spread(c["K"], want["owner"], got["rows"][0]))


def bits_of(got):
    return tgh.step_bits(got["h"], got["root"], got["rows"], got["c"], got["m"], got["alpha"], got["tables"], got["aux_tables"])


@pytest.mark.parametrize("name,flags", hto.STEPS)
def test_the_step_keeps_the_recorded_bits(name, flags):
    """every output bit is what the library gave before the grouped step became the one-level tree"""
    _, got, _ = stepped(name, flags)
    assert bits_of(got) == tgh.recorded()["htree"]["%s/%d" % (name, flags)]


# ---- 3. geometry ----

def same_bits(a, b):
    return (all(np.array_equal(a[k], b[k]) for k in ("h", "root")) and a["alpha"] == b["alpha"] and a["tables"] == b["tables"] and
            a["aux_tables"] == b["aux_tables"] and
            all(np.array_equal(x, y) for k in ("rows", "c", "m") for x, y in zip(a[k], b[k])))


@pytest.mark.parametrize("name", ["three_k70", "few_rows"])
def test_the_bits_do_not_depend_on_the_launch(name, monkeypatch):
    c, got, _ = stepped(name, hto.SAMPLE_ALPHA)
    for waves in (1, 2, 4, 8):
        for form in ("lane", "wave"):
            monkeypatch.setenv("STB_HTREE_WAVES", str(waves))
            monkeypatch.setenv("STB_HTREE_FORM", form)
            assert same_bits(device_step(c), got), (waves, form)


# ---- 4. the law on the device ----

def test_the_chain_keeps_both_marginals():
    import torch

    K, _, t = hto.law_object()
    koff, td = dev(koff_of(K), np.uint64), dev(t, np.uint16)
    off = [dev(o, np.uint64) for o in hto.LAW_OFFS]
    root, rows2 = dev(np.array([0.5, 0.5]), np.float64), dev(np.full((2, 2), 0.5), np.float64)

    def step(r, rows, s):      # (the state stays on the device: r and rows are what the call before left there)
        capi.sample_htree(koff, td, 2, [3, 2], off, root, [None, rows2], hto.LAW_ALPHA, hto.LAW_GAMMA, hto.LAW_SEED, s, want=())
        both = torch.cat([root, rows2.reshape(-1)]).cpu().numpy()
        return both[:2], both[2:].reshape(2, 2)

    kept = hto.law_chain(hto.LAW_SEED, step_fn=step)
    assert len(kept) == hto.LAW_STEPS // hto.LAW_THIN and np.all((kept > 0) & (kept < 1))
    p_root, p_node = hto.law_pvalues(kept)
    print("KS p-values on the device: r_0", p_root, "h_A0", p_node, "means", kept.mean(axis=0))
    assert p_root > 1e-3 and p_node > 1e-3


def beta_cdf(a, b, v, points=200001):
    """the CDF of Beta(a, b) at v by quadrature in y = logit h (the Jacobian h (1 - h) turns a - 1, b - 1 into a, b)"""
    y = np.linspace(-300.0, 300.0, points)
    dens = np.exp(-a * np.logaddexp(0.0, -y) - b * np.logaddexp(0.0, y))
    cdf = np.concatenate([[0.0], np.cumsum(0.5 * (dens[1:] + dens[:-1]) * np.diff(y))])
    v = np.asarray(v, dtype=np.float64)
    return np.interp(np.log(v) - np.log1p(-v), y, cdf / cdf[-1])


def test_childless_nodes_draw_from_the_prior_given_the_new_root():
    # one restaurant, one level-1 node, 4097 level-2 nodes of which the last has the child
    n2 = 4096
    K, t = np.array([2], dtype=np.int32), np.array([3, 5], dtype=np.uint16)
    offs = [np.array([0, 1], dtype=np.uint64), np.concatenate([np.zeros(n2 + 1), [1]]).astype(np.uint64)]
    alpha2 = 3.0
    c = dict(K=K, t=t, offs=offs, root=np.array([0.4, 0.6]), rows=[None, np.full((n2 + 1, 2), 0.5)], alpha=[2.0, alpha2],
             gamma=np.array([1.5, 2.5]), flags=0, seed=46, sweep=0, shape=1.0, scale=1.0, Kmax=2)
    got = device_step(c)
    r0 = float(got["root"][0])
    assert got["c"][1][:n2].sum() == 0 and got["c"][1][n2].sum() == got["aux_tables"][0] >= 2
    first = got["rows"][1][:n2, 0]
    assert np.all((first > 0) & (first < 1))
    pv = hbo.ks_pvalue(beta_cdf(alpha2 * r0, alpha2 * (1.0 - r0), first))
    print("r'_0", r0, "KS p-value of 4096 childless rows", pv, "mean", first.mean())
    assert pv > 1e-3
    # it can fail: the same draws against the root the call was given (this seed's r'_0 is 0.7285 in the replay)
    want = hto.replay(K, t, offs, c["root"], c["rows"], c["alpha"], c["gamma"], c["seed"], c["sweep"], Kmax=2)
    assert abs(r0 - want["root"][0]) <= 1e-10 * want["root"][0] and abs(r0 - 0.4) > 0.3
    assert hbo.ks_pvalue(beta_cdf(alpha2 * 0.4, alpha2 * 0.6, first)) < 1e-9


# ---- 5. the object ----

TREE = [np.array([0, 10, 10, 40, 64], dtype=np.uint64), np.array([0, 2, 2, 4], dtype=np.uint64)]


def small_tree():
    ti, I, Kd = tgh.small_chain()
    ti.set_htree(TREE)
    return ti, I, Kd


def run_chain():
    ti, I, Kd = small_tree()
    a, bpar = 0.3, np.full(I, 2.0)
    try:
        alphas = []
        for it in range(20):
            ti.sample_lik(0.5, 63, it)
            info = ti.sample_htree([1.5, 2.5] if it == 0 else None, 1.0, 64, it, flags=capi.HT_SAMPLE_ALPHA, shape=1.1, scale=20.0)
            alphas.append(list(info.alpha)[:2])
            di = ti.sweep_dishes(a, bpar, 65, it)
            ti.sweep(a, bpar, 66, it)
            assert di.stuck + di.skipped == 0 and info.tables[0] >= info.aux_tables[0] == info.tables[1] >= info.aux_tables[1] >= Kd
        h = ti.get_h().reshape(I, Kd)
        return h, ti.get_hroot(), np.array(alphas), ti.logjoint(a, bpar, True)[0], ti.get_htree_level(1), ti.get_htree_level(2), ti.get()[0]
    finally:
        ti.free()


def test_the_object_chain_repeats_itself():
    one, two = run_chain(), run_chain()
    for x, y in zip(one, two):
        assert np.array_equal(x, y)
    h, root, alphas, lj, rows1, rows2, _ = one
    assert math.isfinite(lj) and np.all(np.isfinite(alphas)) and np.all(alphas > 0) and len(set(alphas[:, 0])) == 20
    assert rows1.shape == (4, h.shape[1]) and rows2.shape == (3, h.shape[1])
    for g, (lo, hi) in enumerate(((0, 10), (10, 10), (10, 40), (40, 64))):     # the pairs hold their level-1 node's row
        assert np.all(h[lo:hi] == rows1[g]) and abs(math.fsum(rows1[g]) - 1.0) <= 2.0 * U * h.shape[1]
    for row in list(rows2) + [root]:
        assert abs(math.fsum(row) - 1.0) <= 2.0 * U * h.shape[1]


def test_a_level_round_trips_and_refusals_leave_the_state():
    L = capi.lib()
    ti, I, Kd = small_tree()
    a, bpar = 0.3, np.full(I, 2.0)
    try:
        # a new tree's upper rows are the object's root; level 1 has nothing before a step
        assert np.array_equal(ti.get_htree_level(2), np.full((3, Kd), 1.0 / Kd))
        with pytest.raises(capi.StbError, match="none has succeeded"):
            ti.get_htree_level(1)
        rows = 0.1 + np.arange(3 * Kd, dtype=np.float64).reshape(3, Kd) / 7.0
        ti.set_htree_level(2, rows)
        assert np.array_equal(ti.get_htree_level(2), rows)
        for bad, match in ((np.zeros((3, Kd)), "rows"), (np.full((3, Kd), math.nan), "rows"), (-rows, "rows")):
            with pytest.raises(capi.StbError, match=match):
                ti.set_htree_level(2, bad)
        assert L.stb_tindic_set_htree_level(ti.h, 1, capi.dp(rows)) != 0 and "level=1" in capi.last_error()
        assert L.stb_tindic_get_htree_level(ti.h, 3, capi.dp(rows)) != 0 and "level=3" in capi.last_error()
        with pytest.raises(capi.StbError, match="none yet"):
            ti.sample_htree(None, 1.0, 1, 0)                        # no concentrations to take up
        info = ti.sample_htree([2.0, 3.0], 1.0, 5, 0, flags=capi.HT_SAMPLE_ALPHA, shape=2.0, scale=3.0)
        alpha = list(info.alpha)[:2]
        before = (ti.get_h(), ti.get_hroot(), ti.get_htree_level(1), ti.get_htree_level(2))
        bad_g = np.full(Kd, 1.0)
        bad_g[Kd - 1] = math.inf
        both = capi.HT_SAMPLE_ALPHA
        for kw, match in ((dict(alpha=[-1.0, 1.0]), r"alpha\[0\]"), (dict(alpha=[1.0, math.nan]), r"alpha\[1\]"),
                          (dict(alpha=[math.inf, 1.0]), r"alpha\[0\]"), (dict(gamma=0.0), "gamma0"),
                          (dict(gamma=bad_g), r"gamma\[%d\]" % (Kd - 1)), (dict(flags=both, shape=0.0), "shape"),
                          (dict(flags=both, scale=math.inf), "scale"), (dict(flags=4), "flags"),
                          (dict(alpha=[1.0], levels=1), "levels=1"), (dict(alpha=None, levels=9), "levels=9")):
            args = dict(alpha=[2.0, 2.0], gamma=1.0, seed=1, sweep=0, flags=0, shape=1.0, scale=1.0)
            args.update(kw)
            with pytest.raises(capi.StbError, match=match):
                ti.sample_htree(**args)
        for off, match in (([[0, 10, 63], [0, 2]], "ranges run"), ([[0, 10, 64], [0, 3]], "ranges run"),
                           ([[0, 40, 10, 64], [0, 3]], "off"), ([[0, 10, 64], [1, 2]], "ranges run")):
            with pytest.raises(capi.StbError, match=match):
                ti.set_htree([np.array(o, dtype=np.uint64) for o in off])
        assert L.stb_tindic_sample_htree(ti.h, None, 1, 0, None) != 0 and "opts" in capi.last_error()
        after = (ti.get_h(), ti.get_hroot(), ti.get_htree_level(1), ti.get_htree_level(2))
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        # ranges and concentrations as they were: the step the object would have taken anyway, against a twin that saw no
        # refusal
        twin, _, _ = small_tree()
        try:
            twin.set_htree_level(2, rows)
            twin.sample_htree([2.0, 3.0], 1.0, 5, 0, flags=capi.HT_SAMPLE_ALPHA, shape=2.0, scale=3.0)
            for o in (ti, twin):
                assert list(o.sample_htree(None, 1.0, 6, 1).alpha)[:2] == alpha
            assert np.array_equal(ti.get_h(), twin.get_h()) and np.array_equal(ti.get_hroot(), twin.get_hroot())
            assert np.array_equal(ti.get_htree_level(2), twin.get_htree_level(2))
        finally:
            twin.free()
        # the grouped step's ranges are not the tree's: _set_hgroups leaves the tree's step as it is
        ti.set_hgroups(None)
        assert list(ti.sample_htree(None, 1.0, 7, 2).tables)[:2][0] > 0
        # the collapsed joint is not this model's; without a tree, or with one level, it answers as before
        with pytest.raises(capi.StbError, match="tree of 2 levels"):
            ti.logjoint_collapsed(a, bpar, alpha=1.0, flags=capi.CJ_INDICATORS)
        ti.set_htree(None)
        ti.set_hroot(None)                     # (the grouped formula reads the root, and the steps above have redrawn it)
        with_none = ti.logjoint_collapsed(a, bpar, alpha=1.0, flags=capi.CJ_INDICATORS)[0]
        ref, _, _ = tgh.small_chain()          # (an object that never had a tree, in the same state: no sweep has run)
        try:
            ref.set_hgroups(None)
            assert ref.logjoint_collapsed(a, bpar, alpha=1.0, flags=capi.CJ_INDICATORS)[0] == with_none
        finally:
            ref.free()
        assert math.isfinite(with_none)
        with pytest.raises(capi.StbError, match="no tree"):
            ti.sample_htree([1.0, 1.0], 1.0, 1, 0, levels=2)
    finally:
        ti.free()


def test_raw_refusals_write_nothing_and_a_failed_step_blocks_the_dish_sweep():
    import torch

    L = capi.lib()
    I, Kd = 64, 6
    koff, td = dev(koff_of(np.full(I, Kd)), np.uint64), dev(np.ones(I * Kd), np.uint16)
    root, h = dev(np.full(Kd, 0.5), np.float64), dev(np.full(I * Kd, 7.0), np.float64)
    rows2 = dev(np.full((2, Kd), 0.25), np.float64)
    off = [dev(np.array([0, 10, 64]), np.uint64), dev(np.array([0, 1, 2]), np.uint64)]
    bad0 = [dev(np.array([0, 70, 64]), np.uint64), off[1]]
    short1 = [off[0], dev(np.array([0, 1, 3]), np.uint64)]
    P = capi._ptr_array
    Gv = (capi.C.c_int * 2)(2, 2)
    G0 = (capi.C.c_int * 2)(2, 0)
    offp = lambda o: P([x.data_ptr() for x in o])
    nodes = P([None, rows2.data_ptr()])
    keep, opts = capi.htree_opts(2, [1.0, 1.0])
    keep2, bad_alpha = capi.htree_opts(2, [1.0, 0.0])
    keep3, nine = capi.htree_opts(2, [1.0, 1.0])
    nine.levels = 9
    _, no_alpha = capi.htree_opts(2, None)
    sp, ob = capi.stream_ptr(), capi.C.byref(opts)
    kp, tp, rp, hp = koff.data_ptr(), td.data_ptr(), root.data_ptr(), h.data_ptr()
    for args, match in (((I, None, tp, Kd, Gv, offp(off), ob, rp, nodes, hp), "required"),
                        ((I, kp, None, Kd, Gv, offp(off), ob, rp, nodes, hp), "required"),
                        ((I, kp, tp, Kd, None, offp(off), ob, rp, nodes, hp), "required"),
                        ((I, kp, tp, Kd, Gv, None, ob, rp, nodes, hp), "required"),
                        ((I, kp, tp, Kd, Gv, offp(off), ob, None, nodes, hp), "required"),
                        ((I, kp, tp, Kd, Gv, offp(off), ob, rp, None, hp), "required"),
                        ((I, kp, tp, Kd, Gv, offp(off), ob, rp, nodes, None), "required"),
                        ((I, kp, tp, Kd, Gv, offp(off), None, rp, nodes, hp), "opts"),
                        ((I, kp, tp, Kd, Gv, offp(off), capi.C.byref(no_alpha), rp, nodes, hp), "alpha is required"),
                        ((I, kp, tp, Kd, Gv, offp(off), capi.C.byref(nine), rp, nodes, hp), "levels=9"),
                        ((I, kp, tp, 0, Gv, offp(off), ob, rp, nodes, hp), "Kmax=0"),
                        ((I, kp, tp, 1025, Gv, offp(off), ob, rp, nodes, hp), "Kmax=1025"),
                        ((I, kp, tp, Kd, G0, offp(off), ob, rp, nodes, hp), r"G\[1\]=0"),
                        ((I, kp, tp, Kd, Gv, P([off[0].data_ptr(), None]), ob, rp, nodes, hp), r"d_off\[1\]"),
                        ((I, kp, tp, Kd, Gv, offp(off), ob, rp, P([None, None]), hp), r"d_hnode\[1\]"),
                        ((I, kp, tp, Kd, Gv, offp(bad0), ob, rp, nodes, hp), "off"),
                        ((I, kp, tp, Kd, Gv, offp(short1), ob, rp, nodes, hp), "ranges run"),
                        ((I, kp, tp, Kd, Gv, offp(off), capi.C.byref(bad_alpha), rp, nodes, hp), r"alpha\[1\]")):
        assert L.stb_sample_htree(*args, None, None, 1, 0, sp, None) != 0, match
        assert re.search(match, capi.last_error()), (match, capi.last_error())
    torch.cuda.synchronize()
    assert torch.all(h == 7.0) and torch.all(root == 0.5) and torch.all(rows2 == 0.25)
    # a failure after the wait: a root so large that alpha r_k is infinite at level 2.  h is then undefined and the dish
    # sweep refused, as after a failed sample_h, until a draw succeeds.  A root so small that alpha r_k + 0 is exactly 0 is no
    # failure: the coordinate is 0 at level 2 and, through alpha 0 + 0, in both leaves, where nobody serves that dish
    a = 0.3
    cust = np.array([0, 0, 1, 0, 1], dtype=np.uint32)          # two restaurants of three dishes; nobody serves the third
    n2 = np.array([2, 1, 0, 1, 1, 0], dtype=np.uint32)
    two = capi.TableIndicators(np.full(2, 3, dtype=np.int32), n2, (n2 > 0).astype(np.uint16), None, cust)
    try:
        two.set_hroot(np.array([0.3, 0.3, 1e308]))
        two.set_htree([np.array([0, 1, 2], dtype=np.uint64), np.array([0, 2], dtype=np.uint64)])
        with pytest.raises(capi.StbError, match="error word 0x") as e:
            two.sample_htree([0.25, 1e10], 1.0, 9, 0, flags=capi.HT_KEEP_ROOT)
        assert e.value.info.error_word & 4
        with pytest.raises(capi.StbError, match="undefined"):
            two.sweep_dishes(a, np.full(2, 2.0), 65, 0)
        with pytest.raises(capi.StbError, match="none has succeeded"):
            two.get_htree_level(1)
        two.set_hroot(None)
        two.set_htree_level(2, np.full((1, 3), 1.0 / 3.0))
        two.sample_htree([0.25, 0.25], 1.0, 9, 0)
        assert two.sweep_dishes(a, np.full(2, 2.0), 65, 0).stuck == 0
        two.set_hroot(np.array([0.3, 0.3, 5e-324]))
        two.sample_htree([0.25, 0.25], 1.0, 9, 1, flags=capi.HT_KEEP_ROOT)
        h2, up = two.get_h().reshape(2, 3), two.get_htree_level(2)
        assert up[0, 2] == 0.0 and np.all(h2[:, 2] == 0.0) and np.all(h2[:, :2] > 0.0) and np.all(up[0, :2] > 0.0)
        assert np.all(np.abs(h2.sum(axis=1) - 1.0) <= 6.0 * 2.0 ** -53)
        assert two.sweep_dishes(a, np.full(2, 2.0), 65, 1).stuck == 0
    finally:
        two.free()


# ---- 6. the example ----

EXE = tgh.EXE
ARGS = ["-J", "8", "-n", "400", "-c", "4", "-s", "5", "-d", "-z", "-w"]


def test_example_on_a_tree():
    assert os.path.exists(EXE), "examples/bin/pyp_resample not built (make -C libstb_amd/csrc)"
    p = subprocess.run([EXE] + ARGS + ["-T", "4:2"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = re.findall(r"^iteration (\d+): base weights on a tree of 2 levels, alpha (\S+) (\S+), (\d+) tables, (\d+) auxiliary at level 1, "
                      r"largest \|sum h - 1\| (\S+)$", p.stdout, re.M)
    assert [int(r[0]) for r in rows] == list(range(4)), p.stdout
    for _, a1, a2, tables, aux, worst in rows:
        assert all(math.isfinite(float(x)) and float(x) > 0 for x in (a1, a2)) and int(tables) >= int(aux) > 0
        assert 0.0 <= float(worst) <= 2.0 * U * 50 * 2           # (the example adds the 50 weights once more itself)
    # without -T the tree's lines are absent; -T without -d -z -w, with -H, or malformed, is refused
    q = subprocess.run([EXE] + ARGS, capture_output=True, text=True, timeout=60)
    assert q.returncode == 0 and "on a tree" not in q.stdout
    for extra in (["-d", "-z", "-T", "4:2"], ARGS + ["-T", "4:2", "-H", "2"], ARGS + ["-T", "4:"], ARGS + ["-T", "0:1"]):
        assert subprocess.run([EXE] + extra, capture_output=True, text=True, timeout=60).returncode == 2, extra
