"""One concentration per group of restaurants, drawn on the device (hyperb.hip, stb_sample_bgroups): the kernels against
the numpy replay of tests/hb_oracle.py, the same bits for every geometry and form, the block sums past one pass of the
lanes, the law on the device, the step on the tcounts / tindic objects with STB_BPAR_RESIDENT, the refusals, and
examples/pyp_resample -d -B.  Seeds and their margins come from tests/test_bgroups_host.py."""
import ctypes as C
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

from devarr import dev_coff, dev_u32
import hb_oracle as hb
import orc
from libstb_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
LAW_N, LAW_START, LAW_SEED = 20000, 1, 100   # as tests/test_bgroups_host.py, where the oracle passes at this seed


class env:
    """environment variables for the calls inside (None: unset)"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def dev_f64(x):
    import torch

    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device="cuda")


def dev_i64(x):
    import torch

    return None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=np.int64), device="cuda")


def step(a, shape, scale, T, N, bpar, goff, seed, sweep, want_rate=True, coff=False):
    """one raw call on host arrays: dict of host arrays, as hb.replay's"""
    bd = dev_f64(bpar)
    bg, Lt, Yt, rate, info = capi.sample_bgroups(a, shape, scale, dev_u32(T), bd, seed, sweep, N=None if coff else dev_u32(N),
                                                 coff=dev_coff(N) if coff else None, goff=dev_i64(goff), want_rate=want_rate)
    return dict(L=Lt.cpu().numpy(), Y=Yt.cpu().numpy().view(np.uint32), bgrp=bg.cpu().numpy(), bpar=bd.cpu().numpy(),
                rate=None if rate is None else rate.cpu().numpy(), kept=int(info.kept_groups), info=info)


@functools.lru_cache(maxsize=None)
def oracle(a, grouping):
    T, N, b, goff = hb.replay_case(grouping)
    shape, scale = hb.REPLAY_PRIOR
    return hb.replay(a, shape, scale, T, N, b, goff, hb.REPLAY_SEEDS[a], hb.REPLAY_SWEEP)


def scatter(bgrp, goff, I):
    return bgrp.copy() if goff is None else np.repeat(bgrp, np.diff(goff))


def same_bits(r, r0):
    return all(np.array_equal(r[k], r0[k], equal_nan=True) for k in ("L", "Y", "bgrp", "bpar", "rate"))


# ---- replay

@pytest.mark.parametrize("grouping", ["each", "one", "ragged"])
@pytest.mark.parametrize("a", sorted(hb.REPLAY_SEEDS))
def test_the_step_equals_the_replay(a, grouping):
    T, N, b, goff = hb.replay_case(grouping)
    I = len(T)
    shape, scale = hb.REPLAY_PRIOR
    seed, sweep = hb.REPLAY_SEEDS[a], hb.REPLAY_SWEEP
    want = oracle(a, grouping)
    got = step(a, shape, scale, T, N, b, goff, seed, sweep)
    assert np.array_equal(got["Y"], want["Y"])
    L, Lw = got["L"], want["L"]
    assert (L[N == 0] == 0).all() and np.isfinite(L).all() and (L[N > 0] > 0).all()
    out = np.abs(L - Lw) > 1e-12 * np.maximum(1.0, Lw)
    print("a=%g %s: %d of %d restaurants outside 1e-12" % (a, grouping, int(out.sum()), I))
    assert out.sum() <= I // 10 ** 5
    lo = np.arange(I) if goff is None else goff[:-1]
    hi = lo + 1 if goff is None else goff[1:]
    for g in range(len(lo)):   # the sum the kernel formed, against the exactly rounded sum of what it summed
        n = int(hi[g] - lo[g])
        ref = math.fsum(L[lo[g]:hi[g]]) + 1.0 / scale
        assert abs(got["rate"][g] - ref) <= 4 * U * max(n, 1) * abs(ref), (g, n)
    assert got["kept"] == 0 and want["kept"] == 0
    rel = np.abs(got["bgrp"] - want["bgrp"]) / want["bgrp"]
    print("  worst b_g error %.2e over %d groups" % (rel.max(), len(rel)))
    assert (rel <= 1e-10).all()
    assert np.array_equal(got["bpar"], scatter(got["bgrp"], goff, I))
    if grouping == "one":   # equal b: stb_sample_logq's L and Q, to the bit
        Q, Lq = capi.sample_logq(3.7, scale, dev_u32(N), seed=seed, sweep=sweep)
        assert np.array_equal(Lq.cpu().numpy(), L) and Q == got["rate"][0]
        assert got["info"].b == got["bgrp"][0]
    else:
        assert got["info"].b != got["info"].b


# ---- the same bits

@pytest.mark.parametrize("grouping", ["each", "ragged"])
def test_waves_and_forms_give_the_same_bits(grouping):
    T, N, b, goff = hb.replay_case(grouping)
    shape, scale = hb.REPLAY_PRIOR
    r0 = None
    for wv in (4, 1, 2, 8):
        for form in (None, "lane", "wave"):
            with env(STB_HYPERB_WAVES=wv, STB_HYPERB_FORM=form):
                r = step(0.3, shape, scale, T, N, b, goff, 7101, 5)
            r0 = r if r0 is None else r0
            assert same_bits(r, r0), (wv, form)
    # the customers as prefix sums, and without Y or the rates coming back
    assert same_bits(step(0.3, shape, scale, T, N, b, goff, 7101, 5, coff=True), r0)
    bd = dev_f64(b)
    bg, Lt, none, _, _ = capi.sample_bgroups(0.3, shape, scale, dev_u32(T), bd, 7101, 5, N=dev_u32(N), goff=dev_i64(goff), want_Y=False)
    assert none is None and np.array_equal(bg.cpu().numpy(), r0["bgrp"]) and np.array_equal(bd.cpu().numpy(), r0["bpar"])
    assert not same_bits(step(0.3, shape, scale, T, N, b, goff, 7101, 6), r0)   # (another sweep: other draws)


def test_ranges_of_one_restaurant_are_the_call_without_ranges():
    T, N, b, _ = hb.replay_case("each")
    shape, scale = hb.REPLAY_PRIOR
    r0 = step(0.9, shape, scale, T, N, b, None, 7102, 5)
    r1 = step(0.9, shape, scale, T, N, b, np.arange(len(T) + 1), 7102, 5)
    assert same_bits(r1, r0)


# ---- lane wrap

def test_block_sums_past_one_pass_of_the_lanes():
    I = 256 * 64 + 257
    shape, scale, a, b = 1.5, 20.0, 0.3, 3.7
    u = synth.unit(I, 31)
    T = (np.arange(I) % 4).astype(np.uint32)
    N = np.where(T == 0, 0, T + np.floor(u * 50)).astype(np.uint32)
    goff = np.array([0, I])
    want = hb.replay(a, shape, scale, T, N, np.full(I, b), goff, 812, 2)
    assert want["margin_gamma"] > 1e-9 and want["margin_y"] > 1e-9
    r0 = None
    for wv in (4, 1, 8):
        with env(STB_HYPERB_WAVES=wv):
            r = step(a, shape, scale, T, N, np.full(I, b), goff, 812, 2)
        r0 = r if r0 is None else r0
        assert same_bits(r, r0), wv
    assert np.array_equal(r0["Y"], want["Y"])
    assert (np.abs(r0["L"] - want["L"]) <= 1e-12 * np.maximum(1.0, want["L"])).all()
    assert r0["rate"][0] == hb.group_rate(r0["L"], 1.0 / scale)          # the association, on the device's own L
    ref = math.fsum(r0["L"]) + 1.0 / scale
    assert abs(r0["rate"][0] - ref) <= 4 * U * I * abs(ref)
    Q, _ = capi.sample_logq(b, scale, dev_u32(N), seed=812, sweep=2)
    assert Q == r0["rate"][0]
    assert abs(r0["bgrp"][0] - want["bgrp"][0]) <= 1e-10 * want["bgrp"][0]
    assert (r0["bpar"] == r0["bgrp"][0]).all()


def test_one_group_past_one_round_of_block_sums():
    """more than 512 blocks of 256 in one group: pass 2 holds 512 block sums at a time and goes round again"""
    I = 140001
    assert (I + 255) // 256 > 512
    shape, scale, a, b = 1.5, 20.0, 0.3, 3.7
    u = synth.unit(I, 37)
    T = (np.arange(I) % 3).astype(np.uint32)
    N = np.where(T == 0, 0, T + np.floor(u * 20)).astype(np.uint32)
    goff = np.array([0, I])
    want = hb.replay(a, shape, scale, T, N, np.full(I, b), goff, 813, 1)
    assert want["margin_gamma"] > 1e-9 and want["margin_y"] > 1e-9
    r0 = None
    for wv in (None, 4, 1):   # (None: the eight waves a range of this size gets)
        with env(STB_HYPERB_WAVES=wv):
            r = step(a, shape, scale, T, N, np.full(I, b), goff, 813, 1)
        r0 = r if r0 is None else r0
        assert same_bits(r, r0), wv
    assert np.array_equal(r0["Y"], want["Y"])
    assert (np.abs(r0["L"] - want["L"]) <= 1e-12 * np.maximum(1.0, want["L"])).all()
    assert r0["rate"][0] == hb.group_rate(r0["L"], 1.0 / scale)
    ref = math.fsum(r0["L"]) + 1.0 / scale
    assert abs(r0["rate"][0] - ref) <= 4 * U * I * abs(ref)
    Q, _ = capi.sample_logq(b, scale, dev_u32(N), seed=813, sweep=1)
    assert Q == r0["rate"][0]
    assert abs(r0["bgrp"][0] - want["bgrp"][0]) <= 1e-10 * want["bgrp"][0]
    assert (r0["bpar"] == r0["bgrp"][0]).all()


# ---- the law on the device

def device_step(a, shape, scale, T, N, bpar, goff, seed, sweep):
    return step(a, shape, scale, T, N, bpar, goff, seed, sweep, want_rate=False)["bpar"]


@pytest.mark.parametrize("case", hb.CASES)
def test_the_devices_chain_holds_the_posterior(case):
    b, post = hb.chain(case, LAW_N, 3, LAW_START, LAW_SEED, step_fn=device_step)
    p = hb.ks_pvalue(post.F(b))
    print("%s: KS p = %.3g after three steps on the device" % (case, p))
    assert np.isfinite(b).all() and (b > 0).all()
    assert p > 1e-3


# ---- the objects

def make(kind, g):
    return capi.TableCounts(g.K, g.n, g.t) if kind == "tcounts" else capi.TableIndicators(g.K, g.n, g.t)


@pytest.mark.parametrize("kind", ["tcounts", "tindic"])
def test_the_step_on_an_object(kind):
    L = capi.lib()
    g = synth.groups(700, 6, 120, "realistic", seed=12)
    a, shape, scale = 0.4, g.shape, g.scale
    b0 = np.exp(np.log(0.05) + synth.unit(g.I, 5) * np.log(400.0))
    obj, ref = make(kind, g), make(kind, g)
    h1 = L.stb_groups_create(g.I, orc.i32p(g.K), None, None, None, None, 0, 0, 3)
    h2 = L.stb_groups_create(g.I, orc.i32p(g.K), None, None, None, None, 0, 0, 3)
    assert h1 and h2, capi.last_error()
    try:
        # set_bpar -> sampleb_groups -> get_bpar is the raw call on the object's counts
        obj.set_bpar(b0)
        assert np.array_equal(obj.get_bpar(), b0)
        bg, info = obj.sampleb_groups(a, shape, scale, seed=41, sweep=3)
        raw = step(a, shape, scale, g.T, g.N, b0, None, 41, 3, coff=kind == "tindic")
        b1 = obj.get_bpar()
        assert np.array_equal(b1, raw["bpar"]) and np.array_equal(bg, raw["bgrp"]) and info.kept_groups == 0
        assert (b1 > 0).all() and np.isfinite(b1).all() and (b1 != b0).all()
        # a sweep with the sentinel has the bits of the same sweep with the read-back vector from the host
        obj.sweep(a, capi.BPAR_RESIDENT, 77, 0, 2)
        ref.sweep(a, b1, 77, 0, 2)
        t1, T1 = obj.get()
        t2, T2 = ref.get()
        assert np.array_equal(t1, t2) and np.array_equal(T1, T2) and not np.array_equal(t1, g.t)
        assert np.array_equal(obj.get_bpar(), b1)
        tot1 = obj.logjoint(a, capi.BPAR_RESIDENT)[0]
        tot2 = ref.logjoint(a, b1)[0]
        assert tot1 == tot2
        # to_groups with the sentinel, then aterms: the host-bpar route's values
        x = np.array([0.2, 0.4, 0.7])
        out1, out2 = np.zeros(3), np.zeros(3)
        obj.to_groups(h1, capi.BPAR_RESIDENT)
        ref.to_groups(h2, b1)
        capi.check(L.stb_groups_aterms(h1, capi.dp(x), 3, capi.dp(out1)))
        capi.check(L.stb_groups_aterms(h2, capi.dp(x), 3, capi.dp(out2)))
        assert np.array_equal(out1, out2) and np.isfinite(out1).all()
        # the trap: after a step a host bpar equal to the values before it must be uploaded again
        obj.set_bpar(b0)
        obj.sampleb_groups(a, shape, scale, seed=41, sweep=4)
        assert not np.array_equal(obj.get_bpar(), b0)
        obj.sweep(a, b0, 78, 0, 1)            # (the same host vector the last upload saw)
        assert np.array_equal(obj.get_bpar(), b0)
        # ranges: one group, and the raw call with the same ranges
        goff = np.array([0, 100, 100, 433, g.I], dtype=np.uint64)
        bgrp0 = np.array([0.5, 1.0, 7.0, 90.0])
        bb = np.repeat(bgrp0, np.diff(goff.astype(np.int64)))
        obj.set_bgroups(goff)
        obj.set_bpar(bb)
        t_now, T_now = obj.get()
        bg, info = obj.sampleb_groups(a, shape, scale, seed=43, sweep=1)
        raw = step(a, shape, scale, T_now, g.N, bb, goff.astype(np.int64), 43, 1)
        assert np.array_equal(bg, raw["bgrp"]) and np.array_equal(obj.get_bpar(), raw["bpar"])
        obj.set_bgroups(np.array([0, g.I], dtype=np.uint64))
        obj.set_bpar(np.full(g.I, 2.5))
        bg, info = obj.sampleb_groups(a, shape, scale, seed=44, sweep=1)
        assert len(bg) == 1 and info.b == bg[0] and (obj.get_bpar() == bg[0]).all()
    finally:
        obj.free()
        ref.free()
        L.stb_groups_free(h1)
        L.stb_groups_free(h2)
        L.stb_sampler_cache_clear()


# ---- refusals

def test_refused_calls_leave_the_concentrations_as_they_were():
    import torch

    L = capi.lib()
    T, N, b, goff = hb.replay_case("ragged")
    shape, scale = hb.REPLAY_PRIOR
    Td, Nd, gd = dev_u32(T), dev_u32(N), dev_i64(goff)

    def refused(bvec, a=0.3, shape=shape, scale=scale, goff=gd, N=Nd, coff=None, word=None):
        bd = dev_f64(bvec)
        with pytest.raises(capi.StbError) as e:
            capi.sample_bgroups(a, shape, scale, Td, bd, 1, 0, N=N, coff=coff, goff=goff)
        assert "stb_sample_bgroups" in str(e.value)
        assert np.array_equal(bd.cpu().numpy(), bvec, equal_nan=True)
        if word is not None:
            assert e.value.info.error_word & word
            assert word == 8 or e.value.info.bad_restaurants >= 1
        return e.value

    for bad in (0.0, -1.0, float("nan"), float("inf")):
        bb = b.copy()
        bb[1500] = bad
        refused(bb, goff=None, word=2)
    bb = b.copy()
    bb[300] = np.nextafter(bb[300], 1.0)       # unequal inside the range 256 .. 511
    e = refused(bb, word=4)
    assert e.info.bad_restaurants == 1
    bad_goff = goff.copy()
    bad_goff[3] = goff[4] + 5                  # ranges out of order
    refused(b, goff=dev_i64(bad_goff), word=8)
    short = goff.copy()
    short[-1] -= 1                             # ... and ranges that do not reach I
    refused(b, goff=dev_i64(short), word=8)
    refused(b, shape=0.0)
    refused(b, shape=-1.0)
    refused(b, scale=0.0)
    refused(b, a=1.0)
    refused(b, a=-0.1)
    refused(b, N=None)                         # neither d_N nor d_coff
    refused(b, coff=dev_coff(N))               # both
    # the objects: the sentinel before any b is resident, a refused step, and the object still works
    g = synth.groups(60, 5, 60, "realistic", seed=2)
    for kind in ("tcounts", "tindic"):
        obj = make(kind, g)
        try:
            with pytest.raises(capi.StbError, match="holds no concentrations"):
                obj.sweep(0.3, capi.BPAR_RESIDENT, 1, 0, 1)
            with pytest.raises(capi.StbError, match="holds no concentrations"):
                obj.sampleb_groups(0.3, 1.1, 20.0, 1, 0)
            with pytest.raises(capi.StbError, match="holds no concentrations"):
                obj.get_bpar()
            with pytest.raises(capi.StbError, match="bpar is required"):   # NULL stays the error it is
                capi.check(getattr(L, "stb_%s_sweep" % kind)(obj.h, 0.3, None, 1, 0, 1))
            bb = np.full(g.I, 4.0)
            bb[7] = -0.1                        # legal for a sweep at a = 0.3, not for the step
            obj.set_bpar(bb)
            obj.sweep(0.3, capi.BPAR_RESIDENT, 1, 0, 1)          # -0.1 > -a
            t_sw, T_sw = obj.get()
            with pytest.raises(capi.StbError, match="must be > -a"):   # ... but not at a smaller discount
                obj.sweep(0.05, capi.BPAR_RESIDENT, 1, 1, 1)
            with pytest.raises(capi.StbError, match="must be > -a"):
                obj.logjoint(0.05, capi.BPAR_RESIDENT)
            t2, T2 = obj.get()
            assert np.array_equal(t2, t_sw) and np.array_equal(T2, T_sw)
            for args in ((0.3, 1.1, 20.0), (0.3, 0.0, 20.0), (1.0, 1.1, 20.0)):
                with pytest.raises(capi.StbError):
                    obj.sampleb_groups(*args, 1, 0)
                assert np.array_equal(obj.get_bpar(), bb)
            t2, T2 = obj.get()
            assert np.array_equal(t2, t_sw) and np.array_equal(T2, T_sw)
            obj.set_bpar(np.full(g.I, 4.0))
            bg, info = obj.sampleb_groups(0.3, 1.1, 20.0, 1, 0)
            assert (bg > 0).all() and np.isfinite(bg).all()
            obj.sweep(0.0, capi.BPAR_RESIDENT, 1, 2, 1)          # after a step every concentration is positive
        finally:
            obj.free()
    L.stb_sampler_cache_clear()
    del torch


# ---- example

def test_example_resamples_a_concentration_per_restaurant():
    exe = os.path.join(ROOT, "examples", "bin", "pyp_resample")
    assert os.path.exists(exe), "examples/bin/pyp_resample not built (make -C libstb_amd/csrc)"
    p = subprocess.run([exe, "-d", "-B", "-J", "4", "-n", "1500", "-a", "0.4", "-b", "15", "-c", "20", "-s", "3"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:] + p.stdout[-2000:]
    rows = re.findall(r"b_i min ([0-9.eE+-]+) median ([0-9.eE+-]+) max ([0-9.eE+-]+)", p.stdout)
    print(p.stdout)
    assert len(rows) == 20, p.stdout
    for lo, med, hi in rows:
        lo, med, hi = float(lo), float(med), float(hi)
        assert math.isfinite(lo) and math.isfinite(hi) and 0 < lo <= med <= hi
    p = subprocess.run([exe, "-d", "-B", "-j", "-J", "3", "-n", "500", "-c", "2"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "-B" in (p.stderr + p.stdout)
