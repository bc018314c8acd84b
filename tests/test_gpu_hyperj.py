"""The joint (a, b) step on the device (libstb_amd/csrc/hyperj.hip; DESIGN.md section 6, deviation 14): k_joint_terms
against the high-precision truth and across launch geometries -- also past one trip per workgroup in x and in j, on sizes
taken from stb_reduce_geometry --, the pair sum alone (stb_groups_ssum), the step against
the replay of tests/hj_oracle.py run on the device's own L values, the object wrappers, the refusals, and
examples/pyp_resample -j.

The bar of R is derived in hj_oracle's header from the kernel's own roundings: the sum over the restaurants of the
term's bar (4 ulp for each device lgamma, one rounding for each of c = b / a, T + c, b + N times lgamma's slope, one
rounding for each product, sum and difference, the term's share 8 u |term| of the block tree) + 4 u |R|.  The bar of a
stage's L adds W's bar (hp_oracle's model bar per pair + 4 u |W|), the prior's four roundings and the two additions
that form L: 8 u (|W| + |R| + |P| + |L|)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from devarr import dev_coff, dev_u32
import hj_oracle as hj
import hp_oracle as hp
import hp_pairs as hpp
import orc
import test_hyperj_host as host
from libstb_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


class waves:
    """STB_HYPERJ_WAVES for the calls inside"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        self.old = os.environ.get("STB_HYPERJ_WAVES")
        os.environ["STB_HYPERJ_WAVES"] = str(self.v)

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("STB_HYPERJ_WAVES", None)
        else:
            os.environ["STB_HYPERJ_WAVES"] = self.old


# ---- k_joint_terms

# (T, N) of restaurant i is TYPES[i % len(TYPES)]: T = 0 with customers, no customers at all, N up to 10^7
TYPES = [(0, 0), (0, 5), (1, 1), (3, 17), (15, 37), (200, 4000), (256, 300), (5000, 10 ** 7), (1, 10 ** 7), (70000, 10 ** 6)]
A64 = np.concatenate([[0.01], 0.01 + 0.97 * (np.arange(1, 63) / 63.0), [0.98]])   # A_MIN .. A_MAX
B64 = np.exp(np.linspace(math.log(0.01), math.log(2000.0), 64))                  # B_MIN .. B_MAX
B64[0], B64[-1] = 0.01, 2000.0
SUB = {(1, 1): ([0], [63]), (3, 2): ([0, 31, 63], [0, 63]),
       (24, 24): (list(np.round(np.linspace(0, 63, 24)).astype(int)),) * 2, (64, 64): (list(range(64)),) * 2}
_type_truth = {}


def type_truth():
    """per type the term's truth and bar over the 64 x 64 grid, computed once"""
    if not _type_truth:
        for T, N in TYPES:
            _type_truth[(T, N)] = hj.term_grid(A64, B64, T, N)
    return _type_truth


def test_the_grid_covers_the_stated_ranges():
    c = B64[None, :] / A64[:, None]
    assert c.min() < 0.0102041 and c.max() == 2e5 and A64[0] == 0.01 and A64[-1] == 0.98


@pytest.mark.parametrize("DJ", [(1, 1), (3, 2), (24, 24), (64, 64)])
@pytest.mark.parametrize("I", [1, 255, 256, 257, 2049])
def test_joint_terms_against_the_truth(I, DJ):
    ia, ib = SUB[DJ]
    a, b = A64[ia], B64[ib]
    first = 4 if I == 1 else 0   # (one restaurant: the type (15, 37))
    kinds = [TYPES[(first + i) % len(TYPES)] for i in range(I)]
    T = np.array([k[0] for k in kinds])
    N = np.array([k[1] for k in kinds])
    got = capi.joint_terms(a, b, dev_u32(T), dev_u32(N)).cpu().numpy()
    tt = type_truth()
    val = np.zeros((len(a), len(b)), dtype=hp.LD)
    bar = np.zeros((len(a), len(b)))
    for k in set(kinds):
        v, e = tt[k]
        cnt = kinds.count(k)
        val += hp.LD(cnt) * v[np.ix_(ia, ib)]
        bar += cnt * e[np.ix_(ia, ib)]
    bar += 4.0 * U * np.abs(val.astype(np.float64))
    err = np.abs((got.astype(hp.LD) - val).astype(np.float64))
    print("I=%d, %d x %d: worst error / bar %.3g (worst error %.3e)" % (I, len(a), len(b), float((err / bar).max()), float(err.max())))
    assert np.isfinite(got).all() and (err <= bar).all()


def test_joint_terms_without_customers_is_zero():
    got = capi.joint_terms([0.3, 0.5], [1.0, 7.0, 9.0], dev_u32(np.array([0, 0, 0])), dev_u32(np.array([0, 0, 0]))).cpu().numpy()
    assert got.shape == (2, 3) and (got == 0).all()


def test_joint_terms_has_the_same_bits_for_every_geometry():
    I = 2049
    kinds = [TYPES[i % len(TYPES)] for i in range(I)]
    Td, Nd = dev_u32([k[0] for k in kinds]), dev_u32([k[1] for k in kinds])
    ia, ib = SUB[(24, 24)]
    ref = None
    for wv in (1, 2, 4, 8, 4):
        with waves(wv):
            got = capi.joint_terms(A64[ia], B64[ib], Td, Nd).cpu().numpy()
        ref = got if ref is None else ref
        assert np.array_equal(got, ref), wv


# ---- k_joint_terms past one trip per workgroup, in x (blocks of restaurants) and in y (the b_j)

HJ_CASES = ["ragged j", "J1", "x trip 3 x 2", "x trip 24 x 24", "x trip 64 x 64", "two x trips 1 x 1"]


def hj_geom(I, DJ, wv=0):
    return capi.reduce_geometry(capi.GEOM_JOINT_TERMS, I, DJ[0], DJ[1], wv)


def hj_width():
    """the workgroups of a launch with more steps than the device takes at once"""
    return hj_geom(1 << 30, (1, 1)).grid_x


def hj_case(label, wv=0):
    """(I, (D, J)) and the case's premise, asserted through the query -- every size from the device at hand"""
    W = hj_width()
    if label == "ragged j":   # 17 blocks: the workgroups left over for j do not divide the 64 b_j evenly
        I, DJ = 4352, (64, 64)
        g = hj_geom(I, DJ)
        assert g.grid_x == 17 and g.grid_y == W // 17 and g.grid_y < 64 and 64 % g.grid_y != 0, (g.grid_x, g.grid_y)
    elif label == "J1":   # MEASUREMENTS section J1's shape: several j trips a workgroup
        I, DJ = 10 ** 5, (24, 24)
        g = hj_geom(I, DJ)
        assert g.blocks == 391 and g.grid_x == g.steps and 2 * g.grid_y <= 24, (g.grid_x, g.grid_y)
    else:
        DJ = {"x trip 3 x 2": (3, 2), "x trip 24 x 24": (24, 24), "x trip 64 x 64": (64, 64), "two x trips 1 x 1": (1, 1)}[label]
        span = 256 * hj_geom(1, DJ, wv).chunks
        if label.startswith("two"):
            I = 2 * span * W + 513
            g = hj_geom(I, DJ, wv)
            assert g.grid_x == W and g.steps > 2 * g.grid_x and g.grid_y == 1
        else:   # a second x trip for one workgroup, and every j in one workgroup
            I = span * W + 1
            g = hj_geom(I, DJ, wv)
            assert g.grid_x == W and g.steps == g.grid_x + 1 and g.grid_y == 1
    return I, DJ


def tiled_counts(I):
    reps = -(-I // len(TYPES))
    return np.tile([k[0] for k in TYPES], reps)[:I], np.tile([k[1] for k in TYPES], reps)[:I]


def tiled_truth(I, DJ):
    """the truth and the bar of R for restaurant i of type TYPES[i mod 10]: multiplicity x the type's"""
    ia, ib = SUB[DJ]
    tt = type_truth()
    val = np.zeros((len(ia), len(ib)), dtype=hp.LD)
    bar = np.zeros((len(ia), len(ib)))
    for k, kind in enumerate(TYPES):
        cnt = I // len(TYPES) + (k < I % len(TYPES))
        v, e = tt[kind]
        val += hp.LD(cnt) * v[np.ix_(ia, ib)]
        bar += cnt * e[np.ix_(ia, ib)]
    return val, bar + 4.0 * U * np.abs(val.astype(np.float64))


def check_tiled(got, I, DJ, what):
    val, bar = tiled_truth(I, DJ)
    err = np.abs((got.astype(hp.LD) - val).astype(np.float64))
    print("%s, I=%d, %d x %d: worst error / bar %.3g (worst error %.3e)" % (what, I, DJ[0], DJ[1], float((err / bar).max()), float(err.max())))
    assert np.isfinite(got).all() and (err <= bar).all()


@pytest.mark.parametrize("label", HJ_CASES)
def test_joint_terms_past_one_trip_against_the_truth(label):
    I, DJ = hj_case(label)
    ia, ib = SUB[DJ]
    T, N = tiled_counts(I)
    Td = dev_u32(T)
    got = capi.joint_terms(A64[ia], B64[ib], Td, dev_u32(N)).cpu().numpy()
    check_tiled(got, I, DJ, label)
    # N as prefix sums (the objects' route) gives the same bits
    got2 = capi.joint_terms(A64[ia], B64[ib], Td, None, coff=dev_coff(N)).cpu().numpy()
    assert np.array_equal(got2, got)


def test_joint_terms_past_one_trip_has_the_same_bits_for_every_geometry():
    """24 x 24 at the size where a workgroup of eight waves makes a second x trip: every workgroup size makes one"""
    DJ = (24, 24)
    I, _ = hj_case("x trip 24 x 24", wv=8)
    ia, ib = SUB[DJ]
    T, N = tiled_counts(I)
    Td, Nd = dev_u32(T), dev_u32(N)
    ref = None
    for wv in (1, 2, 4, 8, 4):
        g = hj_geom(I, DJ, wv)
        assert g.steps > g.grid_x and g.grid_y == 1 and g.chunks == (2 if wv == 8 else 1)
        with waves(wv):
            assert hj_geom(I, DJ).waves == wv
            got = capi.joint_terms(A64[ia], B64[ib], Td, Nd).cpu().numpy()
        if ref is None:
            ref = got
            check_tiled(got, I, DJ, "x trip at eight waves")
        assert np.array_equal(got, ref), wv


def test_joint_terms_outgrows_its_block_sums_and_is_called_again():
    DJ = (24, 24)
    ia, ib = SUB[DJ]
    small, big = 2049, hj_case("J1")[0]
    gs, gb = hj_geom(small, DJ), hj_geom(big, DJ)
    assert gs.need <= gs.cap0 < gb.need
    capi.lib().stb_sampler_cache_clear()   # (this thread's buffer of block sums: the next call allocates cap0 afresh)
    out = []
    for I in (small, big, small, big):
        T, N = tiled_counts(I)
        out.append(capi.joint_terms(A64[ia], B64[ib], dev_u32(T), dev_u32(N)).cpu().numpy())
    check_tiled(out[0], small, DJ, "before the larger call")
    check_tiled(out[1], big, DJ, "the larger call")
    assert np.array_equal(out[2], out[0]) and np.array_equal(out[3], out[1])


# ---- stb_groups_ssum

def _pairs(N, M, G, seed):
    u = synth.unit(2 * G, seed)
    n = (2 + np.floor(u[0::2] * (N - 1))).astype(np.uint32)
    t = np.minimum(1 + np.floor(u[1::2] * np.minimum(n, M)), np.minimum(n, M)).astype(np.uint16)
    n[:4], t[:4] = [N, N, 2, 3], [M, 1, 2, 1]
    K = np.array([G // 2, G - G // 2], dtype=np.int32)
    T = np.array([int(t[:G // 2].sum()), int(t[G // 2:].sum())], dtype=np.uint32)
    return K, n, t, T, np.array([3.0, 7.0])


@pytest.mark.parametrize("N,M", [(1500, 1500), (300, 120)])
def test_ssum_is_the_pair_sum_alone(N, M):
    import torch

    L = capi.lib()
    K, n, t, T, bpar = _pairs(N, M, 4000, seed=N)
    xs = np.concatenate([[0.37, 0.01, 0.98], synth.discount_grid(22)])
    truth = hpp.aterms_truth_by_class([(K, n, t, T, bpar, np.zeros(len(n), dtype=np.int8))], xs, N, M)[0]
    h = hpp._create(L, K, n, t, T, bpar, N, M, 25)
    tabs = capi.DeviceTables(N, M, 25)
    tabs.fill(xs)
    tabs.status()
    dg = capi.DeviceGroups(synth.Groups(I=2, K=K, n=n, t=t, T=T, N=T, bpar=bpar))
    swept = capi.sweep(tabs, dg).cpu().numpy()
    try:
        for D in (1, 3, 25):
            x = xs[:D]
            before = hpp._aterms(L, h, x)
            form = hpp.last_form(L, h)
            cnt = hpp.Counters(L)
            got = capi.groups_ssum(h, x)
            assert hpp.last_form(L, h) == form, (D, form)
            cnt.check("ssum")
            for d in range(D):
                tv = truth.psum[d].sum()
                bar = float(truth.pbar[d].sum()) + 4 * U * abs(float(tv))
                e = abs(float(hp.LD(got[d]) - tv))
                es = abs(float(hp.LD(swept[d]) - tv))
                print("N=%d D=%d d=%d: form %r, error / bar %.3g (stored table + sweep: %.3g)" % (N, D, d, form, e / bar, es / bar))
                assert e <= bar and es <= bar
            # the device entry point leaves the same values on the device
            out = torch.zeros(D, dtype=torch.float64, device="cuda")
            capi.check(L.stb_groups_ssum_device(h, capi.dp(np.ascontiguousarray(x)), D, out.data_ptr(), None))
            capi.check(L.stb_groups_wait(h))
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), got)
            # aterms on the same set afterwards has the bits it had before
            assert np.array_equal(hpp._aterms(L, h, x), before)
            cnt.check("aterms after ssum")
    finally:
        L.stb_groups_free(h)


# ---- the step against the replay

RECT, SHAPE, SCALE = hj.STEP_RECT, hj.STEP_SHAPE, hj.STEP_SCALE
D = J = hj.STEP_D


def _L_truth(g, am, bm, bem):
    return hj.L_truth_grid(g, am, bm, bem, SHAPE, SCALE)


def test_the_step_equals_the_replay_on_the_devices_L():
    L = capi.lib()
    g = hj.step_problem()
    assert g.n.max() <= 60
    Nd = dev_u32(g.N)
    N, M = int(g.n.max()), int(g.t.max())
    h = hpp._create(L, g.K, g.n, g.t, g.T, np.full(g.I, 10.0), N, M, D + 1)
    steps, seed = hj.STEP_STEPS, hj.STEP_SEED
    a, b = hj.STEP_START
    left_out = accepted = 0
    first = None
    points = []   # (a, b, the device's L) of the current and of the proposed point of every step
    try:
        for k in range(steps):
            r = capi.groups_samplejoint(h, Nd, RECT, a, b, SHAPE, SCALE, seed, k, D, J, keep_L=True)
            u = hj.uniforms(seed, k)
            S = r["stages"]
            assert r["evals"] == S + 1 and 1 <= S <= 5
            if first is None:
                first = r["L"]
                # every stage's L within the bar of the oracle's, on the stages the oracle itself lays out
                oracle_stages = hj.stages_of(lambda s, am, bm, bem: _L_truth(g, am, bm, bem)[0], RECT, D, J, u[1])
                assert len(oracle_stages) == S
                for s, st in enumerate(oracle_stages):
                    am, bem, bm, _, _ = hj.cells_of(st["rect"], D, J)
                    Lt, bar = _L_truth(g, am, bm, bem)
                    err = np.abs(r["L"][s].reshape(D, J) - Lt)
                    print("stage %d: rectangle %r, worst L error / bar %.3g" % (s + 1, st["rect"], float((err / bar).max())))
                    assert (err <= bar).all()
                    if s + 1 < S:
                        assert st["box"] == r["box"][s]
            else:
                assert np.array_equal(r["L"], first)   # (the counts do not change: the same grids, the same bits)
            st = hj.stages_of(lambda s, am, bm, bem: r["L"][s].reshape(D, J), RECT, D, J, u[1])
            assert len(st) == S and [q["box"] for q in st] == r["box"]
            pick, ap, betap, bp = hj.propose(st, u)
            la, ok = hj.decide(st, r["L_cur"], r["L_prop"], (a, math.log(b)), (ap, betap), u[4])
            if hj.left_out(st, la, u[4]):
                left_out += 1
            else:
                assert [q["cell"] for q in st] == r["cell"], k
                assert pick + 1 == r["stage_pick"] and ap == r["a_prop"] and bp == r["b_prop"]
                assert abs(la - r["log_alpha"]) <= 1e-9 * max(1.0, abs(la)) and ok == r["accepted"], (k, la, r["log_alpha"])
            points += [(a, b, r["L_cur"]), (r["a_prop"], r["b_prop"], r["L_prop"])]
            accepted += r["accepted"]
            assert (r["a"], r["b"]) == ((r["a_prop"], r["b_prop"]) if r["accepted"] else (a, b))
            a, b = r["a"], r["b"]
            assert RECT[0] <= a <= RECT[1] and RECT[2] <= b <= RECT[3]
        # L at the two points of EVERY step against the truth (the replay above took the device's own values there)
        pts = np.array(points)
        Lt, bar = hj.L_truth_points(g, pts[:, 0], pts[:, 1], SHAPE, SCALE)
        err = np.abs(pts[:, 2] - Lt)
        print("L at %d points: worst error / bar %.3g" % (len(pts), float((err / bar).max())))
        assert (err <= bar).all(), np.nonzero(err > bar)[0][:10]
        print("%d steps, %d stages, %d accepted (the replay on oracle values: %d), %d left out" % (steps, S, accepted, host.ACCEPTED_200, left_out))
        assert left_out <= steps // 100
        # the replay on oracle values (tests/test_hyperj_host.py records its count): the two chains share uniforms and
        # proposals, so a decision differs only where log alpha is within rounding of log u4 -- the steps that may be left
        # out, 1 % at most -- and an independence chain is back in step at the next acceptance
        assert abs(accepted - host.ACCEPTED_200) <= steps // 100
    finally:
        L.stb_groups_free(h)
        L.stb_sampler_cache_clear()


def test_the_tiny_problems_chain_has_the_replays_acceptance_rate():
    """the chain of tests/test_hyperj_host.py (one restaurant, pairs (n, t) <= (12, 4), the same seed, start and 4000 steps)
    on the device.  Tolerance: the CPU test's own 0.005 = 20 steps; the chains share uniforms and proposals, a decision can
    differ only where log alpha is within rounding of log u4, and a differing decision is forgotten at the next acceptance"""
    L = capi.lib()
    n, t = host.N_PAIRS.astype(np.uint32), host.T_PAIRS.astype(np.uint16)
    K = np.array([len(n)], dtype=np.int32)
    T = np.array(host.T_REST, dtype=np.uint32)
    h = hpp._create(L, K, n, t, T, np.array([10.0]), int(n.max()), int(t.max()), host.D + 1)
    Nd = dev_u32(host.N_REST)
    a, b, acc, steps = 0.5, 10.0, 0, 4000
    try:
        for k in range(steps):
            r = capi.groups_samplejoint(h, Nd, host.RECT, a, b, host.SHAPE, host.SCALE, 20261, k, host.D, host.J)
            a, b = r["a"], r["b"]
            acc += r["accepted"]
        rate = acc / steps
        print("tiny problem on the device: %d stages, acceptance rate %.4f (replay %.4f)" % (r["stages"], rate, host.ACCEPT_RATE))
        assert abs(rate - host.ACCEPT_RATE) <= 0.005
    finally:
        L.stb_groups_free(h)
        L.stb_sampler_cache_clear()


# ---- object wrappers

def test_object_wrappers_equal_the_group_set_step():
    L = capi.lib()
    g = synth.groups(300, 10, 200, "realistic", seed=2)
    ti = capi.TableIndicators(g.K, g.n, g.t)
    tc = None
    h = L.stb_groups_create(g.I, orc.i32p(g.K), None, None, None, None, 0, 0, D + 1)
    h2 = None
    assert h, capi.last_error()
    try:
        a, b = 0.3, 5.0
        bpar = np.full(g.I, b)
        ti.sweep(a, bpar, 900, 0, 2)
        # (the set's bpar were never set: accepted -- the step does not read them)
        r1 = ti.samplejoint(h, RECT, a, b, SHAPE, SCALE, seed=5, sweep=3)
        t_now, T_now = ti.get()
        Nb, Mb = C.c_uint(), C.c_uint()
        assert L.stb_groups_shape(h, None, None, C.byref(Nb), C.byref(Mb), None) == 0
        h2 = L.stb_groups_create(g.I, orc.i32p(g.K), orc.u32p(T_now), orc.u32p(g.n), orc.u16p(t_now), orc.dp(bpar), Nb.value,
                                 Mb.value, D + 1)
        assert h2, capi.last_error()
        r2 = capi.groups_samplejoint(h2, dev_u32(g.N), RECT, a, b, SHAPE, SCALE, seed=5, sweep=3)
        assert r1 == r2, (r1, r2)
        # t and T are not written
        t2, T2 = ti.get()
        assert np.array_equal(t2, t_now) and np.array_equal(T2, T_now)
        # the table-count object holds N of its own
        tc = capi.TableCounts(g.K, g.n, t_now)
        r3 = tc.samplejoint(h, RECT, a, b, SHAPE, SCALE, seed=5, sweep=3)
        assert r3 == r1
        t3, T3 = tc.get()
        assert np.array_equal(t3, t_now) and np.array_equal(T3, T_now)
    finally:
        ti.free()
        if tc:
            tc.free()
        L.stb_groups_free(h)
        if h2:
            L.stb_groups_free(h2)
        L.stb_sampler_cache_clear()


# ---- refusals

def test_refusals_leave_the_state_as_it_was():
    L = capi.lib()
    g = synth.groups(40, 5, 50, "realistic", seed=1)
    Nd = dev_u32(g.N)
    N, M = int(g.n.max()), int(g.t.max())
    h = hpp._create(L, g.K, g.n, g.t, g.T, np.full(g.I, 2.0), N, M, D + 1)
    small = hpp._create(L, g.K, g.n, g.t, g.T, np.full(g.I, 2.0), N, M, D)
    uneven = hpp._create(L, g.K, g.n, g.t, g.T, np.where(np.arange(g.I) == 7, 3.0, 2.0), N, M, D + 1)
    ti = capi.TableIndicators(g.K, g.n, g.t)

    def call(hh, rect=RECT, a=0.5, b=10.0, Dg=D, fn=None, head=None):
        o = capi.JointOpts(rect[0], rect[1], rect[2], rect[3], Dg, J, SHAPE, SCALE, 1, 0, 0)
        ao, bo = C.c_double(-1.0), C.c_double(-2.0)
        info = capi.JointInfo()
        f = fn or L.stb_groups_samplejoint
        hd = head if head is not None else (hh, Nd.data_ptr())
        rc = f(*hd, C.byref(o), a, b, C.byref(ao), C.byref(bo), C.byref(info))
        return rc, ao.value, bo.value, capi.last_error()

    try:
        for rect in ((0.005, 0.97, 0.05, 500.0), (0.02, 0.99, 0.05, 500.0), (0.6, 0.6, 0.05, 500.0), (0.7, 0.3, 0.05, 500.0),
                     (0.02, 0.97, 0.001, 500.0), (0.02, 0.97, 0.05, 2500.0), (0.02, 0.97, 9.0, 9.0), (float("nan"), 0.97, 0.05, 500.0)):
            rc, ao, bo, msg = call(h, rect=rect)
            assert rc != 0 and "rectangle" in msg and (ao, bo) == (-1.0, -2.0), rect
        for a, b in ((0.01, 10.0), (0.975, 10.0), (0.5, 0.04), (0.5, 600.0), (float("nan"), 10.0)):
            rc, ao, bo, msg = call(h, a=a, b=b)
            assert rc != 0 and "outside the rectangle" in msg and (ao, bo) == (-1.0, -2.0), (a, b)
        rc, ao, bo, msg = call(small)
        assert rc != 0 and "Dmax" in msg and (ao, bo) == (-1.0, -2.0)
        rc, ao, bo, msg = call(None)
        assert rc != 0 and "null group set" in msg and (ao, bo) == (-1.0, -2.0)
        rc, ao, bo, msg = call(uneven)
        assert rc != 0 and "not all equal" in msg and (ao, bo) == (-1.0, -2.0)
        for fn, obj in ((L.stb_tindic_samplejoint, None), (L.stb_tcounts_samplejoint, None)):
            rc, ao, bo, msg = call(h, fn=fn, head=(obj, h))
            assert rc != 0 and "null object" in msg
        rc, ao, bo, msg = call(h, fn=L.stb_tindic_samplejoint, head=(ti.h, None))
        assert rc != 0 and "null object" in msg
        # a pair outside the set's table bounds: W(a) is log 0, L at the current state is not finite
        n2 = g.n.copy()
        n2[0] = N + 5
        outside = hpp._create(L, g.K, n2, g.t, g.T, np.full(g.I, 2.0), N, M, D + 1)
        rc, ao, bo, msg = call(outside)
        L.stb_groups_free(outside)
        assert rc != 0 and ("not finite" in msg or "non-finite" in msg) and (ao, bo) == (-1.0, -2.0), msg
        # and the set still works
        rc, ao, bo, msg = call(h)
        assert rc == 0 and RECT[0] <= ao <= RECT[1] and RECT[2] <= bo <= RECT[3], msg
    finally:
        ti.free()
        for hh in (h, small, uneven):
            L.stb_groups_free(hh)
        L.stb_sampler_cache_clear()


# ---- example

def test_example_runs_the_joint_loop():
    exe = os.path.join(ROOT, "examples", "bin", "pyp_resample")
    assert os.path.exists(exe), "examples/bin/pyp_resample not built (make -C libstb_amd/csrc)"
    p = subprocess.run([exe, "-j", "-J", "3", "-n", "2000", "-a", "0.4", "-b", "15", "-c", "45", "-s", "3"], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    print(p.stdout)
    m = re.search(r"^joint steps: (\d+) of (\d+) proposals accepted, last a=([0-9.]+) b=([0-9.]+)", p.stdout, re.M)
    assert m, p.stdout
    a, b = float(m.group(3)), float(m.group(4))
    assert int(m.group(2)) == 15 and 0.02 <= a <= 0.97 and 0.05 <= b <= 500.0
    m = re.search(r"posterior means after 45 sweeps: a=([0-9.]+) b=([0-9.]+); tables:", p.stdout)
    assert m and math.isfinite(float(m.group(1))) and math.isfinite(float(m.group(2))), p.stdout
