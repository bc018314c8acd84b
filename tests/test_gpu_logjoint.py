"""The log joint probability of a sampler state on the device (stb_logjoint, stb_tcounts_logjoint, stb_tindic_logjoint;
libstb_amd/csrc/logjoint.hip) against the high-precision truth and the bar of tests/lj_oracle.py -- derived there from
the kernel's own operations --, across launch geometries, on inputs built to trigger every counter, on the two objects,
and with refused arguments.  Shapes: tables N = 48 with M = 48 and M = 7; restaurants of 0, 1, 63, 64, 65 and 129 pairs
(the chunk edges) and sets of 1, 255, 256, 257 and 513 restaurants (the block edges); tiled states of 1031 types past one
trip per workgroup, past the 1024 block sums the last workgroup stages at a time and past the block sums first
allocated, every size taken from stb_reduce_geometry."""
import ctypes as C
import math
import os
from functools import lru_cache

import numpy as np
import pytest

import hj_oracle as hj
import lj_oracle as lj
import orc
from libstb_amd import capi

pytestmark = pytest.mark.gpu
N48 = 48
A_ALL = [0.0, 0.125, 0.5, 0.9]
K_EDGES = [0, 1, 63, 64, 65, 129]


def dev(a, dtype):
    import torch

    a = np.ascontiguousarray(a, dtype=dtype)
    view = {np.uint32: np.int32, np.uint16: np.int16, np.uint64: np.int64}.get(dtype)
    return torch.as_tensor(a.view(view) if view else a, device="cuda")


class waves:
    """STB_LOGJOINT_WAVES for the calls inside"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        self.old = os.environ.get("STB_LOGJOINT_WAVES")
        os.environ["STB_LOGJOINT_WAVES"] = str(self.v)

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("STB_LOGJOINT_WAVES", None)
        else:
            os.environ["STB_LOGJOINT_WAVES"] = self.old


def b_values(I, a):
    """b_i over 1e-3, 1, 1e3 -- and -0.25 at a = 0.5"""
    vals = [1e-3, 1.0, 1e3] + ([-0.25] if a == 0.5 else [])
    return np.array([vals[i % len(vals)] for i in range(I)])


def make_state(K, M, seed):
    """a valid state on the CSR shape K: n = 0 (t = 0), n = 1, t = 1, t = n and the interior all occur; n <= 48 and
    t <= min(n, M) or t = n"""
    rng = np.random.default_rng(seed)
    K = np.asarray(K, dtype=np.int32)
    G = int(K.sum())
    n = rng.integers(0, N48 + 1, size=G).astype(np.uint32)
    kind = rng.integers(0, 5, size=G)
    tm = np.minimum(n, M)
    t = np.where(n > 0, 1 + np.floor(rng.random(G) * tm), 0).astype(np.int64)
    t = np.where((kind == 0) & (n > 0), 1, t)
    t = np.where((kind == 1) & (n > 0), n, t)
    n = np.where(kind == 2, 1, n).astype(np.uint32)
    t = np.where(kind == 2, 1, t).astype(np.uint16)
    h = 0.05 + 0.95 * rng.random(G)
    h[::7] = 1.0
    return K, n, t, h


@lru_cache(maxsize=None)
def device_tables(a, M):
    tabs = capi.DeviceTables(N48, M)
    tabs.fill(a)
    tabs.status()
    return tabs


@lru_cache(maxsize=None)
def truth_tables(a, M):
    return lj.Tables(a, N48, M)


def run_raw(tabs, a, bpar, K, n, t, h, indicators=False, T=None, want_Li=True, flags=None):
    import torch

    koff = np.concatenate([[0], np.cumsum(K)]).astype(np.uint64)
    tot, Li, info = capi.logjoint(tabs, a, dev(bpar, np.float64), dev(koff, np.uint64), dev(n if len(n) else [0], np.uint32),
                                  dev(t if len(t) else [0], np.uint16), None if T is None else dev(T, np.uint32),
                                  None if h is None else dev(h if len(h) else [1.0], np.float64), indicators, want_Li,
                                  flags=flags)
    torch.cuda.synchronize()
    return tot, None if Li is None else Li.cpu().numpy(), info


def check_against(tr, tot, Li, info, indicators, what):
    print(what, "total", tot, "truth", tr["total"][0], "bar", tr["total"][1])
    assert not np.isnan(Li).any() and not math.isnan(tot)
    for i in range(len(Li)):
        assert lj.within(float(Li[i]), float(tr["Li"][i]), float(tr["Li_bar"][i])), (what, i, Li[i], tr["Li"][i], tr["Li_bar"][i])
    for name in ("pairs", "base", "restaurants", "binom"):
        got = getattr(info, name)
        want, bar = tr[name]
        print(what, name, got, want, bar)
        assert not math.isnan(got)
        assert lj.within(got, want, bar), (what, name, got, want, bar)
    if not indicators:
        assert info.binom == 0.0
    assert lj.within(tot, tr["total"][0], tr["total"][1]), (what, tot, tr["total"])
    assert info.outside == tr["outside"] and info.impossible == tr["impossible"]


# ---- the chunk edges, every discount, both tables, both flag values, with and without h

@pytest.mark.parametrize("with_h", [False, True])
@pytest.mark.parametrize("indicators", [False, True])
@pytest.mark.parametrize("M", [48, 7])
@pytest.mark.parametrize("a", A_ALL)
def test_chunk_edges_against_the_truth(a, M, indicators, with_h):
    K, n, t, h = make_state(K_EDGES, M, seed=101 + M)
    h = h if with_h else None
    bpar = b_values(len(K), a)
    tr = lj.truth(K, n, t, h, a, bpar, truth_tables(a, M), indicators)
    tot, Li, info = run_raw(device_tables(a, M), a, bpar, K, n, t, h, indicators, T=tr["T"])
    check_against(tr, tot, Li, info, indicators, f"a={a} M={M} ind={indicators} h={with_h}")
    assert info.outside == 0 and info.impossible == 0 and info.t_mismatch == 0
    assert Li[0] == 0.0  # (a restaurant without pairs)


# ---- the block edges, restaurants without customers among them

def block_state(I, M, seed):
    rng = np.random.default_rng(seed)
    K = rng.integers(0, 4, size=I).astype(np.int32)
    K, n, t, h = make_state(K, M, seed + 1)
    koff = np.concatenate([[0], np.cumsum(K)])
    for i in range(0, I, 5):  # restaurants whose pairs all have n = 0: N_i = 0 with K_i > 0
        n[koff[i]:koff[i + 1]] = 0
        t[koff[i]:koff[i + 1]] = 0
    return K, n, t, h


@pytest.mark.parametrize("I", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("a,M,indicators,with_h", [(0.5, 48, True, True), (0.0, 7, False, False)])
def test_block_edges_against_the_truth(I, a, M, indicators, with_h):
    K, n, t, h = block_state(I, M, seed=7 * I + M)
    h = h if with_h else None
    bpar = b_values(I, a)
    tr = lj.truth(K, n, t, h, a, bpar, truth_tables(a, M), indicators)
    assert I < 5 or (tr["Nc"] == 0).sum() >= I // 5
    tot, Li, info = run_raw(device_tables(a, M), a, bpar, K, n, t, h, indicators, T=tr["T"])
    check_against(tr, tot, Li, info, indicators, f"I={I} a={a} M={M}")
    assert info.outside == 0 and info.impossible == 0 and info.t_mismatch == 0
    assert (Li[tr["Nc"] == 0] == 0.0).all()


# ---- launch geometry

@pytest.mark.parametrize("shape", ["chunks", "blocks"])
def test_the_same_bits_for_every_workgroup_size(shape):
    a, M = 0.5, 7
    K, n, t, h = make_state(K_EDGES, M, 5) if shape == "chunks" else block_state(513, M, 6)
    bpar = b_values(len(K), a)
    ref = None
    for wv in (1, 2, 4, 8, 0):
        with waves(wv):
            tot, Li, info = run_raw(device_tables(a, M), a, bpar, K, n, t, h, True)
        got = (np.float64(tot).tobytes(), Li.tobytes(), bytes(info))
        ref = got if ref is None else ref
        assert got == ref, wv
    # the total does not depend on whether the L_i are asked for
    tot2, none, info2 = run_raw(device_tables(a, M), a, bpar, K, n, t, h, True, want_Li=False)
    assert none is None and (np.float64(tot2).tobytes(), bytes(info2)) == (ref[0], ref[2])


# ---- the counters

def test_counters_are_exact_and_impossible_pairs_give_minus_infinity():
    a, M = 0.5, 7
    K = np.array([4, 5, 3, 2, 70], dtype=np.int32)
    n = np.concatenate([[60, 60, 20, 5], [5, 5, 0, 9, 9], [6, 6, 6], [12, 12], np.full(70, 10)]).astype(np.uint32)
    t = np.concatenate([[3, 60, 10, 2], [0, 6, 2, 9, 1], [2, 3, 1], [8, 3], np.full(70, 3)]).astype(np.uint16)
    h = np.ones(len(n))
    h[9:12] = [0.0, -1.0, math.inf]
    h[14 + 69] = math.nan
    bpar = np.array([1.0, 2.0, 0.5, 3.0, 1e3])
    tr = lj.truth(K, n, t, h, a, bpar, truth_tables(a, M), True)
    # outside: n = 60 twice, t = 10 > M, t = 8 > M; impossible: t = 0, t = 6 > n = 5, n = 0 with t = 2, four bad h
    assert tr["outside"] == 4 and tr["impossible"] == 7
    T = tr["T"].copy()
    T[0] += 1
    T[3] -= 1
    tot, Li, info = run_raw(device_tables(a, M), a, bpar, K, n, t, h, True, T=T)
    assert (info.outside, info.impossible, info.t_mismatch) == (4, 7, 2)
    assert not np.isnan(Li).any()
    assert list(np.isneginf(Li)) == [False, True, True, False, True]
    assert tot == -math.inf and info.pairs == -math.inf and info.base == -math.inf
    assert math.isfinite(info.restaurants) and math.isfinite(info.binom)
    for i in (0, 3):  # the kernel's own sum of t is the one used
        assert lj.within(float(Li[i]), float(tr["Li"][i]), float(tr["Li_bar"][i]))
    assert lj.within(info.restaurants, *tr["restaurants"])
    # without d_T nothing is compared
    _, _, info = run_raw(device_tables(a, M), a, bpar, K, n, t, h, False)
    assert info.t_mismatch == 0 and info.binom == 0.0


def test_without_a_table_and_at_b_zero():
    # no slab and no S1 vector: pairs with n <= 1, and M = 1 with larger n (S^n_1 evaluated in place)
    a = 0.5
    K = np.array([3, 2, 0, 4], dtype=np.int32)
    n = np.array([1, 0, 1, 1, 1, 30, 2, 48, 1], dtype=np.uint32)
    t = np.array([1, 0, 1, 1, 1, 1, 1, 1, 1], dtype=np.uint16)
    h = np.linspace(0.2, 1.0, len(n))
    bpar = np.array([1.0, -0.25, 5.0, 0.0])  # (b = 0 takes the limit)
    tabs = lj.Tables(a, N48, 1, with_table=False)
    for ind in (False, True):
        tr = lj.truth(K, n, t, h, a, bpar, tabs, ind)
        tot, Li, info = run_raw((N48, 1), a, bpar, K, n, t, h, ind, T=tr["T"])
        check_against(tr, tot, Li, info, ind, "no table")
        assert info.outside == 0 and info.t_mismatch == 0 and math.isfinite(tot)
    # an interior pair cannot be answered without a table
    n2, t2 = n.copy(), t.copy()
    n2[5], t2[5] = 30, 4
    _, _, info = run_raw((N48, 48), a, bpar, K, n2, t2, h)
    assert info.outside == 1


# ---- the objects

def object_state(M):
    rng = np.random.default_rng(31)
    K = np.concatenate([[0, 1, 65], rng.integers(1, 12, size=37)]).astype(np.int32)
    return make_state(K, M, 32)


@pytest.mark.parametrize("kind", ["tcounts", "tindic"])
def test_objects_equal_the_raw_call_and_leave_the_state_alone(kind):
    L = capi.lib()
    M = N48
    K, n, t, h = object_state(M)
    t = np.where(n > 0, np.minimum(t, n), 0).astype(np.uint16)
    I = len(K)
    a, b = 0.5, 2.0
    bpar = np.full(I, b)
    obj = capi.TableCounts(K, n, t, h) if kind == "tcounts" else capi.TableIndicators(K, n, t, h)
    g = L.stb_groups_create(I, orc.i32p(K), None, None, None, None, 0, 0, 2)
    assert g, capi.last_error()
    try:
        obj.sweep(a, bpar, 77, 0, 3)
        for ind in (False, True):
            tot, Li, info = obj.logjoint(a, bpar, ind)
            t_now, T_now = obj.get()
            Nobj = max(int(n.max()), 3)
            tabs = capi.DeviceTables(Nobj, min(M, Nobj) if kind == "tindic" else int(n.max()))
            tabs.fill(a)
            tabs.status()
            tot_r, Li_r, info_r = run_raw(tabs, a, bpar, K, n, t_now, h, ind, T=T_now)
            assert np.float64(tot).tobytes() == np.float64(tot_r).tobytes()
            assert Li.tobytes() == Li_r.tobytes() and bytes(info) == bytes(info_r)
            assert info.t_mismatch == 0 and info.outside == 0 and info.impossible == 0
            # against the truth as well
            tr = lj.truth(K, n, t_now, h, a, bpar, lj.Tables(a, Nobj, tabs.M), ind)
            check_against(tr, tot, Li, info, ind, kind)
            # the state is unchanged
            t2, T2 = obj.get()
            assert np.array_equal(t2, t_now) and np.array_equal(T2, T_now)
        # the pair sum and the restaurant terms the library already had, within the two sides' bars
        obj.to_groups(g, bpar)
        W = capi.groups_ssum(g, [a])[0]
        _, wbar = hj.W_truth_bar([a], n, t_now)
        assert abs(info.pairs - W) <= tr["pairs"][1] + wbar[0], (info.pairs, W)
        Ncust = tr["Nc"]
        R = float(capi.joint_terms([a], [b], dev(T_now, np.uint32), dev(Ncust, np.uint32)).cpu().numpy()[0, 0])
        _, rbar = hj.R_points_truth([a], [b], T_now, Ncust)
        assert abs(info.restaurants - R) <= tr["restaurants"][1] + rbar[0], (info.restaurants, R)
        # a second call at a new discount refills the table
        a2 = 0.125
        tot2, Li2, info2 = obj.logjoint(a2, bpar, True)
        tr2 = lj.truth(K, n, t_now, h, a2, bpar, lj.Tables(a2, Nobj, tabs.M), True)
        check_against(tr2, tot2, Li2, info2, True, kind + " refilled")
        assert tot2 != tot
        # ... and back, with Li_host NULL
        tot3, none, info3 = obj.logjoint(a, bpar, True, want_Li=False)
        assert none is None and tot3 == tot and bytes(info3) == bytes(info)
        # refused: the state stays as it was
        for bad in (lambda: obj.logjoint(1.0, bpar), lambda: obj.logjoint(-0.1, bpar),
                    lambda: obj.logjoint(a, np.full(I, -0.6)), lambda: obj.logjoint(a, np.full(I, math.nan))):
            with pytest.raises(capi.StbError):
                bad()
        fn = L.stb_tcounts_logjoint if kind == "tcounts" else L.stb_tindic_logjoint
        tt, inf = C.c_double(1.5), capi.LogJointInfo()
        assert fn(obj.h, a, capi.dp(bpar), 2, C.byref(tt), None, C.byref(inf)) != 0 and b"flags" in L.stb_last_error()
        assert fn(obj.h, a, None, 0, C.byref(tt), None, C.byref(inf)) != 0
        assert fn(None, a, capi.dp(bpar), 0, C.byref(tt), None, C.byref(inf)) != 0
        assert tt.value == 1.5
        t4, T4 = obj.get()
        assert np.array_equal(t4, t_now) and np.array_equal(T4, T_now)
        tot5, _, _ = obj.logjoint(a, bpar, True)
        assert tot5 == tot
    finally:
        obj.free()
        L.stb_groups_free(g)
        L.stb_sampler_cache_clear()


@pytest.mark.parametrize("kind", ["tcounts", "tindic"])
def test_objects_without_a_table_read_none(kind):
    # every n <= 1; and M = 1 with larger n: every t is 1, S^n_1 is evaluated in place
    a, bpar = 0.9, np.array([1.0, 1e-3, 1e3])
    K = np.array([2, 3, 1], dtype=np.int32)
    for n, M in ((np.array([1, 0, 1, 1, 0, 1], dtype=np.uint32), 0), (np.array([5, 0, 48, 2, 1, 17], dtype=np.uint32), 1)):
        t = (n > 0).astype(np.uint16)
        obj = capi.TableCounts(K, n, t, None, M) if kind == "tcounts" else capi.TableIndicators(K, n, t, None, None, M)
        try:
            obj.sweep(a, bpar, 3, 0, 2)
            tot, Li, info = obj.logjoint(a, bpar, True)
            tr = lj.truth(K, n, t, None, a, bpar, lj.Tables(a, N48, 1, with_table=False), True)
            check_against(tr, tot, Li, info, True, f"{kind} M={M}")
            assert info.t_mismatch == 0 and info.outside == 0
        finally:
            obj.free()


def test_the_indicator_objects_slab_follows_the_discount():
    # one object asked at a = 0.3, 0.6 and 0.3 again: every answer is a fresh object's at that discount, bit for bit --
    # the S slab is refilled when the discount changes, neither kept stale nor taken for another discount's
    K = np.array([2, 3], dtype=np.int32)
    n = np.array([6, 1, 4, 2, 5], dtype=np.uint32)
    t = np.array([2, 1, 3, 1, 2], dtype=np.uint16)
    h = np.array([0.5, 1.25, 2.0, 0.75, 1.5])
    bpar = np.array([1.5, 0.25])

    def ask(obj, a):
        tot, Li, info = obj.logjoint(a, bpar, True)
        return np.float64(tot).tobytes(), Li.tobytes(), bytes(info)

    one = capi.TableIndicators(K, n, t, h)
    try:
        seen = []
        for a in (0.3, 0.6, 0.3):
            fresh = capi.TableIndicators(K, n, t, h)
            try:
                want = ask(fresh, a)
            finally:
                fresh.free()
            seen.append(ask(one, a))
            assert seen[-1] == want, a
        assert seen[0] != seen[1] and seen[0] == seen[2]
    finally:
        one.free()


# ---- past one trip per workgroup: tiled states, restaurant i of type i mod P_TYPES (the truth once per type)

P_TYPES = 1031  # prime: no two blocks a workgroup takes hold the same restaurants in the same slots
CONFIGS = [(0.5, 7, True, True), (0.0, 48, False, False)]  # (a, M, indicators, with h)
LJ_CASES = ["tail", "two trips", "stage 1024", "stage 1025", "stage 2049"]


def lj_geom(I, wv=0):
    return capi.reduce_geometry(capi.GEOM_LOGJOINT, I, waves=wv)


def lj_width():
    """the workgroups of a launch with more blocks than the device takes at once"""
    return lj_geom(1 << 30).grid_x


def lj_case(label):
    """(I, its premise, asserted through the query) -- every size from the geometry of the device at hand"""
    W = lj_width()
    if label == "tail":  # one workgroup takes a one-restaurant tail block after a full one
        I = W * 256 + 1
        g = lj_geom(I)
        assert (g.grid_x, g.steps, g.blocks) == (W, W + 1, W + 1) and g.chunks == 1
    elif label == "two trips":  # two or three trips a workgroup, the last block of 129 restaurants
        I = (2 * W + 2) * 256 + 129
        g = lj_geom(I)
        assert g.grid_x == W and g.steps == 2 * g.grid_x + 3
    elif label == "regrow":  # one block sum more than the buffer first allocated holds
        I = int(lj_geom(1).cap0) * 256 + 1
        g = lj_geom(I)
        assert g.need == g.cap0 + 1 and g.need == g.blocks
    else:  # the edges of the last workgroup's staging loop (LJ_STAGE = 1024 block sums a round)
        nblk = int(label.split()[1])
        I = {1024: 1024 * 256, 1025: 1024 * 256 + 1, 2049: 2048 * 256 + 77}[nblk]
        assert lj_geom(I).blocks == nblk
    return I


def type_state(M, seed):
    """P_TYPES restaurants of 0 .. 3 pairs, four of 65 and 129, every fifth without customers (block_state's kinds)"""
    rng = np.random.default_rng(seed)
    K = rng.integers(0, 4, size=P_TYPES).astype(np.int32)
    K[[11, 401, 777, 1029]] = [65, 129, 65, 129]
    K, n, t, h = make_state(K, M, seed + 1)
    koff = np.concatenate([[0], np.cumsum(K)])
    for i in range(0, P_TYPES, 5):
        n[koff[i]:koff[i + 1]] = 0
        t[koff[i]:koff[i + 1]] = 0
    return K, n, t, h


def type_mult(I, first=0):
    """how often each type occurs among I restaurants, restaurant i of type (first + i) mod P_TYPES"""
    return np.roll(I // P_TYPES + (np.arange(P_TYPES) < I % P_TYPES), first)


def first_for(I, last_type=1029):
    """the type to start the tiling at for the last of I restaurants to be of `last_type` (129 pairs): a one-restaurant tail
    block then weighs in every sum"""
    return (last_type - (I - 1)) % P_TYPES


class Tiled:
    """the types tiled to I restaurants, restaurant i of type (first + i) mod P_TYPES, on the device once"""

    def __init__(self, K, n, t, h, bpar, T, I, first=0):
        assert 0 <= first < P_TYPES
        reps = -(-I // P_TYPES) + 1
        self.I, self.reps, self.first = I, reps, first
        kofft = np.concatenate([[0], np.cumsum(np.tile(K, reps), dtype=np.int64)])
        g0, g1 = int(kofft[first]), int(kofft[first + I])
        self.koff = dev((kofft[first:first + I + 1] - g0).astype(np.uint64), np.uint64)
        self.n, self.t = dev(np.tile(n, reps)[g0:g1], np.uint32), dev(np.tile(t, reps)[g0:g1], np.uint16)
        self.h = None if h is None else dev(np.tile(h, reps)[g0:g1], np.float64)
        self.b = dev(self.tile(bpar), np.float64)
        self.T = dev(self.tile(T), np.uint32)

    def run(self, tabs, a, indicators, want_Li=True):
        import torch

        tot, Li, info = capi.logjoint(tabs, a, self.b, self.koff, self.n, self.t, self.T, self.h, indicators, want_Li)
        torch.cuda.synchronize()
        return tot, None if Li is None else Li.cpu().numpy(), info

    def tile(self, x):
        return np.tile(x, self.reps)[self.first:self.first + self.I]


@lru_cache(maxsize=None)
def clean_types(cfg):
    """the types of a configuration, their per-type truth, and the device's L_i of the P_TYPES alone -- held to the truth"""
    a, M, indicators, with_h = CONFIGS[cfg]
    K, n, t, h = type_state(M, seed=900 + cfg)
    h = h if with_h else None
    bpar = b_values(P_TYPES, a)
    assert set(K) >= {0, 1, 2, 3, 65, 129} and (a != 0.5 or (bpar < 0).any())
    per = lj.per_restaurant(K, n, t, h, a, bpar, truth_tables(a, M), indicators)
    assert (per["Nc"] == 0).sum() >= P_TYPES // 5
    tr = lj.tiled(per)
    tot, Li, info = run_raw(device_tables(a, M), a, bpar, K, n, t, h, indicators, T=tr["T"])
    check_against(tr, tot, Li, info, indicators, f"types a={a} M={M}")
    assert info.outside == 0 and info.impossible == 0 and info.t_mismatch == 0
    return (K, n, t, h, bpar), per, Li


def check_totals(tr, tot, info, what):
    """the four components and the total within the bar of the tiled truth"""
    worst = 0.0
    for name, got in (("pairs", info.pairs), ("base", info.base), ("restaurants", info.restaurants), ("binom", info.binom),
                      ("total", tot)):
        want, bar = tr[name]
        ratio = 0.0 if got == want else abs(got - want) / bar if bar > 0 else math.inf
        worst = max(worst, ratio)
        print("%s %s: %.17g, truth %.17g, bar %.3e, error / bar %.3g" % (what, name, got, want, bar, ratio))
        assert not math.isnan(got) and lj.within(got, want, bar), (what, name, got, want, bar)
    print("%s: worst error / bar %.3g" % (what, worst))


def same_bits_for_every_workgroup_size(tl, tabs, a, indicators, ref):
    for wv in (1, 2, 4, 8, 0):
        with waves(wv):
            tot, Li, info = tl.run(tabs, a, indicators)
        assert (np.float64(tot).tobytes(), Li.tobytes(), bytes(info)) == ref, wv
    tot, none, info = tl.run(tabs, a, indicators, want_Li=False)
    assert none is None and (np.float64(tot).tobytes(), bytes(info)) == (ref[0], ref[2])


@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("label", LJ_CASES)
def test_tiled_states_past_one_trip_per_workgroup(label, cfg):
    a, M, indicators, with_h = CONFIGS[cfg]
    I = lj_case(label)
    same = [x for x in LJ_CASES[:LJ_CASES.index(label)] if lj_case(x) == I]
    if same:   # the same restaurants as an earlier case on this device, which ran the checks; both premises hold
        print("%s: I=%d is the case %r on this device, nothing more is run here" % (label, I, same[0]))
        return
    (K, n, t, h, bpar), per, Li_types = clean_types(cfg)
    first = first_for(I) if I % 256 == 1 else 0   # (a tail block of one restaurant: one with 129 pairs)
    tl = Tiled(K, n, t, h, bpar, per["T"], I, first)
    tabs = device_tables(a, M)
    tot, Li, info = tl.run(tabs, a, indicators)
    # (i) every restaurant has the bits of its type
    assert np.array_equal(Li.view(np.uint64), tl.tile(Li_types.view(np.uint64)))
    assert I % 256 != 1 or (K[(first + I - 1) % P_TYPES] == 129 and Li[-1] != 0.0)
    # (ii) the sums against the tiled truth
    check_totals(lj.tiled(per, type_mult(I, first)), tot, info, f"{label} I={I} a={a} M={M}")
    assert info.outside == 0 and info.impossible == 0 and info.t_mismatch == 0
    if not indicators:
        assert info.binom == 0.0
    # (iii) the same bytes for every workgroup size, and without the L_i
    same_bits_for_every_workgroup_size(tl, tabs, a, indicators, (np.float64(tot).tobytes(), Li.tobytes(), bytes(info)))


@pytest.mark.parametrize("cfg", [0, 1])
def test_a_call_that_outgrows_the_block_sums_and_the_calls_after_it(cfg):
    a, M, indicators, with_h = CONFIGS[cfg]
    I = lj_case("regrow")
    (K, n, t, h, bpar), per, Li_types = clean_types(cfg)
    tabs = device_tables(a, M)
    capi.lib().stb_sampler_cache_clear()  # (this thread's buffer of block sums: the next call allocates cap0 afresh)
    small = Tiled(K, n, t, h, bpar, per["T"], 257)
    tot_s, Li_s, info_s = small.run(tabs, a, indicators)
    check_totals(lj.tiled(per, type_mult(257)), tot_s, info_s, f"I=257 a={a} M={M}")
    first = first_for(I)
    big = Tiled(K, n, t, h, bpar, per["T"], I, first)
    tot, Li, info = big.run(tabs, a, indicators)   # replaces the buffer
    assert np.array_equal(Li.view(np.uint64), big.tile(Li_types.view(np.uint64))) and Li[-1] != 0.0
    check_totals(lj.tiled(per, type_mult(I, first)), tot, info, f"regrow I={I} a={a} M={M}")
    assert info.outside == 0 and info.impossible == 0 and info.t_mismatch == 0
    ref = (np.float64(tot).tobytes(), Li.tobytes(), bytes(info))
    tot2, Li2, info2 = small.run(tabs, a, indicators)   # a smaller call in the larger buffer
    assert (np.float64(tot2).tobytes(), Li2.tobytes(), bytes(info2)) == (np.float64(tot_s).tobytes(), Li_s.tobytes(), bytes(info_s))
    same_bits_for_every_workgroup_size(big, tabs, a, indicators, ref)   # ... and the first call again


def test_counters_accumulate_over_a_workgroups_trips():
    """types with impossible pairs, outside pairs and d_T off by one among the clean ones: the counts are the sums of
    multiplicity x the type's, the sums -inf and never NaN, and a clean type keeps its bits (no flag left from a trip)"""
    a, M, indicators = 0.5, 7, True
    (K, n, t, h, bpar), _, Li_clean = clean_types(0)
    n, t, h = n.copy(), t.copy(), h.copy()
    koff = np.concatenate([[0], np.cumsum(K)])
    have = [i for i in range(P_TYPES) if K[i] >= 1]
    kinds = ["t > n", "t = 0 < n", "h = 0", "h < 0", "n > N", "t > M"]
    changed = {}
    for j, i in enumerate(have[3::9][:60]):
        g = koff[i] + (K[i] - 1) * (j % 2)   # the type's first pair, or its last
        kind = kinds[j % len(kinds)]
        n[g], t[g], h[g] = {"t > n": (5, 6, 1.0), "t = 0 < n": (9, 0, 0.5), "h = 0": (6, 2, 0.0), "h < 0": (4, 4, -1.0),
                            "n > N": (60, 3, 0.5), "t > M": (20, 10, 0.5)}[kind]
        changed[i] = kind
    per = lj.per_restaurant(K, n, t, h, a, bpar, truth_tables(a, M), indicators)
    off = np.zeros(P_TYPES, dtype=np.int64)   # d_T off by one, on types with and without pairs, clean and not
    off[2::50] = 1
    off[27::50] = -1
    off[min(changed)] = 1
    off[per["T"] + off < 0] = 1
    clean = np.array([i not in changed for i in range(P_TYPES)])
    assert (off[clean] != 0).sum() >= 10 and (off[~clean] != 0).sum() >= 1 and (K[off != 0] == 0).any()
    # the types alone, held to the truth
    tr1 = lj.tiled(per)
    assert tr1["outside"] == 20 and tr1["impossible"] == 40
    tot1, Li_types, info1 = run_raw(device_tables(a, M), a, bpar, K, n, t, h, indicators, T=per["T"] + off)
    check_against(tr1, tot1, Li_types, info1, indicators, "counter types")
    assert info1.t_mismatch == (off != 0).sum()
    imp = (per["imp_p"] + per["imp_h"]) > 0
    assert np.array_equal(np.isneginf(Li_types), imp) and np.isfinite(Li_types[~imp]).all()
    assert np.array_equal(Li_types[clean].view(np.uint64), Li_clean[clean].view(np.uint64))
    # tiled past two trips a workgroup
    I = lj_case("two trips")
    mult = type_mult(I)
    tr = lj.tiled(per, mult)
    tl = Tiled(K, n, t, h, bpar, per["T"] + off, I)
    ref = None
    for wv in (0, 1, 8):
        with waves(wv):
            tot, Li, info = tl.run(device_tables(a, M), a, indicators)
        assert info.outside == tr["outside"] == int((mult * per["out"]).sum()) and info.outside >= 20 * (I // P_TYPES)
        assert info.impossible == tr["impossible"] and info.t_mismatch == int((mult * (off != 0)).sum())
        assert not np.isnan(Li).any() and not any(math.isnan(x) for x in (tot, info.pairs, info.base, info.restaurants, info.binom))
        assert tot == -math.inf and info.pairs == -math.inf and info.base == -math.inf
        assert lj.within(info.restaurants, *tr["restaurants"]) and lj.within(info.binom, *tr["binom"])
        assert np.array_equal(Li.view(np.uint64), tl.tile(Li_types.view(np.uint64)))
        got = (Li.tobytes(), bytes(info))
        ref = got if ref is None else ref
        assert got == ref, wv
    assert np.isfinite(Li[tl.tile(~imp)]).all()


@pytest.mark.parametrize("kind", ["tcounts", "tindic"])
def test_objects_at_a_second_trip_equal_the_raw_calls(kind):
    """an object of gx * 256 + 1 restaurants (K_i <= 1, n <= 3: nothing to sweep): its log joint has the bits of the raw call,
    and its b step's Q -- the customers as d_coff prefix sums for stb_tindic -- the bits of stb_sample_logq on d_N"""
    L = capi.lib()
    I = lj_case("tail")
    rng = np.random.default_rng(77)
    K = (rng.random(I) < 0.8).astype(np.int32)
    G = int(K.sum())
    n = rng.integers(1, 4, size=G).astype(np.uint32)
    t = (1 + np.floor(rng.random(G) * n)).astype(np.uint16)
    h = 0.05 + 0.95 * rng.random(G)
    assert n.max() == 3 and (t <= n).all() and (t == 2).any() and (K == 0).any()
    a, b = 0.5, 2.0
    bpar = np.full(I, b)
    koff = np.concatenate([[0], np.cumsum(K)])
    Ncust = np.zeros(I, dtype=np.int64)
    Ncust[K > 0] = n
    Tsum = np.zeros(I, dtype=np.int64)
    Tsum[K > 0] = t
    obj = capi.TableCounts(K, n, t, h) if kind == "tcounts" else capi.TableIndicators(K, n, t, h)
    try:
        tabs = capi.DeviceTables(3, 3)
        tabs.fill(a)
        tabs.status()
        for ind in (False, True):
            tot, Li, info = obj.logjoint(a, bpar, ind)
            tot_r, Li_r, info_r = run_raw(tabs, a, bpar, K, n, t, h, ind, T=Tsum)
            assert np.float64(tot).tobytes() == np.float64(tot_r).tobytes()
            assert Li.tobytes() == Li_r.tobytes() and bytes(info) == bytes(info_r)
            assert info.t_mismatch == 0 and info.outside == 0 and info.impossible == 0 and math.isfinite(tot)
        t2, T2 = obj.get()
        assert np.array_equal(t2, t) and np.array_equal(T2, Tsum)
        # the b step's Q
        assert capi.reduce_geometry(capi.GEOM_LOGQ, I).steps > capi.reduce_geometry(capi.GEOM_LOGQ, I).grid_x
        orc.seed_libc(3, 4)
        bn = obj.sampleb(b, 1.1, 20.0, a, seed=515, sweep=6)
        Q = L.stb_sampleb_last_Q()
        Qr, _ = capi.sample_logq(b, 20.0, dev(Ncust, np.uint32), seed=515, sweep=6, want_L=False)
        assert 0.01 <= bn <= 2000 and Q == Qr and math.isfinite(Q) and Q > 1 / 20.0
    finally:
        obj.free()
        L.stb_sampler_cache_clear()


def test_one_thread_interleaves_the_ticket_families():
    """the five per-thread sets of the ticket kernels (csrc/ticket.h) next to each other in one thread, at 257 restaurants:
    one full block and a block of one restaurant, the smallest launch in which the ticket decides anything.  Every call alone
    behind a stb_sampler_cache_clear, then the five back to back, then in the reverse order: the same bytes every time (no
    state passes between the sets), and a set dropped twice is made again whole."""
    import torch

    L = capi.lib()
    I = 257
    a, M, indicators, _ = CONFIGS[0]
    (K, n, t, h, bpar), per, _ = clean_types(0)
    tabs = device_tables(a, M)
    tl = Tiled(K, n, t, h, bpar, per["T"], I)
    Nd = dev(tl.tile(per["Nc"]), np.uint32)
    for which in (capi.GEOM_LOGQ, capi.GEOM_JOINT_TERMS, capi.GEOM_LOGJOINT):
        g = capi.reduce_geometry(which, I, 3, 2)
        assert g.blocks == 2 and g.grid_x == 2, which
    rng = np.random.default_rng(611)
    p, hoff = dev(0.01 + rng.random(I), np.float64), dev(np.arange(I + 1), np.uint64)
    b0 = np.repeat([0.7, 5.0], [100, I - 100])   # (a group's restaurants share its concentration)
    kend = int(np.cumsum(K)[I - 1])
    obj = capi.TableCounts(K[:I], n[:kend], t[:kend])
    obj.set_bgroups(np.array([0, 100, I], dtype=np.uint64))

    def logq():
        Q, Lt = capi.sample_logq(0.7, 20.0, Nd, seed=31, sweep=2)
        assert math.isfinite(Q) and Q > 1 / 20.0
        return np.float64(Q).tobytes(), Lt.cpu().numpy().tobytes()

    def terms():
        R = capi.joint_terms([0.2, 0.5, 0.8], [0.5, 3.0], tl.T, Nd)
        torch.cuda.synchronize()
        R = R.cpu().numpy()
        assert R.shape == (3, 2) and np.isfinite(R).all() and (R != 0.0).all()
        return (R.tobytes(),)

    def logjoint():
        tot, Li, info = tl.run(tabs, a, indicators)
        assert math.isfinite(tot) and info.impossible == 0
        return np.float64(tot).tobytes(), Li.tobytes(), bytes(info)

    def heldout():
        tot, Hi, info = capi.heldout_loglik(p, hoff)
        torch.cuda.synchronize()
        assert math.isfinite(tot) and info.customers == I
        return np.float64(tot).tobytes(), Hi.cpu().numpy().tobytes(), bytes(info)

    def bstep():
        obj.set_bpar(b0)
        bg, info = obj.sampleb_groups(a, 1.1, 20.0, seed=41, sweep=3)
        assert info.kept_groups == 0 and np.isfinite(bg).all() and (bg > 0).all()
        return bg.tobytes(), bytes(info), obj.get_bpar().tobytes()

    calls = [logq, terms, logjoint, heldout, bstep]
    try:
        alone = []
        for f in calls:
            L.stb_sampler_cache_clear()
            alone.append(f())
        forward = [f() for f in calls]
        backward = [f() for f in reversed(calls)][::-1]
        for f, x, y, z in zip(calls, alone, forward, backward):
            assert x == y and x == z, f.__name__
        L.stb_sampler_cache_clear()
        L.stb_sampler_cache_clear()
        assert logq() == alone[0]
    finally:
        obj.free()
        L.stb_sampler_cache_clear()


# ---- refusals of the raw call

def test_the_raw_call_refuses_before_anything_is_queued():
    import torch

    L = capi.lib()
    a, M = 0.5, 7
    K, n, t, h = make_state([3, 2], M, 1)
    tabs = device_tables(a, M)
    koff = dev(np.array([0, 3, 5]), np.uint64)
    nd, td, bd = dev(n, np.uint32), dev(t, np.uint16), dev([1.0, 2.0], np.float64)
    tot, info = C.c_double(2.5), capi.LogJointInfo()

    def call(a=a, flags=0, koff=koff.data_ptr(), nn=nd.data_ptr(), tt=td.data_ptr(), I=2):
        return L.stb_logjoint(tabs.tables.data_ptr(), tabs.S1.data_ptr(), N48, M, a, bd.data_ptr(), I, koff, nn, tt, None, None,
                              flags, None, C.byref(tot), C.byref(info), None)

    for kw, word in (({"a": 1.0}, b"discount"), ({"a": -0.5}, b"discount"), ({"a": math.nan}, b"discount"),
                     ({"flags": 2}, b"flags"), ({"flags": 0x80000001}, b"flags"), ({"koff": None}, b"required"),
                     ({"nn": None}, b"required"), ({"tt": None}, b"required"), ({"I": -1}, b"I=-1")):
        assert call(**kw) != 0, kw
        assert word in L.stb_last_error(), (kw, L.stb_last_error())
        assert tot.value == 2.5
    assert call(I=0) == 0 and tot.value == 0.0 and info.pairs == 0.0 and info.outside == 0
    assert call() == 0 and math.isfinite(tot.value)
    torch.cuda.synchronize()
