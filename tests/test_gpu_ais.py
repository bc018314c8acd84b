"""Annealed importance sampling for unseen documents on the device (stb_seat_anneal, stb_lik_temper,
stb_tindic_heldout_ais; libstb_amd/csrc/seat_ais.hip): every replica's final state bit for bit against the numpy replay
(tests/ais_oracle.py) given the tempered matrices the device itself made, lw, H_i and the total within the derived bars of
the 40-digit truth; the tempered cells against their truth; dead particles, restaurants that are left out, the object's
call, the launch geometry, the refusals, and the law on 20 000 copies of the restaurant tests/test_ais_host.py propagates
exactly."""
import math
import os

import numpy as np
import pytest

import ais_oracle as ao
import st_oracle as sto
import ti_oracle as tio
from libstb_amd import capi
from test_gpu_predict import dev, same_bits

pytestmark = pytest.mark.gpu

SENT_N, SENT_T, SENT_C, SENT_LW = 0x1234567, 0x4321, 0x7654321, -7.5


def table(a, N, M):
    """(the device V table for a at (N, M), its cells as an oracle VTab)"""
    v = capi.DeviceVTables(N, M)
    v.fill(a)
    capi.check(capi.lib().stb_fill_status())
    return v, tio.VTab(v.packed_host(0), N, M)


def bounds(coff, Mgiven):
    maxN = int(np.diff(np.asarray(coff, dtype=np.int64)).max()) if len(coff) > 1 else 0
    N = max(3, maxN)
    return N, min(Mgiven if Mgiven else max(maxN, 1), N)


def tempered(lik, S, betas=None):
    """the S - 1 matrices the sweeps read, fetched through stb_lik_temper"""
    d = dev(lik, np.float64)
    return [capi.lik_temper(d, be).cpu().numpy() for be in ao.ladder(S, betas)[:-1]]


def run(case, a, tabs, R, S, passes=1, betas=None, seed=ao.SEED, sweep=ao.SWEEP, G=None, C=None, bounds_=None):
    import torch

    K, h, bpar, coff, cls, lik = case
    koff = np.concatenate([[0], np.cumsum(np.asarray(K, dtype=np.int64))])
    I, G2, C2 = len(K), int(koff[-1]) * R, int(coff[-1]) * R
    info = torch.zeros(3, dtype=torch.int64, device="cuda")
    lw = torch.full((I, R), SENT_LW, dtype=torch.float64, device="cuda")
    pn = torch.full((max(G2, 1),), SENT_N, dtype=torch.int32, device="cuda")[:G2]
    pt = torch.full((max(G2, 1),), SENT_T, dtype=torch.int16, device="cuda")[:G2]
    pc = torch.full((max(C2, 1),), SENT_C, dtype=torch.int32, device="cuda")[:C2]
    rows, stride = lik.shape
    L = capi.lib()
    need = int(L.stb_seat_anneal_workspace_bytes(I, int(koff[-1]), int(coff[-1]), R, rows, stride))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    d = [dev(bpar, np.float64), dev(koff, np.uint64), None if h is None else dev(h, np.float64), dev(coff, np.uint64),
         dev(cls, np.uint32), dev(lik, np.float64)]
    bp = None
    if betas is not None:
        betas = np.ascontiguousarray(betas, dtype=np.float64)
        bp = capi.dp(betas)
    N, M = (tabs.N, tabs.M) if bounds_ is None else bounds_
    capi.check(L.stb_seat_anneal(None if tabs is None else tabs.tables.data_ptr(), N, M, float(a), d[0].data_ptr(), I,
                                 d[1].data_ptr(), None if d[2] is None else d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                                 d[5].data_ptr(), rows, stride, int(koff[-1]) if G is None else G,
                                 int(coff[-1]) if C is None else C, R, S, bp, passes, seed, sweep, lw.data_ptr(), pn.data_ptr(),
                                 pt.data_ptr(), pc.data_ptr(), info.data_ptr(), ws.data_ptr(), need, None))
    tot, Hi, si = capi.seat_loglik(lw)
    torch.cuda.synchronize()
    return {"lw": lw.cpu().numpy(), "pn": pn.cpu().numpy().view(np.uint32), "pt": pt.cpu().numpy().view(np.uint16),
            "pcust": pc.cpu().numpy().view(np.uint32), "Hi": Hi.cpu().numpy(), "total": tot, "dead_rows": int(si.impossible),
            "info": tuple(int(v) for v in info.cpu().numpy())}


def assert_against_replay(got, rep, tr, K, R, label):
    """the states bit for bit where a restaurant takes part; lw, H_i and the total within the bars"""
    ex = rep["ex"]
    act = rep["active"]
    pairs = np.zeros(ex["G2"], dtype=bool)
    for j in np.flatnonzero(act):
        pairs[ex["koff2"][j]:ex["koff2"][j] + ex["K2"][j]] = True
    assert np.array_equal(got["pn"][pairs], rep["pn"][pairs]), (label, "n")
    assert np.array_equal(got["pt"][pairs], rep["pt"][pairs]), (label, "t")
    assert np.array_equal(got["pcust"][rep["keep"]], rep["pcust"][rep["keep"]]), (label, "cust")
    for j in np.flatnonzero(act):                                  # T = sum t, and every customer counted at its dish
        sl = slice(int(ex["koff2"][j]), int(ex["koff2"][j] + ex["K2"][j]))
        assert int(got["pt"][sl].sum()) == int(rep["pT"][j]) and int(got["pn"][sl].sum()) == int(ex["N2"][j]), (label, j)
    assert got["info"] == (rep["skipped"], rep["dead"], rep["stuck"]), (label, got["info"])
    assert not np.isnan(got["lw"]).any() and not np.isnan(got["Hi"]).any()
    bar = np.where(tr["lw_bar"] > 0, tr["lw_bar"], 1.0)
    exact = (tr["lw_bar"] == 0) & np.isfinite(tr["lw"])
    assert np.array_equal(got["lw"][exact], tr["lw"][exact]), label     # no customers, or left out: 0 exactly
    worst = sto.over_bar(got["lw"], tr["lw"], bar)
    Hi, Hb, tot, tb = ao.finish(K, tr, R)
    worst_H = sto.over_bar(got["Hi"], Hi, np.where(Hb > 0, Hb, 1.0))
    print(label, "largest lw error over its bar", worst, "H_i", worst_H, "total", got["total"], tot, tb)
    assert worst <= 1.0 and worst_H <= 1.0, (label, worst, worst_H)
    assert sto.within(got["total"], tot, tb), (label, got["total"], tot, tb)


def check(case, a, Mgiven, R, S, passes, label, betas=None):
    K, h, bpar, coff, cls, lik = case
    N, M = bounds(coff, Mgiven)
    tabs, vt = table(a, N, M)
    got = run(case, a, tabs, R, S, passes, betas)
    rep = ao.replay(K, h, a, bpar, coff, cls, lik, tempered(lik, S, betas), vt, N, M, ao.SEED, ao.SWEEP, R, S, betas, passes,
                    bars=True)
    tr = ao.truth(K, h, a, bpar, coff, cls, lik, M, rep, R)
    assert_against_replay(got, rep, tr, K, R, label)
    return got, rep


# ---- 1. bits against the replay

@pytest.mark.parametrize("a,neg_b,M,R,S,passes", [(0.5, True, 0, 16, 2, 1), (0.9, True, 0, 3, 5, 2), (0.0, False, 0, 1, 1, 1),
                                                  (0.5, False, 2, 3, 2, 2), (0.0, False, 0, 3, 2, 1), (0.9, True, 2, 1, 5, 1)])
def test_mixed_shapes_in_one_call_equal_the_replay(a, neg_b, M, R, S, passes):
    case = ao.raw_case(a, neg_b)
    K, h, bpar, coff, cls, lik = case
    Nn = np.diff(coff.astype(np.int64))
    assert len(K) == 37 and set(ao.RAW_KS) <= set(K) and set(ao.RAW_NS) <= set(Nn) and (not neg_b or (bpar <= 0.0).any())
    got, rep = check(case, a, M, R, S, passes, "mix a=%g M=%d R=%d S=%d passes=%d" % (a, M, R, S, passes))
    assert rep["skipped"] == 0 and rep["dead"] == 0
    if M == 2:
        assert got["pt"].max() == 2                                    # the truncation binds
    if S == 1:                                                         # no sweep: importance sampling from the prior
        ex = rep["ex"]
        z = np.zeros(ex["G2"], dtype=np.int64)
        so = sto.replay(ex["K2"], z, z, ex["h2"], a, ex["bpar2"], np.concatenate([ex["coff2"], [ex["C2"]]]), M=bounds(coff, M)[1],
                        seed=ao.SEED, sweep=ao.SWEEP)
        assert np.array_equal(got["pcust"], so["cust"]) and np.array_equal(got["pn"], so["n"])
    else:
        one = run(case, a, table(a, *bounds(coff, M))[0], R, 1)
        assert not np.array_equal(one["pcust"], got["pcust"])          # the sweeps moved somebody


def first_restaurants(case, m):
    K, h, bpar, coff, cls, lik = case
    return K[:m], h[:int(K[:m].sum())], bpar[:m], coff[:m + 1], cls[:int(coff[m])], lik


def test_a_ladder_of_the_callers():
    check(first_restaurants(ao.raw_case(0.5), 9), 0.5, 0, 4, 4, 1, "own ladder", betas=(0.01, 0.3, 0.31, 1.0))


# ---- 2. the tempered cells

def test_tempered_cells_against_the_truth():
    sub = 2.0 ** -1074
    lik = np.array([[sub, 2.0 ** -1060, 2.2250738585072014e-308, 1.0, 0.0], [1.5, 1e300, 1e-300, 0.3, 7.25],
                    [0.0, 1.0, 2.0, 1.7976931348623157e308, 0.9999999999999999]])
    d = dev(lik, np.float64)
    for beta in (2.0 ** -20, 0.5, 1.0):
        got = capi.lik_temper(d, beta).cpu().numpy()
        want, bar = ao.temper_truth(lik, beta)
        assert np.array_equal(got == 0.0, lik == 0.0), beta           # 0 exactly where lik is 0, and nowhere else
        assert (got[lik == 1.0] == 1.0).all()
        worst = float((np.abs(got - want)[lik != 0] / bar[lik != 0]).max())
        print("beta", beta, "largest cell error over its bar", worst)
        assert worst <= 1.0, (beta, got, want, bar)


# ---- 3. dead particles

def test_dead_particles_are_counted_and_never_a_nan():
    K, h, bpar, coff, cls, lik = ao.host_case(0.5)
    lik = np.array(lik)
    lik[:, 0] = 0.0               # restaurant 0 has dish 0 alone: dead at the first increment, every particle of it
    lik[1, 1] = 0.0               # elsewhere the prior seating can hit a zero cell, and often does not
    case = (K, h, bpar, coff, cls, lik)
    R, S = 8, 3
    N, M = bounds(coff, 0)
    tabs, vt = table(0.5, N, M)
    got = run(case, 0.5, tabs, R, S)
    rep = ao.replay(K, h, 0.5, bpar, coff, cls, lik, tempered(lik, S), vt, N, M, ao.SEED, ao.SWEEP, R, S, bars=True)
    tr = ao.truth(K, h, 0.5, bpar, coff, cls, lik, M, rep, R)
    dead = rep["lw"] == -math.inf
    alld = dead.all(axis=1)
    part = dead.any(axis=1) & ~alld
    assert alld[0] and part.any() and not dead[3].any()           # a dead restaurant, half-dead ones, one without customers
    assert np.array_equal(got["lw"] == -math.inf, dead)
    assert got["info"][1] == int(dead.sum()) == rep["dead"]
    assert np.array_equal(got["Hi"] == -math.inf, alld) and np.isfinite(got["Hi"][~alld]).all() and got["total"] == -math.inf
    assert got["dead_rows"] == int(alld.sum())
    assert_against_replay(got, rep, tr, K, R, "dead")


# ---- 4. restaurants that are left out

def test_restaurants_that_are_left_out():
    rng = np.random.default_rng(0xA17)
    stride = 8
    # one of each kind among ordinary ones: K > STB_TD_MAXK, K > stride, no dishes with customers, N_i > the table's N
    K = np.array([3, capi.TD_MAXK + 1, 4, stride + 1, 0, 2, 5, 3], dtype=np.int32)
    Nn = np.array([6, 2, 9, 3, 2, 0, 11, 7])
    N, M = 10, 10
    coff = np.concatenate([[0], np.cumsum(Nn)]).astype(np.uint64)
    case = (K, 0.05 + rng.random(int(K.sum())), 0.5 + rng.random(len(K)), coff,
            rng.integers(0, 3, size=int(coff[-1])).astype(np.uint32), 0.05 + rng.random((3, stride)))
    K, h, bpar, coff, cls, lik = case
    R, S = 3, 3
    tabs, vt = table(0.4, N, M)
    got = run(case, 0.4, tabs, R, S)
    rep = ao.replay(K, h, 0.4, bpar, coff, cls, lik, tempered(lik, S), vt, N, M, ao.SEED, ao.SWEEP, R, S, bars=True)
    assert list(np.flatnonzero(rep["ex"]["skip"])) == [1, 3, 4, 6] and got["info"][0] == 4
    for i in (1, 3, 4, 6):
        assert (got["lw"][i] == 0.0).all() and got["Hi"][i] == 0.0, i
    # the customers of a restaurant that is left out are nobody's: its classes were never copied, its dishes never read
    koff = np.concatenate([[0], np.cumsum(K.astype(np.int64))])
    big = slice(int(koff[1]) * R, int(koff[2]) * R)
    assert (got["pn"][big] == SENT_N).all() and (got["pt"][big] == SENT_T).all()     # past the cap: not a pair addressed
    assert_against_replay(got, rep, ao.truth(K, h, 0.4, bpar, coff, cls, lik, M, rep, R), K, R, "left out")
    # G or C misstated: everybody is left out, nothing of the states is written
    for kw in ({"G": int(koff[-1]) - 1}, {"C": int(coff[-1]) + 1}):
        bad = run(case, 0.4, tabs, R, S, **kw)
        assert bad["info"] == (len(K), 0, 0) and not bad["lw"].any() and not bad["Hi"].any() and bad["total"] == 0.0
        assert (bad["pn"] == SENT_N).all() and (bad["pt"] == SENT_T).all() and (bad["pcust"] == SENT_C).all()


# ---- 5. the object

def object_of(case, Mgiven=0):
    K, h, bpar, coff, cls, lik = case
    G = int(np.sum(K))
    ti = capi.TableIndicators(K, np.zeros(G, dtype=np.uint32), np.zeros(G, dtype=np.uint16), h, None, Mgiven)
    ti.set_lik(lik)
    ti.set_heldout(coff, cls)
    return ti


@pytest.mark.parametrize("a,M,R,S,passes", [(0.5, 0, 4, 3, 2), (0.9, 2, 2, 2, 1)])
def test_the_objects_call_equals_the_raw_call(a, M, R, S, passes):
    rng = np.random.default_rng(0xA18)
    Ks = [1, 2, 63, 64, 5, 9, 33]                        # at most 64 dishes: the object takes the register forms
    Nn = [5, 0, 20, 65, 1, 64, 17]
    K = np.array(Ks, dtype=np.int32)
    coff = np.concatenate([[0], np.cumsum(Nn)]).astype(np.uint64)
    case = (K, 0.05 + rng.random(int(K.sum())), 0.3 + rng.random(len(K)), coff,
            rng.integers(0, 3, size=int(coff[-1])).astype(np.uint32), 0.05 + 2.0 * rng.random((3, 64)))
    N, Mt = bounds(coff, M)
    raw = run(case, a, table(a, N, Mt)[0], R, S, passes)
    ti = object_of(case, M)
    try:
        before = (ti.get(), ti.get_state(), ti.heldout_get())
        tot, Hi, info = ti.heldout_ais(a, case[2], R, S, ao.SEED, ao.SWEEP, passes=passes)
        assert same_bits(Hi, raw["Hi"]) and same_bits([tot], [raw["total"]])
        assert (info.skipped, info.dead, info.stuck, info.customers) == raw["info"] + (int(coff[-1]),)
        tot2, Hi2, _ = ti.heldout_ais(a, case[2], R, S, ao.SEED, ao.SWEEP, passes=passes)      # the kept table, not refilled
        assert same_bits(Hi2, Hi) and tot2 == tot
        after = (ti.get(), ti.get_state(), ti.heldout_get())
        for x, y in zip(before, after):
            for u, v in zip(x, y):
                assert np.array_equal(u, v)
        seq_tot, _, _ = ti.heldout_seq(a, case[2], R, ao.SEED, ao.SWEEP)                       # and the twins still run on it
        assert math.isfinite(seq_tot)
    finally:
        ti.free()


def test_the_object_refuses_what_it_must():
    rng = np.random.default_rng(0xA19)
    K = np.array([2, 3], dtype=np.int32)
    coff = np.array([0, 3, 5], dtype=np.uint64)
    cls = np.array([0, 1, 0, 1, 1], dtype=np.uint32)
    lik = 0.1 + rng.random((2, 3))
    full = capi.TableIndicators(K, np.array([1, 0, 0, 2, 0], dtype=np.uint32), np.array([1, 0, 0, 1, 0], dtype=np.uint16))
    empty = object_of((K, None, None, coff, cls, lik))
    nolik = capi.TableIndicators(K, np.zeros(5, dtype=np.uint32), np.zeros(5, dtype=np.uint16))
    try:
        full.set_lik(lik)
        full.set_heldout(coff, cls)
        with pytest.raises(capi.StbError, match="customers of its own"):
            full.heldout_ais(0.5, 1.0, 2, 2, 1, 0)
        nolik.set_heldout(coff, cls)
        with pytest.raises(capi.StbError, match="no likelihood"):
            nolik.heldout_ais(0.5, 1.0, 2, 2, 1, 0)
        for kw, words in (({"S": 0}, "S=0"), ({"passes": 0}, "passes"), ({"particles": 0}, "particles"),
                          ({"particles": 4097}, "particles"), ({"betas": (0.5, 0.5)}, "betas"), ({"betas": (0.5, 0.9)}, "1.0"),
                          ({"a": 1.0}, "discount")):
            args = {"a": 0.5, "particles": 2, "S": 2, "passes": 1, "betas": None, **kw}
            with pytest.raises(capi.StbError, match=words):
                empty.heldout_ais(args["a"], 1.0, args["particles"], args["S"], 1, 0, betas=args["betas"], passes=args["passes"])
        tot, Hi, info = empty.heldout_ais(0.5, 1.0, 2, 2, 1, 0)
        assert math.isfinite(tot) and info.customers == 5
    finally:
        for o in (full, empty, nolik):
            o.free()


def test_the_raw_call_refuses_what_it_must():
    case = ao.host_case(0.5)
    K, h, bpar, coff, cls, lik = case
    N, M = bounds(coff, 0)
    tabs, _ = table(0.5, N, M)
    for kw, words in (({"S": 0}, "S=0"), ({"passes": 0}, "passes"), ({"R": 0}, "particles"), ({"R": 4097}, "particles"),
                      ({"betas": (0.0, 1.0)}, "betas"), ({"betas": (0.7, 0.6, 1.0), "S": 3}, "betas"),
                      ({"betas": (0.5, 1.0000000000000002)}, "betas"), ({"betas": (0.25, 0.5)}, "1.0"), ({"a": -0.5}, "discount"),
                      ({"bounds_": (N, 0)}, "bounds"), ({"bounds_": (N, 65536)}, "M=")):
        args = {"a": 0.5, "R": 2, "S": 2, "passes": 1, "betas": None, "bounds_": None, **kw}
        with pytest.raises(capi.StbError, match=words):
            run(case, args["a"], tabs, args["R"], args["S"], args["passes"], args["betas"], bounds_=args["bounds_"])
    import torch

    d_lik = dev(lik, np.float64)
    koff = dev(np.concatenate([[0], np.cumsum(K.astype(np.int64))]), np.uint64)
    with pytest.raises(capi.StbError, match="matrix and the classes"):
        capi.check(capi.lib().stb_seat_anneal(tabs.tables.data_ptr(), N, M, 0.5, dev(bpar, np.float64).data_ptr(), len(K),
                                              koff.data_ptr(), None, dev(coff, np.uint64).data_ptr(), None, d_lik.data_ptr(), 3, 6,
                                              int(K.sum()), int(coff[-1]), 2, 2, None, 1, 0, 0,
                                              torch.zeros(2 * len(K), dtype=torch.float64, device="cuda").data_ptr(), None, None, None,
                                              None, torch.zeros(1 << 16, dtype=torch.uint8, device="cuda").data_ptr(), 1 << 16, None))
    with pytest.raises(capi.StbError, match="workspace"):
        capi.seat_anneal(tabs, 0.5, dev(bpar, np.float64), koff, dev(coff, np.uint64), dev(cls, np.uint32), d_lik, dev(h, np.float64),
                         2, 2, ws=torch.zeros(64, dtype=torch.uint8, device="cuda"))


# ---- 6. the launch geometry

def test_the_bits_do_not_depend_on_the_launch_geometry():
    # STB_AIS_WAVES is read at every launch; 600 restaurants x 8 particles is more replicas than a grid of one wave a
    # workgroup has workgroups, so at 1 (and only there) the waves take a second replica
    a, R, S = 0.5, 8, 3
    base = ao.raw_case(a)
    K, h, bpar, coff, cls, lik = base
    small = [i for i in range(len(K)) if K[i] <= 65 and coff[i + 1] - coff[i] <= 65][:12]
    koff = np.concatenate([[0], np.cumsum(K.astype(np.int64))])
    reps = 50
    Kb = np.tile(K[small], reps)
    hb = np.tile(np.concatenate([h[koff[i]:koff[i + 1]] for i in small]), reps)
    Nb = np.tile(np.array([int(coff[i + 1] - coff[i]) for i in small]), reps)
    clsb = np.tile(np.concatenate([cls[int(coff[i]):int(coff[i + 1])] for i in small]), reps)
    big = (Kb.astype(np.int32), hb, np.tile(bpar[small], reps), np.concatenate([[0], np.cumsum(Nb)]).astype(np.uint64), clsb, lik)
    assert len(Kb) * R > 4096
    N, M = bounds(big[3], 0)
    tabs, _ = table(a, N, M)
    old = os.environ.get("STB_AIS_WAVES")
    out = {}
    try:
        for w in (1, 2, 4, 8):
            os.environ["STB_AIS_WAVES"] = str(w)
            out[w] = run(big, a, tabs, R, S)
    finally:
        if old is None:
            os.environ.pop("STB_AIS_WAVES", None)
        else:
            os.environ["STB_AIS_WAVES"] = old
    dflt = run(big, a, tabs, R, S)
    for w in (1, 2, 8):
        for f in ("lw", "Hi"):
            assert same_bits(out[w][f], out[4][f]), (w, f)
        for f in ("pn", "pt", "pcust"):
            assert np.array_equal(out[w][f], out[4][f]), (w, f)
        assert out[w]["info"] == out[4]["info"] and out[w]["total"] == out[4]["total"]
    assert same_bits(dflt["lw"], out[4]["lw"])
    # with other restaurants sharing the launch: everybody but the first twelve gets other weights, classes and
    # concentrations (the offsets, so the flat indices and C', stay) -- the twelve keep their bits
    rng = np.random.default_rng(0xA1A)
    k12, c12 = int(Kb[:12].sum()), int(big[3][12])
    h2, b2, cls2 = hb.copy(), big[2].copy(), clsb.copy()
    h2[k12:] = 0.05 + rng.random(len(h2) - k12)
    b2[12:] = 0.5 + rng.random(len(b2) - 12)
    cls2[c12:] = rng.integers(0, ao.RAW_ROWS, size=len(cls2) - c12)
    other = run((big[0], h2, b2, big[3], cls2, lik), a, tabs, R, S)
    assert same_bits(other["lw"][:12], dflt["lw"][:12]) and same_bits(other["Hi"][:12], dflt["Hi"][:12])
    assert np.array_equal(other["pn"][:k12 * R], dflt["pn"][:k12 * R]) and np.array_equal(other["pt"][:k12 * R], dflt["pt"][:k12 * R])
    assert np.array_equal(other["pcust"][:c12 * R], dflt["pcust"][:c12 * R])
    assert not np.array_equal(other["pcust"][c12 * R:], dflt["pcust"][c12 * R:])


# ---- 7. the law

def test_the_mean_weight_of_20000_copies_is_p_w():
    K, h, bpar, coff, cls, lik = ao.law_case()
    want = float(sto.ujoint_states(ao.LAW_NC, ao.LAW_K, ao.LAW_H, ao.LAW_A, ao.LAW_B, ao.LAW_CLS, ao.LAW_LIK).sum())
    tabs, vt = table(ao.LAW_A, 3, 3)
    got = run(ao.law_case(), ao.LAW_A, tabs, 1, 4, 1, ao.LAW_BETAS, seed=ao.LAW_SEED, sweep=ao.LAW_SWEEP)
    mean, tol, off = ao.law_statistic(got["lw"], want)
    print("mean weight", mean, "p(w)", want, "5 sd / sqrt(n)", tol)
    assert got["info"] == (0, 0, 0)
    assert off <= tol, (mean, want, tol)
    # the same statistic from the replay that takes the increment after the sweep: rejected
    af = ao.replay(K, h, ao.LAW_A, bpar, coff, cls, lik, tempered(lik, 4, ao.LAW_BETAS), vt, 3, 3, ao.LAW_SEED, ao.LAW_SWEEP, 1, 4,
                   ao.LAW_BETAS, 1, mut="after")
    mean, tol, off = ao.law_statistic(af["lw"], want)
    assert off > tol, (mean, want, tol)
    # and the device walked the right replay's path on every copy the wrong one shares its seating with
    assert np.array_equal(got["pcust"], af["pcust"]) and not same_bits(got["lw"], af["lw"])
