"""The forward seating as a particle filter on the device (stb_seat_filter, stb_tindic_heldout_pf; libstb_amd/csrc/
seat_pf.hip): every slot's final pairs, the weights, the exponent and the resampling counts bit for bit against the numpy
replay (tests/pf_oracle.py), H_i within the derived bar of the 40-digit truth; the same bits whatever the waves of a
workgroup; the existing kernel when nothing is resampled; dead restaurants, dead particles, the budget, the refusals and
the object's call.  The law itself is judged on the CPU (tests/test_pf_host.py).  A workgroup's second and third
restaurant, past the grid's cap, are tests/test_gpu_pf_geometry.py's."""
import hashlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import pf_oracle as pf
import st_oracle as sto
from libstb_amd import capi
from test_gpu_predict import dev, same_bits
from test_gpu_tdish import assert_state, fetch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT_W, SENT_E, SENT_RES, SENT_N, SENT_T, SENT_H = -7.5, -12345, 0x7BCD, 0x1234567, 0x4321, 99.25


def run_pf(case, a, M, R, tau, seed=pf.SEED, sweep=pf.SWEEP):
    """stb_seat_filter on host arrays into outputs filled with sentinels: a dict of host arrays Hi, w, E, res, pn, pt, the
    five counters (info), the start state after the call (n, t) and the device Hi"""
    import torch

    K, n, t, h, bpar, coff, cls, lik = case
    koff = np.concatenate([[0], np.cumsum(np.asarray(K, dtype=np.int64))])
    I, G = len(K), int(koff[-1]) * R
    d_n, d_t = dev(n, np.uint32), dev(t, np.uint16)
    info = torch.zeros(5, dtype=torch.int64, device="cuda")
    out = {"Hi": torch.full((I,), SENT_H, dtype=torch.float64, device="cuda"),
           "w": torch.full((I, R), SENT_W, dtype=torch.float64, device="cuda"),
           "E": torch.full((I,), SENT_E, dtype=torch.int64, device="cuda"),
           "res": torch.full((I,), SENT_RES, dtype=torch.int32, device="cuda"),
           "pn": torch.full((max(G, 1),), SENT_N, dtype=torch.int32, device="cuda")[:G],
           "pt": torch.full((max(G, 1),), SENT_T, dtype=torch.int16, device="cuda")[:G]}
    capi.seat_filter(a, dev(bpar, np.float64), dev(koff, np.uint64), d_n, d_t, dev(coff, np.uint64),
                     None if h is None else dev(h, np.float64), M, None if cls is None else dev(cls, np.uint32),
                     None if lik is None else dev(lik, np.float64), R, tau, seed, sweep, info=info, out=out)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["res"], got["pn"], got["pt"] = got["res"].view(np.uint32), got["pn"].view(np.uint32), got["pt"].view(np.uint16)
    got.update({"info": tuple(int(v) for v in info.cpu().numpy()), "n": d_n.cpu().numpy().view(np.uint32),
                "t": d_t.cpu().numpy().view(np.uint16), "d_Hi": out["Hi"]})
    return got


def assert_bits(got, rep, case, R, label):
    """the device's outputs against the replay's: bit for bit, a skipped restaurant's still the sentinels (H_i = 0)"""
    K, n, t = case[0], case[1], case[2]
    koff = np.concatenate([[0], np.cumsum(np.asarray(K, dtype=np.int64))])
    assert np.array_equal(got["n"], n) and np.array_equal(got["t"], t), label      # the start state is only read
    for i in range(len(K)):
        sl = slice(int(koff[i]) * R, int(koff[i + 1]) * R)
        if rep["skip"][i]:
            assert got["Hi"][i] == 0.0 and np.all(got["w"][i] == SENT_W) and got["E"][i] == SENT_E, (label, i)
            assert got["res"][i] == SENT_RES and np.all(got["pn"][sl] == SENT_N) and np.all(got["pt"][sl] == SENT_T), (label, i)
            continue
        assert np.array_equal(got["pn"][sl], rep["pn"][sl]) and np.array_equal(got["pt"][sl], rep["pt"][sl]), (label, i)
        assert same_bits(got["w"][i], rep["w"][i]), (label, i, got["w"][i], rep["w"][i])
        assert got["E"][i] == rep["E"][i] and got["res"][i] == rep["res"][i], (label, i)
    assert got["info"] == (rep["skipped"], rep["impossible"], rep["stuck"], rep["dead"], rep["resamplings"]), (label, got["info"])
    assert not np.isnan(got["Hi"]).any()


def assert_H(got, rep, Ht, Hb, label):
    """H_i within the bar of the truth where it was taken; elsewhere within two bars of the replay's (both lie within one
    of the truth)"""
    worst = 0.0
    for i in range(len(Ht)):
        if rep["skip"][i]:
            continue
        if math.isnan(Ht[i]):
            assert abs(got["Hi"][i] - rep["H"][i]) <= 2.0 * Hb[i], (label, i, got["Hi"][i], rep["H"][i], Hb[i])
        else:
            assert sto.within(got["Hi"][i], Ht[i], Hb[i]), (label, i, got["Hi"][i], Ht[i], Hb[i])
            if Hb[i] > 0:
                worst = max(worst, abs(got["Hi"][i] - Ht[i]) / Hb[i])
    print(label, "largest H error over its bar", worst)


def check(case, a, M, R, tau, exact, label, want_res=False):
    K, n, t, h, bpar, coff, cls, lik = case
    rep, Ht, Hb = pf.truth(K, n, t, h, a, bpar, coff, cls, lik, M, pf.SEED, pf.SWEEP, R, tau, restaurants=exact)
    got = run_pf(case, a, M, R, tau)
    assert_bits(got, rep, case, R, label)
    assert_H(got, rep, Ht, Hb, label)
    assert not want_res or rep["resamplings"] >= 3, (label, rep["resamplings"])
    assert tau > 0.0 or rep["resamplings"] == 0
    return got, rep


# ---- 1. bits against the replay

MIX_EXACT = [i for i, (k, c) in enumerate(pf.mix_shapes()) if k * c <= 65 * 10 and c > 0]     # where the truth is taken


@pytest.mark.parametrize("a,M,tau", [(0.5, 0, 0.5), (0.0, 0, 1.0), (0.9, 2, 0.5), (0.5, 0, 0.0)])
def test_mixed_shapes_in_one_launch_equal_the_replay(a, M, tau):
    case = pf.mix_case(a)
    K, n, t, h, bpar, coff, cls, lik = case
    assert len(K) == 37 and set(pf.MIX_K) <= set(K) and set(pf.MIX_C) <= set(np.diff(coff.astype(np.int64)))
    assert n.any() and (a == 0.0 or (bpar <= 0.0).any()) and all(3 <= capi.seat_filter_budget(int(k)) for k in K)
    got, rep = check(case, a, M, 3, tau, MIX_EXACT, "mix a=%g M=%d tau=%g" % (a, M, tau), want_res=tau > 0.0)
    assert rep["skipped"] == 0 and got["info"][0] == 0
    if M == 2:                                                     # the truncation binds
        assert rep["pt"].max() <= max(2, int(t.max()))


@pytest.mark.parametrize("R,shapes,tau", [
    (1, [(1, 3), (2, 65), (64, 64), (65, 5), (130, 4), (5, 0)], 1.0),
    (2, [(1, 3), (2, 65), (64, 64), (65, 5), (130, 4), (5, 0)], 1.0),
    (64, [(1, 5), (64, 12), (80, 12), (2, 0), (63, 1)], 1.0),
    (39, [(130, 10), (65, 10), (63, 3)], 0.5),                      # the budget's limit for K = 130
])
def test_particle_counts_up_to_the_budget_equal_the_replay(R, shapes, tau):
    assert capi.seat_filter_budget(130) == pf.budget(130) == 39 and capi.seat_filter_budget(64) == 64
    assert all(capi.seat_filter_budget(k) == pf.budget(k) for k in (0, 1, 2, 63, 64, 65, 80, 81, 128, 130, 1024, 5000))
    assert all(R <= capi.seat_filter_budget(k) for k, _ in shapes)
    case = pf.make_case(shapes, 0.5, 4321 + R)
    exact = [i for i, (k, c) in enumerate(shapes) if k <= 65 and 0 < c <= 12]
    got, rep = check(case, 0.5, 0, R, tau, exact, "R=%d" % R, want_res=R >= 3)
    assert rep["skipped"] == 0 and got["info"][0] == 0
    if R == 2:
        assert rep["resamplings"] > 0                                   # tau = 1: whenever the two weights differ


# ---- 2. the geometry

def _digest():
    hsh = hashlib.sha256()
    for a, M, R, tau, case in ((0.5, 0, 3, 0.5, pf.mix_case(0.5)), (0.5, 0, 64, 0.5, pf.make_case([(64, 12), (80, 12), (1, 5)], 0.5, 8)),
                               (0.5, 0, 39, 1.0, pf.make_case([(130, 10), (65, 10)], 0.5, 9))):
        got = run_pf(case, a, M, R, tau)
        for f in ("pn", "pt", "w", "E", "res", "Hi"):
            hsh.update(np.ascontiguousarray(got[f]).tobytes())
        hsh.update(repr(got["info"]).encode())
    return hsh.hexdigest()


def test_the_bits_do_not_depend_on_the_waves_of_a_workgroup():
    # a fresh process per setting, the four at once
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    procs = {w: subprocess.Popen([sys.executable, os.path.abspath(__file__), "--digest"], env=dict(env, STB_SEAT_WAVES=str(w)),
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for w in (1, 2, 4, 8)}
    out = {}
    for w, p in procs.items():
        so, se = p.communicate(timeout=120)
        assert p.returncode == 0, (w, se[-2000:])
        out[w] = so.strip().splitlines()[-1]
    assert len(out[4]) == 64 and len(set(out.values())) == 1, out
    assert out[4] == _digest()                                          # and this process, at the default


# ---- 3. against the existing kernel

def test_one_particle_that_never_resamples_is_the_committed_seating():
    import torch

    a = 0.5
    case = pf.make_case([(1, 9), (2, 65), (63, 20), (64, 64), (65, 12), (130, 7), (4, 0)], a, 55)
    K, n, t, h, bpar, coff, cls, lik = case
    koff = np.concatenate([[0], np.cumsum(K)])
    got = run_pf(case, a, 0, 1, 0.0)
    d_n, d_t = dev(n, np.uint32), dev(t, np.uint16)
    lw, T, cust, p = capi.seat_customers(a, dev(bpar, np.float64), dev(koff, np.uint64), d_n, d_t, dev(coff, np.uint64),
                                         dev(h, np.float64), 0, dev(cls, np.uint32), dev(lik, np.float64), 1, True, pf.SEED, pf.SWEEP)
    torch.cuda.synchronize()
    assert np.array_equal(got["pn"], d_n.cpu().numpy().view(np.uint32)) and np.array_equal(got["pt"], d_t.cpu().numpy().view(np.uint16))
    assert got["info"] == (0, 0, 0, 0, 0)
    sr = sto.replay(K, n, t, h, a, bpar, coff, cls, lik, 0, pf.SEED, pf.SWEEP, 1, bars=True)
    tr = sto.truth(K, n, t, h, a, bpar, coff, cls, lik, 0, sr)
    _, _, Hb = pf.truth(K, n, t, h, a, bpar, coff, cls, lik, 0, pf.SEED, pf.SWEEP, 1, 0.0, restaurants=[])
    lw = lw.cpu().numpy()[:, 0]
    for i in range(len(K)):         # one truth, each estimate within its own bar of it
        assert sto.within(lw[i], tr["lw"][i, 0], tr["lw_bar"][i, 0]) and sto.within(got["Hi"][i], tr["lw"][i, 0], Hb[i]), i
        assert abs(got["Hi"][i] - lw[i]) <= tr["lw_bar"][i, 0] + Hb[i], (i, got["Hi"][i], lw[i])
    # the total is stb_seat_loglik's on one particle a restaurant: H = m exactly
    tot, Hi, _ = capi.seat_loglik(got["d_Hi"].reshape(-1, 1))
    assert same_bits(Hi.cpu().numpy(), got["Hi"]) and tot == sto.loglik_total(got["Hi"])


# ---- 4. dead and impossible

def test_a_class_without_likelihood_kills_its_restaurant_and_no_other():
    a, R, tau = 0.5, 3, 0.5
    shapes = [(5, 20), (64, 20), (3, 20), (65, 20)]
    K, n, t, h, bpar, coff, cls, lik = pf.make_case(shapes, a, 66, rows=6, dead_class=5)
    cls = np.where(cls == 5, 0, cls).astype(np.uint32)
    alive_case = (K, n, t, h, bpar, coff, cls.copy(), lik)
    cls[int(coff[2]) + 9] = 5                                           # mid-document, restaurant 2
    case = (K, n, t, h, bpar, coff, cls, lik)
    got, rep = check(case, a, 0, R, tau, [0, 1, 3], "dead")
    assert rep["dead"] == 1 and got["info"][3] == 1 and got["info"][1] == R and got["Hi"][2] == -math.inf
    assert not got["w"][2].any() and np.all(np.isfinite(got["Hi"][[0, 1, 3]]))
    tot, _, sinfo = capi.seat_loglik(got["d_Hi"].reshape(-1, 1))
    assert tot == -math.inf and sinfo.impossible == 1
    # the other restaurants of the launch are untouched: the same bits as without the dead class
    ref = run_pf(alive_case, a, 0, R, tau)
    koff = np.concatenate([[0], np.cumsum(K)])
    for i in (0, 1, 3):
        sl = slice(int(koff[i]) * R, int(koff[i + 1]) * R)
        assert np.array_equal(got["pn"][sl], ref["pn"][sl]) and same_bits(got["w"][i], ref["w"][i]) and got["Hi"][i] == ref["Hi"][i]
    assert math.isfinite(ref["Hi"][2])
    # the customers behind the dead one were still seated: every slot holds the start's customers and all twenty
    sl = slice(int(koff[2]) * R, int(koff[3]) * R)
    assert np.all(got["pn"][sl].reshape(R, 3).sum(axis=1) == int(n[koff[2]:koff[3]].sum()) + 20)


def test_a_dead_particle_is_never_an_ancestor():
    case = pf.partial_case()
    K, n, t, h, bpar, coff, cls, lik = case
    R, seed = 4, 1
    rep = pf.replay(K, n, t, h, 0.5, bpar, coff, cls, lik, 0, seed, 0, R, 1.0, trace=True)
    st = rep["steps"][0][1]
    lost = [r for r in range(R) if not st["kept"][r]]
    assert 0 < len(lost) < R and st["resampled"] and not set(st["anc"]) & set(lost), (lost, st.get("anc"))
    got = run_pf(case, 0.5, 0, R, 1.0, seed=seed, sweep=0)
    assert_bits(got, rep, case, R, "partial")
    assert got["info"][1] == 0 and got["info"][3] == 0 and math.isfinite(got["Hi"][0])
    _, Ht, Hb = pf.truth(K, n, t, h, 0.5, bpar, coff, cls, lik, 0, seed, 0, R, 1.0)
    assert sto.within(got["Hi"][0], Ht[0], Hb[0]), (got["Hi"][0], Ht[0], Hb[0])


# ---- 5. over the budget, refusals

def test_a_restaurant_over_the_budget_is_skipped_and_counted():
    a, tau = 0.5, 0.5
    R = capi.seat_filter_budget(130) + 1
    shapes = [(128, 6), (130, 6), (64, 6), (1024, 2), (2, 6)]
    assert [R <= capi.seat_filter_budget(k) for k, _ in shapes] == [True, False, True, False, True]
    case = pf.make_case(shapes, a, 91)
    got, rep = check(case, a, 0, R, tau, [2, 4], "over budget")
    assert list(rep["skip"]) == [False, True, False, True, False] and got["info"][0] == 2
    # the others' bits are what they are without it
    K, n, t, h, bpar, coff, cls, lik = case
    koff = np.concatenate([[0], np.cumsum(K)])
    keep = np.concatenate([np.arange(koff[i], koff[i + 1]) for i in (0, 2, 4)])
    K2 = np.array([128, 0, 64, 0, 2], dtype=np.int32)                  # (no dishes, customers: skipped; c and C stay)
    alone = run_pf((K2, n[keep], t[keep], h[keep], bpar, coff, cls, lik), a, 0, R, tau)
    assert alone["info"][0] == 2
    o = 0
    for i in (0, 2, 4):
        sl = slice(int(koff[i]) * R, int(koff[i + 1]) * R)
        s2 = slice(o * R, (o + int(K[i])) * R)
        o += int(K[i])
        assert np.array_equal(got["pn"][sl], alone["pn"][s2]) and np.array_equal(got["pt"][sl], alone["pt"][s2]), i
        assert same_bits(got["w"][i], alone["w"][i]) and got["Hi"][i] == alone["Hi"][i] and got["E"][i] == alone["E"][i], i


def test_refusals_leave_the_outputs_untouched():
    import torch

    case = pf.make_case([(3, 4), (5, 2)], 0.5, 3)
    K, n, t, h, bpar, coff, cls, lik = case
    for kw in (dict(a=1.0), dict(a=-0.1), dict(R=0), dict(R=65), dict(R=4097), dict(tau=-0.01), dict(tau=1.5), dict(tau=math.nan),
               dict(M=65536)):
        args = dict(a=0.5, M=0, R=2, tau=0.5)
        args.update(kw)
        with pytest.raises(capi.StbError):
            run_pf(case, args["a"], args["M"], args["R"], args["tau"])
    koff = dev(np.concatenate([[0], np.cumsum(K)]), np.uint64)
    d = dict(bpar=dev(bpar, np.float64), n=dev(n, np.uint32), t=dev(t, np.uint16), coff=dev(coff, np.uint64),
             cls=dev(cls, np.uint32), lik=dev(lik, np.float64))
    Hi = torch.full((2,), SENT_H, dtype=torch.float64, device="cuda")
    w = torch.full((2, 2), SENT_W, dtype=torch.float64, device="cuda")
    L = capi.lib()

    def raw(a=0.5, bp=d["bpar"], ko=koff, nn=d["n"], tt=d["t"], co=d["coff"], cl=d["cls"], lk=d["lik"], rows=lik.shape[0],
            stride=lik.shape[1], R=2, tau=0.5, hi=Hi):
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        return L.stb_seat_filter(a, ptr(bp), 2, ptr(ko), ptr(nn), ptr(tt), None, 0, ptr(co), ptr(cl), ptr(lk), rows, stride, R, tau,
                                 1, 0, ptr(hi), w.data_ptr(), None, None, None, None, None, None)

    for kw in (dict(hi=None), dict(bp=None), dict(ko=None), dict(nn=None), dict(tt=None), dict(co=None), dict(cl=None),
               dict(rows=0), dict(stride=0), dict(R=0), dict(R=65), dict(tau=2.0), dict(tau=math.nan), dict(a=1.0)):
        assert raw(**kw) != 0 and capi.last_error(), kw
    torch.cuda.synchronize()
    assert np.all(Hi.cpu().numpy() == SENT_H) and np.all(w.cpu().numpy() == SENT_W)
    assert raw() == 0
    torch.cuda.synchronize()
    assert np.all(np.isfinite(Hi.cpu().numpy())) and np.all(w.cpu().numpy() > 0.0)


# ---- 6. the object

def test_the_objects_call_is_the_raw_call_and_writes_nothing():
    a, R, tau = 0.45, 8, 0.5
    shapes = [(int(k), int(c)) for k, c in zip([3, 9, 1, 64, 65, 33, 70, 5], [12, 30, 4, 20, 9, 0, 25, 66])]
    K, n, t, h, bpar, coff, cls, lik = pf.make_case(shapes, a, 17)
    n0, t0 = np.maximum(n, 1).astype(np.uint32), np.maximum(t, 1).astype(np.uint16)     # (an object's pairs hold customers)
    t0 = np.minimum(t0, n0).astype(np.uint16)
    case = (K, n0, t0, h, bpar, coff, cls, lik)
    raw = run_pf(case, a, 0, R, tau, seed=31, sweep=2)
    tot_r, _, _ = capi.seat_loglik(raw["d_Hi"].reshape(-1, 1))
    ti = capi.TableIndicators(K, n0, t0, h)
    try:
        ti.set_lik(lik)
        ti.set_heldout(coff, cls)
        ti.heldout(a, bpar, accumulate=True)
        before, acc0 = fetch(ti), ti.heldout_get()
        seq0 = ti.heldout_seq(a, bpar, R, 31, 2)
        tot, Hi, info = ti.heldout_pf(a, bpar, R, tau, 31, 2)
        assert same_bits(Hi, raw["Hi"]) and same_bits(tot, tot_r)
        assert (info.skipped, info.impossible, info.stuck, info.dead, info.resamplings) == raw["info"]
        assert info.customers == int(coff[-1]) and info.resamplings > 0 and info.skipped == 0
        # nothing of the object was written, and the sequential call after it answers as before it
        assert_state(fetch(ti), before)
        acc1 = ti.heldout_get()
        assert same_bits(acc1[0], acc0[0]) and acc1[1] == acc0[1]
        seq1 = ti.heldout_seq(a, bpar, R, 31, 2)
        assert same_bits(seq1[1], seq0[1]) and same_bits(seq1[0], seq0[0])
        # never resampling: the sequential estimate at the same (seed, sweep, R), each within its bar of one truth
        tot0, Hi0, info0 = ti.heldout_pf(a, bpar, R, 0.0, 31, 2)
        sr = sto.replay(K, n0, t0, h, a, bpar, coff, cls, lik, 0, 31, 2, R, bars=True)
        tr = sto.truth(K, n0, t0, h, a, bpar, coff, cls, lik, 0, sr)
        tHi, tHb, _, _ = sto.loglik_truth(tr, range(len(K)), R)
        _, _, Hb = pf.truth(K, n0, t0, h, a, bpar, coff, cls, lik, 0, 31, 2, R, 0.0, restaurants=[])
        assert info0.resamplings == 0
        for i in range(len(K)):
            assert sto.within(Hi0[i], tHi[i], Hb[i]) and abs(Hi0[i] - seq0[1][i]) <= tHb[i] + Hb[i], (i, Hi0[i], seq0[1][i])
        for call in (lambda: ti.heldout_pf(a, bpar, 0, tau, 1, 0), lambda: ti.heldout_pf(a, bpar, 65, tau, 1, 0),
                     lambda: ti.heldout_pf(a, bpar, 4, 1.5, 1, 0), lambda: ti.heldout_pf(1.0, bpar, 4, tau, 1, 0)):
            with pytest.raises(capi.StbError):
                call()
        assert capi.lib().stb_tindic_heldout_pf(ti.h, a, capi.dp(bpar), 4, tau, 1, 0, None, None, None) != 0    # total is required
        assert_state(fetch(ti), before)
    finally:
        ti.free()


if __name__ == "__main__":
    if sys.argv[1:] == ["--digest"]:
        print(_digest())
