"""The particle filter of the forward seating (stb_seat_filter, libstb_amd/csrc/seat_pf.hip) judged on the CPU: the
estimate is unbiased by exact enumeration, resampling triggered by the effective sample size included; a filter that
never resamples is the sequential seating; the numpy replay (tests/pf_oracle.py) lies within the derived bar of the
40-digit truth and wrong replays do not; the rescaling by powers of two is invisible.  The device is held to the replay
by bit-equality in tests/test_gpu_pf.py.  The chain case of tests/test_gpu_pf_geometry.py (three restaurants a workgroup)
holds every hand-over it is meant to, and a replay that forgets one reset between two of them is told apart by what
that file compares."""
import math

import numpy as np
import pytest

import pf_oracle as pf
import st_oracle as sto

# a rare dish 0 that the second customer's class all but demands: a slot whose first customer opened it outweighs one
# whose first customer did not by more than 10 to 1 (the trigger at tau = 0.6 and R = 2), two alike stay 1 to 1
HS = (0.02, 0.98)
LIK = ((0.9, 0.02), (0.9, 0.001))
CLS3 = (0, 1, 0)
PARAMS = ((0.3, 1.5, 4), (0.0, 2.0, 4), (0.9, -0.5, 4), (0.5, 1.0, 2))
A0, R0, TAU0 = 0.5, 3, 0.5


@pytest.mark.parametrize("tau", (0.0, 0.6, 1.0))
@pytest.mark.parametrize("a,b,M", PARAMS)
def test_the_estimate_is_unbiased_by_enumeration(a, b, M, tau):
    PZ, P, resampled, plain = pf.enumerate_filter(HS, a, b, CLS3, LIK, M, tau)
    want = float(sto.ujoint_states(3, 2, HS, a, b, CLS3, LIK, M).sum())
    assert abs(P - 1.0) <= 1e-12
    assert abs(PZ - want) <= 1e-12 * want, (PZ, want)
    if tau == 0.0:
        assert resampled == 0
    if tau == 0.6:                       # the trigger decides: some branches resample and some do not
        assert resampled > 0 and plain > 0, (resampled, plain)
    if tau == 1.0:
        assert resampled > 0


def test_a_filter_that_never_resamples_is_the_sequential_seating():
    K, n, t, h, bpar, coff, cls, lik = pf.host_case()
    koff = np.concatenate([[0], np.cumsum(K)])
    for R in (1, 3):
        rp = pf.replay(K, n, t, h, A0, bpar, coff, cls, lik, 0, pf.SEED, pf.SWEEP, R, 0.0)
        assert rp["resamplings"] == 0 and rp["skipped"] == 0
        for r in range(R):                # slot r is particle r of k_seat: the stream of sweep + r
            so = sto.replay(K, n, t, h, A0, bpar, coff, cls, lik, 0, pf.SEED, pf.SWEEP + r, 1)
            for i in range(len(K)):
                sl = slice(int(koff[i]) * R + r * int(K[i]), int(koff[i]) * R + (r + 1) * int(K[i]))
                assert np.array_equal(rp["pn"][sl], so["n"][koff[i]:koff[i + 1]]), (R, r, i)
                assert np.array_equal(rp["pt"][sl], so["t"][koff[i]:koff[i + 1]]), (R, r, i)
        sr = sto.replay(K, n, t, h, A0, bpar, coff, cls, lik, 0, pf.SEED, pf.SWEEP, R, bars=True)
        tr = sto.truth(K, n, t, h, A0, bpar, coff, cls, lik, 0, sr)
        tHi, tHb, _, _ = sto.loglik_truth(tr, range(len(K)), R)
        _, Ht, Hb = pf.truth(K, n, t, h, A0, bpar, coff, cls, lik, 0, pf.SEED, pf.SWEEP, R, 0.0)
        for i in range(len(K)):
            # both are estimates of the same log mean weight: each within its own bar of its truth, the truths equal
            assert sto.within(rp["H"][i], Ht[i], Hb[i]) and sto.within(rp["H"][i], tHi[i], tHb[i] + Hb[i]), (R, i)


def test_the_replay_lies_within_its_bar_of_the_truth():
    K, n, t, h, bpar, coff, cls, lik = pf.host_case()
    rep, Ht, Hb = pf.truth(K, n, t, h, A0, bpar, coff, cls, lik, 0, pf.SEED, pf.SWEEP, R0, TAU0)
    assert rep["resamplings"] >= 3 and rep["dead"] == 0
    worst = 0.0
    for i in range(len(K)):
        assert sto.within(rep["H"][i], Ht[i], Hb[i]), (i, rep["H"][i], Ht[i], Hb[i])
        if Hb[i] > 0:
            worst = max(worst, abs(rep["H"][i] - Ht[i]) / Hb[i])
            assert Hb[i] <= 1e-11 * max(1.0, abs(Ht[i]))        # the bar is a few hundred ulps, not a licence
    print("largest H error over its bar", worst)
    assert rep["H"][5] == 0.0 and Ht[5] == 0.0                 # no customers


def test_wrong_replays_are_told_apart():
    K, n, t, h, bpar, coff, cls, lik = pf.host_case()
    R, tau = 8, 0.8
    rep, Ht, Hb = pf.truth(K, n, t, h, A0, bpar, coff, cls, lik, 0, pf.SEED, pf.SWEEP, R, tau)
    assert rep["resamplings"] >= 5
    for mut in ("linear", "u4"):          # by bits: the weights' sums, or the states a resampling hands on
        rm = pf.replay(K, n, t, h, A0, bpar, coff, cls, lik, 0, pf.SEED, pf.SWEEP, R, tau, mut=mut)
        same = (np.array_equal(rm["pn"], rep["pn"]) and np.array_equal(rm["pt"], rep["pt"]) and
                np.array_equal(rm["w"].view(np.uint64), rep["w"].view(np.uint64)) and np.array_equal(rm["E"], rep["E"]) and
                np.array_equal(rm["Zm"].view(np.uint64), rep["Zm"].view(np.uint64)))
        assert not same, mut
    for mut in ("noE", "noS1"):           # by the bar
        rm = pf.replay(K, n, t, h, A0, bpar, coff, cls, lik, 0, pf.SEED, pf.SWEEP, R, tau, mut=mut)
        out = [i for i in range(len(K)) if rep["res"][i] > 0 and not sto.within(rm["H"][i], Ht[i], Hb[i])]
        assert len(out) == int((rep["res"] > 0).sum()) > 0, mut


def test_the_rescaling_is_invisible():
    # 400 customers with p about 1e-2: the product of the p underflows a double (1e-800); H stays finite, within the bar
    rng = np.random.default_rng(5)
    K = np.array([3], dtype=np.int32)
    lik = np.exp(rng.uniform(math.log(0.004), math.log(0.02), (4, 3)))
    h = np.array([0.2, 0.3, 0.5])
    coff = np.array([0, 400], dtype=np.uint64)
    cls = rng.integers(0, 4, 400).astype(np.uint32)
    n, t = np.zeros(3, dtype=np.uint32), np.zeros(3, dtype=np.uint16)
    for tau in (0.0, 0.5):
        rep, Ht, Hb = pf.truth(K, n, t, h, 0.3, [1.5], coff, cls, lik, 0, 9, 0, 4, tau)
        assert math.isfinite(rep["H"][0]) and rep["H"][0] < math.log(5e-324) and rep["dead"] == 0
        assert rep["E"][0] < -1100 and sto.within(rep["H"][0], Ht[0], Hb[0]), (rep["H"][0], Ht[0], Hb[0])
        so = sto.replay(K, n, t, h, 0.3, [1.5], coff, cls, lik, 0, 9, 0, 4)
        assert np.all(np.exp(so["lw"]) == 0.0)     # without step 2 every weight would be 0 in a double


def test_the_budget_is_the_headers():
    assert [pf.budget(K) for K in (0, 1, 64, 80, 81, 130, 1024)] == [64, 64, 64, 64, 62, 39, 5]


# ---- the chain case of tests/test_gpu_pf_geometry.py: a workgroup's second and third restaurant

def test_the_chain_case_is_the_full_launch_restricted_to_the_listed_restaurants():
    case, full = pf.chain_case()
    K, n, t, h, bpar, coff, cls, lik = case
    m, L = pf.CHAIN_M, full["listed"]
    assert full["I"] == 2 * pf.GRID_CAP + m == len(full["K"]) == len(full["bpar"]) == len(full["koff"]) - 1 == len(full["coff"]) - 1
    # workgroup g < m of a grid of GRID_CAP takes g, GRID_CAP + g, 2 GRID_CAP + g: the listed ones, three trips each
    assert np.array_equal(L, np.concatenate([s * pf.GRID_CAP + np.arange(m) for s in range(3)])) and len(K) == 3 * m
    assert [(int(k), int(c)) for k, c in zip(K, np.diff(coff.astype(np.int64)))] == [s for tr in pf.CHAIN_TRIPS for s in tr]
    koff = np.concatenate([[0], np.cumsum(K, dtype=np.int64)]).astype(np.uint64)
    assert np.array_equal(full["K"][L], K) and np.array_equal(full["bpar"][L], bpar)
    assert np.array_equal(full["koff"][L], koff[:-1]) and np.array_equal(full["koff"][L + 1], koff[1:])
    assert np.array_equal(full["coff"][L], coff[:-1]) and np.array_equal(full["coff"][L + 1], coff[1:])
    assert full["koff"][-1] == koff[-1] == len(n) == len(t) == len(h) and full["coff"][-1] == coff[-1] == len(cls)
    # the others: no dishes, no customers
    rest = np.ones(full["I"], dtype=bool)
    rest[L] = False
    assert not full["K"][rest].any() and not np.diff(full["coff"].astype(np.int64))[rest].any() and np.all(full["bpar"][rest] == 1.0)
    assert np.all(np.diff(full["koff"].astype(np.int64)) == full["K"])
    assert not (cls >= lik.shape[0]).any() and int((cls == 5).sum()) == 1 and not lik[5].any() and lik[:5].all()


def _kinds(case, rep):
    """per listed restaurant what the workgroup did with it, from the replay's outputs, and the visit's form"""
    K, Cn = case[0], np.diff(case[5].astype(np.int64))
    kind = ["skipped" if rep["skip"][i] else "dead" if rep["dead_mask"][i] else "empty" if Cn[i] == 0 else "alive" for i in range(len(K))]
    form = ["reg" if K[i] <= 64 else "lds" for i in range(len(K))]
    return kind, form


def _hands(kind, m):
    """(kind of the restaurant before, kind of the one after) over every two consecutive trips of a workgroup"""
    return {(kind[i - m], kind[i]) for i in range(m, len(kind))}


def test_the_chains_hold_every_hand_over():
    case, _ = pf.chain_case()
    K, m = case[0], pf.CHAIN_M
    reps = {R: pf.chain_truth(R, tau)[0] for R, tau in pf.CHAIN_RUNS}
    assert sorted(reps) == [4, 39, 40] and pf.budget(130) == 39 and pf.budget(128) >= 40
    for R, rep in reps.items():
        kind, form = _kinds(case, rep)
        hands = _hands(kind, m)
        assert [i for i, k in enumerate(kind) if k == "dead"] == [pf.CHAIN_DEAD] and rep["dead"] == 1, (R, kind)
        assert ("empty", "alive") in hands and ("alive", "empty") in hands, (R, hands)
        assert ("dead", "alive") in hands and rep["resamplings"] > 0, (R, hands)
        if R <= 39:
            assert rep["skipped"] == 0
            walked = [[form[g + s * m] for s in range(3)] for g in range(m) if all(kind[g + s * m] == "alive" for s in range(3))]
            assert ["reg", "lds", "reg"] in walked and ["lds", "reg", "reg"] in walked, (R, walked)
        else:
            assert rep["skipped"] == 5 and [i for i, k in enumerate(kind) if k == "skipped"] == [i for i in range(3 * m) if K[i] == 130]
            assert ("skipped", "alive") in hands and ("alive", "skipped") in hands, hands
    # the buffer a predecessor ends in: both parities before a successor that is seated, in either form of the successor
    rep = reps[39]
    kind, form = _kinds(case, rep)
    assert list(rep["res"]) == [18, 8, 8, 18, 4, 0, 11, 5, 6, 21, 8, 1, 21, 17, 4, 19, 18, 11, 5, 0, 20, 7, 4, 3]
    seen = {(int(rep["res"][i - m]) & 1, form[i]) for i in range(m, 3 * m) if kind[i] == "alive"}
    assert seen == {(0, "reg"), (1, "reg"), (0, "lds"), (1, "lds")}, seen


def _differing(case, rep, Hb, var, R):
    """the (restaurant, output) pairs of trips 1 and 2 in which a variant's results differ from the replay's by more than
    the device tests allow: bits of pn, pt, w, E, res; H by an infinity or by more than two bars"""
    K, m = case[0], pf.CHAIN_M
    koff = np.concatenate([[0], np.cumsum(K, dtype=np.int64)])
    out = []
    for i in range(m, len(K)):
        if rep["skip"][i]:
            continue
        sl = slice(int(koff[i]) * R, int(koff[i + 1]) * R)
        out += [(i, f) for f in ("pn", "pt") if not np.array_equal(var[f][sl], rep[f][sl])]
        out += [(i, "w")] if not np.array_equal(var["w"][i].view(np.uint64), rep["w"][i].view(np.uint64)) else []
        out += [(i, f) for f in ("E", "res") if var[f][i] != rep[f][i]]
        hv, hr = float(var["H"][i]), float(rep["H"][i])
        if (math.isinf(hv) or math.isinf(hr)) and hv != hr or (math.isfinite(hv) and math.isfinite(hr) and abs(hv - hr) > 2.0 * Hb[i]):
            out.append((i, "H"))
    return out


@pytest.mark.parametrize("variant", pf.CHAIN_VARIANTS)
def test_a_forgotten_reset_between_two_trips_is_told_apart(variant):
    case, _ = pf.chain_case()
    # at the budget's limit; the dead restaurant's successors are cheapest at four particles (both are seated there)
    R, tau = pf.CHAIN_RUNS[0] if variant == "keepdead" else pf.CHAIN_RUNS[1]
    rep, _, Hb = pf.chain_truth(R, tau)
    assert not _differing(case, rep, Hb, {f: rep[f] for f in ("pn", "pt", "w", "E", "res", "H")}, R)
    var = pf.chain_variant(case, rep, R, tau, variant)
    diff = _differing(case, rep, Hb, var, R)
    print(variant, "R", R, "differs in", diff)
    assert diff, variant
    # trip 0 has no predecessor: untouched
    koff0 = int(np.cumsum(case[0], dtype=np.int64)[pf.CHAIN_M - 1]) * R
    assert np.array_equal(var["pn"][:koff0], rep["pn"][:koff0]) and np.array_equal(var["E"][:pf.CHAIN_M], rep["E"][:pf.CHAIN_M])
    if variant == "keepdead":
        succ = [pf.CHAIN_DEAD + pf.CHAIN_M, pf.CHAIN_DEAD + 2 * pf.CHAIN_M]
        assert {i for i, _ in diff} == set(succ) and all((i, "H") in diff for i in succ) and np.all(np.isfinite(rep["H"][succ]))
