"""The forward seating's law and its replay, on the CPU (tests/st_oracle.py; the device is held to the replay by
tests/test_gpu_seat.py).

  * the identity behind both uses, by exact enumeration: the weighted path sum into every final state is the dish
    sweep's unnormalised joint, from an empty restaurant and from one that is not, with and without a truncation;
  * with L = 1 and h summing to 1 the final state is a draw from the prior;
  * the replay lies within its derived bars of the 40-digit truth on the raw case;
  * four wrong replays are told apart, two by the bar and two by bits;
  * the law through the replay: 20000 restaurants against the enumerated proposal law;
  * what tests/test_gpu_seat_geometry.py relies on: the synthetic log weights, the long-double truth of their
    log-mean-exp against mpmath, the numpy replay within the rows' bar of it, seven wrong k_seat_sum told apart by the very
    assertions the device meets, the band of the grid case replayed alone, the dish at the uint16 bound.
"""
import itertools
import math

import numpy as np
import pytest

import st_oracle as sto
import td_oracle as tdo

HS = (0.3, 0.7)
LIK = ((0.6, 0.1), (0.4, 0.9))
CLS4 = (0, 1, 1, 0)
PARAMS = ((0.3, 1.5, 4), (0.0, 2.0, 4), (0.9, -0.5, 4), (0.5, 1.0, 2))


def _lprod(z, cls):
    return math.prod(LIK[cls[c]][k] for c, k in enumerate(z))


@pytest.mark.parametrize("a,b,M", PARAMS)
def test_path_sum_is_the_unnormalised_joint(a, b, M):
    acc = sto.enumerate_paths((0, 0), (0, 0), HS, a, b, CLS4, LIK, M)
    st = tdo.states(4, 2, M)
    assert set(acc) == set(st)                       # every state with t <= M is reached, and no other
    want = sto.ujoint_states(4, 2, HS, a, b, CLS4, LIK, M)
    worst = max(abs(acc[s][0] - w) / w for s, w in zip(st, want))
    assert worst <= 1e-12, worst
    # the same, normalised, is td_oracle.joint: what the dish sweep leaves invariant
    pw = np.array([acc[s][0] for s in st])
    assert np.abs(pw / pw.sum() - tdo.joint(4, 2, HS, a, b, CLS4, LIK, M)).max() <= 1e-12


@pytest.mark.parametrize("a,b,M", PARAMS)
def test_path_sum_from_a_start_state(a, b, M):
    # Three customers are seated already, two at dish 0 and one at dish 1; three more come.  The path sum obeys the
    # joint's own recurrence from wherever it starts, so from the start pairs (n0, t0) weighted by their joint it lands
    # on the joint of the six: sum_t0 pi(n0, t0) sum_paths P W = pi(n0 + new, t) prod L, state by state -- and summed over
    # the final states, E[W | start] = p(start + new) / p(start) with the start's tables drawn from their law given n0.
    n0, cls = (2, 1), (1, 0, 1)
    starts = [(ta, 1) for ta in range(1, min(2, M) + 1)]
    accs = {t0: sto.enumerate_paths(n0, t0, HS, a, b, cls, LIK, M) for t0 in starts}
    finals = [(z, (ta, tb)) for z in itertools.product(range(2), repeat=3)
              for ta in range(1, min(n0[0] + z.count(0), M) + 1) for tb in range(1, min(n0[1] + z.count(1), M) + 1)]
    assert set().union(*[set(acc) for acc in accs.values()]) == set(finals)
    worst, total, want_total = 0.0, 0.0, 0.0
    for z, ts in finals:
        ns = tuple(n0[k] + z.count(k) for k in range(2))
        got = sum(sto.ujoint(n0, t0, HS, a, b) * accs[t0].get((z, ts), [0.0])[0] for t0 in starts)
        want = sto.ujoint(ns, ts, HS, a, b) * _lprod(z, cls)
        worst = max(worst, abs(got - want) / want)
        total += got
        want_total += want
    assert worst <= 1e-12, worst
    p_start = sum(sto.ujoint(n0, t0, HS, a, b) for t0 in starts)
    mean_W = sum(sto.ujoint(n0, t0, HS, a, b) / p_start * sum(v[0] for v in accs[t0].values()) for t0 in starts)
    assert abs(mean_W - want_total / p_start) <= 1e-12 * mean_W


def test_without_a_likelihood_the_final_state_is_a_prior_draw():
    hs = (0.25, 0.75)
    for a, b in ((0.3, 1.5), (0.0, 2.0), (0.9, -0.5)):
        acc = sto.enumerate_paths((0, 0), (0, 0), hs, a, b, (0, 0, 0, 0))
        st = tdo.states(4, 2)
        P = np.array([acc[s][1] for s in st])
        PW = np.array([acc[s][0] for s in st])
        assert abs(P.sum() - 1.0) <= 1e-14 and np.abs(PW - P).max() <= 1e-14        # every weight is 1
        assert np.abs(P - tdo.joint(4, 2, hs, a, b)).max() <= 1e-13


# ---------------------------------------------------------------------------------------------------- the replay

A0, M0, R0 = 0.5, 0, 2


def test_the_vectorised_scan_is_the_dish_sweeps():
    rng = np.random.default_rng(1)
    for K in (1, 63, 64, 65, 130):
        q = rng.random((3, K)) ** 3
        pad = np.zeros((3, 64 * -(-K // 64)))
        pad[:, :K] = q
        cum, Z = sto.cumsum64(pad)
        for r in range(3):
            want = tdo.cumsum64(q[r])
            assert np.array_equal(cum[r].view(np.uint64), want.view(np.uint64)) and Z[r] == want[-1]


def test_replay_lies_within_its_bar_of_the_truth():
    K, n, t, h, bpar, coff, cls, lik = sto.raw_case(A0)
    rep, tr = sto.raw_replay(A0, M0, R0, True), sto.raw_truth(A0, M0, R0)
    assert rep["skipped"] == 1 and rep["stuck"] == R0 and rep["impossible"] == 2 * R0
    I = len(K)
    dead = [i for i in range(I) if not np.all(rep["lw"][i] > -math.inf)]
    assert dead == [sto.R_STUCK, sto.R_CLASS]
    for i in range(I):
        for r in range(R0):
            assert sto.within(rep["lw"][i, r], tr["lw"][i, r], tr["lw_bar"][i, r]), (i, r)
    # the bars are bars, not slack: a restaurant of 300 customers is held to a few 1e-13
    assert 0.0 < tr["lw_bar"].max() < 1e-11
    alive = [i for i in range(I - 1) if i not in dead]
    Hi, total, nbad = sto.loglik_replay(rep["lw"][alive])
    tHi, tHb, ttot, ttb = sto.loglik_truth(tr, alive, R0)
    assert nbad == 0 and all(sto.within(Hi[j], tHi[j], tHb[j]) for j in range(len(alive)))
    assert sto.within(total, ttot, ttb) and ttb < 1e-10
    Hi, total, nbad = sto.loglik_replay(rep["lw"])
    assert nbad == 2 and total == -math.inf and not np.isnan(Hi).any() and Hi[sto.R_NOK] == 0.0


def test_wrong_replays_are_told_apart():
    K, n, t, h, bpar, coff, cls, lik = sto.raw_case(A0)
    rep, tr = sto.raw_replay(A0, M0, 1, True), sto.raw_truth(A0, M0, 1)
    alive = [i for i in range(len(K)) if rep["lw"][i, 0] > -math.inf and coff[i + 1] > coff[i]]
    first = [int(coff[i]) for i in alive]
    run = lambda mut: sto.replay(K, n, t, h, A0, bpar, coff, cls, lik, M=M0, seed=sto.SEED, sweep=sto.RAW_SWEEP, mut=mut)  # noqa: E731
    # by the bar: the first customer of a restaurant sees the start state whatever the replay did elsewhere
    for mut in ("t+1", "noTa"):
        bad = run(mut)
        off = [i for i, c in zip(alive, first) if abs(bad["p"][c] - rep["p"][c]) > 2.0 * rep["pbar"][c, 0]]
        # (every restaurant that starts with a table: t a and T a are there to be left out)
        want = [i for i in alive if int(t[int(np.sum(K[:i])):int(np.sum(K[:i + 1]))].sum()) > 0]
        assert off == want, (mut, off, want)
        assert any(not sto.within(bad["lw"][i, 0], tr["lw"][i, 0], tr["lw_bar"][i, 0]) for i in alive)
    # by bits
    lin = run("linear")
    assert (lin["p"].view(np.uint64) != rep["p"].view(np.uint64)).any()
    swp = run("swap")
    assert (swp["cust"] != rep["cust"]).any() or (swp["t"] != rep["t"]).any()
    assert np.array_equal(swp["p"].view(np.uint64)[first], rep["p"].view(np.uint64)[first])   # (p of a start state has no u)


# ---------------------------------------------------------------------------------------------------- the law

def test_law_through_the_replay():
    rep = sto.law_replay()
    cells = sto.law_cells(rep)
    acc = sto.enumerate_paths((0, 0), (0, 0), sto.LAW_H, sto.LAW_A, sto.LAW_B, sto.LAW_CLS, sto.LAW_LIK)
    law = {s: v[1] for s, v in acc.items()}
    assert abs(sum(law.values()) - 1.0) <= 1e-13
    p = sto.chi2_p(cells, law, sto.LAW_I)
    print("chi-square p against the proposal law", p)
    assert p > 1e-3
    wrong = sto.enumerate_paths((0, 0), (0, 0), sto.LAW_H, sto.LAW_A, sto.LAW_B, sto.LAW_CLS, sto.LAW_LIK, mut="noTa")
    pw = sto.chi2_p(cells, {s: v[1] for s, v in wrong.items()}, sto.LAW_I)
    print("chi-square p against the seating without T a", pw)
    assert pw < 1e-9
    # the weights: mean W against p(w), the standard deviation from the enumeration
    pw_true = sum(v[0] for v in acc.values())
    sd = math.sqrt(sum(v[2] for v in acc.values()) - pw_true ** 2)
    W = np.exp(rep["lw"][:, 0])
    print("mean W", W.mean(), "p(w)", pw_true, "sd", sd)
    assert abs(W.mean() - pw_true) <= 5.0 * sd / math.sqrt(sto.LAW_I)
    # p(w) is the joint's normaliser: sum over states of the unnormalised joint
    want = float(sto.ujoint_states(3, 2, sto.LAW_H, sto.LAW_A, sto.LAW_B, sto.LAW_CLS, sto.LAW_LIK).sum())
    assert abs(pw_true - want) <= 1e-13 * want


# ---------------------------------------------------------------------------------------------------- the geometry tests' oracle

LW_R = (1, 2, 3, 63, 64, 65, 127, 128, 129, 4096)      # every particle count tests/test_gpu_seat_geometry.py runs
GX = 1024                                              # a device of 256 compute units: four workgroups each
BIG = ((sto.past_one_block(GX), 3, GX), (sto.past_one_block(GX), 65, GX), (sto.past_one_block(200), 3, 200),
       (4096 * 256 + 1, 1, GX))                        # (I, R, grid_x): past one block (twice, and at the floor), the regrow


def _bits(x):
    return np.float64(x).tobytes()


def test_the_log_weight_types_hold_what_they_promise():
    for R in LW_R:
        lw = sto.lw_types(R)
        assert lw.shape == (257, R) and not lw.flags.writeable and not np.isnan(lw).any()
        assert np.all(lw.max(axis=1) > -math.inf) and lw.max() <= 1.0 and lw[np.isfinite(lw)].min() >= -1400.0
        assert np.all(lw[sto.LW_ALLEQ] == lw[sto.LW_ALLEQ, 0]) and np.argmax(lw[sto.LW_MAXLAST]) == R - 1
        assert lw.max(axis=1).min() <= -499.0
        spread = lw.max(axis=1) - np.where(np.isfinite(lw), lw, math.inf).min(axis=1)
        assert R == 1 or (spread.min() <= 2e-3 and spread.max() > 300.0)
        if R >= 2:
            assert spread[sto.LW_SPREAD] > 745.0 and np.isinf(lw).any(axis=1).sum() >= 10
            assert np.argmax(lw[sto.LW_SPREAD]) >= min(64, R - 1)
            assert np.all(lw[sto.LW_SPREAD, :min(64, R - 1)] < lw[sto.LW_SPREAD].max() - 719.0)
        if R > 64:
            assert np.argmax(lw[sto.LW_MAX64]) == 64
        dead = sto.lw_types(R, dead_row=True)
        assert np.all(dead[256] == -math.inf) and np.array_equal(dead[:256], lw[:256])


def test_the_long_double_truth_agrees_with_mpmath():
    mp = sto.hp._mp()
    for R in (2, 65):
        lw = sto.lw_types(R, dead_row=True)
        tr = sto.loglik_rows_truth(lw)
        assert tr[256] == -math.inf
        for i in (sto.LW_ALLEQ, sto.LW_MAXLAST, sto.LW_SPREAD, sto.LW_MAX64, 8, 100):
            W = [mp.exp(mp.mpf(float(v))) for v in lw[i] if v > -math.inf]
            want = mp.log(mp.fsum(W) / R)
            hi = float(tr[i])
            got = mp.mpf(hi) + mp.mpf(float(tr[i] - sto.hp.LD(hi)))      # (the long double, exactly)
            assert abs(got - want) <= 1e-2 * sto.U * abs(want), (R, i)   # a hundredth of the bar's u |H_i| alone


def test_loglik_replay_lies_within_the_rows_bar_of_the_truth():
    worst = {}
    for R in LW_R:
        for dead_row in (False, True):
            lw = sto.lw_types(R, dead_row=dead_row)
            tr = sto.loglik_rows_truth(lw)
            bar = sto.loglik_rows_bar(lw, tr)
            Hi, total, nbad = sto.loglik_replay(lw)
            worst[R] = max(worst.get(R, 0.0), sto.over_bar(Hi, tr, bar))
            assert worst[R] <= 1.0, (R, worst[R])
            assert nbad == int(dead_row) and (total == -math.inf) == dead_row and (bar[:256] > 0.0).all()
            if not dead_row:
                ttot, tbar = sto.loglik_total_truth(tr, bar)
                assert abs(total - ttot) <= tbar and tbar < 1e-9 * abs(total)
    print("loglik_replay against the long-double truth, largest error over bar by R:", worst)


@pytest.mark.parametrize("mut", ("meanpad", "max64", "base1"))
def test_wrong_rows_leave_the_bar(mut):
    """the assertion of tests/test_gpu_seat_geometry.py on every H_i, applied to a wrong k_seat_sum"""
    for R in LW_R:
        lw = sto.lw_types(R)
        tr = sto.loglik_rows_truth(lw)
        Hi, _, _ = sto.loglik_replay(lw, mut)
        told = not sto.over_bar(Hi, tr, sto.loglik_rows_bar(lw, tr)) <= 1.0
        assert told == (R % 64 != 0 if mut == "meanpad" else R > 64), (mut, R)


@pytest.mark.parametrize("mut", ("plain", "linear", "stale", "skipstage"))
def test_wrong_totals_lose_the_bits(mut):
    """the total's bit-equality, applied to a wrong association on the H_i of the sizes the device tests run"""
    for I, R, gx in BIG:
        Hi = np.resize(sto.loglik_replay(sto.lw_types(R))[0], I)
        right = sto.loglik_total(Hi)
        assert _bits(right) == _bits(sto.loglik_replay(np.resize(sto.lw_types(R), (I, R)) if I < 100000 else
                                                       sto.lw_types(R)[np.arange(I) % 257])[1])
        nblk = -(-I // 256)
        assert nblk > gx and (I % 256 == 1 or I == 70000)
        told = _bits(sto.loglik_total(Hi, mut, gx)) != _bits(right)
        assert told == (nblk > sto.STAGE or mut != "skipstage"), (mut, I, R)
    if mut == "stale":          # three blocks, the last of one restaurant: every particle count tells
        for R in LW_R:
            Hi = np.resize(sto.loglik_replay(sto.lw_types(R))[0], 513)
            assert _bits(sto.loglik_total(Hi, mut)) != _bits(sto.loglik_total(Hi))


def test_a_dead_row_makes_the_total_minus_infinity_and_nothing_else():
    Hi = np.resize(sto.loglik_replay(sto.lw_types(3))[0], 513).copy()
    Hi[[7, 300, 512]] = -math.inf
    assert sto.loglik_total(Hi) == -math.inf


def test_the_band_alone_replays_as_the_band_among_all():
    I, R = 40, 4
    case = sto.grid_case(I)
    K, n, t, h, bpar, coff, cls, lik = case
    band = sto.grid_band(I)
    assert band == list(range(8)) + list(range(31, 40)) and sto.grid_band() == list(range(8)) + list(range(16376, 16385))
    full = sto.replay(K, n, t, h, sto.GRID_A, bpar, coff, cls, lik, seed=sto.GRID_SEED, sweep=sto.GRID_SWEEP, particles=R)
    _, part, tr = sto.grid_band_truth(I, R)
    assert full["skipped"] == 0 and part["skipped"] == I - len(band)
    assert np.array_equal(full["lw"][band].view(np.uint64), part["lw"][band].view(np.uint64))
    assert not part["lw"][[i for i in range(I) if i not in band]].any()
    assert np.isfinite(full["lw"]).all() and len({float(v) for v in full["lw"].reshape(-1)}) > I * R // 2
    assert all(sto.within(part["lw"][i, r], tr["lw"][i, r], tr["lw_bar"][i, r]) for i in band for r in range(R))


def test_the_grid_case_crosses_the_cap_at_one_wave_and_at_no_other():
    items = sto.GRID_I * sto.GRID_R
    assert items == sto.GRID_CAP + 64 and all(-(-items // w) < sto.GRID_CAP for w in (2, 4, 8))
    K, n, t, h, bpar, coff, cls, lik = sto.grid_case()
    assert len(K) == sto.GRID_I and set(K) == {2} and np.all(np.diff(coff.astype(np.int64)) == 3) and n.max() <= 4
    assert np.all((t <= n) & ((t > 0) == (n > 0))) and len(set(bpar)) == sto.GRID_I and set(cls) == {0, 1}


def test_the_bound_case_closes_the_dish_at_65535():
    K, n, t, h, bpar, coff, _, _ = sto.bound_case()
    rep = sto.bound_replay()
    opened = sto.bound_opened(rep)
    print("tables opened, visits after, final t, final T, visits elsewhere:", opened)
    koff = np.concatenate([[0], np.cumsum(K)])
    for i in range(4):
        new, after, tfin, T, other = opened[i]
        assert new == (1 if sto.BOUND_T[i] == 65534 else 0) and tfin == 65535            # one table from 65534, none from 65535
        assert T == int(rep["t"][koff[i]:koff[i + 1]].astype(np.int64).sum())           # and T follows
        assert T - int(t[koff[i]:koff[i + 1]].astype(np.int64).sum()) == int(rep["new"][8 * i:8 * i + 8, 0].sum())
        assert int(rep["n"][koff[i + 1] - 1]) == sto.BOUND_N + 8 - other
    assert rep["impossible"] == rep["stuck"] == rep["skipped"] == 0


def test_the_bound_seed_is_the_first_that_opens_the_table_early():
    assert sto.bound_seed_ok(sto.BOUND_SEED) and not any(sto.bound_seed_ok(s) for s in range(sto.BOUND_SEED))
