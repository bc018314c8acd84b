"""Annealed importance sampling for unseen documents (stb_seat_anneal, libstb_amd/csrc/seat_ais.hip) judged on the CPU: the
ladder is unbiased by exact propagation over every state, the two wrong orders are not; the numpy replay
(tests/ais_oracle.py) lies within its derived bars of the 40-digit truth and wrong replays are told apart; what the call
refuses.  The device is held to the replay in tests/test_gpu_ais.py."""
import math

import numpy as np
import pytest

import ais_oracle as ao
import st_oracle as sto
import ti_oracle as tio

PARAMS = ((0.5, 1.0, None), (0.0, 1.0, None), (0.9, -0.3, None), (0.5, 1.0, 2), (0.9, -0.3, 2))


def p_w(a, b, M):
    return float(sto.ujoint_states(ao.LAW_NC, ao.LAW_K, ao.LAW_H, a, b, ao.LAW_CLS, ao.LAW_LIK, M).sum())


@pytest.mark.parametrize("passes", (1, 2))
@pytest.mark.parametrize("a,b,M", PARAMS)
def test_the_ladder_is_unbiased_by_exact_propagation(a, b, M, passes):
    want = p_w(a, b, M)
    got = ao.exact(ao.LAW_NC, ao.LAW_K, ao.LAW_H, a, b, ao.LAW_CLS, ao.LAW_LIK, ao.LAW_BETAS, passes, M)
    assert abs(got - want) <= 1e-12 * want, (got, want)
    # any ladder, S = 1 (importance sampling from the prior) included
    for betas in ((1.0,), (0.1, 1.0), (0.3, 0.31, 0.9, 1.0)):
        got = ao.exact(ao.LAW_NC, ao.LAW_K, ao.LAW_H, a, b, ao.LAW_CLS, ao.LAW_LIK, betas, passes, M)
        assert abs(got - want) <= 1e-12 * want, (betas, got, want)


def test_the_issues_numbers():
    assert abs(p_w(0.5, 1.0, None) - 0.122846) < 5e-7
    for passes, after, prev in ((1, 0.17737, 0.09181), (2, 0.17620, None)):
        got = ao.exact(ao.LAW_NC, ao.LAW_K, ao.LAW_H, 0.5, 1.0, ao.LAW_CLS, ao.LAW_LIK, ao.LAW_BETAS, passes, None, "after")
        assert abs(got - after) < 5e-6, got
        if prev is not None:
            got = ao.exact(ao.LAW_NC, ao.LAW_K, ao.LAW_H, 0.5, 1.0, ao.LAW_CLS, ao.LAW_LIK, ao.LAW_BETAS, passes, None, "prev")
            assert abs(got - prev) < 5e-6, got


@pytest.mark.parametrize("order", ("after", "prev"))
@pytest.mark.parametrize("passes", (1, 2))
@pytest.mark.parametrize("a,b,M", PARAMS)
def test_the_two_wrong_orders_are_biased(a, b, M, passes, order):
    want = p_w(a, b, M)
    got = ao.exact(ao.LAW_NC, ao.LAW_K, ao.LAW_H, a, b, ao.LAW_CLS, ao.LAW_LIK, ao.LAW_BETAS, passes, M, order)
    assert abs(got - want) > 0.1 * want, (got, want)     # a tenth of p(w), against 1e-12


def test_under_a_truncation_the_seating_is_a_weighted_draw():
    # the prior measure over the states with t <= 2 does not sum to 1: a ladder that started every particle at weight 1
    # would estimate p(w) / Z_0, so lw starts at the seating's own log weight
    z0 = float(sto.ujoint_states(ao.LAW_NC, ao.LAW_K, ao.LAW_H, 0.5, 1.0, M=2).sum())
    assert z0 < 0.99
    assert abs(float(sto.ujoint_states(ao.LAW_NC, ao.LAW_K, ao.LAW_H, 0.5, 1.0).sum()) - 1.0) < 1e-14


# ---- the replay

HOST_CONFIGS = ((0.5, 0), (0.0, 0), (0.9, 2))
HOST_N, HOST_R, HOST_S, HOST_PASSES = 12, 3, 3, 2


def host_run(a, M, mut=None, bars=False, R=HOST_R, S=HOST_S, passes=HOST_PASSES, **kw):
    K, h, bpar, coff, cls, lik = ao.host_case(a)
    Mt = M if M else HOST_N
    vt = tio.ExactV(list(range(1, HOST_N + 1)), a, Mt)
    rep = ao.replay(K, h, a, bpar, coff, cls, lik, ao.numpy_tempered(lik, S), vt, HOST_N, Mt, ao.SEED, ao.SWEEP, R, S, None,
                    passes, mut=mut, bars=bars, **kw)
    return rep, Mt


@pytest.mark.parametrize("a,M", HOST_CONFIGS)
def test_the_replay_lies_within_its_bars_of_the_truth(a, M):
    K, h, bpar, coff, cls, lik = ao.host_case(a)
    rep, Mt = host_run(a, M, bars=True)
    tr = ao.truth(K, h, a, bpar, coff, cls, lik, Mt, rep, HOST_R)
    assert (rep["skipped"], rep["dead"]) == (0, 0)
    worst = sto.over_bar(rep["lw"], tr["lw"], np.where(tr["lw_bar"] > 0, tr["lw_bar"], 1.0))
    print("largest lw error over its bar", worst)
    assert worst <= 1.0
    live = np.abs(tr["lw"]) > 0
    assert (tr["lw_bar"][live] <= 1e-12 * np.maximum(1.0, np.abs(tr["lw"][live]))).all()   # a few hundred ulps, not a licence
    Hi, Hb, tot, tb = ao.finish(K, tr, HOST_R)
    rHi, rtot, rbad = sto.loglik_replay(rep["lw"])
    assert rbad == 0 and sto.over_bar(rHi, Hi, np.where(Hb > 0, Hb, 1.0)) <= 1.0
    assert sto.within(rtot, tot, tb)
    assert rHi[3] == 0.0 and rHi[4] == 0.0      # no customers: the empty product


def test_the_seating_is_the_priors_and_the_sweeps_move_it():
    a, M = 0.5, 0
    K, h, bpar, coff, cls, lik = ao.host_case(a)
    one, _ = host_run(a, M, S=1)
    ex = ao.expand(K, coff, cls, h, bpar, HOST_R, HOST_N, lik.shape[1])
    coffx = np.concatenate([ex["coff2"], [ex["C2"]]])
    z = np.zeros(ex["G2"], dtype=np.int64)
    so = sto.replay(ex["K2"], z, z, ex["h2"], a, ex["bpar2"], coffx, M=HOST_N, seed=ao.SEED, sweep=ao.SWEEP)
    assert np.array_equal(one["pn"], so["n"]) and np.array_equal(one["pcust"], so["cust"])
    # S = 1 is importance sampling from the prior: lw = lw0 + 1.0 * D of the prior seating, nothing moved
    D, _ = ao.D_of(so["cust"], ex["cls2"], ex["coff2"], ex["N2"], lik, np.ones(len(ex["K2"]), dtype=bool))
    assert np.array_equal(one["lw"].reshape(-1), so["lw"][:, 0] + 1.0 * D)
    three, _ = host_run(a, M)
    assert not np.array_equal(three["pcust"], one["pcust"])


@pytest.mark.parametrize("a,M", HOST_CONFIGS)
def test_wrong_replays_are_told_apart(a, M):
    K, h, bpar, coff, cls, lik = ao.host_case(a)
    rep, Mt = host_run(a, M, bars=True)
    tr = ao.truth(K, h, a, bpar, coff, cls, lik, Mt, rep, HOST_R)
    bar = np.where(tr["lw_bar"] > 0, tr["lw_bar"], 1.0)
    # dbeta replaced by beta_s: the same states, lw outside the bar
    bs, _ = host_run(a, M, mut="beta_s")
    assert np.array_equal(bs["pcust"], rep["pcust"]) and np.array_equal(bs["pn"], rep["pn"])
    assert sto.over_bar(bs["lw"], tr["lw"], bar) > 1e6
    # the sweep's number reused across temperatures, the layout without its R: by bits
    ss, _ = host_run(a, M, mut="samesweep")
    assert not np.array_equal(ss["pcust"], rep["pcust"])
    lay, _ = host_run(a, M, mut="layout")
    assert np.array_equal(lay["pcust"], rep["pcust"]) and not np.array_equal(lay["pn"], rep["pn"])
    # the increment after the sweep: the same states, another weight
    af, _ = host_run(a, M, mut="after")
    assert np.array_equal(af["pcust"], rep["pcust"]) and sto.over_bar(af["lw"], tr["lw"], bar) > 1e6


def test_the_expansion_is_the_headers_layout():
    K, h, bpar, coff, cls, lik = ao.host_case(0.5)
    R = 3
    ex = ao.expand(K, coff, cls, h, bpar, R, HOST_N, lik.shape[1])
    koff = np.concatenate([[0], np.cumsum(K)])
    for i in range(len(K)):
        for r in range(R):
            j = i * R + r
            assert ex["koff2"][j] == koff[i] * R + r * K[i] and ex["coff2"][j] == int(coff[i]) * R + r * int(coff[i + 1] - coff[i])
            assert np.array_equal(ex["cls2"][ex["coff2"][j]:ex["coff2"][j] + ex["N2"][j]], cls[int(coff[i]):int(coff[i + 1])])
            assert np.array_equal(ex["h2"][ex["koff2"][j]:ex["koff2"][j] + K[i]], h[koff[i]:koff[i + 1]])
    # gapless: the replicas follow one another, so cumulative sums give the same offsets (st_oracle and td_oracle take K)
    assert np.array_equal(ex["koff2"], np.concatenate([[0], np.cumsum(ex["K2"])])[:-1])
    assert np.array_equal(ex["coff2"], np.concatenate([[0], np.cumsum(ex["N2"])])[:-1])


def test_what_is_left_out():
    K, h, bpar, coff, cls, lik = ao.host_case(0.5)
    # a table of 8 rows: the restaurants of 9 and 12 customers are left out, the others' replicas keep their places
    small, _ = host_run(0.5, 0)
    Kx = ao.expand(K, coff, cls, h, bpar, 2, 8, lik.shape[1])
    assert list(np.flatnonzero(Kx["skip"])) == [1, 2]
    assert list(np.flatnonzero(ao.expand(K, coff, cls, h, bpar, 2, 12, 4)["skip"])) == [2]       # K = 5 > stride = 4
    assert list(np.flatnonzero(ao.expand(K, coff, cls, h, bpar, 2, 12, 6, cap=3)["skip"])) == [2, 5]
    K0 = np.array(K)
    K0[5] = 0                                                                                    # no dishes, one customer
    assert list(np.flatnonzero(ao.expand(K0, coff, cls, h[:-4], bpar, 2, 12, 6)["skip"])) == [5]
    # G or C misstated: everybody, without pairs or customers
    bad = ao.expand(K, coff, cls, h, bpar, 2, 12, 6, G=int(K.sum()) + 1)
    assert bad["skip"].all() and not bad["K2"].any() and not bad["N2"].any()
    vt = tio.ExactV(list(range(1, 13)), 0.5, 12)
    rep = ao.replay(K, h, 0.5, bpar, coff, cls, lik, ao.numpy_tempered(lik, 2), vt, 12, 12, ao.SEED, ao.SWEEP, 2, 2,
                    C=int(coff[-1]) - 1)
    assert rep["skipped"] == len(K) and not rep["lw"].any() and rep["dead"] == 0
    # left out by the table's N: lw = 0, the others as if alone with the same flat indices
    vt8 = tio.ExactV(list(range(1, 9)), 0.5, 8)
    rep8 = ao.replay(K, h, 0.5, bpar, coff, cls, lik, ao.numpy_tempered(lik, 3), vt8, 8, 8, ao.SEED, ao.SWEEP, HOST_R, 3, None, 2)
    assert rep8["skipped"] == 2 and not rep8["lw"][1].any() and not rep8["lw"][2].any()
    assert np.array_equal(rep8["lw"][[0, 3, 4, 5]], small["lw"][[0, 3, 4, 5]])   # (rows up to 8 of either table are the same cells)


def test_a_dead_particle_stays_dead():
    K, h, bpar, coff, cls, lik = ao.host_case(0.5)
    lik = np.array(lik)
    lik[:, 0] = 0.0               # restaurant 0 has dish 0 alone: every particle of it dies at the first increment
    lik[1, 1] = 0.0
    vt = tio.ExactV(list(range(1, 13)), 0.5, 12)
    rep = ao.replay(K, h, 0.5, bpar, coff, cls, lik, ao.numpy_tempered(lik, 3), vt, 12, 12, ao.SEED, ao.SWEEP, 4, 3, None, 1,
                    bars=True)
    assert (rep["lw"][0] == -math.inf).all() and rep["dead"] >= 4
    assert not np.isnan(rep["lw"]).any()
    Hi, tot, bad = sto.loglik_replay(rep["lw"])
    assert Hi[0] == -math.inf and bad >= 1 and tot == -math.inf and not np.isnan(Hi).any()
    alive = (rep["lw"] > -math.inf).any(axis=1)
    assert np.isfinite(Hi[alive]).all()
    tr = ao.truth(K, h, 0.5, bpar, coff, cls, lik, 12, rep, 4)
    assert np.array_equal(tr["lw"] == -math.inf, rep["lw"] == -math.inf)


# ---- the law, by the replay

def test_the_replays_mean_weight_is_p_w_and_the_wrong_orders_is_not():
    K, h, bpar, coff, cls, lik = ao.law_case()
    I = 4000
    K, h, bpar, coff, cls = K[:I], h[:2 * I], bpar[:I], coff[:I + 1], cls[:3 * I]
    vt = tio.ExactV([1, 2, 3], ao.LAW_A)
    want = p_w(ao.LAW_A, ao.LAW_B, None)
    tl = ao.numpy_tempered(lik, 4, ao.LAW_BETAS)
    ok = ao.replay(K, h, ao.LAW_A, bpar, coff, cls, lik, tl, vt, 3, 3, ao.LAW_SEED, ao.LAW_SWEEP, 1, 4, ao.LAW_BETAS, 1)
    mean, tol, off = ao.law_statistic(ok["lw"], want)
    assert off <= tol, (mean, want, tol)
    af = ao.replay(K, h, ao.LAW_A, bpar, coff, cls, lik, tl, vt, 3, 3, ao.LAW_SEED, ao.LAW_SWEEP, 1, 4, ao.LAW_BETAS, 1, mut="after")
    mean, tol, off = ao.law_statistic(af["lw"], want)
    assert off > tol, (mean, want, tol)


# ---- the refusals' conditions

def test_the_refusals_conditions():
    ok = dict(S=4, betas=None, passes=1, particles=16)
    assert ao.refusal(**ok) is None
    assert ao.refusal(**{**ok, "S": 0}) == "S"
    assert ao.refusal(**{**ok, "passes": 0}) == "passes"
    assert ao.refusal(**{**ok, "particles": 0}) == "particles" and ao.refusal(**{**ok, "particles": 4097}) == "particles"
    assert ao.refusal(**{**ok, "particles": 4096}) is None
    for betas in ((0.0, 0.5, 0.75, 1.0), (0.5, 0.5, 0.75, 1.0), (0.25, 0.5, 0.75, 0.99), (0.25, 0.5, 1.0, 1.0),
                  (0.25, 0.5, 0.75, 1.0000000000000002), (0.25, math.nan, 0.75, 1.0), (0.6, 0.5, 0.75, 1.0)):
        assert ao.refusal(**{**ok, "betas": betas}) == "betas", betas
    assert ao.refusal(**{**ok, "betas": (0.25, 0.5, 0.75, 1.0)}) is None
    assert ao.refusal(**{**ok, "S": 1, "betas": (1.0,)}) is None
    assert ao.refusal(**ok, a=1.0) == "a" and ao.refusal(**ok, a=-0.1) == "a"
    assert ao.refusal(**ok, M=65536) == "M" and ao.refusal(**ok, M=0) == "bounds" and ao.refusal(**ok, N=0) == "bounds"
    assert ao.refusal(**ok, I=-1) == "I" and ao.refusal(**ok, I=2 ** 28) == "replicas"
    assert ao.refusal(**ok, lik=False) == "matrix" and ao.refusal(**ok, cls=False) == "matrix"
    # the even ladder ends at exactly 1.0 for every S, and is strictly increasing
    for S in (1, 2, 3, 7, 32, 1000):
        be = ao.ladder(S)
        assert be[-1] == 1.0 and all(x < y for x, y in zip([0.0] + be, be))
