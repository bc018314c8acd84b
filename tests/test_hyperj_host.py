"""The joint (a, b) step's law on the CPU (tests/hj_oracle.py's replay; DESIGN.md section 6, deviation 14): the
independence kernel is reversible with respect to exp(L) with the stage mixture as the proposal, the proposal is a
density that is positive on the whole rectangle, the zoom follows its rule, and a replayed chain has the quadrature
marginals.  The problem is one restaurant with pairs (n, t) <= (12, 4); W comes from hp_oracle's rows."""
import math

import numpy as np
import pytest

import hj_oracle as hj
from libstb_amd import synth

N_PAIRS = np.array([12, 7, 3, 5, 1, 9, 12])
T_PAIRS = np.array([4, 2, 1, 3, 1, 4, 2])
T_REST, N_REST = [int(T_PAIRS.sum())], [int(N_PAIRS.sum())]
RECT = (0.02, 0.97, 0.05, 500.0)
SHAPE, SCALE = 1.1, 20.0
D = J = 24
ACCEPTED_200 = 193      # accepted steps of the replay of hj_oracle's 200-restaurant problem on oracle values (below)
ACCEPT_RATE = 0.8525   # the replayed chain's acceptance rate, recorded from this test's own print (seed 20261, 4000 steps)


def L_points(a, b):
    """L at K points (long double -> double)"""
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    b = np.atleast_1d(np.asarray(b, dtype=np.float64))
    beta = np.log(b)
    pr = ((SHAPE - 1.0) * beta - b / SCALE) + beta
    return (hj.W_truth(a, N_PAIRS, T_PAIRS) + hj.R_points(a, b, T_REST, N_REST) + pr).astype(np.float64)


def L_grid(s, am, bm, bem):
    W = hj.W_truth(am, N_PAIRS, T_PAIRS)
    R = hj.LD(0) + sum(hj.term_grid(am, bm, t, n)[0] for t, n in zip(T_REST, N_REST))
    pr = ((SHAPE - 1.0) * bem - bm / SCALE) + bem
    return (W[:, None] + R + pr[None, :]).astype(np.float64)


@pytest.fixture(scope="module")
def stages():
    return hj.stages_of(L_grid, RECT, D, J, 0.5)


def q_quadrature(stages):
    """the integral of hj.q_density over the rectangle: q is constant on every rectangle of the lattice made of ALL
    stages' cell edges, so its value at the rectangle's midpoint times the area, summed, is exact up to rounding"""
    ea = np.unique(np.concatenate([st["rect"][0] + st["da"] * np.arange(st["D"] + 1) for st in stages] + [[st["rect"][1]] for st in stages]))
    eb = np.unique(np.concatenate([st["rect"][2] + st["db"] * np.arange(st["J"] + 1) for st in stages] + [[st["rect"][3]] for st in stages]))
    terms = []
    for i in range(len(ea) - 1):
        for j in range(len(eb) - 1):
            area = (ea[i + 1] - ea[i]) * (eb[j + 1] - eb[j])
            if area > 0:
                terms.append(hj.q_density(stages, 0.5 * (ea[i] + ea[i + 1]), 0.5 * (eb[j] + eb[j + 1])) * area)
    return math.fsum(terms), len(terms)


def test_the_proposal_is_a_positive_density(stages):
    tot, cells = q_quadrature(stages)
    print("stages %d, integral of q over %d lattice rectangles %.17g" % (len(stages), cells, tot))
    assert abs(tot - 1.0) <= 1e-12
    # positive on the whole rectangle: every stage-1 weight is at least exp(-60), and stage 1 covers the rectangle
    assert stages[0]["rect"] == (RECT[0], RECT[1], math.log(RECT[2]), math.log(RECT[3]))
    assert float(stages[0]["w"].min()) >= math.exp(-60.0) > 0
    u = synth.unit(4000, 77).reshape(-1, 2)
    for ua, ub in u[:500]:
        a = RECT[0] + ua * (RECT[1] - RECT[0])
        beta = stages[0]["rect"][2] + ub * (stages[0]["rect"][3] - stages[0]["rect"][2])
        assert hj.q_density(stages, a, beta) > 0


def test_detailed_balance_with_the_stage_mixture(stages):
    K = 10 ** 4
    u = synth.unit(4 * K, 12345).reshape(K, 4)
    r = stages[0]["rect"]
    ax = r[0] + u[:, 0] * (r[1] - r[0])
    bx = r[2] + u[:, 1] * (r[3] - r[2])
    ay = r[0] + u[:, 2] * (r[1] - r[0])
    by = r[2] + u[:, 3] * (r[3] - r[2])
    # half of the second points inside the last stage's rectangle, where every stage of the mixture contributes
    rl = stages[-1]["rect"]
    ay[::2] = rl[0] + u[::2, 2] * (rl[1] - rl[0])
    by[::2] = rl[2] + u[::2, 3] * (rl[3] - rl[2])
    Lx = L_points(ax, np.exp(bx))
    Ly = L_points(ay, np.exp(by))
    ref = float(max(Lx.max(), Ly.max()))
    worst = 0.0
    for k in range(K):
        qx, qy = hj.q_density(stages, ax[k], bx[k]), hj.q_density(stages, ay[k], by[k])
        px, py = math.exp(Lx[k] - ref), math.exp(Ly[k] - ref)
        la_xy, _ = hj.decide(stages, Lx[k], Ly[k], (ax[k], bx[k]), (ay[k], by[k]), 0.5)
        la_yx, _ = hj.decide(stages, Ly[k], Lx[k], (ay[k], by[k]), (ax[k], bx[k]), 0.5)
        lhs = px * qy * math.exp(min(0.0, la_xy))
        rhs = py * qx * math.exp(min(0.0, la_yx))
        if max(lhs, rhs) > 0:
            worst = max(worst, abs(lhs - rhs) / max(lhs, rhs))
    print("detailed balance: worst relative difference %.3e over %d pairs, %d stages" % (worst, K, len(stages)))
    assert worst <= 1e-12


@pytest.mark.parametrize("sigma", [1e-4, 1e-3, 1e-2, 0.03, 0.1])
def test_zoom_follows_the_rule_on_a_gaussian(sigma):
    rect = (0.02, 0.97, 0.05, 500.0)
    lo, hi = math.log(rect[2]), math.log(rect[3])
    a0, b0 = 0.02 + 0.6180339 * 0.95, lo + 0.4142135 * (hi - lo)
    sa, sb = sigma * 0.95, sigma * (hi - lo)

    def gauss(s, am, bm, bem):
        return -0.5 * (((am - a0) / sa) ** 2)[:, None] - 0.5 * (((bem - b0) / sb) ** 2)[None, :]

    st = hj.stages_of(gauss, rect, D, J, 0.3)
    S = len(st)
    print("sigma %g: %d stages, last rectangle %r" % (sigma, S, st[-1]["rect"]))
    assert 1 <= S <= 5
    for s, q in enumerate(st):
        d0, d1, j0, j1 = q["box"]
        half = 2 * (d1 - d0 + 1) <= D or 2 * (j1 - j0 + 1) <= J
        assert half == (s < S - 1) or (s == 4 and S == 5), (s, q["box"])
        # the box holds the mode, and so does every stage's rectangle
        alo, ahi, blo, bhi = q["rect"]
        assert alo <= a0 <= ahi and blo <= b0 <= bhi
        assert alo + d0 * q["da"] <= a0 <= alo + (d1 + 1) * q["da"] and blo + j0 * q["db"] <= b0 <= blo + (j1 + 1) * q["db"]
        if s:
            p = st[s - 1]["rect"]
            assert p[0] <= alo < ahi <= p[1] and p[2] <= blo < bhi <= p[3]
    # the box is +-sqrt(80) sigma = +-8.94 sigma plus a cell each side.  A tenth of the rectangle: it covers the rectangle,
    # one stage.  A ten-thousandth: while a cell is wider than the box the box is 3 cells and the zoom is 8-fold, cells of
    # 1/24, 1/192, 1/1536 of the rectangle in stages 1 to 3; stage 4's cells are 1/12288 = 0.81 sigma wide, its box
    # 17.9 / 0.81 + 2 = 24 cells, more than half: four stages
    assert S == {1e-4: 4, 0.1: 1}.get(sigma, S)


def test_replayed_chain_has_the_quadrature_marginals(stages):
    n = 4000
    seed = 20261
    S = len(stages)
    # the stages do not depend on the state; the cell a stage picks depends on u1 alone
    us = np.array([hj.uniforms(seed, k) for k in range(n)])
    props = []
    for k in range(n):
        per = [dict(st, cell=int(np.nonzero(np.cumsum(st["w"]) > us[k, 1] * st["Z"])[0][0])) for st in stages]
        props.append(hj.propose(per, us[k]))
    pa = np.array([p[1] for p in props])
    pbeta = np.array([p[2] for p in props])
    Lp = L_points(pa, np.array([p[3] for p in props]))
    a, beta = 0.5, math.log(10.0)
    Lc = float(L_points([a], [math.exp(beta)])[0])
    ca, cb, acc = np.empty(n), np.empty(n), 0
    for k in range(n):
        _, ok = hj.decide(stages, Lc, float(Lp[k]), (a, beta), (pa[k], pbeta[k]), us[k, 4])
        if ok:
            a, beta, Lc = pa[k], pbeta[k], float(Lp[k])
            acc += 1
        ca[k], cb[k] = a, beta
    rate = acc / n
    print("chain: %d stages, acceptance rate %.4f" % (S, rate))
    assert abs(rate - ACCEPT_RATE) <= 0.005
    # quadrature marginals on a fine midpoint lattice
    r = stages[0]["rect"]
    Q = 400
    am, bem, bm, da, db = hj.cells_of(r, Q, Q)
    Lq = L_grid(0, am, bm, bem)
    P = np.exp(Lq - Lq.max())
    P /= P.sum()
    cdf_a = np.concatenate([[0.0], np.cumsum(P.sum(axis=1))])
    cdf_b = np.concatenate([[0.0], np.cumsum(P.sum(axis=0))])
    edges_a = r[0] + da * np.arange(Q + 1)
    edges_b = r[2] + db * np.arange(Q + 1)
    for name, x, edges, cdf in (("a", ca, edges_a, cdf_a), ("beta", cb, edges_b, cdf_b)):
        xs = np.sort(x)
        F = np.interp(xs, edges, cdf)
        i = np.arange(1, n + 1)
        ks = float(max(np.max(i / n - F), np.max(F - (i - 1) / n)))
        # n_eff from the measured autocorrelation (initial positive sequence)
        z = x - x.mean()
        var = float(z @ z) / n
        tau = 1.0
        for lag in range(1, 200):
            rho = float(z[:-lag] @ z[lag:]) / n / var
            if rho <= 0:
                break
            tau += 2.0 * rho
        neff = n / tau
        crit = 2.63 / math.sqrt(neff)
        print("%s: KS %.4f, n_eff %.0f, critical value %.4f" % (name, ks, neff, crit))
        assert ks < crit


def test_detailed_balance_and_mass_with_three_stages():
    """the tiny problem's posterior is broad (one stage); a sharp synthetic L exercises the nested mixture itself"""
    lo, hi = math.log(RECT[2]), math.log(RECT[3])
    a0, b0, sa, sb = 0.61, lo + 0.41 * (hi - lo), 1e-3 * 0.95, 1e-3 * (hi - lo)

    def Lf(a, beta):
        return -0.5 * ((a - a0) / sa) ** 2 - 0.5 * ((beta - b0) / sb) ** 2

    st = hj.stages_of(lambda s, am, bm, bem: Lf(am[:, None], bem[None, :]), RECT, D, J, 0.5)
    assert len(st) == 3
    mass, cells = q_quadrature(st)   # (through cell_of and the nesting of the three stages)
    print("three stages: integral of q over %d lattice rectangles %.17g" % (cells, mass))
    assert abs(mass - 1.0) <= 1e-12
    K = 10 ** 4
    u = synth.unit(4 * K, 999).reshape(K, 4)
    worst, inside = 0.0, 0
    for k in range(K):
        rx, ry = st[k % 3]["rect"], st[(k // 3) % 3]["rect"]
        x = (rx[0] + u[k, 0] * (rx[1] - rx[0]), rx[2] + u[k, 1] * (rx[3] - rx[2]))
        y = (ry[0] + u[k, 2] * (ry[1] - ry[0]), ry[2] + u[k, 3] * (ry[3] - ry[2]))
        Lx, Ly = Lf(*x), Lf(*y)
        qx, qy = hj.q_density(st, *x), hj.q_density(st, *y)
        assert qx > 0 and qy > 0
        inside += hj.cell_of(st[2], *x) >= 0
        # in logs: pi(x) q(y) alpha(x, y) against pi(y) q(x) alpha(y, x)
        lhs = Lx + math.log(qy) + min(0.0, hj.decide(st, Lx, Ly, x, y, 0.5)[0])
        rhs = Ly + math.log(qx) + min(0.0, hj.decide(st, Ly, Lx, y, x, 0.5)[0])
        worst = max(worst, abs(lhs - rhs) / max(1.0, abs(lhs)))
    print("three stages: worst relative difference of the logs %.3e, %d of %d first points inside the last stage" % (worst, inside, K))
    assert worst <= 1e-12 and inside >= K // 3


def test_replay_of_the_200_restaurant_problem_on_oracle_values():
    """the steps tests/test_gpu_hyperj.py compares with the device (same problem, seed, start and number of steps),
    replayed on the oracle's L: at most 1 % fall under either reason for leaving a step out; its accepted count is the
    figure the GPU test holds the device's against"""
    g = hj.step_problem()
    Dg, Jg = hj.STEP_D, hj.STEP_J
    # the stages depend on neither the state nor the uniforms: their L once; the cell a stage picks depends on u1
    base = hj.stages_of(lambda s, am, bm, bem: hj.L_truth_grid(g, am, bm, bem, hj.STEP_SHAPE, hj.STEP_SCALE)[0],
                        hj.STEP_RECT, Dg, Jg, 0.5)
    Ls = []
    for st in base:
        am, bem, bm, _, _ = hj.cells_of(st["rect"], Dg, Jg)
        Ls.append(hj.L_truth_grid(g, am, bm, bem, hj.STEP_SHAPE, hj.STEP_SCALE)[0])
    us = [hj.uniforms(hj.STEP_SEED, k) for k in range(hj.STEP_STEPS)]
    per = [hj.stages_of(lambda s, am, bm, bem: Ls[s], hj.STEP_RECT, Dg, Jg, u[1]) for u in us]
    props = [hj.propose(st, u) for st, u in zip(per, us)]
    Lp, _ = hj.L_truth_points(g, [p[1] for p in props], [p[3] for p in props], hj.STEP_SHAPE, hj.STEP_SCALE)
    a, b = hj.STEP_START
    beta = math.log(b)
    Lc = float(hj.L_truth_points(g, [a], [b], hj.STEP_SHAPE, hj.STEP_SCALE)[0][0])
    out = acc = 0
    for k, (st, u) in enumerate(zip(per, us)):
        _, ap, betap, _ = props[k]
        la, ok = hj.decide(st, Lc, float(Lp[k]), (a, beta), (ap, betap), u[4])
        out += hj.left_out(st, la, u[4])
        if ok:
            a, beta, Lc = ap, betap, float(Lp[k])
            acc += 1
    print("200 restaurants: %d stages, %d of %d accepted, %d left out" % (len(base), acc, hj.STEP_STEPS, out))
    assert out <= hj.STEP_STEPS // 100
    assert acc == ACCEPTED_200
