"""High-precision truth and a replay of the joint (a, b) step (libstb_amd/csrc/hyperj.hip; DESIGN.md section 6, deviation 14).

    L(a, beta) = W(a) + R(a, b) + ((shape - 1) beta - b / scale) + beta,        beta = log b
    W(a)    = sum over pairs with n > 1 of S_S_a(n, t)                          (hp_oracle.rows: long double)
    R(a, b) = sum_i [ T_i log a + lgamma(T_i + b/a) - lgamma(b/a) - lgamma(b + N_i) + lgamma(b) ]   (0 where N_i = 0)

The truth of R takes every distinct (T, N) once: lgamma(T + c) - lgamma(c) as the sum of log(c + k), k < T, in long double
for T <= 256, mpmath at 40 digits beyond; lgamma(b + N) - lgamma(b) from mpmath.

The bar of R (u = 2^-53, L = hp_oracle.L_LGAMMA ulp for a device lgamma, slope(z) >= |z psi(z)|) follows k_joint_terms'
own operations, term = (T la + (lgamma(T + c) - lgc)) - (lgamma(b + N) - lgb):
  * c = b / a and T + c are formed with one rounding each, which moves the two lgammas by at most u slope(c) and
    u (slope(c) + slope(T + c)): u (slope(T + c) + slope(c)) is taken for the pair, as hp_oracle.term_bar does;
  * the two lgammas to L ulp of their values; their difference rounds once: u |diff|;
  * la = log a from the host's libm (1 ulp) and the product T la (one rounding): 2 u |T la|; the sum T la + diff: u |.|;
  * b + N with one rounding: u slope(b + N); lgamma(b + N) and lgamma(b) to L ulp; their difference: u |gN|;
  * the last subtraction: u |term|;
  * the block's tree adds the term in 8 levels of plain double additions, each rounding at most u times the partial sum's
    magnitude, which the magnitudes of its terms bound: 8 u |term| is this term's share;
  * the blocks are added in double-double (no first-order term); hi + lo rounds once, and the truth is rounded to a double
    for the comparison: 4 u |sum| covers both with room.
So bar(R) = sum over restaurants of the term's bar + 4 u |R|.

The replay works on given L values: stages, boxes, weights, the mixture proposal q, the draw and the MH decision, in the
operations the host side of hyperj.hip performs (IEEE doubles, math.exp / math.log are the C library's).
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import hp_oracle as hp  # noqa: E402
from libstb_amd import synth  # noqa: E402

LD = np.longdouble
U = hp.U
_MASK = (1 << 64) - 1
_G = 0x9E3779B97F4A7C15
MAX_STAGES = 5
FLOOR = -60.0
BOX = 40.0
EPS = 1.0 / 64.0


def _mix(z: int) -> int:
    z &= _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def uniforms(seed: int, sweep: int) -> np.ndarray:
    """u[0..5]: elements 0 .. 5 of unit(., key), key = mix(seed + (sweep + 1) gamma); the step uses u[1] .. u[5]"""
    return synth.unit(6, _mix(seed + (sweep + 1) * _G))


# ---------------------------------------------------------------------------------------------------- the truth

def prior(shape: float, scale: float, beta: float, b: float) -> float:
    return ((shape - 1.0) * beta - b / scale) + beta


def W_truth(a, n, t):
    """W(a_d) for every a_d (long double): sum over pairs with n > 1 of log S^n_t"""
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    n = np.asarray(n, dtype=np.int64)
    t = np.asarray(t, dtype=np.int64)
    keep = n > 1
    n, t = n[keep], t[keep]
    out = np.zeros(a.shape[0], dtype=LD)
    if n.size == 0:
        return out
    N, M = int(n.max()), int(t.max())
    for r, v, e in hp.rows(a, N, M):
        sel = t[n == r]
        if sel.size:
            lg = hp.logs(v, e)
            for m in sel:
                out += lg[:, int(m)]
    return out


def _lgamma_abs(x):
    return np.abs(np.vectorize(math.lgamma, otypes=[np.float64])(np.asarray(x, dtype=np.float64)))


def term_grid(a, b, T: int, N: int):
    """one restaurant's term over the grid a[D] x b[J]: (value [D, J] long double, bar [D, J])"""
    mp = hp._mp()
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    D, J = a.shape[0], b.shape[0]
    if N == 0:
        return np.zeros((D, J), dtype=LD), np.zeros((D, J))
    c = b.astype(LD)[None, :] / a.astype(LD)[:, None]
    la = np.log(a.astype(LD))[:, None]
    if T <= 256:
        diff = np.zeros((D, J), dtype=LD)
        for k in range(T):
            diff += np.log(c + LD(k))
    else:
        diff = np.empty((D, J), dtype=LD)
        for d in range(D):
            for j in range(J):
                z = mp.mpf(float(b[j])) / mp.mpf(float(a[d]))
                v = mp.loggamma(T + z) - mp.loggamma(z)
                hi = float(v)
                diff[d, j] = LD(hi) + LD(float(v - hi))
    gN = np.empty(J, dtype=LD)
    for j in range(J):
        v = mp.loggamma(mp.mpf(float(b[j])) + N) - mp.loggamma(mp.mpf(float(b[j])))
        hi = float(v)
        gN[j] = LD(hi) + LD(float(v - hi))
    Tla = LD(T) * la
    val = (Tla + diff) - gN[None, :]
    cd = b[None, :] / a[:, None]
    f = lambda x: np.abs(np.asarray(x, dtype=np.float64))  # noqa: E731
    bar = U * (hp.L_LGAMMA * (_lgamma_abs(T + cd) + _lgamma_abs(cd)) + hp._slope(T + cd) + hp._slope(cd) + f(diff)
               + 2.0 * f(Tla) + f(Tla + diff)
               + (hp.L_LGAMMA * (_lgamma_abs(b + N) + _lgamma_abs(b)) + hp._slope(b + N) + f(gN))[None, :]
               + 9.0 * f(val))
    return val, bar


def _rise(z, n: int):
    """lgamma(z + n) - lgamma(z) for an array z (long double): the sum of log(z + k), k < n, up to n = 256, mpmath beyond"""
    z = np.asarray(z, dtype=LD)
    if n <= 256:
        out = np.zeros(z.shape, dtype=LD)
        for k in range(n):
            out += np.log(z + LD(k))
        return out
    mp = hp._mp()
    out = np.empty(z.shape, dtype=LD)
    for idx in np.ndindex(z.shape):
        hi = float(z[idx])
        zm = mp.mpf(hi) + mp.mpf(float(z[idx] - LD(hi)))
        v = mp.loggamma(zm + n) - mp.loggamma(zm)
        vh = float(v)
        out[idx] = LD(vh) + LD(float(v - vh))
    return out


def R_points(a, b, T, N):
    """R(a_k, b_k) at K points (long double) for restaurants T[I], N[I]"""
    a = np.asarray(a, dtype=np.float64).astype(LD)
    b = np.asarray(b, dtype=np.float64).astype(LD)
    out = np.zeros(a.shape, dtype=LD)
    for Ti, Ni in zip(np.asarray(T, dtype=np.int64), np.asarray(N, dtype=np.int64)):
        if Ni > 0:
            out += (LD(int(Ti)) * np.log(a) + _rise(b / a, int(Ti))) - _rise(b, int(Ni))
    return out


def _rise_table(z, nmax: int):
    """tab[n] = lgamma(z + n) - lgamma(z), n = 0 .. nmax, for an array z (long double): running sums of log(z + k)"""
    z = np.asarray(z, dtype=LD)
    tab = np.zeros((nmax + 1,) + z.shape, dtype=LD)
    for k in range(nmax):
        tab[k + 1] = tab[k] + np.log(z + LD(k))
    return tab


def R_points_truth(a, b, T, N):
    """(R(a_k, b_k) long double [K], its bar [K]) at K points for restaurants T[I], N[I] with counts up to 4096: the terms
    and bars of term_grid, point by point (the rises from one table of running log sums per argument)"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    T = np.asarray(T, dtype=np.int64)
    N = np.asarray(N, dtype=np.int64)
    assert T.max() <= 4096 and N.max() <= 4096
    aL, bL = a.astype(LD), b.astype(LD)
    cd = b / a
    riseT = _rise_table(bL / aL, int(T.max()))
    riseN = _rise_table(bL, int(N.max()))
    la = np.log(aL)
    lg_c, lg_b = _lgamma_abs(cd), _lgamma_abs(b)
    f = lambda x: np.abs(np.asarray(x, dtype=np.float64))  # noqa: E731
    val = np.zeros(a.shape, dtype=LD)
    bar = np.zeros(a.shape)
    types, counts = np.unique(np.stack([T, N], axis=1), axis=0, return_counts=True)
    for (Ti, Ni), cnt in zip(types, counts):
        if Ni == 0:
            continue
        Ti, Ni = int(Ti), int(Ni)
        diff, gN, Tla = riseT[Ti], riseN[Ni], LD(Ti) * la
        v = (Tla + diff) - gN
        e = U * (hp.L_LGAMMA * (_lgamma_abs(Ti + cd) + lg_c) + hp._slope(Ti + cd) + hp._slope(cd) + f(diff) + 2.0 * f(Tla)
                 + f(Tla + diff) + hp.L_LGAMMA * (_lgamma_abs(b + Ni) + lg_b) + hp._slope(b + Ni) + f(gN) + 9.0 * f(v))
        val += LD(int(cnt)) * v
        bar += float(cnt) * e
    return val, bar + 4.0 * U * f(val)


def W_truth_bar(a, n, t):
    """(W[d] long double, bar[d]): hp_oracle's model bar per pair + 4 u |W|"""
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    n = np.asarray(n, dtype=np.int64)
    t = np.asarray(t, dtype=np.int64)
    slope = hp.K1 + hp.K2 / (1.0 - a)
    W = np.zeros(len(a), dtype=LD)
    bar = np.zeros(len(a))
    for r, v, e in hp.rows(a, int(n.max()), int(t.max())):
        sel = t[(n == r) & (n > 1)]
        if sel.size:
            y = hp.logs(v, e)[:, sel]
            W += y.sum(axis=1)
            bar += U * (slope * r * sel.size + 4.0 * np.abs(y.astype(np.float64)).sum(axis=1) + 16.0 * sel.size)
    return W, bar + 4 * U * np.abs(W.astype(np.float64))


def L_truth_grid(g, am, bm, bem, shape: float, scale: float):
    """(L [D, J] as doubles, bar) on a stage's midpoints for the counts g (n, t, T, N): W's and R's bars, the prior's four
    roundings and the two additions that form L: 8 u (|W| + |R| + |P| + |L|)"""
    W, wb = W_truth_bar(am, g.n, g.t)
    R, rb = R_truth(am, bm, g.T, g.N)
    P = ((shape - 1.0) * bem - bm / scale) + bem
    Lt = (W[:, None] + R.astype(LD) + P[None, :]).astype(np.float64)
    bar = wb[:, None] + rb + 8 * U * (np.abs(W.astype(np.float64))[:, None] + np.abs(R) + np.abs(P)[None, :] + np.abs(Lt))
    return Lt, bar


def L_truth_points(g, a, b, shape: float, scale: float):
    """(L [K] as doubles, bar [K]) at K points (a_k, b_k), as L_truth_grid"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    W, wb = W_truth_bar(a, g.n, g.t)
    R, rb = R_points_truth(a, b, g.T, g.N)
    beta = np.array([math.log(x) for x in b])
    P = ((shape - 1.0) * beta - b / scale) + beta
    Lt = (W + R + P).astype(np.float64)
    bar = wb + rb + 8 * U * (np.abs(W.astype(np.float64)) + np.abs(R.astype(np.float64)) + np.abs(P) + np.abs(Lt))
    return Lt, bar


# the problem of the step-against-replay tests: 200 restaurants x 20 dishes, n <= 60; rectangle, prior, grid, seed, steps
STEP_RECT = (0.02, 0.97, 0.05, 500.0)
STEP_SHAPE, STEP_SCALE = 1.1, 20.0
STEP_D = STEP_J = 24
STEP_SEED, STEP_STEPS, STEP_START = 4711, 300, (0.5, 10.0)


def step_problem():
    return synth.groups(200, 20, 60, "realistic", seed=77)


def left_out(stages, log_alpha: float, u4: float) -> bool:
    """a step the comparison with the device leaves out: a cumulative weight within 1e-12 relative of u1 Z in some stage,
    or |log alpha - log u4| < 1e-9"""
    lu = math.log(u4) if u4 > 0 else -math.inf
    return min(q["near"] for q in stages) < 1e-12 or abs(log_alpha - lu) < 1e-9


def R_truth(a, b, T, N):
    """(R [D, J] as doubles, bar [D, J]) for restaurants T[I], N[I]: every distinct (T, N) once"""
    T = np.asarray(T, dtype=np.int64)
    N = np.asarray(N, dtype=np.int64)
    D, J = len(a), len(b)
    val = np.zeros((D, J), dtype=LD)
    bar = np.zeros((D, J))
    if T.size:
        types, counts = np.unique(np.stack([T, N], axis=1), axis=0, return_counts=True)
        for (Ti, Ni), cnt in zip(types, counts):
            v, e = term_grid(a, b, int(Ti), int(Ni))
            val += LD(int(cnt)) * v
            bar += float(cnt) * e
    R = val.astype(np.float64)
    return R, bar + 4.0 * U * np.abs(R)


# ---------------------------------------------------------------------------------------------------- the replay

def cells_of(rect, D: int, J: int):
    """(a_mid[D], beta_mid[J], b_mid[J], da, db) of a stage's rectangle (a_lo, a_hi, beta_lo, beta_hi)"""
    alo, ahi, blo, bhi = rect
    da = (ahi - alo) / float(D)
    db = (bhi - blo) / float(J)
    am = [alo + (float(d) + 0.5) * da for d in range(D)]
    bm = [blo + (float(j) + 0.5) * db for j in range(J)]
    return np.array(am), np.array(bm), np.array([math.exp(x) for x in bm]), da, db


def cell_of(st, a: float, beta: float) -> int:
    """the cell d J + j of a point in a stage, or -1 outside its rectangle"""
    alo, ahi, blo, bhi = st["rect"]
    if not (alo <= a <= ahi and blo <= beta <= bhi):
        return -1
    D, J = st["D"], st["J"]
    d = min(max(int(math.floor((a - alo) / st["da"])), 0), D - 1)
    j = min(max(int(math.floor((beta - blo) / st["db"])), 0), J - 1)
    return d * J + j


def stage_of(L, rect, u1: float):
    """what one stage makes of its L[D, J]: maximum, floored weights, total, cumulative weights (d-major), the cell u1
    picks, the padded and clipped box, and how close u1 Z comes to a cumulative weight (relative)"""
    L = np.asarray(L, dtype=np.float64)
    D, J = L.shape
    mx = float(L.max())
    w = np.exp(np.maximum(L - mx, FLOOR)).reshape(-1)
    cum = np.cumsum(w)
    Z = float(cum[-1])
    target = u1 * Z
    hit = np.nonzero(cum > target)[0]
    pick = int(hit[0]) if hit.size else D * J - 1
    near = float(np.min(np.abs(cum - target))) / target if target > 0 else 1.0
    dd, jj = np.nonzero(L >= mx - BOX)
    box = (max(int(dd.min()) - 1, 0), min(int(dd.max()) + 1, D - 1), max(int(jj.min()) - 1, 0), min(int(jj.max()) + 1, J - 1))
    _, _, _, da, db = cells_of(rect, D, J)
    return {"rect": tuple(rect), "D": D, "J": J, "da": da, "db": db, "mx": mx, "w": w, "Z": Z, "cell": pick, "box": box,
            "near": near}


def next_rect(st):
    """the box as the next stage's rectangle, or None when the stage is the last by the rule (the cap aside)"""
    D, J = st["D"], st["J"]
    d0, d1, j0, j1 = st["box"]
    if not (2 * (d1 - d0 + 1) <= D or 2 * (j1 - j0 + 1) <= J):
        return None
    alo, ahi, blo, bhi = st["rect"]
    return (alo + float(d0) * st["da"], ahi if d1 == D - 1 else alo + float(d1 + 1) * st["da"],
            blo + float(j0) * st["db"], bhi if j1 == J - 1 else blo + float(j1 + 1) * st["db"])


def stages_of(eval_grid, rect_ab, D: int, J: int, u1: float):
    """the nested stages over the caller's rectangle (a_lo, a_hi, b_lo, b_hi); eval_grid(s, a_mid, b_mid, beta_mid) -> L[D, J]"""
    rect = (rect_ab[0], rect_ab[1], math.log(rect_ab[2]), math.log(rect_ab[3]))
    out = []
    for s in range(MAX_STAGES):
        am, bem, bm, _, _ = cells_of(rect, D, J)
        st = stage_of(eval_grid(s, am, bm, bem), rect, u1)
        out.append(st)
        rect = next_rect(st)
        if rect is None:
            break
    return out


def eps_of(S: int):
    return [EPS] * (S - 1) + [1.0 - float(S - 1) / 64.0]


def q_density(stages, a: float, beta: float) -> float:
    """the mixture proposal's density at (a, beta), in (a, beta) coordinates"""
    q = 0.0
    for st, eps in zip(stages, eps_of(len(stages))):
        k = cell_of(st, a, beta)
        if k >= 0:
            q += eps / (st["Z"] * (st["da"] * st["db"])) * float(st["w"][k])
    return q


def propose(stages, u):
    """(stage index, a', beta', b') from u[5] (stage), the stage's own pick for u[1], and u[2], u[3]"""
    S = len(stages)
    pick, cum = S - 1, 0.0
    for s in range(S - 1):
        cum += EPS
        if u[5] < cum:
            pick = s
            break
    st = stages[pick]
    d, j = divmod(st["cell"], st["J"])
    a = min(st["rect"][0] + (float(d) + float(u[2])) * st["da"], st["rect"][1])
    beta = min(st["rect"][2] + (float(j) + float(u[3])) * st["db"], st["rect"][3])
    return pick, a, beta, math.exp(beta)


def decide(stages, L_cur: float, L_new: float, x_cur, x_new, u4: float):
    """(log alpha, accepted) of the independence Metropolis-Hastings test; x = (a, beta)"""
    la = (L_new - L_cur) + (math.log(q_density(stages, *x_cur)) - math.log(q_density(stages, *x_new)))
    lu = math.log(u4) if u4 > 0 else -math.inf
    return la, lu < la
