"""Replay, exact law, high-precision truth and error bar of the seating run as a particle filter (libstb_amd/csrc/
seat_pf.hip; include/stb_hip.h "the seating as a particle filter"; test infrastructure only).

Replay (numpy float64) -- written from the header's text
--------------------------------------------------------
  A visit is st_oracle's: st_oracle.replay is called on one customer of every restaurant at a time (one call a slot r, on
  the slots' present states, with sweep + r: its c and C are the true ones because the customers not yet seated are
  handed to restaurants without dishes, which it skips), so theta, q, the scan, k*, the impossible and stuck rules and
  new-or-old are its code and not a copy.  Steps 1 to 6 of the header follow in Python floats, one operation a line:
  ilogb is frexp's exponent - 1, ldexp is math.ldexp, the two scans are st_oracle.cumsum64 on a (1, 64) row, u4 is
  st_oracle.unit(particle_key(seed, sweep, 0), 2 c + 1).  H = numpy's log(v) + E * log(2): the device's log is its own, so
  H is compared within the bar, everything else bit for bit.

Exact law: enumerate_filter() walks every joint path of R = 2 slots with the uniforms integrated out, the law of
systematic resampling at R = 2 included.

Truth: along the replay's path, with its decisions, rescalings and ancestors held fixed, p_c(r) is a quotient of exact
integers (fractions.Fraction of the doubles: sum_k L_k (n_k - t_k a + (b + T a) h_k [k not at the truncation]) / (b + N);
sum_k L_k h_k where N = 0; 0 for a class outside the matrix) and steps 1 to 6 are taken by mpmath at 40 digits.

The bar of H (u = 2^-53), from the operations -- nothing here reads a device result
-----------------------------------------------------------------------------------
  rho_r, the relative error of w_r: 0 at the start and after a resampling (w = 1.0 exactly); a customer adds
      bar(p) / p + u (p's own bar, st_oracle's, and the one product).  The rescaling is exact.
  S1: a sum of non-negative terms: max_r rho_r + (R - 1) u (the scan's additions).
  a resampling: Zm = Zm * (S1 / R): rho_Z += rho_S1 + 2 u (the division and the product).  Renormalising Zm is exact.
  the finish: v = Zm * (S1 / R): rho_v = rho_Z + rho_S1 + 2 u.  H = log(v) + E * ln 2: log of a relatively perturbed
      argument plus its own ulp, rho_v + 2 u |log v|; the product E * ln 2 and the constant's own rounding, 2 u |E ln 2|;
      the last sum u |H|.
  Everything times st_oracle.SLACK for the second order.

The chains (chain_case, chain_variant): a launch past k_seat_pf's grid cap in which eight workgroups take three listed
restaurants each, and what a kernel that forgot one reset between two of them would return.
"""
from __future__ import annotations

import math
import os
import sys
from fractions import Fraction
from functools import lru_cache

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import st_oracle as sto  # noqa: E402
from st_oracle import cumsum64, particle_key, unit  # noqa: E402

U = sto.U
NEG_INF = -math.inf
MAXR = 64
LN2 = math.log(2.0)
LDS_DYN = 61440     # bytes of a workgroup's LDS left to the slots' states (PF_LDS_DYN)
GRID_CAP = 1 << 20  # k_seat_pf's grid is capped at this many workgroups


def budget(K: int) -> int:
    """stb_seat_filter_budget written from the header: min(64, 61440 / (12 K')), K' = K rounded up to even, at least 2"""
    kp = 2 if K < 2 else (K + 1) & ~1
    return min(MAXR, LDS_DYN // (12 * kp))


def ilogb(x: float) -> int:
    return math.frexp(x)[1] - 1


def _scan_last(w, R, linear=False):
    row = np.zeros((1, 64))
    row[0, :R] = w
    cum, Z = cumsum64(row, linear=linear)
    return cum[0], float(Z[0])


def skipped_mask(K, Cn, R, stride=None):
    K = np.asarray(K, dtype=np.int64)
    return sto.skipped_mask(K, Cn, stride) | np.array([R > budget(int(k)) for k in K], dtype=bool)


def replay(K, n, t, h, a, bpar, coff, cls=None, lik=None, M: int = 0, seed: int = 0, sweep: int = 0, particles: int = 1,
           tau: float = 0.5, mut=None, trace: bool = False, start=None, only=None):
    """stb_seat_filter on one start state.  Returns a dict: pn, pt (the slots' final pairs in the device's layout, a
    skipped restaurant's zero), w (I, R), E [I], Zm [I], res [I], anc (per restaurant a list of (c, ancestors)), H [I]
    (0 for a skipped restaurant), skipped, impossible, stuck, dead, resamplings, skip (the mask); with trace: steps, per
    restaurant a list over its customers of dicts p, pbar (R each), n0, t0 (the slots' pairs before the visit, (R, K_i)),
    e, S1, resampled, ez, anc, kept (slots not zeroed).
    mut: 'linear' (the weights' scan left to right), 'u4' (u4 taken from u3's element), 'noE' (E left out of H),
    'noS1' (S1 / R left out of Zm at a resampling)
    start, only: a wrong kernel's hand-over (chain_variant).  start: {restaurant: a dict of what it begins with instead
    of the header's: nn, tt ((R, K_i) pairs), w [R], E, Zm, res, dead}; only: the restaurants that are walked -- the others
    keep what they began with and their outputs mean nothing.  Neither given, nothing here is touched."""
    K = np.asarray(K, dtype=np.int64)
    I = K.shape[0]
    R = int(particles)
    assert 1 <= R <= MAXR and 0.0 <= tau <= 1.0
    koff = np.concatenate([[0], np.cumsum(K)]).astype(np.int64)
    coff = np.asarray(coff, dtype=np.int64)
    Cn = np.diff(coff)
    C = int(coff[-1])
    bpar = np.array(np.broadcast_to(np.asarray(bpar, dtype=np.float64), (I,)))
    n = np.asarray(n, dtype=np.int64)
    t = np.asarray(t, dtype=np.int64)
    stride = None if lik is None else np.asarray(lik).shape[1]
    skip = skipped_mask(K, Cn, R, stride)
    nn = [np.tile(n[koff[i]:koff[i + 1]], (R, 1)) for i in range(I)]      # (R, K_i) a restaurant
    tt = [np.tile(t[koff[i]:koff[i + 1]], (R, 1)) for i in range(I)]
    w = np.ones((I, R))
    E = np.zeros(I, dtype=np.int64)
    Zm = np.ones(I)
    S1s = np.full(I, float(R))
    res = np.zeros(I, dtype=np.int64)
    dead = np.zeros(I, dtype=bool)
    anc = [[] for _ in range(I)]
    steps = [[] for _ in range(I)]
    out = {"skipped": int(skip.sum()), "impossible": 0, "stuck": 0}
    walk = ~skip
    if only is not None:
        walk = walk & np.isin(np.arange(I), np.fromiter(only, dtype=np.int64))
    for i, s0 in (start or {}).items():
        if "nn" in s0:
            nn[i], tt[i] = np.array(s0["nn"], dtype=np.int64), np.array(s0["tt"], dtype=np.int64)
            assert nn[i].shape == tt[i].shape == (R, int(K[i]))
        w[i] = s0.get("w", w[i])
        E[i], Zm[i], res[i], dead[i] = s0.get("E", 0), s0.get("Zm", 1.0), s0.get("res", 0), s0.get("dead", False)
    key0 = np.uint64(particle_key(seed, sweep, 0))
    cls_full = None if cls is None else np.asarray(cls)
    for j in range(int(Cn[walk].max()) if walk.any() else 0):
        act = [i for i in range(I) if walk[i] and Cn[i] > j]
        # the call's restaurants: the active ones, each followed by one without dishes that holds the customers up to the
        # next one's (skipped there); before the first, one that holds the customers ahead of it
        Kc, co, bp = [0], [0], [1.0]
        for i in act:
            co.append(int(coff[i]) + j)
            Kc.append(int(K[i]))
            bp.append(float(bpar[i]))
            co.append(int(coff[i]) + j + 1)
            Kc.append(0)
            bp.append(1.0)
        co.append(C)
        pre = {i: (nn[i].copy(), tt[i].copy()) for i in act} if trace else None
        pj = np.zeros((len(act), R))
        pb = np.zeros((len(act), R))
        for r in range(R):
            n_r = np.concatenate([nn[i][r] for i in act])
            t_r = np.concatenate([tt[i][r] for i in act])
            h_r = None if h is None else np.concatenate([np.asarray(h)[koff[i]:koff[i + 1]] for i in act])
            rp = sto.replay(Kc, n_r, t_r, h_r, a, bp, co, cls_full, lik, M=M, seed=seed, sweep=sweep + r, particles=1, bars=True)
            out["impossible"] += rp["impossible"]
            out["stuck"] += rp["stuck"]
            o = 0
            for m, i in enumerate(act):
                Ki = int(K[i])
                nn[i][r] = rp["n"][o:o + Ki]
                tt[i][r] = rp["t"][o:o + Ki]
                o += Ki
                pj[m, r] = rp["p"][int(coff[i]) + j]
                pb[m, r] = rp["pbar"][int(coff[i]) + j, 0]
        for m, i in enumerate(act):
            if dead[i]:
                continue
            c = int(coff[i]) + j
            wi = w[i] * pj[m]                                                   # 1.
            st = {"p": pj[m].copy(), "pbar": pb[m].copy(), "resampled": False}
            if trace:
                st["n0"], st["t0"] = pre[i]
            posi = [r for r in range(R) if wi[r] > 0.0]
            if not posi:                                                        # 2.
                dead[i] = True
                w[i] = wi
                st["dead"] = True
                steps[i].append(st)
                continue
            e = max(ilogb(wi[r]) for r in posi)
            kept = np.array([wi[r] > 0.0 and ilogb(wi[r]) >= e - 1000 for r in range(R)])
            wi = np.array([math.ldexp(wi[r], -e) if kept[r] else 0.0 for r in range(R)])
            E[i] += e
            cum, S1 = _scan_last(wi, R, linear=(mut == "linear"))               # 3.
            _, S2 = _scan_last(wi * wi, R, linear=(mut == "linear"))
            st.update({"e": e, "kept": kept, "S1": S1})
            S1s[i] = S1
            if j + 1 < Cn[i] and S1 * S1 < (tau * float(R)) * S2:               # 4.
                z = Zm[i] * (S1 / float(R)) if mut != "noS1" else Zm[i]         # 5.
                ez = ilogb(z)
                Zm[i] = math.ldexp(z, -ez)
                E[i] += ez
                u4 = float(unit(key0, np.uint64(2 * c + 1) if mut != "u4" else np.uint64(2 * C + 1 + c)))
                A = np.zeros(R, dtype=np.int64)
                for s in range(R):
                    thr = ((float(s) + u4) / float(R)) * S1
                    hit = [r for r in posi if kept[r] and cum[r] > thr]
                    A[s] = hit[0] if hit else max(r for r in posi if kept[r])
                nn[i], tt[i] = nn[i][A].copy(), tt[i][A].copy()
                wi = np.ones(R)
                res[i] += 1
                anc[i].append((c, A))
                st.update({"resampled": True, "ez": ez, "anc": A})
            w[i] = wi
            steps[i].append(st)
    H = np.zeros(I)
    for i in range(I):
        if skip[i] or Cn[i] == 0:
            continue
        if dead[i]:
            H[i] = NEG_INF
            continue
        v = Zm[i] * (S1s[i] / float(R))                                         # 6.
        with np.errstate(divide="ignore"):
            H[i] = float(np.log(v)) + (float(E[i]) * LN2 if mut != "noE" else 0.0) if v > 0.0 else NEG_INF
    pn = np.zeros(int(koff[-1]) * R, dtype=np.uint32)
    pt = np.zeros(int(koff[-1]) * R, dtype=np.uint16)
    for i in range(I):
        if not skip[i]:
            o = int(koff[i]) * R
            pn[o:o + R * int(K[i])] = nn[i].reshape(-1)
            pt[o:o + R * int(K[i])] = tt[i].reshape(-1)
    out.update({"pn": pn, "pt": pt, "w": w, "E": E, "Zm": Zm, "res": res.astype(np.uint32), "anc": anc, "H": H, "skip": skip,
                "dead": int(dead.sum()), "resamplings": int(res.sum()), "dead_mask": dead, "S1": S1s})
    if trace:
        out["steps"] = steps
    return out


# ---------------------------------------------------------------------------------------------------- the truth

def _exact_p(nn, tt, hs, L, a: Fraction, b: Fraction, Mb: int):
    """the visit's p on the pairs (nn, tt) as a Fraction; L None: a class outside the matrix"""
    if L is None:
        return Fraction(0)
    N, T = int(sum(nn)), int(sum(tt))
    if N == 0:
        return sum((Lk * hk for Lk, hk in zip(L, hs)), Fraction(0))
    g = b + T * a
    num = Fraction(0)
    for nk, tk, hk, Lk in zip(nn, tt, hs, L):
        nk, tk = int(nk), int(tk)
        num += Lk * (nk - tk * a + (0 if (nk >= 1 and tk + 1 > Mb) else g * hk))
    return num / (b + N)


def truth(K, n, t, h, a, bpar, coff, cls, lik, M, seed, sweep, particles, tau, restaurants=None):
    """(rep, H_true [I], H_bar [I]): the traced replay; the docstring's bar of every restaurant that was not skipped (from
    the replay's own p and bar(p): no exact arithmetic); and along the replay's path the truth of H for the restaurants
    listed (None: all), NaN for the others"""
    mp = sto.hp._mp()
    rep = replay(K, n, t, h, a, bpar, coff, cls, lik, M, seed, sweep, particles, tau, trace=True)
    K = np.asarray(K, dtype=np.int64)
    I, R = K.shape[0], int(particles)
    koff = np.concatenate([[0], np.cumsum(K)]).astype(np.int64)
    coff = np.asarray(coff, dtype=np.int64)
    Mb = int(M) if M else 65535
    bpar = np.broadcast_to(np.asarray(bpar, dtype=np.float64), (I,))
    fa = Fraction(float(a))
    Ht, Hb = np.zeros(I), np.zeros(I)
    listed = set(range(I) if restaurants is None else restaurants)
    for i in range(I):
        if rep["skip"][i] or coff[i + 1] == coff[i]:
            continue
        exact = i in listed
        if not exact:
            Ht[i] = math.nan
        Ki, k0 = int(K[i]), int(koff[i])
        hs = [Fraction(float(h[k0 + k])) if h is not None else Fraction(1) for k in range(Ki)] if exact else None
        fb = Fraction(float(bpar[i]))
        w = [mp.mpf(1)] * R
        rho = [0.0] * R
        Zm, rhoZ, E = mp.mpf(1), 0.0, 0
        S1, rhoS = mp.mpf(R), 0.0
        isdead = False
        for j, st in enumerate(rep["steps"][i]):
            c = int(coff[i]) + j
            L = None
            if exact and lik is None:
                L = [Fraction(1)] * Ki
            elif exact and int(cls[c]) < lik.shape[0]:
                L = [Fraction(float(lik[int(cls[c]), k])) for k in range(Ki)]
            for r in range(R):
                if exact:
                    p = _exact_p(st["n0"][r], st["t0"][r], hs, L, fa, fb, Mb)
                    assert (p == 0) == (st["p"][r] == 0.0), (i, j, r, p, st["p"][r])
                    w[r] = w[r] * (mp.mpf(p.numerator) / mp.mpf(p.denominator))
                if st["p"][r] > 0.0:
                    rho[r] += st["pbar"][r] / st["p"][r] + U
            if st.get("dead"):
                isdead = True
                break
            E += st["e"]
            rhoS = max(rho[r] for r in range(R) if st["kept"][r]) + (R - 1) * U
            if exact:
                w = [mp.ldexp(w[r], -st["e"]) if st["kept"][r] else mp.mpf(0) for r in range(R)]
                S1 = mp.fsum(w)
            if st["resampled"]:
                E += st["ez"]
                rhoZ += rhoS + 2.0 * U
                rho = [0.0] * R
                if exact:
                    Zm = mp.ldexp(Zm * (S1 / R), -st["ez"])
                    w = [mp.mpf(1)] * R
        if isdead:
            Ht[i] = NEG_INF
            continue
        assert E == int(rep["E"][i])
        lv = float(mp.log(Zm * (S1 / R))) if exact else float(np.log(rep["Zm"][i] * (rep["S1"][i] / R)))
        if exact:
            Ht[i] = float(mp.log(Zm * (S1 / R)) + E * mp.log(2))
        Habs = abs(Ht[i]) if exact else abs(rep["H"][i])
        Hb[i] = ((rhoZ + rhoS + 2.0 * U) + 2.0 * U * abs(lv) + 2.0 * U * abs(E * LN2) + U * Habs) * sto.SLACK
    return rep, Ht, Hb


# ---------------------------------------------------------------------------------------------------- exact law, R = 2

def enumerate_filter(hs, a: float, b: float, cls, lik, M, tau: float):
    """every joint path of R = 2 slots from empty pairs, the uniforms integrated out, the systematic resampling's law
    included (P(A = (0,0)) = max(0, 2 W0 - 1), P(A = (1,1)) = 1 - min(1, 2 W0), (0,1) the rest, W0 = w0 / S1): returns
    (sum P Zhat, sum P, leaves that resampled at least once, leaves that never did)"""
    K, R = len(hs), 2
    Mb = M or 65535
    tot = [0.0, 0.0, 0, 0]

    def moves(nn, tt, c):
        T, N = sum(tt), sum(nn)
        g, den = b + T * a, b + N
        xs = [nn[k] - tt[k] * a for k in range(K)]
        ys = [0.0 if (nn[k] >= 1 and tt[k] + 1 > Mb) else g * hs[k] for k in range(K)]
        th = [hs[k] if N == 0 else (xs[k] + ys[k]) / den for k in range(K)]
        q = [th[k] * lik[cls[c]][k] for k in range(K)]
        Z = sum(q)
        pc = Z
        if not Z > 0.0:
            pc, q, Z = 0.0, th, sum(th)
        out = []
        for k in range(K):
            if q[k] <= 0.0:
                continue
            heads = [(True, 1.0)] if nn[k] == 0 else [(True, ys[k] / (xs[k] + ys[k])), (False, xs[k] / (xs[k] + ys[k]))]
            for new, ph in heads:
                if ph > 0.0:
                    n2, t2 = list(nn), list(tt)
                    n2[k] += 1
                    t2[k] += int(new)
                    out.append((q[k] / Z * ph, pc, tuple(n2), tuple(t2)))
        return out

    def walk(c, states, w, Zm, P, nres):
        for P0, p0, n0, t0 in moves(*states[0], c):
            for P1, p1, n1, t1 in moves(*states[1], c):
                w2 = (w[0] * p0, w[1] * p1)
                P2 = P * P0 * P1
                S1, S2 = w2[0] + w2[1], w2[0] * w2[0] + w2[1] * w2[1]
                s2 = ((n0, t0), (n1, t1))
                if c + 1 == len(cls):
                    tot[0] += P2 * Zm * (S1 / R)
                    tot[1] += P2
                    tot[2 if nres else 3] += 1
                elif S1 > 0.0 and S1 * S1 < (tau * R) * S2:
                    W0 = w2[0] / S1
                    for A, PA in (((0, 0), max(0.0, 2.0 * W0 - 1.0)), ((1, 1), 1.0 - min(1.0, 2.0 * W0)),
                                  ((0, 1), 1.0 - max(0.0, 2.0 * W0 - 1.0) - (1.0 - min(1.0, 2.0 * W0)))):
                        if PA > 0.0:
                            walk(c + 1, (s2[A[0]], s2[A[1]]), (1.0, 1.0), Zm * (S1 / R), P2 * PA, nres + 1)
                else:
                    walk(c + 1, s2, w2, Zm, P2, nres)

    empty = (tuple([0] * K), tuple([0] * K))
    walk(0, (empty, empty), (1.0, 1.0), 1.0, 1.0, 0)
    return tuple(tot)


# ---------------------------------------------------------------------------------------------------- the cases

SEED, SWEEP = 0x9F17, 2


def make_case(shapes, a: float, seed: int, rows: int = 5, start: bool = True, dead_class=None):
    """(K, n, t, h, bpar, coff, cls, lik) for shapes = [(K_i, customers_i)]: a non-empty start state in every second restaurant (start), a matrix of
    `rows` classes over the largest K_i whose entries span four decades (so that the weights part); with a > 0 every third restaurant has
    -a < b <= 0.  dead_class: that row of the matrix is all zero"""
    rng = np.random.default_rng(seed)
    K = np.array([s[0] for s in shapes], dtype=np.int32)
    Cn = np.array([s[1] for s in shapes], dtype=np.int64)
    G = int(K.sum())
    n = np.zeros(G, dtype=np.uint32)
    t = np.zeros(G, dtype=np.uint16)
    if start:
        n = rng.integers(0, 6, G).astype(np.uint32)
        n[np.repeat(np.arange(len(K)) % 2 == 0, K)] = 0        # (the even ones start empty: their weights part soonest)
        t = np.where(n > 0, np.minimum(1 + rng.integers(0, 2, G), n), 0).astype(np.uint16)
    h = rng.dirichlet(np.ones(max(int(K.max()), 1)))[np.concatenate([np.arange(k) for k in K])] if G else np.zeros(0)
    h = np.asarray(h, dtype=np.float64)
    bpar = rng.uniform(0.5, 3.0, len(K))
    if a > 0:
        bpar[::3] = -a * rng.uniform(0.0, 0.9, len(bpar[::3]))
    coff = np.concatenate([[0], np.cumsum(Cn)]).astype(np.uint64)
    cls = rng.integers(0, rows, int(coff[-1])).astype(np.uint32)
    lik = np.exp(rng.uniform(math.log(1e-4), 0.0, (rows, max(int(K.max()), 1))))
    if dead_class is not None:
        lik[dead_class] = 0.0
    return K, n, t, h, bpar, coff, cls, lik


@lru_cache(maxsize=None)
def host_case():
    """a small raw case for the CPU tests: K over a block edge, a non-empty start state, 40 customers each"""
    return make_case([(1, 40), (2, 40), (5, 40), (64, 40), (65, 40), (7, 0)], 0.5, 77)


MIX_K = (1, 2, 63, 64, 65, 130)
MIX_C = (0, 1, 64, 65, 130)


def mix_shapes():
    """37 restaurants: every K of MIX_K with every customer count of MIX_C (130 customers only where K <= 2: the replay's
    cost), and seven more around the block edges"""
    sh = [(k, c if (c < 130 or k <= 2) else 66) for k in MIX_K for c in MIX_C]
    return sh + [(3, 7), (64, 2), (65, 3), (130, 9), (17, 64), (128, 5), (0, 0)]


@lru_cache(maxsize=None)
def mix_case(a: float):
    return make_case(mix_shapes(), a, 1234)


def partial_case():
    """one restaurant in which a slot dies while the others live: dish 0 is all but impossible to open (h = 1e-305), the
    first class splits the slots evenly over the two dishes and the second one can sit at dish 0 only -- a slot that
    has nobody there falls 1e-305 behind, past the 2^-1000 of step 2"""
    K = np.array([2], dtype=np.int32)
    h = np.array([1e-305, 1.0])
    lik = np.array([[1.0, 1e-305], [1.0, 0.0]])
    cls = np.array([0, 1, 1, 0, 1], dtype=np.uint32)
    coff = np.array([0, 5], dtype=np.uint64)
    return K, np.zeros(2, dtype=np.uint32), np.zeros(2, dtype=np.uint16), h, np.array([1.0]), coff, cls, lik


# ---------------------------------------------------------------------------------------------------- the chains

# A launch of more than GRID_CAP restaurants: workgroup g takes restaurant g, then GRID_CAP + g, then 2 GRID_CAP + g.  The
# listed restaurants are three such trips of the first CHAIN_M workgroups, (K_i, customers_i) each; every other
# restaurant of the launch has no dishes and no customers.  Down a column: register form -> LDS form -> register form,
# LDS -> register -> register, a dead restaurant -> a live one, no customers -> some and some -> none; at 39 particles
# K_i = 130 fills the LDS, at 40 those five are skipped.
CHAIN_A = 0.5
CHAIN_M = 8
CHAIN_TRIPS = (((5, 21), (130, 9), (3, 20), (64, 20), (130, 6), (2, 0), (65, 12), (1, 7)),
               ((130, 8), (3, 22), (65, 9), (1, 5), (2, 23), (64, 19), (128, 6), (5, 20)),
               ((2, 20), (64, 13), (130, 7), (5, 0), (63, 21), (3, 9), (1, 6), (130, 5)))
CHAIN_DEAD = 2                                    # the listed restaurant that dies mid-document (trip 0)
CHAIN_RUNS = ((4, 0.5), (39, 1.0), (40, 0.5))     # (particles, tau)
CHAIN_VARIANTS = ("keepE", "keepZ", "keepw", "keepdead", "keepres", "stale")


@lru_cache(maxsize=None)
def chain_case():
    """(case, full): the listed restaurants alone, in launch order, as make_case's tuple, and the whole launch of
    I = 2 GRID_CAP + CHAIN_M restaurants as a dict: I, K, koff, coff, bpar (full length; a filler's b is 1) and
    listed (the listed restaurants' indices, ascending).  The fillers hold neither dishes nor customers, so n, t, h, cls
    and lik are the compact case's and the listed restaurants' offsets are the compact case's too."""
    trips = len(CHAIN_TRIPS)
    shapes = [s for tr in CHAIN_TRIPS for s in tr]
    K, n, t, h, bpar, coff, cls, lik = make_case(shapes, CHAIN_A, 777, rows=6, dead_class=5)
    cls = np.where(cls == 5, 0, cls).astype(np.uint32)
    cls[int(coff[CHAIN_DEAD]) + 9] = 5              # restaurant 2 of trip 0 dies at its tenth customer
    listed = (np.arange(trips, dtype=np.int64)[:, None] * GRID_CAP + np.arange(CHAIN_M, dtype=np.int64)[None, :]).reshape(-1)
    I = (trips - 1) * GRID_CAP + CHAIN_M
    Kf, Cf, bf = np.zeros(I, dtype=np.int32), np.zeros(I, dtype=np.int64), np.ones(I)
    Kf[listed], Cf[listed], bf[listed] = K, np.diff(coff.astype(np.int64)), bpar
    full = {"I": I, "K": Kf, "koff": np.concatenate([[0], np.cumsum(Kf, dtype=np.int64)]).astype(np.uint64),
            "coff": np.concatenate([[0], np.cumsum(Cf)]).astype(np.uint64), "bpar": bf, "listed": listed}
    for x in (K, n, t, h, bpar, coff, cls, lik) + tuple(v for v in full.values() if isinstance(v, np.ndarray)):
        x.setflags(write=False)
    return (K, n, t, h, bpar, coff, cls, lik), full


def chain_exact(case):
    """the listed restaurants whose truth is cheap"""
    K, coff = case[0], case[5].astype(np.int64)
    return [i for i in range(len(K)) if K[i] <= 65 and 0 < coff[i + 1] - coff[i] <= 12]


@lru_cache(maxsize=None)
def chain_truth(R: int, tau: float):
    """(rep, H_true, H_bar) of the compact chain case at pf.SEED, pf.SWEEP, M = 0"""
    case, _ = chain_case()
    K, n, t, h, bpar, coff, cls, lik = case
    return truth(K, n, t, h, CHAIN_A, bpar, coff, cls, lik, 0, SEED, SWEEP, R, tau, restaurants=chain_exact(case))


def chain_pred(rep, i: int):
    """the restaurant whose registers and LDS a workgroup still holds when it starts listed restaurant i: the nearest one
    up its column that was not skipped (a skipped one leaves before it touches either); None on the first trip"""
    p = i - CHAIN_M
    while p >= 0 and rep["skip"][p]:
        p -= CHAIN_M
    return p if p >= 0 else None


def chain_variant(case, rep, R: int, tau: float, variant: str):
    """What a kernel that forgot one reset between a workgroup's trips would return for the compact chain case: rep's pn,
    pt, w, E, Zm, res, H and dead_mask with the restaurants of trips 1 and 2 replayed from the hand-over instead of the
    header's start, a trip at a time, each from what the variant left behind on the trip before.
      keepE, keepZ, keepres: E, Zm, res start from the predecessor's final value;  keepw: the weights do;
      keepdead: the successor of a dead restaurant starts dead;
      stale: dish k < min(K_i, K_pred) of every slot starts from the predecessor's final pair, not from the start state."""
    assert variant in CHAIN_VARIANTS
    K, n, t, h, bpar, coff, cls, lik = case
    koff = np.concatenate([[0], np.cumsum(np.asarray(K, dtype=np.int64))])
    cur = {f: np.array(rep[f]) for f in ("pn", "pt", "w", "E", "Zm", "res", "H", "dead_mask")}

    def pairs(f, i):
        return cur[f][int(koff[i]) * R:int(koff[i + 1]) * R].reshape(R, int(K[i])).astype(np.int64)

    m = CHAIN_M
    for trip in range(1, len(K) // m):
        start = {}
        for i in range(trip * m, (trip + 1) * m):
            p = chain_pred(rep, i)
            if rep["skip"][i] or p is None:
                continue
            if variant == "keepE":
                start[i] = {"E": int(cur["E"][p])}
            elif variant == "keepZ":
                start[i] = {"Zm": float(cur["Zm"][p])}
            elif variant == "keepres":
                start[i] = {"res": int(cur["res"][p])}
            elif variant == "keepw":
                start[i] = {"w": cur["w"][p].copy()}
            elif variant == "keepdead":
                if cur["dead_mask"][p]:
                    start[i] = {"dead": True}
            else:
                kk = int(min(K[i], K[p]))
                nn = np.tile(np.asarray(n, dtype=np.int64)[koff[i]:koff[i + 1]], (R, 1))
                tt = np.tile(np.asarray(t, dtype=np.int64)[koff[i]:koff[i + 1]], (R, 1))
                nn[:, :kk], tt[:, :kk] = pairs("pn", p)[:, :kk], pairs("pt", p)[:, :kk]
                start[i] = {"nn": nn, "tt": tt}
        if not start:
            continue
        rv = replay(K, n, t, h, CHAIN_A, bpar, coff, cls, lik, 0, SEED, SWEEP, R, tau, start=start, only=start.keys())
        for i in start:
            sl = slice(int(koff[i]) * R, int(koff[i + 1]) * R)
            cur["pn"][sl], cur["pt"][sl] = rv["pn"][sl], rv["pt"][sl]
            for f in ("w", "E", "Zm", "res", "H", "dead_mask"):
                cur[f][i] = rv[f][i]
    return cur
