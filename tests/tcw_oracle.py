"""numpy restatement of the windowed table-count sweep of stb_tcounts_sweep_window / stb_sample_tcounts_window
(include/stb_hip.h), the checker of tests/test_tcwin_host.py and tests/test_gpu_tcwin.py, and the exact transition
matrices of that chain (and of the reference's, without the acceptance test) for small restaurants.

Tables as in tests/tc_oracle.py: (S1, packed cells, M).
"""
from __future__ import annotations

import itertools

import numpy as np

import tc_oracle as tco
from libstb_amd import synth

TIE = tco.TIE  # a proposal with |u1 Z - C(tau)| <= TIE Z, or an acceptance with |u2 Z' - Z| <= TIE max(Z, u2 Z'), is a near-tie


def uniforms(seed: int, s: int, G: int):
    """(u1, u2) of flat pairs g = 0 .. G-1 in sweep s: elements 2g+1 and 2g+2 of the stream (array entries 2g, 2g+1)"""
    u = synth.unit(2 * G, tco.sweep_key(seed, s))
    return u[0::2], u[1::2]


def window(x: int, W: int, Mt: int):
    """[lo(x), hi(x)] = [max(1, x - W), min(Mt, x + W)]"""
    return max(1, x - W), min(Mt, x + W)


def step(lw: np.ndarray, t: int, W: int, u1: float, u2: float, ref: bool):
    """one visit given log w(tau), tau = 1 .. Mt: (new t, near-tie of the proposal, near-tie of the acceptance)"""
    Mt = len(lw)
    lo, hi = window(t, W, Mt)
    C = np.cumsum(np.exp(lw[lo - 1:hi] - lw[lo - 1:hi].max()))
    Z = C[-1]
    tp = lo + int(np.searchsorted(C, u1 * Z, side="right"))
    tie1 = bool(np.any(np.abs(u1 * Z - C) <= TIE * Z))
    if ref or tp == t:
        return tp, tie1, False
    lp, hp = window(tp, W, Mt)
    lo2, hi2 = min(lo, lp), max(hi, hp)
    m2 = lw[lo2 - 1:hi2].max()
    Zt = float(np.sum(np.exp(lw[lo - 1:hi] - m2)))
    Zp = float(np.sum(np.exp(lw[lp - 1:hp] - m2)))
    tie2 = abs(u2 * Zp - Zt) <= TIE * max(Zt, u2 * Zp)
    return (tp if u2 * Zp < Zt else t), tie1, bool(tie2)


def sweep(K, n, t, h, a, bpar, M, S1, tab, Mt_tab, W, seed, s, ref=False, N=None):
    """one windowed sweep; returns (t, T, near-ties).  h None: all 1.  Pairs with n > N (when N is given) keep t."""
    t = np.array(t, dtype=np.uint16)
    u1, u2 = uniforms(seed, s, len(n))
    koff = np.concatenate([[0], np.cumsum(K)]).astype(np.int64)
    T = np.zeros(len(K), dtype=np.uint32)
    ties = 0
    for i in range(len(K)):
        Ti = int(t[koff[i]:koff[i + 1]].astype(np.int64).sum())
        for g in range(koff[i], koff[i + 1]):
            ng, tg = int(n[g]), int(t[g])
            if ng == 0 or (N is not None and ng > N):
                continue
            if min(ng, M) == 1:
                new = 1
            else:
                lw = tco.log_weights(ng, Ti - tg, a, float(bpar[i]), 1.0 if h is None else float(h[g]), M, S1, tab, Mt_tab)
                new, t1, t2 = step(lw, tg, W, float(u1[g]), float(u2[g]), ref)
                ties += t1 + t2
            Ti += new - tg
            t[g] = new
        T[i] = Ti
    return t, T, ties


# ---- exact laws --------------------------------------------------------------------------------------------------

def states(ns, M=None):
    return list(itertools.product(*[range(1, min(nk, M or nk) + 1) for nk in ns]))


def joint(ns, hs, a, b, S1, tab, M):
    """tco.log_joint over states(ns, M), normalised"""
    lj = np.array([tco.log_joint(ns, ts, a, b, hs, S1, tab, M) for ts in states(ns, M)])
    p = np.exp(lj - lj.max())
    return p / p.sum()


def pair_kernel(lw: np.ndarray, W: int, ref: bool) -> np.ndarray:
    """the Mt x Mt transition matrix of one visit given log w: the proposal w restricted to win(t), accepted with
    min(1, Z(t) / Z(tau')) (ref: always)"""
    Mt = len(lw)
    w = np.exp(lw - lw.max())
    Z = np.array([w[window(x, W, Mt)[0] - 1:window(x, W, Mt)[1]].sum() for x in range(1, Mt + 1)])
    P = np.zeros((Mt, Mt))
    for x in range(1, Mt + 1):
        lo, hi = window(x, W, Mt)
        for y in range(lo, hi + 1):
            if y != x:
                P[x - 1, y - 1] = w[y - 1] / Z[x - 1] * (1.0 if ref else min(1.0, Z[x - 1] / Z[y - 1]))
        P[x - 1, x - 1] = 1.0 - P[x - 1].sum()
    return P


def sweep_matrix(ns, hs, a, b, W, S1, tab, M, ref=False) -> np.ndarray:
    """the transition matrix over states(ns, M) of one sweep of one restaurant (pairs in order)"""
    st = states(ns, M)
    idx = {s: j for j, s in enumerate(st)}
    P = np.eye(len(st))
    for k in range(len(ns)):
        A = np.zeros((len(st), len(st)))
        for s in st:
            Tm = sum(s) - s[k]
            lw = tco.log_weights(ns[k], Tm, a, b, hs[k], M, S1, tab, M)
            Pk = pair_kernel(lw, W, ref)
            for tn in range(1, len(lw) + 1):
                q = Pk[s[k] - 1, tn - 1]
                if q:
                    A[idx[s], idx[s[:k] + (tn,) + s[k + 1:]]] += q
        P = P @ A
    return P


def stationary(P: np.ndarray) -> np.ndarray:
    """the stationary distribution of a row-stochastic matrix (pi P = pi, sum pi = 1)"""
    m = P.shape[0]
    A = np.vstack([P.T - np.eye(m), np.ones(m)])
    rhs = np.zeros(m + 1)
    rhs[-1] = 1.0
    return np.linalg.lstsq(A, rhs, rcond=None)[0]
