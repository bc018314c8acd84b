"""numpy restatement of the table-indicator sweep of stb_tindic_* / stb_sample_tindic (include/stb_hip.h), the checker of
tests/test_tindic_host.py and tests/test_gpu_tindic.py, and the exact transition matrices of that chain.

A V table is VTab(packed, N, M): the cells V^n_m, rows n = 2 .. N, m = 2 .. min(n, M), back to back without padding --
orc.fill_V's layout, and what capi.DeviceVTables.packed_host gives of the device's own slab, so the oracle's draws see the
same cells as the device's.
"""
from __future__ import annotations

import itertools
import math

import numpy as np

from libstb_amd import synth


class VTab:
    def __init__(self, packed, N: int, M: int):
        self.v, self.N, self.M = np.asarray(packed, dtype=np.float64), N, M
        lens = [0, 0] + [min(n - 1, M - 1) for n in range(2, N + 1)]
        self.off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)  # off[n]: first cell of row n

    def V(self, n: int, m: int) -> float:
        """stb_lookup_V's semantics: 0 outside 2 <= m <= min(n, M), 2 <= n <= N"""
        if m < 2 or n < 2 or m > n or n > self.N or m > self.M:
            return 0.0
        return float(self.v[self.off[n] + m - 2])


def sweep_key(seed: int, s: int) -> int:
    return int(synth.splitmix64(s + 1, seed)[s])


def uniforms(seed: int, s: int, C: int) -> np.ndarray:
    """(u1, u2) of flat customers c = 0 .. C-1 in sweep s: elements 2c and 2c+1 of unit(2C, key_s)"""
    u = synth.unit(2 * C, sweep_key(seed, s))
    return u[0::2], u[1::2]


def odds(n: int, t: int, T: int, h: float, a: float, b: float, V: float, ref: bool) -> float:
    """h (b + T a) t / (n - t) V, left to right in doubles (ref: / (n - t + 1))"""
    return h * (b + float(T) * a) * float(t) / float(n - t + 1 if ref else n - t) * V


def visit(n: int, t: int, T: int, h: float, a: float, b: float, vt, u1: float, u2: float, ref: bool, N: int):
    """one customer of pair (n, t, h) in a restaurant with total T: the new (t, T)"""
    if n <= 1 or n > N:
        return t, T
    if t > 1 and float(n - 1) * u1 < float(t - 1):
        t, T = t - 1, T - 1
    o = odds(n, t, T, h, a, b, vt.V(n, t + 1), ref)
    p = 1.0 if math.isinf(o) else o / (o + 1.0)
    if u2 < p:
        t, T = t + 1, T + 1
    return t, T


def pair_order(K, n):
    """cust of pair order: every restaurant's pairs k repeated n_k times"""
    out, g = [], 0
    for Ki in K:
        for k in range(int(Ki)):
            out.extend([k] * int(n[g]))
            g += 1
    return np.array(out, dtype=np.uint32)


def sweep(K, n, t, h, a, bpar, vt, N, seed, s, cust=None, ref=False):
    """one sweep; returns (t, T).  h None: all 1; cust None: pair order."""
    K = np.asarray(K)
    t = np.array(t, dtype=np.int64)
    if cust is None:
        cust = pair_order(K, n)
    C = len(cust)
    u1, u2 = uniforms(seed, s, C)
    koff = np.concatenate([[0], np.cumsum(K)]).astype(np.int64)
    T = np.zeros(len(K), dtype=np.int64)
    c = 0
    for i in range(len(K)):
        Ti = int(t[koff[i]:koff[i + 1]].sum())
        b = float(bpar[i])
        Ci = int(np.asarray(n[koff[i]:koff[i + 1]], dtype=np.int64).sum())
        for cc in range(c, c + Ci):
            g = koff[i] + int(cust[cc])
            hg = 1.0 if h is None else float(h[g])
            t[g], Ti = visit(int(n[g]), int(t[g]), Ti, hg, a, b, vt, float(u1[cc]), float(u2[cc]), ref, N)
        c += Ci
        T[i] = Ti
    return t.astype(np.uint16), T.astype(np.uint32)


# ---- exact laws --------------------------------------------------------------------------------------------------

def stirling(n: int, a: float) -> np.ndarray:
    """S^n_{m,a} for m = 0 .. n (generalised Stirling numbers: S^{k+1}_m = S^k_{m-1} + (k - m a) S^k_m), in doubles"""
    S = np.zeros(n + 1)
    S[0] = 1.0
    for k in range(n):
        new = np.zeros(n + 1)
        for m in range(1, k + 2):
            new[m] = S[m - 1] + ((k - m * a) * S[m] if m <= k else 0.0)
        S = new
    return S


class ExactV:
    """V^n_m = S^n_m / S^n_{m-1} from stirling(), with VTab's interface (bounds N, M)"""

    def __init__(self, ns, a: float, M: int | None = None):
        self.N = max(ns)
        self.M = self.N if M is None else M
        self.rows = {n: stirling(n, a) for n in set(ns)}

    def V(self, n: int, m: int) -> float:
        if m < 2 or n < 2 or m > n or m > self.M or n not in self.rows:
            return 0.0
        S = self.rows[n]
        return float(S[m] / S[m - 1])


def states(ns, M=None):
    return list(itertools.product(*[range(1, min(nk, M or nk) + 1) for nk in ns]))


def joint(ns, hs, a: float, b: float, M=None) -> np.ndarray:
    """the PYP joint (b|a)_T prod_k S^{n_k}_{t_k,a} h_k^{t_k} of one restaurant over states(ns, M), normalised"""
    S = {n: stirling(n, a) for n in set(ns)}
    p = []
    for ts in states(ns, M):
        T = sum(ts)
        v = float(np.prod([b + j * a for j in range(T)]))
        for nk, tk, hk in zip(ns, ts, hs):
            v *= S[nk][tk] * hk ** tk
        p.append(v)
    p = np.array(p)
    return p / p.sum()


def sweep_matrix(ns, hs, a: float, b: float, order, vt, ref=False, M=None) -> np.ndarray:
    """the transition matrix over states(ns, M) of one sweep of one restaurant visiting dishes `order` (a customer
    sequence of dish indices; every dish k appears ns[k] times) -- what `visit` does, with the uniforms integrated out"""
    st = states(ns, M)
    idx = {s: j for j, s in enumerate(st)}
    P = np.eye(len(st))
    for k in order:
        n = ns[k]
        A = np.zeros((len(st), len(st)))
        for s in st:
            if n <= 1:
                A[idx[s], idx[s]] = 1.0
                continue
            t, T = s[k], sum(s)
            pr = (t - 1) / (n - 1) if t > 1 else 0.0
            for tr, w in ((t - 1, pr), (t, 1.0 - pr)):
                if w == 0.0:
                    continue
                Tr = T - (t - tr)
                o = odds(n, tr, Tr, hs[k], a, b, vt.V(n, tr + 1), ref)
                p = 1.0 if math.isinf(o) else o / (o + 1.0)
                for tn, q in ((tr + 1, p), (tr, 1.0 - p)):
                    if q:
                        A[idx[s], idx[s[:k] + (tn,) + s[k + 1:]]] += w * q
        P = P @ A
    return P


def stationary(P: np.ndarray) -> np.ndarray:
    """the stationary distribution of a row-stochastic matrix (pi P = pi, sum pi = 1)"""
    m = P.shape[0]
    A = np.vstack([P.T - np.eye(m), np.ones(m)])
    rhs = np.zeros(m + 1)
    rhs[-1] = 1.0
    return np.linalg.lstsq(A, rhs, rcond=None)[0]
