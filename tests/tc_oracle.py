"""numpy restatement of the table-count sweep of stb_tcounts_* / stb_sample_tcounts (include/stb_hip.h), the checker of
tests/test_tcounts_host.py and tests/test_gpu_tcounts.py.

A table is (S1, packed cells, M): S1[n-1] = log S^n_1 and the cells of orc.fill_S's layout (rows n = 3.., m = 2 ..
min(n-1, M)); DeviceTables.packed_host gives the device's own slab in the same layout.
"""
from __future__ import annotations

import numpy as np

import orc
from libstb_amd import synth

TIE = 1e-9  # a draw with |u W - C(tau)| <= TIE W for some tau is reported as a near-tie


def sweep_key(seed: int, s: int) -> int:
    return int(synth.splitmix64(s + 1, seed)[s])


def uniforms(seed: int, s: int, G: int) -> np.ndarray:
    """u of flat pairs g = 0 .. G-1 in sweep s"""
    return synth.unit(G, sweep_key(seed, s))


def S_row(n: int, tmax: int, S1, tab, M: int) -> np.ndarray:
    """S_S(n, tau) for tau = 1 .. tmax (tmax <= min(n, M)), the semantics of stb_lookup_S"""
    out = np.empty(tmax)
    out[0] = 0.0 if n == 1 else S1[n - 1]
    hi = min(tmax, n - 1)
    if hi >= 2:
        o = orc.row_offset(n, M)
        out[1:hi] = tab[o:o + hi - 1]
    if tmax == n and n >= 2:
        out[n - 1] = 0.0
    return out


def log_weights(n: int, Tm: int, a: float, b: float, h: float, M: int, S1, tab, Mt: int) -> np.ndarray:
    """log w(tau), tau = 1 .. min(n, M): S_S(n, tau) + (tau-1) log h + sum_{s=Tm+1}^{Tm+tau-1} log(b + s a)"""
    tmax = min(n, M)
    tau = np.arange(1, tmax + 1, dtype=np.float64)
    terms = np.log(b + (Tm + tau[1:] - 1.0) * a)
    L = np.concatenate([[0.0], np.cumsum(terms)])
    return S_row(n, tmax, S1, tab, Mt) + (tau - 1.0) * np.log(h) + L


def draw(lw: np.ndarray, u: float):
    """(tau, near-tie): the smallest tau with C(tau) > u W, weights scaled by exp(-max log w), W = C(tau_max)"""
    C = np.cumsum(np.exp(lw - lw.max()))
    W = C[-1]
    tau = int(np.searchsorted(C, u * W, side="right")) + 1
    return tau, bool(np.any(np.abs(u * W - C) <= TIE * W))


def sweep(K, n, t, h, a, bpar, M, S1, tab, Mt, seed, s):
    """one sweep; returns (t, T, near-ties).  h None: all 1."""
    t = np.array(t, dtype=np.uint16)
    u = uniforms(seed, s, len(n))
    koff = np.concatenate([[0], np.cumsum(K)]).astype(np.int64)
    T = np.zeros(len(K), dtype=np.uint32)
    ties = 0
    for i in range(len(K)):
        Ti = int(t[koff[i]:koff[i + 1]].astype(np.int64).sum())
        for g in range(koff[i], koff[i + 1]):
            ng, tg = int(n[g]), int(t[g])
            if ng == 0:
                continue
            if min(ng, M) == 1:
                new = 1
            else:
                lw = log_weights(ng, Ti - tg, a, float(bpar[i]), 1.0 if h is None else float(h[g]), M, S1, tab, Mt)
                new, tie = draw(lw, float(u[g]))
                ties += tie
            Ti += new - tg
            t[g] = new
        T[i] = Ti
    return t, T, ties


def log_joint(ns, ts, a, b, hs, S1, tab, M):
    """log of the PYP joint (b|a)_T prod_k S^{n_k}_{t_k,a} h_k^{t_k} of one restaurant (up to a constant)"""
    T = int(sum(ts))
    v = float(np.sum(np.log(b + np.arange(T) * a))) if T else 0.0
    for nk, tk, hk in zip(ns, ts, hs):
        v += S_row(nk, tk, S1, tab, M)[tk - 1] + tk * np.log(hk)
    return v
