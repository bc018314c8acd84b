"""numpy restatement of the dish sweep of stb_tindic_sweep_dishes / stb_sample_tdishes (include/stb_hip.h, "dishes"), the
checker of tests/test_td_oracle.py and tests/test_gpu_tdish.py, and the exact transition matrices of that chain.

V tables are ti_oracle's VTab (the device's own cells) or ExactV; the uniforms are ti_oracle's stream, u3 of customer c
element 2C + c of unit(3C, key_s).  The cumulative sums are taken in the header's association (cumsum64).
"""
from __future__ import annotations

import itertools
import math

import numpy as np

import ti_oracle as tio
from libstb_amd import synth


def AB(n: int, t: int, h: float, a: float, M: int, vt):
    """(A, B) of a pair (n, t, h): z = L (A + g B) is the weight of seating one more customer there"""
    if n == 0:
        return 0.0, h
    dn = float(n)
    if t == 1:
        U = dn - a
    else:
        V = vt.V(n, t)
        U = (dn - float(t) * a) + (1.0 / V if V != 0.0 else math.inf)
    A = U * float(n - t + 1) / dn
    if t + 1 > M:
        R = 0.0
    elif t == n:
        R = 1.0
    else:
        R = (dn - float(t + 1) * a) * vt.V(n, t + 1) + 1.0
    B = h * float(t) * R / dn
    return A, B


def cumsum64(z: np.ndarray) -> np.ndarray:
    """cumulative sums of z in the header's association: blocks of 64 (padded with 0), a Kogge-Stone inclusive scan inside
    a block, block bases added in sequence; one value per padded lane (Z is the last)"""
    K = len(z)
    nb = max(1, (K + 63) // 64)
    x = np.zeros((nb, 64))
    x.reshape(-1)[:K] = z
    d = 1
    while d < 64:
        x[:, d:] = x[:, d:] + x[:, :-d]
        d *= 2
    base = 0.0
    for j in range(nb):
        x[j] = base + x[j]
        base = x[j, 63]
    return x.reshape(-1)


def choose(z: np.ndarray, u3: float):
    """k*, or None when Z is not positive and finite"""
    cum = cumsum64(z)
    Z = float(cum[-1])
    if not (Z > 0.0 and math.isfinite(Z)):
        return None
    thr = u3 * Z
    pos = z > 0.0
    hit = np.flatnonzero(pos & (cum[:len(z)] > thr))
    return int(hit[0]) if len(hit) else int(np.flatnonzero(pos)[-1])


def sweep(K, n, t, h, a, bpar, vt, N, M, seed, s, cust, cls=None, lik=None, maxk=1024):
    """one dish sweep; returns (n, t, T, cust, skipped, stuck).  h None: all 1; lik None: every L is 1.  M: the column
    bound the draws are truncated at (the table's)."""
    K = np.asarray(K)
    n = np.array(n, dtype=np.int64)
    t = np.array(t, dtype=np.int64)
    cust = np.array(cust, dtype=np.int64)
    C = len(cust)
    u = synth.unit(3 * C, tio.sweep_key(seed, s))
    koff = np.concatenate([[0], np.cumsum(K)]).astype(np.int64)
    T = np.zeros(len(K), dtype=np.int64)
    skipped = stuck = 0
    c0 = 0
    for i in range(len(K)):
        Ki, g0 = int(K[i]), int(koff[i])
        ni, ti = n[g0:g0 + Ki], t[g0:g0 + Ki]  # views
        Ci = int(ni.sum())
        Ti = int(ti.sum())
        T[i] = Ti
        cs = range(c0, c0 + Ci)
        c0 += Ci
        if Ci > N or Ki > maxk or (lik is not None and Ki > lik.shape[1]):
            skipped += 1
            continue
        b = float(bpar[i])
        hi = np.ones(Ki) if h is None else np.asarray(h[g0:g0 + Ki], dtype=np.float64)
        A, B = np.zeros(Ki), np.zeros(Ki)
        for k in range(Ki):
            A[k], B[k] = AB(int(ni[k]), int(ti[k]), float(hi[k]), a, M, vt)
        for c in cs:
            k0 = int(cust[c])
            n0, t0, A0, B0, T0 = int(ni[k0]), int(ti[k0]), A[k0], B[k0], Ti
            nn, tt = n0, t0
            if nn >= 2:
                if tt > 1 and float(nn - 1) * float(u[2 * c]) < float(tt - 1):
                    tt, Ti = tt - 1, Ti - 1
                nn -= 1
            else:
                nn, tt, Ti = 0, 0, Ti - 1
            ni[k0], ti[k0] = nn, tt
            A[k0], B[k0] = AB(nn, tt, float(hi[k0]), a, M, vt)
            g = b + float(Ti) * a
            z = A + g * B
            if lik is not None:
                z = lik[int(cls[c]), :Ki] * z
            else:
                z = 1.0 * z
            ks = choose(z, float(u[2 * C + c]))
            if ks is None:
                ni[k0], ti[k0], A[k0], B[k0], Ti = n0, t0, A0, B0, T0
                stuck += 1
                continue
            nn, tt = int(ni[ks]), int(ti[ks])
            if nn == 0:
                nn, tt, Ti = 1, 1, Ti + 1
            else:
                nn += 1
                o = tio.odds(nn, tt, Ti, float(hi[ks]), a, b, vt.V(nn, tt + 1), False)
                p = 1.0 if math.isinf(o) else o / (o + 1.0)
                if float(u[2 * c + 1]) < p:
                    tt, Ti = tt + 1, Ti + 1
            ni[ks], ti[ks] = nn, tt
            A[ks], B[ks] = AB(nn, tt, float(hi[ks]), a, M, vt)
            cust[c] = ks
        T[i] = Ti
    return n.astype(np.uint32), t.astype(np.uint16), T.astype(np.uint32), cust.astype(np.uint32), skipped, stuck


# ---- exact laws: one restaurant, states (z, t) with z the customers' dishes ------------------------------------------

def counts(z, K):
    return tuple(int(x) for x in np.bincount(np.asarray(z, dtype=np.int64), minlength=K))


def states(Nc: int, K: int, M=None):
    out = []
    for z in itertools.product(range(K), repeat=Nc):
        ns = counts(z, K)
        for ts in itertools.product(*[range(1, min(nk, M or nk) + 1) if nk else (0,) for nk in ns]):
            out.append((z, ts))
    return out


def joint(Nc: int, K: int, hs, a: float, b: float, cls=None, lik=None, M=None) -> np.ndarray:
    """pi(z, t) ~ (b|a)_T prod_k S^{n_k}_{t_k} h_k^{t_k} prod_c L[cls_c][z_c] over states(Nc, K, M), normalised"""
    S = {m: tio.stirling(m, a) for m in range(1, Nc + 1)}
    p = []
    for z, ts in states(Nc, K, M):
        ns = counts(z, K)
        v = float(np.prod([b + j * a for j in range(sum(ts))]))
        for nk, tk, hk in zip(ns, ts, hs):
            if nk:
                v *= S[nk][tk] * hk ** tk
        if lik is not None:
            for c, zc in enumerate(z):
                v *= lik[cls[c]][zc]
        p.append(v)
    p = np.array(p)
    return p / p.sum()


def visit_matrix(c: int, Nc: int, K: int, hs, a: float, b: float, cls=None, lik=None, M=None, first_dish=False) -> np.ndarray:
    """the transition matrix over states(Nc, K, M) of one visit to customer c, the uniforms integrated out.
    first_dish: u3 ignored, the customer always takes the first dish of positive weight (a wrong law, for tests)"""
    vt = tio.ExactV(list(range(1, Nc + 1)), a, M)
    Mb = M or Nc
    st = states(Nc, K, M)
    idx = {s: j for j, s in enumerate(st)}
    P = np.zeros((len(st), len(st)))
    for z, ts in st:
        src = idx[(z, ts)]
        ns = counts(z, K)
        k0 = z[c]
        n0, t0 = ns[k0], ts[k0]
        if n0 >= 2:
            pr = (t0 - 1) / (n0 - 1) if t0 > 1 else 0.0
            removed = [(t0 - 1, pr), (t0, 1.0 - pr)]
        else:
            removed = [(0, 1.0)]
        for tr, w in removed:
            if w == 0.0:
                continue
            n1 = list(ns)
            t1 = list(ts)
            n1[k0], t1[k0] = n0 - 1, tr
            T = sum(t1)
            g = b + T * a
            zw = np.zeros(K)
            for k in range(K):
                A, B = AB(n1[k], t1[k], hs[k], a, Mb, vt)
                zw[k] = (1.0 if lik is None else lik[cls[c]][k]) * (A + g * B)
            Z = zw.sum()
            if not Z > 0.0:
                P[src, src] += w
                continue
            if first_dish:
                pk = np.zeros(K)
                pk[np.flatnonzero(zw > 0.0)[0]] = 1.0
            else:
                pk = zw / Z
            for k in range(K):
                if pk[k] == 0.0:
                    continue
                zn = z[:c] + (k,) + z[c + 1:]
                if n1[k] == 0:
                    outs = [(1, 1.0)]
                else:
                    nn, tt = n1[k] + 1, t1[k]
                    o = tio.odds(nn, tt, T, hs[k], a, b, vt.V(nn, tt + 1), False)
                    p = 1.0 if math.isinf(o) else o / (o + 1.0)
                    outs = [(tt + 1, p), (tt, 1.0 - p)]
                for tn, q in outs:
                    if q:
                        t2 = list(t1)
                        t2[k] = tn
                        P[src, idx[(zn, tuple(t2))]] += w * pk[k] * q
    return P


def sweep_matrix(Nc: int, K: int, hs, a: float, b: float, cls=None, lik=None, M=None, first_dish=False) -> np.ndarray:
    """one sweep: customers 0 .. Nc-1 in sequence"""
    P = np.eye(len(states(Nc, K, M)))
    for c in range(Nc):
        P = P @ visit_matrix(c, Nc, K, hs, a, b, cls, lik, M, first_dish)
    return P


def marginal_nt(p: np.ndarray, Nc: int, K: int, M=None):
    """the law of (n-vector, t-vector) under a law p over states(Nc, K, M): (cells, probabilities)"""
    acc = {}
    for (z, ts), v in zip(states(Nc, K, M), p):
        key = (counts(z, K), ts)
        acc[key] = acc.get(key, 0.0) + float(v)
    cells = sorted(acc)
    return cells, np.array([acc[c] for c in cells])
