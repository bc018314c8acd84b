"""Replay, exact propagation, high-precision truth and error bars of annealed importance sampling for unseen documents
(libstb_amd/csrc/seat_ais.hip; include/stb_hip.h "annealed importance sampling"; test infrastructure only).

    restaurants start empty; 0 = beta_0 < beta_1 < .. < beta_S = 1; f_s = prior x prod_c L[cls_c][z_c]^beta_s
    x_0 ~ prior (weighted by the seating's own W under a truncation);  for s = 1 .. S:  lw += (beta_s - beta_{s-1}) D(x_{s-1}),
    then, s < S, x_s = `passes` dish sweeps of x_{s-1} under L^beta_s;  E[exp lw] = Z_S = p(w | L, h, a, b)

Replay -- a composition, written from the header's text
-------------------------------------------------------
  expand() makes the replicated problem in numpy: replica j = i R + r, pairs from koff[i] R + r K_i, customers from
  coff[i] R + r N_i, the restaurant's classes, h and b, n = t = 0.  st_oracle.replay seats it from the prior (one committed
  particle, no matrix, sweep number `sweep`) and its lw is where lw starts.  Per temperature: D in the header's association
  (customer q of a replica in lane q mod 64, a lane adds in increasing q by pr_oracle.dd_add, lanes 0 .. min(64, N) - 1 are
  merged in lane order: the lane's hi by dd_add, its lo added to lo; D = hi + lo), lw = lw + dbeta * D, and td_oracle.sweep
  once a pass under the tempered matrix of that temperature -- an ARGUMENT (the device's are fetched through
  stb_lik_temper; on the CPU numpy's exp(beta * log(lik)) serves), sweeps numbered sweep + 1 + (s - 1) passes + p.
  td_oracle.sweep takes a restaurant's customers from its n; a replica of a restaurant that is left out holds no seating, so
  the sweep is given a stand-in for it of stride + 1 pairs with its N_i customers at pair 0: skipped there (K > stride), and
  the flat customer indices of everybody else stay what they are.  numpy's log is not the device's: the states are
  compared bit for bit, lw, H_i and the total within the bars.

Truth: along the replay's path.  lw0 by st_oracle.truth (a quotient of exact integers); D = sum_c log L_c by mpmath at 40
digits on the exact doubles; lw = lw0 + sum_s dbeta_s D_s with dbeta_s the doubles the host formed.

The bars (u = 2^-53; a correctly rounded operation errs by u relative, a library function by its ulp, 2 u), from the
operations alone -- nothing here reads a device result
---------------------------------------------------------------------------------------------------------------------
  a tempered cell v = exp(beta * log(L)): x = log(L) errs by 2 u |x|; y = beta * x carries beta times that and rounds,
      2 u |y| + u |y|; exp turns an absolute error e of its argument into a relative one and has its own ulp:
      bar(v) = v (3 u |y| + 2 u) + 2^-1074 (the last term: a subnormal result is rounded to a multiple of 2^-1074)
  D: every log errs by 2 u |x_c|; the double-double additions lose u^2 a term (inside the slack); hi + lo rounds once:
      bar(D) = 2 u sum_c |x_c| + u |D|
  lw: the start, st_oracle's bar of the seating's lw; each of the S steps multiplies (u |dbeta D| and dbeta bar(D)) and
      adds (u |lw| of the result):  bar(lw) = bar(lw0) + sum_s (dbeta_s bar(D_s) + u |dbeta_s D_s| + u |lw_s|)
  H_i and the total: st_oracle.loglik_truth's, from bar(lw).
  Everything times 1 + 2^-20 for the second order.
"""
from __future__ import annotations

import math
import os
import sys
from functools import lru_cache

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hp_oracle as hp  # noqa: E402
import pr_oracle as pro  # noqa: E402
import st_oracle as sto  # noqa: E402
import td_oracle as tdo  # noqa: E402
import ti_oracle as tio  # noqa: E402

U = hp.U
SLACK = pro.SLACK
MAXK = pro.MAXK
NEG_INF = -math.inf
MAXPART = 4096
MUTS = ("beta_s", "samesweep", "layout", "after")


# ---------------------------------------------------------------------------------------------------- the ladder

def ladder(S: int, betas=None):
    """the S temperatures as the launcher forms them: the caller's, or (double)s / (double)S with beta_S = 1.0"""
    if betas is not None:
        return [float(b) for b in betas]
    return [1.0 if s == S else float(s) / float(S) for s in range(1, S + 1)]


def refusal(S: int, betas, passes: int, particles: int, a: float = 0.5, M: int = 1, N: int = 3, I: int = 1,
            lik: bool = True, cls: bool = True):
    """the reason stb_seat_anneal refuses these arguments before anything is queued, or None: the header's list"""
    if not (0.0 <= a < 1.0):
        return "a"
    if I < 0:
        return "I"
    if M > 65535:
        return "M"
    if particles < 1 or particles > MAXPART:
        return "particles"
    if N < 1 or M < 1:
        return "bounds"
    if S < 1:
        return "S"
    if passes < 1:
        return "passes"
    prev = 0.0
    for b in ladder(S, betas):
        if not (b > prev) or not (b <= 1.0):
            return "betas"
        prev = b
    if prev != 1.0:
        return "betas"
    if I * particles > 2 ** 31 - 1:
        return "replicas"
    if not lik or not cls:
        return "matrix"
    return None


# ---------------------------------------------------------------------------------------------------- the expansion

def expand(K, coff, cls, h, bpar, R: int, N: int, stride: int, cap: int = MAXK, G=None, C=None, mut=None):
    """the replicated problem of k_ais_expand: a dict K2, N2 [I R], koff2, coff2 [I R] (every replica's first pair and
    first customer, by the header's formulas), cls2 [C R], h2 [G R] or None, bpar2 [I R], skip [I], rest [I R].  G, C: what
    the caller states for koff[I] and coff[I]; a disagreement leaves everybody out, without pairs or customers.
    mut 'layout': the wrong layout koff[i] + r K_i"""
    K = np.asarray(K, dtype=np.int64)
    I = K.shape[0]
    coff = np.asarray(coff, dtype=np.int64)
    koff = np.concatenate([[0], np.cumsum(K)]).astype(np.int64)
    Nc = np.diff(coff)
    rest = np.repeat(np.arange(I), R)
    r = np.tile(np.arange(R), I)
    bpar = np.broadcast_to(np.asarray(bpar, dtype=np.float64), (I,))
    if (G is not None and G != koff[-1]) or (C is not None and C != coff[-1]):
        z = np.zeros(I * R, dtype=np.int64)
        return {"K2": z, "N2": z, "koff2": z, "coff2": z, "cls2": np.zeros(0, dtype=np.int64), "h2": None,
                "bpar2": np.ones(I * R), "skip": np.ones(I, dtype=bool), "rest": rest, "G2": 0, "C2": 0}
    skip = (K > cap) | (K > stride) | ((K == 0) & (Nc > 0)) | (Nc > N)
    K2, N2 = K[rest], Nc[rest]
    koff2 = koff[rest] * R + r * K2
    if mut == "layout":
        koff2 = koff[rest] + r * K2
    coff2 = coff[rest] * R + r * N2
    G2, C2 = int(koff[-1]) * R, int(coff[-1]) * R
    cls2 = np.zeros(C2, dtype=np.int64)
    h2 = None if h is None else np.zeros(G2)
    cls = np.asarray(cls, dtype=np.int64)
    for j in range(I * R):
        i = int(rest[j])
        cls2[coff2[j]:coff2[j] + N2[j]] = cls[coff[i]:coff[i + 1]]
        if h is not None:
            h2[koff2[j]:koff2[j] + K2[j]] = np.asarray(h, dtype=np.float64)[koff[i]:koff[i + 1]]
    return {"K2": K2, "N2": N2, "koff2": koff2, "coff2": coff2, "cls2": cls2, "h2": h2, "bpar2": bpar[rest].copy(), "skip": skip,
            "rest": rest, "G2": G2, "C2": C2}


# ---------------------------------------------------------------------------------------------------- D

def D_of(cust, cls2, coff2, N2, lik, active):
    """(D [replicas], sum_c |log L_c| [replicas]) of the replicas marked active, in the header's association"""
    lik = np.asarray(lik, dtype=np.float64)
    rows, stride = lik.shape
    J = len(N2)
    D, sab = np.zeros(J), np.zeros(J)
    for Nc in np.unique(N2[active]):
        Nc = int(Nc)
        if Nc == 0:
            continue
        js = np.flatnonzero(active & (N2 == Nc))
        idx = coff2[js][:, None] + np.arange(Nc)[None, :]
        cl, k = np.asarray(cls2, dtype=np.int64)[idx], np.asarray(cust, dtype=np.int64)[idx]
        ok = (cl < rows) & (k < stride)
        L = np.where(ok, lik[np.minimum(cl, rows - 1), np.minimum(k, stride - 1)], 0.0)
        pos = L > 0.0
        x = np.where(pos, np.log(np.where(pos, L, 1.0)), NEG_INF)
        m = len(js)
        hi, lo = np.zeros((m, 64)), np.zeros((m, 64))
        for q in range(Nc):
            l = q % 64
            hi[:, l], lo[:, l] = pro.dd_add(hi[:, l], lo[:, l], x[:, q])
        th, tl = np.zeros(m), np.zeros(m)
        for l in range(min(64, Nc)):
            th, tl = pro.dd_add(th, tl, hi[:, l])
            tl = tl + lo[:, l]
        D[js] = th + tl
        sab[js] = np.where(pos, np.abs(x), 0.0).sum(axis=1)
    return D, sab


# ---------------------------------------------------------------------------------------------------- the replay

def _sweep_view(ex, n, t, cust, stride):
    """what td_oracle.sweep is given: every replica that is left out (or has no pairs) replaced by a stand-in of
    stride + 1 pairs holding its customers at pair 0 -- skipped there, its customers counted"""
    K2, N2, skip, rest = ex["K2"], ex["N2"], ex["skip"], ex["rest"]
    J = len(K2)
    dummy = skip[rest] | (K2 == 0)
    Kv = np.where(dummy, stride + 1, K2)
    koffv = np.concatenate([[0], np.cumsum(Kv)]).astype(np.int64)
    nv = np.zeros(int(koffv[-1]), dtype=np.int64)
    tv = np.zeros(int(koffv[-1]), dtype=np.int64)
    hv = None if ex["h2"] is None else np.ones(int(koffv[-1]))
    custv = np.array(cust, dtype=np.int64)
    for j in range(J):
        a0 = int(koffv[j])
        if dummy[j]:
            nv[a0] = N2[j]
            tv[a0] = 1 if N2[j] else 0
            custv[ex["coff2"][j]:ex["coff2"][j] + N2[j]] = 0
        else:
            g0 = int(ex["koff2"][j])
            nv[a0:a0 + K2[j]] = n[g0:g0 + K2[j]]
            tv[a0:a0 + K2[j]] = t[g0:g0 + K2[j]]
            if hv is not None:
                hv[a0:a0 + K2[j]] = ex["h2"][g0:g0 + K2[j]]
    return Kv, koffv, nv, tv, hv, custv, dummy


def replay(K, h, a, bpar, coff, cls, lik, tempered, vt, N: int, M: int, seed: int, sweep: int, particles: int, S: int,
           betas=None, passes: int = 1, G=None, C=None, mut=None, bars: bool = False):
    """stb_seat_anneal.  tempered: the S - 1 matrices of temperatures 1 .. S - 1.  vt: the V table's cells (ti_oracle.VTab
    or ExactV) at the bounds (N, M).  Returns a dict: lw (I, R), pn, pt [G R], pT [I R], pcust [C R] (the final states in
    the replicated layout; zeros where a restaurant is left out), skipped, dead, stuck, and with bars: steps, a list of
    (dbeta, D, sum |log L|, lw after the step, the customers' dishes the step read) per temperature, seat (the prior seating's replay with bars) and ex (the expansion).
    mut, the wrong replays: 'beta_s' takes beta_s for dbeta_s, 'samesweep' numbers every temperature's sweeps from
    sweep + 1, 'layout' places replica r's pairs at koff[i] + r K_i, 'after' takes the increment after the sweep."""
    K = np.asarray(K, dtype=np.int64)
    I, R = K.shape[0], int(particles)
    lik = np.asarray(lik, dtype=np.float64)
    rows, stride = lik.shape
    be = ladder(S, betas)
    ex = expand(K, coff, cls, h, bpar, R, N, stride, G=G, C=C, mut=mut)
    K2, N2, rest, skip = ex["K2"], ex["N2"], ex["rest"], ex["skip"]
    J = I * R
    active = ~skip[rest]
    out = {"skipped": int(skip.sum()), "dead": 0, "stuck": 0}
    coffx = np.concatenate([ex["coff2"], [ex["C2"]]]).astype(np.int64)
    # ---- x_0 ~ prior
    right = expand(K, coff, cls, h, bpar, R, N, stride, G=G, C=C) if mut == "layout" else ex
    seat = sto.replay(K2, np.zeros(right["G2"], dtype=np.int64), np.zeros(right["G2"], dtype=np.int64), right["h2"], a, ex["bpar2"],
                      coffx, M=M, seed=seed, sweep=sweep, particles=1, bars=bars)
    n, t, T, cust = (seat[k].astype(np.int64) for k in ("n", "t", "T", "cust"))
    lw = np.where(active, seat["lw"][:, 0], 0.0)
    out["stuck"] += seat["stuck"]
    steps = []
    zrows = int(np.max(ex["cls2"])) + 1 if len(ex["cls2"]) else rows

    def sweeps_of(s):
        nonlocal n, t, T, cust
        Lt = np.asarray(tempered[s - 1], dtype=np.float64)
        if zrows > rows:                    # (a class outside the matrix reads zeros, as the kernel has it)
            Lt = np.concatenate([Lt, np.zeros((zrows - rows, stride))])
        for p in range(passes):
            num = sweep + 1 + (0 if mut == "samesweep" else (s - 1) * passes) + p
            Kv, koffv, nv, tv, hv, custv, dummy = _sweep_view(right, n, t, cust, stride)
            nv, tv, Tv, custv, _, stuck = tdo.sweep(Kv, nv, tv, hv, a, ex["bpar2"], vt, N, M, seed, num, custv, ex["cls2"], Lt)
            out["stuck"] += stuck
            for j in np.flatnonzero(~dummy):
                g0, a0 = int(right["koff2"][j]), int(koffv[j])
                n[g0:g0 + K2[j]] = nv[a0:a0 + K2[j]]
                t[g0:g0 + K2[j]] = tv[a0:a0 + K2[j]]
                T[j] = Tv[j]
                c0 = int(ex["coff2"][j])
                cust[c0:c0 + N2[j]] = custv[c0:c0 + N2[j]]

    prev = 0.0
    for s in range(1, S + 1):
        dbeta = be[s - 1] if mut == "beta_s" else be[s - 1] - prev
        prev = be[s - 1]
        if mut == "after" and s < S:
            sweeps_of(s)
        D, sab = D_of(cust, ex["cls2"], ex["coff2"], N2, lik, active)
        with np.errstate(invalid="ignore"):
            lw = np.where(active, lw + dbeta * D, 0.0)
        steps.append((dbeta, D, sab, lw.copy(), cust.copy() if bars else None))
        if mut != "after" and s < S:
            sweeps_of(s)
    out["dead"] = int((active & (lw == NEG_INF)).sum())
    # ---- the outputs in the layout of ex (the wrong layout scatters the replicas where it believes them to be)
    pn, pt = np.zeros(max(right["G2"], 1), dtype=np.int64)[:right["G2"]], np.zeros(max(right["G2"], 1), dtype=np.int64)[:right["G2"]]
    for j in np.flatnonzero(active):
        g0, gr = int(ex["koff2"][j]), int(right["koff2"][j])
        pn[g0:g0 + K2[j]] = n[gr:gr + K2[j]]
        pt[g0:g0 + K2[j]] = t[gr:gr + K2[j]]
    keep = np.zeros(ex["C2"], dtype=bool)
    for j in np.flatnonzero(active):
        keep[ex["coff2"][j]:ex["coff2"][j] + N2[j]] = True
    out.update({"lw": lw.reshape(I, R), "pn": pn.astype(np.uint32), "pt": pt.astype(np.uint16),
                "pT": np.where(active, T, 0).astype(np.uint32), "pcust": np.where(keep, cust, 0).astype(np.uint32),
                "active": active, "keep": keep})
    if bars:
        out.update({"steps": steps, "seat": seat, "ex": ex})
    return out


# ---------------------------------------------------------------------------------------------------- truth and bars

def temper_truth(lik, beta: float):
    """(exp(beta log L) cell by cell by mpmath on the exact doubles, rounded to double; the docstring's bar)"""
    mp = hp._mp()
    lik = np.asarray(lik, dtype=np.float64)
    want, bar = np.zeros(lik.shape), np.zeros(lik.shape)
    for e, L in np.ndenumerate(lik):
        if L == 0.0:
            continue
        y = mp.mpf(float(beta)) * mp.log(mp.mpf(float(L)))
        v = mp.exp(y)
        want[e] = float(v)
        bar[e] = (float(v) * (3.0 * U * abs(float(y)) + 2.0 * U)) * SLACK + 2.0 ** -1074
    return want, bar


def truth(K, h, a, bpar, coff, cls, lik, M: int, rep, particles: int):
    """along the path of rep (a replay with bars=True): a dict lw (I, R), lw_bar (I, R), W {i: R mpf} -- st_oracle.truth's
    shape, so st_oracle.loglik_truth finishes it.  A restaurant left out has lw = 0, W = 1, bar 0"""
    mp = hp._mp()
    K = np.asarray(K, dtype=np.int64)
    I, R = K.shape[0], int(particles)
    ex, seat = rep["ex"], rep["seat"]
    J = I * R
    active = rep["active"]
    coffx = np.concatenate([ex["coff2"], [ex["C2"]]]).astype(np.int64)
    z = np.zeros(ex["G2"], dtype=np.int64)
    st = sto.truth(ex["K2"], z, z, ex["h2"], a, ex["bpar2"], coffx, None, None, M, seat,
                   restaurants=[int(j) for j in np.flatnonzero(active)])
    lik = np.asarray(lik, dtype=np.float64)
    rows, stride = lik.shape
    logL = {}

    def exact_D(j, cust_s):
        c0, Nj = int(ex["coff2"][j]), int(ex["N2"][j])
        tot = mp.mpf(0)
        cells, cnt = np.unique(np.stack([ex["cls2"][c0:c0 + Nj], cust_s[c0:c0 + Nj]], axis=1), axis=0, return_counts=True)
        for (cl, k), m in zip(cells, cnt):
            key = (int(cl), int(k))
            if key not in logL:
                L = float(lik[key]) if key[0] < rows and key[1] < stride else 0.0
                logL[key] = mp.log(mp.mpf(L)) if L > 0.0 else None
            if logL[key] is None:
                return None
            tot += int(m) * logL[key]
        return tot

    lw, bar, W = np.zeros(J), np.zeros(J), [mp.mpf(1)] * J
    for j in np.flatnonzero(active):
        j = int(j)
        W0 = st["W"][j][0] if int(ex["N2"][j]) else mp.mpf(1)
        dead = W0 == 0
        acc = mp.mpf(0) if dead else mp.log(W0)
        b = float(st["lw_bar"][j, 0])
        for dbeta, D, sab, lws, cust_s in rep["steps"]:
            De = None if dead else exact_D(j, cust_s)
            if De is None:
                dead = True
                continue
            acc += mp.mpf(float(dbeta)) * De
            b += dbeta * (2.0 * U * sab[j] + U * abs(D[j])) + U * abs(dbeta * D[j]) + U * abs(lws[j])
        lw[j] = NEG_INF if dead else float(acc)
        bar[j] = 0.0 if dead else b * SLACK
        W[j] = mp.mpf(0) if dead else mp.exp(acc)
    return {"lw": lw.reshape(I, R), "lw_bar": bar.reshape(I, R), "W": {i: W[i * R:(i + 1) * R] for i in range(I)}}


def finish(K, tr, particles: int):
    """(H_i, their bars, the total, its bar) of truth()'s result: st_oracle.loglik_truth over every restaurant"""
    return sto.loglik_truth(tr, range(len(K)), int(particles))


# ---------------------------------------------------------------------------------------------------- exact propagation

ORDERS = ("right", "after", "prev")


def exact(Nc: int, K: int, hs, a: float, b: float, cls, lik, betas, passes: int = 1, M=None, order: str = "right") -> float:
    """E[exp lw] with every uniform integrated out: v <- (v . exp(dbeta D)) P_s over td_oracle.states(Nc, K, M), v_0 the
    prior measure st_oracle.ujoint_states (what the seating's weighted draw represents), P_s = `passes` exact sweep matrices
    under lik^beta_s.  order, the wrong ladders: 'after' takes the increment after the sweep, 'prev' sweeps under the
    previous temperature"""
    lik = np.asarray(lik, dtype=np.float64)
    st = tdo.states(Nc, K, M)
    v = sto.ujoint_states(Nc, K, hs, a, b, M=M)
    with np.errstate(divide="ignore"):
        D = np.array([sum(math.log(lik[cls[c]][z[c]]) if lik[cls[c]][z[c]] > 0.0 else NEG_INF for c in range(Nc)) for z, _ in st])
    prev, S = 0.0, len(betas)
    for s, be in enumerate(betas, 1):
        inc = np.exp((be - prev) * D)
        if s < S:
            Lt = lik ** (prev if order == "prev" else be)
            P = np.linalg.matrix_power(tdo.sweep_matrix(Nc, K, hs, a, b, cls, Lt, M), passes)
            v = (v @ P) * inc if order == "after" else (v * inc) @ P
        else:
            v = v * inc
        prev = be
    return float(v.sum())


# ---------------------------------------------------------------------------------------------------- the cases

SEED, SWEEP = 0xA15, 7

LAW_NC, LAW_K, LAW_A, LAW_B = 3, 2, 0.5, 1.0
LAW_H = (0.6, 0.4)
LAW_CLS = (0, 1, 0)
LAW_LIK = ((0.9, 0.2), (0.1, 0.8))
LAW_BETAS = (0.25, 0.5, 0.75, 1.0)
LAW_I, LAW_SEED, LAW_SWEEP = 20000, 5, 0


def numpy_tempered(lik, S: int, betas=None):
    """the S - 1 tempered matrices by numpy's own log and exp: what a CPU replay is given (the device's are fetched)"""
    lik = np.asarray(lik, dtype=np.float64)
    out = []
    for be in ladder(S, betas)[:-1]:
        with np.errstate(divide="ignore"):
            out.append(np.where(lik == 0.0, 0.0, np.exp(np.float64(be) * np.log(np.where(lik == 0.0, 1.0, lik)))))
    return out


@lru_cache(maxsize=None)
def law_case():
    """20000 equal empty restaurants of the exact propagation's case: (K, h, bpar, coff, cls, lik)"""
    I = LAW_I
    out = (np.full(I, LAW_K, dtype=np.int32), np.tile(np.array(LAW_H), I), np.full(I, LAW_B),
           (LAW_NC * np.arange(I + 1)).astype(np.uint64), np.tile(np.array(LAW_CLS, dtype=np.uint32), I), np.array(LAW_LIK))
    for x in out:
        x.setflags(write=False)
    return out


def law_statistic(lw, want: float):
    """(mean of exp(lw), 5 sd / sqrt(n) from the sample, |mean - want|)"""
    w = np.exp(np.asarray(lw, dtype=np.float64).reshape(-1))
    tol = 5.0 * float(w.std(ddof=1)) / math.sqrt(len(w))
    return float(w.mean()), tol, abs(float(w.mean()) - want)


HOST_K = (1, 2, 5, 3, 0, 4)
HOST_N = (7, 12, 9, 0, 0, 1)


@lru_cache(maxsize=None)
def host_case(a: float):
    """six small empty restaurants for the CPU (exact Stirling numbers reach N = 12): (K, h, bpar, coff, cls, lik); every
    a > 0 has restaurant 1 at -a < b < 0; one has no customers, one neither dishes nor customers"""
    rng = np.random.default_rng([0xA15, int(a * 1000)])
    K = np.array(HOST_K, dtype=np.int32)
    G = int(K.sum())
    h = 0.05 + rng.random(G)
    bpar = 0.3 + 3.0 * rng.random(len(K))
    if a > 0.0:
        bpar[1] = -0.5 * a
    coff = np.concatenate([[0], np.cumsum(HOST_N)]).astype(np.uint64)
    cls = rng.integers(0, 3, size=int(coff[-1])).astype(np.uint32)
    lik = 0.05 + 2.0 * rng.random((3, 6))
    out = (K, h, bpar, coff, cls, lik)
    for x in out:
        x.setflags(write=False)
    return out


RAW_KS = (1, 2, 63, 64, 65, 130)
RAW_NS = (0, 1, 63, 64, 65, 130)
RAW_ROWS, RAW_STRIDE = 4, 136


@lru_cache(maxsize=None)
def raw_case(a: float, neg_b: bool = False):
    """37 mixed empty restaurants: every K_i of RAW_KS with every N_i of RAW_NS, and one with neither dishes nor customers
    in the middle: (K, h, bpar, coff, cls, lik).  neg_b (a > 0): every third restaurant has -a < b <= 0.  The matrix has no
    zero cell (dead particles have a test of their own) but spans six decades"""
    rng = np.random.default_rng([0xA16, int(a * 1000), int(neg_b)])
    pairs = [(k, n) for k in RAW_KS for n in RAW_NS]
    order = rng.permutation(len(pairs))
    K = [pairs[j][0] for j in order]
    Nn = [pairs[j][1] for j in order]
    K.insert(18, 0)
    Nn.insert(18, 0)
    K = np.array(K, dtype=np.int32)
    G = int(K.sum())
    h = 0.05 + rng.random(G)
    bpar = 0.3 + 4.0 * rng.random(len(K))
    if neg_b:
        bpar[::3] = -a * rng.random(len(bpar[::3])) * 0.9
        bpar[0] = 0.0
    coff = np.concatenate([[0], np.cumsum(Nn)]).astype(np.uint64)
    cls = rng.integers(0, RAW_ROWS, size=int(coff[-1])).astype(np.uint32)
    lik = 10.0 ** rng.uniform(-4.0, 2.0, size=(RAW_ROWS, RAW_STRIDE))
    out = (K, h, bpar, coff, cls, lik)
    for x in out:
        x.setflags(write=False)
    return out
