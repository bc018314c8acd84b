"""The laws of the device samplers in long double, written from the mathematics (test infrastructure only).

tc_oracle / tcw_oracle / pt_oracle replay the kernels' own arithmetic on the device's own slab: a wrong cell, or a wrong
row read shared by kernel and replay, cancels there.  This module restates the LAWS -- k_tcounts' conditional, k_tcwin's
windowed Metropolis-Hastings step, k_partition's sequential size law -- on the truth's cells (hp_oracle.rows), with plain
sequential long-double sums: no tree scans, no chunks, no LDS cap.  What the kernels and this module share is only the
counter-based uniforms (synth.unit, tco.sweep_key; elements g+1, 2g+1 / 2g+2, g 65536 + r + 1).

A draw compares u W with the cumulative weights C(tau).  Device and truth may differ only where u W lies within the
device's rounding of some C(tau): such a draw is UNDECIDED.  The bar eps below is derived from the kernels' roundings; it
reads nothing the device returns.  tests/test_samplers_truth_host.py chooses seeds at which every case has no undecided
draw, so tests/test_gpu_samplers_truth.py can demand equality.

Error model (derivation), u = 2^-53
-----------------------------------
The truth's own error -- cells to 3 n 2^-64 relative (hp_oracle), sums of at most 4100 terms at 2^-64 -- is below 1/500
of every bar here and is not carried.

1. A log weight of k_tcounts (tcounts.hip tc_logw): log w(tau) = S + (tau-1) log h + P(tau), P the prefix sum of
   x_k = log(b + (T_ + k) a), k = 1 .. tau-1.  delta(tau) >= |log w_device - log w_true| has the parts
     * the cell: hp.bar(n, a, S) for 2 <= tau < n, hp.s1bar for tau = 1, 0 for tau = n (S^n_n = 1 is written as 0.0);
     * a log term: T_ + k is an exact integer; the product and the sum round once each (an fma only rounds less) and for
       b >= 0 both operands are positive, so the argument is off by at most 2u relative, which moves the log by 2u; the
       log itself is held to 2 ulp of its value (the HIP math library states 1):  2u + 2u |x_k| a term, summed over k < tau;
     * the scan's association: a term reaches its prefix through 6 adds inside a wave (Hillis-Steele), at most nw adds
       over the waves' sums, one add of the wave prefix, one of the carry, and one carry update for every earlier chunk --
       depth(nt, tmax) = 6 + nt/64 + 2 + ceil(tmax/nt) adds, each rounding a partial sum of magnitude at most
       A(tau) = sum_{k<tau} |x_k|:  u depth A(tau), depth the worst of nt = 64, 128, 256, 512, 1024;
     * (tau-1) log h: log h to 2 ulp, the product rounds once:  3u (tau-1) |log h|;
     * the two additions S + . + .: each rounds a partial sum of at most |S| + (tau-1)|log h| + A(tau).
2. A scaled weight v = exp(log w - max): the device's max differs from the truth's, but it is one number for the whole
   row -- a common factor of C and W that drops out of C(tau) > u W.  The subtraction rounds once (u |log w - max|; where
   that exceeds 750 the weight is below 1e-325 of W and cannot move a comparison) and exp is held to 2 ulp:
       rho(tau) = expm1(delta(tau)) + u min(|log w - max|, 750) + 2u.
3. C(tau): the second scan adds positive numbers, every partial sum at most C(tau):
       |C_device - C_true| <= E(tau) = sum_{tau' <= tau} rho(tau') v(tau') + u depth C(tau)     (non-decreasing in tau).
   The target u W rounds once.  So the device decides as the truth wherever
       |u W - C(tau)| > E(tau) + u E(tmax) + u_53 u W,   which  eps W = 2 E(tmax) + u W  covers for every tau.
   eps depends on (n, a, b, T_, h, tmax) through the truth's weights only.
4. k_tcwin (tcwin.hip): the same weights over the span [slo, shi] (at most 4W+1 values, nc chunks of 64), relative to a
   constant of the span (log w(t), or the span's first prefix) which the scale removes.  delta as in 1 with A and the term
   count taken over the span, the factor of log h at most |tau - t| and depth = 6 + nc + 1.  The proposal is 2-3 on the
   window; the acceptance compares u2 Z(t') with Z(t), both butterfly sums (depth 6 + nc) of positive terms on one scale:
       decided iff |u2 Z(t') - Z(t)| > E_Z(t) + u2 E_Z(t') + u u2 Z(t'),   E_Z = sum rho e + u (6 + nc) Z.
5. k_partition (partition.hip pt_weight): log w(l) = (F(l) + S^{N-l}_M) - S^N_{M+1}, F the prefix sum of
   x_j = log(((j-1 - a) (N-j+1)) / (j-1)).  The subtrahend's cell error is common to every l and drops out.  Parts:
     * the cell S^{N-l}_M: hp.bar / hp.s1bar / 0 as above;
     * a term: the difference, the product and the quotient round once each, 3u on the argument, and the log to 2 ulp:
       3u + 2u |x_j|, summed over j <= l;
     * the scan: depth = 6 + nc + 1 with nc = ceil(L/64), times A_F(l) = sum_{j<=l} |x_j|;
     * F + S rounds at u (|F| + |S|), the subtraction at u |F + S - S^N_{M+1}|.
   rho = expm1(delta) + 2u (no max pass: the scale is the law's own total), then 3 with depth = 6 + nc + 1.

What draws cannot see: a relative weight error far below 1 / (number of draws) moves no draw.  The cases here make about
6300 draws, so cell errors below about 1e-4 relative are invisible to them; that part rests on the table tests (test_gpu_hp*).
"""
from __future__ import annotations

import functools

import numpy as np

import hp_oracle as hp
import pt_oracle as pto
import tc_oracle as tco
from libstb_amd import synth

LD = np.longdouble
U = hp.U
THREADS = (64, 128, 256, 512, 1024)

# One way at a time to break the replay (tests/test_samplers_truth_host.py): None, or one of
#   "tminus", "left", "tmax", "logcarry64", "logcarry256", "ccarry", "row4097", "winclip", "pt_la", "pt_carry65"
MUTANT = None


class mutant:
    """with hs.mutant("left"): ... runs the replay broken that way"""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        global MUTANT
        self.old, MUTANT = MUTANT, self.name

    def __exit__(self, *exc):
        global MUTANT
        MUTANT = self.old


# ---------------------------------------------------------------------------------------------------- the cells

class Cells:
    """log S^n_m of one discount in long double, rows n in `need` (all rows when None); row(n)[m], m = 0 .. min(n, M)"""

    def __init__(self, a: float, N: int, M: int):
        self.a, self.N, self.M, self.rows, self._dense = float(a), N, M, {}, None

    def row(self, n: int):
        return self.rows[n]

    def S(self, n: int, m: int):
        """stb_lookup_S's semantics for 1 <= m <= min(n, M): S^n_n = 0, column 1 the truth's S^n_1"""
        return LD(0) if m == n else self.rows[n][m]

    def S_row(self, n: int, tmax: int):
        """S(n, tau) for tau = 1 .. tmax (tmax <= min(n, M))"""
        out = self.rows[n][1:tmax + 1].copy()
        if tmax == n:
            out[n - 1] = LD(0)
        return out

    def S_col(self, m: int, ns):
        """S(n, m) for the rows ns (every row kept; m <= min(n, M))"""
        if self._dense is None:
            self._dense = np.full((self.N + 1, self.M + 1), np.nan, dtype=LD)
            for n, r in self.rows.items():
                self._dense[n, :len(r)] = r
                if n <= self.M:
                    self._dense[n, n] = LD(0)
        return self._dense[np.asarray(ns), m]


@functools.lru_cache(maxsize=8)
def cells(a_list, N: int, M: int, need=None):
    """{a: Cells} for the discounts of the tuple a_list, from one pass of hp.rows; need: a tuple of the rows to keep"""
    out = {a: Cells(a, N, M) for a in a_list}
    keep = None if need is None else set(need)
    for n, v, e in hp.rows(np.array(a_list, dtype=np.float64), N, M):
        if keep is None or n in keep:
            lg = hp.logs(v, e)
            for d, a in enumerate(a_list):
                out[a].rows[n] = lg[d].copy()
    return out


def cells_for(a: float, n: int, M: int) -> Cells:
    return cells((float(a),), n, min(n, M), (n,))[float(a)]


def cell_bar(a: float, n, m, y):
    """the device's bar on log S^n_m = y as stb_lookup_S reads it (n, m, y broadcast)"""
    n, m, y = np.broadcast_arrays(np.asarray(n), np.asarray(m), np.asarray(y, dtype=np.float64))
    out = np.asarray(hp.bar(n, a, y), dtype=np.float64).copy()
    one = (m == 1) & (n > 1)
    if np.any(one):
        out[one] = hp.s1bar(n[one], a, y[one])
    out[m == n] = 0.0
    return out


# ---------------------------------------------------------------------------------------------------- k_tcounts

def depth_full(tmax: int) -> int:
    return max(6 + nt // 64 + 2 + -(-tmax // nt) for nt in THREADS)


class Row:
    """the log weights of a pair and what their bars need"""

    def __init__(self, n, Tminus, a, b, h, M, c: Cells):
        assert b >= 0.0, "the error model is written for b >= 0"
        if MUTANT == "tminus":
            Tminus += 1
        tmax = min(n, M)
        if MUTANT == "tmax" and tmax > 1:
            tmax -= 1
        if MUTANT == "row4097" and tmax > 4096:
            tmax = 4096
        self.n, self.tmax, self.c = n, tmax, c
        tau = np.arange(1, tmax + 1)
        self.S = c.S_row(n, tmax)
        if MUTANT == "left" and tmax >= 3:
            hi = min(tmax, n - 1)
            self.S[2:hi] = c.S_row(n, tmax)[1:hi - 1]
        self.x = np.zeros(tmax, dtype=LD)  # x[tau-1] = log(b + (T_ + tau - 1) a), tau >= 2
        self.x[1:] = np.log(LD(b) + (LD(Tminus) + tau[1:].astype(LD) - LD(1)) * LD(a))
        P = np.cumsum(self.x)
        if MUTANT in ("logcarry64", "logcarry256"):
            ch = 64 if MUTANT == "logcarry64" else 256
            P = np.concatenate([np.cumsum(self.x[o:o + ch]) for o in range(0, tmax, ch)])
        self.logh = np.log(LD(h))
        self.lw = self.S + (tau - 1).astype(LD) * self.logh + P

    def delta(self, lo: int, hi: int, tref, depth: int):
        """delta(tau) for tau = lo .. hi, the log terms summed from lo (tref None: the factor of log h is tau - 1)"""
        tau = np.arange(lo, hi + 1)
        ax = np.abs(self.x[lo - 1:hi].astype(np.float64))
        ax[0] = 0.0 if lo > 1 else ax[0]  # (the span's first tau takes no term of its own)
        A = np.cumsum(ax) if tref is None else np.full(len(tau), ax.sum())
        k = (tau - lo).astype(np.float64) if tref is None else np.full(len(tau), float(hi - lo))
        hl = np.abs(float(self.logh)) * (np.abs(tau - 1) if tref is None else np.abs(tau - tref))
        S = np.abs(self.S[lo - 1:hi].astype(np.float64))
        return (cell_bar(self.c.a, self.n, tau, S) + 2 * U * k + 2 * U * A + U * depth * A + 3 * U * hl + 2 * U * (S + hl + A))


def log_weights(n, Tminus, a, b, h, M, c: Cells = None):
    """log w(tau), tau = 1 .. min(n, M), in long double: S_S(n, tau) + (tau-1) log h + sum_{s=T_+1}^{T_+tau-1} log(b + s a)"""
    return Row(n, Tminus, a, b, h, M, c or cells_for(a, n, M)).lw


def _cum(lw, rho_delta, depth):
    """(C, E): the cumulative scaled weights and the bar of C's device value (sections 2-3)"""
    d = (lw - lw.max()).astype(np.float64)
    v = np.exp(lw - lw.max())
    C = np.cumsum(v)
    if MUTANT == "ccarry":
        C = np.concatenate([np.cumsum(v[o:o + 256]) for o in range(0, len(v), 256)])
    rho = np.expm1(rho_delta) + U * np.minimum(np.abs(d), 750.0) + 2 * U
    E = np.cumsum(rho * v.astype(np.float64)) + U * depth * C.astype(np.float64)
    return C, E


def _first(C, u):
    """(tau - 1, u W): the first index with C > u W (the last one when rounding leaves none)"""
    target = LD(u) * C[-1]
    hit = np.flatnonzero(C > target)
    return (int(hit[0]) if hit.size else len(C) - 1), target


def _draw(row: Row, u: float):
    """(tau, margin, eps): margin = min |u W - C| / (eps W); the draw is decided iff margin > 1"""
    C, E = _cum(row.lw, row.delta(1, row.tmax, None, depth_full(row.tmax)), depth_full(row.tmax))
    k, target = _first(C, u)
    W = float(C[-1])
    if not W > 0.0:  # (only a broken replay gets here)
        return k + 1, 0.0, np.inf
    eps = 2.0 * float(E[-1]) / W + U
    margin = float(np.min(np.abs(target - C))) / (eps * W)
    return k + 1, margin, eps


def draw(lw, u, eps=0.0):
    """(tau, decided): the smallest tau with C(tau) > u W; decided iff |u W - C(tau')| > eps W for every tau'"""
    lw = np.asarray(lw, dtype=LD)
    C = np.cumsum(np.exp(lw - lw.max()))
    k, target = _first(C, u)
    return k + 1, bool(np.min(np.abs(target - C)) > eps * C[-1])


class Stats:
    """what a chain of draws saw: draws, undecided ones, the smallest margin, the largest eps"""

    def __init__(self):
        self.draws, self.undecided, self.margin, self.eps = 0, 0, np.inf, 0.0

    def add(self, margin, eps):
        self.draws += 1
        self.undecided += not margin > 1.0
        self.margin = min(self.margin, margin)
        self.eps = max(self.eps, eps)


def sweep(K, n, t, h, a, bpar, M, c: Cells, seed, s, stats: Stats = None, N=None):
    """one sweep of k_tcounts' law: (t, T, undecided draws).  h None: all 1; pairs with n > N keep t."""
    st = stats or Stats()
    t = np.array(t, dtype=np.uint16)
    u = synth.unit(len(n), tco.sweep_key(seed, s))  # element g + 1
    koff = np.concatenate([[0], np.cumsum(K)]).astype(np.int64)
    T = np.zeros(len(K), dtype=np.uint32)
    und0 = st.undecided
    for i in range(len(K)):
        Ti = int(t[koff[i]:koff[i + 1]].astype(np.int64).sum())
        for g in range(koff[i], koff[i + 1]):
            ng, tg = int(n[g]), int(t[g])
            if ng == 0 or (N is not None and ng > N):
                continue
            new = 1
            if min(ng, M) >= 2:
                row = Row(ng, Ti - tg, a, float(bpar[i]), 1.0 if h is None else float(h[g]), M, c)
                new, margin, eps = _draw(row, float(u[g]))
                st.add(margin, eps)
            Ti += new - tg
            t[g] = new
        T[i] = Ti
    return t, T, st.undecided - und0


# ---------------------------------------------------------------------------------------------------- k_tcwin

def window(x: int, W: int, Mt: int):
    hi = min(Mt, x + W)
    if MUTANT == "winclip":
        hi = min(Mt - 1, x + W)
    return max(1, x - W), hi


def _window_step(row: Row, t: int, W: int, u1: float, u2: float, ref: bool):
    """(t', margin of the proposal, margin of the acceptance or inf, eps of the proposal)"""
    Mt, lw = row.tmax, row.lw
    lo, hi = window(t, W, Mt)
    slo, shi = max(1, t - 2 * W), min(Mt, t + 2 * W)
    nc = (shi - slo + 64) // 64
    dl = row.delta(slo, shi, t, 6 + nc + 1)
    C, E = _cum(lw[lo - 1:hi], dl[lo - slo:hi - slo + 1], 6 + nc + 1)
    k, target = _first(C, u1)
    Z = float(C[-1])
    eps = 2.0 * float(E[-1]) / Z + U
    m1 = float(np.min(np.abs(target - C))) / (eps * Z)
    tp = lo + k
    if ref or tp == t:
        return tp, m1, np.inf, eps
    lp, hp_ = window(tp, W, Mt)
    lo2, hi2 = min(lo, lp), max(hi, hp_)
    m2 = lw[lo2 - 1:hi2].max()

    def Zof(l, h_):
        d = (lw[l - 1:h_] - m2).astype(np.float64)
        e = np.exp(lw[l - 1:h_] - m2)
        rho = np.expm1(dl[l - slo:h_ - slo + 1]) + U * np.minimum(np.abs(d), 750.0) + 2 * U
        z = e.sum()
        return z, float(np.sum(rho * e.astype(np.float64))) + U * (6 + nc) * float(z)

    Zt, Et = Zof(lo, hi)
    Zp, Ep = Zof(lp, hp_)
    lhs = LD(u2) * Zp
    bar2 = Et + u2 * Ep + U * float(lhs)
    return (tp if lhs < Zt else t), m1, float(abs(lhs - Zt)) / bar2, eps


def window_step(lw, t, W, u1, u2, ref, eps=0.0):
    """one visit given log w(tau), tau = 1 .. Mt: (t', decided) with one relative bar eps on both comparisons"""
    lw = np.asarray(lw, dtype=LD)
    Mt = len(lw)
    lo, hi = window(t, W, Mt)
    C = np.cumsum(np.exp(lw[lo - 1:hi] - lw[lo - 1:hi].max()))
    k, target = _first(C, u1)
    ok = bool(np.min(np.abs(target - C)) > eps * C[-1])
    tp = lo + k
    if ref or tp == t:
        return tp, ok
    lp, hp_ = window(tp, W, Mt)
    m2 = lw[min(lo, lp) - 1:max(hi, hp_)].max()
    Zt, Zp = np.exp(lw[lo - 1:hi] - m2).sum(), np.exp(lw[lp - 1:hp_] - m2).sum()
    lhs = LD(u2) * Zp
    return (tp if lhs < Zt else t), ok and bool(abs(lhs - Zt) > eps * max(Zt, lhs))


def window_sweep(K, n, t, h, a, bpar, M, c: Cells, W, seed, s, ref=False, stats: Stats = None, N=None):
    """one windowed sweep of k_tcwin's law: (t, T, undecided draws)"""
    st = stats or Stats()
    t = np.array(t, dtype=np.uint16)
    uu = synth.unit(2 * len(n), tco.sweep_key(seed, s))  # elements 2g + 1, 2g + 2
    koff = np.concatenate([[0], np.cumsum(K)]).astype(np.int64)
    T = np.zeros(len(K), dtype=np.uint32)
    und0 = st.undecided
    for i in range(len(K)):
        Ti = int(t[koff[i]:koff[i + 1]].astype(np.int64).sum())
        for g in range(koff[i], koff[i + 1]):
            ng, tg = int(n[g]), int(t[g])
            if ng == 0 or (N is not None and ng > N):
                continue
            new = 1
            if min(ng, M) >= 2:
                row = Row(ng, Ti - tg, a, float(bpar[i]), 1.0 if h is None else float(h[g]), M, c)
                new, m1, m2, eps = _window_step(row, tg, W, float(uu[2 * g]), float(uu[2 * g + 1]), ref)
                st.add(min(m1, m2), eps)
            Ti += new - tg
            t[g] = new
        T[i] = Ti
    return t, T, st.undecided - und0


# ---------------------------------------------------------------------------------------------------- k_partition

def round_log_weights(Nr: int, Mc: int, a: float, c: Cells):
    """(log w(l), l = 1 .. L = Nr - Mc; delta(l); depth): w(l) = C(Nr-1, l-1) (1-a)_{l-1} S^{Nr-l}_Mc / S^Nr_{Mc+1}"""
    L = Nr - Mc
    l = np.arange(1, L + 1)
    x = np.zeros(L, dtype=LD)
    lm = l[1:].astype(LD)
    first = lm - LD(a) if MUTANT == "pt_la" else lm - LD(1) - LD(a)
    x[1:] = np.log((first * (LD(Nr) - lm + LD(1))) / (lm - LD(1)))
    F = np.cumsum(x)
    if MUTANT == "pt_carry65" and L > 64:
        F[64:] = np.cumsum(x[64:])
    Sv = c.S_col(Mc, Nr - l)
    ptot = c.S(Nr, Mc + 1)
    lw = (F + Sv) - ptot
    depth = 6 + (L + 63) // 64 + 1
    ax = np.abs(x.astype(np.float64))
    bars = cell_bar(c.a, Nr - l, Mc, Sv.astype(np.float64))
    FS = np.abs(F.astype(np.float64)) + np.abs(Sv.astype(np.float64))
    delta = (bars + 3 * U * (l - 1) + 2 * U * np.cumsum(ax) + U * depth * np.cumsum(ax) + U * FS
             + U * np.abs(lw.astype(np.float64)))
    return lw, delta, depth


def _partition_round(Nr, Mc, a, u, c: Cells):
    lw, delta, depth = round_log_weights(Nr, Mc, a, c)
    w = np.exp(lw)
    C = np.cumsum(w)
    rho = np.expm1(delta) + 2 * U
    E = np.cumsum(rho * w.astype(np.float64)) + U * depth * C.astype(np.float64)
    k, target = _first(C, u)
    W = float(C[-1])
    eps = 2.0 * float(E[-1]) / W + U
    return k + 1, float(np.min(np.abs(target - C))) / (eps * W), eps


def partition_round(Nr, Mc, a, u, M, c: Cells = None):
    """(l, decided) of one round: Nr customers unplaced, Mc >= 1 tables to open after this one (Mc + 1 <= M)"""
    assert Mc + 1 <= M
    if Nr - Mc == 1:
        return 1, True
    l, margin, _ = _partition_round(Nr, Mc, a, u, c or cells((float(a),), Nr, Mc + 1, None)[float(a)])
    return l, margin > 1.0


def partition(n, t, a, N, M, S, c: Cells, seed, sweep_, stats: Stats = None):
    """the whole call of k_partition's law: (cnt[S], sizes per pair in draw order (None: nothing written), undecided)"""
    st = stats or Stats()
    key = tco.sweep_key(seed, sweep_)
    cnt = np.zeros(S, dtype=np.int64)
    sizes, und0 = [], st.undecided
    for g in range(len(n)):
        ng, tg = int(n[g]), int(t[g])
        if ng == 0:
            sizes.append([] if tg == 0 else None)
            continue
        if tg == ng:
            sizes.append([1] * ng)
            continue
        if tg == 0 or tg > ng or ng >= S or (tg > 1 and (ng > N or tg > M)):
            cnt[0] += 1
            sizes.append(None)
            continue
        Nr, sz = ng, []
        for r in range(tg - 1):
            Mc = tg - 1 - r
            l = 1
            if Nr - Mc > 1:
                l, margin, eps = _partition_round(Nr, Mc, a, pto.unit_at(key, g * 65536 + r + 1), c)
                st.add(margin, eps)
            sz.append(l)
            Nr -= l
        sz.append(Nr)
        for x in sz:
            cnt[x] += 1
        sizes.append(sz)
    return cnt, sizes, st.undecided - und0
