"""Replay, exact path enumeration, high-precision truth and error bars of the forward seating (libstb_amd/csrc/seat.hip;
include/stb_hip.h "seating customers one by one"; test infrastructure only).

    a customer of class w sits in dish k at an old table with weight L_k (n_k - t_k a), at a new one with L_k (b + T a) h_k,
    both over b + N;  p_c = sum_k theta_k L_k on the state before c;  W = prod_c p_c;  H_i = log((1/R) sum_r W_r)

Replay (numpy float64, one ufunc an operation: no contraction) -- written from the header's text
------------------------------------------------------------------------------------------------
  Items (a restaurant's particle) of the same K_i and customer count are taken together, one customer position a step.
  g = b + T * a; den = b + N; x = n - t * a; y = 0 where n >= 1 and t + 1 > M, else g * h; theta = (x + y) / den, h where
  N = 0; q = theta * L (+0.0 past K_i); cumulative sums by td_oracle.cumsum64's association on a (.., blocks, 64) array;
  Z the last; thr = u3 * Z; k* the first k with q > 0 and cum > thr, else the last with q > 0; impossible: the same on
  q = theta, then k = 0; new = n_k* = 0 or u2 * (x + y) < y.  lw: log(p_c) by pr_oracle.dd_add in seating order (numpy's
  log: the device's is its own, so lw, H_i and the total are compared within the bars, the state and p bit for bit).
  The stream of particle r is ti_oracle.sweep_key(seed, sweep + r); u2 = unit element 2c + 2, u3 = element 2C + 1 + c.

Exact law: enumerate() walks every path of a short sequence with the uniforms integrated out.

Truth: along the replay's path p_c = (sum n L - a sum t L + g sum' h L) / den as a quotient of exact integers (every
double is an integer over a power of two; sum' leaves out the dishes at the truncation); W is the product of the
numerators over the product of the denominators by mpmath at 40 digits, lw = log W, H_i = log(mean_r W_r).

The bars (u = 2^-53), from the operations -- nothing here reads a device result
-------------------------------------------------------------------------------
  theta as pr_oracle: e_x = u (|t a| + |x|); e_g = u (|T a| + |g|); e_y = e_g h + u |g h| (0 where y is the constant 0);
      e_num = e_x + e_y + u |x + y|; bar(theta) = |theta| (e_num / |num| + 2 u) (the sum den and the division); N = 0: 0.
  p: every product rounds once, the scan adds at most six times inside a block and once a block base:
      bar(p) = sum_k bar(theta_k) L_k + u (1 + 6 + blocks) sum_k |q_k|
  x_c = log(p_c): bar(x) = bar(p) / p + 2 u |x| (the log of a relatively perturbed argument plus its own ulp)
  lw: sum_c bar(x_c) + u |lw| (the double-double sum loses u^2 a term: inside the slack; hi + lo rounds once)
  H_i = m + log(s / R), s = sum_r exp(lw_r - m): a log-mean-exp moves by at most the largest move of an argument,
      max_r bar(lw_r); d_r = lw_r - m rounds (u |d_r|), exp has its ulp (2 u), the R - 1 additions of positive terms
      ((R - 1) u), the division (u): rho = max_r u |d_r| + (R + 2) u is the relative error of s / R; the log adds
      rho + 2 u |log(s / R)|, the last sum u |H_i|.
  total: sum_i bar(H_i) + 8 u sum_i |H_i| (the block tree of 256: eight levels) + u (2 |total| + 16), as pr_oracle.
  Everything times 1 + 2^-20 for the second order.

stb_seat_loglik alone (tests/test_gpu_seat_geometry.py): lw_types are exact doubles, so max_r bar(lw_r) = 0 and the H_i bar
is loglik_rows_bar against loglik_rows_truth (x87 long double); given the H_i, the total is loglik_total bit for bit.
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
import td_oracle as tdo  # noqa: E402
import ti_oracle as tio  # noqa: E402

U = hp.U
NEG_INF = -math.inf
MAXK = pro.MAXK
SLACK = pro.SLACK
_GAMMA = np.uint64(0x9E3779B97F4A7C15)


# ---------------------------------------------------------------------------------------------------- the uniforms

def _mix64(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def unit(key, j):
    """element j of the stream of key (uniforms.h's stb_unit), on arrays"""
    with np.errstate(over="ignore"):
        z = _mix64(np.asarray(key, dtype=np.uint64) + np.asarray(j, dtype=np.uint64) * _GAMMA)
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def particle_key(seed: int, sweep: int, r: int) -> int:
    return tio.sweep_key(seed, sweep + r)


# ---------------------------------------------------------------------------------------------------- the replay

def cumsum64(q, linear: bool = False):
    """td_oracle.cumsum64 on the last axis of an (m, 64 nb) array: (cum, Z).  linear: the wrong association, left to right"""
    m, KP = q.shape
    if linear:
        cum = np.cumsum(q, axis=1)
        return cum, cum[:, -1].copy()
    nb = KP // 64
    x = q.reshape(m, nb, 64).copy()
    d = 1
    while d < 64:
        x[:, :, d:] = x[:, :, d:] + x[:, :, :-d]
        d *= 2
    base = np.zeros(m)
    for j in range(nb):
        x[:, j, :] = base[:, None] + x[:, j, :]
        base = x[:, j, 63].copy()
    return x.reshape(m, KP), base


def skipped_mask(K, Cn, stride=None, maxk=MAXK):
    K = np.asarray(K, dtype=np.int64)
    m = K > maxk
    if stride is not None:
        m |= K > stride
    return m | ((K == 0) & (np.asarray(Cn) > 0))


def replay(K, n, t, h, a, bpar, coff, cls=None, lik=None, M: int = 0, seed: int = 0, sweep: int = 0, particles: int = 1,
           rows=None, mut=None, bars: bool = False):
    """stb_seat_customers on one start state.  Returns a dict: n, t (particle 0's final pairs; a skipped restaurant's
    as they were), T [I], cust [C], p [C] (particle 0's), lw (I, particles), skipped, impossible, stuck (visits over all
    particles), and with bars: pbar (C, particles), pall (C, particles), ks, new (C, particles) -- the paths.
    mut: 't+1', 'noTa', 'linear' or 'swap', the wrong replays"""
    K = np.asarray(K, dtype=np.int64)
    I = K.shape[0]
    koff = np.concatenate([[0], np.cumsum(K)]).astype(np.int64)
    coff = np.asarray(coff, dtype=np.int64)
    Cn = np.diff(coff)
    C = int(coff[-1])
    bpar = np.broadcast_to(np.asarray(bpar, dtype=np.float64), (I,))
    R = int(particles)
    Mb = int(M) if M else 65535
    a = np.float64(a)
    n_out = np.array(n, dtype=np.int64)
    t_out = np.array(t, dtype=np.int64)
    stride = None
    if lik is not None:
        lik = np.asarray(lik, dtype=np.float64)
        rows = lik.shape[0] if rows is None else rows
        stride = lik.shape[1]
    skip = skipped_mask(K, Cn, stride)
    T_out = np.zeros(I, dtype=np.int64)
    for i in range(I):
        T_out[i] = int(t_out[koff[i]:koff[i + 1]].sum())
    cust = np.zeros(C, dtype=np.int64)
    p_out = np.zeros(C)
    lw = np.zeros((I, R))
    out = {"skipped": int(skip.sum()), "impossible": 0, "stuck": 0}
    if bars:
        out.update({"pbar": np.zeros((C, R)), "pall": np.zeros((C, R)), "ks": np.zeros((C, R), dtype=np.int64),
                    "new": np.zeros((C, R), dtype=bool)})
    keys = np.array([particle_key(seed, sweep, r) for r in range(R)], dtype=np.uint64)
    groups = {}
    for i in range(I):
        if not skip[i]:
            groups.setdefault((int(K[i]), int(Cn[i])), []).append(i)
    for (Ki, Ci), members in groups.items():
        mem = np.asarray(members, dtype=np.int64)
        if Ki == 0 or Ci == 0:
            continue
        nb = -(-Ki // 64)
        KP = 64 * nb
        m = len(mem) * R
        rest = np.repeat(mem, R)                       # item -> restaurant
        key = np.tile(keys, len(mem))
        col = np.arange(KP)
        live = np.broadcast_to(col[None, :] < Ki, (m, KP))
        idx = koff[rest][:, None] + np.minimum(col, Ki - 1)[None, :]
        nn = np.where(live, np.asarray(n, dtype=np.int64)[idx], 0)
        tt = np.where(live, np.asarray(t, dtype=np.int64)[idx], 0)
        hh = np.where(live, np.asarray(h, dtype=np.float64)[idx], 0.0) if h is not None else np.where(live, 1.0, 0.0)
        b = bpar[rest]
        T, N = tt.sum(axis=1), nn.sum(axis=1)
        hi, lo = np.zeros(m), np.zeros(m)
        dead = np.zeros(m, dtype=bool)
        ar = np.arange(m)
        likp = None
        if lik is not None:
            likp = np.zeros((rows + 1, KP))            # (row `rows`: a class outside the matrix)
            W = min(KP, stride)
            likp[:rows, :W] = lik[:rows, :W]
        for j in range(Ci):
            c = coff[rest] + j
            u2 = unit(key, 2 * c.astype(np.uint64) + np.uint64(2))
            u3 = unit(key, np.uint64(2 * C + 1) + c.astype(np.uint64))
            if mut == "swap":
                u2, u3 = u3, u2
            Tf, Nf = T.astype(np.float64), N.astype(np.float64)
            g = b + Tf * a if mut != "noTa" else b + 0.0
            den = b + Nf
            tx = tt + 1 if mut == "t+1" else tt
            ta = tx.astype(np.float64) * a
            x = nn.astype(np.float64) - ta
            gh = g[:, None] * hh
            capped = (nn >= 1) & (tt + 1 > Mb)
            y = np.where(capped, 0.0, gh)
            num = x + y
            with np.errstate(divide="ignore", invalid="ignore"):
                th = np.where((N == 0)[:, None], hh, num / den[:, None])
            th = np.where(live, th, 0.0)
            if likp is not None:
                w = np.minimum(np.asarray(cls, dtype=np.int64)[c], rows)
                L = likp[w]
            else:
                L = np.ones((m, KP))
            q = np.where(live, th * L, 0.0)
            cum, Z = cumsum64(q, linear=(mut == "linear"))
            bad = ~((Z > 0.0) & np.isfinite(Z))
            pc = np.where(bad, 0.0, Z)
            stuck = np.zeros(m, dtype=bool)
            if bad.any():
                cum2, Z2 = cumsum64(th[bad], linear=(mut == "linear"))
                q = q.copy()
                q[bad], cum[bad], Z[bad] = th[bad], cum2, Z2
                stuck[bad] = ~((Z2 > 0.0) & np.isfinite(Z2))
            thr = u3 * Z
            pos = q > 0.0
            with np.errstate(invalid="ignore"):
                hit = pos & (cum > thr[:, None])
            last = KP - 1 - np.argmax(pos[:, ::-1], axis=1)
            ks = np.where(hit.any(axis=1), np.argmax(hit, axis=1), last)
            ks = np.where(stuck, 0, ks)
            ns, xs, ys = nn[ar, ks], x[ar, ks], y[ar, ks]
            with np.errstate(invalid="ignore"):
                new = (ns == 0) | (u2 * (xs + ys) < ys)
            if bars:
                e_x = U * (np.abs(ta) + np.abs(x))
                e_g = U * (np.abs(Tf * a) + np.abs(g))
                e_y = np.where(capped, 0.0, e_g[:, None] * hh + U * np.abs(gh))
                e_num = e_x + e_y + U * np.abs(num)
                with np.errstate(divide="ignore", invalid="ignore"):
                    thb = np.where(live & (num != 0.0), np.abs(th) * (e_num / np.abs(num) + 2.0 * U), 0.0)
                thb = np.where((N == 0)[:, None], 0.0, thb)
                pb = ((thb * L).sum(axis=1) + U * (7 + nb) * np.abs(np.where(bad[:, None], 0.0, q)).sum(axis=1)) * SLACK
                rr = ar % R
                out["pbar"][c, rr], out["pall"][c, rr], out["ks"][c, rr], out["new"][c, rr] = pb, pc, ks, new
            nn[ar, ks] += 1
            tt[ar, ks] += new
            N = N + 1
            T = T + new
            dead |= bad
            with np.errstate(divide="ignore"):
                xl = np.where(bad, 0.0, np.log(np.where(bad, 1.0, pc)))
            hi, lo = pro.dd_add(hi, lo, xl)
            out["impossible"] += int(bad.sum())
            out["stuck"] += int(stuck.sum())
            first = ar % R == 0
            cust[c[first]] = ks[first]
            p_out[c[first]] = pc[first]
        lw[rest, ar % R] = np.where(dead, NEG_INF, hi + lo)
        first = np.flatnonzero(ar % R == 0)
        for it in first:
            i = int(rest[it])
            n_out[koff[i]:koff[i + 1]] = nn[it, :Ki]
            t_out[koff[i]:koff[i + 1]] = tt[it, :Ki]
            T_out[i] = int(T[it])
    out.update({"n": n_out.astype(np.uint32), "t": t_out.astype(np.uint16), "T": T_out.astype(np.uint32),
                "cust": cust.astype(np.uint32), "p": p_out, "lw": lw})
    return out


LOGLIK_MUTS = ("meanpad", "max64", "base1", "plain", "linear", "stale", "skipstage")
STAGE = 1024      # ST_STAGE: block sums the last workgroup stages at a time


def loglik_total(Hi, mut=None, grid_x=None):
    """k_seat_sum's total of the H_i it was given: dead rows (-inf) as 0.0, padded with 0.0 to whole blocks of 256, every
    block by pro.block_tree, the block sums in order in double-double, hi + lo; -inf when a row is dead.  The kernel's own
    association leaves no rounding freedom here: the device's total has these bits.  mut, the wrong totals: 'plain' adds
    the block sums in plain double; 'linear' adds a block left to right; 'stale' leaves in the tail of a short last block
    what the workgroup's previous block (grid_x blocks earlier; without grid_x the one before) held; 'skipstage' leaves out
    the second STAGE block sums."""
    Hi = np.asarray(Hi, dtype=np.float64)
    I = Hi.shape[0]
    dead = Hi == NEG_INF
    nblk = max(1, -(-I // 256))
    full = np.zeros(nblk * 256)
    full[:I] = np.where(dead, 0.0, Hi)
    full = full.reshape(nblk, 256)
    if mut == "stale" and nblk > 1 and I % 256:
        prev = nblk - 1 - grid_x if grid_x and nblk - 1 - grid_x >= 0 else nblk - 2
        full[-1, I % 256:] = full[prev, I % 256:]
    part = np.cumsum(full, axis=1)[:, -1] if mut == "linear" else pro.block_tree(full)
    if mut == "skipstage":
        part = np.concatenate([part[:STAGE], part[2 * STAGE:]])
    if mut == "plain":
        total = 0.0
        for v in part:
            total = total + float(v)
    else:
        total = float(pro.ordered_dd_sum(part))
    return NEG_INF if dead.any() else total


def loglik_replay(lw, mut=None, grid_x=None):
    """stb_seat_loglik on lw (I, R): (H_i, total, restaurants whose H_i is -inf).  mut, the wrong rows: 'meanpad' takes the
    mean over 64 ceil(R / 64) particles, 'max64' the maximum over the first 64 particles only, 'base1' the sum over the
    first 64 only; the wrong totals are loglik_total's"""
    lw = np.asarray(lw, dtype=np.float64)
    I, R = lw.shape
    m = (lw[:, :64] if mut == "max64" else lw).max(axis=1)
    ok = m > NEG_INF
    s = np.zeros(I)
    Rs = min(R, 64) if mut == "base1" else R
    Rm = 64 * -(-R // 64) if mut == "meanpad" else R
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for r in range(Rs):
            s = s + np.where(ok, np.exp(np.where(ok, lw[:, r] - m, 0.0)), 0.0)
        Hi = np.where(ok, m + np.log(np.where(ok, s / np.float64(Rm), 1.0)), NEG_INF)
    return Hi, loglik_total(Hi, mut, grid_x), int((~ok).sum())


def loglik_rows_truth(lw):
    """H_i = log((1/R) sum_r exp(lw_ir)) of every row in x87 long double (hp_oracle.check_longdouble refuses a platform
    without it): np.longdouble [I], -inf for a row of -inf only.  The inputs are exact doubles; lw_r - m rounds to 2^-64
    relatively, exp and log are long double's, and the R - 1 additions of positive terms lose at most R 2^-64 of s: at
    R = 4096 that is two u against a bar of 4098 u, and less for fewer particles."""
    hp.check_longdouble()
    lw = np.asarray(lw, dtype=np.float64).astype(hp.LD)
    R = lw.shape[1]
    m = lw.max(axis=1)
    ok = m > NEG_INF
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.where(ok[:, None], lw - np.where(ok, m, hp.LD(0))[:, None], hp.LD(0))
        s = np.where(ok, np.exp(d).sum(axis=1), hp.LD(1))
        return np.where(ok, m + np.log(s / hp.LD(R)), hp.LD(NEG_INF))


def loglik_rows_bar(lw, Hi):
    """the docstring's H_i bar of rows whose lw are exact (max_r bar(lw_r) = 0): rho = max_r u |d_r| + (R + 2) u over the
    live particles, plus 2 u |log(s / R)| = 2 u |H_i - m|, plus u |H_i|, times SLACK; 0 for a row of -inf only.  Hi: the
    truth's (any H_i within the bar gives the same bar to second order)"""
    lw = np.asarray(lw, dtype=np.float64)
    R = lw.shape[1]
    Hi = np.asarray(Hi).astype(np.float64)
    m = lw.max(axis=1)
    ok = m > NEG_INF
    with np.errstate(invalid="ignore"):
        d = np.where(np.isfinite(lw) & ok[:, None], np.abs(lw - np.where(ok, m, 0.0)[:, None]), 0.0).max(axis=1)
        rho = U * d + (R + 2) * U
        bar = (rho + 2.0 * U * np.abs(Hi - m) + U * np.abs(Hi)) * SLACK
    return np.where(ok, bar, 0.0)


def loglik_total_truth(Hi, Hb):
    """(the sum of the truth's H_i, its bar): the docstring's total bar, sum_i bar(H_i) + 8 u sum_i |H_i| + u (2 |total| + 16),
    times SLACK; (-inf, 0) when a row is dead.  The long-double sum of I terms loses at most I 2^-64 sum |H_i|: under the
    8 u sum |H_i| by a factor of 2^14 / I (I <= 2^21 here: a hundredth)"""
    Hi = np.asarray(Hi)
    if (Hi == NEG_INF).any():
        return NEG_INF, 0.0
    tot = Hi.astype(hp.LD).sum()
    bar = (float(np.sum(Hb)) + 8.0 * U * float(np.abs(Hi).sum()) + U * (2.0 * abs(float(tot)) + 16.0)) * SLACK
    return tot, bar


def over_bar(got, want, bar) -> float:
    """the largest |got - want| / bar; infinities must agree exactly (else inf), a NaN is inf"""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want)
    bar = np.asarray(bar, dtype=np.float64)
    inf = ~np.isfinite(want.astype(np.float64))
    if np.isnan(got).any() or not np.array_equal(got[inf], want[inf].astype(np.float64)) or np.isinf(got[~inf]).any():
        return math.inf
    if inf.all():
        return 0.0
    err = np.abs(got[~inf].astype(hp.LD) - want[~inf].astype(hp.LD)).astype(np.float64)
    return float((err / bar[~inf]).max())


LW_TYPES, LW_SEED = 257, 0x10C1
LW_ALLEQ, LW_MAXLAST, LW_SPREAD, LW_MAX64 = 0, 1, 2, 4      # row types of a fixed make; the last type may be dead


@lru_cache(maxsize=None)
def lw_types(R: int, seed: int = LW_SEED, dead_row: bool = False):
    """257 rows of R synthetic log weights (read-only): particle r of row i lies up to dep_i below the row's offset off_i,
    off_i in [-500, 0] (one at -500), dep_i from 1e-3 to 600, log-uniform.  Rows 8, 13, 18, .. (i mod 5 = 3, R >= 2) have
    dead particles (-inf) among live ones; row LW_ALLEQ has all particles equal; row LW_MAXLAST its maximum, by 1, at the
    last particle; row LW_SPREAD (R >= 2) its live particles 720 to 820 apart -- the low ones first, the high ones from
    particle 64 on (R <= 64: the last alone), so a maximum over the first 64 overflows and a sum over them flushes to 0;
    row LW_MAX64 (R > 64) its maximum at particle 64.  dead_row: the last type is -inf throughout.  257 is coprime to 256:
    tiled over I restaurants (row type i mod 257), every block of 256 sees another phase."""
    rng = np.random.default_rng([seed, R])
    T = LW_TYPES
    off = -500.0 * rng.random(T)
    off[6] = -500.0
    dep = 10.0 ** rng.uniform(-3.0, math.log10(600.0), size=T)
    lw = off[:, None] - dep[:, None] * rng.random((T, R))
    if R >= 2:
        for i in range(8, T, 5):
            dead = rng.random(R) < 0.3
            dead[int(rng.integers(R))] = False
            lw[i, dead] = NEG_INF
        low = off[LW_SPREAD] - 720.0 - 100.0 * rng.random(R)
        high = np.arange(R) >= 64 if R > 64 else np.arange(R) == R - 1
        lw[LW_SPREAD] = np.where(high, off[LW_SPREAD] - rng.random(R), low)
    lw[LW_ALLEQ] = off[LW_ALLEQ]
    lw[LW_MAXLAST, R - 1] = lw[LW_MAXLAST].max() + 1.0
    if R > 64:
        lw[LW_MAX64, 64] = lw[LW_MAX64].max() + 0.5
    if dead_row:
        lw[T - 1] = NEG_INF
    lw.setflags(write=False)
    return lw


def past_one_block(grid_x: int) -> int:
    """restaurants that give a grid of grid_x workgroups one block sum more than a step each (70000 at least)"""
    return max(70000, grid_x * 256 + 1)


# ---------------------------------------------------------------------------------------------------- truth and bars

_S = 1126  # every double is an integer over 2^1126


def _dyad(v: float) -> int:
    num, den = float(v).as_integer_ratio()
    return num * ((1 << _S) // den)


def truth(K, n, t, h, a, bpar, coff, cls, lik, M, rep, restaurants=None):
    """mpmath truth along the paths of rep (a replay with bars=True): a dict lw (I, R) floats (-inf for a dead particle),
    lw_bar (I, R), W (per restaurant a list of R mpf), for the restaurants listed (None: all that were not skipped)"""
    mp = hp._mp()
    K = np.asarray(K, dtype=np.int64)
    I = K.shape[0]
    koff = np.concatenate([[0], np.cumsum(K)]).astype(np.int64)
    coff = np.asarray(coff, dtype=np.int64)
    R = rep["lw"].shape[1]
    Mb = int(M) if M else 65535
    an, ad = float(a).as_integer_ratio()
    ea = ad.bit_length() - 1
    bpar = np.broadcast_to(np.asarray(bpar, dtype=np.float64), (I,))
    rows = 1 if lik is None else lik.shape[0]
    lw, lw_bar, Ws = np.zeros((I, R)), np.zeros((I, R)), {}
    skip = skipped_mask(K, np.diff(coff), None if lik is None else lik.shape[1])
    for i in (range(I) if restaurants is None else restaurants):
        if skip[i]:
            continue
        Ki, k0 = int(K[i]), int(koff[i])
        Li = [[(_dyad(lik[w, k]) if lik is not None else 1 << _S) for k in range(Ki)] for w in range(rows)]
        Hd = [_dyad(h[k0 + k]) if h is not None else 1 << _S for k in range(Ki)]
        n0 = [int(v) for v in n[k0:k0 + Ki]]
        t0 = [int(v) for v in t[k0:k0 + Ki]]
        cap0 = [n0[k] >= 1 and t0[k] + 1 > Mb for k in range(Ki)]
        A0 = [sum(n0[k] * Li[w][k] for k in range(Ki)) for w in range(rows)]
        B0 = [sum(t0[k] * Li[w][k] for k in range(Ki)) for w in range(rows)]
        G0 = [sum(Hd[k] * Li[w][k] for k in range(Ki) if not cap0[k]) for w in range(rows)]
        F0 = [sum(Hd[k] * Li[w][k] for k in range(Ki)) for w in range(rows)]   # N = 0: theta = h on every dish
        bn, bd = float(bpar[i]).as_integer_ratio()
        eb = bd.bit_length() - 1
        E = 2 * _S + ea                      # p = num / den * 2^-E with the integers below
        Ws[i] = []
        for r in range(R):
            nn, tt, cap = list(n0), list(t0), list(cap0)
            A, B, G = list(A0), list(B0), list(G0)
            T, N = sum(t0), sum(n0)
            Wn, Wd, cnt, bar, dead = mp.mpf(1), mp.mpf(1), 0, 0.0, False
            for c in range(int(coff[i]), int(coff[i + 1])):
                w = int(cls[c]) if lik is not None else 0
                if w >= rows:
                    num, den = 0, 1
                elif N == 0:
                    num, den = F0[w] << ea, 1
                else:
                    num = (A[w] << (_S + ea + eb)) - ((an * B[w]) << (_S + eb)) + ((bn << ea) + ((T * an) << eb)) * G[w]
                    den = bn + (N << eb)
                pr = rep["pall"][c, r]
                if num > 0 and pr > 0.0:
                    Wn *= num
                    Wd *= den
                    cnt += 1
                    bar += rep["pbar"][c, r] / pr + 2.0 * U * abs(math.log(pr))
                else:
                    assert num == 0 and pr == 0.0, (i, r, c, num, pr)
                    dead = True
                k, new = int(rep["ks"][c, r]), bool(rep["new"][c, r])
                for v in range(rows):
                    A[v] += Li[v][k]
                    if new:
                        B[v] += Li[v][k]
                nn[k] += 1
                tt[k] += int(new)
                N += 1
                T += int(new)
                if not cap[k] and tt[k] + 1 > Mb:
                    cap[k] = True
                    for v in range(rows):
                        G[v] -= Hd[k] * Li[v][k]
            W = mp.ldexp(Wn / Wd, -cnt * E)
            Ws[i].append(mp.mpf(0) if dead else W)
            lw[i, r] = NEG_INF if dead else float(mp.log(W))
            lw_bar[i, r] = 0.0 if dead else (bar + U * abs(lw[i, r])) * SLACK
    return {"lw": lw, "lw_bar": lw_bar, "W": Ws}


def loglik_truth(tr, restaurants, R: int):
    """(H_i, H_i's bars, total, total's bar) over the first R particles of truth()'s result, for the restaurants listed"""
    mp = hp._mp()
    Hi, Hb = [], []
    tot, tot_abs, any_inf = mp.mpf(0), 0.0, False
    for i in restaurants:
        W = tr["W"][i][:R]
        s = mp.fsum(W)
        if s == 0:
            Hi.append(NEG_INF)
            Hb.append(0.0)
            any_inf = True
            continue
        Hm = mp.log(s / R)
        lw, lb = tr["lw"][i, :R], tr["lw_bar"][i, :R]
        alive = lw > NEG_INF
        m = float(lw[alive].max())
        rho = U * float(np.abs(lw[alive] - m).max()) + (R + 2) * U
        bar = float(lb[alive].max()) + rho + 2.0 * U * abs(float(Hm) - m) + U * abs(float(Hm))
        Hi.append(float(Hm))
        Hb.append(bar * SLACK)
        tot += Hm
        tot_abs += abs(float(Hm))
    total = NEG_INF if any_inf else float(tot)
    tbar = (sum(Hb) + 8.0 * U * tot_abs + U * (2.0 * abs(float(tot)) + 16.0)) * SLACK
    return np.array(Hi), np.array(Hb), total, tbar


within = pro.within


# ---------------------------------------------------------------------------------------------------- exact path law

def ujoint(ns, ts, hs, a: float, b: float) -> float:
    """(b|a)_T / (b)_N prod_k S^{n_k}_{t_k} h_k^{t_k}, the leading b of both products cancelled (so b <= 0 < b + a works)"""
    T, N = sum(ts), sum(ns)
    v = 1.0
    for j in range(1, T):
        v *= b + j * a
    for j in range(1, N):
        v /= b + j
    for nk, tk, hk in zip(ns, ts, hs):
        if nk:
            v *= tio.stirling(nk, a)[tk] * hk ** tk
    return v


def ujoint_states(Nc: int, K: int, hs, a: float, b: float, cls=None, lik=None, M=None) -> np.ndarray:
    """ujoint times prod_c L[cls_c][z_c] over td_oracle.states(Nc, K, M), in that order: td_oracle.joint before it is
    normalised, divided by (b)_N"""
    out = []
    for z, ts in tdo.states(Nc, K, M):
        v = ujoint(tdo.counts(z, K), ts, hs, a, b)
        if lik is not None:
            v *= math.prod(lik[cls[c]][k] for c, k in enumerate(z))
        out.append(v)
    return np.array(out)


def enumerate_paths(n0, t0, hs, a: float, b: float, cls, lik=None, M=None, mut=None):
    """every path of the customers cls (their classes, in order) from the start pairs (n0, t0), the uniforms integrated
    out: {(z, final t): [sum P W, sum P, sum P W^2]}, z the new customers' dishes.  mut 'noTa': the wrong seating"""
    K = len(n0)
    Mb = M or 65535
    acc = {}

    def walk(c, nn, tt, z, P, W):
        if c == len(cls):
            e = acc.setdefault((z, tuple(tt)), [0.0, 0.0, 0.0])
            e[0] += P * W
            e[1] += P
            e[2] += P * W * W
            return
        T, N = sum(tt), sum(nn)
        g = b + T * a if mut != "noTa" else b
        den = b + N
        xs = [nn[k] - tt[k] * a for k in range(K)]
        ys = [0.0 if (nn[k] >= 1 and tt[k] + 1 > Mb) else g * hs[k] for k in range(K)]
        th = [hs[k] if N == 0 else (xs[k] + ys[k]) / den for k in range(K)]
        q = [th[k] * (1.0 if lik is None else lik[cls[c]][k]) for k in range(K)]
        Z = sum(q)
        pc = Z
        if not Z > 0.0:
            pc, q, Z = 0.0, th, sum(th)
        for k in range(K):
            if q[k] <= 0.0:
                continue
            heads = [(True, 1.0)] if nn[k] == 0 else [(True, ys[k] / (xs[k] + ys[k])), (False, xs[k] / (xs[k] + ys[k]))]
            for new, ph in heads:
                if ph <= 0.0:
                    continue
                n2, t2 = list(nn), list(tt)
                n2[k] += 1
                t2[k] += int(new)
                walk(c + 1, n2, t2, z + (k,), P * q[k] / Z * ph, W * pc)

    walk(0, list(n0), list(t0), (), 1.0, 1.0)
    return acc


# ---------------------------------------------------------------------------------------------------- the cases

SEED = 0x5EA7

R_SET = (1, 2, 7, 64)
R_STUCK, R_CLASS, R_NOK = 0, 1, 12   # h = 0 under a zero column; a class >= rows; no dishes, three customers


@lru_cache(maxsize=None)
def raw_case(a: float):
    """pr_oracle.raw_case's twelve restaurants as a seating case, (K, n, t, h, bpar, coff, cls, lik): the held-out
    customers are the ones to seat.  Column 0 of the matrix is zero and restaurant 0 (one dish) is empty with h = 0: its
    visit is impossible and stuck; a customer of restaurant 1 has a class outside the matrix; a thirteenth restaurant has
    no dishes and three customers (skipped)."""
    K, n, t, h, bpar, hoff, hcls, lik = pro.raw_case(a)
    K = np.concatenate([K, [0]]).astype(np.int32)
    n, t, h, lik, cls = n.copy(), t.copy(), h.copy(), lik.copy(), hcls.copy()
    lik[:, 0] = 0.0
    n[0], t[0], h[0] = 0, 0, 0.0
    cls[int(hoff[R_CLASS]) + 5] = pro.RAW_ROWS
    coff = np.concatenate([hoff, [int(hoff[-1]) + 3]]).astype(np.uint64)
    cls = np.concatenate([cls, [0, 1, 2]]).astype(np.uint32)
    bpar = np.concatenate([bpar, [1.0]])
    out = (K, n, t, h, bpar, coff, cls, lik)
    for x in out:
        x.setflags(write=False)
    return out


RAW_CONFIGS = ((0.0, 0), (0.5, 0), (0.999, 0), (0.5, 2))   # (a, M); every a > 0 has restaurant pr_oracle.R_NEGB at -a < b < 0
RAW_SWEEP = 3


@lru_cache(maxsize=None)
def raw_replay(a: float, M: int, particles: int = 1, bars: bool = False):
    K, n, t, h, bpar, coff, cls, lik = raw_case(a)
    return replay(K, n, t, h, a, bpar, coff, cls, lik, M=M, seed=SEED, sweep=RAW_SWEEP, particles=particles, bars=bars)


@lru_cache(maxsize=None)
def raw_truth(a: float, M: int, particles: int):
    K, n, t, h, bpar, coff, cls, lik = raw_case(a)
    return truth(K, n, t, h, a, bpar, coff, cls, lik, M, raw_replay(a, M, particles, True))


LAW_I, LAW_A, LAW_B, LAW_SWEEP = 20000, 0.4, 1.2, 0
LAW_H = (0.35, 0.65)
LAW_CLS = (0, 1, 0)
LAW_LIK = ((0.7, 0.2), (0.3, 0.8))
LAW_SEED = 11     # chosen on the CPU so that the replay passes tests/test_seat_host.py's law test


@lru_cache(maxsize=None)
def law_case():
    """20000 equal restaurants of 3 customers, 2 dishes, 2 classes, empty: (K, n, t, h, bpar, coff, cls, lik)"""
    I = LAW_I
    K = np.full(I, 2, dtype=np.int32)
    out = (K, np.zeros(2 * I, dtype=np.uint32), np.zeros(2 * I, dtype=np.uint16), np.tile(np.array(LAW_H), I),
           np.full(I, LAW_B), (3 * np.arange(I + 1)).astype(np.uint64), np.tile(np.array(LAW_CLS, dtype=np.uint32), I),
           np.array(LAW_LIK))
    for x in out:
        x.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def law_replay(seed: int = LAW_SEED):
    K, n, t, h, bpar, coff, cls, lik = law_case()
    return replay(K, n, t, h, LAW_A, bpar, coff, cls, lik, seed=seed, sweep=LAW_SWEEP)


GRID_I, GRID_R, GRID_A, GRID_SEED, GRID_SWEEP = 16385, 64, 0.4, 0x6E1D, 5
GRID_CAP = 1 << 20    # k_seat's grid is capped at this many workgroups


@lru_cache(maxsize=None)
def grid_case(I: int = GRID_I):
    """I restaurants of 2 dishes and 3 customers to seat, random small start pairs, h, a b per restaurant, 2 classes and a
    2 x 2 matrix: (K, n, t, h, bpar, coff, cls, lik).  At GRID_I and GRID_R particles a launch of one wave a workgroup has
    GRID_CAP + 64 items: the particles of the last restaurant are the grid-stride loop's second step."""
    rng = np.random.default_rng([GRID_SEED, I])
    n = rng.integers(0, 5, size=2 * I).astype(np.uint32)
    t = np.where(n > 0, 1 + np.floor(rng.random(2 * I) * n), 0).astype(np.uint16)
    out = (np.full(I, 2, dtype=np.int32), n, t, 0.05 + rng.random(2 * I), 0.3 + 4.0 * rng.random(I),
           (3 * np.arange(I + 1)).astype(np.uint64), rng.integers(0, 2, size=3 * I).astype(np.uint32), np.array(LAW_LIK))
    for x in out:
        x.setflags(write=False)
    return out


def grid_band(I: int = GRID_I):
    """the restaurants held to the replay: the last nine (at GRID_I, the second step and the eight before it) and the
    first eight, in index order"""
    return list(range(8)) + list(range(I - 9, I))


def band_case(case, band):
    """the case with every restaurant outside the band turned into one without dishes (skipped): the flat customer indices
    and C stay, so the band's streams do"""
    K, n, t, h, bpar, coff, cls, lik = case
    koff = np.concatenate([[0], np.cumsum(K)]).astype(np.int64)
    band = sorted(band)
    keep = np.concatenate([np.arange(koff[i], koff[i + 1]) for i in band]).astype(np.int64)
    K2 = np.zeros_like(K)
    K2[band] = K[band]
    return K2, n[keep], t[keep], h[keep], bpar, coff, cls, lik


@lru_cache(maxsize=None)
def grid_band_truth(I: int = GRID_I, R: int = GRID_R):
    """(the band, its replay with bars on band_case, the truth along it)"""
    band = grid_band(I)
    K, n, t, h, bpar, coff, cls, lik = band_case(grid_case(I), band)
    rep = replay(K, n, t, h, GRID_A, bpar, coff, cls, lik, seed=GRID_SEED, sweep=GRID_SWEEP, particles=R, bars=True)
    return band, rep, truth(K, n, t, h, GRID_A, bpar, coff, cls, lik, 0, rep, restaurants=band)


BOUND_A, BOUND_B, BOUND_N, BOUND_C, BOUND_SWEEP = 0.5, 1.0e5, 70000, 8, 0
BOUND_T = (65534, 65535, 65534, 65535)     # the pinned dish's tables: restaurants 0, 1 (K = 1) and 2, 3 (K = 65, dish 64)
# The smallest seed from 0 for which, in the replay, the pinned dish of restaurants 0 and 2 (t = 65534) opens its table
# with at least two of the eight customers still to come to it: they meet the dish at t = 65535, where a table more would
# wrap the uint16, and both restaurants of 65 dishes seat somebody at another dish as well (tests/test_seat_host.py:
# test_the_bound_seed_is_the_first_that_opens_the_table_early).
BOUND_SEED = 1


def bound_seed_ok(seed: int) -> bool:
    o = bound_opened(bound_replay(seed))
    return all(o[i][0] == 1 and o[i][1] >= 2 for i in (0, 2)) and all(o[i][4] >= 1 for i in (2, 3))


@lru_cache(maxsize=None)
def bound_case():
    """M = 0 (the kernel's 65535) and b = 1e5, so that a customer of the pinned dish opens a table with probability 0.78
    while it may: four restaurants of eight customers, the pinned dish (n = 70000, h = 1) at t = 65534 and at 65535, alone
    (K = 1, the register form) and as dish 64 of 65 (the LDS form; the others n = t = 1, h = 1e-3: one visit in twenty).
    (K, n, t, h, bpar, coff, None, None)"""
    K = np.array([1, 1, 65, 65], dtype=np.int32)
    n, t, h = [], [], []
    for Ki, tb in zip(K, BOUND_T):
        n += [1] * (Ki - 1) + [BOUND_N]
        t += [1] * (Ki - 1) + [tb]
        h += [1.0e-3] * (Ki - 1) + [1.0]
    out = (K, np.array(n, dtype=np.uint32), np.array(t, dtype=np.uint16), np.array(h), np.full(4, BOUND_B),
           (BOUND_C * np.arange(5)).astype(np.uint64))
    for x in out:
        x.setflags(write=False)
    return out + (None, None)


@lru_cache(maxsize=None)
def bound_replay(seed: int = BOUND_SEED):
    K, n, t, h, bpar, coff, _, _ = bound_case()
    return replay(K, n, t, h, BOUND_A, bpar, coff, M=0, seed=seed, sweep=BOUND_SWEEP, bars=True)


def bound_opened(rep):
    """per restaurant (tables the pinned dish opened, its visits after the first of them, its final t, the final T, the
    visits of other dishes)"""
    K, n, t, h, bpar, coff, _, _ = bound_case()
    out = []
    for i, Ki in enumerate(K):
        sl = slice(int(coff[i]), int(coff[i + 1]))
        at = rep["ks"][sl, 0] == Ki - 1
        new = rep["new"][sl, 0] & at
        first = int(np.argmax(new)) if new.any() else BOUND_C
        koff = int(np.sum(K[:i]))
        out.append((int(new.sum()), int(at[first + 1:].sum()), int(rep["t"][koff + Ki - 1]), int(rep["T"][i]),
                    int((~at).sum())))
    return out


def law_cells(rep):
    """the final states of law_replay as a dict {(z, t): count}"""
    z = rep["cust"].reshape(LAW_I, 3)
    tt = rep["t"].reshape(LAW_I, 2)
    keys, cnt = np.unique(np.concatenate([z, tt], axis=1), axis=0, return_counts=True)
    return {(tuple(int(v) for v in k[:3]), tuple(int(v) for v in k[3:])): int(c) for k, c in zip(keys, cnt)}


def chi2_p(cells, law, total: int, floor: float = 5.0):
    """the chi-square p-value of the counts `cells` against the law {state: probability}; states expected less than
    `floor` times are taken together; a state outside the law's support makes it 0"""
    from scipy.stats import chi2
    if any(k not in law or law[k] <= 0.0 for k in cells):
        return 0.0
    big = [(total * pr, cells.get(k, 0)) for k, pr in law.items() if total * pr >= floor]
    small = [(total * pr, cells.get(k, 0)) for k, pr in law.items() if 0.0 < total * pr < floor]
    if small:
        big.append((sum(e for e, _ in small), sum(o for _, o in small)))
    stat = sum((o - e) ** 2 / e for e, o in big)
    return float(chi2.sf(stat, len(big) - 1))
