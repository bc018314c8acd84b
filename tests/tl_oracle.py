"""A numpy replay of the device draws of the likelihood matrix and the base weights (include/stb_hip.h, "the likelihood
and the base weights": stb_sample_lik, stb_tindic_sample_h) and of the data term's association (stb_lik_loglik), written
from the header's text.

  key = mix(seed + (sweep+1) gamma); cell e owns key_e = mix(key + (e+1) gamma); its uniforms are elements 1, 2, ... of that
  substream (hq_oracle.unit).  e = w stride + k for the likelihood, e = k for the base weights.
  log Gamma(alpha >= 1) variate: d = alpha - 1/3, c = 1/sqrt(9 d); an attempt takes u1, u2, x = sqrt(-2 log u1) cos(2 pi u2),
  w = 1 + c x; w <= 0 ends the attempt; else v = w^3, a third uniform u, accepted when
  log u < ((x x / 2 + d) - d v) + d log v, giving log d + log v.  alpha < 1: the variate of alpha + 1, plus log(u') / alpha.
  Normalisation of a column: M = max lg; e = exp(lg - M); rows in chunks of 256, a chunk's sum in row order from its first,
  Z the chunk sums in chunk order; lik = e / Z.

Every replay also returns the smallest acceptance margin it met: |log u - right-hand side| over every attempt that reached
the test, and |w| for the w > 0 test.  A seed whose margin is tiny sits on a tie that a transcendental's last bit decides.
"""
import math

import numpy as np

import hq_oracle as hqo

CHUNK = 256


def log_gamma(alpha, key_e):
    """(log of a Gamma(alpha) variate per cell, smallest margin); raises if a loop ran out"""
    alpha = np.asarray(alpha, dtype=np.float64)
    n = alpha.shape[0]
    small = alpha < 1.0
    al = np.where(small, alpha + 1.0, alpha)
    k = np.zeros(n, dtype=np.uint64)
    out = np.full(n, np.nan)
    live = np.ones(n, dtype=bool)
    d = al - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    margin = math.inf
    for _ in range(hqo.CAP):
        idx = np.nonzero(live)[0]
        if idx.size == 0:
            break
        ki = key_e[idx]
        k[idx] += np.uint64(1)
        u1 = hqo.unit(ki, k[idx])
        k[idx] += np.uint64(1)
        u2 = hqo.unit(ki, k[idx])
        x = np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)
        w = 1.0 + c[idx] * x
        margin = min(margin, float(np.abs(w).min()))
        pos = w > 0.0
        idx, x, w = idx[pos], x[pos], w[pos]
        if idx.size == 0:
            continue
        ki = key_e[idx]
        v = w * w * w
        k[idx] += np.uint64(1)
        u = hqo.unit(ki, k[idx])
        lv = np.log(v)
        lu = np.log(u)
        di = d[idx]
        rhs = ((0.5 * (x * x) + di) - di * v) + di * lv
        margin = min(margin, float(np.abs(lu - rhs).min()))
        acc = lu < rhs
        out[idx[acc]] = np.log(di[acc]) + lv[acc]
        live[idx[acc]] = False
    if live.any():
        raise RuntimeError("a Gamma draw was not accepted within %d attempts" % hqo.CAP)
    if small.any():
        idx = np.nonzero(small)[0]
        k[idx] += np.uint64(1)
        u = hqo.unit(key_e[idx], k[idx])
        out[idx] = out[idx] + np.log(u) / alpha[idx]
    return out, margin


def cell_keys(seed: int, sweep: int, cells: int):
    key = hqo.sweep_key(seed, sweep)
    with np.errstate(over="ignore"):
        return hqo.mix(key + (np.arange(cells, dtype=np.uint64) + np.uint64(1)) * hqo.GAMMA)


def chunk_sums(x):
    """the column sums of x (rows, stride) in the header's association: a chunk of 256 rows in row order starting from its
    first row, then the chunks in order"""
    rows = x.shape[0]
    total = None
    for w0 in range(0, rows, CHUNK):
        s = x[w0].copy()
        for w in range(w0 + 1, min(rows, w0 + CHUNK)):
            s = s + x[w]
        total = s if total is None else total + s
    return total


def normalise(lg):
    """lg (rows, stride) -> the matrix whose columns sum to 1"""
    M = lg.max(axis=0)
    e = np.exp(lg - M[None, :])
    return e / chunk_sums(e)[None, :]


def sample_lik(cnt, beta, seed: int, sweep: int):
    """(lik (rows, stride), smallest margin); beta a scalar or rows values"""
    cnt = np.asarray(cnt)
    rows, stride = cnt.shape
    b = np.broadcast_to(np.asarray(beta, dtype=np.float64).reshape(-1, 1), (rows, stride)) if np.ndim(beta) else float(beta)
    alpha = (b + cnt.astype(np.float64)).reshape(-1)
    lg, margin = log_gamma(alpha, cell_keys(seed, sweep, rows * stride))
    return normalise(lg.reshape(rows, stride)), margin


def table_counts(K, t):
    """c_k = sum of t_ik over the restaurants with K_i > k, k < max K"""
    c = np.zeros(int(max(K)), dtype=np.int64)
    g = 0
    for Ki in K:
        c[:Ki] += np.asarray(t[g:g + Ki], dtype=np.int64)
        g += Ki
    return c


def sample_h(K, t, gamma, seed: int, sweep: int):
    """(h_k for k < max K, smallest margin); gamma a scalar or max K values"""
    c = table_counts(K, t)
    alpha = np.broadcast_to(np.asarray(gamma, dtype=np.float64), c.shape) + c.astype(np.float64)
    lg, margin = log_gamma(alpha, cell_keys(seed, sweep, len(c)))
    e = np.exp(lg - lg.max())
    Z = e[0]
    for k in range(1, len(e)):
        Z = Z + e[k]
    return e / Z, margin


def spread_h(K, hk):
    """h_k at every pair (i, k)"""
    return np.concatenate([hk[:Ki] for Ki in K])


def loglik(cnt, lik):
    """(sum cnt log lik in the header's association, cells with a count and no likelihood)"""
    cnt = np.asarray(cnt)
    lik = np.asarray(lik, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.where(cnt > 0, cnt.astype(np.float64) * np.log(lik), 0.0)
    col = chunk_sums(x)
    tot = col[0]
    with np.errstate(invalid="ignore"):
        for k in range(1, len(col)):
            tot = tot + col[k]
    return float(tot), int(np.sum((cnt > 0) & (lik == 0.0)))


# ---- the replay cases of tests/test_gpu_tlik.py; tests/test_tlik_host.py checks every one's margin on the CPU ----

def mixed_counts(rows: int, stride: int, seed: int):
    """counts that are 0, 1, or log-uniform up to 10^4, about a third each"""
    rng = np.random.default_rng(seed)
    big = np.floor(np.exp(rng.random((rows, stride)) * math.log(1e4))).astype(np.uint32)
    kind = rng.integers(0, 3, size=(rows, stride))
    cnt = np.where(kind == 0, 0, np.where(kind == 1, 1, big)).astype(np.uint32)
    cnt.reshape(-1)[::997] = 10000
    return cnt


def mixed_beta(rows: int, seed: int):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0.02, 0.3, 0.9, 1.0, 2.5, 7.0]), size=rows)


LIK_CASES = {
    # name: (rows, stride, beta ("vec": mixed_beta), seed, sweep)
    "600x70_b0.05": (600, 70, 0.05, 1101, 0),
    "600x70_b1.5": (600, 70, 1.5, 1102, 3),
    "600x70_vec": (600, 70, "vec", 1103, 7),
    "1x1": (1, 1, 0.5, 1104, 0),
    "1x65": (1, 65, 0.5, 1105, 1),
    "256x64": (256, 64, 0.5, 1106, 2),
    "257x65": (257, 65, 0.5, 1107, 5),
}


def lik_case(name):
    """(cnt, beta, seed, sweep) of a case"""
    rows, stride, beta, seed, sweep = LIK_CASES[name]
    return mixed_counts(rows, stride, seed), (mixed_beta(rows, seed + 50) if beta == "vec" else beta), seed, sweep


# the base weights' replay: restaurants of unequal K
H_CASE = dict(K=[5, 3, 1], n=[9, 4, 0, 7, 2, 6, 1, 3, 5], t=[3, 1, 0, 7, 1, 2, 1, 3, 2],
              gamma=[0.4, 1.0, 2.5, 0.08, 1.7], seed=1201, sweep=4)
# ... and once more on the same object with a scalar prior: (gamma0, seed, sweep)
H_CASE_SCALAR = (2.0, 77, 0)
