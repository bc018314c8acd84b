"""A numpy replay of the device draw of -log q_i, q_i ~ Beta(b, N_i) (libstb_amd/csrc/hyperq.hip, include/stb_hip.h
stb_sample_logq), and the closed forms its law is checked against.  No scipy: digamma and trigamma by recurrence plus
the asymptotic series.

The draw, as the header specifies it:
  key = mix(seed + (sweep+1) gamma); key_i = mix(key + (i+1) gamma); uniform k = 1, 2, ... of restaurant i is m 2^-53, m
  the top 53 bits of mix(key_i + k gamma), with 2^-54 in place of m = 0.
  log Gamma(alpha >= 1) variate: d = alpha - 1/3, c = 1/sqrt(9 d); an attempt takes u1, u2, x = sqrt(-2 log u1) cos(2 pi u2),
  w = 1 + c x; w <= 0 ends the attempt; else v = w^3, a third uniform u, accepted when
  log u < ((x x / 2 + d) - d v) + d log v, giving log d + log v.  alpha < 1: log Gamma(alpha + 1) variate + log(u') / alpha.
  A restaurant draws shape b first, then shape N_i; D = log G_N - log G_b; L = log1p(exp D) (D <= 0), D + log1p(exp(-D)).
"""
import math

import numpy as np

GAMMA = np.uint64(0x9E3779B97F4A7C15)
CAP = 64
_M64 = (1 << 64) - 1


def mix(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def sweep_key(seed: int, sweep: int) -> np.uint64:
    return mix(np.uint64((seed + (sweep + 1) * int(GAMMA)) & _M64))


def unit(key_i, k):
    """uniform number k (array, per restaurant) of the substreams key_i, inside the open interval (0, 1)"""
    with np.errstate(over="ignore"):
        m = mix(key_i + k * GAMMA) >> np.uint64(11)
    u = m.astype(np.float64) * (1.0 / 9007199254740992.0)
    return np.where(m == 0, 1.0 / 18014398509481984.0, u)


def _f(x, dtype):
    return np.asarray(x, dtype=dtype)


def _log_gamma_ge1(alpha, key_i, k, dtype):
    """log of a Gamma(alpha >= 1) variate per lane; k (uint64 array) is advanced in place.  The transcendentals run in
    `dtype` (float64, or longdouble for the sensitivity check) and are rounded to float64 where the kernel holds a
    double; the accept test's arithmetic is float64's."""
    n = alpha.shape[0]
    out = np.full(n, np.nan)
    live = np.ones(n, dtype=bool)
    d = alpha - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    ld = np.log(_f(d, dtype)).astype(np.float64)
    for _ in range(CAP):
        idx = np.nonzero(live)[0]
        if idx.size == 0:
            break
        ki = key_i[idx]
        k[idx] += np.uint64(1)
        u1 = unit(ki, k[idx])
        k[idx] += np.uint64(1)
        u2 = unit(ki, k[idx])
        lu1 = np.log(_f(u1, dtype)).astype(np.float64)
        cs = np.cos(_f(6.283185307179586 * u2, dtype)).astype(np.float64)
        x = np.sqrt(-2.0 * lu1) * cs
        w = 1.0 + c[idx] * x
        pos = w > 0.0
        idx, x, w = idx[pos], x[pos], w[pos]
        ki = key_i[idx]
        v = w * w * w
        k[idx] += np.uint64(1)
        u = unit(ki, k[idx])
        lv = np.log(_f(v, dtype)).astype(np.float64)
        lu = np.log(_f(u, dtype)).astype(np.float64)
        di = d[idx]
        acc = lu < ((0.5 * (x * x) + di) - di * v) + di * lv
        out[idx[acc]] = ld[idx[acc]] + lv[acc]
        live[idx[acc]] = False
    return out, live.any()


def _log_gamma(alpha, key_i, k, dtype):
    small = alpha < 1.0
    lg, bad = _log_gamma_ge1(np.where(small, alpha + 1.0, alpha), key_i, k, dtype)
    if small.any():
        idx = np.nonzero(small)[0]
        k[idx] += np.uint64(1)
        u = unit(key_i[idx], k[idx])
        lg[idx] = lg[idx] + np.log(_f(u, dtype)).astype(np.float64) / alpha[idx]
    return lg, bad


def replay_L(b: float, N, seed: int, sweep: int, dtype=np.float64, first: int = 0):
    """L_i = -log q_i for restaurants first .. first + len(N) - 1 (0 where N_i = 0); raises if a loop ran out"""
    N = np.asarray(N, dtype=np.uint64)
    n = N.shape[0]
    key = sweep_key(seed, sweep)
    with np.errstate(over="ignore"):
        key_i = mix(key + (np.arange(first, first + n, dtype=np.uint64) + np.uint64(1)) * GAMMA)
    L = np.zeros(n)
    idx = np.nonzero(N > 0)[0]
    if idx.size == 0:
        return L
    ki = key_i[idx]
    k = np.zeros(idx.size, dtype=np.uint64)
    lgb, bad1 = _log_gamma(np.full(idx.size, float(b)), ki, k, dtype)
    lgn, bad2 = _log_gamma(N[idx].astype(np.float64), ki, k, dtype)
    if bad1 or bad2:
        raise RuntimeError("a Gamma draw was not accepted within %d attempts" % CAP)
    D = lgn - lgb
    Dx = _f(D, dtype)
    with np.errstate(over="ignore"):
        Lpos = D + np.log1p(np.exp(-Dx)).astype(np.float64)
        Lneg = np.log1p(np.exp(np.minimum(Dx, 0))).astype(np.float64)
    L[idx] = np.where(D > 0.0, Lpos, Lneg)
    return L


def mixed_restaurants(I: int):
    """the restaurants of the device replay test: N = 0, N = 1, N up to 10^7, in a fixed pattern"""
    from libstb_amd import synth

    u = synth.unit(I, 4242)
    N = np.floor(np.exp(u * math.log(1e7))).astype(np.uint32)  # log-uniform on [1, 10^7)
    N[::7] = 0
    N[1::7] = 1
    N[2::1001] = 10 ** 7
    return N


# ---- closed forms: E L = psi(b + N) - psi(b), Var L = psi'(b) - psi'(b + N) for q ~ Beta(b, N), L = -log q

def digamma(x: float) -> float:
    s = 0.0
    while x < 12.0:
        s -= 1.0 / x
        x += 1.0
    i2 = 1.0 / (x * x)
    return s + math.log(x) - 0.5 / x - i2 * (1.0 / 12 - i2 * (1.0 / 120 - i2 * (1.0 / 252 - i2 * (1.0 / 240 - i2 / 132))))


def trigamma(x: float) -> float:
    s = 0.0
    while x < 12.0:
        s += 1.0 / (x * x)
        x += 1.0
    i2 = 1.0 / (x * x)
    return s + 1.0 / x + 0.5 * i2 + (1.0 / x) * i2 * (1.0 / 6 - i2 * (1.0 / 30 - i2 * (1.0 / 42 - i2 * (1.0 / 30 - i2 * 5.0 / 66))))


def mean_L(b: float, N: float) -> float:
    return digamma(b + N) - digamma(b)


def var_L(b: float, N: float) -> float:
    return trigamma(b) - trigamma(b + N)


def moment_check(L, b: float, N: float, sigmas: float = 5.0):
    """(ok, text): the sample mean within `sigmas` exact standard errors of psi(b+N) - psi(b); the sample variance
    within `sigmas` standard errors -- from the sample's own fourth moment -- of psi'(b) - psi'(b+N)"""
    L = np.asarray(L, dtype=np.float64)
    n = L.shape[0]
    m, v = mean_L(b, N), var_L(b, N)
    xm = float(L.mean())
    se_m = math.sqrt(v / n)
    dev = L - xm
    s2 = float((dev * dev).sum() / (n - 1))
    m4 = float((dev ** 4).mean())
    se_v = math.sqrt(max(m4 - s2 * s2 * (n - 3) / (n - 1), 0.0) / n)
    zm = (xm - m) / se_m
    zv = (s2 - v) / se_v if se_v > 0 else (0.0 if s2 == v else math.inf)
    text = "b=%g N=%g n=%d: mean %.9g (exact %.9g, z=%+.2f)  var %.9g (exact %.9g, z=%+.2f)" % (b, N, n, xm, m, zm, s2, v, zv)
    return abs(zm) <= sigmas and abs(zv) <= sigmas, text


def ks_stat(p) -> float:
    """sqrt(n) D for values p that are uniform on (0, 1) under the hypothesis"""
    p = np.sort(np.asarray(p, dtype=np.float64))
    n = p.shape[0]
    i = np.arange(1, n + 1, dtype=np.float64)
    D = max(float((i / n - p).max()), float((p - (i - 1) / n).max()))
    return math.sqrt(n) * D
