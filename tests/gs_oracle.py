"""A numpy replay of the Gaussian-observation steps (libstb_amd/csrc/gauss.hip), written from the text of include/stb_hip.h,
"Gaussian observations": the dishes' statistics in the header's chunk association, the Normal-Gamma draw from the
counter-based uniforms, the matrix of densities, the data term and the collapsed evidence -- and the 40-digit mpmath truth
of the two totals, with the bars their own operations give them.

  Sums over the customers of a dish: chunks of 256 customers by flat index; a chunk's members one after another in customer
  order starting from the first member; chunks without members skipped; the partials in chunk order in double-double
  (dd_add below: TwoSum on the high word), the result hi + lo.
  Pass A: n_k, S_kd, mean = S / n.  Pass B: Q = sum (x - mean)(x - mean).  n_k = 0: +0.0.
  Draw: key_e = mix(key + (e+1) gamma), e = k D + d; log Gamma(alpha_n) by tl_oracle's recipe; tau = exp(lg - log beta_n);
  the next two uniforms u1, u2; mu = m_n + sqrt(-2 log u1) cos(2 pi u2) / sqrt(kappa_n tau).
  Matrix: H_k = sum_d 0.5 log tau, q = sum_d ((x - mu)(x - mu)) tau, both in d order from the d = 0 term;
  l = H - 0.5 q; the row is exp(l - max l), zeros where the maximum is not finite.
  Totals: blocks of 256 terms by the block tree (x[l] + x[l+64]) + (x[l+128] + x[l+192]), then the shuffle tree 32 .. 1;
  the block sums in order in double-double.

u = 2^-53 below.  Every bar is one rounding (u relative) per floating-point operation, E_LOG roundings per log and E_LGAMMA
per lgamma (the device's libm is not correctly rounded; lgamma relative to max(|value|, 1)), propagated to first order.
Nothing is fitted to what the code returns.
"""
import math

import numpy as np

import hq_oracle as hqo
import tl_oracle as tlo

CHUNK = 256
BLOCK = 256
U = 2.0 ** -53
E_LOG = 2.0
E_LGAMMA = 4.0
LOG_2PI = 1.8378770664093453
HALF_LOG_2PI = 0.9189385332046727


def prior(kappa0, alpha0, beta0, D, m0=None):
    """the prior as a dict of FP64 values: beta0 a scalar or D values, m0 None (zeros) or D values"""
    return dict(kappa0=float(kappa0), alpha0=float(alpha0),
                beta0=np.broadcast_to(np.asarray(beta0, dtype=np.float64), (D,)).copy(),
                m0=np.zeros(D) if m0 is None else np.asarray(m0, dtype=np.float64).copy())


# ---- sums ----

def dd_add(hi, lo, x):
    """stb_common.h's dd_add on arrays (or scalars): (hi, lo) + x"""
    with np.errstate(invalid="ignore", over="ignore"):
        t = hi + x
        bb = t - hi
        corr = (hi - (t - bb)) + (x - bb)
    lo = lo + np.where(np.isfinite(t), corr, 0.0)
    return t, lo


def dish_sums(v, cust, K):
    """(sum over the members of every dish of the rows of v (C, D), in the header's association; n_k)"""
    v = np.asarray(v, dtype=np.float64)
    cust = np.asarray(cust).astype(np.int64)
    C, D = v.shape
    out = np.zeros((K, D))
    n = np.zeros(K, dtype=np.int64)
    for k in range(K):
        idx = np.nonzero(cust == k)[0]
        n[k] = idx.size
        if idx.size == 0:
            continue
        ch = idx // CHUNK
        chunks, first, counts = np.unique(ch, return_index=True, return_counts=True)
        rank = np.arange(idx.size) - np.repeat(first, counts)
        slot = np.repeat(np.arange(chunks.size), counts)
        part = v[idx[rank == 0]].copy()  # every listed chunk has a first member, in chunk order
        for r in range(1, int(counts.max())):
            sel = rank == r
            part[slot[sel]] = part[slot[sel]] + v[idx[sel]]
        hi, lo = np.zeros(D), np.zeros(D)
        for j in range(chunks.size):
            hi, lo = dd_add(hi, lo, part[j])
        out[k] = hi + lo
    return out, n


def stats(x, cust, K):
    """(n (K) int64, mean (K, D), Q (K, D), skipped) by the two passes"""
    x = np.asarray(x, dtype=np.float64)
    cust = np.asarray(cust).astype(np.int64)
    D = x.shape[1]
    S, n = dish_sums(x, cust, K)
    mean = np.zeros((K, D))
    has = n > 0
    mean[has] = S[has] / n[has].astype(np.float64)[:, None]
    inside = cust < K
    dev = np.zeros_like(x)
    dev[inside] = x[inside] - mean[cust[inside]]
    Q, _ = dish_sums(dev * dev, cust, K)
    Q[~has] = 0.0
    return n, mean, Q, int((~inside).sum())


def one_pass_Q(x, cust, K):
    """the tempting wrong step: sum x^2 - n xbar^2, the sums in the same association"""
    x = np.asarray(x, dtype=np.float64)
    S, n = dish_sums(x, cust, K)
    S2, _ = dish_sums(x * x, cust, K)
    nn = np.maximum(n, 1).astype(np.float64)[:, None]
    xbar = S / nn
    return S2 - nn * (xbar * xbar)


# ---- the draw ----

def posterior(n, mean, Q, pr):
    """(kappa_n, m_n, alpha_n, beta_n), each (K, D), in the header's operation order; the prior's own for n_k = 0"""
    n = np.asarray(n).astype(np.int64)
    K, D = mean.shape
    k0, a0, b0, m0 = pr["kappa0"], pr["alpha0"], pr["beta0"][None, :], pr["m0"][None, :]
    nn = n.astype(np.float64)[:, None]
    dm = mean - m0
    kn = k0 + nn
    mn = (k0 * m0 + nn * mean) / kn
    an = a0 + 0.5 * nn
    bn = (b0 + 0.5 * Q) + 0.5 * (((k0 * nn) / kn) * (dm * dm))
    empty = np.broadcast_to((n == 0)[:, None], (K, D))
    kn = np.where(empty, k0, np.broadcast_to(kn, (K, D)))
    mn = np.where(empty, np.broadcast_to(m0, (K, D)), mn)
    an = np.where(empty, a0, np.broadcast_to(an, (K, D)))
    bn = np.where(empty, np.broadcast_to(b0, (K, D)), bn)
    return kn, mn, an, bn


def log_gamma_counted(alpha, key_e):
    """tl_oracle.log_gamma with the number of uniforms every cell took: (log G, count, smallest margin)"""
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
    return out, k, margin


def draw(n, mean, Q, pr, seed: int, sweep: int):
    """(mu (K, D), tau (K, D), smallest acceptance margin)"""
    K, D = mean.shape
    kn, mn, an, bn = posterior(n, mean, Q, pr)
    keys = tlo.cell_keys(seed, sweep, K * D)
    lg, k, margin = log_gamma_counted(an.reshape(-1), keys)
    lt = lg - np.log(bn.reshape(-1))
    tau = np.exp(lt)
    u1 = hqo.unit(keys, k + np.uint64(1))
    u2 = hqo.unit(keys, k + np.uint64(2))
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)
    mu = mn.reshape(-1) + z / np.sqrt(kn.reshape(-1) * tau)
    return mu.reshape(K, D), tau.reshape(K, D), margin


# ---- the matrix ----

def dish_H(tau):
    hl = 0.5 * np.log(tau)
    H = hl[:, 0].copy()
    for d in range(1, tau.shape[1]):
        H = H + hl[:, d]
    return H


def log_density(x, mu, tau):
    """l (C, K) = H_k - 0.5 q_ck"""
    x, mu, tau = (np.asarray(v, dtype=np.float64) for v in (x, mu, tau))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        H = dish_H(tau)
        q = None
        for d in range(x.shape[1]):
            t = x[:, d, None] - mu[None, :, d]
            s = (t * t) * tau[None, :, d]
            q = s if q is None else q + s
        return H[None, :] - 0.5 * q


def lik(x, mu, tau, stride=None):
    """(the matrix (C, stride), dead rows)"""
    l = log_density(x, mu, tau)
    C, K = l.shape
    stride = K if stride is None else stride
    out = np.zeros((C, stride))
    if C == 0:
        return out, 0
    with np.errstate(invalid="ignore"):
        m = np.where(np.isnan(l), -np.inf, l).max(axis=1)
        dead = ~np.isfinite(m)
        out[:, :K] = np.exp(l - np.where(dead, 0.0, m)[:, None])
    out[dead] = 0.0
    return out, int(dead.sum())


# ---- the totals ----

def block_total(v):
    """the terms v in blocks of 256 by the block tree, the block sums in order in double-double: hi + lo"""
    v = np.asarray(v, dtype=np.float64)
    nblk = (v.size + BLOCK - 1) // BLOCK
    if nblk == 0:
        return 0.0
    p = np.zeros(nblk * BLOCK)
    p[:v.size] = v
    p = p.reshape(nblk, 4, 64)
    with np.errstate(invalid="ignore"):
        a = (p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3])
        off = 32
        while off >= 1:
            a = a[:, :off] + a[:, off:2 * off]
            off //= 2
    hi, lo = 0.0, 0.0
    for b in range(nblk):
        hi, lo = dd_add(hi, lo, a[b, 0])
    return float(hi + lo)


def loglik(x, cust, mu, tau):
    """(log p(x | z, mu, tau), skipped)"""
    x = np.asarray(x, dtype=np.float64)
    cust = np.asarray(cust).astype(np.int64)
    C, D = x.shape
    K = mu.shape[0]
    inside = cust < K
    v = np.zeros(C)
    if inside.any():
        l = log_density(x[inside], mu, tau)
        v[inside] = l[np.arange(l.shape[0]), cust[inside]]
    return block_total(v) + float(C * D) * (-HALF_LOG_2PI), int((~inside).sum())


def logml_cells(n, mean, Q, pr):
    n = np.asarray(n).astype(np.int64)
    K, D = mean.shape
    kn, mn, an, bn = posterior(n, mean, Q, pr)
    out = np.zeros((K, D))
    lg = np.vectorize(math.lgamma)
    a0, k0 = pr["alpha0"], pr["kappa0"]
    for k in range(K):
        if n[k] == 0:
            continue
        out[k] = ((((lg(an[k]) - math.lgamma(a0)) + a0 * np.log(pr["beta0"])) - an[k] * np.log(bn[k]))
                  + 0.5 * (math.log(k0) - np.log(kn[k]))) - (0.5 * float(n[k])) * LOG_2PI
    return out


def logml(n, mean, Q, pr):
    return block_total(logml_cells(n, mean, Q, pr).reshape(-1))


# ---- the truth ----

def _mp():
    import mpmath

    mpmath.mp.dps = 40
    return mpmath


def mp_stats(members):
    """(n, mean, Q) of one dish's one dimension in 40 digits"""
    mp = _mp()
    xs = [mp.mpf(float(v)) for v in members]
    n = len(xs)
    if n == 0:
        return 0, mp.mpf(0), mp.mpf(0)
    mean = mp.fsum(xs) / n
    return n, mean, mp.fsum((v - mean) ** 2 for v in xs)


def mp_logml_cell(n, mean, Q, k0, a0, b0, m0):
    """log p(x_1..n) of one (dish, dimension) under the Normal-Gamma prior, from its statistics, in 40 digits"""
    mp = _mp()
    if n == 0:
        return mp.mpf(0)
    n_, mean, Q, k0, a0, b0, m0 = mp.mpf(n), mp.mpf(mean), mp.mpf(Q), mp.mpf(k0), mp.mpf(a0), mp.mpf(b0), mp.mpf(m0)
    kn = k0 + n_
    an = a0 + n_ / 2
    bn = b0 + Q / 2 + k0 * n_ * (mean - m0) ** 2 / (2 * kn)
    return (mp.loggamma(an) - mp.loggamma(a0) + a0 * mp.log(b0) - an * mp.log(bn) + (mp.log(k0) - mp.log(kn)) / 2
            - n_ / 2 * mp.log(2 * mp.pi))


def mp_logml(n, mean, Q, pr):
    """the evidence from the FP64 statistics (n, mean, Q) as given, in 40 digits"""
    mp = _mp()
    K, D = mean.shape
    return mp.fsum(mp_logml_cell(int(n[k]), float(mean[k, d]), float(Q[k, d]), pr["kappa0"], pr["alpha0"],
                                 float(pr["beta0"][d]), float(pr["m0"][d])) for k in range(K) for d in range(D))


def mp_loglik(x, cust, mu, tau):
    mp = _mp()
    K = mu.shape[0]
    tot = mp.mpf(0)
    for c in range(x.shape[0]):
        k = int(cust[c])
        if k >= K:
            continue
        for d in range(x.shape[1]):
            t = mp.mpf(float(tau[k, d]))
            tot += mp.log(t) / 2 - (mp.mpf(float(x[c, d])) - mp.mpf(float(mu[k, d]))) ** 2 * t / 2
    return tot - mp.mpf(x.shape[0] * x.shape[1]) * mp.log(2 * mp.pi) / 2


# ---- the bars ----

def Q_bar(members, mean):
    """the two-pass Q of n members: every term (x - mean)^2 carries one rounding for the subtraction and one for the product
    (3 u relative to first order), the n - 1 additions one each on a running sum of at most Q (the double-double across
    chunks adds u^2 terms: the final hi + lo is one more rounding), and the rounded mean shifts Q by n delta^2 exactly, the
    cross term vanishing around the true mean: delta <= u |mean| (min(n, 256) + 2), a chunk's sequential additions, hi + lo
    and the division"""
    x = np.asarray(members, dtype=np.float64)
    n = x.size
    Q = float(((x - mean) ** 2).sum())
    delta = U * abs(mean) * (min(n, CHUNK) + 2.0)
    return (3.0 + n) * U * Q + n * delta * delta


def loglik_bar(x, cust, mu, tau):
    """v_c: H_k carries E_LOG + 1 roundings a term and D - 1 additions on sum_d |0.5 log tau|; q's terms three roundings each
    and D - 1 additions of non-negative terms; l one more on |H| + 0.5 q.  The block tree is 8 additions deep on sum |v|,
    the double-double is exact to u^2, and hi + lo, the constant's product and its addition are one rounding each"""
    x = np.asarray(x, dtype=np.float64)
    cust = np.asarray(cust).astype(np.int64)
    C, D = x.shape
    K = mu.shape[0]
    inside = cust < K
    habs = np.abs(0.5 * np.log(tau)).sum(axis=1)
    k = cust[inside]
    q = (((x[inside] - mu[k]) ** 2) * tau[k]).sum(axis=1)
    per = (E_LOG + 1.0 + D) * U * habs[k] + (3.0 + D) * U * 0.5 * q + U * (habs[k] + 0.5 * q)
    mag = float((habs[k] + 0.5 * q).sum())
    const = C * D * HALF_LOG_2PI
    return float(per.sum()) + 8.0 * U * mag + 2.0 * U * (mag + const) + U * const


def logml_bar(n, mean, Q, pr):
    """a cell: lgamma E_LGAMMA roundings relative to max(|value|, 1), twice; alpha_n one rounding, which lgamma turns into
    u alpha_n |digamma(alpha_n)| <= u alpha_n (|log alpha_n| + 1 / alpha_n); beta_n eight roundings relative (its terms are
    non-negative), so log beta_n moves by 8 u and carries E_LOG more; the products one each; five left-to-right additions on
    at most the sum of the terms' magnitudes.  The block tree is 8 additions deep, hi + lo one rounding"""
    n = np.asarray(n).astype(np.int64)
    K, D = mean.shape
    kn, mn, an, bn = posterior(n, mean, Q, pr)
    a0, k0 = pr["alpha0"], pr["kappa0"]
    lg = np.vectorize(math.lgamma)
    bar, mag = 0.0, 0.0
    for k in range(K):
        if n[k] == 0:
            continue
        t1, t2 = np.abs(lg(an[k])), abs(math.lgamma(a0))
        t3 = np.abs(a0 * np.log(pr["beta0"]))
        t4 = np.abs(an[k] * np.log(bn[k]))
        t5 = 0.5 * (abs(math.log(k0)) + np.abs(np.log(kn[k])))
        t6 = 0.5 * n[k] * LOG_2PI
        terms = t1 + t2 + t3 + t4 + t5 + t6
        cell = (E_LGAMMA * (np.maximum(t1, 1.0) + max(t2, 1.0)) + an[k] * (np.abs(np.log(an[k])) + 1.0 / an[k])
                + (E_LOG + 1.0) * t3 + an[k] * (8.0 + E_LOG) + 2.0 * t4 + (E_LOG + 2.0) * t5 + 0.5 + 2.0 * t6 + 5.0 * terms)
        bar += float(cell.sum()) * U
        mag += float(terms.sum())
    return bar + 9.0 * U * mag


# ---- the tiny chain: 2 restaurants x 3 customers x 2 dishes, D = 1, against the enumerated p(z | x) ----

CHAIN = dict(I=2, Nc=3, K=2, a=0.3, b=1.0, x=(-1.1, -0.6, 0.9, 1.2, 0.7, -0.8), burn=20, thin=2)
# (prior, iterations) under which each wrong variant below is told from the right law; the right law holds under both
CHAIN_PRIORS = {"weak": ((0.5, 1.5, 1.0), 2020), "strong": ((4.0, 1.5, 1.0), 3020)}
CHAIN_WRONG = {"variance": "weak", "uncentred": "weak", "no_kappa": "strong", "stale": "strong"}
CHAIN_SEED = 9100


def chain_x():
    return np.array(CHAIN["x"]).reshape(-1, 1)


def chain_cell(z):
    """the partition of the six customers: exchanging the two dishes' names, between whose images the chain passes only
    rarely, leaves it as it is"""
    z = np.asarray(z).astype(np.int64)
    return tuple(int(v) for v in (z ^ z[0]))


def chain_exact(pr):
    """p(partition | x): the PYP prior of (z, t) with h = 1/2, summed over t, times the evidence"""
    import td_oracle as tdo
    import ti_oracle as tio

    Nc, K, a, b = (CHAIN[k] for k in ("Nc", "K", "a", "b"))
    one = tdo.states(Nc, K)
    S = {m: tio.stirling(m, a) for m in range(1, Nc + 1)}
    x, acc = chain_x(), {}
    for s0 in one:
        for s1 in one:
            v = 1.0
            for z, ts in (s0, s1):
                v *= float(np.prod([b + j * a for j in range(sum(ts))]))
                for nk, tk in zip(tdo.counts(z, K), ts):
                    if nk:
                        v *= S[nk][tk] * 0.5 ** tk
            z = np.array(s0[0] + s1[0])
            n, mean, Q, _ = stats(x, z, K)
            v *= math.exp(logml(n, mean, Q, pr))
            acc[chain_cell(z)] = acc.get(chain_cell(z), 0.0) + v
    tot = sum(acc.values())
    return {k: v / tot for k, v in acc.items()}


def chain_run(law, pr, iterations, seed=CHAIN_SEED):
    """(the kept partitions, the smallest acceptance margin of the draws): redraw (mu, tau), rewrite the matrix, one dish
    sweep of td_oracle under it.  law: "right", or a wrong variant -- "variance" tau read as a variance by the matrix,
    "no_kappa" kappa_n left out of mu's spread, "uncentred" Q = sum x^2, "stale" the first matrix never rewritten"""
    import td_oracle as tdo
    import ti_oracle as tio

    I, Nc, K, a, b = (CHAIN[k] for k in ("I", "Nc", "K", "a", "b"))
    x = chain_x()
    vt = tio.ExactV(list(range(1, Nc + 1)), a, Nc)
    Ks, bpar, h = np.full(I, K), np.full(I, b), np.full(I * K, 0.5)
    cust = np.array([0, 1, 0, 1, 0, 1])
    n = np.concatenate([tdo.counts(cust[:Nc], K), tdo.counts(cust[Nc:], K)]).astype(np.uint32)
    t = (n > 0).astype(np.uint16)
    kept, worst, first = [], math.inf, None
    for s in range(iterations):
        nn, mean, Q, _ = stats(x, cust, K)
        if law == "uncentred":
            Q = dish_sums(x * x, cust, K)[0]
        mu, tau, margin = draw(nn, mean, Q, pr, seed + 1, s)
        worst = min(worst, margin)
        if law == "no_kappa":
            kn, mn, _, _ = posterior(nn, mean, Q, pr)
            mu = mn + (mu - mn) * np.sqrt(kn)
        L, _ = lik(x, mu, 1.0 / tau if law == "variance" else tau)
        first = L if first is None else first
        n, t, _, cust, _, _ = tdo.sweep(Ks, n, t, h, a, bpar, vt, Nc, Nc, seed, s, cust, np.arange(I * Nc),
                                        first if law == "stale" else L)
        if s >= CHAIN["burn"] and s % CHAIN["thin"] == 0:
            kept.append(chain_cell(cust))
    return kept, worst
