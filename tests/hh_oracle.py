"""A numpy replay of the grouped base-weight step (libstb_amd/csrc/hgroups.hip; include/stb_hip.h stb_sample_hgroups),
written from the header's text on tl_oracle's log-Gamma variates and normalisation and hb_oracle's y stream and step, and
the law the root is checked against.

  key = mix(seed + (sweep+1) gamma); cell e = g Kmax + k owns key_e = mix(key + (e+1) gamma).
  c_gk   tables of group g at dish k;  w = alpha r_k
  m_gk   [c_gk >= 1] + sum_{j=1}^{c_gk-1} [u_j (w + j) < w], u_j element j of mix(key_e ^ SALT_Y): hb_oracle.replay_Y with
         a = 1, a "restaurant" per cell (b = w, T = c_gk) -- j * 1.0 is exact, so the comparison is the header's
  r'     Dirichlet(gamma_k + s_k), s_k = sum_g m_gk, root cell k on mix(mix(key ^ SALT_R) + (k+1) gamma)
  alpha' hb_oracle.replay (a = 0, one group of G "restaurants" with N = C_g, T = M_g, b = alpha) on seed ^ SALT_A
  h_g    Dirichlet(alpha' r'_k + c_gk) on key_e
Every Dirichlet: lg_k the log-Gamma variate, M the largest, e_k = exp(lg_k - M), Z the e_k added in k order, e_k / Z.
The replay reports the smallest margin of the Gamma acceptance tests (as tl_oracle does) and of the Bernoulli comparisons.
"""
import math

import numpy as np

import hb_oracle as hbo
import hq_oracle as hqo
import tl_oracle as tlo

SALT_R = np.uint64(0x6A09E667F3BCC909)
SALT_A = 0xA54FF53A5F1D36F1
KEEP_ROOT, SAMPLE_ALPHA = 1, 2
LAWS = ("right", "no_first", "no_j")   # the step, and two wrong ones: the [c >= 1] table dropped; a constant w / (w + 1)
_HB_LAW = {"right": "right", "no_first": "no_first", "no_j": "no_k"}


def group_counts(K, t, goff, Kmax=None):
    """c[G, Kmax]: the tables of every group at every dish (goff None: a group a restaurant)"""
    K = np.asarray(K, dtype=np.int64)
    I = len(K)
    Kmax = int(K.max()) if Kmax is None else Kmax
    goff = np.arange(I + 1) if goff is None else np.asarray(goff, dtype=np.int64)
    G = len(goff) - 1
    owner = np.searchsorted(goff, np.arange(I), side="right") - 1      # the last range that starts at or before i
    owner = np.minimum(owner, G - 1)
    c = np.zeros((G, Kmax), dtype=np.int64)
    koff = np.concatenate([[0], np.cumsum(K)])
    rest = np.repeat(np.arange(I), K)
    k = np.arange(int(koff[-1])) - koff[rest]
    np.add.at(c, (owner[rest], k), np.asarray(t, dtype=np.int64))
    return c, owner


def aux_tables(c, w, seed, sweep, law="right"):
    """(m[G, Kmax], smallest relative margin of a Bernoulli comparison); w[Kmax] = alpha r"""
    G, Kmax = c.shape
    my = [math.inf]
    wf = np.broadcast_to(np.asarray(w, dtype=np.float64), (G, Kmax)).reshape(-1)
    m = hbo.replay_Y(1.0, wf, c.reshape(-1), seed, sweep, _HB_LAW[law], my)
    return m.astype(np.int64).reshape(G, Kmax), my[0]


def dirichlet_rows(shape, keys):
    """(rows normalised as the header says, smallest margin); shape[rows, Kmax], keys flat.  A shape of exactly 0 (an
    underflowed base weight under no count) takes no uniform: its coordinate is 0"""
    rows, Kmax = shape.shape
    flat = shape.reshape(-1)
    pos = flat != 0.0
    lg = np.full(flat.shape, -np.inf)
    lg[pos], margin = tlo.log_gamma(flat[pos], np.asarray(keys)[pos])
    lg = lg.reshape(rows, Kmax)
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    Z = e[:, 0].copy()
    for k in range(1, Kmax):
        Z = Z + e[:, k]
    return e / Z[:, None], margin


def root_keys(seed, sweep, Kmax):
    keyR = hqo.mix(hqo.sweep_key(seed, sweep) ^ SALT_R)
    with np.errstate(over="ignore"):
        return hqo.mix(keyR + (np.arange(Kmax, dtype=np.uint64) + np.uint64(1)) * hqo.GAMMA)


def draw_root(s, gamma, seed, sweep):
    shape = np.broadcast_to(np.asarray(gamma, dtype=np.float64), s.shape) + s.astype(np.float64)
    r, margin = dirichlet_rows(shape.reshape(1, -1), root_keys(seed, sweep, len(s)))
    return r[0], margin


def draw_alpha(alpha, C, M, shape, scale, seed, sweep):
    """(alpha', hb_oracle.replay's dict)"""
    G = len(C)
    out = hbo.replay(0.0, shape, scale, np.asarray(M, dtype=np.uint32), np.asarray(C, dtype=np.uint32), np.full(G, float(alpha)),
                     np.array([0, G], dtype=np.int64), (seed ^ SALT_A) & ((1 << 64) - 1), sweep)
    return float(out["bgrp"][0]), out


def draw_groups(c, root, alpha, seed, sweep):
    """(hgrp[G, Kmax], smallest margin)"""
    G, Kmax = c.shape
    shape = (alpha * np.asarray(root, dtype=np.float64))[None, :] + c.astype(np.float64)
    return dirichlet_rows(shape, tlo.cell_keys(seed, sweep, G * Kmax))


def spread(K, owner, hgrp):
    """the groups' weights at every pair (i, k)"""
    return np.concatenate([hgrp[g, :Ki] for Ki, g in zip(K, owner)])


def replay(K, t, goff, root, alpha, gamma, seed, sweep, flags=0, shape=1.0, scale=1.0, law="right", Kmax=None,
           root_new=None, alpha_new=None):
    """the whole step: dict with c, m, tables, aux_tables, root (r'), alpha (alpha'), hgrp, h, margin_gamma, margin_y.
    root_new / alpha_new, when given, replace the replay's own r' / alpha' in the group draw (a device's values)"""
    c, owner = group_counts(K, t, goff, Kmax)
    root = np.asarray(root, dtype=np.float64)
    m, my = aux_tables(c, alpha * root, seed, sweep, law)
    mg = math.inf
    r1 = root
    if not flags & KEEP_ROOT:
        r1, mr = draw_root(m.sum(axis=0), gamma, seed, sweep)
        mg = min(mg, mr)
    a1 = float(alpha)
    if flags & SAMPLE_ALPHA:
        a1, hb = draw_alpha(alpha, c.sum(axis=1), m.sum(axis=1), shape, scale, seed, sweep)
        mg, my = min(mg, hb["margin_gamma"]), min(my, hb["margin_y"])
    hgrp, mh = draw_groups(c, r1 if root_new is None else root_new, a1 if alpha_new is None else alpha_new, seed, sweep)
    return dict(c=c, m=m, tables=int(c.sum()), aux_tables=int(m.sum()), root=r1, alpha=a1, hgrp=hgrp, owner=owner,
                h=spread(K, owner, hgrp), margin_gamma=min(mg, mh), margin_y=my)


# ---- the law of the root for two dishes: p(r | c) ~ Dir(r; gamma) prod_gk Gamma(alpha r_k + c_gk) / Gamma(alpha r_k)

_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


class RootPosterior:
    """r_0's posterior for K = 2 by quadrature in x = logit r_0 (trapezoid on a fine grid), with its CDF"""

    def __init__(self, c, alpha, gamma, points=80001):
        c = np.asarray(c, dtype=np.int64)
        x = np.linspace(-45.0, 45.0, points)
        l0, l1 = -np.logaddexp(0.0, -x), -np.logaddexp(0.0, x)     # log r_0, log r_1
        lp = gamma[0] * l0 + gamma[1] * l1                          # (the Jacobian r_0 r_1 turns gamma - 1 into gamma)
        for k, lr in ((0, l0), (1, l1)):
            w = alpha * np.exp(lr)
            for cg in c[:, k]:
                for j in range(int(cg)):                            # Gamma(w + c) / Gamma(w) = prod_j (w + j)
                    lp = lp + np.log(w + j)
        lp -= lp.max()
        dens = np.exp(lp)
        cdf = np.concatenate([[0.0], np.cumsum(0.5 * (dens[1:] + dens[:-1]) * np.diff(x))])
        self.x, self.cdf = x, cdf / cdf[-1]

    def F(self, r0):
        r0 = np.asarray(r0, dtype=np.float64)
        return np.interp(np.log(r0) - np.log1p(-r0), self.x, self.cdf)


# the fixture of the law tests: K = 2 dishes, G = 3 groups
LAW_C = np.array([[5, 1], [0, 9], [2, 2]], dtype=np.int64)
LAW_ALPHA = 3.0
LAW_GAMMA = np.array([0.7, 1.3])
LAW_SEED = 8801            # test_hgroups_host checks this seed's chain on the CPU; test_gpu_hgroups runs it on the device
LAW_STEPS, LAW_BURN, LAW_THIN = 10000, 100, 5


def law_object():
    """(K, n, t, goff) of restaurants whose group counts are LAW_C: one restaurant a group"""
    K = np.full(3, 2, dtype=np.int32)
    t = LAW_C.reshape(-1).astype(np.uint16)
    return K, t.astype(np.uint32), t, np.arange(4, dtype=np.uint64)


def root_chain(seed, law="right", steps=LAW_STEPS, burn=LAW_BURN, thin=LAW_THIN, step_fn=None):
    """r_0 of steps 2-3 iterated on the fixture from r = (1/2, 1/2), sweeps 0, 1, ...: the kept values (after `burn`, every
    `thin`-th).  step_fn(root, sweep) -> r' replaces the replay (the device)"""
    r = np.array([0.5, 0.5])
    kept = []
    for s in range(burn + steps):
        if step_fn is None:
            m, _ = aux_tables(LAW_C, LAW_ALPHA * r, seed, s, law)
            r, _ = draw_root(m.sum(axis=0), LAW_GAMMA, seed, s)
        else:
            r = step_fn(r, s)
        if s >= burn and (s - burn) % thin == 0:
            kept.append(r[0])
    return np.array(kept)


def law_pvalue(r0):
    return hbo.ks_pvalue(RootPosterior(LAW_C, LAW_ALPHA, LAW_GAMMA).F(r0))


# ---- the exact Antoniak pmf: P(m | c, w) = |s(c, m)| w^m / (w)_c, |s| the unsigned Stirling numbers of the first kind

def antoniak_pmf(c: int, w: float):
    s = [1]                                        # |s(0, 0)|
    for n in range(c):                             # |s(n+1, m)| = n |s(n, m)| + |s(n, m-1)|
        s = [(n * s[m] if m < len(s) else 0) + (s[m - 1] if m >= 1 else 0) for m in range(len(s) + 1)]
    rising = math.prod(w + j for j in range(c))
    return np.array([s[m] * w ** m / rising for m in range(c + 1)])


# ---- the replay cases of tests/test_gpu_hgroups.py; tests/test_hgroups_host.py checks every one's margins on the CPU ----

REPLAY_I = 3000
REPLAY_K = (1, 2, 63, 64, 65, 130)
RANGE_SIZES = (1, 255, 256, 257, 513, 0, 8)      # then the rest; the range of 8 holds only t = 0
CASES = {
    # name: (grouping, Kmax (0: the ragged K), flags, seed, sweep)
    "ragged_full": ("ragged", 0, SAMPLE_ALPHA, 9101, 3),
    "ragged_keep": ("ragged", 0, KEEP_ROOT, 9102, 0),
    "each_keep": ("each", 0, KEEP_ROOT, 9103, 7),
    "k1024_alpha": ("ragged", 1024, KEEP_ROOT | SAMPLE_ALPHA, 9104, 1),
}
CASE_PRIOR = (2.0, 4.0)                          # shape, scale of the concentration


def case(name):
    """dict(K, t, goff, root, alpha, gamma, flags, seed, sweep, shape, scale): alpha r_k >= 0.5 and gamma >= 0.5"""
    grouping, Kmax, flags, seed, sweep = CASES[name]
    rng = np.random.default_rng(seed)
    I = REPLAY_I
    if Kmax:
        K = np.where(np.arange(I) % 500 == 0, Kmax, np.array((1, 2, 5))[np.arange(I) % 3]).astype(np.int32)
    else:
        K = np.array(REPLAY_K, dtype=np.int32)[(np.arange(I) * 7 + 3) % len(REPLAY_K)]
        Kmax = int(K.max())
    P = int(K.sum())
    t = rng.choice(np.array([0, 1, 2, 3, 40], dtype=np.uint16), size=P)
    sizes = list(RANGE_SIZES)
    sizes.append(I - sum(sizes))
    goff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    koff = np.concatenate([[0], np.cumsum(K)])
    e0 = int(goff[6])
    t[koff[e0]:koff[e0 + 8]] = 0
    # the range of one restaurant: c_gk = t, on both sides of 257 (a wave takes a cell with c_gk > 257)
    t[:koff[1]] = np.resize(np.array([258, 257, 1, 0, 2, 259, 300, 256], dtype=np.uint16), int(K[0]))
    if grouping == "each":
        goff = None
    root = 0.5 + rng.random(Kmax)                 # (positive, not normalised)
    alpha = 1.0 + 2.0 * rng.random()              # alpha r_k >= 0.5
    gamma = 0.5 + 2.0 * rng.random(Kmax)
    shape, scale = CASE_PRIOR
    return dict(K=K, t=t, goff=goff, root=root, alpha=alpha, gamma=gamma, flags=flags, seed=seed, sweep=sweep,
                shape=shape, scale=scale, Kmax=Kmax)


def replay_case(name, **kw):
    c = case(name)
    return replay(c["K"], c["t"], c["goff"], c["root"], c["alpha"], c["gamma"], c["seed"], c["sweep"], c["flags"],
                  c["shape"], c["scale"], Kmax=c["Kmax"], **kw)
