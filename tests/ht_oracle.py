"""A numpy replay of the base-weight step on a tree of nested groups (libstb_amd/csrc/htree.hip; include/stb_hip.h
stb_sample_htree), written from the header's text on hh_oracle's pieces (the counts, the Dirichlet rows, the root),
hb_oracle's step for the concentrations and tl_oracle's / hq_oracle's streams, and the law the chain is checked against.

  key = mix(seed + (sweep+1) gamma); key_1 = key, key_l = mix(key ^ (SALT_L + l)) for l >= 2.
  Cell e = v Kmax + k of level l owns key_e = mix(key_l + (e+1) gamma).
  up, l = 1 .. L     w = alpha_l h_par(v),k on the stored row of level l + 1 (the root at l = L);
                     m_vk = [c_vk >= 1] + sum_{j=1}^{c_vk-1} [u_j (w + j) < w], u_j element j of mix(key_e ^ SALT_Y);
                     the parent's counts are the sums of its children's m
  r'                 hh_oracle.draw_root on the sums handed up by level L
  alpha'_l           hb_oracle.replay (a = 0): all nodes concatenated, N = C_v, T = M_v, b = alpha_l, a range a level, on
                     seed ^ SALT_A
  down, l = L .. 1   h'_v = Dirichlet(alpha'_l h'_par(v) + c_v) on key_e (hh_oracle.dirichlet_rows)
Arrays over levels are lists indexed l - 1.
"""
import math

import numpy as np

import hb_oracle as hbo
import hh_oracle as hho
import hq_oracle as hqo

SALT_L = 0x3C6EF372FE94F82B
SALT_A = hho.SALT_A
KEEP_ROOT, SAMPLE_ALPHA = 1, 2
MAXL = 8
# the step, and two wrong ones: all tables handed up in place of the auxiliary ones; the [c >= 1] table dropped at level 2
LAWS = ("right", "counts_up", "no_first_2")
_M64 = (1 << 64) - 1


def level_keys(seed, sweep, L):
    key = hqo.sweep_key(seed, sweep)
    return [key] + [hqo.mix(np.uint64((int(key) ^ ((SALT_L + l) & _M64)) & _M64)) for l in range(2, L + 1)]


def cell_keys(key, cells):
    with np.errstate(over="ignore"):
        return hqo.mix(key + (np.arange(cells, dtype=np.uint64) + np.uint64(1)) * hqo.GAMMA)


def owners(off, below):
    """the range of every item of the level below: the last range that starts at or before it"""
    off = np.asarray(off, dtype=np.int64)
    return np.minimum(np.searchsorted(off, np.arange(below), side="right") - 1, len(off) - 2)


def aux_tables(c, w, key, first=True):
    """(m[G, Kmax], smallest relative margin of a Bernoulli comparison) of a level on its key; w[G, Kmax]"""
    G, Kmax = c.shape
    cf = c.reshape(-1).astype(np.int64)
    wf = np.ascontiguousarray(np.broadcast_to(w, (G, Kmax)), dtype=np.float64).reshape(-1)
    ky = hqo.mix(cell_keys(key, G * Kmax) ^ hbo.SALT_Y)
    cnt = np.maximum(cf - 1, 0)
    m = (cf >= 1).astype(np.int64) if first else np.zeros(G * Kmax, dtype=np.int64)
    tot = int(cnt.sum())
    margin = math.inf
    if tot:
        owner = np.repeat(np.arange(G * Kmax), cnt)
        start = np.cumsum(cnt) - cnt
        j = (np.arange(tot) - start[owner] + 1).astype(np.uint64)
        u = hqo.unit(ky[owner], j)
        b = wf[owner]
        lhs = u * (b + j.astype(np.float64))
        pos = b > 0.0                     # (under w = 0, an underflowed parent weight, u j < 0 never holds: no tie to sit on)
        margin = float(np.min(np.abs(lhs[pos] - b[pos]) / b[pos])) if pos.any() else math.inf
        m += np.bincount(owner, weights=(lhs < b).astype(np.float64), minlength=G * Kmax).astype(np.int64)
    return m.reshape(G, Kmax), margin


def replay(K, t, offs, root, rows, alpha, gamma, seed, sweep, flags=0, shape=1.0, scale=1.0, law="right", Kmax=None,
           root_new=None, alpha_new=None, rows_new=None):
    """the whole step.  offs[l] cuts level l (the restaurants for l = 0) into the nodes of level l + 1; rows[l] (l >= 1)
    are the stored rows of level l + 1 on entry (rows[0] is not read).  Returns a dict with, per level, c, m, tables,
    aux_tables, alpha (alpha') and rows (the new ones), with root (r'), h (the pairs), owner (every restaurant's level-1
    node), margin_gamma, margin_y and min_shape (the smallest shape of any Gamma variate).  root_new / alpha_new / rows_new (entries l >= 1), when given, replace the replay's
    own r' / alpha' / upper rows in the draws below them (a device's values)"""
    L = len(offs)
    assert 1 <= L <= MAXL
    alpha = [float(a) for a in np.atleast_1d(alpha)]
    root = np.asarray(root, dtype=np.float64)
    G = [len(o) - 1 for o in offs]
    keys = level_keys(seed, sweep, L)
    c1, owner1 = hho.group_counts(K, t, offs[0], Kmax)
    Kmax = c1.shape[1]
    own = [owner1] + [owners(offs[l], G[l - 1]) for l in range(1, L)]     # own[l]: level l's items -> level l + 1's nodes
    c, m = [c1], []
    my = math.inf
    for l in range(L):                                                    # up
        top = l + 1 == L
        base = root[None, :].repeat(G[l], axis=0) if top else np.asarray(rows[l + 1], dtype=np.float64)[own[l + 1]]
        ml, margin = aux_tables(c[l], alpha[l] * base, keys[l], first=not (law == "no_first_2" and l == 1))
        my = min(my, margin)
        m.append(ml)
        up = c[l] if law == "counts_up" else ml
        if top:
            s = up.sum(axis=0)
        else:
            nxt = np.zeros((G[l + 1], Kmax), dtype=np.int64)
            np.add.at(nxt, own[l + 1], up)
            c.append(nxt)
    mg = math.inf
    r1 = root
    if not flags & KEEP_ROOT:
        r1, mr = hho.draw_root(s, gamma, seed, sweep)
        mg = min(mg, mr)
    a1 = list(alpha)
    if flags & SAMPLE_ALPHA:
        C = np.concatenate([x.sum(axis=1) for x in c])
        M = np.concatenate([x.sum(axis=1) for x in m])
        b = np.concatenate([np.full(G[l], alpha[l]) for l in range(L)])
        noff = np.concatenate([[0], np.cumsum(G)]).astype(np.int64)
        hb = hbo.replay(0.0, shape, scale, M.astype(np.uint32), C.astype(np.uint32), b, noff, (seed ^ SALT_A) & _M64, sweep)
        a1 = [float(x) for x in hb["bgrp"]]
        mg, my = min(mg, hb["margin_gamma"]), min(my, hb["margin_y"])
    new = [None] * L
    low = math.inf if flags & KEEP_ROOT else float((np.broadcast_to(np.asarray(gamma, dtype=np.float64), s.shape) + s).min())
    parent = (r1 if root_new is None else np.asarray(root_new, dtype=np.float64))[None, :]
    for l in range(L - 1, -1, -1):                                        # down
        top = l + 1 == L
        a = a1[l] if alpha_new is None else float(alpha_new[l])
        base = parent.repeat(G[l], axis=0) if top else parent[own[l + 1]]
        low = min(low, float((a * base + c[l].astype(np.float64)).min()))
        new[l], mh = hho.dirichlet_rows(a * base + c[l].astype(np.float64), cell_keys(keys[l], G[l] * Kmax))
        mg = min(mg, mh)
        parent = new[l] if rows_new is None or l == 0 or rows_new[l] is None else np.asarray(rows_new[l], dtype=np.float64)
    return dict(c=c, m=m, tables=[int(x.sum()) for x in c], aux_tables=[int(x.sum()) for x in m], root=r1, alpha=a1, rows=new,
                owner=owner1, h=hho.spread(K, owner1, new[0]), margin_gamma=mg, margin_y=my, min_shape=low)


# ---- the law for two dishes and two levels: the root r, the level-2 rows h_A and h_B, the leaves' rows summed out.
# Given r the two nodes are independent:   p(r, h_A, h_B | c) ~ Dir(r; gamma) prod_{v = A, B} Beta(h_v0; alpha_2 r) L_v(h_v),
# L_v(h) = prod_{leaves g of v} prod_k Gamma(alpha_1 h_k + c_gk) / Gamma(alpha_1 h_k)

LAW_LEAVES = np.array([[5, 1], [0, 9], [2, 2]], dtype=np.int64)       # A holds the first two leaves, B the third
LAW_OFFS = (np.array([0, 1, 2, 3], dtype=np.uint64), np.array([0, 2, 3], dtype=np.uint64))
LAW_ALPHA = (2.0, 3.0)                                                 # alpha_1, alpha_2
LAW_GAMMA = np.array([0.7, 1.3])
LAW_SEED = 8802
LAW_STEPS, LAW_BURN, LAW_THIN = hho.LAW_STEPS, hho.LAW_BURN, hho.LAW_THIN

_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


class TreePosterior:
    """the marginals of r_0 and h_A0 by two-dimensional quadrature in x = logit r_0 and y = logit h_0 (trapezoid)"""

    def __init__(self, points=1601, span=40.0):
        x = np.linspace(-span, span, points)
        l0, l1 = -np.logaddexp(0.0, -x), -np.logaddexp(0.0, x)          # log of the first and second component
        a1, a2 = LAW_ALPHA

        def loglik(leaves):                                             # log L_v on the y grid
            out = np.zeros(points)
            for row in leaves:
                for k, lh in ((0, l0), (1, l1)):
                    for j in range(int(row[k])):                        # Gamma(w + c) / Gamma(w) = prod_j (w + j)
                        out = out + np.log(a1 * np.exp(lh) + j)
            return out

        w0, w1 = a2 * np.exp(l0), a2 * np.exp(l1)                       # alpha_2 r on the x grid
        # log Beta(h_0; alpha_2 r) dy at (x, y): the Jacobian h_0 h_1 turns the exponents w - 1 into w
        lbeta = (math.lgamma(a2) - _lgamma(w0) - _lgamma(w1))[:, None] + w0[:, None] * l0[None, :] + w1[:, None] * l1[None, :]
        lA, lB = loglik(LAW_LEAVES[:2]), loglik(LAW_LEAVES[2:])
        trap = np.full(points, x[1] - x[0])
        trap[0] = trap[-1] = 0.5 * (x[1] - x[0])
        FA = np.exp(lbeta + lA[None, :]) @ trap                         # int Beta(h_A) L_A(h_A) dh_A, on the x grid
        FB = np.exp(lbeta + lB[None, :]) @ trap
        prior = np.exp(LAW_GAMMA[0] * l0 + LAW_GAMMA[1] * l1)
        dens_r = prior * FA * FB
        dens_h = np.exp(lA) * ((prior * FB * trap) @ np.exp(lbeta))
        self.x = x
        self.cdf_r, self.cdf_h = self._cdf(dens_r), self._cdf(dens_h)

    def _cdf(self, dens):
        cdf = np.concatenate([[0.0], np.cumsum(0.5 * (dens[1:] + dens[:-1]) * np.diff(self.x))])
        return cdf / cdf[-1]

    def _F(self, cdf, v):
        v = np.asarray(v, dtype=np.float64)
        return np.interp(np.log(v) - np.log1p(-v), self.x, cdf)

    def F_root(self, r0):
        return self._F(self.cdf_r, r0)

    def F_node(self, hA0):
        return self._F(self.cdf_h, hA0)


def law_object():
    """(K, n, t) of three restaurants whose tables are LAW_LEAVES, a restaurant a leaf"""
    K = np.full(3, 2, dtype=np.int32)
    t = LAW_LEAVES.reshape(-1).astype(np.uint16)
    return K, t.astype(np.uint32), t


def law_chain(seed, law="right", steps=LAW_STEPS, burn=LAW_BURN, thin=LAW_THIN, step_fn=None):
    """(r_0, h_A0) of the step iterated on the fixture from r = (1/2, 1/2) and level-2 rows of (1/2, 1/2), sweeps 0, 1, ...:
    the kept values (after `burn`, every `thin`-th).  step_fn(root, rows2, sweep) -> (r', rows2') replaces the replay (the
    device).  The replay skips level 1's rows: no later draw reads them"""
    K, _, t = law_object()
    r, rows2 = np.array([0.5, 0.5]), np.full((2, 2), 0.5)
    own = owners(LAW_OFFS[1], 3)
    kept = []
    for s in range(burn + steps):
        if step_fn is None:
            k1, k2 = level_keys(seed, s, 2)
            m1, _ = aux_tables(LAW_LEAVES, LAW_ALPHA[0] * rows2[own], k1)
            c2 = np.zeros((2, 2), dtype=np.int64)
            np.add.at(c2, own, LAW_LEAVES if law == "counts_up" else m1)
            m2, _ = aux_tables(c2, LAW_ALPHA[1] * r[None, :].repeat(2, axis=0), k2, first=law != "no_first_2")
            r, _ = hho.draw_root(m2.sum(axis=0), LAW_GAMMA, seed, s)
            rows2, _ = hho.dirichlet_rows(LAW_ALPHA[1] * r[None, :].repeat(2, axis=0) + c2.astype(np.float64), cell_keys(k2, 4))
        else:
            r, rows2 = step_fn(r, rows2, s)
        if s >= burn and (s - burn) % thin == 0:
            kept.append((r[0], rows2[0, 0]))
    return np.array(kept)


_POST = []


def law_pvalues(kept):
    """(KS p-value of r_0, of h_A0) of a chain's kept values"""
    if not _POST:
        _POST.append(TreePosterior())
    post = _POST[0]
    return hbo.ks_pvalue(post.F_root(kept[:, 0])), hbo.ks_pvalue(post.F_node(kept[:, 1]))


# ---- the replay cases of tests/test_gpu_htree.py; tests/test_htree_host.py checks every one's margins on the CPU ----

CASE_PRIOR = (2.0, 4.0)                          # shape, and scale / Kmax, of the concentrations' prior
CASES = ("two_ragged", "three_k70", "one_each", "few_rows", "k1024")
VARIANTS = (0, SAMPLE_ALPHA)                     # every case with both; KEEP_ROOT_CASE once more with the root kept
KEEP_ROOT_CASE = "two_ragged"
STEPS = [(n, f) for n in CASES for f in VARIANTS] + [(KEEP_ROOT_CASE, KEEP_ROOT)]
CASE_SEEDS = {"two_ragged": (9301, 2), "three_k70": (9302, 0), "one_each": (9303, 5), "few_rows": (9304, 1), "k1024": (9305, 3)}


def even_off(n, G):
    return (np.arange(G + 1, dtype=np.int64) * n // G).astype(np.uint64)


def case(name, flags=0):
    """dict(K, t, offs, G, root, rows, alpha, gamma, flags, seed, sweep, shape, scale, Kmax)"""
    seed, sweep = CASE_SEEDS[name]
    rng = np.random.default_rng(seed)
    if name == "two_ragged":
        # 37 restaurants of 1 .. 5 dishes; level 1: 7 ranges, the third empty; level 2: 3 nodes, the second childless
        I, Kmax = 37, 5
        K = (1 + (np.arange(I) * 3 + 1) % 5).astype(np.int32)
        offs = [np.array([0, 5, 11, 11, 18, 19, 30, 37], dtype=np.uint64), np.array([0, 3, 3, 7], dtype=np.uint64)]
        t = rng.choice(np.array([0, 1, 2, 3, 40], dtype=np.uint16), size=int(K.sum()))
    elif name == "three_k70":
        # Kmax = 70 crosses the 64-lane column block; dish 0 carries enough tables that a level-1 cell and, under the large
        # alpha_1, a handed-up level-2 cell exceed 257
        I, Kmax = 90, 70
        K = np.where(np.arange(I) % 3 == 0, 70, np.array((66, 3))[np.arange(I) % 2]).astype(np.int32)
        offs = [even_off(I, 9), np.array([0, 2, 5, 5, 9], dtype=np.uint64), np.array([0, 3, 4], dtype=np.uint64)]
        t = rng.choice(np.array([0, 1, 2, 5], dtype=np.uint16), size=int(K.sum()))
        t[np.concatenate([[0], np.cumsum(K)])[:-1]] = 900
    elif name == "one_each":
        I, Kmax = 11, 6
        K = np.full(I, 6, dtype=np.int32)
        K[4] = 2
        offs = [np.array([0, 4, 4, 11], dtype=np.uint64), np.array([0, 3], dtype=np.uint64), np.array([0, 1], dtype=np.uint64)]
        t = rng.choice(np.array([0, 1, 4, 300], dtype=np.uint16), size=int(K.sum()))
    elif name == "few_rows":
        # one node a level; two restaurants with 60000 tables at a dish each: the rows are cut into parts
        I, Kmax = 2, 3
        K = np.full(I, 3, dtype=np.int32)
        offs = [np.array([0, 2], dtype=np.uint64), np.array([0, 1], dtype=np.uint64)]
        t = np.array([60000, 2, 0, 1, 59999, 0], dtype=np.uint16)
    elif name == "k1024":
        I, Kmax = 12, 1024
        K = np.where(np.arange(I) % 4 == 0, 1024, np.array((1, 2, 5))[np.arange(I) % 3]).astype(np.int32)
        offs = [np.array([0, 3, 4, 9, 12], dtype=np.uint64), np.array([0, 1, 4], dtype=np.uint64)]
        t = rng.choice(np.array([0, 1, 2, 3, 40], dtype=np.uint16), size=int(K.sum()))
        t[:4] = (258, 257, 1, 300)
    else:
        raise KeyError(name)
    L = len(offs)
    G = [len(o) - 1 for o in offs]
    # a row that is drawn is a parent's weights one call later, and its entries are of the size 1 / Kmax: concentrations of a
    # few Kmax and a gamma of 20 and more keep every Gamma shape near 1 or above, so that no weight underflows to zero
    # (a child's shape alpha * 0 + 0 would be the step's error 4)
    root = (0.5 + rng.random(Kmax)) / Kmax                             # (positive, not normalised)
    rows = [None] + [(0.5 + rng.random((G[l], Kmax))) / Kmax for l in range(1, L)]
    alpha = [Kmax * (2.0 + 2.0 * rng.random()) for _ in range(L)]
    if name == "three_k70":                                            # a tenth of dish 0's 9000 tables a node are auxiliary ones
        alpha[0] = 400.0
        rows[1][:, 0] = 0.9
    if name == "few_rows":
        alpha[0] = 3000.0
    gamma = 20.0 + 5.0 * rng.random(Kmax)
    shape, scale = CASE_PRIOR[0], CASE_PRIOR[1] * Kmax
    return dict(K=K, t=t, offs=offs, G=G, root=root, rows=rows, alpha=alpha, gamma=gamma, flags=flags, seed=seed, sweep=sweep,
                shape=shape, scale=scale, Kmax=Kmax)


def replay_case(name, flags=0, **kw):
    c = case(name, flags)
    return replay(c["K"], c["t"], c["offs"], c["root"], c["rows"], c["alpha"], c["gamma"], c["seed"], c["sweep"], c["flags"],
                  c["shape"], c["scale"], Kmax=c["Kmax"], **kw)
