"""The oracle of the Gibbs chain a table-indicator object runs (examples/pyp_resample -d -z -L -w -C -K [-H | -T | -V] and
-X), composed from the oracles of its steps, and the exact posterior of a model small enough to enumerate.  No replay
arithmetic lives here:

  sweep_dishes    td_oracle.sweep            sweep           ti_oracle.sweep
  sample_lik      tl_oracle.sample_lik       sample_h        tl_oracle.sample_h
  sample_hgroups  hh_oracle.replay           sampleb_groups  hb_oracle.replay
  sample_htree    ht_oracle.replay           sample_classes  cg_oracle.sample_classes
  generate        cg_oracle.generate (st_oracle.replay under the prior, then every class)
  sample_gauss    gs_oracle.stats, gs_oracle.draw, gs_oracle.lik
  sample_beta     dc_oracle.replay, columns of the (class, dish) counts over the matrix's shape
  sample_gamma    dc_oracle.replay, the one row c_k = sum_i t_ik

A State holds everything a step reads or writes; step() takes one to the next and reports the margins of the draws it
made; PROGRAMS are the example's iterations -- flat, grouped (-H), tree (-T), missing (-V with every third class missing)
and gauss (-X) -- and PROLOGUES what runs once before them; run() is the pure CPU chain.  fetch() fills a State from an
object; check_step() holds a step's outcome, a device's or a wrong chain's, against the oracle's.

The exact target: I = 2 restaurants of Nc = 3 customers, K = 2 dishes, 2 classes, a, b, a symmetric
beta and a symmetric gamma fixed.  With h and the matrix summed out,

    p(z, t) ~ prod_i (b|a)_{T_i} / (b)_{N_i} prod_k S^{n_ik}_{t_ik}(a)
            x Gamma(K gamma) / Gamma(K gamma + sum_k c_k) prod_k Gamma(gamma + c_k) / Gamma(gamma)       c_k = sum_i t_ik
            x prod_k Gamma(R beta) / Gamma(R beta + cnt_.k) prod_w Gamma(beta + cnt_wk) / Gamma(beta)

over the 18 x 18 states (z, t) of the two restaurants.  The four steps dishes, lik, h, indicators at fixed hyper-parameters
are Gibbs steps of the joint over (z, t, h, matrix), so the (z, t) they visit have this law; the restaurants meet only in
c_k and cnt_wk, that is through the redrawn h and matrix.
"""
from __future__ import annotations

import dataclasses
import math
from functools import lru_cache

import numpy as np

import cg_oracle as cgo
import dc_oracle as dco
import gs_oracle as gso
import hb_oracle as hbo
import hh_oracle as hho
import ht_oracle as hto
import orc
import td_oracle as tdo
import ti_oracle as tio
import tl_oracle as tlo


@dataclasses.dataclass
class State:
    K: np.ndarray                 # [I] dishes a restaurant
    n: np.ndarray                 # [G] customers a pair
    t: np.ndarray                 # [G] tables a pair
    T: np.ndarray                 # [I] tables a restaurant
    cust: np.ndarray              # [C] every customer's dish (local pair index), restaurants back to back
    cls: np.ndarray               # [C] every customer's class
    h: np.ndarray                 # [G] base weights at the pairs
    lik: np.ndarray               # (rows, stride) the matrix
    root: np.ndarray              # [Kmax] the root of the grouped base weights
    alpha: float | None           # the concentration the last sample_hgroups left (None: none yet)
    bpar: np.ndarray              # [I] concentrations
    beta: float
    gamma: float
    a: float
    hgoff: np.ndarray | None = None   # the ranges of sample_hgroups (None: a restaurant a group)
    bgoff: np.ndarray | None = None   # the ranges of sampleb_groups
    htoff: tuple | None = None        # the tree: htoff[l] cuts level l (the restaurants for l = 0) into level l + 1's nodes
    hrows: tuple | None = None        # the stored rows of the levels 2 .. L (hrows[l - 2]: G_l x Kmax)
    alphas: tuple | None = None       # every level's concentration as the last sample_htree left it (None: none yet)
    x: np.ndarray | None = None       # [C, D] the observations (observation mode: cls = arange(C), lik is C x K)
    mu: np.ndarray | None = None      # [K, D] the dishes' means
    tau: np.ndarray | None = None     # [K, D] and precisions
    gprior: dict | None = None        # gs_oracle.prior

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)

    def Ni(self):
        return np.array([x.sum() for x in np.split(np.asarray(self.n, dtype=np.int64), np.cumsum(self.K)[:-1])])

    def bounds(self):
        """(N, M) of the V table an object holds from its first dish sweep on (created with M = 0)"""
        big = int(self.Ni().max())
        N = max(big, 3)
        return N, min(max(big, 1), N)

    def integers(self):
        return self.n, self.t, self.T, self.cust


def fetch(ti, base: State) -> State:
    """the object's state through its getters -- the classes, and where the mode has them the tree's stored rows and the
    dishes' parameters, among them; what no getter returns -- K, the ranges, x, the priors, a, beta, gamma and the
    concentrations the step infos reported -- is carried over from `base`"""
    from libstb_amd import capi

    more = dict(cls=ti.get_classes()[0])
    if base.htoff is not None:
        more["hrows"] = tuple(ti.get_htree_level(l) for l in range(2, len(base.htoff) + 1))
    if base.x is not None:
        more["mu"], more["tau"] = ti.get_gauss()
    t, T = ti.get()
    n, cust = ti.get_state()
    p, rows, stride, q = ti.lik_device()
    lik = np.empty((rows, stride), dtype=np.float64)
    L = capi.lib()
    capi.check(L.stb_memcpy_d2h(lik.ctypes.data, p, lik.nbytes, q))
    capi.check(L.stb_stream_sync(q))
    return base.replace(n=n, t=t, T=T, cust=cust, h=ti.get_h(), lik=lik, root=ti.get_hroot(), bpar=ti.get_bpar(), **more)


def class_counts(st: State, cust=None) -> np.ndarray:
    """customers per (class, dish) over the matrix's shape (what _sample_lik, _sample_beta and CJ_DATA count)"""
    cnt = np.zeros(st.lik.shape, dtype=np.uint32)
    np.add.at(cnt, (st.cls.astype(np.int64), np.asarray(st.cust if cust is None else cust, dtype=np.int64)), 1)
    return cnt


@lru_cache(maxsize=None)
def host_vtab(a: float, N: int, M: int):
    """the V table of the CPU oracle (oracle/liboracle.so), for chains that run without a device"""
    return tio.VTab(orc.fill_V(a, N, M), N, M)


# every prior of the example: (shape, scale)
PRIOR_BETA, PRIOR_GAMMA, PRIOR_ALPHA, PRIOR_B = (1.1, 1.0), (1.1, 10.0), (1.1, 20.0), (1.1, 20.0)
ALPHA0 = 5.0     # the grouped step's concentration before it has drawn one


def class_mask(C: int) -> np.ndarray:
    """the missing classes of the program `missing`: every third customer's"""
    return (np.arange(C) % 3 == 0).astype(np.uint8)


def step(st: State, name: str, seed: int, sweep: int, vtab=host_vtab, **kw):
    """one step of the object's method `name` on `st`: (the next State, a dict with the step's counters and, where the
    underlying oracle reports them, margin_gamma / margin_y).  vtab(a, N, M) gives the V table (a device's own cells where
    the bits are compared).  kw: sample_lik cnt (the counts to draw from, for the wrong laws); sample_hgroups flags,
    root_new, alpha_new (a device's r' and alpha' for the group draw, as tests/test_gpu_hgroups.py feeds them);
    sample_htree root_new, alpha_new (one a level), rows_new (the levels 2 .. L) likewise; sample_gauss cust, mu_new, tau_new"""
    if name == "sweep_dishes":
        N, M = st.bounds()
        n, t, T, cust, skipped, stuck = tdo.sweep(st.K, st.n, st.t, st.h, st.a, st.bpar, vtab(st.a, N, M), N, M, seed, sweep,
                                                  st.cust, st.cls, st.lik)
        return st.replace(n=n, t=t, T=T, cust=cust), dict(skipped=skipped, stuck=stuck)
    if name == "sweep":
        N, M = st.bounds()
        t, T = tio.sweep(st.K, st.n, st.t, st.h, st.a, st.bpar, vtab(st.a, N, M), N, seed, sweep, st.cust)
        return st.replace(t=t, T=T), {}
    if name == "sample_lik":
        lik, margin = tlo.sample_lik(kw.get("cnt", class_counts(st)), st.beta, seed, sweep)
        return st.replace(lik=lik), dict(margin_gamma=margin)
    if name == "sample_h":
        hk, margin = tlo.sample_h(st.K, st.t, st.gamma, seed, sweep)
        return st.replace(h=tlo.spread_h(st.K, hk)), dict(margin_gamma=margin)
    if name == "sample_hgroups":
        flags = kw.get("flags", hho.SAMPLE_ALPHA)
        alpha = ALPHA0 if st.alpha is None else st.alpha
        shape, scale = PRIOR_ALPHA
        r = hho.replay(st.K, st.t, st.hgoff, st.root, alpha, st.gamma, seed, sweep, flags, shape, scale,
                       root_new=kw.get("root_new"), alpha_new=kw.get("alpha_new"))
        return st.replace(h=r["h"], root=r["root"], alpha=r["alpha"]), dict(
            tables=r["tables"], aux_tables=r["aux_tables"], margin_gamma=r["margin_gamma"], margin_y=r["margin_y"])
    if name == "sample_htree":
        L = len(st.htoff)
        alpha = [ALPHA0] * L if st.alphas is None else list(st.alphas)
        shape, scale = PRIOR_ALPHA
        rows_new = kw.get("rows_new")
        r = hto.replay(st.K, st.t, list(st.htoff), st.root, [None] + list(st.hrows), alpha, st.gamma, seed, sweep,
                       hto.SAMPLE_ALPHA, shape, scale, Kmax=len(st.root), root_new=kw.get("root_new"),
                       alpha_new=kw.get("alpha_new"), rows_new=None if rows_new is None else [None] + list(rows_new))
        return st.replace(h=r["h"], root=r["root"], hrows=tuple(r["rows"][1:]), alphas=tuple(r["alpha"]), alpha=r["alpha"][0]), dict(
            tables=r["tables"], aux_tables=r["aux_tables"], rows1=r["rows"][0], margin_gamma=r["margin_gamma"],
            margin_y=r["margin_y"])
    if name == "sample_classes":
        cls, (skipped, stuck, drawn) = cgo.sample_classes(st.lik, st.cust, seed, sweep, st.cls, class_mask(len(st.cust)))
        return st.replace(cls=cls), dict(skipped=skipped, stuck=stuck, drawn=drawn)
    if name == "generate":
        coff = np.concatenate([[0], np.cumsum(st.Ni())]).astype(np.uint64)
        r = cgo.generate(st.K, st.h, st.a, st.bpar, coff, st.lik, M=0, seed=seed, sweep=sweep)
        skipped, stuck, drawn = r["cls_info"]
        return st.replace(n=r["n"], t=r["t"], T=r["T"], cust=r["cust"], cls=r["cls"]), dict(
            skipped=skipped, stuck=stuck, drawn=drawn, seat=(r["skipped"], r["impossible"], r["stuck"]))
    if name == "sample_gauss":
        # statistics from kw's cust (the wrong chains) or the state's; the matrix from kw's mu_new, tau_new (a device's)
        n, mean, Q, skipped = gso.stats(st.x, kw.get("cust", st.cust), int(st.K.max()))
        mu, tau, margin = gso.draw(n, mean, Q, st.gprior, seed, sweep)
        kn, mn, _, _ = gso.posterior(n, mean, Q, st.gprior)
        lik, dead = gso.lik(st.x, kw.get("mu_new", mu), kw.get("tau_new", tau))
        return st.replace(mu=mu, tau=tau, lik=lik), dict(
            skipped=skipped, dead=dead, margin_gamma=margin, mu_scale=np.maximum(np.abs(mn), 1.0 / np.sqrt(kn * tau)))
    if name == "sampleb_groups":
        shape, scale = PRIOR_B
        goff = None if st.bgoff is None else np.asarray(st.bgoff, dtype=np.int64)
        r = hbo.replay(st.a, shape, scale, st.T, st.Ni().astype(np.uint32), st.bpar, goff, seed, sweep)
        return st.replace(bpar=r["bpar"]), dict(bgrp=r["bgrp"], kept=r["kept"], margin_gamma=r["margin_gamma"],
                                                margin_y=r["margin_y"])
    if name in ("sample_beta", "sample_gamma"):
        if name == "sample_beta":
            (shape, scale), cnt, s, orient = PRIOR_BETA, class_counts(st), st.beta, dco.COLUMNS
        else:
            (shape, scale), s, orient = PRIOR_GAMMA, st.gamma, dco.ROWS
            cnt = tlo.table_counts(st.K, st.t).astype(np.uint32)[None, :]
        r = dco.replay(cnt, 1.0, s, shape, scale, seed, sweep, orient)
        out = dict(s=r["s"], count=r["count"], aux_tables=r["aux_tables"], nonempty=r["nonempty"],
                   margin_gamma=r["margin_gamma"], margin_y=r["margin_y"])
        return (st.replace(beta=r["s"]) if name == "sample_beta" else st.replace(gamma=r["s"])), out
    raise ValueError(name)


# (method, the offset of its seed from the chain's): the order and the seeds of examples/pyp_resample.c
PROGRAMS = {
    "flat": (("sweep_dishes", 2), ("sample_beta", 5), ("sample_gamma", 6), ("sample_lik", 3), ("sample_h", 4), ("sweep", 0),
             ("sampleb_groups", 1)),
    "grouped": (("sweep_dishes", 2), ("sample_beta", 5), ("sample_lik", 3), ("sample_hgroups", 4), ("sweep", 0),
                ("sampleb_groups", 1)),
    "tree": (("sweep_dishes", 2), ("sample_beta", 5), ("sample_lik", 3), ("sample_htree", 4), ("sweep", 0), ("sampleb_groups", 1)),
    # the example draws no class inside its loop: sample_classes takes the first offset the example leaves free
    "missing": (("sweep_dishes", 2), ("sample_classes", 11), ("sample_beta", 5), ("sample_lik", 3), ("sample_h", 4), ("sweep", 0),
                ("sampleb_groups", 1)),
    # -X's own offsets (dish sweep 0, draw 2, h 3, b 1); it runs no indicator sweep: the next free offset
    "gauss": (("sample_gauss", 2), ("sweep_dishes", 0), ("sample_h", 3), ("sweep", 12), ("sampleb_groups", 1)),
}
PROLOGUES = {"missing": (("generate", 7),)}      # once, at sweep 0, before the first iteration
FIXED = ("sweep_dishes", "sample_lik", "sample_h", "sweep")      # the steps of `flat` that draw no hyper-parameter
LAWS = ("right", "stale_lik", "no_h", "lik_prior")


def restrict(program, names=FIXED):
    return tuple(p for p in program if p[0] in names)


def margin_of(info) -> float:
    return min(info.get("margin_gamma", math.inf), info.get("margin_y", math.inf))


def run(program, st: State, iterations: int, seed: int, a_at=None, law="right", vtab=host_vtab, keep=None):
    """the pure CPU chain: `iterations` rounds of `program` (a name in PROGRAMS or a tuple), sweep index = iteration, the
    discount replaced by a_at[it] before iteration it, a named program's PROLOGUES first.  Returns (the State after every iteration, the smallest margin met);
    keep(st) -> anything: the list holds that instead.  law: one of LAWS -- the wrong ones, for the power of the law test:
    stale_lik draws the matrix from the class counts of before the iteration's dish sweep, no_h never draws h again,
    lik_prior draws the matrix from the prior"""
    prologue = PROLOGUES.get(program, ()) if isinstance(program, str) else ()
    program = PROGRAMS[program] if isinstance(program, str) else program
    out, worst = [], math.inf
    for name, off in prologue:
        st, info = step(st, name, seed + off, 0, vtab)
        worst = min(worst, margin_of(info))
    for it in range(iterations):
        if a_at and it in a_at:
            st = st.replace(a=a_at[it])
        stale = class_counts(st) if law != "right" else None
        for name, off in program:
            kw = {}
            if name == "sample_h" and law == "no_h":
                continue
            if name == "sample_lik" and law == "stale_lik":
                kw["cnt"] = stale
            if name == "sample_lik" and law == "lik_prior":
                kw["cnt"] = np.zeros_like(stale)
            st, info = step(st, name, seed + off, it, vtab, **kw)
            worst = min(worst, margin_of(info))
        out.append(st if keep is None else keep(st))
    return out, worst


def collapsed_truth(st: State, indicators: bool, flat: bool):
    """the truth of stb_tindic_logjoint_collapsed on `st` with CJ_DATA and CJ_FLAT (flat) or CJ_ROOT, composed from
    lj_oracle.truth (h absent) and dm_oracle.truth: a dict of (value, bar) for pairs, restaurants, binom, tables, data,
    root and total.  The root term and its bar are those of tests/test_gpu_dirmult.py; the total adds the six components in
    plain doubles: five roundings of at most u / 2 times a partial sum each, 3 u sum |component| on top of their bars"""
    import dm_oracle as dmo
    import hp_oracle as hp
    import lj_oracle as lj

    mp = hp._mp()
    N, M = st.bounds()
    base = lj.truth(st.K, st.n, st.t, None, st.a, st.bpar, lj.Tables(st.a, N, M), indicators)
    out = {k: base[k] for k in ("pairs", "restaurants", "binom")}
    out["root"] = (0.0, 0.0)
    if flat:
        out["tables"] = dmo.truth(tlo.table_counts(st.K, st.t).astype(np.uint32)[None, :], st.gamma, dmo.ROWS)["total"]
    else:
        c, _ = hho.group_counts(st.K, st.t, st.hgoff)
        out["tables"] = dmo.truth(c.astype(np.uint32), st.root, dmo.ROWS, st.alpha)["total"]
        Kd = len(st.root)
        R = mp.fsum(mp.mpf(float(r)) for r in st.root)
        g = mp.mpf(float(st.gamma))
        logs = [(g - 1) * mp.log(mp.mpf(float(r)) / R) for r in st.root]
        val = mp.loggamma(Kd * g) - Kd * mp.loggamma(g) + mp.fsum(logs)
        mags = float(abs(mp.loggamma(Kd * g)) + Kd * abs(mp.loggamma(g)) + mp.fsum(abs(x) for x in logs))
        out["root"] = (float(val), hp.U * ((hp.L_LGAMMA + 3.0) * mags + Kd * abs(float(st.gamma) - 1.0) * (Kd + 2.0) + 16.0))
    out["data"] = dmo.truth(class_counts(st), st.beta, dmo.COLUMNS)["total"]
    names = ("pairs", "restaurants", "binom", "tables", "data", "root")
    out["total"] = (math.fsum(out[k][0] for k in names),
                    sum(out[k][1] for k in names) + 3.0 * hp.U * sum(abs(out[k][0]) for k in names))
    return out


# ---- the handover cases of tests/test_gpu_chain.py; tests/test_chain_host.py checks every one's margins on the CPU ----

A_CHANGE = {3: 0.55}      # between iterations 2 and 3: the V and S slabs are filled again for another discount
ITERATIONS = 6
CASE_SEEDS = {("mixed", "flat"): 4100, ("mixed", "grouped"): 4200, ("tiny", "flat"): 4300, ("tiny", "grouped"): 4400,
              # the first of 4500, 4600, .. whose pure CPU chain keeps every margin above 1e-7 (tests/test_chain_host.py)
              ("mixed", "tree"): 4500, ("tiny", "tree"): 4500, ("generated", "missing"): 4500, ("g8", "gauss"): 4500,
              ("g65", "gauss"): 4500}
HELDOUT_CASE = ("mixed", "flat")     # the chain that also runs with the held-out calls between its iterations
HELDOUT_PARTICLES, HELDOUT_TAU, HELDOUT_OFFSET = 4, 0.5, 8      # the example's seed offset; its sweep is 4096 iteration


def heldout_set(st: State):
    """(hoff, hcls): 0 .. 6 held-out customers a restaurant (one restaurant with none, one with 6), classes below the
    state's"""
    rng = np.random.default_rng(4004)
    I = len(st.K)
    cnt = rng.integers(0, 7, size=I)
    cnt[0], cnt[-1] = 0, 6
    hoff = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    return hoff, rng.integers(0, int(st.cls.max()) + 1, size=int(hoff[-1])).astype(np.uint32)


def case(name: str, program: str) -> State:
    """the start of a handover case.  mixed: K_i = 1, 64, 65, 130, 7, 7, 3, 70 with 8 .. 40 customers a restaurant in pair
    order, 3 classes under a matrix of 5 rows x 136 (rows past the classes' and columns past the largest K are drawn from
    the prior), the ranges 0, 1, 1, 4, 8 (one empty) for the grouped base weights and the concentrations.  tiny: the law's
    model.  g8, g65: gauss_case"""
    if name == "tiny":
        st = law_start(TINY_START)
        hgoff = np.array([0, 1, 2], dtype=np.uint64)
    else:
        rng = np.random.default_rng(4001)
        K = np.array([1, 64, 65, 130, 7, 7, 3, 70], dtype=np.int32)
        Ni = np.array([8, 40, 33, 40, 17, 9, 12, 25])
        n = np.concatenate([rng.multinomial(c, rng.dirichlet(np.full(k, 0.3))) for c, k in zip(Ni, K)]).astype(np.uint32)
        t = np.where(n > 0, 1 + np.floor(rng.random(len(n)) * np.minimum(n, 3)), 0).astype(np.uint16)
        cust = tio.pair_order(K, n)
        cls = rng.integers(0, 3, size=len(cust)).astype(np.uint32)
        T = np.array([x.sum() for x in np.split(t.astype(np.int64), np.cumsum(K)[:-1])], dtype=np.uint32)
        st = State(K=K, n=n, t=t, T=T, cust=cust, cls=cls, h=0.05 + rng.random(len(n)), lik=0.1 + rng.random((5, 136)),
                   root=np.full(130, 1.0 / 130), alpha=None, bpar=0.5 + 2.0 * rng.random(8), beta=0.4, gamma=0.7, a=0.35)
        hgoff = np.array([0, 1, 1, 4, 8], dtype=np.uint64)
    if name in GAUSS_CASES:
        return gauss_case(name)
    if program in ("grouped", "tree"):      # (the restaurants of a range share one concentration: the first one's)
        sizes = np.diff(hgoff.astype(np.int64))
        st = st.replace(bgoff=hgoff, gamma=1.0, bpar=np.repeat(st.bpar[hgoff[:-1][sizes > 0].astype(np.int64)], sizes[sizes > 0]))
    if program == "grouped":
        st = st.replace(hgoff=hgoff)
    if program == "tree":
        # tiny: one level, the grouped step's ranges.  mixed: two levels, an empty node at each, a node of one restaurant
        htoff = (hgoff,) if name == "tiny" else (hgoff, np.array([0, 1, 1, 4], dtype=np.uint64))
        Kmax = len(st.root)
        st = st.replace(htoff=htoff, hrows=tuple(np.full((len(o) - 1, Kmax), 1.0 / Kmax) for o in htoff[1:]))
    if program == "missing":      # the corpus is generated from this matrix: zeros, a column with one positive cell
        st = st.replace(lik=cgo.matrix_with_zeros(5, 136, 4002))
    return st


# (I, K, D, the prior): g8 boosts its Gamma draws (alpha0 < 1) under a prior with a vector for beta0 and for m0; g65 takes
# the dish sweep through LDS, the matrix in two blocks of dishes from the transposed copies, the statistics past 16 dimensions
GAUSS_CASES = {
    "g8": (6, 8, 2, lambda: gso.prior(0.7, 0.4, np.array([0.5, 0.8]), 2, m0=np.array([-1.0, 1.0]))),
    "g65": (5, 65, 17, lambda: gso.prior(0.01, 1.0, 1.0, 17)),
}


def gauss_case(name: str) -> State:
    """the start of a Gaussian case, as examples/pyp_resample -X builds it: 8 .. 40 customers a restaurant, x around one of
    four centres (a restaurant prefers one), every customer at a random dish but the last, which starts empty, a table a
    pair in use, h = 1 / K; the parameters the object starts with are mu = 0, tau = 1"""
    I, Kd, D, pr = GAUSS_CASES[name]
    rng = np.random.default_rng([4003, Kd])
    Ni = rng.integers(8, 41, size=I)
    Ni[0], Ni[-1] = 8, 40
    C = int(Ni.sum())
    rest = np.repeat(np.arange(I), Ni)
    d = np.arange(D)
    centre = np.array([8.0 * np.where((j >> (d & 1)) & 1, 1.0, -1.0) + np.where(d > 1, 2.0 * j, 0.0) for j in range(4)])
    z = np.where(rng.random(C) < 0.7, rest % 4, rng.integers(0, 4, size=C))
    x = centre[z] + rng.normal(0.0, 1.0, size=(C, D))
    cust = rng.integers(0, Kd - 1, size=C).astype(np.uint32)
    n = np.zeros(I * Kd, dtype=np.uint32)
    np.add.at(n, rest * Kd + cust, 1)
    t = (n > 0).astype(np.uint16)
    mu, tau = np.zeros((Kd, D)), np.ones((Kd, D))
    return State(K=np.full(I, Kd, dtype=np.int32), n=n, t=t, T=t.reshape(I, Kd).sum(axis=1).astype(np.uint32), cust=cust,
                 cls=np.arange(C, dtype=np.uint32), h=np.full(I * Kd, 1.0 / Kd), lik=gso.lik(x, mu, tau)[0],
                 root=np.full(Kd, 1.0 / Kd), alpha=None, bpar=np.full(I, 1.0), beta=1.0, gamma=1.0, a=0.1, x=x, mu=mu, tau=tau,
                 gprior=pr())


def make_object(st: State):
    """a capi.TableIndicators in the state `st` (cust in pair order is left to the object: None)"""
    from libstb_amd import capi

    pair = np.array_equal(st.cust, tio.pair_order(st.K, st.n))
    ti = capi.TableIndicators(st.K, st.n, st.t, st.h, None if pair else st.cust)
    if st.x is not None:
        ti.set_obs(st.x)
        ti.set_gauss(st.mu, st.tau)
    else:
        ti.set_classes(st.cls, int(st.cls.max()) + 1)
        ti.set_lik(st.lik)
    ti.set_bpar(st.bpar)
    if st.hgoff is not None:
        ti.set_hgroups(st.hgoff)
    if st.htoff is not None:
        ti.set_htree(list(st.htoff))
    if st.bgoff is not None:
        ti.set_bgroups(st.bgoff)
    return ti


def gauss_prior(st: State):
    """the State's prior as capi.gauss_prior's pair (a scalar beta0 and no m0 where the prior is that plain)"""
    from libstb_amd import capi

    pr = st.gprior
    b0 = pr["beta0"]
    return capi.gauss_prior(pr["kappa0"], pr["alpha0"], float(b0[0]) if np.all(b0 == b0[0]) else b0,
                            pr["m0"] if pr["m0"].any() else None)


# ---- a step's outcome against the oracle's: what tests/test_gpu_chain.py holds the device to, and tests/test_chain_host.py
# the wrong chains ----

U = 2.0 ** -53
FIELDS = ("n", "t", "T", "cust", "cls", "h", "lik", "root", "bpar", "hrows", "mu", "tau")
INTEGERS = ("n", "t", "T", "cust", "cls")
WRITES = {"sweep_dishes": ("n", "t", "T", "cust"), "sweep": ("t", "T"), "sample_lik": ("lik",), "sample_h": ("h",),
          "sample_hgroups": ("h", "root"), "sampleb_groups": ("bpar",), "sample_beta": (), "sample_gamma": (),
          "sample_htree": ("h", "root", "hrows"), "sample_classes": ("cls",), "generate": ("n", "t", "T", "cust", "cls"),
          "sample_gauss": ("lik", "mu", "tau")}


def same(x, y) -> bool:
    """to the bit; a field a mode does not have is None on both sides, the tree's rows a tuple of arrays"""
    if x is None or y is None:
        return x is None and y is None
    if isinstance(x, tuple):
        return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
    x, y = np.asarray(x), np.asarray(y)
    if x.dtype.kind == "f":
        return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x, dtype=np.float64).view(np.uint64),
                                                     np.ascontiguousarray(y, dtype=np.float64).view(np.uint64))
    return np.array_equal(x, y)


def assert_replayed(got, want, what):
    """the single-step tests' standing bar (tests/test_gpu_tlik.py): 1e-10 relative where the replay's value is >= 1e-280,
    1e-290 absolute below; no cell left out.  Returns the largest relative error"""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    assert got.shape == want.shape and not np.isnan(got).any(), what
    big = want >= 1e-280
    err = np.abs(got - want)
    rel = float((err[big] / want[big]).max()) if big.any() else 0.0
    small = float(err[~big].max()) if (~big).any() else 0.0
    assert rel <= 1e-10, (what, rel)
    assert small <= 1e-290, (what, small)
    return rel


def check_step(name, where, before, after, want, got, info, unfed=None):
    """one step's outcome `after` (info `got`) against the oracle's `want` (info `info`) on `before`.  unfed (sample_htree):
    the oracle's outcome when nothing of the device's was fed to it; None: `want` is that.  Returns the step's largest
    relative error over the 1e-10 bar"""
    worst = 0.0

    def replayed(g, w, what):
        nonlocal worst
        worst = max(worst, assert_replayed(g, w, what) / 1e-10)

    unfed = want if unfed is None else unfed
    assert margin_of(info) > 1e-9, (where, "a draw of this step sits on a tie", margin_of(info))
    for f in FIELDS:                                      # what the step's contract says it does not write: to the bit
        if f not in WRITES[name]:
            assert same(getattr(after, f), getattr(before, f)), (where, f, "was written")
    for f in INTEGERS:                                    # integers: bit for bit
        assert np.array_equal(getattr(after, f), getattr(want, f)), (where, f)
    for k in ("skipped", "stuck", "drawn", "seat", "dead", "tables", "aux_tables", "count", "nonempty", "kept"):
        if k in info:
            assert got[k] == info[k], (where, k, got[k], info[k])
    rows, Kmax = after.lik.shape[0], int(after.K.max())
    if name == "sample_lik":
        replayed(after.lik, want.lik, where + " lik")
        assert all(abs(math.fsum(after.lik[:, k]) - 1.0) <= 2.0 * U * rows for k in range(after.lik.shape[1])), where
    if name in ("sample_h", "sample_hgroups", "sample_htree"):
        replayed(after.h, want.h, where + " h")
        koff = np.concatenate([[0], np.cumsum(after.K)])
        full = [i for i in range(len(after.K)) if after.K[i] == Kmax]
        assert full and all(abs(math.fsum(after.h[koff[i]:koff[i + 1]]) - 1.0) <= 2.0 * U * Kmax for i in full), where
    if name == "sample_hgroups":
        replayed(after.root, want.root, where + " root")
        assert abs(math.fsum(after.root) - 1.0) <= 2.0 * U * Kmax, where
        assert abs(got["alpha"] - want.alpha) <= 1e-10 * want.alpha and got["alpha"] != before.alpha, (where, got["alpha"], want.alpha)
    if name == "sample_htree":
        L = len(after.htoff)
        # level 1's rows are the pairs' h: the scatter the next dish sweep reads, and the rows the object stores
        replayed(got["rows1"], info["rows1"], where + " level 1")
        assert same(after.h, hho.spread(after.K, hho.group_counts(after.K, after.t, after.htoff[0], Kmax)[1], got["rows1"])), where
        # every value the replay was fed -- the root, the upper rows, the concentrations -- against the replay fed nothing
        replayed(after.root, unfed.root, where + " root")
        assert abs(math.fsum(after.root) - 1.0) <= 2.0 * U * Kmax, where
        assert len(after.hrows) == len(unfed.hrows) == L - 1, where
        for l in range(L - 1):
            replayed(after.hrows[l], want.hrows[l], where + " level %d" % (l + 2))
            replayed(after.hrows[l], unfed.hrows[l], where + " level %d, nothing fed" % (l + 2))
            assert all(abs(math.fsum(r) - 1.0) <= 2.0 * U * Kmax for r in after.hrows[l]), where
        assert len(got["alphas"]) == L and got["alphas"] != (None if before.alphas is None else tuple(before.alphas)), where
        for l in range(L):
            assert abs(got["alphas"][l] - unfed.alphas[l]) <= 1e-10 * unfed.alphas[l], (where, l, got["alphas"], unfed.alphas)
            worst = max(worst, abs(got["alphas"][l] - unfed.alphas[l]) / unfed.alphas[l] / 1e-10)
    if name == "sample_gauss":
        # mu and tau against the replay on the replay's own statistics (tests/test_gpu_gauss.py's scale for mu); the
        # matrix against the replay's on the parameters it was fed
        assert np.all(np.isfinite(after.mu)) and np.all(after.tau > 0.0) and np.all(np.isfinite(after.tau)), where
        rel_tau = float((np.abs(after.tau - want.tau) / want.tau).max())
        rel_mu = float((np.abs(after.mu - want.mu) / info["mu_scale"]).max())
        assert rel_tau <= 1e-10 and rel_mu <= 1e-10, (where, rel_tau, rel_mu)
        worst = max(worst, rel_tau / 1e-10, rel_mu / 1e-10)
        replayed(after.lik, want.lik, where + " lik")
        assert int(np.sum(after.lik.max(axis=1) != 1.0)) == info["dead"], where      # a row's largest cell is exp(0)
    if name == "sampleb_groups":
        assert np.all(np.abs(after.bpar - want.bpar) <= 1e-10 * want.bpar), (where, "bpar")
        assert np.all(np.abs(got["bgrp"] - info["bgrp"]) <= 1e-10 * info["bgrp"]), (where, "bgrp")
        assert not np.array_equal(after.bpar, before.bpar), where
        worst = max(worst, float((np.abs(after.bpar - want.bpar) / want.bpar).max()) / 1e-10)
    if name in ("sample_beta", "sample_gamma"):
        assert abs(got["s"] - info["s"]) <= 1e-10 * info["s"] and got["s"] != (before.beta if name == "sample_beta" else before.gamma), where
        worst = max(worst, abs(got["s"] - info["s"]) / info["s"] / 1e-10)
    return worst


# ---- the exact target on the tiny flat model ----

LAW = dict(I=2, Nc=3, K=2, R=2, a=0.3, b=1.0, beta=0.15, gamma=0.25, cls=(0, 0, 1, 0, 1, 1))
LAW_SEED, LAW_START_SEED = 7300, 7301
LAW_ITERATIONS, LAW_THIN = 1500, 2          # 4 calls an iteration: 6000, the cap of a device law test (dc_oracle.LAW_STEPS)


@lru_cache(maxsize=None)
def enumerate_states():
    """every (z, t) of the two restaurants: a list of ((z_0, t_0), (z_1, t_1)), z_i the three customers' dishes"""
    one = tdo.states(LAW["Nc"], LAW["K"])
    return [(s0, s1) for s0 in one for s1 in one]


def log_p_terms(state):
    """the terms of log of the unnormalised p(z, t) above, in log-gamma and generalised Stirling numbers"""
    a, b, beta, gamma, K, R, Nc = (LAW[k] for k in ("a", "b", "beta", "gamma", "K", "R", "Nc"))
    lg = math.lgamma
    v = []
    c = np.zeros(K, dtype=np.int64)
    cnt = np.zeros((R, K), dtype=np.int64)
    for i, (z, ts) in enumerate(state):
        ns = tdo.counts(z, K)
        v += [math.log(b + j * a) for j in range(sum(ts))] + [-math.log(b + j) for j in range(Nc)]
        v += [math.log(tio.stirling(nk, a)[tk]) for nk, tk in zip(ns, ts) if nk]
        c += np.array(ts)
        for cc, zc in enumerate(z):
            cnt[LAW["cls"][i * Nc + cc], zc] += 1
    v += [lg(K * gamma), -lg(K * gamma + float(c.sum()))] + [lg(gamma + float(ck)) - lg(gamma) for ck in c]
    for k in range(K):
        v += [lg(R * beta), -lg(R * beta + float(cnt[:, k].sum()))] + [lg(beta + float(x)) - lg(beta) for x in cnt[:, k]]
    return v


def log_p(state) -> float:
    return math.fsum(log_p_terms(state))


@lru_cache(maxsize=None)
def exact_p():
    lp = np.array([log_p(s) for s in enumerate_states()])
    p = np.exp(lp - lp.max())
    return p / p.sum()


def state_of(s, h=None, lik=None) -> State:
    """an enumerated state as a State (h and the matrix all ones unless given)"""
    K, Nc, I = LAW["K"], LAW["Nc"], LAW["I"]
    z = np.concatenate([np.array(x[0]) for x in s]).astype(np.uint32)
    t = np.concatenate([np.array(x[1]) for x in s]).astype(np.uint16)
    n = np.concatenate([tdo.counts(x[0], K) for x in s]).astype(np.uint32)
    return State(K=np.full(I, K, dtype=np.int32), n=n, t=t, T=t.reshape(I, K).sum(axis=1).astype(np.uint32), cust=z,
                 cls=np.array(LAW["cls"], dtype=np.uint32), h=np.ones(I * K) if h is None else h,
                 lik=np.ones((LAW["R"], K)) if lik is None else lik, root=np.full(K, 1.0 / K), alpha=None,
                 bpar=np.full(I, LAW["b"]), beta=LAW["beta"], gamma=LAW["gamma"], a=LAW["a"])


TINY_START = (((0, 1, 0), (2, 1)), ((1, 0, 1), (1, 1)))    # the handover case `tiny`: both dishes in use in both restaurants


def law_start(s=None) -> State:
    """(z, t) drawn from p (or the enumerated state s), then h and the matrix from their conditionals given it: the law
    test's chain starts in its stationary law"""
    rng = np.random.default_rng(LAW_START_SEED)
    st = state_of(enumerate_states()[rng.choice(len(exact_p()), p=exact_p())] if s is None else s)
    st, _ = step(st, "sample_lik", LAW_START_SEED, 0)
    st, _ = step(st, "sample_h", LAW_START_SEED + 1, 0)
    return st


@lru_cache(maxsize=None)
def beta_median(p: float, q: float) -> float:
    """the median of Beta(p, q), by bisection on mpmath's regularised incomplete beta function"""
    import mpmath as mp

    lo, hi = 0.0, 1.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if mp.betainc(p, q, 0, mid, regularized=True) < 0.5:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def count_cell(st: State):
    """(|n_00 - n_10|, T_0 + T_1): what the two restaurants' customers and tables do together; exchanging the dishes' names,
    under which p is symmetric and between whose two images the chain passes only rarely, leaves it as it is"""
    K = LAW["K"]
    return abs(int(st.n[0]) - int(st.n[K])), int(st.T.sum())


def cells(st: State):
    """the statistic of the law test: count_cell, and for either dish k whether the matrix's cell lik[0, k] lies above the
    median of its conditional given the customers, Beta(beta + cnt_0k, beta + cnt_1k) with the counts of both restaurants
    (two classes: a column is one Beta variate).  After an iteration the matrix is a draw from that conditional whatever
    (z, t) are, so under the exact law the two bits are fair coins independent of count_cell -- and a matrix drawn from
    other counts than the state's, or a sweep that read another matrix than the object's, is not"""
    cnt = class_counts(st).astype(np.float64)
    beta = LAW["beta"]
    bits = tuple(int(float(st.lik[0, k]) > beta_median(beta + cnt[0, k], beta + cnt[1, k])) for k in range(LAW["K"]))
    return bits + count_cell(st)


def exact_cells(kept: int = LAW_ITERATIONS // LAW_THIN):
    """(index: cell -> bin, probabilities of the bins) under the exact law.  Cells whose expected count over `kept` states
    is below 10 share the last bin; when that bin stays below 10 the smallest cell kept joins it"""
    acc = {}
    for s, v in zip(enumerate_states(), exact_p()):
        for bits in ((0, 0), (0, 1), (1, 0), (1, 1)):
            key = bits + count_cell(state_of(s))
            acc[key] = acc.get(key, 0.0) + 0.25 * float(v)
    return merge_cells(acc, kept)


def merge_cells(acc, kept: int):
    own = sorted((c for c in acc if kept * acc[c] >= 10.0), key=lambda c: -acc[c])
    rest = sum(v for c, v in acc.items() if c not in own)
    while 0.0 < kept * rest < 10.0:
        rest += acc[own.pop()]
    index = {c: (own.index(c) if c in own else len(own)) for c in acc}
    probs = np.array([acc[c] for c in own] + ([rest] if rest > 0.0 else []))
    return index, probs


def cell_counts(keys, index, bins: int):
    """the counts of the bins over the kept cells `keys`; a cell the law gives no mass counts in the last bin"""
    return np.bincount([index.get(k, bins - 1) for k in keys], minlength=bins).astype(np.float64)


def chi2_pvalue(counts, probs) -> float:
    ex = probs / probs.sum() * counts.sum()
    x, k = float(np.sum((counts - ex) ** 2 / ex)), len(probs) - 1
    try:
        from scipy.stats import chi2

        return float(chi2.sf(x, k))
    except ImportError:  # Wilson-Hilferty, as tests/test_gpu_tdish.py
        z = ((x / k) ** (1.0 / 3.0) - (1.0 - 2.0 / (9.0 * k))) / math.sqrt(2.0 / (9.0 * k))
        return 0.5 * math.erfc(z / math.sqrt(2.0))


def law_chain(law="right", seed=LAW_SEED, iterations=LAW_ITERATIONS, thin=LAW_THIN):
    """the kept states' ((n, t, cust) as bytes, cell) of the four fixed steps from law_start(), every thin-th iteration"""
    kept, worst = run(restrict(PROGRAMS["flat"]), law_start(), iterations, seed, law=law,
                      keep=lambda s: (s.n.tobytes() + s.t.tobytes() + s.cust.tobytes(), cells(s)))
    return kept[thin - 1::thin], worst


def lag1(x) -> float:
    x = np.asarray(x, dtype=np.float64) - np.mean(x)
    return float(np.dot(x[1:], x[:-1]) / np.dot(x, x))


# the law of the wrong chain stale_lik on exact_cells()'s bins: the frequencies of the 15000 kept states of
# law_chain("stale_lik", STALE_SEED, STALE_ITERATIONS), run once on the CPU (a minute); the device's counts are held against
# it, and tests/test_chain_host.py holds the short stale_lik replay against it
STALE_SEED, STALE_ITERATIONS = 7400, 30000
STALE_CELLS = (0.03527, 0.04733, 0.04880, 0.03967, 0.03780, 0.05080, 0.04940, 0.03567, 0.02233, 0.06707, 0.05853, 0.02180,
               0.02327, 0.02227, 0.02613, 0.01960, 0.01280, 0.03687, 0.03667, 0.01347, 0.01313, 0.02033, 0.02127, 0.01313,
               0.00860, 0.03007, 0.03007, 0.00940, 0.14847)
