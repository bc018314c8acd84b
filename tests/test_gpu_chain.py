"""The Gibbs chain of a table-indicator object, as examples/pyp_resample composes it from the object's steps -- the programs
flat (-d -z -L -w -C -K), grouped (-H), tree (-T), missing (-V, with every third class drawn again each iteration) and gauss
(-X), and the held-out calls (-P -Q -F) between the iterations of flat: every step against its oracle on the state the step
before left on the device (tests/ch_oracle.py), what a step does not write left as it was, the joint, the data term and the
prediction after every iteration, and the chain's law against the exact posterior of a model small enough to enumerate.
tests/test_chain_host.py checks the margins of the seeds used here, the target, the power of the law test and of the step
comparison on the CPU."""
import itertools
import math
from functools import lru_cache

import numpy as np
import pytest

import ch_oracle as ch
import gs_oracle as gso
import lj_oracle as lj
import pr_oracle as pro
import ti_oracle as tio
import tl_oracle as tlo
from libstb_amd import capi

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
RES = capi.BPAR_RESIDENT
FIELDS = ch.FIELDS       # (with WRITES, assert_replayed and check_step in ch_oracle: the host tests share them)


@lru_cache(maxsize=None)
def device_vtab(a, N, M):
    """the slab an object holds for discount a, as an oracle VTab: the device's own cells (tests/test_gpu_tdish.py)"""
    v = capi.DeviceVTables(N, M)
    v.fill(a)
    capi.check(capi.lib().stb_fill_status())
    return tio.VTab(v.packed_host(0), N, M)


def call(ti, name, seed, sweep, st):
    """the object's method `name` with the example's arguments on the hyper-parameters of `st`: a dict as ch_oracle.step's"""
    if name == "sweep_dishes":
        info = ti.sweep_dishes(st.a, RES, seed, sweep)
        return dict(skipped=info.skipped, stuck=info.stuck)
    if name == "sweep":
        ti.sweep(st.a, RES, seed, sweep)
        return {}
    if name == "sample_lik":
        ti.sample_lik(st.beta, seed, sweep)
        return {}
    if name == "sample_h":
        ti.sample_h(st.gamma, seed, sweep)
        return {}
    if name == "sample_hgroups":
        shape, scale = ch.PRIOR_ALPHA
        info = ti.sample_hgroups(ch.ALPHA0 if st.alpha is None else 0.0, st.gamma, seed, sweep, flags=capi.HG_SAMPLE_ALPHA,
                                 shape=shape, scale=scale)
        return dict(alpha=info.alpha, tables=info.tables, aux_tables=info.aux_tables)
    if name == "sample_htree":          # alpha NULL from the second call on: what the step before left on the device
        shape, scale = ch.PRIOR_ALPHA
        L = len(st.htoff)
        info = ti.sample_htree([ch.ALPHA0] * L if st.alphas is None else None, st.gamma, seed, sweep, flags=capi.HT_SAMPLE_ALPHA,
                               shape=shape, scale=scale)
        return dict(alphas=tuple(info.alpha)[:L], tables=list(info.tables)[:L], aux_tables=list(info.aux_tables)[:L],
                    rows1=ti.get_htree_level(1))
    if name == "sample_classes":
        info = ti.sample_classes(seed, sweep, ch.class_mask(ti.C))
        return dict(skipped=info.skipped, stuck=info.stuck, drawn=info.drawn)
    if name == "generate":
        si, ci = ti.generate(st.a, RES, seed, sweep)
        assert si.customers == ti.C
        return dict(skipped=ci.skipped, stuck=ci.stuck, drawn=ci.drawn, seat=(si.skipped, si.impossible, si.stuck))
    if name == "sample_gauss":
        info = ti.sample_gauss(ch.gauss_prior(st), seed, sweep)
        return dict(skipped=info.skipped, dead=info.dead)
    if name == "sampleb_groups":
        shape, scale = ch.PRIOR_B
        bgrp, info = ti.sampleb_groups(st.a, shape, scale, seed, sweep)
        return dict(bgrp=bgrp, kept=info.kept_groups)
    shape, scale = ch.PRIOR_BETA if name == "sample_beta" else ch.PRIOR_GAMMA
    fn, s = (ti.sample_beta, st.beta) if name == "sample_beta" else (ti.sample_gamma, st.gamma)
    info = fn(s, shape, scale, seed, sweep)
    return dict(s=info.s, count=info.count, aux_tables=info.aux_tables, nonempty=info.nonempty)


def carry(st, method, got):
    """the hyper-parameters a step's info reports, which no getter returns, into the State the next fetch starts from"""
    if method == "sample_beta":
        return st.replace(beta=got["s"])
    if method == "sample_gamma":
        return st.replace(gamma=got["s"])
    if method == "sample_hgroups":
        return st.replace(alpha=got["alpha"])
    if method == "sample_htree":
        return st.replace(alphas=got["alphas"], alpha=got["alphas"][0])
    return st


def fed(method, after, got):
    """what of the device's outcome the replay is fed for the draws downstream of it"""
    if method == "sample_hgroups":
        return dict(root_new=after.root, alpha_new=got["alpha"])
    if method == "sample_htree":
        return dict(root_new=after.root, alpha_new=got["alphas"], rows_new=after.hrows)
    if method == "sample_gauss":
        return dict(mu_new=after.mu, tau_new=after.tau)
    return {}


def exact_loglik(cnt, lik):
    """(sum cnt log lik, sum |cnt log lik|) in mpmath (tests/test_gpu_tlik.py)"""
    import mpmath as mp

    nz = cnt > 0
    x = [mp.mpf(float(c)) * mp.log(mp.mpf(float(l))) for c, l in zip(cnt[nz], lik[nz])]
    return float(mp.fsum(x)), float(mp.fsum(abs(v) for v in x))


def check_joint(ti, st, where):
    """the log joint with h and the indicators against the truth, term by term (tests/test_gpu_logjoint.py); returns the
    largest error over its bar"""
    N, M = st.bounds()
    tot, Li, info = ti.logjoint(st.a, RES, indicators=True)
    tr = lj.truth(st.K, st.n, st.t, st.h, st.a, st.bpar, lj.Tables(st.a, N, M), True)
    worst = 0.0
    for k, g in (("pairs", info.pairs), ("base", info.base), ("restaurants", info.restaurants), ("binom", info.binom),
                 ("total", tot)):
        assert lj.within(g, *tr[k]), (where, k, g, tr[k])
        if math.isfinite(g) and tr[k][1] > 0.0:
            worst = max(worst, abs(g - tr[k][0]) / tr[k][1])
    assert all(lj.within(g, w, b) for g, w, b in zip(Li, tr["Li"], tr["Li_bar"])), where
    assert info.outside == 0 and info.impossible == 0 and info.t_mismatch == 0 and math.isfinite(tot), where
    return worst


def check_iteration(ti, st, where, program):
    """the joint, the data term and the prediction of the state an iteration left; returns the largest error over its bar"""
    worst = 0.0
    if program in ("flat", "grouped", "missing"):
        flat = program != "grouped"
        flags = capi.CJ_INDICATORS | capi.CJ_DATA | (capi.CJ_FLAT if flat else capi.CJ_ROOT)
        tot, ci = ti.logjoint_collapsed(st.a, RES, 1.0 if flat else 0.0, st.gamma, st.beta, flags)
        tr = ch.collapsed_truth(st, indicators=True, flat=flat)
        for k in ("pairs", "restaurants", "binom", "tables", "data", "root"):
            assert lj.within(getattr(ci, k), *tr[k]), (where, k, getattr(ci, k), tr[k])
            if tr[k][1] > 0.0:
                worst = max(worst, abs(getattr(ci, k) - tr[k][0]) / tr[k][1])
        assert lj.within(tot, *tr["total"]), (where, tot, tr["total"])
        assert ci.lj.outside == 0 and ci.lj.impossible == 0 and ci.lj.t_mismatch == 0 and ci.root_left_out == 0, where
        assert ci.dm_tables.count == int(st.T.sum()) and ci.dm_data.count == len(st.cust), where
    else:
        worst = max(worst, check_joint(ti, st, where))
    if program == "tree" and len(st.htoff) > 1:           # the grouped formula is not a deeper tree's model
        with pytest.raises(capi.StbError):
            ti.logjoint_collapsed(st.a, RES, 0.0, st.gamma, st.beta, capi.CJ_INDICATORS | capi.CJ_DATA | capi.CJ_ROOT)
    if program == "gauss":
        # the evidence on statistics replayed from the fetched cust, the data term on the fetched parameters: each
        # against the 40-digit truth within its derived bar (tests/gs_oracle.py)
        n, mean, Q, _ = gso.stats(st.x, st.cust, int(st.K.max()))
        got, want, bar = ti.gauss_logml(ch.gauss_prior(st)), float(gso.mp_logml(n, mean, Q, st.gprior)), gso.logml_bar(n, mean, Q, st.gprior)
        assert abs(got - want) <= bar, (where, "logml", got, want, bar)
        worst = max(worst, abs(got - want) / bar)
        got, want, bar = ti.gauss_loglik(), float(gso.mp_loglik(st.x, st.cust, st.mu, st.tau)), gso.loglik_bar(st.x, st.cust, st.mu, st.tau)
        assert abs(got - want) <= bar, (where, "loglik", got, want, bar)
        worst = max(worst, abs(got - want) / bar)
    else:
        # the data term: test_gpu_tlik's bar against the exactly rounded sum, for the device and for tl_oracle.loglik
        cnt = ch.class_counts(st)
        rows, stride = cnt.shape
        got, imp = ti.loglik()
        want, mag = exact_loglik(cnt, st.lik)
        bar = U * (258 + math.ceil(rows / 256) + stride) * mag
        rep, rep_imp = tlo.loglik(cnt, st.lik)
        assert imp == rep_imp == 0 and abs(got - want) <= bar and abs(rep - want) <= bar, (where, got, rep, want, bar)
        worst = max(worst, abs(got - want) / bar)
        assert np.array_equal(ti.class_counts(), cnt[:ti.rows]) and ti.rows >= int(st.cls.max()) + 1, where
        assert not cnt[ti.rows:].any(), where
    # the prediction: theta bit for bit (tests/test_gpu_predict.py)
    theta, _, _ = pro.theta_replay(st.K, st.n, st.t, st.h, st.a, st.bpar)
    Kmax = int(st.K.max())
    assert np.array_equal(ti.predict(st.a, RES), theta[:, :Kmax]), where
    return worst


def replayed_chain(name, program, seed, each=None):
    """the object's chain of (name, program), every step against its oracle on the state the step before left on the
    device and every iteration's state against check_iteration; each(it, ti, st), when given, runs after every iteration.
    Returns the State after every iteration"""
    st = ch.case(name, program)
    cpu, worst = ch.run(program, st, ch.ITERATIONS, seed, a_at=ch.A_CHANGE)
    assert worst > 1e-7
    states, over_step, over_it = [], 0.0, 0.0
    ti = ch.make_object(st)
    try:
        for it in range(-1 if ch.PROLOGUES.get(program) else 0, ch.ITERATIONS):      # -1: the prologue, at sweep 0
            if it in ch.A_CHANGE:
                st = st.replace(a=ch.A_CHANGE[it])
            for method, off in (ch.PROGRAMS[program] if it >= 0 else ch.PROLOGUES[program]):
                where = "%s %s iteration %d %s" % (name, program, it, method)
                before = ch.fetch(ti, st)
                got = call(ti, method, seed + off, max(it, 0), before)
                st = carry(st, method, got)
                after = ch.fetch(ti, st)
                want, info = ch.step(before, method, seed + off, max(it, 0), vtab=device_vtab, **fed(method, after, got))
                unfed = ch.step(before, method, seed + off, max(it, 0), vtab=device_vtab)[0] if method == "sample_htree" else None
                over_step = max(over_step, ch.check_step(method, where, before, after, want, got, info, unfed))
            if it < 0:
                continue
            last = ch.fetch(ti, st)
            over_it = max(over_it, check_iteration(ti, last, "%s %s iteration %d" % (name, program, it), program))
            if each is not None:
                each(it, ti, last)
            states.append(last)
        for f in ch.INTEGERS:                             # the pure CPU chain: the margins of test_chain_host.py apply
            assert np.array_equal(getattr(states[-1], f), getattr(cpu[-1], f)), (name, program, f)
    finally:
        ti.free()
    print(name, program, "worst error over bar: a step's replay %.3g, an iteration's totals %.3g" % (over_step, over_it))
    return states


@pytest.mark.parametrize("name,program", list(ch.CASE_SEEDS))
def test_every_step_acts_on_the_state_the_last_one_left(name, program):
    states = replayed_chain(name, program, ch.CASE_SEEDS[name, program])
    assert len(states) == ch.ITERATIONS
    if program == "missing":                              # the classes are state the chain writes
        assert len({s.cls.tobytes() for s in states}) > 1


def test_a_one_level_tree_is_the_grouped_step_through_the_object():
    """(tiny, tree) against (tiny, grouped) on the tree case's seed: h, the root, the concentration and the integers after
    every iteration, bit for bit"""
    seed = ch.CASE_SEEDS["tiny", "tree"]
    out = {}
    for program in ("tree", "grouped"):
        st = ch.case("tiny", program)
        ti = ch.make_object(st)
        rows = []
        try:
            for it in range(ch.ITERATIONS):
                if it in ch.A_CHANGE:
                    st = st.replace(a=ch.A_CHANGE[it])
                for method, off in ch.PROGRAMS[program]:
                    st = carry(st, method, call(ti, method, seed + off, it, st))
                rows.append(ch.fetch(ti, st))
        finally:
            ti.free()
        out[program] = rows
    for it, (x, y) in enumerate(zip(out["tree"], out["grouped"])):
        for f in ch.INTEGERS + ("h", "root", "lik", "bpar"):
            assert ch.same(getattr(x, f), getattr(y, f)), (it, f)
        assert x.alphas == (y.alpha,) and x.beta == y.beta, (it, x.alphas, y.alpha)
    assert len({x.alpha for x in out["tree"]}) == ch.ITERATIONS


def dev(x, dtype):
    import torch

    view = {np.uint64: np.int64, np.uint32: np.int32, np.uint16: np.int16}.get(dtype)
    x = np.array(x, dtype=dtype, order="C")
    return torch.as_tensor(x.view(view) if view else x, device="cuda")


def raw_heldout(st, hoff, hcls, seed, sweep, acc, samples):
    """the raw calls on the fetched state `st`: (p, the state's (total, H_i), the running estimate's after p went into acc,
    heldout_seq's, heldout_pf's), acc the device tensor the running sum lives in"""
    koff = dev(np.concatenate([[0], np.cumsum(st.K.astype(np.int64))]), np.uint64)
    args = (st.a, dev(st.bpar, np.float64), koff, dev(st.n, np.uint32), dev(st.t, np.uint16))
    d_h, d_hoff, d_hcls, d_lik = dev(st.h, np.float64), dev(hoff, np.uint64), dev(hcls, np.uint32), dev(st.lik, np.float64)
    R, tau = ch.HELDOUT_PARTICLES, ch.HELDOUT_TAU
    _, p = capi.predict_dishes(*args, d_h, 0, d_hoff, d_hcls, d_lik)
    one = capi.heldout_loglik(p, d_hoff)
    capi.predict_dishes(*args, d_h, 0, d_hoff, d_hcls, d_lik, p=acc, accumulate=True)
    run = capi.heldout_loglik(acc, d_hoff, samples)
    lw, _, _, _ = capi.seat_customers(*args, d_hoff, d_h, 0, d_hcls, d_lik, R, seed=seed, sweep=sweep)
    seq = capi.seat_loglik(lw)
    o = capi.seat_filter(*args, d_hoff, d_h, 0, d_hcls, d_lik, R, tau, seed, sweep, want_w=False, want_states=False)
    pf = capi.seat_loglik(o["Hi"].reshape(-1, 1))
    return p.cpu().numpy(), one, run, seq, (pf[0], o["Hi"], pf[2])


def test_the_heldout_calls_between_iterations_leave_the_chain_on_its_path():
    """(mixed, flat) with heldout, heldout(accumulate), heldout_seq and heldout_pf after every iteration: every step still
    against its oracle, every call leaves every field as it was and answers as the raw calls on the fetched state, the
    accumulator is the running sum of the raw p in iteration order, and the chain ends where the CPU chain does and where
    the device's own chain without these calls does"""
    import torch

    name, program = ch.HELDOUT_CASE
    seed = ch.CASE_SEEDS[name, program]
    hoff, hcls = ch.heldout_set(ch.case(name, program))
    Hc = int(hoff[-1])
    assert 0 in np.diff(hoff.astype(np.int64)) and 6 in np.diff(hoff.astype(np.int64))
    acc = torch.zeros(Hc, dtype=torch.float64, device="cuda")
    total = np.zeros(Hc)
    ps = []

    def bits(x, y):
        return ch.same(np.asarray(x, dtype=np.float64), np.asarray(y.cpu().numpy() if hasattr(y, "cpu") else y, dtype=np.float64))

    def each(it, ti, st):
        nonlocal total
        if it == 0:
            ti.set_heldout(hoff, hcls)
        where = "held-out calls after iteration %d" % it
        sd, sw = seed + ch.HELDOUT_OFFSET, it * 4096
        p, one, run, seq, pf = raw_heldout(st, hoff, hcls, sd, sw, acc, it + 1)
        ps.append(p)
        total = p if it == 0 else total + p               # one lane owns a customer: the values added in call order
        got = [ti.heldout(st.a, RES), ti.heldout(st.a, RES, accumulate=True),
               ti.heldout_seq(st.a, RES, ch.HELDOUT_PARTICLES, sd, sw),
               ti.heldout_pf(st.a, RES, ch.HELDOUT_PARTICLES, ch.HELDOUT_TAU, sd, sw)]
        now = ch.fetch(ti, st)
        for f in FIELDS:
            assert ch.same(getattr(now, f), getattr(st, f)), (where, f, "was written")
        for what, g, w in zip(("heldout", "heldout accumulate", "heldout_seq", "heldout_pf"), got, (one, run, seq, pf)):
            assert bits(g[0], w[0]) and bits(g[1], w[1]) and math.isfinite(g[0]), (where, what, g[0], w[0])
            assert g[2].impossible == w[2].impossible == 0 and g[2].customers == Hc and g[2].skipped == 0, (where, what)
        accd, S = ti.heldout_get()
        assert S == it + 1 and bits(accd, total) and bits(accd, acc), where
        assert it == 0 or not np.array_equal(ps[-1], ps[-2]), where

    states = replayed_chain(name, program, seed, each)
    plain = ch.case(name, program)
    tj = ch.make_object(plain)
    try:
        for it in range(ch.ITERATIONS):
            if it in ch.A_CHANGE:
                plain = plain.replace(a=ch.A_CHANGE[it])
            for method, off in ch.PROGRAMS[program]:
                plain = carry(plain, method, call(tj, method, seed + off, it, plain))
            now = ch.fetch(tj, plain)
            for f in FIELDS:
                assert ch.same(getattr(now, f), getattr(states[it], f)), (it, f)
            assert (now.beta, now.gamma) == (states[it].beta, states[it].gamma), it
    finally:
        tj.free()


def test_the_chain_keeps_the_exact_posterior():
    st0 = ch.law_start()
    program = ch.restrict(ch.PROGRAMS["flat"])
    replay, worst = ch.law_chain("right")
    index, probs = ch.exact_cells()
    calls, kept = 0, []
    ti = ch.make_object(st0)
    try:
        for it in range(ch.LAW_ITERATIONS):
            for method, off in program:
                call(ti, method, ch.LAW_SEED + off, it, st0)
                calls += 1
            if (it + 1) % ch.LAW_THIN == 0:
                s = ch.fetch(ti, st0)
                kept.append((s.n.tobytes() + s.t.tobytes() + s.cust.tobytes(), ch.cells(s)))
    finally:
        ti.free()
    assert calls <= 6000 and len(kept) == len(replay) == ch.LAW_ITERATIONS // ch.LAW_THIN and worst > 1e-7
    differ = [j for j, (g, w) in enumerate(zip(kept, replay)) if g[0] != w[0]]
    assert not differ, ("the device's chain leaves the replay's at kept state", differ[0])
    counts = ch.cell_counts([c for _, c in kept], index, len(probs))
    pv = ch.chi2_pvalue(counts, probs)
    bad = ch.chi2_pvalue(counts, np.array(ch.STALE_CELLS))
    print("bins", len(probs), "p-value against the exact posterior", pv, "against the law of stale_lik", bad)
    assert pv > 1e-3
    assert bad < 1e-6


def test_the_devices_joint_ranks_states_as_the_enumeration_does():
    """20 enumerated states of the tiny model: the object's collapsed joint (flat, data term, (n, t) form) plus the Gamma
    prior of every b -- the scalar the header leaves to the caller, here the same for every state -- against log p, pair by
    pair within the two states' bars of ch_oracle.collapsed_truth and 4 u sum |term| for the doubles of log p"""
    states = ch.enumerate_states()
    shape, scale = ch.PRIOR_B
    b = ch.LAW["b"]
    prior = ch.LAW["I"] * ((shape - 1.0) * math.log(b) - b / scale - math.lgamma(shape) - shape * math.log(scale))
    rows = []
    for j in list(range(3, 324, 16))[:20]:            # the probes of tests/test_chain_host.py
        st = ch.state_of(states[j])
        ti = ch.make_object(st)
        try:
            tot, ci = ti.logjoint_collapsed(st.a, st.bpar, 1.0, st.gamma, st.beta, capi.CJ_FLAT | capi.CJ_DATA)
        finally:
            ti.free()
        terms = ch.log_p_terms(states[j])
        bar = ch.collapsed_truth(st, indicators=False, flat=True)["total"][1]
        assert ci.binom == 0.0 and ci.root == 0.0 and math.isfinite(tot)
        rows.append((tot + prior, math.fsum(terms), bar + 4.0 * U * sum(abs(x) for x in terms) + 2.0 * U * abs(tot + prior)))
    assert len(rows) == 20
    worst = 0.0
    for (g1, p1, b1), (g2, p2, b2) in itertools.combinations(rows, 2):
        worst = max(worst, abs((g1 - g2) - (p1 - p2)) / (b1 + b2))
        assert abs((g1 - g2) - (p1 - p2)) <= b1 + b2, (g1, g2, p1, p2)
    print("largest error over bar", worst)
