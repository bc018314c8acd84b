"""The Gibbs chain of a table-indicator object, as examples/pyp_resample -d -z -L -w -C -K [-H] composes it from the
object's steps: every step against its oracle on the state the step before left on the device (tests/ch_oracle.py), what
a step does not write left as it was, the collapsed joint, the data term and the prediction after every iteration, and the
chain's law against the exact posterior of a model small enough to enumerate.  tests/test_chain_host.py checks the
margins of the seeds used here, the target and the power of the law test on the CPU."""
import itertools
import math
from functools import lru_cache

import numpy as np
import pytest

import ch_oracle as ch
import lj_oracle as lj
import pr_oracle as pro
import ti_oracle as tio
import tl_oracle as tlo
from libstb_amd import capi

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
RES = capi.BPAR_RESIDENT
FIELDS = ("n", "t", "T", "cust", "h", "lik", "root", "bpar")
WRITES = {"sweep_dishes": ("n", "t", "T", "cust"), "sweep": ("t", "T"), "sample_lik": ("lik",), "sample_h": ("h",),
          "sample_hgroups": ("h", "root"), "sampleb_groups": ("bpar",), "sample_beta": (), "sample_gamma": ()}


@lru_cache(maxsize=None)
def device_vtab(a, N, M):
    """the slab an object holds for discount a, as an oracle VTab: the device's own cells (tests/test_gpu_tdish.py)"""
    v = capi.DeviceVTables(N, M)
    v.fill(a)
    capi.check(capi.lib().stb_fill_status())
    return tio.VTab(v.packed_host(0), N, M)


def assert_replayed(got, want, what):
    """the single-step tests' standing bar (tests/test_gpu_tlik.py): 1e-10 relative where the replay's value is >= 1e-280,
    1e-290 absolute below; no cell left out"""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    assert got.shape == want.shape and not np.isnan(got).any(), what
    big = want >= 1e-280
    err = np.abs(got - want)
    rel = float((err[big] / want[big]).max()) if big.any() else 0.0
    small = float(err[~big].max()) if (~big).any() else 0.0
    assert rel <= 1e-10, (what, rel)
    assert small <= 1e-290, (what, small)


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
    if name == "sampleb_groups":
        shape, scale = ch.PRIOR_B
        bgrp, info = ti.sampleb_groups(st.a, shape, scale, seed, sweep)
        return dict(bgrp=bgrp, kept=info.kept_groups)
    shape, scale = ch.PRIOR_BETA if name == "sample_beta" else ch.PRIOR_GAMMA
    fn, s = (ti.sample_beta, st.beta) if name == "sample_beta" else (ti.sample_gamma, st.gamma)
    info = fn(s, shape, scale, seed, sweep)
    return dict(s=info.s, count=info.count, aux_tables=info.aux_tables, nonempty=info.nonempty)


def exact_loglik(cnt, lik):
    """(sum cnt log lik, sum |cnt log lik|) in mpmath (tests/test_gpu_tlik.py)"""
    import mpmath as mp

    nz = cnt > 0
    x = [mp.mpf(float(c)) * mp.log(mp.mpf(float(l))) for c, l in zip(cnt[nz], lik[nz])]
    return float(mp.fsum(x)), float(mp.fsum(abs(v) for v in x))


def check_step(name, where, before, after, want, got, info):
    """one step's outcome `after` (info `got`) against the oracle's `want` (info `info`) on `before`"""
    assert ch.margin_of(info) > 1e-9, (where, "a draw of this step sits on a tie", ch.margin_of(info))
    for f in FIELDS:                                      # what the step's contract says it does not write: to the bit
        if f not in WRITES[name]:
            assert np.array_equal(getattr(after, f), getattr(before, f)), (where, f, "was written")
    for f in ("n", "t", "T", "cust"):                     # integers: bit for bit
        assert np.array_equal(getattr(after, f), getattr(want, f)), (where, f)
    for k in ("skipped", "stuck", "tables", "aux_tables", "count", "nonempty", "kept"):
        if k in info:
            assert got[k] == info[k], (where, k, got[k], info[k])
    rows, Kmax = after.lik.shape[0], int(after.K.max())
    if name == "sample_lik":
        assert_replayed(after.lik, want.lik, where + " lik")
        assert all(abs(math.fsum(after.lik[:, k]) - 1.0) <= 2.0 * U * rows for k in range(after.lik.shape[1])), where
    if name in ("sample_h", "sample_hgroups"):
        assert_replayed(after.h, want.h, where + " h")
        koff = np.concatenate([[0], np.cumsum(after.K)])
        full = [i for i in range(len(after.K)) if after.K[i] == Kmax]
        assert full and all(abs(math.fsum(after.h[koff[i]:koff[i + 1]]) - 1.0) <= 2.0 * U * Kmax for i in full), where
    if name == "sample_hgroups":
        assert_replayed(after.root, want.root, where + " root")
        assert abs(math.fsum(after.root) - 1.0) <= 2.0 * U * Kmax, where
        assert abs(got["alpha"] - want.alpha) <= 1e-10 * want.alpha and got["alpha"] != before.alpha, (where, got["alpha"], want.alpha)
    if name == "sampleb_groups":
        assert np.all(np.abs(after.bpar - want.bpar) <= 1e-10 * want.bpar), (where, "bpar")
        assert np.all(np.abs(got["bgrp"] - info["bgrp"]) <= 1e-10 * info["bgrp"]), (where, "bgrp")
        assert not np.array_equal(after.bpar, before.bpar), where
    if name in ("sample_beta", "sample_gamma"):
        assert abs(got["s"] - info["s"]) <= 1e-10 * info["s"] and got["s"] != (before.beta if name == "sample_beta" else before.gamma), where


def check_iteration(ti, st, where, flat):
    """the collapsed joint, the data term and the prediction of the state an iteration left"""
    flags = capi.CJ_INDICATORS | capi.CJ_DATA | (capi.CJ_FLAT if flat else capi.CJ_ROOT)
    tot, ci = ti.logjoint_collapsed(st.a, RES, 1.0 if flat else 0.0, st.gamma, st.beta, flags)
    tr = ch.collapsed_truth(st, indicators=True, flat=flat)
    for k in ("pairs", "restaurants", "binom", "tables", "data", "root"):
        assert lj.within(getattr(ci, k), *tr[k]), (where, k, getattr(ci, k), tr[k])
    assert lj.within(tot, *tr["total"]), (where, tot, tr["total"])
    assert ci.lj.outside == 0 and ci.lj.impossible == 0 and ci.lj.t_mismatch == 0 and ci.root_left_out == 0, where
    assert ci.dm_tables.count == int(st.T.sum()) and ci.dm_data.count == len(st.cust), where
    # the data term: test_gpu_tlik's bar against the exactly rounded sum, for the device and for tl_oracle.loglik
    cnt = ch.class_counts(st)
    rows, stride = cnt.shape
    got, imp = ti.loglik()
    want, mag = exact_loglik(cnt, st.lik)
    bar = U * (258 + math.ceil(rows / 256) + stride) * mag
    rep, rep_imp = tlo.loglik(cnt, st.lik)
    assert imp == rep_imp == 0 and abs(got - want) <= bar and abs(rep - want) <= bar, (where, got, rep, want, bar)
    assert np.array_equal(ti.class_counts(), cnt[:int(st.cls.max()) + 1]), where
    # the prediction: theta bit for bit (tests/test_gpu_predict.py)
    theta, _, _ = pro.theta_replay(st.K, st.n, st.t, st.h, st.a, st.bpar)
    Kmax = int(st.K.max())
    assert np.array_equal(ti.predict(st.a, RES), theta[:, :Kmax]), where


@pytest.mark.parametrize("name,program", list(ch.CASE_SEEDS))
def test_every_step_acts_on_the_state_the_last_one_left(name, program):
    seed = ch.CASE_SEEDS[name, program]
    st = ch.case(name, program)
    cpu, worst = ch.run(program, st, ch.ITERATIONS, seed, a_at=ch.A_CHANGE)
    assert worst > 1e-7
    ti = ch.make_object(st)
    try:
        for it in range(ch.ITERATIONS):
            if it in ch.A_CHANGE:
                st = st.replace(a=ch.A_CHANGE[it])
            for method, off in ch.PROGRAMS[program]:
                where = "%s %s iteration %d %s" % (name, program, it, method)
                before = ch.fetch(ti, st)
                got = call(ti, method, seed + off, it, before)
                if method == "sample_beta":
                    st = st.replace(beta=got["s"])
                elif method == "sample_gamma":
                    st = st.replace(gamma=got["s"])
                elif method == "sample_hgroups":
                    st = st.replace(alpha=got["alpha"])
                after = ch.fetch(ti, st)
                fed = dict(root_new=after.root, alpha_new=got["alpha"]) if method == "sample_hgroups" else {}
                want, info = ch.step(before, method, seed + off, it, vtab=device_vtab, **fed)
                check_step(method, where, before, after, want, got, info)
            check_iteration(ti, ch.fetch(ti, st), "%s %s iteration %d" % (name, program, it), program == "flat")
        last = ch.fetch(ti, st)
        for f in ("n", "t", "T", "cust"):                 # the pure CPU chain: the margins of test_chain_host.py apply
            assert np.array_equal(getattr(last, f), getattr(cpu[-1], f)), (name, program, f)
    finally:
        ti.free()


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
