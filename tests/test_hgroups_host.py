"""The grouped base-weight step without a GPU: the entry points exist, the replay cases of tests/test_gpu_hgroups.py sit on
no tie, the replayed auxiliary tables follow the exact Antoniak law, the replayed chain keeps the root's posterior (and two
wrong laws do not), and the draws depend on (seed, sweep, cell) alone."""
import math
import os
import re
from functools import lru_cache

import numpy as np
import pytest

import hh_oracle as hho
import hq_oracle as hqo
from libstb_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stb_sample_hgroups", "stb_tindic_set_hgroups", "stb_tindic_set_hroot", "stb_tindic_get_hroot",
         "stb_tindic_sample_hgroups")
MARGIN = 1e-9        # the Gamma acceptance tests (test_tlik_host's bar)
MARGIN_Y = 1e-13     # the Bernoulli comparisons, relative: both sides are the same few roundings of the same doubles


def test_entry_points_exist():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "stb_hip.h")).read()
    source = open(os.path.join(ROOT, "libstb_amd", "capi.py")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert 'sig("%s"' % name in source, name
    for name in ("set_hgroups", "set_hroot", "get_hroot", "sample_hgroups"):
        assert hasattr(capi.TableIndicators, name), name
    assert hasattr(capi, "sample_hgroups")
    assert C_sizes() == (48, 32)
    # refused before any device is touched
    opts = capi.HGroupsOpts(1.0, 1.0, 1.0, 1.0, None, 0, 0)
    info = capi.HGroupsInfo()
    assert L.stb_sample_hgroups(3, None, None, 2, 3, None, capi.C.byref(opts), None, None, None, None, None, 1, 0, None,
                                capi.C.byref(info)) != 0 and "required" in capi.last_error()
    assert L.stb_tindic_sample_hgroups(None, capi.C.byref(opts), 1, 0, None) != 0 and "null object" in capi.last_error()
    assert L.stb_tindic_set_hgroups(None, 0, None) != 0 and "null object" in capi.last_error()
    assert L.stb_tindic_set_hroot(None, None) != 0 and "null object" in capi.last_error()
    assert L.stb_tindic_get_hroot(None, None) != 0 and "null" in capi.last_error()


def C_sizes():
    return capi.C.sizeof(capi.HGroupsOpts), capi.C.sizeof(capi.HGroupsInfo)


@lru_cache(maxsize=None)
def replayed(name):
    return hho.replay_case(name)


@pytest.mark.parametrize("name", list(hho.CASES))
def test_replay_cases_sit_on_no_tie(name):
    c, out = hho.case(name), replayed(name)
    print(name, "margins: gamma", out["margin_gamma"], "bernoulli", out["margin_y"], "tables", out["tables"], "aux", out["aux_tables"])
    assert out["margin_gamma"] >= MARGIN and out["margin_y"] >= MARGIN_Y
    assert c["gamma"].min() >= 0.5 and (c["alpha"] * c["root"]).min() >= 0.5
    cg = out["c"]
    assert (cg > 257).any() and (cg == 257).any() and (cg == 258).any() and (cg == 1).any() and (cg == 0).any()
    assert set(np.unique(c["K"])) >= ({1, 2, 1024} if c["Kmax"] == 1024 else set(hho.REPLAY_K))
    if c["goff"] is not None:
        sizes = np.diff(c["goff"].astype(np.int64))
        assert tuple(sizes[:7]) == hho.RANGE_SIZES and cg[6].sum() == 0 and cg[5].sum() == 0
    U = 2.0 ** -53
    for row in list(out["hgrp"]) + ([] if c["flags"] & hho.KEEP_ROOT else [out["root"]]):
        assert abs(math.fsum(row) - 1.0) <= 2.0 * U * c["Kmax"]
    assert out["m"].min() >= 0 and np.all(out["m"] <= cg) and np.all((out["m"] >= 1) == (cg >= 1))
    assert out["alpha"] > 0 and (out["alpha"] != c["alpha"]) == bool(c["flags"] & hho.SAMPLE_ALPHA)


def chi2_sf(x, k):
    """the upper tail of chi-square with k degrees of freedom (regularised upper incomplete gamma, by series / fraction)"""
    a, x = 0.5 * k, 0.5 * x
    if x <= 0:
        return 1.0
    if x < a + 1.0:
        term = total = 1.0 / a
        n = a
        while abs(term) > 1e-17 * abs(total):
            n += 1.0
            term *= x / n
            total += term
        return 1.0 - total * math.exp(-x + a * math.log(x) - math.lgamma(a))
    b, c, d = x + 1.0 - a, 1e300, 1.0 / (x + 1.0 - a)
    h = d
    for i in range(1, 500):
        an = -i * (i - a)
        b += 2.0
        d = 1.0 / (an * d + b) if an * d + b != 0 else 1e300
        c = b + an / c if c != 0 else 1e-300
        h *= d * c
        if abs(d * c - 1.0) < 1e-16:
            break
    return h * math.exp(-x + a * math.log(x) - math.lgamma(a))


def test_replayed_tables_follow_the_antoniak_law():
    # every (c, w) of the grid in one step's matrix, 400 sweeps pooled: the counts of m against the Stirling-number pmf
    cs, ws = np.arange(0, 9), np.array([0.5, 1.0, 3.7])
    c = np.repeat(cs[:, None], len(ws), axis=1)
    sweeps = 400
    hist = np.zeros((len(cs), len(ws), 10))
    for s in range(sweeps):
        m, _ = hho.aux_tables(c, ws, 4242, s)
        for a in range(len(cs)):
            for b in range(len(ws)):
                hist[a, b, m[a, b]] += 1
    chi, dof = 0.0, 0
    for a, cc in enumerate(cs):
        for b, w in enumerate(ws):
            p = hho.antoniak_pmf(int(cc), float(w))
            assert abs(p.sum() - 1.0) < 1e-12
            assert hist[a, b, cc + 1:].sum() == 0 and (cc == 0 or hist[a, b, 0] == 0)
            live = p * sweeps >= 5.0                  # (cells of fewer than 5 expected are pooled into one)
            obs = np.concatenate([hist[a, b, :cc + 1][live], [hist[a, b, :cc + 1][~live].sum()]])
            exp = np.concatenate([p[live], [p[~live].sum()]]) * sweeps
            keep = exp > 0
            if keep.sum() >= 2:
                chi += float((((obs - exp) ** 2)[keep] / exp[keep]).sum())
                dof += int(keep.sum()) - 1
    pv = chi2_sf(chi, dof)
    print("chi-square", chi, "dof", dof, "p", pv)
    assert pv > 1e-3
    # it can fail: the same counts against the pmf of another w
    p_wrong = hho.antoniak_pmf(8, 1.0)
    live = p_wrong * sweeps >= 5.0
    obs, exp = hist[8, 2, :9][live], p_wrong[live] * sweeps
    assert chi2_sf(float(((obs - exp) ** 2 / exp).sum()), int(live.sum()) - 1) < 1e-9


@pytest.mark.parametrize("law", hho.LAWS)
def test_the_replayed_chain_keeps_the_roots_posterior(law):
    r0 = hho.root_chain(hho.LAW_SEED, law)
    assert len(r0) == hho.LAW_STEPS // hho.LAW_THIN
    pv = hho.law_pvalue(r0)
    print(law, "KS p-value", pv, "mean r_0", r0.mean())
    if law == "right":
        assert pv > 1e-3
    else:
        assert pv < 1e-9


def test_the_roots_posterior_is_a_distribution():
    post = hho.RootPosterior(hho.LAW_C, hho.LAW_ALPHA, hho.LAW_GAMMA)
    assert post.cdf[0] == 0.0 and post.cdf[-1] == 1.0 and np.all(np.diff(post.cdf) >= 0)
    # with no tables the posterior is the prior Beta(0.7, 1.3): its mean 0.35
    prior = hho.RootPosterior(np.zeros((3, 2), dtype=np.int64), 3.0, hho.LAW_GAMMA)
    r = 1.0 / (1.0 + np.exp(-prior.x))
    mean = float(np.sum(0.5 * (r[1:] + r[:-1]) * np.diff(prior.cdf)))
    assert abs(mean - 0.35) < 1e-4


def test_the_draws_depend_on_seed_sweep_and_cell_alone():
    K = np.array([3, 1, 3, 2], dtype=np.int32)
    t = np.array([4, 0, 9, 2, 1, 1, 300, 5, 0], dtype=np.uint16)
    root, gamma = np.array([0.6, 0.9, 1.4]), np.array([0.5, 1.0, 2.0])
    a = hho.replay(K, t, None, root, 2.0, gamma, 11, 2)
    b = hho.replay(K, t, None, root, 2.0, gamma, 11, 3)
    c = hho.replay(K, t, None, root, 2.0, gamma, 12, 2)
    for o in (b, c):
        assert not np.array_equal(a["hgrp"], o["hgrp"]) and not np.array_equal(a["root"], o["root"])
        assert np.array_equal(a["c"], o["c"])
    # ranges of one restaurant each are the same groups
    d = hho.replay(K, t, np.arange(5), root, 2.0, gamma, 11, 2)
    for name in ("c", "m", "root", "hgrp", "h"):
        assert np.array_equal(a[name], d[name]), name
    # a cell's auxiliary tables and group variate are the same whatever lies around it: the first two groups alone
    e = hho.replay(K[:2], t[:4], None, root, 2.0, gamma, 11, 2, flags=hho.KEEP_ROOT)
    f = hho.replay(K, t, None, root, 2.0, gamma, 11, 2, flags=hho.KEEP_ROOT)
    assert np.array_equal(e["m"], f["m"][:2]) and np.array_equal(e["hgrp"], f["hgrp"][:2])
    # the root's stream is not a group's: root cell k and group cell e = k differ
    assert not np.array_equal(hho.root_keys(11, 2, 3), __import__("tl_oracle").cell_keys(11, 2, 3))
    # pairs of a restaurant are its group's first K_i weights
    assert np.array_equal(a["h"][:3], a["hgrp"][0]) and a["h"][3] == a["hgrp"][1, 0] and np.array_equal(a["h"][7:], a["hgrp"][3, :2])
    # G = 1, alpha = 1, root = gamma with the root kept: stb_tindic_sample_h's replay to the bit
    import tl_oracle as tlo
    g1 = hho.replay(K, t, np.array([0, 4]), gamma, 1.0, gamma, 11, 2, flags=hho.KEEP_ROOT)
    hk, _ = tlo.sample_h(list(K), list(t), gamma, 11, 2)
    assert np.array_equal(g1["hgrp"][0], hk)
    # the unit's open interval, as the y stream needs it
    assert 0.0 < hqo.unit(np.array([1], dtype=np.uint64), np.array([1], dtype=np.uint64))[0] < 1.0
