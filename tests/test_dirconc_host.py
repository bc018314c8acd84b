"""CPU checks of the Dirichlet concentration step's replay (tests/dc_oracle.py): the Antoniak identity and pmf behind
the auxiliary tables, the law of the replayed chain against the posterior by quadrature, the power of that check against
three wrong laws, and the margins of every case tests/test_gpu_dirconc.py replays on the device.

The chain's length (6000 steps: the device test's cap), burn-in, thinning and seeds are chosen here so that the right law
alone passes; DESIGN.md section 6 records the p-values."""
import math

import numpy as np
import pytest

import dc_oracle as dco
import hh_oracle as hho


@pytest.mark.parametrize("w", [1e-3, 0.5, 1.0, 37.5])
def test_antoniak_identity(w):
    """sum_m |s(c, m)| w^m = Gamma(w + c) / Gamma(w) for c <= 8: the pmf the auxiliary tables follow sums to one"""
    for c in range(9):
        s = [1]
        for n in range(c):
            s = [(n * s[m] if m < len(s) else 0) + (s[m - 1] if m >= 1 else 0) for m in range(len(s) + 1)]
        lhs = sum(s[m] * w ** m for m in range(c + 1))
        rhs = math.exp(math.lgamma(w + c) - math.lgamma(w))
        assert abs(lhs - rhs) <= 1e-12 * rhs, (c, lhs, rhs)
        assert abs(hho.antoniak_pmf(c, w).sum() - 1.0) <= 1e-12


@pytest.mark.parametrize("c,w", [(1, 0.3), (2, 0.7), (5, 1.5), (8, 0.05), (8, 6.0)])
def test_replayed_tables_follow_the_pmf(c, w):
    """20000 cells of count c under weight w (a multinomial each, one category, v = 1, s = w): chi-square against the pmf"""
    n = 20000
    out = dco.replay(np.full((n, 1), c, dtype=np.uint32), 1.0, w, 1.0, 1.0, 4400 + c, 0, dco.ROWS)
    got = np.bincount(out["m"][:, 0], minlength=c + 1).astype(np.float64)
    pmf = hho.antoniak_pmf(c, w)
    assert got[0] == 0 and pmf[0] == 0.0
    keep = pmf * n >= 5.0
    chi2 = float((((got - pmf * n) ** 2)[keep] / (pmf * n)[keep]).sum())
    dof = int(keep.sum()) - 1
    assert got[~keep].sum() <= 40, got
    assert chi2 <= dof + 4.0 * math.sqrt(2.0 * max(dof, 1)) + 10.0, (chi2, dof)     # (beyond p ~ 1e-3 for every dof here)


@pytest.fixture(scope="module")
def right_chains():
    return {fix: dco.chain(fix, dco.LAW_SEED[fix]) for fix in dco.LAW_FIX}


@pytest.mark.parametrize("fix", list(dco.LAW_FIX))
def test_law(fix, right_chains):
    p = dco.law_pvalue(fix, right_chains[fix])
    print(fix, "p =", p)
    assert p > 1e-3, p


@pytest.mark.parametrize("law", ["no_first", "no_q", "no_V"])
def test_wrong_laws_are_rejected(law):
    with np.errstate(all="ignore"):
        kept = dco.chain("3x2", dco.LAW_SEED["3x2"], law=law, steps=dco.WRONG_STEPS)
        p = dco.law_pvalue("3x2", kept)
    print(law, "p =", p)
    assert p < 1e-9, p


@pytest.mark.parametrize("name", list(dco.CASES))
def test_case_margins(name):
    """no decision of a replayed case hangs on the last bits of a transcendental"""
    r = dco.replay_case(name)
    assert r["margin_gamma"] > 1e-9 and r["margin_y"] > 1e-9, (r["margin_gamma"], r["margin_y"])
    c = dco.case(name)
    body = c["cnt"][:, :c["cols"]]
    assert r["count"] == int(body.sum())
    assert ((r["m"][:, :c["cols"]] >= (body > 0)) & (r["m"][:, :c["cols"]] <= body)).all()
    assert (r["m"][:, c["cols"]:] == 0).all()


def test_law_chain_margins(right_chains):
    """the device's law test replays the 3x2 chain: every step of it keeps its margins"""
    f = dco.LAW_FIX["3x2"]
    s, worst = 1.0, math.inf
    for t in range(dco.LAW_BURN + dco.LAW_STEPS):
        r = dco.replay(f["cnt"], f["v"], s, f["shape"], f["scale"], dco.LAW_SEED["3x2"], t, dco.ROWS)
        s = r["s"]
        worst = min(worst, r["margin_gamma"], r["margin_y"])
    assert worst > 1e-9, worst
