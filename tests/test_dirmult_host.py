"""The log marginal of multinomials under a Dirichlet prior (libstb_amd/csrc/dirmult.hip) without a GPU: the law's
identities in mpmath, the numpy replay of the kernel's operations (tests/dm_oracle.py) against the 40-digit truth on every
case of the GPU tests, and wrong replays told apart -- by the bar, or by bits where only an association changes."""
import math

import numpy as np
import pytest

import dm_oracle as dmo
import hp_oracle as hp


def logml_mp(c, w):
    mp = hp._mp()
    W, C = mp.fsum(w), sum(c)
    return (mp.loggamma(W) - mp.loggamma(W + C)) + mp.fsum(mp.loggamma(wj + cj) - mp.loggamma(wj) for wj, cj in zip(w, c))


def log_dir(h, w):
    mp = hp._mp()
    return mp.loggamma(mp.fsum(w)) - mp.fsum(mp.loggamma(x) for x in w) + mp.fsum((x - 1) * mp.log(p) for x, p in zip(w, h))


C5 = (0, 1, 8, 9, 300)


def w5():
    mp = hp._mp()
    return [mp.mpf(x) for x in ("0.003", "1.75", "0.5", "12.25", "0.0625")]


def test_the_formula_is_the_polya_urn():
    mp = hp._mp()
    w = w5()
    W = mp.fsum(w)
    seen, n, lp = [0] * 5, 0, mp.mpf(0)
    order = [j for j, c in enumerate(C5) for _ in range(c)]
    np.random.default_rng(5).shuffle(order)          # (exchangeable: any order gives the same product)
    for j in order:
        lp += mp.log((w[j] + seen[j]) / (W + n))
        seen[j] += 1
        n += 1
    assert abs(lp - logml_mp(C5, w)) < mp.mpf("1e-30")


def test_the_formula_is_the_likelihood_times_prior_over_posterior():
    mp = hp._mp()
    w = w5()
    raw = [mp.mpf(x) for x in ("0.2", "1.3", "0.05", "2.5", "0.7")]
    h = [x / mp.fsum(raw) for x in raw]
    post = [x + c for x, c in zip(w, C5)]
    val = mp.fsum(c * mp.log(p) for c, p in zip(C5, h)) + log_dir(h, w) - log_dir(h, post)
    assert abs(val - logml_mp(C5, w)) < mp.mpf("1e-30")


def test_the_base_term_of_the_log_joint_regroups_to_the_group_counts():
    """sum_i H_i = sum_i sum_k t_ik log h_{g(i) k} equals sum_g sum_k c_gk log h_gk"""
    mp = hp._mp()
    rng = np.random.default_rng(11)
    I, K, goff = 7, 5, [0, 2, 2, 6, 7]
    t = rng.integers(0, 9, size=(I, K))
    hg = [[mp.mpf(int(v)) / 97 for v in row] for row in rng.integers(1, 40, size=(len(goff) - 1, K))]
    owner = [max(g for g in range(len(goff) - 1) if goff[g] <= i) for i in range(I)]
    lhs = mp.fsum(int(t[i, k]) * mp.log(hg[owner[i]][k]) for i in range(I) for k in range(K))
    c = np.zeros((len(goff) - 1, K), dtype=np.int64)
    for i in range(I):
        c[owner[i]] += t[i]
    rhs = mp.fsum(int(c[g, k]) * mp.log(hg[g][k]) for g in range(len(goff) - 1) for k in range(K))
    assert abs(lhs - rhs) < mp.mpf("1e-30")


@pytest.mark.parametrize("name", dmo.CASES)
def test_the_replay_lies_within_the_bar_of_the_truth(name):
    got, want = dmo.case_replay(name), dmo.case_truth(name)
    for k in ("nonzero", "count", "zero_weight", "impossible"):
        assert got[k] == want[k], k
    ratio = dmo.worst_ratio(got, want)
    print(name, "worst |replay - truth| / bar", ratio, "total", got["total"], "bar", want["total"][1])
    assert not np.isnan(got["each"]).any() and ratio <= 1.0


@pytest.mark.parametrize("variant", ["arg_minus_one", "no_norm", "short_rise"])
def test_a_wrong_replay_is_outside_the_bar(variant):
    worst = {name: dmo.worst_ratio(dmo.case_replay(name, variant), dmo.case_truth(name)) for name in ("rows_257_7", "cellcols")}
    print(variant, worst)
    assert all(r > 1.0 for r in worst.values())


def test_another_association_changes_bits():
    name = "rows_%d_3" % dmo.ROWS_PAST_A_TRIP
    good, other = dmo.case_replay(name), dmo.case_replay(name, "block_order")
    assert np.array_equal(good["each"], other["each"])
    assert (good["cells"], good["norms"], good["total"]) != (other["cells"], other["norms"], other["total"])


def test_edge_rules_of_the_replay():
    w = np.array([0.0, 1.5, 2.0])
    ok = dmo.replay(np.array([[0, 3, 9], [0, 0, 0]]), w, dmo.ROWS)
    assert ok["zero_weight"] == 2 and ok["impossible"] == 0 and math.isfinite(ok["total"]) and ok["each"][1] == 0.0
    bad = dmo.replay(np.array([[1, 3, 9], [0, 1, 0]]), w, dmo.ROWS)
    assert bad["impossible"] == 1 and bad["total"] == -math.inf and bad["each"][0] == -math.inf and math.isfinite(bad["each"][1])
    for orient in (dmo.ROWS, dmo.COLUMNS):
        zero = dmo.replay(np.zeros((3, 3), dtype=np.uint32), np.array([0.5, 1.0, 2.0]), orient)
        assert zero["total"] == 0.0 and zero["cells"] == 0.0 and zero["norms"] == 0.0 and not zero["each"].any()
