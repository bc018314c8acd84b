"""The likelihood and base-weight draws without a GPU: the entry points exist, the numpy replay (tests/tl_oracle.py)
normalises as the header says, and no replay case of tests/test_gpu_tlik.py sits on an acceptance tie."""
import math
import os
import re

import numpy as np
import pytest

import tl_oracle as tlo
from libstb_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stb_sample_lik", "stb_lik_loglik", "stb_tindic_sample_lik", "stb_tindic_sample_h", "stb_tindic_loglik")
# the replay tests leave no cell out, so no acceptance decision may hang on a transcendental's last bits
MARGIN = 1e-9


def test_entry_points_exist():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "stb_hip.h")).read()
    source = open(os.path.join(ROOT, "libstb_amd", "capi.py")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert 'sig("%s"' % name in source, name
    for name in ("sample_lik", "sample_h", "loglik"):
        assert hasattr(capi.TableIndicators, name), name
    assert hasattr(capi, "sample_lik") and hasattr(capi, "lik_loglik")
    # refused before any device is touched
    assert L.stb_sample_lik(None, 3, 3, None, 0.5, None, 1, 0, None) != 0 and "required" in capi.last_error()
    assert L.stb_tindic_sample_lik(None, None, 0.5, 1, 0) != 0 and "null object" in capi.last_error()
    assert L.stb_tindic_sample_h(None, None, 1.0, 1, 0) != 0 and "null object" in capi.last_error()
    assert L.stb_tindic_loglik(None, None, None) != 0 and "null object" in capi.last_error()


@pytest.mark.parametrize("name", list(tlo.LIK_CASES))
def test_replay_cases_sit_on_no_tie_and_sum_to_one(name):
    cnt, beta, seed, sweep = tlo.lik_case(name)
    lik, margin = tlo.sample_lik(cnt, beta, seed, sweep)
    print(name, "smallest acceptance margin", margin)
    assert margin >= MARGIN, (name, margin)
    rows = cnt.shape[0]
    assert np.all(np.isfinite(lik)) and lik.min() >= 0.0 and lik.max() <= 1.0
    for k in range(cnt.shape[1]):
        assert abs(math.fsum(lik[:, k]) - 1.0) <= 2.0 * 2.0 ** -53 * rows, (name, k)
    if rows == 1:
        assert np.all(lik == 1.0)
    else:
        assert len(np.unique(lik)) > lik.size // 2


def test_the_mixed_counts_take_both_branches():
    cnt, beta, _, _ = tlo.lik_case("600x70_b0.05")
    assert (cnt == 0).mean() > 0.2 and (cnt == 1).mean() > 0.2 and cnt.max() == 10000
    _, beta, _, _ = tlo.lik_case("600x70_vec")
    assert (beta < 1.0).any() and (beta > 1.0).any() and (beta == 1.0).any()


def test_one_row_is_exactly_one():
    for stride, beta in ((1, 0.01), (7, 3.0), (130, 0.5)):
        lik, _ = tlo.sample_lik(np.arange(stride, dtype=np.uint32).reshape(1, stride), beta, 5, 9)
        assert np.all(lik == 1.0)


def test_base_weight_case_sits_on_no_tie():
    c = tlo.H_CASE
    assert list(tlo.table_counts(c["K"], c["t"])) == [3 + 2 + 2, 1 + 1, 0 + 3, 7, 1]
    hk, margin = tlo.sample_h(c["K"], c["t"], c["gamma"], c["seed"], c["sweep"])
    print("smallest acceptance margin", margin)
    assert margin >= MARGIN
    assert abs(math.fsum(hk) - 1.0) <= 2.0 * 2.0 ** -53 * len(hk) and hk.min() > 0.0
    g2, seed2, sweep2 = tlo.H_CASE_SCALAR
    hk2, margin2 = tlo.sample_h(c["K"], c["t"], g2, seed2, sweep2)
    print("smallest acceptance margin, scalar gamma", margin2)
    assert margin2 >= MARGIN and abs(math.fsum(hk2) - 1.0) <= 2.0 * 2.0 ** -53 * len(hk2)
    h = tlo.spread_h(c["K"], hk)
    assert len(h) == sum(c["K"]) and h[5] == hk[0] and h[8] == hk[0] and h[7] == hk[2]


def test_the_draws_depend_on_seed_sweep_and_cell_alone():
    cnt = tlo.mixed_counts(5, 9, 3)
    a, _ = tlo.sample_lik(cnt, 0.7, 11, 2)
    b, _ = tlo.sample_lik(cnt, 0.7, 11, 3)
    c, _ = tlo.sample_lik(cnt, 0.7, 12, 2)
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    # the log-Gamma variate of cell e is the same whatever the matrix around it
    lg, _ = tlo.log_gamma(np.full(45, 2.5), tlo.cell_keys(11, 2, 45))
    lg2, _ = tlo.log_gamma(np.full(20, 2.5), tlo.cell_keys(11, 2, 20))
    assert np.array_equal(lg[:20], lg2)


def test_loglik_association_and_impossible_cells():
    rng = np.random.default_rng(4)
    cnt = tlo.mixed_counts(300, 5, 8)
    lik = rng.random((300, 5)) + 0.01
    tot, imp = tlo.loglik(cnt, lik)
    want = math.fsum((cnt.astype(np.float64) * np.log(lik)).reshape(-1))
    assert imp == 0 and abs(tot - want) <= 1e-12 * abs(want)
    w, k = np.argwhere(cnt > 0)[0]
    lik[w, k] = 0.0
    tot, imp = tlo.loglik(cnt, lik)
    assert tot == -math.inf and imp == 1
    lik[w, k] = 0.5
    w, k = np.argwhere(cnt == 0)[0]
    before = tlo.loglik(cnt, lik)
    lik[w, k] = 0.0
    assert tlo.loglik(cnt, lik) == before and not math.isnan(before[0])
