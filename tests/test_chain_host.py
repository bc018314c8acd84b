"""The chain's oracle without a GPU (tests/ch_oracle.py): the enumerated target against the project's own collapsed joint,
the law of the pure CPU chain and the power of the test against three wrong laws, the thinning, and the margins of every
seed tests/test_gpu_chain.py replays on the device."""
import itertools
import math
from functools import lru_cache

import numpy as np
import pytest

import ch_oracle as ch

U = 2.0 ** -53
PROBES = list(range(3, 324, 16))[:20]       # 20 of the 324 enumerated states


def test_the_enumeration_is_complete():
    st = ch.enumerate_states()
    assert len(st) == 18 * 18 and len(set(st)) == len(st) and len(PROBES) == 20
    p = ch.exact_p()
    assert abs(p.sum() - 1.0) < 1e-14 and p.min() > 0.0
    # beta and gamma are symmetric: exchanging the two dishes' names leaves p as it is
    idx = {s: j for j, s in enumerate(st)}
    swap = lambda s: tuple((tuple(1 - z for z in zi), ti[::-1]) for zi, ti in s)
    assert max(abs(p[j] - p[idx[swap(s)]]) for j, s in enumerate(st)) < 1e-15


def test_the_enumerated_weights_agree_with_the_collapsed_joint():
    """log p differences against the truth of the library's collapsed joint (flat model, data term, (n, t) form), within
    the two states' bars from lj_oracle and dm_oracle, and 4 u sum |term| for the doubles log_p itself adds up"""
    st = ch.enumerate_states()
    rows = []
    for j in PROBES:
        tr = ch.collapsed_truth(ch.state_of(st[j]), indicators=False, flat=True)["total"]
        terms = ch.log_p_terms(st[j])
        rows.append((math.fsum(terms), tr[0], tr[1] + 4.0 * U * sum(abs(x) for x in terms)))
    worst = 0.0
    for (lp1, t1, b1), (lp2, t2, b2) in itertools.combinations(rows, 2):
        worst = max(worst, abs((lp1 - lp2) - (t1 - t2)) / (b1 + b2))
        assert abs((lp1 - lp2) - (t1 - t2)) <= b1 + b2
    print("largest error over bar", worst, "over", len(rows) * (len(rows) - 1) // 2, "pairs")
    assert len({round(r[0], 9) for r in rows}) > 10         # the probes are not one state's weight over and over


@lru_cache(maxsize=None)
def chain(law):
    kept, worst = ch.law_chain(law)
    index, probs = ch.exact_cells()
    return kept, worst, ch.cell_counts([c for _, c in kept], index, len(probs)), index, probs


def test_the_pure_chain_keeps_the_exact_law():
    assert 4 * ch.LAW_ITERATIONS <= 6000
    kept, worst, counts, index, probs = chain("right")
    assert len(kept) == ch.LAW_ITERATIONS // ch.LAW_THIN and len(probs) >= 12
    assert (probs * len(kept)).min() >= 10.0 and abs(probs.sum() - 1.0) < 1e-12
    pv = ch.chi2_pvalue(counts, probs)
    print("bins", len(probs), "p-value of the right law", pv, "smallest margin", worst)
    assert pv > 1e-3 and worst > 1e-7


@pytest.mark.parametrize("law", [l for l in ch.LAWS if l != "right"])
def test_a_wrong_law_is_seen(law):
    kept, worst, counts, index, probs = chain(law)
    pv = ch.chi2_pvalue(counts, probs)
    print("p-value of", law, pv)
    assert pv < 1e-6


def test_the_thinning():
    kept, _, _, index, probs = chain("right")
    big = min(index, key=index.get)                        # the bins are sorted: bin 0 is the largest cell
    assert index[big] == 0
    r = ch.lag1([1.0 if c == big else 0.0 for _, c in kept])
    print("lag-1 autocorrelation of cell", big, "at thinning", ch.LAW_THIN, ":", r)
    assert abs(r) < 0.05


def test_the_committed_wrong_law_describes_the_wrong_chain():
    """ch_oracle.STALE_CELLS, which the device's counts are held against: the bins of exact_cells(), a law, far from the
    exact one, and the law of the stale_lik replay of this file"""
    _, _, counts, index, probs = chain("stale_lik")
    q = np.array(ch.STALE_CELLS)
    assert q.shape == probs.shape and abs(q.sum() - 1.0) < 1e-4 and q.min() > 0.0
    pv = ch.chi2_pvalue(counts, q)
    print("the stale_lik replay against its committed law", pv)
    assert pv > 1e-3


@pytest.mark.parametrize("name,program", list(ch.CASE_SEEDS))
def test_margins_of_the_handover_cases(name, program):
    states, worst = ch.run(program, ch.case(name, program), ch.ITERATIONS, ch.CASE_SEEDS[name, program], a_at=ch.A_CHANGE)
    print(name, program, "smallest margin", worst)
    assert worst > 1e-7
    first, last = ch.case(name, program), states[-1]
    assert any(not np.array_equal(first.cust, s.cust) for s in states) and any(not np.array_equal(first.t, s.t) for s in states)
    assert last.a == ch.A_CHANGE[3] and last.beta != first.beta and not np.array_equal(last.bpar, first.bpar)
    if program == "grouped":
        assert last.alpha not in (None, ch.ALPHA0) and not np.array_equal(last.root, first.root)
    else:
        assert last.gamma != first.gamma
