"""The chain's oracle without a GPU (tests/ch_oracle.py): the enumerated target against the project's own collapsed joint,
the law of the pure CPU chain and the power of the test against three wrong laws, the thinning, the margins of every
seed tests/test_gpu_chain.py replays on the device -- the programs tree, missing and gauss among them -- the one-level tree
as the grouped step, and the power of the step comparison against three stale handovers."""
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
    steps = [m for m, _ in ch.PROGRAMS[program]]
    assert any(not np.array_equal(first.cust, s.cust) for s in states) and any(not np.array_equal(first.t, s.t) for s in states)
    assert last.a == ch.A_CHANGE[3] and not np.array_equal(last.bpar, first.bpar)
    assert (last.beta != first.beta) == ("sample_beta" in steps) and (last.gamma != first.gamma) == ("sample_gamma" in steps)
    if program == "grouped":
        assert last.alpha not in (None, ch.ALPHA0) and not np.array_equal(last.root, first.root)
    if program == "tree":
        assert len(last.alphas) == len(first.htoff) and ch.ALPHA0 not in last.alphas and not np.array_equal(last.root, first.root)
        assert all(not np.array_equal(x, y) for x, y in zip(last.hrows, first.hrows))
        if name == "mixed":     # an empty node and a node of one restaurant at level 1, an empty node at level 2
            sizes = [np.diff(o.astype(np.int64)) for o in first.htoff]
            assert len(sizes) == 2 and 0 in sizes[0] and 1 in sizes[0] and 0 in sizes[1] and int(first.K.max()) == 130
    if program == "missing":
        assert first.lik.shape == (5, 136) and (first.lik == 0.0).any()
        assert len({s.cls.tobytes() for s in states}) > 1 and int(last.cls.max()) >= 3
    if program == "gauss":
        K, D = int(first.K.max()), first.x.shape[1]
        assert (first.n.reshape(-1, K).sum(axis=0) == 0).any() and 8 <= first.Ni().min() and first.Ni().max() <= 40
        assert (K > 64) == (name == "g65") and (D > 16) == (name == "g65") and (first.gprior["alpha0"] < 1.0) == (name == "g8")
        assert not np.array_equal(last.mu, states[0].mu) and last.lik.shape == (len(first.cust), K)


def test_new_seeds_are_the_first_with_their_margin():
    """every case added after the first four: no earlier seed of 4500, 4600, .. keeps its chain's margins above 1e-7"""
    for (name, program), seed in list(ch.CASE_SEEDS.items())[4:]:
        assert seed in (4500, 4600, 4700, 4800, 4900)
        for earlier in range(4500, seed, 100):
            assert ch.run(program, ch.case(name, program), ch.ITERATIONS, earlier, a_at=ch.A_CHANGE)[1] <= 1e-7, (name, earlier)


def test_a_one_level_tree_is_the_grouped_step():
    """(tiny, tree) and (tiny, grouped) on one seed: h, the root, the concentration and the integers after every iteration,
    bit for bit"""
    seed = ch.CASE_SEEDS["tiny", "tree"]
    tree, _ = ch.run("tree", ch.case("tiny", "tree"), ch.ITERATIONS, seed, a_at=ch.A_CHANGE)
    grouped, _ = ch.run("grouped", ch.case("tiny", "grouped"), ch.ITERATIONS, seed, a_at=ch.A_CHANGE)
    for it, (x, y) in enumerate(zip(tree, grouped)):
        for f in ch.INTEGERS + ("h", "root", "lik", "bpar"):
            assert ch.same(getattr(x, f), getattr(y, f)), (it, f)
        assert x.alphas == (y.alpha,) and x.beta == y.beta and x.hrows == (), it
    assert len({x.alpha for x in tree}) == ch.ITERATIONS


# ---- the step comparison can fail: a chain with a stale handover, held against the right oracle as a device is ----

WRONG = {"stale_t": ("mixed", "tree", "sample_htree", 0), "stale_cls": ("generated", "missing", "sample_lik", 0),
         "stale_cust": ("g8", "gauss", "sample_gauss", 1)}     # (case, program, the step that shows it, at iteration)


def wrong_chain(name, program, wrong):
    """the chain of (name, program) with the handover `wrong` (None: none) run in a device's place: every step's outcome
    through ch_oracle.check_step against the oracle's on the state the wrong chain was in"""
    seed = ch.CASE_SEEDS[name, program]
    st = ch.case(name, program)
    for m, off in ch.PROLOGUES.get(program, ()):
        st, _ = ch.step(st, m, seed + off, 0)
    old_cust = st.cust
    for it in range(ch.ITERATIONS):
        if it in ch.A_CHANGE:
            st = st.replace(a=ch.A_CHANGE[it])
        old_t = st.t                                       # of before the iteration's dish sweep
        for m, off in ch.PROGRAMS[program]:
            where = "%s %s iteration %d %s" % (name, program, it, m)
            want, info = ch.step(st, m, seed + off, it)
            after, got = want, info
            if wrong == "stale_t" and m == "sample_htree":
                after, got = ch.step(st.replace(t=old_t), m, seed + off, it)
                after = after.replace(t=st.t)
            if wrong == "stale_cls" and m == "sample_classes":
                old_cls = st.cls
            if wrong == "stale_cls" and m == "sample_lik":
                after, got = ch.step(st, m, seed + off, it, cnt=ch.class_counts(st.replace(cls=old_cls)))
            if wrong == "stale_cust" and m == "sample_gauss":
                after, got = ch.step(st, m, seed + off, it, cust=old_cust)
                old_cust = st.cust                        # (what the next iteration's sweep starts from: one sweep earlier)
            got = dict(got)
            if m == "sample_htree":
                got["alphas"] = tuple(after.alphas)
            ch.check_step(m, where, st, after, want, got, info)
            st = after


def test_the_right_chain_passes_the_step_comparison():
    for name, program, _, _ in WRONG.values():
        wrong_chain(name, program, None)


@pytest.mark.parametrize("wrong", list(WRONG))
def test_a_stale_handover_is_caught_at_the_first_iteration_that_can_show_it(wrong):
    name, program, method, it = WRONG[wrong]
    with pytest.raises(AssertionError) as e:
        wrong_chain(name, program, wrong)
    print(wrong, "caught:", str(e.value)[:200])
    assert "%s %s iteration %d %s" % (name, program, it, method) in str(e.value)
