"""The samplers' long-double laws (tests/hs_oracle.py) on the host: every case of tests/test_gpu_samplers_truth.py has no
undecided draw (so the GPU test may demand equality), the laws are the enumerated laws on small shapes, and every case
notices the mistake it exists for.

What draws cannot see: a relative weight error well below 1 / (number of draws) moves no draw.  The cases make about
6300 draws, so they say nothing about cell errors below about 1e-4 relative; that part rests on the table tests
(tests/test_gpu_hp.py, tests/test_gpu_hp_shapes.py)."""
from fractions import Fraction

import numpy as np
import pytest

import hp_oracle as hp
import hs_cases as hc
import hs_oracle as hs
import pt_oracle as pto
import tc_oracle as tco
import tcw_oracle as tcw

LD = np.longdouble


# ---- every case is decided by the truth alone ----

def check_decided(name, st):
    print(f"{name}: draws {st.draws}, undecided {st.undecided}, smallest |uW - C| / (eps W) {st.margin:.3g}, "
          f"largest eps {st.eps:.3g}")
    assert st.draws > 0
    assert st.undecided == 0, "choose another seed for this case (tests/hs_cases.py)"
    assert st.margin >= 1.0


@pytest.mark.parametrize("case", hc.tc_cases(), ids=lambda c: c.name)
def test_tcounts_cases_are_decided(case):
    out, st = hc.tc_truth(case)
    check_decided(case.name, st)
    assert not np.array_equal(out[-1][0], case.t)


@pytest.mark.parametrize("case", hc.tcw_cases(), ids=lambda c: c.name)
def test_tcwin_cases_are_decided(case):
    check_decided(case.name, hc.tcw_truth(case)[1])


@pytest.mark.parametrize("S", hc.PT_S)
@pytest.mark.parametrize("a", hc.A_SET)
def test_partition_cases_are_decided(a, S):
    cnt, sizes, st = hc.pt_truth(a, S)
    check_decided(f"pt_a{a:g}_S{S}", st)
    n, t = hc.pt_pairs()
    assert all(sz is None or sum(sz) == int(n[g]) for g, sz in enumerate(sizes))
    if S > 1024:
        assert cnt[2:1024].sum() > 0 and cnt[1024:].sum() > 0 and cnt[0] == 0  # sizes either side of the LDS histogram
    else:
        assert cnt[0] == np.count_nonzero((n >= S) & (t != n))


def test_thresholds_of_the_cases():
    """the shapes sit where the kernels change behaviour (tcounts.hip, tcwin.hip, partition.hip)"""
    tm = set(hc.TMAX)
    for nt in (64, 128, 256, 512, 1024):
        assert {nt - 1, nt, nt + 1} <= tm
    assert {4095, 4096, 4097} <= tm                                   # STB_TC_CAP
    assert 4 * 15 + 1 <= 64 < 4 * 16 + 1 and 15 in hc.TCW_W and 16 in hc.TCW_W  # one chunk / several
    assert {63, 64, 65, 127, 128, 129} <= set(hc.PT_L)


# ---- the law is the law ----

def double_table(a, N, M):
    S1, S, _ = hp.tables(a, N, M)[0]
    return S1.astype(np.float64), S.astype(np.float64)


@pytest.mark.parametrize("a,b,hs_", [(0.0, 2.0, (1.0, 1.0)), (0.5, 1.5, (0.7, 1.3)), (0.999, 0.25, (2.0, 0.5))])
def test_conditional_is_the_joints(a, b, hs_):
    """hs.log_weights of a pair against the enumerated joint tco.log_joint with the other pair held: equal up to a
    constant of the row, to 1e-15 of the log joint's size"""
    ns = (12, 7)
    S1, tab = double_table(a, 12, 12)
    worst = 0.0
    for k in (0, 1):
        for other in range(1, ns[1 - k] + 1):
            lw = hs.log_weights(ns[k], other, a, b, hs_[k], 12)
            lj = np.array([tco.log_joint(ns, (tau, other) if k == 0 else (other, tau), a, b, hs_, S1, tab, 12)
                           for tau in range(1, ns[k] + 1)], dtype=LD)
            d = (lj - lw) - (lj[0] - lw[0])
            scale = np.maximum(1.0, np.abs(lj).max())
            worst = max(worst, float(np.abs(d).max() / scale))
    print(f"a={a}: worst |d log w| / |log joint| = {worst:.3g}")
    assert worst <= 1e-15


def ld_pair_kernel(lw, W, ref):
    """the transition matrix of one visit from hs.window and long-double sums"""
    Mt = len(lw)
    w = np.exp(lw - lw.max())
    Z = [w[hs.window(x, W, Mt)[0] - 1:hs.window(x, W, Mt)[1]].sum() for x in range(1, Mt + 1)]
    P = np.zeros((Mt, Mt), dtype=LD)
    for x in range(1, Mt + 1):
        lo, hi = hs.window(x, W, Mt)
        for y in range(lo, hi + 1):
            if y != x:
                P[x - 1, y - 1] = w[y - 1] / Z[x - 1] * (LD(1) if ref else min(LD(1), Z[x - 1] / Z[y - 1]))
        P[x - 1, x - 1] = LD(1) - P[x - 1].sum()
    return P


@pytest.mark.parametrize("ref", [False, True])
@pytest.mark.parametrize("W", [1, 2, 5])
def test_window_step_is_the_pair_kernel(W, ref):
    """hs.window_step against tcw_oracle.pair_kernel.  Both matrices are built from the same log weights -- hs's, rounded
    to doubles -- so that the comparison is of the two laws, not of their inputs (hs.log_weights against tc_oracle's is
    test_conditional_is_the_joints, and once more below): moves agree to 1e-15 relative, staying to 1e-15 of the row's
    total 1.  And window_step lands where the matrix says at the middle of every cell of (u1, u2)."""
    a, b, h, n, Tm = 0.4, 1.5, 0.8, 12, 5
    lw = hs.log_weights(n, Tm, a, b, h, 12)
    S1, tab = double_table(a, 12, 12)
    lw_tc = tco.log_weights(n, Tm, a, b, h, 12, S1, tab, 12)
    assert float(np.max(np.abs(lw_tc - lw))) <= 1e-15 * float(np.abs(lw).max())
    lw64 = np.asarray(lw, dtype=np.float64)
    P = tcw.pair_kernel(lw64, W, ref)
    Q = ld_pair_kernel(lw64.astype(LD), W, ref)
    off = ~np.eye(n, dtype=bool) & (P > 0)
    assert np.array_equal(P > 0, np.asarray(Q > 0))
    rel = float(np.max(np.abs(P[off] - Q[off]) / Q[off]))
    dia = float(np.max(np.abs(np.diag(P) - np.diag(Q))))
    print(f"W={W} ref={ref}: moves {rel:.3g} relative, staying {dia:.3g}")
    assert rel <= 1e-15 and dia <= 1e-15
    w = np.exp(lw - lw.max())
    for t in range(1, n + 1):
        lo, hi = hs.window(t, W, n)
        C = np.concatenate([[LD(0)], np.cumsum(w[lo - 1:hi])])
        for y in range(lo, hi + 1):
            u1 = float((C[y - lo] + C[y - lo + 1]) / 2 / C[-1])
            lp, hp_ = hs.window(y, W, n)
            acc = 1.0 if ref or y == t else min(1.0, float(C[-1] / w[lp - 1:hp_].sum()))
            for u2, want in ((acc * 0.999, y), (acc * 1.001, t)):
                if u2 < 1.0:
                    got, ok = hs.window_step(lw, t, W, u1, u2, ref, 1e-9)
                    assert ok and got == (y if (ref or y == t) else want), (t, y, u2)


def exact_partition_law(n, t, a):
    """pt_oracle's enumeration (pto.partitions) with the definition's weights in exact rationals"""
    fa = Fraction(float(a))
    w = {}
    for p in pto.partitions(n, t):
        v = Fraction(1)
        for s in p:
            for j in range(s - 1):
                v *= 1 - fa + j
        num = Fraction(1)
        for j in range(2, n + 1):
            num *= j
        for s in p:
            for j in range(2, s + 1):
                num /= j
        for m in np.unique(p, return_counts=True)[1]:
            for j in range(2, int(m) + 1):
                num /= j
        w[p] = v * num
    Z = sum(w.values())
    return {p: v / Z for p, v in w.items()}


def hs_partition_law(n, t, a):
    """the law of hs's sequential rounds over multisets, in long double"""
    c = hs.cells((float(a),), n, t, None)[float(a)]
    law = {(): LD(1)}
    for r in range(t - 1):
        Mc = t - 1 - r
        nxt = {}
        for seq, p in law.items():
            Nr = n - sum(seq)
            pl = np.exp(hs.round_log_weights(Nr, Mc, a, c)[0]) if Nr - Mc > 1 else [LD(1)]
            for l, q in enumerate(pl, 1):
                nxt[seq + (l,)] = nxt.get(seq + (l,), LD(0)) + p * q
        law = nxt
    out = {}
    for seq, p in law.items():
        key = tuple(sorted(seq + (n - sum(seq),), reverse=True))
        out[key] = out.get(key, LD(0)) + p
    return out


@pytest.mark.parametrize("n,t,a", [(8, 3, 0.5), (12, 4, 0.2), (10, 5, 0.8), (12, 6, 0.0), (11, 3, 0.999)])
def test_partition_rounds_are_the_enumerated_law(n, t, a):
    got, want = hs_partition_law(n, t, a), exact_partition_law(n, t, a)
    assert set(got) == set(want)
    pt = pto.truth(n, t, a)
    rel = max(abs(float(got[p] / LD(want[p].numerator) * LD(want[p].denominator)) - 1.0) for p in want)
    rel_pt = max(abs(float(got[p]) / pt[p] - 1.0) for p in want)
    print(f"n={n} t={t} a={a}: {rel:.3g} of the exact law, {rel_pt:.3g} of pt_oracle.truth (doubles)")
    assert rel <= 1e-15
    assert rel_pt <= 1e-15


def test_partition_round_draws_its_law():
    a, Nr, Mc = 0.3, 12, 3
    lw = hs.round_log_weights(Nr, Mc, a, hs.cells((a,), Nr, Mc + 1, None)[a])[0]
    C = np.concatenate([[LD(0)], np.cumsum(np.exp(lw))])
    assert abs(float(C[-1]) - 1.0) <= 1e-15  # the recursion: the weights sum to 1
    for l in range(1, Nr - Mc + 1):
        assert hs.partition_round(Nr, Mc, a, float((C[l - 1] + C[l]) / 2), Mc + 1) == (l, True)
    assert hs.partition_round(5, 4, a, 0.3, 5) == (1, True)


def test_draw_and_its_bar():
    lw = np.log(np.array([1.0, 2.0, 1.0], dtype=LD))
    assert hs.draw(lw, 0.1, 1e-9) == (1, True) and hs.draw(lw, 0.5, 1e-9) == (2, True)
    assert hs.draw(lw, 0.8, 1e-9) == (3, True)
    assert hs.draw(lw, 0.25 + 1e-12, 1e-9) == (2, False) and hs.draw(lw, 0.25 - 1e-12, 1e-9) == (1, False)


# ---- the cases can see the mistakes they exist for ----

def tc_changed(case, name):
    want = hc.tc_truth(case)[0]
    with hs.mutant(name):
        got = hc._tc_truth.__wrapped__(case.name)[0]
    return any(not np.array_equal(g[0], w[0]) for g, w in zip(got, want))


def tcw_changed(case, name):
    want = hc.tcw_truth(case)[0]
    with hs.mutant(name):
        got = hc._tcw_truth.__wrapped__(case.name)[0]
    return any(not np.array_equal(g[0], w[0]) for g, w in zip(got, want))


@pytest.mark.parametrize("name,case", [
    ("tminus", hc.tc_boundary()), ("tminus", hc.tc_trunc(4097)), ("left", hc.tc_boundary()), ("left", hc.tc_big_T()),
    ("tmax", hc.tc_boundary()), ("tmax", hc.tc_trunc(64)), ("logcarry64", hc.tc_boundary()),
    ("logcarry256", hc.tc_boundary()), ("ccarry", hc.tc_boundary()), ("ccarry", hc.tc_trunc(4097)),
    # (a row of 4097 ends at 4097 visibly only where tau = 4097 carries weight: a = 0.999, where S^n_{n-1} is small)
    ("row4097", hc.tc_params(0.999, True)), ("row4097", hc.tc_params(0.999, False))],
    ids=lambda x: x if isinstance(x, str) else x.name)
def test_tcounts_mutants_are_noticed(name, case):
    assert tc_changed(case, name)


@pytest.mark.parametrize("case", [hc.tcw_trunc(16, False), hc.tcw_trunc(16, True), hc.tcw_trunc(15, False),
                                  hc.tcw_params(0.999, 1.0)], ids=lambda c: c.name)
def test_window_clip_mutant_is_noticed(case):
    assert tcw_changed(case, "winclip")


@pytest.mark.parametrize("name", ["pt_la", "pt_carry65"])
def test_partition_mutants_are_noticed(name):
    a = 0.5
    want = hc.pt_truth(a, hc.PT_S[0])[1]
    with hs.mutant(name):
        got = hc.pt_truth.__wrapped__(a, hc.PT_S[0])[1]
    changed = [g for g in range(len(want)) if got[g] != want[g]]
    assert changed
    if name == "pt_carry65":  # only rounds with L >= 65 can differ
        n, t = hc.pt_pairs()
        assert all(int(n[g]) - int(t[g]) + 1 >= 65 for g in changed)
