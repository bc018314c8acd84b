"""The conditions test_gpu_hp_shapes.py rests on, checked without a device: the pair generator's density ceilings and what it
never drops, the sensitivity of the sums to one pair answered from a neighbouring cell, and the mpmath aterms2 truth
against the exact product."""
from fractions import Fraction

import numpy as np
import pytest

import hp_oracle as hp
import hp_pairs as P

SHAPES = [(1201, 209), (1202, 210), (1250, 81), (1250, 82), (1250, 145), (1250, 146), (1300, 465), (1300, 466), (1500, 1500),
          (4001, 301), (4001, 1001), (30000, 60), (70000, 130), (140000, 90), (10000, 10000)]
NO_SPARSE_SET, LOC = P.NO_SPARSE_SET, P.LOC
LOCALISED = [s for s in SHAPES if s not in ((1500, 1500), (10000, 10000))]


def test_mirrored_block_rows():
    """block rows (hb2 / hb3 / hb4, grid) per N from the mirrored formulas: the period is 63 rows up to 16384, 46 up to 131072"""
    for N, want in ((1500, (48, 48, 48, 48)), (4001, (48, 48, 48, 48)), (10000, (48, 48, 48, 48)), (16384, (48, 48, 48, 48)),
                    (30000, (40, 24, 40, 40)), (70000, (40, 24, 40, 40)), (41000, (40, 24, 40, 40)), (131072, (40, 24, 40, 40)),
                    (140000, (32, 24, 32, 32))):
        got = (P.hb_geometry(N, 2)[0], P.hb_geometry(N, 3)[0], P.hb_geometry(N, 4)[0], P.grid_geometry(N, 4)[0])
        assert got == want, (N, got)
    assert [P.hb_geometry(1500, c)[1] for c in (2, 3, 4)] + [P.grid_geometry(1500, 8)[1]] == [80, 144, 208, 464]
    assert [P.hb_geometry(30000, c)[1] for c in (2, 3, 4)] + [P.grid_geometry(30000, 8)[1]] == [88, 168, 216, 472]
    assert [P.hb_geometry(140000, c)[1] for c in (2, 3, 4)] + [P.grid_geometry(140000, 8)[1]] == [96, 168, 224, 480]


@pytest.mark.parametrize("N,M", SHAPES, ids=lambda v: str(v))
def test_density_and_coverage(N, M):
    """the targeted set lies between 0.04 and 1/3 of the cells, the sparse set at or below 0.04; after thinning every class
    that is never dropped is there for every geometry (targeted_pairs asserts check_coverage itself; again here)"""
    cells = P.table_cells(N, M)
    K, n, t, T, bpar, cls = P.targeted_pairs(N, M, rho=1.0 / 3.0)
    assert 0.04 * cells < len(n) and 3 * len(n) <= cells, (len(n), cells)
    P.check_coverage(N, M, n, t, cls)
    assert int(K.sum()) == len(n) and np.array_equal(np.add.reduceat(t.astype(np.uint64), np.r_[0, np.cumsum(K)[:-1]]), T)
    if (N, M) in NO_SPARSE_SET:
        with pytest.raises(P.BudgetTooSmall):
            P.targeted_pairs(N, M, rho=0.04)
        return
    K, n, t, T, bpar, cls = P.targeted_pairs(N, M, rho=0.04)
    assert len(n) <= 0.04 * cells
    P.check_coverage(N, M, n, t, cls)
    assert int(np.count_nonzero(cls == P.HEAVY)) == P.HEAVY_COUNT


def test_thin_set_for_records_in_global_memory():
    N = M = 46000
    UC = P.hb_geometry(N, 2)[1]
    assert (min(N - 1, M) - 1 + UC - 1) // UC + 2 > 512 >= (40999 - 1 + UC - 1) // UC + 2   # (41000 columns: records still in LDS)
    cells = P.table_cells(N, M)
    K, n, t, T, bpar, cls = P.targeted_pairs(N, M, stride=64, rho=2e6 / cells)
    assert len(n) <= 2_000_000
    P.check_coverage(N, M, n, t, cls)


@pytest.mark.parametrize("N,M", LOCALISED, ids=lambda v: str(v))
def test_sensitivity(N, M):
    """one pair answered from the cell left of it or above it moves its sum by more than the sum's bar: for every sum of
    the class-by-class hand-over (every class, every piece of the classes of whole rows, both pair sets, the four discounts
    of the hand-over) but those named in hp_pairs.CANNOT_HOLD, which are asserted NOT to meet it -- the list is exact; and
    for the whole-set sums below CHUNK_FROM rows (beyond, 10^5 .. 10^6 pairs share one bar: there the class sums count)"""
    names = ["targeted"] + ([] if (N, M) in NO_SPARSE_SET else ["sparse"])
    sets = [P.targeted_pairs(N, M, rho=1.0 / 3.0)] + ([] if (N, M) in NO_SPARSE_SET else [P.targeted_pairs(N, M, rho=0.04)])
    bad = []
    for name, tr in zip(names, P.aterms_truth_by_class(sets, P.XS[:6], N, M)):
        named = P.CANNOT_HOLD.get((N, M, name), {})
        for c, cname in enumerate(P.CLASSES):
            for k in tr.chunks(c):
                m = tr.margin([c], k)[LOC]
                for a, v in zip(P.XS[LOC], m):
                    if (v > 1.0) == (k in named.get((cname, float(a)), [])):
                        bad.append((name, cname, float(a), k, float(v)))
        if N < P.CHUNK_FROM:
            assert np.all(tr.margin()[LOC] > 1.0), (N, M, name, tr.margin()[LOC])
        else:
            assert len(tr.chunks(P.BLOCK)) > 32 and len(tr.chunks(P.GROUP)) >= 1
    assert not bad, bad


def test_aterms2_truth_against_the_exact_product():
    """hp.aterms2's table part is log prod_{i=1}^{s-1} (i - x): for dyadic x and small s the product is an exact rational"""
    T, bpar = np.array([], dtype=np.uint32), np.array([])
    for x in (0.5, 0.25, 3 * 2.0 ** -30, 1 - 2.0 ** -20):
        cnt = np.zeros(40, dtype=np.uint32)
        cnt[[2, 3, 4, 5, 17, 39]] = [1, 2, 3, 5, 7, 11]
        val, bar = hp.aterms2(x, cnt, T, bpar)
        mp = hp._mp()
        want = mp.mpf(0)
        for s in np.nonzero(cnt)[0]:
            prod = Fraction(1)
            for i in range(1, int(s)):
                prod *= Fraction(i) - Fraction(x)
            want += int(cnt[s]) * (mp.log(mp.mpf(prod.numerator)) - mp.log(mp.mpf(prod.denominator)))
        wl = hp.LD(float(want)) + hp.LD(float(want - float(want)))
        assert abs(float(wl - val)) <= 2.0 ** -60 * max(1.0, abs(float(want))), (x, float(want), float(val))
        assert 0 < bar < 1e-10
    assert hp.aterms2(0.37, np.zeros(70000, dtype=np.uint32), T, bpar)[0] == 0
