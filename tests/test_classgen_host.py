"""The class draw's contract on the CPU (include/stb_hip.h, "customers' classes drawn on the device"): tests/cg_oracle.py's
replay against tl_oracle's normaliser, against a scan, on the rule's edges, against wrong replays, and in law -- alone and
alternated with the dish sweep's replay, where the pair must leave p(z, t, cls | lik, h, a, b) invariant.

Only test_the_new_calls_are_exported touches the library (and fails without it).  Every other test here exercises the
numpy replay alone: it establishes that the replay is the contract -- its association, its rule, its law.  The kernels are
then held to that replay bit for bit in tests/test_gpu_classgen.py; nothing here says anything about them by itself."""
import math
from functools import lru_cache

import numpy as np
import pytest

import cg_oracle as cgo
import st_oracle as sto
import td_oracle as tdo
import ti_oracle as tio
import tl_oracle as tlo
from libstb_amd import capi


def test_the_new_calls_are_exported():
    L = capi.lib()
    for name in ("stb_sample_classes", "stb_tindic_sample_classes", "stb_tindic_generate", "stb_tindic_get_classes"):
        assert hasattr(L, name), name
    assert [f[0] for f in capi.ClassesInfo._fields_] == ["skipped", "stuck", "drawn"]


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 513, 1000])
def test_Z_is_the_normalisers_to_the_bit(rows):
    lik = cgo.matrix_with_zeros(rows, 7, 3)
    cum, Z = cgo.cum_columns(lik)
    want = tlo.chunk_sums(lik)
    assert Z.tobytes() == want.tobytes()
    assert cum[-1].tobytes() == Z.tobytes()
    if rows > 257:   # and the association is not the plain one (a second chunk of one row adds as the plain sum does)
        assert any(cgo.cum_columns(cgo.matrix_with_zeros(rows, 7, s), plain=True)[1].tobytes() !=
                   cgo.cum_columns(cgo.matrix_with_zeros(rows, 7, s))[1].tobytes() for s in range(8))


@pytest.mark.parametrize("rows", [1, 2, 255, 257, 513, 1000])
def test_cum_is_monotone_and_the_search_is_the_scan(rows):
    rng = np.random.default_rng(rows)
    lik = cgo.matrix_with_zeros(rows, 4, 11)
    cum, Z = cgo.cum_columns(lik)
    assert np.all(np.diff(cum, axis=0) >= 0.0)
    grew = np.vstack([cum[:1] > 0.0, np.diff(cum, axis=0) > 0.0])
    assert np.all(lik[grew] > 0.0)                    # the sum grows only at a cell of positive weight
    for k in range(4):
        if not Z[k] > 0.0:
            continue
        for u in list(rng.random(40)) + [0.0, 0.5, 1.0 - 2.0 ** -53]:
            w = cgo.choose(cum[:, k], Z[k], u)
            assert w == cgo.choose_linear(cum[:, k], Z[k], u) and lik[w, k] > 0.0, (k, u)
    u = rng.random(300)
    dishes = rng.integers(0, 4, size=300)
    ok = (Z > 0.0)[dishes]
    got = cgo.draw(cum, Z, dishes[ok], u[ok])
    assert [int(x) for x in got] == [cgo.choose_linear(cum[:, k], Z[k], x) for k, x in zip(dishes[ok], u[ok])]


def test_the_rule_at_explicit_uniforms():
    top = 1.0 - 2.0 ** -53
    # a first row of zero, a last row of zero
    col = np.array([0.0, 0.25, 0.0, 0.5, 0.0])
    cum, Z = cgo.cum_columns(col[:, None])
    c, Z = cum[:, 0], float(Z[0])
    assert Z == 0.75
    assert cgo.choose(c, Z, 0.0) == 1                 # u = 0: the first row of positive weight, not row 0
    assert cgo.choose(c, Z, 0.25 / 0.75) == 3         # thr = cum_1 exactly: > moves on
    assert cgo.choose(c, Z, np.nextafter(1.0 / 3.0, 0.0)) == 1
    assert cgo.choose(c, Z, top) == 3                 # never the trailing zero
    # one positive cell: every u gives it
    one = np.zeros(600)
    one[300] = 3.0
    cum, Z = cgo.cum_columns(one[:, None])
    for u in (0.0, 0.3, top):
        assert cgo.choose(cum[:, 0], float(Z[0]), u) == cgo.choose_linear(cum[:, 0], float(Z[0]), u) == 300
    # u = 0 on a column whose first cell is positive
    cum, Z = cgo.cum_columns(np.array([[0.5], [0.5]]))
    assert cgo.choose(cum[:, 0], 1.0, 0.0) == 0 and cgo.choose(cum[:, 0], 1.0, 0.5) == 1


def test_the_fallback_is_out_of_reach_for_normal_Z_and_reached_below():
    """fl(u Z) < Z for every u < 1 and every Z > 2^-1022: u <= 1 - 2^-53, so u Z <= Z - Z 2^-53; the gap below Z is
    2^(e-53) at Z = 2^e (the product is then Z's predecessor exactly) and 2^(e-52) > Z 2^-53 > half of it otherwise (the
    product lies nearer the predecessor).  At Z = 2^-1022 the gap below is a subnormal's 2^-1074, the product a tie that
    goes to the even Z; below that Z 2^-53 is under half a gap.  So the fallback is reachable, at Z <= 2^-1022 only."""
    top = 1.0 - 2.0 ** -53
    rng = np.random.default_rng(1)
    Zs = [1.0, 2.0 ** -1021, np.nextafter(2.0 ** -1022, 1.0), 2.0 ** 1023, np.nextafter(2.0, 1.0), np.nextafter(1.0, 2.0), 0.75, 3.0,
          1e-300, 1e300, float(np.finfo(np.float64).max)]
    Zs += list(np.ldexp(1.0 + rng.random(2000), rng.integers(-1021, 1023, size=2000)))
    for Z in Zs:
        assert not cgo.fallback_reached(Z, top), Z
        assert np.float64(top) * np.float64(Z) == np.nextafter(np.float64(Z), 0.0), Z
    # the counter-examples
    assert cgo.fallback_reached(2.0 ** -1022, top)
    d = 2.0 ** -1074
    assert cgo.fallback_reached(d, 0.75) and not cgo.fallback_reached(d, 0.25)
    # ... and the rule stays total there: two cells of the smallest subnormal, Z = 2 d
    col = np.zeros(9)
    col[3] = col[7] = d
    cum, Z = cgo.cum_columns(col[:, None])
    c, Z = cum[:, 0], float(Z[0])
    assert Z == 2 * d
    assert [cgo.choose(c, Z, u) for u in (0.1, 0.4, 0.6, 0.9, top)] == [3, 7, 7, 7, 7]
    assert [cgo.choose_linear(c, Z, u) for u in (0.1, 0.4, 0.6, 0.9, top)] == [3, 7, 7, 7, 7]
    assert cgo.fallback_reached(Z, 0.9) and not cgo.fallback_reached(Z, 0.6)


def test_wrong_replays_are_told_apart_by_bits():
    m = cgo.MUT_CASE
    rng = np.random.default_rng(m["seed"])
    lik = cgo.matrix_with_zeros(m["rows"], m["stride"], m["seed"])
    # a customer whose threshold is a cumulative sum exactly: the one place where >= and > part
    cum, Z = cgo.cum_columns(lik)
    cust = rng.integers(0, m["stride"], size=m["C"])
    cls0 = np.full(m["C"], 0xABCD, dtype=np.uint32)
    want, info = cgo.sample_classes(lik, cust, m["seed"], m["sweep"], cls0)
    assert info == (0, 0, m["C"]) and want.max() < m["rows"]
    got, _ = cgo.sample_classes(lik, cust, m["seed"], m["sweep"], cls0, mut="u3")
    assert not np.array_equal(got, want)
    # the plain sum: other bits in cum and Z, and a threshold between the two sums of a row sends the customer elsewhere
    pcum, pZ = cgo.cum_columns(lik, plain=True)
    k = 2
    assert pZ[k].tobytes() != Z[k].tobytes()
    parted = 0
    for w in (w for w in range(257, 513) if pcum[w, k] != cum[w, k] and lik[w, k] > 0.0):
        j0 = int(round(min(pcum[w, k], cum[w, k]) / Z[k] * 2.0 ** 53))
        for j in range(j0 - 2, j0 + 3):           # the uniforms whose thresholds lie about the row's two sums
            u = j * 2.0 ** -53
            parted += cgo.choose(cum[:, k], float(Z[k]), u) != cgo.choose(pcum[:, k], float(pZ[k]), u)
    assert parted >= 10, parted
    # (the case's own stream cannot part these two, nor > from >=: the sums differ by a few units of 2^-53 relative, and a
    # threshold equals a sum only by such a coincidence -- some 10^-13 a customer.  So the uniforms are built for it.)
    # >= for >, on the fixed case: the uniforms whose threshold is a row's cumulative sum to the bit
    hits = 0
    for w in (w for w in range(1, 512) if cum[w - 1, k] < cum[w, k] < Z[k]):   # (at the last growth both forms agree)
        j0 = int(round(cum[w, k] / Z[k] * 2.0 ** 53))
        for j in range(j0 - 2, j0 + 3):
            u = j * 2.0 ** -53
            if u * Z[k] == cum[w, k]:
                hits += 1
                a, b = cgo.choose(cum[:, k], float(Z[k]), u), cgo.choose(cum[:, k], float(Z[k]), u, ge=True)
                assert b == w and a > w and lik[a, k] > 0.0, (w, a, b)
    assert hits >= 10, hits
    # ... and on dyadic weights, so that u Z lands on a cumulative sum for the u = j / 8 a column of eight equal cells gives
    lik8 = np.full((8, 1), 0.125)
    cum8, Z8 = cgo.cum_columns(lik8)
    assert float(Z8[0]) == 1.0
    assert [cgo.choose(cum8[:, 0], 1.0, j / 8.0) for j in range(8)] == list(range(8))
    assert [cgo.choose(cum8[:, 0], 1.0, j / 8.0, ge=True) for j in range(8)] == [0] + list(range(7))
    assert cgo.choose(cum[:, 0], float(Z[0]), 0.0, ge=True) == 0 and lik[0, 0] == 0.0     # ... and picks a class of no weight


def test_masked_skipped_and_stuck_customers_keep_their_class():
    lik = cgo.matrix_with_zeros(300, 6, 9, zero_col=4)
    rng = np.random.default_rng(2)
    C = 500
    cust = rng.integers(0, 8, size=C)                   # dishes 6, 7 are past the stride
    mask = (rng.random(C) < 0.6).astype(np.uint8)
    cls0 = rng.integers(0, 300, size=C).astype(np.uint32)
    got, (skipped, stuck, drawn) = cgo.sample_classes(lik, cust, 3, 1, cls0, mask)
    live = mask != 0
    assert skipped == int((live & (cust >= 6)).sum()) > 0 and stuck == int((live & (cust == 4)).sum()) > 0
    assert skipped + stuck + drawn == int(live.sum())
    keep = ~live | (cust >= 6) | (cust == 4)
    assert np.array_equal(got[keep], cls0[keep])
    full, _ = cgo.sample_classes(lik, cust, 3, 1, cls0)
    assert np.array_equal(got[~keep], full[~keep])      # a class does not depend on who shares the call
    assert np.all(lik[got[~keep], cust[~keep]] > 0.0)


# ---- the law of the replay

def test_the_law_of_the_replay():
    lik = cgo.law_matrix()
    D, n = cgo.LAW_DISHES, cgo.LAW_DRAWS
    assert np.allclose(lik.sum(axis=0), 1.0)
    for k in range(D):
        assert cgo.merged_mass(lik[:, k], n) <= 0.02, (k, cgo.merged_mass(lik[:, k], n))
    cust = np.repeat(np.arange(D), n)
    cls, info = cgo.sample_classes(lik, cust, cgo.LAW_SEED, cgo.LAW_SWEEP, np.zeros(D * n, dtype=np.uint32))
    assert info == (0, 0, D * n)
    for k in range(D):
        mine = cls[k * n:(k + 1) * n]
        p = cgo.hist_p(mine, lik[:, k], n)
        q = cgo.hist_p(mine, lik[:, (k + 1) % D], n)
        print("dish", k, "p", p, "against the next dish's column", q)
        assert p > 1e-3 and q < 1e-9


# ---- the joint law through replays

@lru_cache(maxsize=None)
def joint_chain():
    """the joint-law case: (the cells after generate, the cells after JOINT_ROUNDS of (dish sweep, class draw), the
    classes changed per round)"""
    K, h, bpar, coff, lik = cgo.joint_case()
    seed, a = cgo.JOINT_SEED, cgo.JOINT_A
    rp = cgo.generate(K, h, a, bpar, coff, lik, seed=seed, sweep=0)
    assert rp["cls_info"] == (0, 0, 3 * cgo.JOINT_I) and (rp["skipped"], rp["impossible"], rp["stuck"]) == (0, 0, 0)
    first = cgo.joint_cells(rp["cust"], rp["t"], rp["cls"])
    vt = tio.ExactV([1, 2, 3], a)
    n, t, cust, cls = rp["n"], rp["t"], rp["cust"], rp["cls"]
    changed = []
    for r in range(1, cgo.JOINT_ROUNDS + 1):
        n, t, _, cust, skipped, stuck = tdo.sweep(K, n, t, h, a, bpar, vt, 3, 3, seed, r, cust, cls, lik)
        assert (skipped, stuck) == (0, 0)
        new, _ = cgo.sample_classes(lik, cust, seed, r, cls)
        changed.append(int((new != cls).sum()))
        cls = new
    return first, cgo.joint_cells(cust, t, cls), changed


def test_generate_and_the_alternation_keep_the_joint_law():
    law = cgo.joint_law()
    total = cgo.JOINT_I
    assert cgo.merged_mass(list(law.values()), total) <= 0.02
    first, last, changed = joint_chain()
    p0, p1 = sto.chi2_p(first, law, total), sto.chi2_p(last, law, total)
    wrong = cgo.joint_law(cgo.swapped(cgo.JOINT_LIK))
    q = sto.chi2_p(last, wrong, total)
    print("generate p", p0, "after the rounds p", p1, "columns exchanged p", q, "classes changed", changed)
    assert p0 > 1e-3 and p1 > 1e-3 and q < 1e-9
    assert min(changed) >= 1
