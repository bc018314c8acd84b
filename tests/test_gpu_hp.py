"""Every numeric device output against the high-precision truth (tests/hp_oracle.py) under the error model written out
there: log S tables of every fill form, S^n_1, float tables, V tables, the fused / grid / table-then-sweep `aterms` sums
over pairs placed where fused walks go wrong, restaurant terms and `bterms`.  The oracle's 1e-10 bar (the other test
files) stays; this one is 10^3 times tighter where the oracle itself is off by tens of units of 2^-53."""
import ctypes as C

import numpy as np
import pytest

import hp_oracle as hp
import orc
from hp_pairs import (FORMS, XS, Counters, _aterms, _check_sums, _create, _note, aterms_truth, check_form, expected_form,
                      grid_geometry, hb_geometry, targeted_pairs, walk_geometry)
from libstb_amd import capi, synth

pytestmark = pytest.mark.gpu

U = hp.U
EXTREME = [0.0, 5e-324, 3 * 2.0 ** -30, 0.01, 0.37, 0.5, 0.98, 0.999, 0.99999, 1 - 2.0 ** -20]
MIXED = [0.0, 0.5, 0.999, 5e-324]
LINEAR = [capi.FILL_SCALED, capi.FILL_HB, capi.FILL_PC, capi.FILL_CHAIN]

_truth = {}


def truth(a, N, M, want_v=False):
    """the truth of (a..., N, M) in packed orders, cached per module"""
    key = (tuple(float(x) for x in np.atleast_1d(a)), N, M, want_v)
    if key not in _truth:
        _truth[key] = hp.tables(list(key[0]), N, M, want_v)
    return _truth[key]


def check_S(form, T, a, N, M):
    """every cell and S^n_1 of the device tables T (one per discount in a) against the truth under the model bar"""
    n, _ = hp.cell_coords(N, M)
    tr = truth(a, N, M)
    for d, ad in enumerate(a):
        S1t, St, _ = tr[d]
        got = T.packed_host(d)
        assert got.shape == St.shape
        if St.size:
            b = hp.bar(n, ad, St.astype(np.float64))
            e = hp.err(got, St).astype(np.float64)
            r = float(np.max(e / b))
            _note(form, ad, r)
            assert r <= 1.0, (form, ad, N, M, r, int(np.argmax(e / b)))
        g1 = T.S1[d].cpu().numpy()
        n1 = np.arange(1, N + 1)
        r1 = float(np.max(hp.err(g1, S1t).astype(np.float64) / hp.s1bar(n1, ad, S1t.astype(np.float64))))
        _note(form + ":S1", ad, r1)
        assert r1 <= 1.0, (form, "S1", ad, r1)


def check_logdomain(T, a, N, M):
    """FILL_LOGDOMAIN follows the reference's order: its worst error against the truth <= 4x the oracle's + 1e-15, for
    the cells and for S^n_1 (the running sum of log((n-1) - a) that column 1 of this form carries)"""
    tr = truth(a, N, M)
    for d, ad in enumerate(a):
        S1t, St, _ = tr[d]
        S1o, tab = orc.fill_S(ad, N, M)
        pairs = [("S1", T.S1[d].cpu().numpy(), S1o, S1t)]
        if St.size:
            pairs.append(("cells", T.packed_host(d), tab, St))
        for what, got, orac, want in pairs:
            eo = float(np.max(hp.scaled_err(orac, want)))
            eg = float(np.max(hp.scaled_err(got, want)))
            _note(f"logdomain:{what}(x oracle)", ad, eg / (4 * eo + 1e-15))
            assert eg <= 4 * eo + 1e-15, (what, ad, N, M, eg, eo)


RAGGED = [(3, 2), (10, 10), (65, 33), (130, 129), (500, 7), (1000, 1000), (1500, 260)]


@pytest.mark.parametrize("variant", LINEAR + [capi.FILL_LOGDOMAIN])
@pytest.mark.parametrize("N,M", RAGGED)
def test_fill_forms_against_the_truth(N, M, variant):
    """the ragged shapes of test_ragged_shapes_vs_oracle, all ten extreme discounts in one batched call"""
    a = np.array(EXTREME)
    T = capi.DeviceTables(N, M, D=len(a))
    T.tables.fill_(float("nan"))
    T.fill(a, variant)
    T.status()
    if variant == capi.FILL_LOGDOMAIN:
        check_logdomain(T, a, N, M)
    else:
        check_S(f"variant{variant}", T, a, N, M)


@pytest.mark.parametrize("N,M,a", [(30000, 60, (0.37, 0.999)), (70000, 130, (0.5,))])
def test_tall_narrow_tables_against_the_truth(N, M, a):
    """one or two strips, thousands of blocks, row counts beyond 2^14 and 2^16 (the halo-block form)"""
    a = np.array(a)
    T = capi.DeviceTables(N, M, D=len(a))
    T.tables.fill_(float("nan"))
    L = capi.lib()
    before = L.stb_fill_fallbacks()
    T.fill(a, capi.FILL_HB)
    T.status()
    assert L.stb_fill_fallbacks() == before
    check_S("hb-tall", T, a, N, M)


@pytest.mark.parametrize("D,N", [(3, 1200), (8, 1200), (64, 1500)])
def test_batched_extremes_against_the_truth(D, N):
    """D tables in one default-form call, 0, 5e-324 and a near 1 mixed among ordinary discounts"""
    a = np.resize(np.array(MIXED + EXTREME + list(synth.discount_grid(64))), D)
    T = capi.DeviceTables(N, N, D=D)
    T.tables.fill_(float("nan"))
    T.fill(a)
    T.status()
    check_S(f"default-D{D}", T, a, N, N)


GEOMETRIES = [("hb", {"STB_HB_C": "1", "STB_HB_P": "3", "STB_HB_ROWS": "16"}, capi.FILL_HB),
              ("hb", {"STB_HB_C": "4", "STB_HB_P": "2", "STB_HB_ROWS": "24"}, capi.FILL_HB),
              ("hb", {"STB_HB_C": "2", "STB_HB_P": "7", "STB_HB_ROWS": "48"}, capi.FILL_HB),
              ("pc", {"STB_FILL_R": "60"}, capi.FILL_PC),
              ("pc", {"STB_PC_CONSUMERS": "3", "STB_FILL_R": "32"}, capi.FILL_PC)]


@pytest.mark.parametrize("name,env,variant", GEOMETRIES, ids=[f"{g[0]}-" + "-".join(g[1].values()) for g in GEOMETRIES])
def test_geometries_against_the_truth(monkeypatch, name, env, variant):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a = np.array(MIXED)
    N, M = 900, 700
    T = capi.DeviceTables(N, M, D=len(a))
    T.tables.fill_(float("nan"))
    T.fill(a, variant)
    T.status()
    check_S(f"{name}-geom", T, a, N, M)


def test_full_table_against_the_truth():
    """all 49 985 001 cells of one N = M = 10^4 table in the default form, row by row against the streamed truth"""
    N = M = 10000
    a = 0.37
    T = capi.DeviceTables(N, M, D=1)
    T.tables.fill_(float("nan"))
    T.fill([a])
    T.status()
    tab = T.tables[0].cpu().numpy()
    S1 = T.S1[0].cpu().numpy()
    worst = worst1 = 0.0
    for n, v, e in hp.rows([a], N, M):
        lg = hp.logs(v, e)[0]
        r1 = float(hp.err(S1[n - 1:n], lg[1:2])[0]) / float(hp.s1bar(n, a, float(lg[1])))
        assert r1 <= 1.0, ("S1", n, r1)                 # (a NaN fails here too)
        worst1 = max(worst1, r1)
        if n < 3:
            continue
        ln = min(n - 2, M - 1)
        o = T.rowoff(n)
        t = lg[2:2 + ln]
        r = hp.err(tab[o:o + ln], t).astype(np.float64) / hp.bar(n, a, t.astype(np.float64))
        assert np.all(r <= 1.0), (n, float(np.nanmax(r)), int(np.count_nonzero(~(r <= 1.0))))
        worst = max(worst, float(r.max()))
    _note("default-10^4", a, worst)
    _note("default-10^4:S1", a, worst1)


# ------------------------------------------------------------------------------------------------ float and V tables

def test_float_tables_against_the_truth():
    """S_FLOAT written by the halo-block fill (stb_fill_Sf) and narrowed from a double slab (stb_table_to_float): each cell
    is float32(truth) but where the truth lies within its double bar of a float rounding boundary (one ulp, counted)"""
    N = M = 1500
    a = np.array(MIXED + [0.37, 0.99999])
    L = capi.lib()
    assert L.stb_fill_takes_kind(N, M, len(a), 1)
    F = capi.DeviceFloatTables(N, M, D=len(a))
    F.tables.fill_(float("nan"))
    F.fill(a)
    T = capi.DeviceTables(N, M, D=len(a))
    T.fill(a)
    torch = capi._torch()
    narrowed = torch.empty_like(T.tables, dtype=torch.float32)
    capi.check(L.stb_table_to_float(T.tables.data_ptr(), narrowed.data_ptr(), T.tables.numel(), capi.stream_ptr()))
    torch.cuda.synchronize()
    n, _ = hp.cell_coords(N, M)
    tr = truth(a, N, M)
    for route, tabs in (("Sf", F), ("to_float", None)):
        allowed = 0
        for d, ad in enumerate(a):
            _, St, _ = tr[d]
            if tabs is None:
                full = narrowed[d].cpu().numpy()
                got = np.concatenate([full[T.rowoff(k):T.rowoff(k) + min(k - 2, M - 1)] for k in range(3, N + 1)])
            else:
                got = tabs.packed_host(d)
            bad, ok = hp.float_rule(got, St, hp.bar(n, ad, St.astype(np.float64)))
            allowed += ok
            assert bad == 0, (route, ad, bad)
            r1 = float(np.max(hp.err(F.S1[d].cpu().numpy(), tr[d][0]).astype(np.float64)
                              / hp.s1bar(np.arange(1, N + 1), ad, tr[d][0].astype(np.float64))))
            assert r1 <= 1.0, (route, ad, r1)
        print(f"float tables ({route}): {allowed} of {len(a) * n.size} cells took the one-ulp allowance")


def _vcheck(form, got, Vt, n, ad):
    ok = np.isfinite(Vt.astype(np.float64))
    b = hp.vbar(n[ok], ad, Vt[ok].astype(np.float64))
    r = float(np.max(hp.err(got[ok], Vt[ok]).astype(np.float64) / b))
    _note(form, ad, r)
    assert r <= 1.0, (form, ad, r)
    return b, ok


@pytest.mark.parametrize("N,M", [(1500, 1500), (2000, 900)])
def test_V_tables_against_the_truth(N, M):
    """V^n_m = S^n_m / S^n_{m-1} as double (stb_fill_V: the block-floating cells divided, 512 rows and up) under the
    ratio bar, and as float (stb_fill_Vf) under the float rule with that bar"""
    a = np.array(MIXED + [0.37, 0.98])
    n, _ = hp.vcell_coords(N, M)
    tr = truth(a, N, M, want_v=True)
    V = capi.DeviceVTables(N, M, D=len(a))
    V.tables.fill_(float("nan"))
    V.fill(a)
    Vf = capi.DeviceVTables(N, M, D=len(a), dtype="f32")
    Vf.tables.fill_(float("nan"))
    Vf.fill(a)
    allowed = 0
    for d, ad in enumerate(a):
        Vt = tr[d][2]
        b, ok = _vcheck("V-f64", V.packed_host(d), Vt, n, ad)
        bad, k = hp.float_rule(Vf.packed_host(d)[ok], Vt[ok], b)
        allowed += k
        assert bad == 0, ("V-f32", ad, bad)
    print(f"V as float: {allowed} cells took the one-ulp allowance")


@pytest.mark.parametrize("N,exact", [(300, False), (2000, True)])
def test_V_reference_recurrence_against_the_truth(N, exact):
    """the reference's own V recurrence (stb_fill_V_exact; stb_fill_V below 512 rows) drifts with n: its worst error
    against the truth at most 4x the oracle's on the same table, + 1e-15"""
    M = N
    a = np.array([0.01, 0.37, 0.5, 0.98])
    tr = truth(a, N, M, want_v=True)
    V = capi.DeviceVTables(N, M, D=len(a))
    V.fill(a, exact=exact)
    for d, ad in enumerate(a):
        Vt = tr[d][2]
        ok = np.isfinite(Vt.astype(np.float64))
        o = orc.fill_V(ad, N, M)
        eo = float(np.max(np.abs(o[ok].astype(hp.LD) / Vt[ok] - 1)))
        eg = float(np.max(np.abs(V.packed_host(d)[ok].astype(hp.LD) / Vt[ok] - 1)))
        _note("V-exact(x oracle)", ad, eg / (4 * eo + 1e-15))
        assert eg <= 4 * eo + 1e-15, (ad, eg, eo)


# ------------------------------------------------------------------------------------------------ aterms sums

NP = 1500


@pytest.fixture(scope="module")
def shared_rule_off():
    """the automatic shared-GPU rule pinned off (a slow launch on a busy machine would send every later evaluation through
    stored tables, silently), and restored"""
    L = capi.lib()
    L.stb_set_shared_gpu(0)
    try:
        yield L
    finally:
        L.stb_set_shared_gpu(-1)


@pytest.mark.parametrize("name,env,Ds", FORMS, ids=[f[0] for f in FORMS])
def test_aterms_forms_against_the_truth(monkeypatch, shared_rule_off, name, env, Ds):
    """each fused / grid / two-pass form, forced through its switch, on the targeted pairs; the form the library reports
    (stb_groups_last_form) is the one the case names, its strips the mirrored geometry, and no evaluation fell back"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    L = shared_rule_off
    geoms, _ = walk_geometry(NP, NP)
    if "STB_GRID_C" in env:                              # the form's own strips are among those the pairs straddle
        gc = C.c_int()
        assert L.stb_grid_shape(NP, NP, max(Ds), C.byref(gc), None, None) == 0 and gc.value == int(env["STB_GRID_C"])
        assert grid_geometry(NP, gc.value) in geoms
    if "STB_HB_DOT_C" in env:
        assert hb_geometry(NP, int(env["STB_HB_DOT_C"])) in geoms
    K, n, t, T, bpar, cls = targeted_pairs(NP, NP)
    want = aterms_truth(K, n, t, T, bpar, XS, NP, NP, cls)
    watch = Counters(L)
    h = _create(L, K, n, t, T, bpar, NP, NP, max(Ds))
    try:
        for D in Ds:
            _check_sums(name, _aterms(L, h, XS[:D]), want[:D])
            check_form(L, h, f"{name}-D{D}", expected_form(name, env, NP), NP)
        _check_sums(name + "-tables", _aterms(L, h, XS[:max(Ds)], tables=True), want[:max(Ds)])
        check_form(L, h, name + "-tables", expected_form("tables", {}, NP), NP)
        watch.check(name)
    finally:
        L.stb_groups_free(h)


def test_aterms_on_pairs_made_new_and_log_zero():
    """a kept set given new pairs through stb_groups_pairs_begin / _put / _commit (the slab-built lists) against the truth
    of the new pairs; a pair outside the support (t > n) gives -inf"""
    L = capi.lib()
    K, n, t, T, bpar, _ = targeted_pairs(NP, NP)
    K2, n2, t2, T2, bpar2, _ = targeted_pairs(NP, NP, seed=99)
    assert np.array_equal(K, K2)
    x = XS[:8]
    h = _create(L, K, n, t, T, bpar, NP, NP, len(x))
    try:
        _check_sums("fused", _aterms(L, h, x), aterms_truth(K, n, t, T, bpar, x, NP, NP))
        mn, mt = C.c_uint(), C.c_uint()
        capi.check(L.stb_groups_pairs_begin(h))
        off = 0
        for k in K.tolist():
            capi.check(L.stb_groups_pairs_put(h, orc.u32p(n2[off:off + k].copy()), orc.u16p(t2[off:off + k].copy()), k,
                                              C.byref(mn), C.byref(mt)))
            off += k
        capi.check(L.stb_groups_pairs_commit(h, orc.u32p(T2), orc.dp(bpar2), NP, NP))
        _check_sums("new-pairs", _aterms(L, h, x), aterms_truth(K, n2, t2, T2, bpar2, x, NP, NP))
        nb, tb = n2.copy(), t2.copy()
        nb[5], tb[5] = 5, 9
        capi.check(L.stb_groups_update_pairs(h, orc.u32p(nb), orc.u16p(tb)))
        assert np.all(np.isneginf(_aterms(L, h, x)))
    finally:
        L.stb_groups_free(h)


# ------------------------------------------------------------------------------------------------ restaurant terms, bterms

def _groups(T, bpar):
    I = len(T)
    K = np.ones(I, dtype=np.int32)
    g = synth.Groups(I=I, K=K, n=np.asarray(T, dtype=np.uint32), t=np.ones(I, dtype=np.uint16),
                     T=np.asarray(T, dtype=np.uint32), N=np.asarray(T, dtype=np.uint32),
                     bpar=np.asarray(bpar, dtype=np.float64))
    return g


def test_restaurant_terms_and_bterms_against_mpmath():
    """capi.restaurant_terms, capi.bterms and stb_bterms_eval against the mpmath terms: b/x on and next to lgamma's zeros
    (1 and 2), tiny and huge arguments, large T"""
    T = np.array([1, 1, 2, 5, 40, 1000, 60000, 3, 7, 1])
    xs = np.array([0.5, 0.25, 0.999, 0.01, 0.37])
    bpar = np.array([0.5, 0.5000001, 1.0, 0.9999999, 0.74, 2.0, 3.7, 1e-6, 500.0, 0.25])   # b/x = 1 and 2 at x = 0.5, 0.25
    g = _groups(T, bpar)
    dg = capi.DeviceGroups(g)
    got = capi.restaurant_terms(xs, dg).cpu().numpy()
    for d, x in enumerate(xs):
        tv, tb = hp.LD(0), 0.0
        for i in range(len(T)):
            v, b = hp.restaurant_term(x, int(T[i]), float(bpar[i]))
            tv += hp.LD(v)
            tb += b
        tb += 4 * U * abs(float(tv))
        e = abs(float(hp.LD(got[d]) - tv))
        _note("restaurant_terms", x, e / tb)
        assert e <= tb, (x, got[d], float(tv), e, tb)
    Q, shape = 0.8, 1.1
    for apar in (0.5, 0.3):
        bx = np.array([apar, 2 * apar, 1e-3, 0.9 * apar, 250.0])        # x/apar = 1, 2, tiny, near 1, large
        got = capi.bterms(bx, Q, shape, apar, dg).cpu().numpy()
        h = capi.lib().stb_bterms_create(g.T.ctypes.data_as(capi.c_u32_p), g.I)
        assert h, capi.last_error()
        try:
            ev = np.zeros(len(bx))
            capi.check(capi.lib().stb_bterms_eval(h, capi.dp(np.ascontiguousarray(bx)), len(bx), Q, shape, apar, capi.dp(ev)))
        finally:
            capi.lib().stb_bterms_free(h)
        for d, x in enumerate(bx):
            tv, tb = hp.bterms(x, Q, shape, T, apar)
            tb += 4 * U * abs(tv)
            for form, val in (("bterms", got[d]), ("bterms_eval", ev[d])):
                e = abs(val - tv)
                _note(form, x, e / tb)
                assert e <= tb, (form, apar, x, val, tv, e, tb)
