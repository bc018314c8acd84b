"""The table-free `aterms` forms against the long-double truth at the shapes a sampler works at (test_gpu_hp.py holds them
to it at N = M = 1500 only): blocks of 40, 32 and 24 rows, strips that end at M instead of the diagonal, a last strip of
one column, 7 strips a workgroup, strip records read from global memory, the default dispatch on sparse pairs, a kept set
with one discount and with new bounds -- each case asserting which form the library reports it ran
(stb_groups_last_form), that its strips are the mirrored geometry, and that nothing fell back.  And stb_hist_aterms2
against mpmath.

Every shape takes two pair sets (hp_pairs.targeted_pairs): the targeted set (at most 1/3 of the cells) and the same classes
thinned to 0.04 of the cells, where the default dispatch is the grid form's and the lists are the dense words of
k_emit_both.  Where the pairs that are never dropped alone exceed 0.04 of the cells (1250 x 81 and x 82) there is no second
set; test_hp_shapes_host.py pins that.

Cuts made before anything ran, for the time the truth takes on one CPU thread: shapes of 4001 rows and more evaluate at
most 16 discounts a call (the D = 29 and 64 cases of FORMS become D = 16 there).

Sensitivity (hp_pairs.Truth.margin, printed with every sum): the nearest neighbouring cell of any pair of a sum against
the sum's bar; above 1, one pair answered from the cell beside or above it cannot hide.  test_hp_shapes_host.py asserts it
on the CPU for every class sum of every shape up to 140000 x 90 at the discounts of the hand-over, and for the whole-set
sums below 30000 rows.  From 30000 rows on the whole-set sums do not meet it (10^5 .. 10^6 pairs under one bar): there
the class sums are the ones that count, with the two classes of whole rows handed over in 64 pieces by row
(hp_pairs.chunk_of).  The (shape, class, discount, piece) sums that still cannot meet it are listed by name in
hp_pairs.CANNOT_HOLD -- mostly a = 0.5 on rows beyond ~35000 -- and asserted to be exactly those.  The 10^4 and 46000
cases check whole-set sums only; their margins are printed (46000, a = 0.01: 2.2; the sparse set at 10^4: 3.1 at a = 0.01,
below 1 at 0.5, 0.999 and 0.99999)."""
import ctypes as C

import numpy as np
import pytest

import hp_oracle as hp
import hp_pairs as P
import orc
from hp_pairs import FORMS, LOC, NO_SPARSE_SET, XS, Counters, _aterms, _check_sums, _create, _note, check_form, expected_form
from libstb_amd import capi

pytestmark = pytest.mark.gpu

CHEAP = [(1201, 209), (1202, 210), (1250, 81), (1250, 82), (1250, 145), (1250, 146), (1300, 465), (1300, 466)]
MID = [(4001, 301), (4001, 1001)]
TALL = [(30000, 60), (70000, 130), (140000, 90)]
# block rows (hb2, hb3, hb4, grid): min(48, stb_period_rows(N)) cut to a multiple of 8 (of 24 with 3 columns a lane) -- the
# period is 63 rows up to N = 16384, 46 up to 131072, 39 beyond; the mirrored formulas must give these, and the library too
BLOCK_ROWS = {30000: (40, 24, 40, 40), 70000: (40, 24, 40, 40), 140000: (32, 24, 32, 32), 10000: (48, 48, 48, 48),
              46000: (40, 24, 40, 40)}


def dcap(N):
    return 64 if N < 4001 else 16


def pair_sets(N, M):
    """[(set name, pairs)]: the targeted set, G <= cells / 3, and the sparse targeted set, G <= 0.04 cells"""
    out = [("targeted", P.targeted_pairs(N, M, rho=1.0 / 3.0))]
    if (N, M) not in NO_SPARSE_SET:
        out.append(("sparse", P.targeted_pairs(N, M, rho=0.04)))
    return out


_shape = {}


def shape_truth(N, M, D, sets=None):
    """(the pair sets of a shape, their truths at XS[:D]), one pass over the truth's rows, cached for the module"""
    key = (N, M, D)
    if key not in _shape:
        sets = sets if sets is not None else pair_sets(N, M)
        _shape[key] = (sets, P.aterms_truth_by_class([s[1] for s in sets], XS[:D], N, M))
    return _shape[key]


@pytest.fixture(scope="module", autouse=True)
def shared_rule_off():
    """the automatic shared-GPU rule pinned off for the module and restored: with it off a walk that gives up on a busy
    machine is a counted fallback and a failed assertion, not a silent pass through stored tables"""
    L = capi.lib()
    L.stb_set_shared_gpu(0)
    try:
        yield L
    finally:
        L.stb_set_shared_gpu(-1)


def check_mirrors(N, M):
    """the mirrored geometries against the library, and against the block rows of BLOCK_ROWS"""
    P.walk_geometry(N, M)
    rows = (P.hb_geometry(N, 2)[0], P.hb_geometry(N, 3)[0], P.hb_geometry(N, 4)[0], P.grid_geometry(N, 4)[0])
    assert rows == BLOCK_ROWS.get(N, (48, 48, 48, 48)), (N, rows)


def run_form(L, N, M, name, env, Ds, sets, truths, D_of=None):
    """one form on every pair set of a shape: each D of Ds (discounts XS[:D], or D_of(D) tiled) under the bar, the form
    reported, the counters unchanged; then the same sums through stored tables"""
    if "STB_GRID_C" in env:
        gc = C.c_int()
        rc = L.stb_grid_shape(N, M, max(Ds), C.byref(gc), None, None)
        assert rc == 0 and gc.value == int(env["STB_GRID_C"]), ("the grid form refuses this shape", N, M, rc, gc.value)
    for (sname, (K, n, t, T, bpar, _)), tr in zip(sets, truths):
        want = tr.sums()
        print(f"{N}x{M} {sname}: G = {len(n)} ({len(n) / P.table_cells(N, M):.4f} of the cells), whole-set margin {tr.margin()[:max(Ds)]}")
        watch = Counters(L)
        h = _create(L, K, n, t, T, bpar, N, M, max(Ds))
        try:
            for D in Ds:
                idx = np.arange(D) if D_of is None else D_of(D)
                label = f"{name}-{N}x{M}-{sname}-D{D}"
                _check_sums(label, _aterms(L, h, XS[idx]), [want[i] for i in idx])
                check_form(L, h, label, expected_form(name, env, N), N)
            D = max(Ds)
            idx = np.arange(D) if D_of is None else D_of(D)
            _check_sums(f"{name}-tables-{N}x{M}-{sname}", _aterms(L, h, XS[idx], tables=True), [want[i] for i in idx])
            check_form(L, h, f"{name}-tables-{N}x{M}-{sname}", expected_form("tables", {}, N), N)
            watch.check((name, N, M, sname))
        finally:
            L.stb_groups_free(h)


@pytest.mark.parametrize("name,env,Ds", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("N,M", CHEAP + MID + TALL, ids=lambda v: str(v))
def test_forms_at_working_shapes(monkeypatch, N, M, name, env, Ds):
    """every form of FORMS on both pair sets of every shape up to 140000 x 90"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    L = capi.lib()
    check_mirrors(N, M)
    Ds = tuple(sorted({min(D, dcap(N)) for D in Ds}))
    sets, truths = shape_truth(N, M, dcap(N))
    run_form(L, N, M, name, env, Ds, sets, truths)


@pytest.mark.parametrize("N,M", CHEAP + MID + TALL, ids=lambda v: str(v))
def test_classes_one_at_a_time(N, M):
    """after the whole-set check, each class alone in the same kept set (stb_groups_update_pairs; the set keeps G, the rest
    are (1, 1) pairs, which contribute nothing); from 30000 rows on the two classes of whole rows go in 64 pieces by row: a
    failure names the class and the piece, under the bar of those pairs alone"""
    L = capi.lib()
    sets, truths = shape_truth(N, M, dcap(N))
    x = XS[LOC]
    for (sname, (K, n, t, T, bpar, cls)), tr in zip(sets, truths):
        watch = Counters(L)
        h = _create(L, K, n, t, T, bpar, N, M, len(x))
        try:
            whole = tr.sums()
            _check_sums(f"classes-{N}x{M}-{sname}-all", _aterms(L, h, x), [whole[i] for i in LOC])
            piece = P.chunk_of(N, n, cls)
            for c, cname in enumerate(P.CLASSES):
                for k in tr.chunks(c):
                    sel = (cls == c) & (piece == k)
                    nc = np.where(sel, n, 1).astype(np.uint32)
                    tc = np.where(sel, t, 1).astype(np.uint16)
                    capi.check(L.stb_groups_update_pairs(h, orc.u32p(nc), orc.u16p(tc)))
                    want = tr.sums([c], k)
                    label = f"classes-{N}x{M}-{sname}-{cname}" + (f"-piece{k}" if len(tr.chunks(c)) > 1 else "")
                    print(f"{label}: {int(np.count_nonzero(sel))} pairs, margin {tr.margin([c], k)[LOC]}")
                    _check_sums(label, _aterms(L, h, x), [want[i] for i in LOC])
                    check_form(L, h, label, {"fused": 1}, N)
            watch.check(("classes", N, M, sname))
        finally:
            L.stb_groups_free(h)


def _tiled(k):
    return lambda D: np.arange(D) % k


def test_working_scale_10k(monkeypatch):
    """10^4 x 10^4, 7 strips a workgroup in the summing halo-block form: hb4 at D = 3 and D = 24 (four truths tiled; the
    kernels do not know that they repeat) on both sets; on the sparse set the DEFAULT route at D = 64, which must be the
    grid form, and at D = 8, which must be the halo-block form"""
    N = M = 10000
    L = capi.lib()
    check_mirrors(N, M)
    sets, truths = shape_truth(N, M, 4)
    monkeypatch.setenv("STB_HB_DOT_C", "4")
    run_form(L, N, M, "hb4", {"STB_HB_DOT_C": "4"}, (3, 24), sets, truths, D_of=_tiled(4))
    monkeypatch.delenv("STB_HB_DOT_C")
    (sname, (K, n, t, T, bpar, _)), tr = sets[1], truths[1]
    assert sname == "sparse" and len(n) <= 0.04 * P.table_cells(N, M)
    want = tr.sums()
    watch = Counters(L)
    h = _create(L, K, n, t, T, bpar, N, M, 64)
    try:
        for D, which_ok in ((64, (3, 4, 5)), (8, (2,))):
            idx = np.arange(D) % 4
            _check_sums(f"default-10k-sparse-D{D}", _aterms(L, h, XS[idx]), [want[i] for i in idx])
            got = check_form(L, h, f"default-10k-sparse-D{D}", {"fused": 1, "sparse": 1}, N)
            assert got["which"] in which_ok, (D, got)
        watch.check("default-10k")
    finally:
        L.stb_groups_free(h)


def mirrored_hb_sum_C(N, M, Dmax):
    """fill_hb.hip stb_hb_sum_C: 2 columns a lane while Dmax tables' strips of 80 columns are at most 1.5 waves a compute
    unit, 3 while their strips of 144 are at most 2.25, else 4"""
    cus = capi._torch().cuda.get_device_properties(0).multi_processor_count
    cmax = min(M, N - 1)
    waves2, waves3 = Dmax * ((cmax - 1 + 79) // 80), Dmax * ((cmax - 1 + 143) // 144)
    return 2 if waves2 <= cus * 3 // 2 else (3 if waves3 <= cus * 9 // 4 else 4)


def test_record_offsets_from_global_memory_46k(monkeypatch):
    """46000 x 46000 with 2 columns a lane: blocks of 40 rows, strips of 88 own columns, 523 strips -- JW + 2 = 525 > 512
    (HB_RECOFF_LDS), so the summing instantiation of k_fill_hb reads its strip record offsets from global memory (41000
    columns are 466 such strips and stay in LDS; 46000 leaves 13 strips of margin should the library's count differ from
    the mirror's by one or two).  D = 2 with the same discount twice: forced hb2, then the DEFAULT route with the switch
    removed, which must report stb_hb_sum_C's own choice (4 columns a lane here, not the forced 2).  Edges on every 64th
    row so that G stays under 2 x 10^6."""
    N = M = 46000
    L = capi.lib()
    check_mirrors(N, M)
    UC = P.hb_geometry(N, 2)[1]
    assert (min(N - 1, M) - 1 + UC - 1) // UC + 2 >= 512 + 8
    cells = P.table_cells(N, M)
    pairs = P.targeted_pairs(N, M, stride=64, rho=2e6 / cells)
    assert len(pairs[1]) <= 2_000_000
    sets, truths = shape_truth(N, M, 1, sets=[("thin", pairs)])
    print(f"{N}x{M} thin: whole-set margin {truths[0].margin()}")
    monkeypatch.setenv("STB_HB_DOT_C", "2")
    run_form(L, N, M, "hb2", {"STB_HB_DOT_C": "2"}, (2,), sets, truths, D_of=_tiled(1))
    monkeypatch.delenv("STB_HB_DOT_C")
    want_C = mirrored_hb_sum_C(N, M, 2)
    assert want_C != 2
    K, n, t, T, bpar, _ = pairs
    want = truths[0].sums()
    watch = Counters(L)
    h = _create(L, K, n, t, T, bpar, N, M, 2)
    try:
        _check_sums(f"default-{N}x{M}-thin-D2", _aterms(L, h, XS[[0, 0]]), [want[0], want[0]])
        got = check_form(L, h, f"default-{N}x{M}-thin-D2", {"fused": 1, "sparse": 1}, N)
        assert got["which"] == 2 and got["C"] == want_C, (got, want_C)
        _check_sums(f"default-tables-{N}x{M}-thin", _aterms(L, h, XS[[0, 0]], tables=True), [want[0], want[0]])
        check_form(L, h, f"default-tables-{N}x{M}-thin", {"fused": 0}, N)
        watch.check("default-46k")
    finally:
        L.stb_groups_free(h)


# ------------------------------------------------------------------------------------------------ the reused-set route

def _hand_over(L, h, K, n, t, T, bpar, N, M):
    capi.check(L.stb_groups_pairs_begin(h))
    off = 0
    for k in K.tolist():
        capi.check(L.stb_groups_pairs_put(h, orc.u32p(n[off:off + k].copy()), orc.u16p(t[off:off + k].copy()), k, None, None))
        off += k
    capi.check(L.stb_groups_pairs_commit(h, orc.u32p(T), orc.dp(bpar), N, M))


@pytest.mark.parametrize("N,M,N2,M2", [(4001, 301, 3000, 400), (1500, 1500, 1700, 1300)])
def test_reused_set_single_discount_and_new_bounds(monkeypatch, N, M, N2, M2):
    """what samplea does between Gibbs iterations: a kept set (stb_groups_update_restaurants: new T and bpar) evaluates
    D = 1 fused, at several discounts; then new pairs arrive with NEW BOUNDS (both changed), the set is marked kept again,
    and D = 1 and D = 8 are held to the truth of the new pairs at the new bounds -- lists and strips must follow them"""
    monkeypatch.setenv("STB_ATERMS_FUSE1", "0")   # (a FRESH set's single discount goes through stored tables: fused == 1 is `reused`)
    L = capi.lib()
    K, n, t, T, bpar, cls = P.targeted_pairs(N, M, rho=1.0 / 3.0)
    T2 = (T + 3).astype(np.uint32)
    bpar2 = bpar[::-1].copy()
    tr = P.aterms_truth_by_class([(K, n, t, T2, bpar2, cls)], XS[:8], N, M)[0].sums()
    watch = Counters(L)
    h = _create(L, K, n, t, T, bpar, N, M, 8)
    try:
        fresh = P.aterms_truth_by_class([(K, n, t, T, bpar, cls)], XS[:1], N, M)[0].sums()
        _check_sums(f"fresh-{N}x{M}-D1", _aterms(L, h, XS[:1]), fresh)
        check_form(L, h, f"fresh-{N}x{M}-D1", {"fused": 0}, N)
        capi.check(L.stb_groups_update_restaurants(h, orc.u32p(T2), orc.dp(bpar2)))
        for d in range(8):
            _check_sums(f"reused-{N}x{M}-D1", _aterms(L, h, XS[d:d + 1]), tr[d:d + 1])
            check_form(L, h, f"reused-{N}x{M}-D1", {"fused": 1, "sparse": 1}, N)
        Kb, nb, tb, Tb, bparb, clsb = P.targeted_pairs(N2, M2, seed=99, rho=1.0 / 3.0)
        G = len(n)
        assert len(nb) != G                      # (the set keeps G: the new pairs are cut or padded with (1, 1) to it)
        if len(nb) >= G:
            nb, tb, clsb = nb[:G].copy(), tb[:G].copy(), clsb[:G].copy()
        else:
            pad = G - len(nb)
            nb = np.concatenate([nb, np.ones(pad, dtype=np.uint32)])
            tb = np.concatenate([tb, np.ones(pad, dtype=np.uint16)])
            clsb = np.concatenate([clsb, np.zeros(pad, dtype=np.int8)])
        Tb = np.add.reduceat(tb.astype(np.uint64), np.r_[0, np.cumsum(K)[:-1]]).astype(np.uint32)
        assert int(nb.max()) <= N2 and int(tb.max()) <= M2
        _hand_over(L, h, K, nb, tb, Tb, bparb, N2, M2)
        Nn, Mn = C.c_uint(), C.c_uint()
        capi.check(L.stb_groups_shape(h, None, None, C.byref(Nn), C.byref(Mn), None))
        assert (Nn.value, Mn.value) == (N2, M2)
        trb = P.aterms_truth_by_class([(K, nb, tb, Tb, bparb, clsb)], XS[:8], N2, M2)[0].sums()
        # a commit that carries T and bpar clears `reused`: a fresh set again, its single discount through stored tables
        _check_sums(f"new-bounds-{N2}x{M2}-fresh-D1", _aterms(L, h, XS[:1]), trb[:1])
        check_form(L, h, f"new-bounds-{N2}x{M2}-fresh-D1", {"fused": 0}, N2)
        capi.check(L.stb_groups_update_restaurants(h, orc.u32p(Tb), orc.dp(bparb)))
        for d in (0, 3, 6):
            _check_sums(f"new-bounds-{N2}x{M2}-D1", _aterms(L, h, XS[d:d + 1]), trb[d:d + 1])
            check_form(L, h, f"new-bounds-{N2}x{M2}-D1", {"fused": 1, "sparse": 1}, N2)
        _check_sums(f"new-bounds-{N2}x{M2}-D8", _aterms(L, h, XS[:8]), trb)
        check_form(L, h, f"new-bounds-{N2}x{M2}-D8", {"fused": 1, "sparse": 1}, N2)
        watch.check(("reused", N, M))
    finally:
        L.stb_groups_free(h)


# ------------------------------------------------------------------------------------------------ aterms2

S_HIST = 70000
X2 = [3 * 2.0 ** -30, 0.01, 0.37, 0.5, 0.999, 1 - 2.0 ** -20]


def _histograms():
    rng = np.random.default_rng(11)
    cnt = np.zeros(S_HIST, dtype=np.uint32)
    cnt[[2, 3, 4, 5]] = [7, 1, 123456, 3]                # the three product branches and the first lgamma one
    cnt[S_HIST - 1] = 2
    sizes = rng.choice(np.arange(6, S_HIST - 1), size=300, replace=False)
    cnt[sizes] = rng.integers(1, 100000, size=300)
    cnt[sizes[0]] = 2 ** 32 - 1                          # one count of 2^32 - 1
    cnt[0], cnt[1] = 9, 12345                            # ignored by aterms2
    return [("counts", cnt), ("all-zero", np.zeros(S_HIST, dtype=np.uint32))]


@pytest.mark.parametrize("route", ["create", "device-filled"])
def test_hist_aterms2_against_mpmath(route):
    """stb_hist_aterms2 -- the posterior stb_samplea2_hist samples from -- against hp.aterms2 under its derived bar: a
    histogram of 70000 sizes through stb_hist_create, and through stb_hist_create_empty with the counts copied to the
    device and stb_hist_restaurants; D = 1 and D = 64, the most a call accepts"""
    L = capi.lib()
    T = np.array([1, 2, 5, 40, 1000, 60000, 3], dtype=np.uint32)
    bpar = np.array([0.5, 1.0, 0.74, 2.0, 3.7, 1e-6, 500.0])
    xs = np.resize(np.array(X2), 64)
    for hname, cnt in _histograms():
        if route == "create":
            H = capi.Histogram(S_HIST, len(T), cnt=cnt, T=T, bpar=bpar)
        else:
            H = capi.Histogram(S_HIST, len(T))
            p, st = H.device_counts()
            capi.check(L.stb_memcpy_h2d(p, cnt.ctypes.data_as(C.c_void_p), cnt.nbytes, st))
            capi.check(L.stb_stream_sync(st))
            H.restaurants(T, bpar)
            assert np.array_equal(H.counts(), cnt)
        want = [hp.aterms2(x, cnt, T, bpar) for x in X2]
        got64 = np.asarray(H.aterms2(xs))
        got1 = np.array([np.asarray(H.aterms2(np.array([x])))[0] for x in X2])
        for d, x in enumerate(xs):
            tv, b = want[d % len(X2)]
            e = abs(float(hp.LD(got64[d]) - hp.LD(tv)))
            if d < len(X2):
                _note(f"aterms2-{route}-{hname}-D64", x, e / b)
                e1 = abs(float(hp.LD(got1[d]) - hp.LD(tv)))
                _note(f"aterms2-{route}-{hname}-D1", x, e1 / b)
                assert e1 <= b, (route, hname, "D1", x, got1[d], tv, e1, b)
            assert e <= b, (route, hname, "D64", d, x, got64[d], tv, e, b)
        H.free()
