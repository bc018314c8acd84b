"""The slope of log S in the discount on the device: every cell of stb_fill_dS's g slab and dS1 against the long-double truth
(tests/hd_oracle.py) under the bar derived there from the kernel's own roundings, at the shapes where k_fill_da changes
behaviour (taken from the built kernel's constants); look-ups, the restaurant terms' derivative, the gradient of aterms on
a group set and the mode it leads to."""
import ctypes as C

import numpy as np
import pytest

import hd_oracle as hd
import hp_oracle as hp
import orc
from libstb_amd import capi, synth

pytestmark = pytest.mark.gpu
LD = np.longdouble
A4 = np.array([0.0, 1.0 / 16, 0.5, 0.98])


def geometry(N=1500):
    v = [C.c_int() for _ in range(5)]
    capi.lib().stb_fill_dS_geometry(N, *[C.byref(x) for x in v])
    return [x.value for x in v]   # rows per launch, owned columns, halo columns, rows per trip, rows per period


def shapes():
    R, OW, H, U, P = geometry()
    assert R >= 8 and OW >= 8 and 2 * P < R + 1500
    out = [(4, 3), (12, 11),
           (R + 1, R + 1), (R + 2, R + 2),           # one launch exactly / a second launch of one row
           (OW + 40, OW + 1), (OW + 40, OW + 2),     # the last column of block 0 / the first of block 1
           (H + OW + 40, H + OW + 2),                # the first block whose halo holds real columns only
           (700, 100),                               # M clipped well below N; several periods a launch, several launches
           (1500, 1500)]
    return out


_truth = {}


def truth(N, M):
    if (N, M) not in _truth:
        _truth[(N, M)] = hd.tables(A4, N, M)
    return _truth[(N, M)]


def check_slab(t, d, a, N, M, tr, label):
    ds1_t, g_t = tr
    n, m = hp.cell_coords(N, M)
    got = t.packed_host(d)
    err = hp.err(got, g_t).astype(np.float64)
    bar = hd.gbar(n, a, g_t.astype(np.float64))
    ratio = float(np.max(err / np.maximum(bar, 1e-300))) if err.size else 0.0
    s1 = t.dS1[d].cpu().numpy()
    e1 = hp.err(s1, ds1_t).astype(np.float64)
    b1 = hd.ds1bar(np.arange(1, N + 1), ds1_t.astype(np.float64))
    r1 = float(np.max(e1[1:] / b1[1:])) if N > 1 else 0.0
    print(f"{label} N={N} M={M} a={a}: worst g err/bar {ratio:.3f}, worst dS1 err/bar {r1:.3f}")
    assert s1[0] == 0.0
    assert np.all(np.isfinite(got)) and ratio <= 1.0 and r1 <= 1.0, (label, N, M, a, ratio, r1)
    return got, s1


@pytest.mark.parametrize("N,M", shapes())
def test_every_cell_against_the_truth(N, M):
    """D = 4 (all discounts), each table bit-equal to its single fill and to a D = 3 batch; two runs the same bits"""
    t4 = capi.DeviceSlopeTables(N, M, 4)
    t4.fill(A4)
    got = [check_slab(t4, d, float(A4[d]), N, M, truth(N, M)[d], "D=4") for d in range(4)]
    t1 = capi.DeviceSlopeTables(N, M, 1)
    for d in range(4):
        t1.fill(A4[d:d + 1])
        assert np.array_equal(t1.packed_host(0), got[d][0]) and np.array_equal(t1.dS1[0].cpu().numpy(), got[d][1])
    t3 = capi.DeviceSlopeTables(N, M, 3)
    t3.fill(A4[1:])
    for d in range(3):
        assert np.array_equal(t3.packed_host(d), got[d + 1][0]) and np.array_equal(t3.dS1[d].cpu().numpy(), got[d + 1][1])
    t4.fill(A4)
    for d in range(4):
        assert np.array_equal(t4.packed_host(d), got[d][0])


def test_other_periods_and_rows_per_launch_hold_the_bar(monkeypatch):
    """STB_FILL_P / STB_FILL_R move the renormalisations and the launch boundaries (the only switches the kernel has; its
    workgroup size is fixed): every cell stays under the bar, and a repeated fill gives the same bits"""
    N, M = 700, 100
    t = capi.DeviceSlopeTables(N, M, 4)
    for env in ({"STB_FILL_P": "7"}, {"STB_FILL_R": "50"}, {"STB_FILL_R": "33", "STB_FILL_P": "5"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        t.fill(A4)
        got = [check_slab(t, d, float(A4[d]), N, M, truth(N, M)[d], str(env))[0] for d in range(4)]
        t.fill(A4)
        for d in range(4):
            assert np.array_equal(t.packed_host(d), got[d]), env
        for k in env:
            monkeypatch.delenv(k)


def test_log_S_slab_of_the_same_call_is_fill_pcs(monkeypatch):
    N, M = 300, 290
    t = capi.DeviceSlopeTables(N, M, 3, with_S=True)
    t.fill(A4[1:])
    s = capi.DeviceTables(N, M, 3)
    s.fill(A4[1:], variant=capi.FILL_PC)
    for d in range(3):
        assert np.array_equal(t.packed_host(d, "S"), s.packed_host(d))
        assert np.array_equal(t.S1[d].cpu().numpy(), s.S1[d].cpu().numpy())
        check_slab(t, d, float(A4[1 + d]), N, M, hd.tables(A4[1 + d:2 + d], N, M)[0], "with S")


def test_refusals_are_stb_fill_S_s():
    import torch

    L = capi.lib()
    t = capi.DeviceSlopeTables(40, 30, 2)
    a = np.array([0.5, 0.5])
    args = lambda **k: dict(dict(a=a, D=2, N=40, M=30, gs=t.stride, ds=40, ws=t.ws_bytes), **k)

    def call(a, D, N, M, gs, ds, ws):
        return L.stb_fill_dS(capi.dp(a), D, N, M, t.g.data_ptr(), gs, t.dS1.data_ptr(), ds, None, 0, None, 0, t.ws.data_ptr(), ws, None)

    assert call(**args()) == 0
    for bad, msg in ((args(gs=t.elems - 2), "strides too small"), (args(ds=39), "strides too small"), (args(gs=t.elems + 1), "even"),
                     (args(a=np.array([0.5, 1.0])), "outside [0,1)"), (args(a=np.array([-0.1, 0.5])), "outside [0,1)"),
                     (args(N=1), "too small"), (args(M=1), "too small"), (args(D=0), "D=0"), (args(ws=64), "workspace")):
        assert call(**bad) != 0 and msg in capi.last_error(), (bad, capi.last_error())
    torch.cuda.synchronize()


def test_lookup_cases():
    N, M = 60, 20
    a = 0.3
    t = capi.DeviceSlopeTables(N, M, 1)
    t.fill([a])
    n = np.array([5, 1, 7, 7, 60, 61, 61, 3, 0, 30, 30, 30, 60, 2, 25], dtype=np.uint32)
    m = np.array([5, 1, 1, 0, 1, 1, 61, 9, 0, 20, 21, 2, 20, 1, 24], dtype=np.uint32)
    got = t.lookup(n, m)
    ds1, g = hd.tables([a], N, M)[0]
    for nn, mm, v in zip(n.tolist(), m.tolist(), got.tolist()):
        if nn == mm:
            assert v == 0.0
        elif mm == 1:
            if nn <= N:
                assert v == float(t.dS1[0, nn - 1]) and abs(v - float(ds1[nn - 1])) <= hd.ds1bar(nn, float(ds1[nn - 1]))
            else:
                assert v != v
        elif mm == 0 or nn < mm or mm > M or nn > N:
            assert v != v, (nn, mm, v)
        else:
            want = float(g[hp._s_rowoff(nn, M) + mm - 2])
            assert abs(v - want) <= hd.gbar(nn, a, want), (nn, mm)


def test_restaurant_terms_da_against_mpmath():
    import torch

    L = capi.lib()
    Ts = [0, 1, 2, hd.PSI_CUT - 1, hd.PSI_CUT, hd.PSI_CUT + 1, 500, 40000]
    zs = [1e-3, 0.3, 15.9, 16.0, 700.0, 1e5]
    xs = np.array([0.05, 0.5, 0.93])
    T = np.array([t for t in Ts for _ in zs], dtype=np.uint32)
    for x in xs:
        # one restaurant a call, so that every (T, b / x) is held to its own bar; then all of them as a sum
        b = np.array([z * x for _ in Ts for z in zs])
        dT = torch.as_tensor(T.view(np.int32), device="cuda")
        db = torch.as_tensor(b, device="cuda")
        out = torch.empty(1, dtype=torch.float64, device="cuda")
        ws_bytes = int(L.stb_terms_workspace_bytes(len(T), 1))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        xa = np.array([x])
        worst = 0.0
        for i in range(len(T)):
            capi.check(L.stb_restaurant_terms_da(capi.dp(xa), 1, dT[i:].data_ptr(), db[i:].data_ptr(), 1, out.data_ptr(), ws.data_ptr(), ws_bytes, None))
            val, bar = hd.restaurant_term_da(x, int(T[i]), float(b[i]))
            err = abs(float(out.item()) - float(val))
            if bar > 0:
                worst = max(worst, err / (bar + 4 * hd.U * abs(float(val))))
            assert err <= bar + 4 * hd.U * abs(float(val)), (x, int(T[i]), float(b[i]), float(out.item()), float(val), bar)
        capi.check(L.stb_restaurant_terms_da(capi.dp(xa), 1, dT.data_ptr(), db.data_ptr(), len(T), out.data_ptr(), ws.data_ptr(), ws_bytes, None))
        val, bar = hd.restaurant_terms_da(x, T, b)
        assert abs(float(out.item()) - float(val)) <= bar
        print(f"x={x}: worst single-term err/bar {worst:.3f}")


# ---------------------------------------------------------------------------------------------------- group sets

def make_set(g, N, M, Dmax, n=None, t=None):
    L = capi.lib()
    n = g.n if n is None else n
    t = g.t if t is None else t
    h = L.stb_groups_create(g.I, orc.i32p(g.K), orc.u32p(g.T), orc.u32p(n), orc.u16p(t), orc.dp(g.bpar), N, M, Dmax)
    assert h, capi.last_error()
    return h


def aterms(h, x):
    out = np.zeros(len(x))
    capi.check(capi.lib().stb_groups_aterms(h, capi.dp(np.ascontiguousarray(x)), len(x), capi.dp(out)))
    return out


@pytest.fixture(scope="module")
def working_set():
    g = synth.groups(50, 40, n_max=600, profile="wide", seed=11, bpar=7.0)
    x = np.array([0.07, 0.2, 0.33, 0.5, 0.61, 0.75, 0.9, 0.97])
    tr = [hd.grad(float(a), g.n, g.t, g.T, g.bpar) for a in x]
    return g, x, tr


def test_aterms_grad_values_and_gradients(working_set):
    g, x, tr = working_set
    N, M = int(g.n.max()), int(g.t.max())
    h = make_set(g, N, M, 8)
    try:
        for D in (1, 3, 8):
            val, grad = capi.groups_aterms_grad(h, x[:D])
            assert np.array_equal(val, aterms(h, x[:D]))
            for d in range(D):
                want, bar = tr[d]
                print(f"D={D} a={x[d]}: grad {grad[d]:.15g} truth {want:.15g} err/bar {abs(grad[d] - want) / bar:.3f}")
                assert abs(grad[d] - want) <= bar, (D, d, grad[d], want, bar)
            v2, g2 = capi.groups_aterms_grad(h, x[:D])
            assert np.array_equal(g2, grad) and np.array_equal(v2, val)
    finally:
        capi.lib().stb_groups_free(h)


def test_aterms_grad_log0_pair_and_new_pairs(working_set):
    g, x, tr = working_set
    L = capi.lib()
    N, M = int(g.n.max()), int(g.t.max())
    nb, tb = g.n.copy(), g.t.copy()
    nb[5], tb[5] = 9, 12                                     # t > n: S_S is log 0
    h = make_set(g, N, M, 3, nb, tb)
    try:
        val, grad = capi.groups_aterms_grad(h, x[:3])
        assert np.all(np.isneginf(val)) and np.all(np.isnan(grad))
        # new pairs with new (smaller) bounds: the gradient follows them
        g2 = synth.groups(50, 40, n_max=200, profile="realistic", seed=5, bpar=7.0)
        capi.check(L.stb_groups_pairs_begin(h))
        capi.check(L.stb_groups_pairs_put(h, orc.u32p(g2.n), orc.u16p(g2.t), len(g2.n), None, None))
        capi.check(L.stb_groups_pairs_commit(h, orc.u32p(g2.T), orc.dp(g2.bpar), int(g2.n.max()), int(g2.t.max())))
        val, grad = capi.groups_aterms_grad(h, x[1:3])
        for d in range(2):
            want, bar = hd.grad(float(x[1 + d]), g2.n, g2.t, g2.T, g2.bpar)
            assert abs(grad[d] - want) <= bar, (d, grad[d], want, bar)
        assert np.array_equal(val, aterms(h, x[1:3]))
    finally:
        L.stb_groups_free(h)


def test_aterms_grad_refusals(working_set):
    g, x, tr = working_set
    L = capi.lib()
    val, grad = np.full(8, 123.0), np.full(8, 456.0)
    call = lambda h, xx, D: L.stb_groups_aterms_grad(h, capi.dp(xx), D, capi.dp(val), capi.dp(grad))
    h = make_set(g, 600, 600, 3)
    e = L.stb_groups_create(g.I, orc.i32p(g.K), None, None, None, None, 0, 0, 3)   # an empty set
    assert e, capi.last_error()
    try:
        assert call(h, x[:4].copy(), 4) != 0 and "outside 1..3" in capi.last_error()
        assert call(h, np.array([0.5, 1.0]), 2) != 0 and call(h, np.array([0.0]), 1) != 0
        assert call(None, x[:1].copy(), 1) != 0
        assert call(e, x[:1].copy(), 1) != 0 and "no pairs" in capi.last_error()
        assert np.all(val == 123.0) and np.all(grad == 456.0)
    finally:
        L.stb_groups_free(h)
        L.stb_groups_free(e)


@pytest.fixture(scope="module")
def mode_set():
    g = synth.groups(12, 10, n_max=150, profile="realistic", seed=21, bpar=5.0)
    fn = lambda xs: hd.grad_many(xs, g.n, g.t, g.T, g.bpar)
    root = hd.bisect_root(fn, 0.02, 0.95, 1e-12)
    return g, fn, root


@pytest.mark.parametrize("Dmax", [8, 3])
def test_modea_finds_the_truths_root(mode_set, Dmax):
    g, fn, root = mode_set
    tol = 1e-7
    h = make_set(g, int(g.n.max()), int(g.t.max()), Dmax)
    try:
        a_hat, curv, info = capi.groups_modea(h, 0.02, 0.95, tol, 40)
        rep = hd.modea_replay(fn, 0.02, 0.95, tol, 40, Dmax)
        print(f"Dmax={Dmax}: a_hat {a_hat:.12f} root {root:.12f} replay {rep['a_hat']:.12f} rounds {info.rounds} evals {info.evals} curv {curv:.6g}")
        assert abs(a_hat - root) <= tol and abs(rep["a_hat"] - root) <= tol
        assert info.at_bound == 0 and info.lo <= a_hat <= info.hi and info.hi - info.lo <= tol
        assert info.g_lo > 0 >= info.g_hi
        assert info.rounds == rep["rounds"] and info.evals == rep["evals"] == info.rounds * min(Dmax, 8) + 3
        # the gradients the device reports are the truth's within their bars
        pts = np.array([info.lo, info.hi, a_hat, a_hat - info.delta, a_hat + info.delta])
        tr = [hd.grad(float(p), g.n, g.t, g.T, g.bpar) for p in pts]
        for got, (want, bar) in zip((info.g_lo, info.g_hi, info.grad), tr[:3]):
            assert abs(got - want) <= bar
        # curvature: the truth's difference quotient at the same points; each gradient is off by at most its bar, the
        # subtraction and the division round once each
        want = (tr[4][0] - tr[3][0]) / (2 * info.delta)
        bound = (tr[3][1] + tr[4][1]) / (2 * info.delta) + 4 * hd.U * abs(want)
        assert curv < 0 and abs(curv - want) <= bound, (curv, want, bound)
        again = capi.groups_modea(h, 0.02, 0.95, tol, 40)
        assert again[0] == a_hat and again[1] == curv and again[2].evals == info.evals and again[2].grad == info.grad
    finally:
        capi.lib().stb_groups_free(h)


def test_modea_bounds_and_refusals(mode_set):
    g, fn, root = mode_set
    L = capi.lib()
    h = make_set(g, int(g.n.max()), int(g.t.max()), 8)
    h2 = make_set(g, int(g.n.max()), int(g.t.max()), 2)
    e = L.stb_groups_create(g.I, orc.i32p(g.K), None, None, None, None, 0, 0, 8)
    try:
        a_hat, curv, info = capi.groups_modea(h, root + 0.05, 0.9, 1e-6, 40)
        assert info.at_bound == -1 and a_hat == root + 0.05 and info.rounds == 1 and info.g_lo <= 0 and info.lo == info.hi == a_hat
        a_hat, curv, info = capi.groups_modea(h, 0.05, root - 0.05, 1e-6, 40)
        assert info.at_bound == 1 and a_hat == root - 0.05 and info.rounds == 1 and info.g_hi >= 0
        ah, cv, inf = C.c_double(-7.0), C.c_double(-8.0), capi.ModeaInfo()
        inf.rounds = -9
        call = lambda hh, lo, hi, tol=1e-6, r=40: L.stb_groups_modea(hh, lo, hi, tol, r, C.byref(ah), C.byref(cv), C.byref(inf))
        for bad in ((h, 0.0, 0.5), (h, 0.5, 0.5), (h, 0.6, 0.5), (h, 0.5, 1.0), (h, float("nan"), 0.5)):
            assert call(*bad) != 0 and "interval" in capi.last_error()
        assert call(h, 0.1, 0.9, 0.0) != 0 and call(h, 0.1, 0.9, 1e-6, 0) != 0
        assert call(e, 0.1, 0.9) != 0 and "no pairs" in capi.last_error()
        assert call(h2, 0.1, 0.9) != 0 and "Dmax" in capi.last_error()
        assert call(None, 0.1, 0.9) != 0
        assert ah.value == -7.0 and cv.value == -8.0 and inf.rounds == -9
    finally:
        for s in (h, h2, e):
            L.stb_groups_free(s)
