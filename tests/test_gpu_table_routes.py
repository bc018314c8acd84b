"""S_FLOAT and V tables of the table interface across changes of fill route (stable_host.c provision / build).

A float table is filled one of two ways, chosen again at every fill: directly as floats by the halo-block kernel
(stb_fill_Sf / stb_fill_Vf, no double slab), or into a double slab that stb_table_to_float narrows (stb_fill_S /
stb_fill_V).  Which one applies depends on the bounds (stb_fill_takes_kind: 512 rows or more), on the shared-GPU mode
(stb_set_shared_gpu, or two slow launches) and on STB_FLOAT_NARROW, and all three change while a table lives.  Each
history below makes a float table, switches routes under it, remakes or grows it, and compares every row with the CPU
oracle after each step; a double S_STABLE|S_UVTABLE table goes through the same steps as the control.

Metrics: log S within one float ulp of the oracle narrowed (and 99 % identical), S1 within 1e-10, V within 2^-23, U and
UV within 2^-23 of the double control; the double control itself within 1e-10 of the oracle."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import orc
from libstb_amd import capi

pytestmark = pytest.mark.gpu

NB = 1500        # bounds where both direct fills (kinds 1 and 3) apply: asserted by every history, not assumed
SMALL = 300      # below STB_HB_MIN_N = 512: made on the narrow route
F32 = 2.0 ** -23
CONTROL = capi.S_STABLE | capi.S_UVTABLE
FLAGS = {
    "S": capi.S_STABLE | capi.S_FLOAT,
    "V": capi.S_UVTABLE | capi.S_FLOAT,
    "SV": capi.S_STABLE | capi.S_UVTABLE | capi.S_FLOAT,
    "double": CONTROL,
}


@pytest.fixture(autouse=True)
def automatic_mode(monkeypatch):
    """the shared-GPU mode is process-wide: every test starts and ends on the automatic rule, direct routes allowed"""
    monkeypatch.delenv("STB_FLOAT_NARROW", raising=False)
    L = capi.lib()
    L.stb_set_shared_gpu(-1)
    try:
        yield L
    finally:
        L.stb_set_shared_gpu(-1)


@lru_cache(maxsize=None)
def oracle(a, N, M):
    S1, tab = orc.fill_S(a, N, M)
    return S1, tab, orc.fill_V(a, N, M)


def s_offsets(n, M):
    n = n.astype(np.int64)
    k = n - 3
    return np.where(n <= M + 1, k * (k + 1) // 2, (M - 1) * M // 2 + (n - M - 2) * (M - 1))


@lru_cache(maxsize=None)
def cells(which, N, M, full=True):
    """(n, m) to look at in a table of bounds (N, M): every row at columns 2, the middle and the last one below the
    bound, plus four complete rows (full).  which 0: log S, rows 3..N, m <= min(n-1, M); which 1: V, rows 2..N-2,
    m <= min(n, M-2) -- S_V grows the table from row usedN-1 / column usedM-1 on (lib/stable.c:903)"""
    if which == 0:
        lo, hi, last = 3, N, lambda r: min(r - 1, M)
    else:
        lo, hi, last = 2, N - 2, lambda r: min(r, M - 2)
    got = set()
    for n in range(lo, hi + 1):
        e = last(n)
        got.update((n, m) for m in (2, (2 + e) // 2, e) if 2 <= m <= e)
    if full:
        for n in {hi, (hi + 3) // 2, min(M + 1, hi), 513}:
            if lo <= n <= hi:
                got.update((n, m) for m in range(2, last(n) + 1))
    n, m = np.array(sorted(got), dtype=np.uint32).T
    return np.ascontiguousarray(n), np.ascontiguousarray(m)


@lru_cache(maxsize=None)
def v_offsets(N, M):
    O = orc.oracle()
    return np.array([O.orc_vrow_offset(r, M) if r >= 2 else 0 for r in range(N + 1)], dtype=np.int64)


def probe(t, which, n, m):
    out = np.empty(n.shape[0])
    up = C.POINTER(C.c_uint)
    capi.lib().stb_table_probe(t.sp, which, n.ctypes.data_as(up), m.ctypes.data_as(up), n.shape[0], capi.dp(out))
    return out


def assert_float_close(got, want, what):
    """got: what the float table returned; want: the double it should hold, narrowed"""
    w32 = want.astype(np.float32)
    assert np.all(got == got.astype(np.float32).astype(np.float64)), f"{what}: not stored as float"
    bad = np.abs(got - w32) > np.spacing(np.abs(w32))
    assert not bad.any(), f"{what}: {bad.sum()} cells off by more than one float ulp, first {np.flatnonzero(bad)[:5]}"
    same = np.mean(got == w32)
    assert same >= 0.99, f"{what}: only {same:.4f} identical"


def assert_rel(got, want, rel, what):
    err = np.abs(got - want) / np.abs(want)
    assert np.all(err <= rel), f"{what}: relative error {err.max():.3e} > {rel:.3e} at {np.argmax(err)}"


def assert_close(got, want, what):
    """the parity metric of the double tables: |x - y| <= 1e-10 max(1, |y|)"""
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    assert np.all(err <= 1e-10), f"{what}: error {err.max():.3e} > 1e-10 at {np.argmax(err)}"


def route(L, N):
    return L.stb_fill_takes_kind(N, N, 1, 1), L.stb_fill_takes_kind(N, N, 1, 3)


class Subject:
    """a table with the flags under test and its double control, put through the same steps"""

    def __init__(self, flags, initN, a):
        self.L = capi.lib()
        self.flags = flags
        self.t = capi.Table(initN, initN, NB, NB, a, flags)
        self.ctrl = self.t if flags == CONTROL else capi.Table(initN, initN, NB, NB, a, CONTROL)
        self.a = a

    def tables(self):
        return (self.t,) if self.ctrl is self.t else (self.t, self.ctrl)

    def remake(self, a):
        for x in self.tables():
            rc = x.remake(a)
            assert rc == 0, f"S_remake({a}) failed: {capi.last_error()}"
        self.a = a

    def grow(self, n, m):
        """through an accessor, as a sampler grows its table (S_S, or S_V where there is no S table)"""
        acc = "S" if self.flags & capi.S_STABLE else "V"
        for x in self.tables():
            getattr(x, acc)(n, m)
        assert (self.t.usedN, self.t.usedM) == (self.ctrl.usedN, self.ctrl.usedM)

    def check(self, slab=False):
        t, ctrl, a, flags = self.t, self.ctrl, self.a, self.flags
        N, M = t.usedN, t.usedM
        S1o, So, Vo = oracle(a, N, M)
        fl = bool(flags & capi.S_FLOAT)
        assert_close(np.array([t.S1(n) for n in range(1, N + 1)]), S1o, "S1")
        if flags & capi.S_STABLE:
            n, m = cells(0, N, M)
            got, want = probe(t, 0, n, m), So[s_offsets(n, M) + m - 2]
            if fl:
                assert_float_close(got, want, "S")
            else:
                assert_close(got, want, "S")
        if flags & capi.S_UVTABLE:
            n, m = cells(1, N, M)
            got, want = probe(t, 1, n, m), Vo[v_offsets(N, M)[n] + m - 2]
            if fl:
                assert np.all(got == got.astype(np.float32).astype(np.float64)), "V: not stored as float"
                assert_rel(got, want, F32, "V")
            else:
                assert_close(got, want, "V")
            n, m = cells(1, N, M, False)
            k = m < n  # (S_UV answers m = n and m = n + 1 in closed form)
            n, m = n[k].astype(np.int64), m[k].astype(np.int64)
            want = Vo[v_offsets(N, M)[n] + m - 2]
            gu = np.array([t.U(int(r), int(c)) for r, c in zip(n, m)])
            guv = np.array([t.UV(int(r), int(c)) for r, c in zip(n, m)])
            if ctrl is t:
                c = n - m * a
                assert_close(gu, c + 1.0 / want, "U")
                assert_close(guv, c * want + 1.0, "UV")
            else:
                assert (ctrl.usedN, ctrl.usedM) == (N, M)
                assert_rel(gu, np.array([ctrl.U(int(r), int(c)) for r, c in zip(n, m)]), F32, "U")
                assert_rel(guv, np.array([ctrl.UV(int(r), int(c)) for r, c in zip(n, m)]), F32, "UV")
        if slab:
            assert self.has_double_slab(), "no double slab for the bounds after a fill on the double route"

    def has_double_slab(self):
        """the table holds on the device what the double route needs at its current bounds, double slab included (a
        float table on the direct route holds less: its double slab is missing, or sized for smaller bounds)"""
        L, N, M = self.L, self.t.usedN, self.t.usedM
        fb = 4 if self.flags & capi.S_FLOAT else 0
        need = int(L.stb_fill_workspace_bytes(N, M, 1)) + 8 * N
        if self.flags & capi.S_STABLE:
            need += (8 + fb) * max(2, int(L.stb_elems(N, M)))
        if self.flags & capi.S_UVTABLE:
            need += (8 + fb) * max(2, int(L.stb_velems(N, M)))
            if not self.flags & capi.S_STABLE:
                need += 8 * (int(L.stb_elems(N, 2)) + 2)  # (the scratch of the S1-only fill)
        dv, hs = C.c_ulonglong(), C.c_ulonglong()
        L.stb_table_bytes(self.t.sp, C.byref(dv), C.byref(hs))
        return dv.value >= need

    def free(self):
        for x in self.tables():
            x.free()


@pytest.fixture(params=list(FLAGS), ids=list(FLAGS))
def flags(request):
    return FLAGS[request.param]


@pytest.fixture
def subjects():
    made = []
    yield made
    for s in made:
        s.free()


def make(subjects, flags, initN, a):
    subjects.append(Subject(flags, initN, a))
    return subjects[-1]


def shared(L, mode):
    L.stb_set_shared_gpu(mode)
    assert L.stb_shared_gpu_mode() == (1 if mode == 1 else 0)


def test_bounds_take_the_direct_routes(automatic_mode):
    """the histories' premise: at NB both float fills go direct, and shared mode sends both to the double slab"""
    L = automatic_mode
    assert route(L, NB) == (1, 1)
    assert route(L, SMALL) == (0, 0)
    shared(L, 1)
    assert route(L, NB) == (0, 0)


def test_made_direct_then_shared(flags, subjects, automatic_mode):
    """made on the direct route (no double slab), remade in shared mode, remade back on the direct route"""
    L = automatic_mode
    assert route(L, NB) == (1, 1)
    s = make(subjects, flags, NB, 0.5)
    s.check()
    assert s.has_double_slab() == (flags == CONTROL)
    shared(L, 1)
    s.remake(0.05)
    s.check(slab=True)
    shared(L, -1)
    assert route(L, NB) == (1, 1)
    s.remake(0.95)
    s.check()


def test_made_shared_then_direct(flags, subjects, automatic_mode):
    L = automatic_mode
    shared(L, 1)
    s = make(subjects, flags, NB, 0.5)
    s.check(slab=True)
    shared(L, -1)
    assert route(L, NB) == (1, 1)
    s.remake(0.05)
    s.check()
    s.remake(0.95)
    s.check()


def test_grown_past_512_then_shared(flags, subjects, automatic_mode):
    """made below 512 rows (a double slab for those bounds), grown onto the direct route (the slab stays small), then
    remade in shared mode: the double fill needs a slab for the grown bounds"""
    L = automatic_mode
    s = make(subjects, flags, SMALL, 0.5)
    s.check(slab=True)
    s.grow(1400, 700)
    N, M = s.t.usedN, s.t.usedM
    assert N >= 512 and (L.stb_fill_takes_kind(N, M, 1, 1), L.stb_fill_takes_kind(N, M, 1, 3)) == (1, 1), (N, M)
    s.check()
    assert s.has_double_slab() == (flags == CONTROL)  # (the float table's double slab: still the 300-row one)
    shared(L, 1)
    s.remake(0.05)
    s.check(slab=True)
    shared(L, -1)
    s.remake(0.95)
    s.check()


def test_grown_while_shared_then_remade(flags, subjects, automatic_mode):
    L = automatic_mode
    s = make(subjects, flags, SMALL, 0.5)
    shared(L, 1)
    s.grow(1400, 700)
    assert s.t.usedN >= 512
    s.check(slab=True)
    shared(L, -1)
    s.remake(0.05)
    s.check()
    shared(L, 1)
    s.remake(0.95)
    s.check(slab=True)


def test_shared_by_the_automatic_rule(flags, subjects, automatic_mode):
    """two launches reported 500 x slower than expected switch the mode: the next remake takes the double route"""
    L = automatic_mode
    s = make(subjects, flags, NB, 0.5)
    s.check()
    assert s.has_double_slab() == (flags == CONTROL)
    L.stb_note_launch_span(725.0, 1.4)
    L.stb_note_launch_span(725.0, 1.4)
    assert L.stb_shared_gpu_mode() == 1 and route(L, NB) == (0, 0)
    s.remake(0.05)
    s.check(slab=True)
    shared(L, -1)
    s.remake(0.95)
    s.check()


def test_float_narrow_against_direct(flags, subjects, automatic_mode, monkeypatch):
    """STB_FLOAT_NARROW=1 (the double slab, narrowed) against the direct route at the same discount, the narrow table
    switching routes with the variable"""
    L = automatic_mode
    assert route(L, NB) == (1, 1)
    monkeypatch.setenv("STB_FLOAT_NARROW", "1")
    nar = make(subjects, flags, NB, 0.5)
    monkeypatch.delenv("STB_FLOAT_NARROW")
    dire = make(subjects, flags, NB, 0.5)
    assert dire.has_double_slab() == (flags == CONTROL)
    for a, narrow in ((0.5, True), (0.05, False), (0.95, True)):
        if a != 0.5:
            if narrow:
                monkeypatch.setenv("STB_FLOAT_NARROW", "1")
            nar.remake(a)
            monkeypatch.delenv("STB_FLOAT_NARROW", raising=False)
            dire.remake(a)
        nar.check(slab=narrow)
        dire.check()
        if flags & capi.S_STABLE:
            n, m = cells(0, NB, NB)
            x, y = probe(nar.t, 0, n, m), probe(dire.t, 0, n, m)
            if flags & capi.S_FLOAT:
                assert_float_close(x, y, "S narrow vs direct")
            else:
                assert_close(x, y, "S narrow vs direct")
        if flags & capi.S_UVTABLE:
            n, m = cells(1, NB, NB)
            x, y = probe(nar.t, 1, n, m), probe(dire.t, 1, n, m)
            if flags & capi.S_FLOAT:
                assert_rel(x, y, F32, "V narrow vs direct")
            else:
                assert_close(x, y, "V narrow vs direct")


@pytest.mark.parametrize("N", [SMALL, NB])
def test_one_table_fill_refuses_short_strides(N, automatic_mode):
    """D = 1 fills check the slab size they are given (table_stride) and S1's (s1_stride) before anything is queued.
    The buffers are full size, so an unchecked fill would write into memory of its own; they are NaN beforehand and
    must stay so.  The exact sizes are then accepted, odd or not, and fill the table."""
    L = automatic_mode
    torch = capi._torch()
    M = N
    el, vel = int(L.stb_elems(N, M)), int(L.stb_velems(N, M))
    wsb = int(L.stb_fill_workspace_bytes(N, M, 1))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    a = np.array([0.5])
    st = capi.stream_ptr()
    S1o, So, Vo = oracle(0.5, N, M)
    direct = route(L, N) == (1, 1)
    assert direct == (N >= 512)
    for name, dt, need, with_s1, floats in (("stb_fill_S", torch.float64, el, True, False),
                                            ("stb_fill_Sf", torch.float32, el, True, True),
                                            ("stb_fill_V", torch.float64, vel, False, False),
                                            ("stb_fill_Vf", torch.float32, vel, False, True)):
        f = getattr(L, name)
        slab = torch.full((need,), float("nan"), dtype=dt, device="cuda")
        S1 = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")

        def call(ts, s1s):
            if with_s1:
                args = [capi.dp(a), 1, N, M, slab.data_ptr(), ts, S1.data_ptr(), s1s, ws.data_ptr(), wsb]
                return f(*(args + [capi.FILL_SCALED, st] if name == "stb_fill_S" else args + [st]))
            return f(capi.dp(a), 1, N, M, slab.data_ptr(), ts, ws.data_ptr(), wsb, st)

        for ts, s1s in ((need - 2, N),) + (((need, N - 1), (need - 2, N - 1)) if with_s1 else ()):
            assert call(ts, s1s) != 0, (name, ts, s1s)
            assert "strides too small" in capi.last_error(), (name, capi.last_error())
        torch.cuda.synchronize()
        assert bool(torch.isnan(slab).all()) and bool(torch.isnan(S1).all()), name
        if floats and not direct:
            continue  # (no kernel stores floats at these bounds: the table interface narrows a double slab)
        capi.check(call(need, N))
        capi.check(L.stb_fill_status())
        torch.cuda.synchronize()
        h = slab.double().cpu().numpy()
        if with_s1:
            assert orc.close(S1.cpu().numpy(), S1o)
            rows = np.array([3, N // 2, N], dtype=np.uint32)
            for r in rows:
                o = int(L.stb_rowoff(int(r), M))
                got, want = h[o:o + r - 2], So[orc.row_offset(int(r), M):orc.row_offset(int(r), M) + r - 2]
                if floats:
                    assert_float_close(got, want, f"{name} row {r}")
                else:
                    assert_close(got, want, f"{name} row {r}")
        else:
            for r in (2, N // 2, N):
                o, ov = int(L.stb_vrowoff(r, M)), int(orc.oracle().orc_vrow_offset(r, M))
                got, want = h[o:o + r - 1], Vo[ov:ov + r - 1]
                if floats:
                    assert_rel(got, want, F32, f"{name} row {r}")
                else:
                    assert_close(got, want, f"{name} row {r}")
