"""The draws of samplea / sampleb and of their device-resident variants, accounted for end to end without an observed number
(tests/hs_replay.py):
  (A) every value of the run's trace is within the derived bar of the long-double / mpmath truth at the abscissa the device
      was actually asked for, and
  (B) the library's own arms_simple, from the same libc streams and handed exactly those values, visits exactly those
      abscissae and returns exactly that draw and code.
With both, the draw is ARMS on a posterior that is right to the bar at every point visited.  This reaches what only the
samplers drive: bounds rounded to multiples of 128 (STB_SAMPLEA_QUANT) with M clipped to N, the three starting abscissae
evaluated in one batched call and served by bitwise equality of x, the single-abscissa fused evaluation at abscissae ARMS
chose, the speculative evaluation on a kept set (STB_SAMPLEA_CACHE=1), the borrowed-T bterms context with Q drawn on the
device, and the trace itself.  Small sets only: the kernels at working shapes are tests/test_gpu_hp_shapes.py's job."""
import ctypes as C

import numpy as np
import pytest

import hs_replay as hr
import orc
from libstb_amd import capi, synth

pytestmark = pytest.mark.gpu

A_STARTS = [0.01, 0.0100001, 0.15, 0.21, 0.5, 0.78, 0.9, 0.9799999, 0.98]
A_PARS = [0.05, 0.5, 0.93]
B_STARTS = [0.01, 10.0, 2000.0]
SEEDS = (777, 12345)


# ---- the sets

def cut(g, keep, edit=None):
    """the pairs of g under the mask `keep`, restaurant by restaurant (edit(n, t) may change them in place); T and N anew"""
    rest = np.repeat(np.arange(g.I), g.K)[keep]
    n, t = g.n[keep].copy(), g.t[keep].copy()
    if edit:
        edit(n, t)
    K = np.bincount(rest, minlength=g.I).astype(np.int32)
    assert K.min() >= 1 and np.all(t <= n)
    T = np.bincount(rest, weights=t, minlength=g.I).astype(np.uint32)
    N = np.bincount(rest, weights=n, minlength=g.I).astype(np.uint32)
    return synth.Groups(I=g.I, K=K, n=n, t=t, T=T, N=N, bpar=g.bpar.copy())


def _top(value):
    def edit(n, t):
        n[int(np.argmax(n))] = value
    return edit


def _few_tables(n, t):
    np.minimum(t, 8, out=t)


def _edges(n, t):
    n[0], t[0] = 0, 0
    n[1], t[1] = 1, 1
    n[2], t[2] = 1, 1
    t[3], t[4] = n[3], n[4]
    n[5], t[5] = 2, 2
    n[6], t[6] = 2, 1
    n[-1], t[-1] = 0, 0
    t[-2] = n[-2]


_sets = {}


def the_set(name):
    if name not in _sets:
        w = synth.groups(20, 30, 300, "wide")
        if name == "small_wide":
            s = w
        elif name == "small_real":
            s = synth.groups(20, 30, 300, "realistic")
        elif name == "mid_wide":
            s = synth.groups(100, 100, 1000, "wide")
        elif name == "top128":     # max n + 1 == 128 exactly
            s = cut(w, w.n <= 127, _top(127))
            assert int(s.n.max()) + 1 == 128
        elif name == "top129":     # max n + 1 == 129: the bounds round up to 256
            s = cut(w, w.n <= 128, _top(128))
            assert int(s.n.max()) + 1 == 129
        elif name == "few_tables":  # M clamped to 10, rounded to 128 and clipped to N
            s = cut(w, w.n <= 126, _few_tables)
            assert int(s.t.max()) <= 8 and int(s.n.max()) < 128
        elif name == "edges":      # pairs with n <= 1 and pairs with t == n
            s = cut(w, np.arange(w.pairs) % 3 == 0, _edges)
            assert np.any(s.n == 0) and np.any(s.n == 1) and np.count_nonzero((s.t == s.n) & (s.n > 1)) >= 4
        else:
            raise KeyError(name)
        _sets[name] = s
    return _sets[name]


ALL_SETS = ["small_wide", "small_real", "mid_wide", "top128", "top129", "few_tables", "edges"]


def ragged(g):
    NP = C.POINTER(C.c_uint32) * g.I
    TP = C.POINTER(C.c_uint16) * g.I
    n, t = NP(), TP()
    off = 0
    for i in range(g.I):
        n[i] = C.cast(g.n.ctypes.data + 4 * off, C.POINTER(C.c_uint32))
        t[i] = C.cast(g.t.ctypes.data + 2 * off, C.POINTER(C.c_uint16))
        off += int(g.K[i])
    return n, t


def dev_u32(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32), device="cuda")


# ---- the check

def check_run(what, draw, init, truth_of, beta=None):
    """the sampler call just made: its trace and draw against (A) and (B).  init = [lower, start, upper] of the Python
    bracket; truth_of(xs) -> [(truth, bar)]; beta: see hr.replay_arms"""
    L = capi.lib()
    count = L.stb_sampler_trace_count()
    assert 0 < count < hr.TRACE_CAP, (what, count)     # (a trace that reached the cap has lost values)
    xs, ys, code = capi.sampler_trace()
    assert len(xs) == count and np.all(np.isfinite(ys)) and draw == draw, (what, draw, ys)
    truth = truth_of(xs)
    e, bar = hr.errs(ys, truth)
    ratio = e / bar
    worst = int(np.argmax(ratio))
    three = float(np.max(ratio[:3]))
    later = float(np.max(ratio[3:])) if count > 3 else 0.0
    rep = hr.replay_arms(init[0], init[1], init[2], ys, seeds=SEEDS, beta=beta)
    diff = hr.replay_differences(xs, code, draw, rep)
    print(f"replay {what}: {count} evaluations, code {code}, worst err/bar {ratio[worst]:.3g} (the starting three "
          f"{three:.3g}, later ones {later:.3g}); replay {'bit-equal' if not diff else 'DIFFERS: ' + '; '.join(diff)}")
    assert np.all(e <= bar), (what, "A", worst, float(xs[worst]), float(ys[worst]), float(truth[worst][0]), float(e[worst]),
                              float(bar[worst]))
    assert diff == [], (what, "B", diff)
    assert init[0] <= draw <= init[2]
    return xs, ys


@pytest.fixture(autouse=True)
def clean(monkeypatch):
    """ARMS (STB_SAMPLER at its default), the library's own switches unset, nothing kept from another test"""
    for v in ("STB_SAMPLER", "STB_SAMPLEA_CACHE", "STB_SAMPLEA_QUANT"):
        monkeypatch.delenv(v, raising=False)
    capi.lib().stb_sampler_cache_clear()
    yield
    capi.lib().stb_sampler_cache_clear()


# ---- samplea

def a_truth(s, T=None, bpar=None, t=None):
    return lambda xs: hr.aterms_truth(s.K, s.n, s.t if t is None else t, s.T if T is None else T,
                                      s.bpar if bpar is None else bpar, xs)


def call_samplea(s, a_in, T=None, bpar=None, getval=None, nt=None):
    L = capi.lib()
    n, t = nt or ragged(s)
    T = s.T if T is None else T
    bpar = s.bpar if bpar is None else bpar
    orc.seed_libc(*SEEDS)
    if getval is not None:
        return L.samplea(a_in, s.I, orc.i32p(s.K), orc.u32p(T), None, None, getval, orc.dp(bpar), None, 1, 0)
    return L.samplea(a_in, s.I, orc.i32p(s.K), orc.u32p(T), n, t, None, orc.dp(bpar), None, 1, 0)


@pytest.mark.parametrize("name,a_in", [(s, 0.5) for s in ALL_SETS] + [("small_wide", a) for a in A_STARTS if a != 0.5])
def test_samplea(name, a_in):
    s = the_set(name)
    got = call_samplea(s, a_in)
    check_run(f"samplea {name} a_in={a_in!r}", got, hr.a_bracket(a_in), a_truth(s))


@pytest.mark.parametrize("name", ["top128", "top129"])
def test_samplea_on_the_references_exact_bounds(monkeypatch, name):
    monkeypatch.setenv("STB_SAMPLEA_QUANT", "1")
    s = the_set(name)
    got = call_samplea(s, 0.5)
    check_run(f"samplea {name} QUANT=1", got, hr.a_bracket(0.5), a_truth(s))


def test_samplea_getval_form():
    s = the_set("small_wide")
    offs = np.concatenate([[0], np.cumsum(s.K)])

    @capi.GETVAL
    def getval(pn, pt, i, k):
        pn[0] = int(s.n[offs[i] + k])
        pt[0] = int(s.t[offs[i] + k])

    got = call_samplea(s, 0.5, getval=getval)
    check_run("samplea small_wide getval", got, hr.a_bracket(0.5), a_truth(s))


@pytest.mark.parametrize("name", ["small_wide", "top129"])
def test_samplea_on_a_kept_set(monkeypatch, name):
    """STB_SAMPLEA_CACHE=1, unchanged pairs with changed bpar and T: the second call's three starting values come from the
    evaluation queued ahead of the fingerprint, its later ones sum inside the table walk.  Then one count changed with all
    shapes the same: the values queued on the guess must be thrown away."""
    monkeypatch.setenv("STB_SAMPLEA_CACHE", "1")
    s = the_set(name)
    nt = ragged(s)
    got = call_samplea(s, 0.5, nt=nt)
    check_run(f"samplea {name} CACHE=1 first call", got, hr.a_bracket(0.5), a_truth(s))
    bpar2 = np.linspace(0.5, 30.0, s.I)
    T2 = (s.T + np.arange(s.I, dtype=np.uint32) % 3).astype(np.uint32)
    got = call_samplea(s, 0.3, T=T2, bpar=bpar2, nt=nt)
    check_run(f"samplea {name} CACHE=1 second call", got, hr.a_bracket(0.3), a_truth(s, T=T2, bpar=bpar2))
    s3 = synth.Groups(I=s.I, K=s.K, n=s.n.copy(), t=s.t.copy(), T=s.T, N=s.N, bpar=s.bpar)
    s3.n[int(np.argmin(np.where(s3.n > 1, s3.n, 1 << 30)))] += 1       # (the bounds stay: only the fingerprint can tell)
    got = call_samplea(s3, 0.5)
    check_run(f"samplea {name} CACHE=1 after a fingerprint miss", got, hr.a_bracket(0.5), a_truth(s3))


# ---- stb_groups_samplea

@pytest.mark.parametrize("Dmax", [3, 8])
def test_groups_samplea_on_host_pairs(Dmax):
    L = capi.lib()
    s = the_set("small_wide")
    N, M = hr.reference_bounds(s.n, s.t)
    h = L.stb_groups_create(s.I, orc.i32p(s.K), orc.u32p(s.T), orc.u32p(s.n), orc.u16p(s.t), orc.dp(s.bpar), N, M, Dmax)
    assert h, capi.last_error()
    try:
        for a_in in (0.5, 0.98):
            orc.seed_libc(*SEEDS)
            got = capi.groups_samplea(h, a_in)
            check_run(f"stb_groups_samplea Dmax={Dmax} a_in={a_in!r}", got, hr.a_bracket(a_in), a_truth(s))
    finally:
        L.stb_groups_free(h)


def test_groups_samplea_on_a_set_the_device_filled():
    L = capi.lib()
    s = the_set("small_real")
    a = 0.4
    tc = capi.TableCounts(s.K, s.n, s.t)
    h = L.stb_groups_create(s.I, orc.i32p(s.K), None, None, None, None, 0, 0, 3)
    assert h, capi.last_error()
    try:
        tc.sweep(a, s.bpar, 55, 0, 1)
        tc.to_groups(h, s.bpar)
        orc.seed_libc(*SEEDS)
        got = capi.groups_samplea(h, a)
        t_now, T_now = tc.get()
        assert not np.array_equal(t_now, s.t)
        check_run("stb_groups_samplea after stb_tcounts_to_groups", got, hr.a_bracket(a), a_truth(s, T=T_now, t=t_now))
    finally:
        tc.free()
        L.stb_groups_free(h)


# ---- sampleb and the device b step

B_CASES = [(a, b) for a in A_PARS for b in B_STARTS]


def b_truth(s, Q, apar, T=None):
    return lambda xs: hr.bterms_truth(xs, Q, s.shape, s.T if T is None else T, apar)


@pytest.mark.parametrize("name,apar,b_in", [(s, a, b) for s in ("small_wide", "small_real") for a, b in B_CASES]
                         + [("mid_wide", 0.5, 10.0), ("mid_wide", 0.93, 2000.0)])
def test_sampleb_with_host_counts(name, apar, b_in):
    L = capi.lib()
    s = the_set(name)
    orc.seed_libc(*SEEDS)
    Q = hr.beta_Q(b_in, s.scale, s.N)
    orc.seed_libc(*SEEDS)
    got = L.sampleb(b_in, s.I, s.shape, s.scale, orc.u32p(s.N), orc.u32p(s.T), apar, None, 1, 0)
    check_run(f"sampleb {name} a={apar!r} b_in={b_in!r}", got, hr.b_bracket(b_in), b_truth(s, Q, apar),
              beta=(b_in, s.scale, s.N))


@pytest.mark.parametrize("apar,b_in", B_CASES)
def test_sampleb_device(apar, b_in):
    """Q drawn on the device (stb_sampleb_last_Q), T borrowed where it lives; only rand() is read on the host (ARMS): the
    replay draws no Beta variate"""
    L = capi.lib()
    s = the_set("small_wide")
    dN, dT = dev_u32(s.N), dev_u32(s.T)
    orc.seed_libc(*SEEDS)
    got = capi.sampleb_device(b_in, s.shape, s.scale, dN, dT, apar, seed=4, sweep=1)
    Q = L.stb_sampleb_last_Q()
    assert Q > 1.0 / s.scale
    check_run(f"stb_sampleb_device a={apar!r} b_in={b_in!r}", got, hr.b_bracket(b_in), b_truth(s, Q, apar))


@pytest.mark.parametrize("kind", ["tcounts", "tindic"])
@pytest.mark.parametrize("apar,b_in", B_CASES)
def test_sampleb_on_the_objects(kind, apar, b_in):
    L = capi.lib()
    s = the_set("small_real")
    obj = capi.TableCounts(s.K, s.n, s.t) if kind == "tcounts" else capi.TableIndicators(s.K, s.n, s.t)
    try:
        obj.sweep(apar, s.bpar, 77, 0, 1)
        orc.seed_libc(*SEEDS)
        got = obj.sampleb(b_in, s.shape, s.scale, apar, seed=123, sweep=9)
        Q = L.stb_sampleb_last_Q()
        _, T_now = obj.get()
        assert Q > 1.0 / s.scale
        check_run(f"stb_{kind}_sampleb a={apar!r} b_in={b_in!r}", got, hr.b_bracket(b_in), b_truth(s, Q, apar, T=T_now))
    finally:
        obj.free()
