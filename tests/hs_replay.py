"""An end-to-end account of a samplea / sampleb draw without any observed number (test infrastructure only; reads nothing
from the reference tree or the device).

arms_simple is a deterministic function of libc's rand() stream and of the sequence of posterior values it is handed, and
csrc/arms.c is bit-exact to the reference on the CPU (tests/test_host_logic.py).  So a draw is accounted for by
  (A) every value of the run's trace lies within the derived bar of the truth at the abscissa the device was asked for
      (aterms_truth / bterms_truth below: the bars of hp_pairs / hp_oracle, no new constant), and
  (B) the library's own arms_simple, from the same streams and handed exactly those values, visits exactly those abscissae
      and returns exactly that draw and code (replay_arms).
The brackets of csrc/samplea.c and csrc/sampleb.c are restated here: the same expressions in the same order.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

import hp_oracle as hp
import hp_pairs as hpp
import orc
from libstb_amd import capi

# include/psample.h
A_MIN = 0.01
A_MAX = 0.98
SQUEEZEA = 0.2
B_MIN = 0.01
B_MAX = 2000
NPRE = 3
TRACE_CAP = 1024   # csrc/sampler_trace.c CAP: a longer trace keeps its count and loses the values


def a_bracket(mya: float):
    """csrc/samplea.c a_bracket: [lower, start, upper]"""
    inita = [A_MIN, mya, A_MAX]
    if math.fabs(inita[1] - A_MAX) / A_MAX < 0.00001:
        inita[1] = A_MAX * 0.999 + A_MIN * 0.001
    if math.fabs(inita[1] - A_MIN) / A_MIN < 0.00001:
        inita[1] = A_MIN * 0.999 + A_MAX * 0.001
    if inita[1] - SQUEEZEA > A_MIN:
        inita[0] = inita[1] - SQUEEZEA
    if inita[1] + SQUEEZEA < A_MAX:
        inita[2] = inita[1] + SQUEEZEA
    return inita


def b_bracket(b_in: float):
    """csrc/sampleb.c draw_b_posterior, the ARMS branch: [B_MIN, start, B_MAX]"""
    initb = [B_MIN, 1, B_MAX]
    initb[1] = b_in
    if math.fabs(initb[1] - B_MAX) / B_MAX < 0.00001:
        initb[1] = B_MAX * 0.999 + B_MIN * 0.001
    if math.fabs(initb[1] - B_MIN) / B_MIN < 0.00001:
        initb[1] = B_MIN * 0.999 + B_MAX * 0.001
    return [float(v) for v in initb]


def first_abscissae(init):
    """csrc/samplea.c a_first_abscissae (and sampleb.c's copy): the three abscissae ARMS fixes before any evaluation"""
    return [init[0] + (i + 1.0) * (init[2] - init[0]) / (NPRE + 1.0) for i in range(NPRE)]


def beta_Q(b_in: float, scale: float, N) -> float:
    """sampleb's Q = 1/scale - sum log Beta(b_in, N_i) drawn from the rand48 stream as csrc/sampleb.c:169-178 draws it"""
    L = capi.lib()
    Q = 1.0 / scale
    for Ni in N:
        if Ni <= 0:
            continue
        Q -= math.log(L.gsl_rng_beta(b_in, float(int(Ni))))
    return Q


def replay_arms(xl, xprev, xr, ys, seeds=(777, 12345), beta=None):
    """(code, xs, draw, overrun): the library's arms_simple(3, xl, xr, ..., dometrop = 0, xprev) from the libc streams seeded
    as the run's were, its posterior the recorded values: the i-th call is answered ys[i] and the x it asked for is kept.
    beta = (b_in, scale, N): sampleb with host counts first draws its Beta variates (beta_Q) from the same streams; the
    replay consumes the same draws.  The callback never raises; a call past the end of ys is answered ys[-1] and sets
    overrun."""
    L = capi.lib()
    ys = [float(y) for y in ys]
    xs = []
    state = {"overrun": False}

    def post(x, _):
        i = len(xs)
        xs.append(x)
        if i >= len(ys):
            state["overrun"] = True
            return ys[-1] if ys else 0.0
        return ys[i]

    cb = capi.LOGDENS(post)
    orc.seed_libc(*seeds)
    if beta is not None:
        beta_Q(*beta)
    lo, hi, prev, out = C.c_double(xl), C.c_double(xr), C.c_double(xprev), C.c_double(float("nan"))
    code = L.arms_simple(3, C.byref(lo), C.byref(hi), cb, None, 0, C.byref(prev), C.byref(out))
    return int(code), xs, out.value, state["overrun"]


def reference_bounds(n, t):
    """(N, M) of the table the reference's samplea builds: M = max(max t + 1, 10), N = max(max n + 1, M)"""
    M = max(int(t.max()) + 1 if len(t) else 1, 10)
    N = max(int(n.max()) + 1 if len(n) else 1, M)
    return N, M


_a_truths = {}


def aterms_truth(K, n, t, T, bpar, xs):
    """[(truth, bar)] of aterms at every abscissa of a trace in ONE pass over the truth's rows (hp_pairs.aterms_truth's
    values and bars at the reference's bounds; kept here under a key that holds T and bpar too, which the sampler cases
    change over unchanged pairs)"""
    K, n, t, T = (np.ascontiguousarray(v) for v in (K, n, t, T))
    bpar = np.ascontiguousarray(bpar, dtype=np.float64)
    xs = np.asarray(xs, dtype=np.float64)
    N, M = reference_bounds(n, t)
    key = (K.tobytes(), n.tobytes(), t.tobytes(), T.tobytes(), bpar.tobytes(), xs.tobytes())
    if key not in _a_truths:
        cls = np.zeros(len(n), dtype=np.int8)
        _a_truths[key] = hpp.aterms_truth_by_class([(K, n, t, T, bpar, cls)], xs, N, M)[0].sums()
    return _a_truths[key]


def bterms_truth(xs, Q, shape, T, apar):
    """[(truth, bar)] of bterms per abscissa: hp_oracle.bterms and its bar + 4 u |truth| (as tests/test_gpu_hp.py holds the
    device's bterms)"""
    out = []
    for x in xs:
        tv, tb = hp.bterms(float(x), Q, shape, T, apar)
        out.append((tv, tb + 4 * hp.U * abs(tv)))
    return out


def same(a: float, b: float) -> bool:
    """bit-equal doubles (two NaNs count as equal: a draw ARMS never wrote)"""
    return (a != a and b != b) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


def replay_differences(xs, code, draw, rep):
    """what statement (B) finds wrong, as text ([] when the replay `rep` of replay_arms is the run (xs, code, draw))"""
    rcode, rxs, rdraw, overrun = rep
    out = []
    if overrun:
        out.append(f"the replay asked for more values than the run's {len(xs)}")
    if len(rxs) != len(xs):
        out.append(f"the replay made {len(rxs)} evaluations, the run {len(xs)}")
    for i, (a, b) in enumerate(zip(xs, rxs)):
        if not same(float(a), float(b)):
            out.append(f"abscissa {i}: run {float(a).hex()}, replay {float(b).hex()}")
            break
    if rcode != code:
        out.append(f"code: run {code}, replay {rcode}")
    if not same(float(draw), float(rdraw)):
        out.append(f"draw: run {float(draw).hex()}, replay {float(rdraw).hex()}")
    return out


def errs(ys, truth):
    """(|y - truth|, bar) per abscissa as doubles (the difference taken in long double)"""
    e = np.array([abs(float(hp.LD(float(y)) - hp.LD(tv))) for y, (tv, _) in zip(ys, truth)])
    return e, np.array([float(b) for _, b in truth])
