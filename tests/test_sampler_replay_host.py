"""tests/hs_replay.py on the CPU: the replay proves itself on analytic densities (and demonstrably fails when one value is
moved), the Python brackets are the recorded runs' brackets, and the reference's recorded samplea / sampleb runs are held
to the truth -- with the reference's own summation noise printed next to the device's bar (MEASUREMENTS.md reads the
table from these lines; nothing is asserted on the noise)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import hs_replay as hr
import orc
from libstb_amd import capi, synth
from test_host_logic import density

fh = float.fromhex
NAN = float("nan")

SETS = {"small_wide": (20, 30, 300, "wide"), "small_real": (20, 30, 300, "realistic"), "mid_wide": (100, 100, 1000, "wide")}
A_STARTS = [0.01, 0.0100001, 0.15, 0.21, 0.5, 0.78, 0.9, 0.9799999, 0.98]


def load(golden_dir, name):
    with open(os.path.join(golden_dir, name)) as f:
        return json.load(f)


def run_arms(c, ys_out):
    """arms_simple on the analytic density of an arms.json case (dometrop = 0): (xs, code, draw), the values into ys_out"""
    L = capi.lib()
    p0, p1, p2 = (fh(v) for v in c["p"])
    calls = []
    inner = density(c["kind"], p0, p1, p2, calls)

    def post(x, _):
        y = inner(x, None)
        ys_out.append(y)
        return y

    cb = capi.LOGDENS(post)
    orc.seed_libc(c["seed"], 12345)
    xl, xr = C.c_double(fh(c["xl"])), C.c_double(fh(c["xr"]))
    xprev, xsamp = C.c_double(fh(c["xprev"])), C.c_double(NAN)
    code = L.arms_simple(3, C.byref(xl), C.byref(xr), cb, None, 0, C.byref(xprev), C.byref(xsamp))
    return calls, code, xsamp.value


def arms_cases(golden_dir):
    return [c for c in load(golden_dir, "arms.json") if c["dometrop"] == 0]


# ---- the helper proves itself

def test_replay_reproduces_arms_on_analytic_densities(golden_dir):
    cases = arms_cases(golden_dir)
    assert {c["kind"] for c in cases} == {0, 1, 2, 3, 4}
    for c in cases:
        ys = []
        xs, code, draw = run_arms(c, ys)
        assert [x.hex() for x in xs] == c["xs"] and code == c["code"]     # (the run is the recorded one)
        rep = hr.replay_arms(fh(c["xl"]), fh(c["xprev"]), fh(c["xr"]), ys, seeds=(c["seed"], 12345))
        assert hr.replay_differences(xs, code, draw, rep) == [], (c, rep)


def test_replay_fails_when_one_value_is_moved(golden_dir):
    """statement (B) cannot pass by construction: with ONE y moved by 1e-6 relative the replay reports a differing abscissa
    or an overrun.  The run: the first of arms.json that draws (code 0) with at least three evaluations after the three
    starting ones, its first value moved (the envelope every later abscissa is drawn from is built on it).  Not every value
    moves a run -- one so far below the others that its exponential vanishes in the envelope's areas does not -- so for the
    other runs it is only asked that some value of the starting three does."""
    runs = [c for c in arms_cases(golden_dir) if c["code"] == 0 and c["ncalls"] >= 6]
    assert len(runs) >= 8

    def moved_run(c, k):
        ys = []
        xs, code, draw = run_arms(c, ys)
        moved = list(ys)
        moved[k] = ys[k] * (1.0 + 1e-6)
        assert moved[k] != ys[k]
        rep = hr.replay_arms(fh(c["xl"]), fh(c["xprev"]), fh(c["xr"]), moved, seeds=(c["seed"], 12345))
        diff = hr.replay_differences(xs, code, draw, rep)
        return len(ys), diff, any(d.startswith("abscissa") for d in diff) or rep[3]

    c = runs[0]
    count, diff, caught = moved_run(c, 0)
    print(f"moved y[0] of kind {c['kind']} seed {c['seed']} ({count} evaluations) by 1e-6 relative: " + "; ".join(diff))
    assert caught, diff
    for c in runs[1:]:
        assert any(moved_run(c, k)[2] for k in range(3)), (c["kind"], c["seed"])


def test_replay_callback_never_raises_past_the_end(golden_dir):
    c = next(c for c in arms_cases(golden_dir) if c["code"] == 0 and c["ncalls"] >= 6)
    ys = []
    xs, code, draw = run_arms(c, ys)
    rcode, rxs, rdraw, overrun = hr.replay_arms(fh(c["xl"]), fh(c["xprev"]), fh(c["xr"]), ys[:4], seeds=(c["seed"], 12345))
    assert overrun and len(rxs) > 4 and [x.hex() for x in rxs[:4]] == c["xs"][:4]
    rcode, rxs, rdraw, overrun = hr.replay_arms(fh(c["xl"]), fh(c["xprev"]), fh(c["xr"]), ys, seeds=(c["seed"], 12345))
    assert not overrun


# ---- the brackets

def test_a_bracket_is_the_recorded_runs(golden_dir):
    """the recorded samplea runs (they start at 0.5, 0.1 and 0.98): the bracket ARMS was given and its first three abscissae,
    bit for bit.  The starts of A_STARTS no run was recorded at are checked against the C code's own expressions written
    out by hand here; tests/test_gpu_sampler_replay.py pins them to the library's trace on the device."""
    recs = load(golden_dir, "samplers.json")["samplea"]
    seen = set()
    for rec in recs:
        a_in = fh(rec["a_in"])
        init = hr.a_bracket(a_in)
        assert init[0].hex() == rec["trace"]["xl"] and init[2].hex() == rec["trace"]["xr"], (a_in, init)
        assert [x.hex() for x in hr.first_abscissae(init)] == rec["trace"]["x"][:3], a_in
        seen.add(a_in)
    assert {0.5, 0.98} <= seen & set(A_STARTS)
    lo_start, hi_start = 0.01 * 0.999 + 0.98 * 0.001, 0.98 * 0.999 + 0.01 * 0.001
    want = {0.01: [0.01, lo_start, lo_start + 0.2], 0.0100001: [0.01, lo_start, lo_start + 0.2],     # the lower nudge
            0.15: [0.01, 0.15, 0.15 + 0.2], 0.21: [0.01, 0.21, 0.21 + 0.2],                         # 0.21 - 0.2 > 0.01 is false
            0.5: [0.5 - 0.2, 0.5, 0.5 + 0.2], 0.78: [0.78 - 0.2, 0.78, 0.98], 0.9: [0.9 - 0.2, 0.9, 0.98],
            0.9799999: [hi_start - 0.2, hi_start, 0.98], 0.98: [hi_start - 0.2, hi_start, 0.98]}       # the upper nudge
    for a_in in A_STARTS:
        init = hr.a_bracket(a_in)
        assert init == want[a_in], (a_in, init, want[a_in])
        x3 = hr.first_abscissae(init)
        assert init[0] < x3[0] < x3[1] < x3[2] < init[2] and init[0] <= init[1] <= init[2]


def test_b_bracket_is_the_recorded_runs(golden_dir):
    seen = set()
    for rec in load(golden_dir, "samplers.json")["sampleb"]:
        if fh(rec["apar"]) == 0.0:
            continue
        b_in = fh(rec["b_in"])
        init = hr.b_bracket(b_in)
        assert init[0].hex() == rec["trace"]["xl"] and init[2].hex() == rec["trace"]["xr"]
        assert [x.hex() for x in hr.first_abscissae(init)] == rec["trace"]["x"][:3], b_in
        seen.add(b_in)
    assert seen == {0.5, 10.0, 2000.0}
    assert hr.b_bracket(2000.0)[1] == 2000 * 0.999 + 0.01 * 0.001 and hr.b_bracket(0.01)[1] == 0.01 * 0.999 + 2000 * 0.001
    assert hr.b_bracket(10.0) == [0.01, 10.0, 2000.0]


# ---- the recorded reference runs against the truth

def a_records(golden_dir):
    return [r for r in load(golden_dir, "samplers.json")["samplea"] if r["set"] in SETS]


def b_records(golden_dir):
    return [r for r in load(golden_dir, "samplers.json")["sampleb"] if r["set"] in SETS and fh(r["apar"]) != 0.0]


def noise_line(what, ys, truth, xs, want_x, draw, want_draw, n_agree, code_agree):
    e, bar = hr.errs(ys, truth)
    tv = np.array([abs(float(t)) for t, _ in truth])
    relx = float(np.max(np.abs(np.array(xs[:len(want_x)]) - np.array(want_x[:len(xs)])) / np.abs(np.array(want_x[:len(xs)]))))
    print(f"{what}: {len(ys)} evaluations, max |y_ref - truth| {e.max():.3e} ({np.max(e / tv):.2e} relative), largest device bar "
          f"{bar.max():.3e}, worst |y_ref - truth| / bar {np.max(e / bar):.3g}; ARMS on the truth: count "
          f"{'agrees' if n_agree else 'differs'}, code {'agrees' if code_agree else 'differs'}, max rel dx {relx:.2e}, "
          f"|draw - recorded| {abs(draw - want_draw):.2e}")


@pytest.mark.parametrize("index", range(9))
def test_recorded_samplea_runs_against_the_truth(golden_dir, index):
    L = capi.lib()
    rec = a_records(golden_dir)[index]
    g = synth.groups(*SETS[rec["set"]])
    want_x = [fh(v) for v in rec["trace"]["x"]]
    want_y = [fh(v) for v in rec["trace"]["y"]]
    truth = hr.aterms_truth(g.K, g.n, g.t, g.T, g.bpar, want_x)
    e, _ = hr.errs(want_y, truth)
    # ARMS on float(truth) from the same streams: where it asks for a recorded abscissa the pass above answers
    known = {x: float(tv) for x, (tv, _) in zip(want_x, truth)}
    xs = []

    def post(x, _):
        xs.append(x)
        if x not in known:
            known[x] = float(hr.aterms_truth(g.K, g.n, g.t, g.T, g.bpar, [x])[0][0])
        return known[x]

    a_in = fh(rec["a_in"])
    init = hr.a_bracket(a_in)
    orc.seed_libc(777, 12345)
    lo, hi, prev, out = C.c_double(init[0]), C.c_double(init[2]), C.c_double(init[1]), C.c_double(NAN)
    code = L.arms_simple(3, C.byref(lo), C.byref(hi), capi.LOGDENS(post), None, 0, C.byref(prev), C.byref(out))
    noise_line(f"samplea {rec['set']} a_in={a_in!r}", want_y, truth, xs, want_x, out.value, fh(rec["a_out"]),
               len(xs) == rec["trace"]["count"], code == rec["trace"]["code"])
    for y, (tv, _), d in zip(want_y, truth, e):
        assert d <= 1e-10 * abs(float(tv)), (rec["set"], a_in, y, float(tv), d)


@pytest.mark.parametrize("index", range(9))
def test_recorded_sampleb_runs_against_the_truth(golden_dir, index):
    L = capi.lib()
    rec = b_records(golden_dir)[index]
    g = synth.groups(*SETS[rec["set"]])
    b_in, apar = fh(rec["b_in"]), fh(rec["apar"])
    want_x = [fh(v) for v in rec["trace"]["x"]]
    want_y = [fh(v) for v in rec["trace"]["y"]]
    orc.seed_libc(777, 12345)
    Q = hr.beta_Q(b_in, g.scale, g.N)
    truth = hr.bterms_truth(want_x, Q, g.shape, g.T, apar)
    e, _ = hr.errs(want_y, truth)
    known = {x: float(tv) for x, (tv, _) in zip(want_x, truth)}
    xs = []

    def post(x, _):
        xs.append(x)
        if x not in known:
            known[x] = float(hr.bterms_truth([x], Q, g.shape, g.T, apar)[0][0])
        return known[x]

    init = hr.b_bracket(b_in)
    orc.seed_libc(777, 12345)
    assert hr.beta_Q(b_in, g.scale, g.N) == Q
    lo, hi, prev, out = C.c_double(init[0]), C.c_double(init[2]), C.c_double(init[1]), C.c_double(NAN)
    code = L.arms_simple(3, C.byref(lo), C.byref(hi), capi.LOGDENS(post), None, 0, C.byref(prev), C.byref(out))
    noise_line(f"sampleb {rec['set']} b_in={b_in!r} a={apar!r}", want_y, truth, xs, want_x, out.value, fh(rec["b_out"]),
               len(xs) == rec["trace"]["count"], code == rec["trace"]["code"])
    for y, (tv, _), d in zip(want_y, truth, e):
        assert d <= 1e-10 * abs(float(tv)), (rec["set"], b_in, apar, y, float(tv), d)


def test_the_records_are_the_ones_the_issue_names(golden_dir):
    assert len(a_records(golden_dir)) == 9 and len(b_records(golden_dir)) == 9
    assert {r["set"] for r in a_records(golden_dir)} == set(SETS) == {r["set"] for r in b_records(golden_dir)}
