"""The class draw on the device (libstb_amd/csrc/classgen.hip; include/stb_hip.h, "customers' classes drawn on the device"):
bit for bit against tests/cg_oracle.py's replay, whatever the geometry; the object's calls; the joint law of
(dish sweep, class draw) on the device."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import cg_oracle as cgo
import st_oracle as sto
import tl_oracle as tlo
from libstb_amd import capi
from test_gpu_predict import dev, same_bits
from test_gpu_seat import make_object, object_case
from test_gpu_tdish import assert_state, fetch
from test_gpu_tlik import assert_replayed, read_lik

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_CAP = 2048          # CG_GRID_CAP: k_cls_draw's grid is capped at this many workgroups, of 256 lanes by default
PAST_ONE_STEP = GRID_CAP * 256 + 77


def run_raw(lik, cust, seed, sweep, cls0, mask=None, info0=(0, 0, 0)):
    """stb_sample_classes on host arrays: (cls after the call, the three counters)"""
    import torch

    d_cls = dev(cls0, np.uint32)
    d_info = torch.as_tensor(np.array(info0, dtype=np.int64), device="cuda")
    capi.sample_classes(dev(lik, np.float64), dev(cust, np.uint32), seed, sweep, d_cls,
                        None if mask is None else torch.as_tensor(np.ascontiguousarray(mask, dtype=np.uint8), device="cuda"), d_info)
    torch.cuda.synchronize()
    return d_cls.cpu().numpy().view(np.uint32), tuple(int(v) for v in d_info.cpu().numpy())


def raw_case(rows, K, pad, C, seed=0xC1A5):
    """(lik with zero cells and, where there is room, a zero column; dishes up to K + 1, the last two past a stride of K;
    a mask; the classes before)"""
    stride = K + pad
    rng = np.random.default_rng([seed, rows, stride, C])
    lik = cgo.matrix_with_zeros(rows, stride, seed, zero_col=(2 if stride > 2 else None))
    if stride > 3 and rows >= 9:      # a column whose Z is the smallest subnormal twice: the rule's second form is reached
        lik[:, 3] = 0.0
        lik[3, 3] = lik[7, 3] = 2.0 ** -1074
    cust = rng.integers(0, stride + 2, size=C).astype(np.uint32)
    mask = (rng.random(C) < 0.7).astype(np.uint8)
    cls0 = rng.integers(0, rows, size=C).astype(np.uint32)
    return lik, cust, mask, cls0


@pytest.mark.parametrize("rows", [1, 2, 255, 256, 257, 513, 1000])
@pytest.mark.parametrize("pad", [0, 3])
def test_the_raw_call_equals_the_replay(rows, pad):
    K = 130 if rows in (257, 1000) else 5          # dishes past one block of 64 lanes
    for C in (0, 1, 63, 64, 65, 5000):
        lik, cust, mask, cls0 = raw_case(rows, K, pad, C)
        for m in (None, mask):
            want, winfo = cgo.sample_classes(lik, cust, 77, 3, cls0, m)
            got, ginfo = run_raw(lik, cust, 77, 3, cls0, m, info0=(5, 6, 7))
            assert np.array_equal(got, want), (C, m is None, np.flatnonzero(got != want)[:10])
            assert ginfo == (winfo[0] + 5, winfo[1] + 6, winfo[2] + 7), (C, ginfo, winfo)       # added to what was there
            if m is not None:
                assert np.array_equal(got[m == 0], cls0[m == 0])
        if C == 5000:
            full, info = cgo.sample_classes(lik, cust, 77, 3, cls0)
            assert info[0] > 0 and info[2] > 0 and (info[1] > 0) == (K + pad > 2)
            drawn = (cust < K + pad) & (lik.sum(axis=0) > 0.0)[np.minimum(cust, K + pad - 1)]
            assert np.all(lik[full[drawn], cust[drawn]] > 0.0)               # never a class of zero weight
            if K + pad > 3 and rows >= 9:
                u = cgo.uniforms(77, 3, C)[cust == 3]
                assert any(cgo.fallback_reached(2.0 ** -1073, x) for x in u) and set(full[cust == 3]) == {3, 7}


def test_a_call_past_one_grid_step():
    C = PAST_ONE_STEP
    rng = np.random.default_rng(8)
    lik = cgo.matrix_with_zeros(300, 9, 5)
    cust = rng.integers(0, 9, size=C).astype(np.uint32)
    cls0 = np.full(C, 0xABCD, dtype=np.uint32)
    want, winfo = cgo.sample_classes(lik, cust, 9, 1, cls0)
    got, ginfo = run_raw(lik, cust, 9, 1, cls0)
    assert np.array_equal(got, want) and ginfo == winfo and winfo[2] == C
    assert not np.array_equal(got[:77], got[C - 77:])


def test_no_call_without_its_arrays():
    import torch

    L = capi.lib()
    lik = dev(np.ones((4, 3)), np.float64)
    cust = dev(np.zeros(5), np.uint32)
    cls = dev(np.full(5, 9), np.uint32)
    for args in ((None, 4, 3, cust.data_ptr(), None, 5, 1, 0, cls.data_ptr(), None, None),
                 (lik.data_ptr(), 4, 3, None, None, 5, 1, 0, cls.data_ptr(), None, None),
                 (lik.data_ptr(), 4, 3, cust.data_ptr(), None, 5, 1, 0, None, None, None),
                 (lik.data_ptr(), 0, 3, cust.data_ptr(), None, 5, 1, 0, cls.data_ptr(), None, None),
                 (lik.data_ptr(), 4, 0, cust.data_ptr(), None, 5, 1, 0, cls.data_ptr(), None, None)):
        assert L.stb_sample_classes(*args) != 0 and capi.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(cls.cpu().numpy(), np.full(5, 9))


# ---- geometry

def _digest():
    h = hashlib.sha256()
    for rows, K, pad, C in ((1000, 130, 3, 5000), (257, 130, 0, 65), (513, 5, 3, 5000)):
        lik, cust, mask, cls0 = raw_case(rows, K, pad, C)
        got, info = run_raw(lik, cust, 77, 3, cls0, mask)
        h.update(got.tobytes())
        h.update(np.array(info, dtype=np.int64).tobytes())
    return h.hexdigest()


def test_the_bits_do_not_depend_on_the_waves_of_a_workgroup():
    # a fresh process per setting, the four at once
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    procs = {w: subprocess.Popen([sys.executable, os.path.abspath(__file__), "--digest"], env=dict(env, STB_CLS_WAVES=str(w)),
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for w in (1, 2, 4, 8)}
    out = {}
    for w, p in procs.items():
        so, se = p.communicate(timeout=120)
        assert p.returncode == 0, (w, se[-2000:])
        out[w] = so.strip().splitlines()[-1]
    assert len(out[4]) == 64 and len(set(out.values())) == 1, out
    assert out[4] == _digest()                                  # and this process, at the default


# ---- the object

def test_generate_is_the_composition_and_the_replay():
    a = 0.45
    case = object_case(True)
    K, n, t, h, bpar, coff, cls, lik = case
    rp = cgo.generate(K, h, a, bpar, coff, lik, seed=77, sweep=4)
    ti, tj = make_object(case), make_object(case)
    try:
        si, ci = ti.generate(a, bpar, 77, 4)
        assert_state(fetch(ti), (rp["n"], rp["t"], rp["T"], rp["cust"]))
        got, rows = ti.get_classes()
        assert np.array_equal(got, rp["cls"]) and rows == lik.shape[0]
        assert (si.skipped, si.impossible, si.stuck, si.customers) == (0, 0, 0, int(coff[-1]))
        assert (ci.skipped, ci.stuck, ci.drawn) == rp["cls_info"]
        # the four calls a caller can write around the draw
        tj.set_lik(None)
        tj.seat(a, bpar, 77, 4)
        tj.set_lik(lik)
        cj = tj.sample_classes(77, 4)
        assert_state(fetch(tj), fetch(ti))
        assert np.array_equal(tj.get_classes()[0], got) and (cj.skipped, cj.stuck, cj.drawn) == rp["cls_info"]
        # another stream, another corpus
        ti.generate(a, bpar, 77, 5)
        assert not np.array_equal(ti.get_classes()[0], got)
    finally:
        ti.free()
        tj.free()


def test_the_object_goes_on_after_a_draw_and_nothing_else_is_written():
    a = 0.45
    case = object_case(True)
    K, n, t, h, bpar, coff, cls, lik = case
    C = int(coff[-1])
    rng = np.random.default_rng(4)
    mask = (rng.random(C) < 0.5).astype(np.uint8)
    ti = make_object(case)
    bare = capi.TableIndicators(K, n, t, h)         # created without classes, in pair order
    try:
        before, h0 = fetch(ti), ti.get_h()
        want, winfo = cgo.sample_classes(lik, before[3], 21, 2, cls, mask)
        ci = ti.sample_classes(21, 2, mask)
        got, rows = ti.get_classes()
        assert np.array_equal(got, want) and rows == lik.shape[0] and (ci.skipped, ci.stuck, ci.drawn) == winfo
        assert np.array_equal(got[mask == 0], cls[mask == 0]) and not np.array_equal(got, cls)
        assert_state(fetch(ti), before)
        assert same_bits(ti.get_h(), h0)
        assert same_bits(read_lik(ti), lik)
        # the counts and the data term of the fetched state
        cnt = np.zeros(lik.shape, dtype=np.uint32)
        np.add.at(cnt, (want, before[3]), 1)
        assert np.array_equal(ti.class_counts(), cnt)
        tot, imp = ti.loglik()
        wtot, wimp = tlo.loglik(cnt, lik)
        assert imp == wimp and wimp > 0 and tot == wtot == -np.inf         # a kept class of no weight at its dish
        # without a wait, then the next draw of the matrix from the counts of the classes that call left
        assert ti.sample_classes(22, 0, want_info=False) is None
        cls2, _ = ti.get_classes()
        want2, _ = cgo.sample_classes(lik, before[3], 22, 0, want)
        assert np.array_equal(cls2, want2)
        cnt2 = np.zeros(lik.shape, dtype=np.uint32)
        np.add.at(cnt2, (want2, before[3]), 1)
        tot, imp = ti.loglik()                    # every class drawn: none without weight
        wtot, wimp = tlo.loglik(cnt2, lik)
        bar = 2.0 ** -53 * 4.0 * float(np.sum(cnt2 * np.abs(np.log(np.where(cnt2 > 0, lik, 1.0)))))
        assert imp == wimp == 0 and abs(tot - wtot) <= bar, (tot, wtot, bar)
        ti.sample_lik(0.5, 31, 0)
        wlik, margin = tlo.sample_lik(cnt2, 0.5, 31, 0)
        assert margin > 1e-9
        assert_replayed(read_lik(ti), wlik, "the matrix drawn from the drawn classes' counts")
        assert_state(fetch(ti), before)
        # an object without classes gets them; its sequence is pair order
        with pytest.raises(capi.StbError, match="lik"):
            bare.sample_classes(5, 0)
        bare.set_lik(lik)
        with pytest.raises(capi.StbError, match="mask"):
            bare.sample_classes(5, 0, mask)
        with pytest.raises(capi.StbError, match="classes"):
            bare.get_classes()
        bi = bare.sample_classes(5, 0)
        bcust = bare.get_state()[1]
        wb, wbi = cgo.sample_classes(lik, bcust, 5, 0, np.zeros(C, dtype=np.uint32))
        assert np.array_equal(bare.get_classes()[0], wb) and (bi.skipped, bi.stuck, bi.drawn) == wbi
        assert bare.class_counts().sum() == C
    finally:
        ti.free()
        bare.free()


def test_refusals_leave_the_object_as_it_was():
    a = 0.45
    case = object_case(False)
    K, n, t, h, bpar, coff, cls, lik = case
    ti = make_object(case)
    ref = make_object(case, flags=capi.TI_REF_ODDS)
    nolik = make_object(case, with_lik=False)
    more = make_object(case)
    try:
        more.set_classes(cls, lik.shape[0] + 2)       # classes set with more rows than the matrix has
        before, cls0 = fetch(ti), ti.get_classes()
        bad_b = bpar.copy()
        bad_b[3] = -a
        for call in (lambda: ti.generate(1.0, bpar, 1, 0), lambda: ti.generate(-0.5, bpar, 1, 0), lambda: ti.generate(a, bad_b, 1, 0),
                     lambda: ref.generate(a, bpar, 1, 0), lambda: nolik.generate(a, bpar, 1, 0), lambda: nolik.sample_classes(1, 0),
                     lambda: more.sample_classes(1, 0), lambda: more.generate(a, bpar, 1, 0)):
            with pytest.raises(capi.StbError):
                call()
        L = capi.lib()
        assert L.stb_tindic_sample_classes(None, None, 1, 0, None) != 0
        assert L.stb_tindic_generate(None, a, capi.dp(bpar), 1, 0, None, None) != 0
        assert L.stb_tindic_generate(ti.h, a, None, 1, 0, None, None) != 0
        assert L.stb_tindic_get_classes(None, None, None) != 0
        for o in (ti, ref, nolik, more):
            assert_state(fetch(o), before)
        got = ti.get_classes()
        assert np.array_equal(got[0], cls0[0]) and got[1] == cls0[1] == lik.shape[0]
        assert more.get_classes()[1] == lik.shape[0] + 2 and np.array_equal(more.get_classes()[0], cls)
    finally:
        for o in (ti, ref, nolik, more):
            o.free()


# ---- the joint law on the device

def test_generate_and_the_alternation_keep_the_joint_law_on_the_device():
    K, h, bpar, coff, lik = cgo.joint_case()
    I, a, seed = cgo.JOINT_I, cgo.JOINT_A, cgo.JOINT_SEED
    law = cgo.joint_law()
    assert cgo.merged_mass(list(law.values()), I) <= 0.02
    ti = capi.TableIndicators(K, np.tile(np.array([2, 1], dtype=np.uint32), I), np.tile(np.array([1, 1], dtype=np.uint16), I), h)
    try:
        ti.set_lik(lik)
        si, ci = ti.generate(a, bpar, seed, 0)
        assert (si.skipped, si.impossible, si.stuck, ci.skipped, ci.stuck, ci.drawn) == (0, 0, 0, 0, 0, 3 * I)
        (n0, t0, T0, cust0), cls0 = fetch(ti), ti.get_classes()[0]
        rp = cgo.generate(K, h, a, bpar, coff, lik, seed=seed, sweep=0)
        assert_state((n0, t0, T0, cust0), (rp["n"], rp["t"], rp["T"], rp["cust"]))
        assert np.array_equal(cls0, rp["cls"])
        p0 = sto.chi2_p(cgo.joint_cells(cust0, t0, cls0), law, I)
        cls = cls0
        changed = []
        for r in range(1, cgo.JOINT_ROUNDS + 1):
            info = ti.sweep_dishes(a, bpar, seed, r)
            assert (info.skipped, info.stuck) == (0, 0)
            ti.sample_classes(seed, r, want_info=False)
            new = ti.get_classes()[0]
            changed.append(int((new != cls).sum()))
            cls = new
        n1, t1, T1, cust1 = fetch(ti)
        last = cgo.joint_cells(cust1, t1, cls)
        p1 = sto.chi2_p(last, law, I)
        q = sto.chi2_p(last, cgo.joint_law(cgo.swapped(cgo.JOINT_LIK)), I)
        print("generate p", p0, "after the rounds p", p1, "columns exchanged p", q, "classes changed", changed)
        assert p0 > 1e-3 and p1 > 1e-3 and q < 1e-9
        assert min(changed) >= 1
    finally:
        ti.free()


# ---- the example

EXE = os.path.join(ROOT, "examples", "bin", "pyp_resample")


def test_example_generates_its_corpus_on_the_device():
    import math
    import re

    assert os.path.exists(EXE), "examples/bin/pyp_resample not built (make -C libstb_amd/csrc)"
    base = [EXE, "-J", "3", "-n", "400", "-c", "4", "-s", "5", "-d", "-z"]
    p = subprocess.run(base + ["-V", "300"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    assert re.search(r"^corpus generated on the device: 1200 customers, 1200 classes drawn over 300 rows, 0 left alone$", p.stdout, re.M), p.stdout
    assert re.search(r"^start state seated on the device: 1200 customers, log weight \S+, 0 impossible visits$", p.stdout, re.M), p.stdout
    rows = re.findall(r"^iteration (\d+): generated corpus data (\S+) collapsed (\S+)$", p.stdout, re.M)
    assert [int(r[0]) for r in rows] == [0, 1, 2, 3], p.stdout
    assert all(math.isfinite(float(r[1])) and float(r[1]) < 0.0 and math.isfinite(float(r[2])) for r in rows), p.stdout
    # without -V the lines are the old ones; -V alone, or with too few rows, is refused
    q = subprocess.run(base, capture_output=True, text=True, timeout=60)
    assert q.returncode == 0 and "generated" not in q.stdout and "seated on the device" not in q.stdout
    for args in (["-V", "300"], ["-d", "-V", "300"], ["-d", "-z", "-V", "1"]):
        assert subprocess.run([EXE] + args, capture_output=True, text=True, timeout=60).returncode == 2, args


if __name__ == "__main__":
    if sys.argv[1:] == ["--digest"]:
        print(_digest())
