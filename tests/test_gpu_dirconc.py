"""The Dirichlet concentrations drawn on the device (libstb_amd/csrc/dirconc.hip; include/stb_hip.h stb_sample_dirconc,
stb_tindic_sample_beta, stb_tindic_sample_gamma): the step against the numpy replay (tests/dc_oracle.py) in both
orientations, launch geometries, the anchor to stb_sample_hgroups, the object layer, the law, the edges and
examples/pyp_resample -K.  tests/test_dirconc_host.py checks the margins of every seed used here on the CPU."""
import math
import os
import re
import subprocess
import time
from functools import lru_cache

import numpy as np
import pytest

import dc_oracle as dco
import hh_oracle as hho
from libstb_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(x, dtype):
    import torch

    a = np.ascontiguousarray(x, dtype=dtype)
    view = {np.uint16: np.int16, np.uint32: np.int32, np.uint64: np.int64}.get(dtype)
    return torch.as_tensor(a.view(view) if view else a, device="cuda")


def u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def device_step(c, **kw):
    """the raw call on a case dict (dc_oracle.case); kw overrides its entries.  Returns dict of numpy arrays + info"""
    import torch

    c = dict(c, **kw)
    v = c["v"] if np.ndim(c["v"]) == 0 else dev(c["v"], np.float64)
    s1, out, info = capi.sample_dirconc(dev(c["cnt"], np.uint32), v, c["s"], c["shape"], c["scale"], c["seed"], c["sweep"],
                                        c["orientation"], c["cols"])
    torch.cuda.synchronize()
    return dict(s=s1, m=u32(out["m"]), M=u32(out["M"]), count=info.count, aux_tables=info.aux_tables, nonempty=info.nonempty,
                zero_weight=info.zero_weight, error_word=info.error_word)


@lru_cache(maxsize=None)
def stepped(name):
    return dco.case(name), device_step(dco.case(name)), dco.replay_case(name)


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("m", "M")) and all(a[k] == b[k] for k in ("s", "count", "aux_tables", "nonempty"))


# ---- 1. the step against the replay ----

@pytest.mark.parametrize("name", list(dco.CASES))
def test_the_step_equals_the_replay(name):
    c, got, want = stepped(name)
    assert np.array_equal(got["m"], want["m"]), "m (every cell of the matrix's shape, 0 in the padding)"
    assert np.array_equal(got["M"], want["M"]), "M"
    assert got["count"] == want["count"] and got["aux_tables"] == want["aux_tables"] and got["nonempty"] == want["nonempty"]
    assert got["zero_weight"] == 0 and got["error_word"] == 0
    print(name, "s'", got["s"], "replay", want["s"], "relative", abs(got["s"] - want["s"]) / want["s"])
    assert abs(got["s"] - want["s"]) <= 1e-10 * want["s"] and got["s"] != c["s"]


def test_the_cases_reach_the_paths_they_are_for():
    body = lambda n: dco.case(n)["cnt"][:, :dco.case(n)["cols"]]
    assert dco.CASES["cols_257_7"][1] > 256 and dco.CASES["cols_3_65"][2] > 64 and dco.CASES["cols_300_70_96"][3] > 70
    assert set(np.unique(body("cols_cells"))) == set(dco.CELL_C)
    for n in ("cols_300_70_96", "cols_big", "rows_2_1024"):                   # cells on both sides of the wave form
        assert body(n).max() - 1 > 256 and ((body(n) >= 2) & (body(n) <= 257)).any()
    assert body("rows_big").max() == 300000
    assert stepped("cols_300_70_96")[1]["nonempty"] == 69 and stepped("cols_300_70_96")[1]["M"][5] == 0   # an empty multinomial


# ---- 2. geometry ----

@pytest.mark.parametrize("name", ["cols_300_70_96", "cols_big", "cols_cells", "cols_3_65", "rows_2_1024", "rows_big", "rows_513_3"])
def test_the_bits_do_not_depend_on_the_launch(name, monkeypatch):
    c, got, _ = stepped(name)
    for waves, form in ((1, "lane"), (2, "wave"), (4, "lane"), (8, "wave"), (8, ""), (1, ""), (4, "wave")):
        monkeypatch.setenv("STB_DIRCONC_WAVES", str(waves))
        monkeypatch.setenv("STB_DIRCONC_FORM", form)
        assert same_bits(device_step(c), got), (waves, form)


# ---- 3. the anchor to stb_sample_hgroups, bit for bit ----

def test_rows_on_a_normalised_root_is_the_grouped_steps_concentration():
    import torch

    rng = np.random.default_rng(77)
    I, Kmax = 300, 4
    K = np.full(I, Kmax, dtype=np.int32)
    t = rng.choice(np.array([0, 1, 2, 3, 40, 300], dtype=np.uint16), size=I * Kmax)
    goff = np.array([0, 1, 100, 100, 257, 300], dtype=np.uint64)
    root = np.array([0.5, 0.25, 0.125, 0.125])                       # sums to exactly 1.0: B = alpha, scale_B = scale
    alpha, shape, scale, seed, sweep = 1.7, 2.0, 4.0, 9301, 6
    koff = np.concatenate([[0], np.cumsum(K.astype(np.int64))])
    rd = dev(root, np.float64)
    _, out, info = capi.sample_hgroups(dev(koff, np.uint64), dev(t, np.uint16), Kmax, rd, alpha, 1.0, seed, sweep,
                                       goff=dev(goff, np.uint64), flags=capi.HG_KEEP_ROOT | capi.HG_SAMPLE_ALPHA, shape=shape,
                                       scale=scale, want=("c", "m"))
    torch.cuda.synchronize()
    s1, mine, dinfo = capi.sample_dirconc(out["c"], dev(root, np.float64), alpha, shape, scale, seed, sweep, capi.DM_ROWS)
    torch.cuda.synchronize()
    assert torch.equal(mine["m"], out["m"])
    assert s1 == info.alpha and s1 != alpha, (s1, info.alpha)
    assert dinfo.count == info.tables and dinfo.aux_tables == info.aux_tables


# ---- 4. the object ----

def small_object(seed=71):
    """64 restaurants of 6 dishes, 3 classes, a likelihood matrix of stride 8; dish 5 of the matrix's shape has no customer"""
    rng = np.random.default_rng(seed)
    I, Kd, Nc, rows = 64, 6, 30, 3
    cust = rng.integers(0, Kd - 1, size=I * Nc).astype(np.uint32)
    cls = rng.integers(0, rows, size=I * Nc).astype(np.uint32)
    n = np.stack([np.bincount(cust[i * Nc:(i + 1) * Nc].astype(np.int64), minlength=Kd) for i in range(I)]).astype(np.uint32)
    t = np.minimum(n, 1 + (n > 3)).astype(np.uint16)
    ti = capi.TableIndicators(np.full(I, Kd, dtype=np.int32), n.reshape(-1), t.reshape(-1), None, cust)
    ti.set_classes(cls, rows)
    ti.set_lik(None, rows, 8)
    return ti, I, Kd, rows


def state_of(ti):
    t, T = ti.get()
    n, cust = ti.get_state()
    return t, T, n, cust, ti.get_h(), ti.get_hroot(), ti.class_counts()


def test_the_objects_draws_are_the_raw_call_on_their_counts_and_write_nothing():
    import torch

    ti, I, Kd, rows = small_object()
    try:
        ti.sample_lik(0.5, 63, 0)
        ti.sample_h(1.0, 64, 0)
        before = state_of(ti)
        cnt = ti.class_counts()
        assert cnt.shape == (rows, 8) and cnt[:, 5:].sum() == 0
        for base in (None, np.array([0.5, 1.0, 2.5])):
            info = ti.sample_beta(0.8, 1.1, 1.0, 401, 3, base=base)
            v = 1.0 if base is None else dev(base, np.float64)
            s1, _, raw = capi.sample_dirconc(dev(cnt, np.uint32), v, 0.8, 1.1, 1.0, 401, 3, capi.DM_COLUMNS)
            assert info.s == s1 and info.s > 0 and info.s != 0.8
            assert (info.count, info.aux_tables, info.nonempty) == (raw.count, raw.aux_tables, raw.nonempty)
            assert info.count == cnt.sum() and info.nonempty == 5          # the dishes without a customer contribute nothing
        t = before[0].reshape(I, Kd).astype(np.uint32)
        ck = t.sum(axis=0, dtype=np.uint32)[None, :]
        for base in (None, 0.2 + np.arange(Kd) / 4.0):
            info = ti.sample_gamma(1.3, 1.1, 10.0, 402, 5, base=base)
            v = 1.0 if base is None else dev(base, np.float64)
            s1, _, raw = capi.sample_dirconc(dev(ck, np.uint32), v, 1.3, 1.1, 10.0, 402, 5, capi.DM_ROWS)
            assert info.s == s1 and info.s > 0 and info.s != 1.3
            assert (info.count, info.aux_tables, info.nonempty) == (raw.count, raw.aux_tables, 1) and info.count == ck.sum()
        torch.cuda.synchronize()
        for a, b in zip(before, state_of(ti)):
            assert np.array_equal(a, b)
        # refusals: _sample_lik's and _sample_h's, and the step's own
        for kw, match in ((dict(s=0.0), "s_in"), (dict(s=math.nan), "s_in"), (dict(shape=-1.0), "shape"), (dict(scale=math.inf), "scale"),
                          (dict(base=np.array([1.0, 0.0, 1.0])), "base")):
            args = dict(s=1.0, shape=1.0, scale=1.0, seed=1, sweep=0, base=None)
            args.update(kw)
            with pytest.raises(capi.StbError, match=match):
                ti.sample_beta(**args)
            if "base" not in kw:
                with pytest.raises(capi.StbError, match=match):
                    ti.sample_gamma(**args)
        L = capi.lib()
        assert L.stb_tindic_sample_beta(ti.h, None, 1.0, 1.0, 1.0, 1, 0, None) != 0 and "info" in capi.last_error()
        assert L.stb_tindic_sample_gamma(None, None, 1.0, 1.0, 1.0, 1, 0, None) != 0 and "null object" in capi.last_error()
        bare = capi.TableIndicators(np.full(2, 2, dtype=np.int32), np.ones(4, dtype=np.uint32), np.ones(4, dtype=np.uint16))
        odd = capi.TableIndicators(np.full(2, 2, dtype=np.int32), np.ones(4, dtype=np.uint32), np.ones(4, dtype=np.uint16), None, None, 0,
                                   capi.TI_REF_ODDS)
        try:
            with pytest.raises(capi.StbError, match="classes are not set"):
                bare.sample_beta(1.0, 1.0, 1.0, 1, 0)
            with pytest.raises(capi.StbError, match="STB_TI_REF_ODDS"):
                odd.sample_gamma(1.0, 1.0, 1.0, 1, 0)
            assert bare.sample_gamma(1.0, 1.0, 1.0, 1, 0).count == 4
        finally:
            bare.free()
            odd.free()
        for a, b in zip(before, state_of(ti)):
            assert np.array_equal(a, b)
    finally:
        ti.free()


# ---- 5. the law on the device ----

def test_the_chain_keeps_its_posterior():
    import torch

    f = dco.LAW_FIX["3x2"]
    cnt, v = dev(f["cnt"], np.uint32), dev(f["v"], np.float64)
    seed = dco.LAW_SEED["3x2"]

    def step(s, t):
        return capi.sample_dirconc(cnt, v, s, f["shape"], f["scale"], seed, t, capi.DM_ROWS, want=())[0]

    assert dco.LAW_BURN + dco.LAW_STEPS <= 6000
    kept = dco.chain("3x2", seed, step_fn=step)
    torch.cuda.synchronize()
    assert len(kept) == dco.LAW_STEPS // dco.LAW_THIN and np.all(np.isfinite(kept)) and np.all(kept > 0)
    pv = dco.law_pvalue("3x2", kept)
    print("KS p-value of s on the device", pv, "mean", kept.mean())
    assert pv > 1e-3


# ---- 6. the edges ----

def raw(cnt, rows, cols, stride, flags, v, w0, s, shape, scale, m, M, info):
    ptr = lambda x: None if x is None else x.data_ptr()
    return capi.lib().stb_sample_dirconc(ptr(cnt), rows, cols, stride, flags, ptr(v), w0, s, shape, scale, ptr(m), ptr(M), 1, 0,
                                         capi.stream_ptr(), None if info is None else capi.C.byref(info))


def test_refusals_leave_the_outputs_untouched():
    import torch

    cnt = dev(np.ones((3, 4)), np.uint32)
    m, M = dev(np.full((3, 4), 7), np.uint32), dev(np.full(4, 7), np.uint32)
    info = capi.DirConcInfo(-3.0, 11, 12, 13, 14, 15, 16)
    ok = dict(cnt=cnt, rows=3, cols=4, stride=4, flags=capi.DM_COLUMNS, v=None, w0=1.0, s=1.0, shape=1.0, scale=1.0, m=m, M=M, info=info)
    for kw, match in ((dict(cnt=None), "required"), (dict(info=None), "required"), (dict(cols=0), "cols=0"), (dict(cols=5), "cols=5"),
                      (dict(flags=0), "flags"), (dict(flags=3), "flags"), (dict(flags=4), "flags"), (dict(w0=0.0), "w0"),
                      (dict(w0=math.inf), "w0"), (dict(s=0.0), "s="), (dict(s=-1.0), "s="), (dict(s=math.nan), "s="),
                      (dict(s=math.inf), "s="), (dict(shape=0.0), "shape"), (dict(shape=math.nan), "shape"), (dict(scale=-2.0), "scale"),
                      (dict(scale=math.inf), "scale"), (dict(rows=0), "rows=0"), (dict(rows=0, flags=capi.DM_ROWS), "rows=0"),
                      (dict(rows=2 ** 31, flags=capi.DM_ROWS), "multinomials")):
        args = dict(ok, **kw)
        assert raw(**args) != 0, kw
        assert re.search(match, capi.last_error()), (match, capi.last_error())
    torch.cuda.synchronize()
    assert torch.all(m == 7) and torch.all(M == 7)
    assert (info.s, info.count, info.aux_tables, info.nonempty, info.zero_weight, info.error_word, info.reserved) == (-3.0, 11, 12, 13, 14, 15, 16)


def test_weights_of_zero():
    cnt = np.array([[3, 0, 300], [0, 0, 0], [1, 2, 0]], dtype=np.uint32)
    v = np.array([1.0, 0.0, 0.5])
    for orientation, mat in ((dco.COLUMNS, cnt), (dco.ROWS, cnt.T.copy())):
        c = dict(cnt=mat, cols=3, v=v, s=1.2, shape=1.5, scale=4.0, seed=6201, sweep=1, orientation=orientation)
        got = device_step(c)
        want = dco.replay(mat, v, 1.2, 1.5, 4.0, 6201, 1, orientation)     # (a cell without a count draws nothing there either)
        assert want["margin_gamma"] > 1e-9 and want["margin_y"] > 1e-9
        assert np.array_equal(got["m"], want["m"]) and np.array_equal(got["M"], want["M"])
        assert got["zero_weight"] == 3 and got["count"] == 306 and abs(got["s"] - want["s"]) <= 1e-10 * want["s"]
        # a count under a zero weight, a negative weight, a NaN, no weight at all
        for bad_v, bit in ((np.array([1.0, 1.0, 0.0]), 4), (np.array([1.0, -1.0, 1.0]), 1), (np.array([1.0, math.nan, 1.0]), 1),
                           (np.array([math.inf, 1.0, 1.0]), 1)):
            with pytest.raises(capi.StbError, match="error word 0x") as e:
                device_step(c, v=bad_v)
            assert e.value.info.error_word & bit and math.isnan(e.value.info.s), (bad_v, e.value.info.error_word)
    with pytest.raises(capi.StbError, match="error word 0x") as e:
        device_step(dict(cnt=np.zeros((3, 3), dtype=np.uint32), cols=3, v=np.zeros(3), s=1.0, shape=1.0, scale=1.0, seed=1, sweep=0,
                         orientation=dco.ROWS))
    assert e.value.info.error_word & 2


@pytest.mark.parametrize("orientation", [dco.COLUMNS, dco.ROWS])
def test_a_total_past_32_bits_fails_quickly_and_draws_nothing(orientation):
    """two cells of 2^31 in one multinomial: error bit 8 after the wait, within a second (the cells' 2^32 draws are never
    started), and m receives no draw: it is all zero, as is sum M"""
    import torch

    cells = np.array([[2 ** 31], [2 ** 31]], dtype=np.uint32)
    cnt = dev(cells if orientation == dco.COLUMNS else cells.T.copy(), np.uint32)
    capi.sample_dirconc(dev(np.ones((2, 2)), np.uint32), 1.0, 1.0, 1.0, 1.0, 1, 0, orientation)    # (the library is warm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with pytest.raises(capi.StbError, match="error word 0x8") as e:
        capi.sample_dirconc(cnt, 1.0, 1.0, 1.0, 1.0, 5, 0, orientation, want=())
    took = time.perf_counter() - t0
    print("failed after", took, "s")
    assert took < 1.0 and e.value.info.error_word == 8 and e.value.info.count == 2 ** 32 and e.value.info.aux_tables == 0
    m = dev(np.full(cnt.shape, 7), np.uint32)
    info = capi.DirConcInfo()
    assert raw(cnt, cnt.shape[0], cnt.shape[1], cnt.shape[1], orientation, None, 1.0, 1.0, 1.0, 1.0, m, None, info) != 0
    torch.cuda.synchronize()
    assert torch.all(m == 0) and info.error_word == 8


def test_a_matrix_without_counts_draws_from_the_prior():
    c = dict(cnt=np.zeros((3, 2), dtype=np.uint32), cols=2, v=np.array([0.5, 1.0, 0.25]), s=0.7, shape=2.0, scale=1.5, seed=6202, sweep=0,
             orientation=dco.COLUMNS)
    got = device_step(c)
    want = dco.replay(c["cnt"], c["v"], c["s"], c["shape"], c["scale"], c["seed"], c["sweep"], c["orientation"])
    assert want["margin_gamma"] > 1e-9
    assert got["count"] == 0 and got["aux_tables"] == 0 and got["nonempty"] == 0 and not got["m"].any()
    assert abs(got["s"] - want["s"]) <= 1e-10 * want["s"]


# ---- 7. the example ----

EXE = os.path.join(ROOT, "examples", "bin", "pyp_resample")
ARGS = ["-J", "8", "-n", "400", "-c", "6", "-s", "5", "-d", "-z", "-L", "-w", "-C"]


@pytest.mark.parametrize("extra", [[], ["-H", "4"]])
def test_example_with_drawn_concentrations(extra):
    assert os.path.exists(EXE), "examples/bin/pyp_resample not built (make -C libstb_amd/csrc)"
    p = subprocess.run([EXE] + ARGS + ["-K"] + extra, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    beta = re.findall(r"^iteration (\d+): beta (\S+) from (\d+) customers, (\d+) auxiliary$", p.stdout, re.M)
    assert [int(r[0]) for r in beta] == list(range(6)), p.stdout
    for _, b, n, aux in beta:
        assert math.isfinite(float(b)) and float(b) > 0 and int(n) >= int(aux) > 0
    gamma = re.findall(r"^iteration (\d+): gamma (\S+) from (\d+) tables, (\d+) auxiliary$", p.stdout, re.M)
    if extra:
        assert not gamma                                          # under -H the base weights have a root: its gamma stays
    else:
        assert [int(r[0]) for r in gamma] == list(range(6)), p.stdout
        assert all(math.isfinite(float(g)) and float(g) > 0 for _, g, _, _ in gamma)
    joint = re.findall(r"^iteration \d+: collapsed log joint (\S+) ", p.stdout, re.M)
    assert len(joint) == 6 and all(math.isfinite(float(x)) for x in joint), p.stdout
    # without -K no such line; -K without -d -z -w is refused
    q = subprocess.run([EXE] + ARGS + extra, capture_output=True, text=True, timeout=60)
    assert q.returncode == 0 and not re.search(r": (beta|gamma) \S+ from", q.stdout)
    assert subprocess.run([EXE, "-d", "-z", "-K"], capture_output=True, text=True, timeout=60).returncode == 2
