"""The device samplers against the long-double laws of tests/hs_oracle.py at the shapes where the kernels change behaviour
(tests/hs_cases.py): k_tcounts on every chunk boundary, either side of its LDS cap, truncated, at every workgroup size and
at the edges of (a, b, h, T_); k_tcwin either side of its one-chunk switch with the span clipped at 1 and at Mt;
k_partition with L on its chunk boundaries.  Every draw must equal the truth's: tests/test_samplers_truth_host.py shows
that no draw of these cases lies within the kernels' rounding of a boundary.  k_tindic_wave is replayed by
tests/ti_oracle.py on rows longer than its 64-cell window."""
import contextlib
import os

import numpy as np
import pytest

import hs_cases as hc
import ti_oracle as tio
from libstb_amd import capi

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def env(name, value):
    """the variable set to value, or unset (value None: the library's default) for the block"""
    old = os.environ.get(name)
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = str(value)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


def explain(c, before, got, want, what):
    """the first differing pair: its n, t, T_, the two draws, and how the kernel ran"""
    g = int(np.flatnonzero(got != want)[0])
    koff = np.concatenate([[0], np.cumsum(c.K)])
    i = int(np.searchsorted(koff, g, side="right")) - 1
    Tm = int(want[koff[i]:g].astype(np.int64).sum() + before[g + 1:koff[i + 1]].astype(np.int64).sum())
    return (f"{c.name} [{what}]: pair {g} of restaurant {i}: n={int(c.n[g])} t={int(before[g])} T_={Tm} M={c.M} a={c.a} "
            f"b={c.bpar[i]} h={None if c.h is None else c.h[g]}: device tau={int(got[g])}, truth tau={int(want[g])}; "
            f"{int(np.count_nonzero(got != want))} pairs differ")


def check_state(c, before, got_t, got_T, want, what):
    assert np.array_equal(got_t, want[0]), explain(c, before, got_t, want[0], what)
    assert np.array_equal(got_T, want[1]), (c.name, what, got_T, want[1])


# ---- k_tcounts ----

def tc_object(c, one_launch, what):
    truth = hc.tc_truth(c)[0]
    tc = capi.TableCounts(c.K, c.n, c.t, c.h, c.M)
    try:
        if one_launch:
            tc.sweep(c.a, c.bpar, c.seed, 0, c.sweeps)
            # (the first sweep's draws already differ if anything does: report against the last state of the truth)
            check_state(c, truth[-2][0] if c.sweeps > 1 else c.t, *tc.get(), truth[-1], what + f", nsweeps={c.sweeps}")
        else:
            before = c.t
            for s in range(c.sweeps):
                tc.sweep(c.a, c.bpar, c.seed, s)
                check_state(c, before, *tc.get(), truth[s], what + f", sweep {s}")
                before = truth[s][0]
    finally:
        tc.free()


@pytest.mark.parametrize("one_launch", [False, True])
def test_tcounts_boundary_rows(one_launch):
    tc_object(hc.tc_boundary(), one_launch, "threads=256")


@pytest.mark.parametrize("threads", hc.TC_THREADS)
def test_tcounts_boundary_rows_at_every_workgroup_size(threads):
    with env("STB_TCOUNTS_THREADS", threads):
        tc_object(hc.tc_boundary(), False, f"threads={threads}")
        tc_object(hc.tc_boundary(), True, f"threads={threads}")


def tc_raw(c):
    """the case through stb_sample_tcounts on a table of the case's bounds (N, M): the raw entry's own tau_max = min(N, M)"""
    import torch

    truth = hc.tc_truth(c)[0]
    tabs = capi.DeviceTables(c.N, c.M)
    tabs.fill(c.a)
    tabs.status()
    dev = "cuda"
    koff = torch.as_tensor(np.concatenate([[0], np.cumsum(c.K)]).astype(np.int64), device=dev)
    d_n = torch.as_tensor(c.n.view(np.int32), device=dev)
    d_t = torch.as_tensor(c.t.view(np.int16), device=dev).clone()
    T0 = np.add.reduceat(c.t.astype(np.int64), np.concatenate([[0], np.cumsum(c.K)[:-1]])).astype(np.uint32)
    d_T = torch.as_tensor(T0.view(np.int32), device=dev).clone()
    d_b = torch.as_tensor(c.bpar, device=dev)
    d_h = torch.as_tensor(c.h, device=dev)
    before = c.t
    for s in range(c.sweeps):
        capi.check(capi.lib().stb_sample_tcounts(tabs.tables.data_ptr(), tabs.S1.data_ptr(), c.N, c.M, c.a, d_b.data_ptr(),
                                                 len(c.K), koff.data_ptr(), d_n.data_ptr(), d_t.data_ptr(), d_T.data_ptr(),
                                                 d_h.data_ptr(), c.seed, s, capi.stream_ptr()))
        torch.cuda.synchronize()
        check_state(c, before, d_t.cpu().numpy().view(np.uint16), d_T.cpu().numpy().view(np.uint32), truth[s],
                    f"raw call, sweep {s}")
        before = truth[s][0]


def test_tcounts_boundary_rows_raw_call():
    tc_raw(hc.tc_boundary())


@pytest.mark.parametrize("M", hc.TC_TRUNC_M)
def test_tcounts_truncated_raw_call(M):
    tc_raw(hc.tc_trunc(M))


@pytest.mark.parametrize("a", [0.0, 0.999])
def test_tcounts_parameter_edges_raw_call(a):
    tc_raw(hc.tc_params(a, True))


@pytest.mark.parametrize("M", hc.TC_TRUNC_M)
def test_tcounts_truncated(M):
    tc_object(hc.tc_trunc(M), False, "threads=256")
    tc_object(hc.tc_trunc(M), True, "threads=256")


@pytest.mark.parametrize("with_h", [True, False])
@pytest.mark.parametrize("a", hc.A_SET)
def test_tcounts_parameter_edges(a, with_h):
    tc_object(hc.tc_params(a, with_h), False, "threads=256")


@pytest.mark.parametrize("threads", [64, 256])
def test_tcounts_large_T(threads):
    with env("STB_TCOUNTS_THREADS", threads):
        tc_object(hc.tc_big_T(), False, f"threads={threads}")


# ---- k_tcwin ----

def tcw_object(c, what):
    truth = hc.tcw_truth(c)[0]
    tc = capi.TableCounts(c.K, c.n, c.t, c.h, c.M)
    try:
        before = c.t
        for s in range(c.sweeps):
            tc.sweep_window(c.a, c.bpar, c.W, c.seed, s, ref=c.ref)
            check_state(c, before, *tc.get(), truth[s], f"{what}, W={c.W}, ref={c.ref}, sweep {s}")
            before = truth[s][0]
    finally:
        tc.free()


@pytest.mark.parametrize("waves", [None, 1, 8])
@pytest.mark.parametrize("ref", [False, True])
@pytest.mark.parametrize("W", hc.TCW_W)
def test_tcwin_either_side_of_the_one_chunk_switch(W, ref, waves):
    with env("STB_TCWIN_WAVES", waves):
        tcw_object(hc.tcw_main(W, ref), f"waves={waves or 4}")
        tcw_object(hc.tcw_trunc(W, ref), f"waves={waves or 4}")


@pytest.mark.parametrize("b", hc.B_SET)
@pytest.mark.parametrize("a", hc.A_SET)
def test_tcwin_parameter_edges(a, b):
    tcw_object(hc.tcw_params(a, b), "waves=4")


# ---- k_partition ----

@pytest.fixture(scope="module")
def pt_tabs():
    """the partition cases' tables, one a discount, filled on first use and released with the module"""
    tabs = {}

    def get(a):
        if a not in tabs:
            tabs[a] = capi.DeviceTables(hc.PT_N, hc.PT_M)
            tabs[a].fill(a)
            tabs[a].status()
        return tabs[a]

    yield get
    tabs.clear()


@pytest.mark.parametrize("waves", [None, 1, 8])
@pytest.mark.parametrize("S", hc.PT_S)
@pytest.mark.parametrize("a", hc.A_SET)
def test_partition_on_chunk_boundaries(pt_tabs, a, S, waves):
    import torch

    n, t = hc.pt_pairs()
    want_cnt, want_sz, _ = hc.pt_truth(a, S)
    soff = np.concatenate([[0], np.cumsum(t.astype(np.int64))]).astype(np.int64)
    d_n = torch.as_tensor(n.view(np.int32), device="cuda")
    d_t = torch.as_tensor(t.view(np.int16), device="cuda")
    d_soff = torch.as_tensor(soff, device="cuda")
    d_sz = torch.full((int(soff[-1]),), -1, dtype=torch.int16, device="cuda")
    with env("STB_PARTITION_WAVES", waves):
        cnt = capi.sample_partition(pt_tabs(a), a, d_n, d_t, S, hc.PT_SEED[a], 0, sizes=d_sz, soff=d_soff)
    torch.cuda.synchronize()
    cnt = cnt.cpu().numpy().view(np.uint32).astype(np.int64)
    sz = d_sz.cpu().numpy().view(np.uint16)
    for g in range(len(n)):
        got = [int(x) for x in sz[soff[g]:soff[g + 1]]]
        if want_sz[g] is None:
            assert all(x == 0xFFFF for x in got), (g, int(n[g]), int(t[g]))
            continue
        if got != want_sz[g]:
            r = next(j for j in range(len(got)) if got[j] != want_sz[g][j])
            Nr = int(n[g]) - sum(want_sz[g][:r])
            raise AssertionError(f"pair {g}: n={int(n[g])} t={int(t[g])} a={a} S={S} waves={waves or 4}: round {r} with "
                                 f"N={Nr}, M={int(t[g]) - 1 - r}, L={Nr - (int(t[g]) - 1 - r)}: device l={got[r]}, "
                                 f"truth l={want_sz[g][r]}")
    assert np.array_equal(cnt, want_cnt), np.flatnonzero(cnt != want_cnt)[:10]


# ---- k_tindic_wave (and the lane form) on rows longer than the wave's 64-cell window ----

def ti_state():
    """rows up to 300 with t starting at 1 and at n: the window has to move over the whole row"""
    rng = np.random.default_rng(8)
    n = np.array([300, 300, 129, 65, 64, 200, 1, 0, 300, 70, 257, 2], dtype=np.uint32)
    t = np.array([1, 300, 129, 1, 64, 1, 1, 0, 150, 70, 1, 2], dtype=np.uint16)
    K = np.array([4, 4, 4], dtype=np.int32)
    h = 0.05 + 1.95 * rng.random(len(n))
    return K, n, t, h, np.array([0.5, 3.0, 50.0])


def shuffled_order(rng, K, n):
    out, g = [], 0
    for Ki in K:
        seq = np.repeat(np.arange(Ki, dtype=np.uint32), n[g:g + Ki].astype(np.int64))
        rng.shuffle(seq)
        out.append(seq)
        g += Ki
    return np.concatenate(out).astype(np.uint32)


_ti_want = {}


def ti_truth(order, a, vt, N, seed, sweeps):
    if order not in _ti_want:
        K, n, t, h, bpar = ti_state()
        cust = shuffled_order(np.random.default_rng(9), K, n) if order == "shuffled" else None
        out = []
        for s in range(sweeps):
            t, T = tio.sweep(K, n, t, h, a, bpar, vt, N, seed, s, cust)
            out.append((t, T))
        _ti_want[order] = (cust, out)
    return _ti_want[order]


@pytest.mark.parametrize("form", ["wave", "lane"])
@pytest.mark.parametrize("order", ["pair", "shuffled"])
def test_tindic_forms_on_long_rows(monkeypatch, order, form):
    a, seed, sweeps = 0.6, 41, 3
    K, n, t, h, bpar = ti_state()
    v = capi.DeviceVTables(300, 300)
    v.fill(a)
    capi.check(capi.lib().stb_fill_status())
    cust, want = ti_truth(order, a, tio.VTab(v.packed_host(0), 300, 300), 300, seed, sweeps)
    monkeypatch.setenv("STB_TINDIC_FORM", form)
    ti = capi.TableIndicators(K, n, t, h, cust, 0, 0)
    try:
        for s in range(sweeps):
            ti.sweep(a, bpar, seed, s)
            got_t, got_T = ti.get()
            assert np.array_equal(got_t, want[s][0]), (form, order, s, np.flatnonzero(got_t != want[s][0])[:10])
            assert np.array_equal(got_T, want[s][1])
        assert not np.array_equal(want[-1][0], t)
    finally:
        ti.free()
