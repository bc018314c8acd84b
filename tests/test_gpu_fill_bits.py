"""The bytes a table fill and a fused evaluation leave, on every route of the fill's plan and in every strip shape of the
halo-block spine, against a recording of an earlier commit's library (tests/golden/fill_bits.json names it;
tools/record_fill_bits.py): a refactor of the fill's plan or of the spine's kernels leaves every one of them as it was.

Fill cases: a SHA-256 of the slab's stored cells (row padding left out) and of the S1 vectors where the fill writes
them; each at the smallest bounds at which its route exists -- for the spine, at which a table has more than one spine
workgroup, so that records travel between workgroups through the fetcher wave.  Fused cases: the doubles stb_groups_aterms returns for 2000
synthetic pairs.  A fused case that the recorded commit itself did not reproduce from run to run is marked in the
recording ("exact": false) and compared at the evaluations' usual 1e-10 instead."""
import contextlib
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from libstb_amd import capi, synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fill_bits.json")

# name -> (entry point, N, M, D, variant (stb_fill_S only), environment, shared-GPU mode)
FILLS = {
    "chain D=1": ("S", 64, 64, 1, capi.FILL_SCALED, {}, -1),
    "chain D=3": ("S", 64, 64, 3, capi.FILL_SCALED, {}, -1),
    "chain D=65 (discounts by copy)": ("S", 64, 64, 65, capi.FILL_SCALED, {}, -1),
    "hb S": ("S", 512, 512, 1, capi.FILL_SCALED, {}, -1),
    "hb Sf": ("Sf", 512, 512, 1, None, {}, -1),
    "hb V": ("V", 512, 512, 1, None, {}, -1),
    "hb Vf": ("Vf", 512, 512, 1, None, {}, -1),
    "hb S 600x200 D=2": ("S", 600, 200, 2, capi.FILL_SCALED, {}, -1),
    "hb S STB_A_BY_VALUE=0": ("S", 512, 512, 1, capi.FILL_SCALED, {"STB_A_BY_VALUE": "0"}, -1),
    "V exact 600": ("Vx", 600, 600, 1, None, {}, -1),
    "V below 512 rows": ("V", 100, 100, 1, None, {}, -1),
    "pc 300 D=2": ("S", 300, 300, 2, capi.FILL_PC, {}, -1),
    "rows-log 100": ("S", 100, 100, 1, capi.FILL_LOGDOMAIN, {}, -1),
    "shared S 600": ("S", 600, 600, 1, capi.FILL_SCALED, {}, 1),
    "shared V 600": ("V", 600, 600, 1, None, {}, 1),
    # the halo-block spine across workgroups (the fetcher at work): the smallest shapes with more than one spine workgroup a
    # table, in every strip shape and output kind
    "hb S C=4 P=2": ("S", 512, 512, 1, capi.FILL_SCALED, {"STB_HB_C": "4", "STB_HB_P": "2"}, -1),  # 3 strips, 2 workgroups
    "hb Sf C=4 P=2": ("Sf", 512, 512, 1, None, {"STB_HB_C": "4", "STB_HB_P": "2"}, -1),  # the 16-byte float row
    "hb V C=4 P=2": ("V", 512, 512, 1, None, {"STB_HB_C": "4", "STB_HB_P": "2"}, -1),  # the extra halo lane
    "hb Vf C=4 P=2": ("Vf", 512, 512, 1, None, {"STB_HB_C": "4", "STB_HB_P": "2"}, -1),
    "hb S C=1 rows=16 P=3": ("S", 512, 512, 1, capi.FILL_SCALED, {"STB_HB_C": "1", "STB_HB_ROWS": "16", "STB_HB_P": "3"}, -1),  # 11 strips, 4 workgroups
    "hb S C=2 rows=24": ("S", 512, 512, 1, capi.FILL_SCALED, {"STB_HB_C": "2", "STB_HB_ROWS": "24"}, -1),  # blocks not 48 rows in line; 5 strips
    "hb S C=2 P=7 700x700": ("S", 700, 700, 1, capi.FILL_SCALED, {"STB_HB_C": "2", "STB_HB_P": "7"}, -1),  # 9 strips, 2 workgroups of 7
    "hb S split=0": ("S", 512, 512, 1, capi.FILL_SCALED, {"STB_HB_SPLIT": "0"}, -1),  # no quartered last tiles
    "hb S 600x200 D=3 C=4 P=2": ("S", 600, 200, 3, capi.FILL_SCALED, {"STB_HB_C": "4", "STB_HB_P": "2"}, -1),
}
# name -> (bound N = M, D, environment, the form it takes: [fused, list layout -- 0 chain, 2 halo blocks, 3 and up grid])
# (without STB_ATERMS_HB=0 an evaluation takes the halo-block sum at 300 rows too: the chain form's sum, which goes
# through the fill's plan with the evaluation's request, is the last case)
FUSED = {
    "300 D=1 (halo-block sum)": (300, 1, {}, [1, 2]),
    "300 D=2 (halo-block sum)": (300, 2, {}, [1, 2]),
    "600 D=2 (halo-block sum)": (600, 2, {}, [1, 2]),
    "600 D=32 STB_ATERMS_GRID=1 (grid)": (600, 32, {"STB_ATERMS_GRID": "1"}, [1, 3]),
    "300 D=1 STB_ATERMS_HB=0 (stored tables)": (300, 1, {"STB_ATERMS_HB": "0"}, [0, 0]),
    "300 D=2 STB_ATERMS_HB=0 (chain sum)": (300, 2, {"STB_ATERMS_HB": "0"}, [1, 0]),
    # more than one spine workgroup a table: the summing fill's and the grid walk's fetchers
    "600 D=2 STB_HB_DOT_C=3": (600, 2, {"STB_HB_DOT_C": "3"}, [1, 2]),  # 5 strips, 2 workgroups
    "600 D=2 STB_HB_DOT_C=4 STB_HB_DOT_P=2": (600, 2, {"STB_HB_DOT_C": "4", "STB_HB_DOT_P": "2"}, [1, 2]),
    "600 D=32 grid C=4 P=2": (600, 32, {"STB_ATERMS_GRID": "1", "STB_GRID_C": "4", "STB_GRID_P": "2"}, [1, 4]),
    "600 D=32 grid C=8 P=1": (600, 32, {"STB_ATERMS_GRID": "1", "STB_GRID_C": "8", "STB_GRID_P": "1"}, [1, 5]),
    "600 D=32 grid C=4 jobs": (600, 32, {"STB_ATERMS_GRID": "1", "STB_GRID_C": "4", "STB_GRID_HELP_NW": "1"}, [1, 4]),  # (tests/hp_pairs.py's grid4jobs)
}


@contextlib.contextmanager
def setting(env, mode=-1):
    L = capi.lib()
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    L.stb_set_shared_gpu(mode)
    try:
        yield L
    finally:
        L.stb_set_shared_gpu(-1)
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def discounts(D):
    return np.array([0.5]) if D == 1 else np.ascontiguousarray(synth.discount_grid(max(D, 64))[:D])


def stored_cells(L, vtable, N, M):
    """element offsets of the stored cells in a slab, row after row"""
    if vtable:
        rows = [(int(L.stb_vrowoff(n, M)), min(n - 1, M - 1)) for n in range(2, N + 1)]
    else:
        rows = [(int(L.stb_rowoff(n, M)), min(n - 2, M - 1)) for n in range(3, N + 1)]
    return np.concatenate([np.arange(o, o + ln, dtype=np.int64) for o, ln in rows])


def sha(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def fill_bits(name):
    entry, N, M, D, variant, env, mode = FILLS[name]
    torch = capi._torch()
    vtable, floats = entry[0] == "V", entry.endswith("f")
    with setting(env, mode) as L:
        elems = int(L.stb_velems(N, M) if vtable else L.stb_elems(N, M))
        stride = max(32, (elems + 31) // 32 * 32)
        slab = torch.zeros((D, stride), dtype=torch.float32 if floats else torch.float64, device="cuda")
        S1 = torch.zeros((D, N), dtype=torch.float64, device="cuda")
        wsb = int(L.stb_fill_workspace_bytes(N, M, D))
        ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda")
        a, st = discounts(D), capi.stream_ptr()
        head = [capi.dp(a), D, N, M, slab.data_ptr(), stride]
        if entry == "S":
            rc = L.stb_fill_S(*head, S1.data_ptr(), N, ws.data_ptr(), wsb, variant, st)
        elif entry == "Sf":
            rc = L.stb_fill_Sf(*head, S1.data_ptr(), N, ws.data_ptr(), wsb, st)
        else:
            rc = {"V": L.stb_fill_V, "Vf": L.stb_fill_Vf, "Vx": L.stb_fill_V_exact}[entry](*head, ws.data_ptr(), wsb, st)
        capi.check(rc)
        capi.check(L.stb_fill_status())
        torch.cuda.synchronize()
        out = {"slab": sha(slab.cpu().numpy()[:, stored_cells(L, vtable, N, M)])}
        if not vtable:
            out["S1"] = sha(S1.cpu().numpy())
    return out


def fused_values(name):
    N, D, env, _ = FUSED[name]
    g = synth.groups(20, 100, N, "wide")
    u32p, u16p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint16), C.POINTER(C.c_int32)
    with setting(env) as L:
        h = L.stb_groups_create(g.I, g.K.ctypes.data_as(i32p), g.T.ctypes.data_as(u32p), g.n.ctypes.data_as(u32p), g.t.ctypes.data_as(u16p),
                                capi.dp(g.bpar), N, N, D)
        assert h, capi.last_error()
        try:
            x, out = discounts(D), np.zeros(D)
            capi.check(L.stb_groups_aterms(h, capi.dp(x), D, capi.dp(out)))
            form = [C.c_int(), C.c_int()]  # (fused, which list layout: 0 chain, 1 checkpointed, 2 halo blocks, 3 and up grid)
            capi.check(L.stb_groups_last_form(h, C.byref(form[0]), C.byref(form[1]), None, None, None))
        finally:
            L.stb_groups_free(h)
    return out, [q.value for q in form]


def hexes(v):
    return [float(x).hex() for x in v]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_recording_holds_every_case(golden):
    assert sorted(golden["fill"]) == sorted(FILLS) and sorted(golden["fused"]) == sorted(FUSED)
    assert all(golden["fused"][name]["form"] == FUSED[name][3] for name in FUSED)


@pytest.mark.parametrize("name", list(FILLS))
def test_a_fill_keeps_the_recorded_bytes(name, golden):
    assert fill_bits(name) == golden["fill"][name]


@pytest.mark.parametrize("name", list(FUSED))
def test_a_fused_evaluation_keeps_the_recorded_doubles(name, golden):
    want, (got, form) = golden["fused"][name], fused_values(name)
    assert form == want["form"]
    if want["exact"]:
        assert hexes(got) == want["hex"]
    else:
        w = np.array([float.fromhex(s) for s in want["hex"]])
        assert np.all(np.abs(got - w) <= 1e-10 * np.maximum(1.0, np.abs(w))), (got, w)
