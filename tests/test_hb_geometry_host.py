"""The strip geometry of the halo-block fill and of the grid walk, as the library reports it -- stb_fill_workspace_bytes,
stb_fill_tuning (code, C, R, launches) and stb_grid_shape (C, G, K) -- against a recording of the commit before the two
forms' host sides took their strip shape from one helper (tests/golden/hb_geometry.json, tools/record_hb_geometry.py).

No GPU is needed: without a device the library counts an MI355X's 256 compute units, and the reports launch nothing.
Every shape is asked at every number of tables under every setting, one setting at a time; the environment is read at
every call, so a change made through os.environ holds for the next one."""
import contextlib
import ctypes as C
import json
import os

from libstb_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hb_geometry.json")

SHAPES = [(3, 2), (512, 512), (512, 2), (600, 200), (900, 700), (4000, 4000), (10000, 10000), (16500, 500), (70000, 130), (1 << 19, 64)]
TABLES = (1, 2, 8, 32, 64)

SETTINGS = {"default": {}}
SETTINGS.update({"STB_HB_C=%d,STB_HB_ROWS=%d" % (c, r): {"STB_HB_C": str(c), "STB_HB_ROWS": str(r)} for c in (1, 2, 4) for r in (16, 24, 48)})
SETTINGS.update({"%s=%s" % kv: dict([kv]) for kv in [("STB_HB_P", "7"), ("STB_GRID_C", "2"), ("STB_GRID_C", "4"), ("STB_GRID_C", "8"),
                                                     ("STB_GRID_P", "2"), ("STB_FILL_P", "24")]})

# what the geometry reads, and what chooses the form that stb_fill_tuning reports: cleared but for the setting under test
GEOMETRY_ENV = ("STB_HB_C", "STB_HB_ROWS", "STB_HB_P", "STB_HB_DOT_P", "STB_HB_DOT_C", "STB_FILL_P", "STB_GRID_C", "STB_GRID_P", "STB_GRID_ROWS",
                "STB_GRID_G", "STB_GRID_K", "STB_GRID_C8_WGS", "STB_GRID_PHASES", "STB_GRID_HELP", "STB_GRID_JOB_MB", "STB_GRID_JOBS", "STB_HB",
                "STB_HB_MIN_N", "STB_HB_MAX_SPINE", "STB_HB_MAX_MCELLS", "STB_CHAIN_MAX_COLS", "STB_CK", "STB_CK_MIN_MCELLS", "STB_CK_MAX_MCELLS",
                "STB_FILL_VARIANT", "STB_FILL_R", "STB_FILL_C", "STB_PC_CONSUMERS", "STB_SHARED_GPU")


@contextlib.contextmanager
def setting(env):
    L = capi.lib()
    saved = {k: os.environ.pop(k) for k in GEOMETRY_ENV if k in os.environ}
    os.environ.update(env)
    L.stb_set_shared_gpu(-1)
    try:
        yield L
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(saved)


def report(L, N, M, D):
    """[workspace bytes, form code, C, R, launches, grid shape: status, C, G, K]"""
    c, r, n = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    code = L.stb_fill_tuning(N, M, D, C.byref(c), C.byref(r), C.byref(n))
    gc, gg, gk = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    grc = L.stb_grid_shape(N, M, D, C.byref(gc), C.byref(gg), C.byref(gk))
    return [int(L.stb_fill_workspace_bytes(N, M, D)), code, c.value, r.value, n.value, grc, gc.value, gg.value, gk.value]


def key(N, M, D):
    return "%d,%d,%d" % (N, M, D)


def record():
    out = {}
    for name, env in SETTINGS.items():
        with setting(env) as L:
            out[name] = {key(N, M, D): report(L, N, M, D) for N, M in SHAPES for D in TABLES}
    return out


def test_the_reports_keep_the_recorded_geometry():
    with open(GOLDEN) as f:
        want = json.load(f)["geometry"]
    keys = sorted(key(N, M, D) for N, M in SHAPES for D in TABLES)
    assert sorted(want) == sorted(SETTINGS) and all(sorted(want[n]) == keys for n in want)
    # what the recording must hold (seen on the recorded commit): the halo-block form at 512 rows, strips of 80 own columns
    # and blocks of 48 rows in one launch; the grid walk there with 2 columns a lane, groups of 24 rows, every 2nd staged
    assert want["default"]["512,512,1"][1:] == [6, 80, 48, 1, 0, 2, 24, 2]
    assert want["STB_GRID_C=8"]["10000,10000,64"][5:7] == [0, 8]
    assert all(row[0] > 0 for rows in want.values() for row in rows.values())
    got = record()
    bad = [(n, k, got[n][k], want[n][k]) for n in want for k in want[n] if got[n][k] != want[n][k]]
    assert not bad, "%d of %d rows differ, first (setting, shape, got, recorded): %r" % (len(bad), len(SETTINGS) * len(keys), bad[:5])
