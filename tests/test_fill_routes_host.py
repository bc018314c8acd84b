"""Which form a table fill takes, as stb_fill_tuning and stb_fill_takes_kind report it, against a recording of the
commit before the fill's choice of form became one plan (tests/golden/fill_routes.json, tools/record_fill_routes.py).

No GPU is needed: without a device the library counts an MI355X's 256 compute units, and the reports launch nothing.
Every shape is asked under every setting, one setting at a time; the environment is read at every call, so a change
made through os.environ holds for the next one."""
import contextlib
import ctypes as C
import json
import os

from libstb_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fill_routes.json")

SHAPES = [(2, 2, 1), (3, 2, 1), (100, 100, 1), (300, 300, 1), (511, 511, 1), (512, 512, 1), (512, 2, 1), (600, 600, 2),
          (1000, 1000, 64), (2000, 2000, 128), (3000, 200, 100), (4000, 4000, 8), (4000, 4000, 64), (10000, 10000, 1),
          (10000, 10000, 8), (10000, 10000, 24), (10000, 10000, 25), (10000, 10000, 32), (50000, 100, 4), (20000, 20000, 1),
          (20000, 20000, 4), (1 << 20, 64, 1), (1 << 27, 2, 1)]  # (the last one: the rows-log bound)

# name -> (environment, shared-GPU mode)
SETTINGS = {"default": ({}, -1), "shared": ({}, 1)}
SETTINGS.update({"%s=%s" % kv: (dict([kv]), -1) for kv in
                 [("STB_HB", "0"), ("STB_HB", "1"), ("STB_HB_MIN_N", "100"), ("STB_HB_MAX_SPINE", "10"), ("STB_HB_MAX_MCELLS", "1"),
                  ("STB_CHAIN_MAX_COLS", "0"), ("STB_CK", "1")] + [("STB_FILL_VARIANT", str(v)) for v in (0, 1, 5, 6, 7, 8, 9)] +
                 [("STB_FILL_R", "32")]})
SETTINGS["STB_FILL_C=4,STB_FILL_VARIANT=1"] = ({"STB_FILL_C": "4", "STB_FILL_VARIANT": "1"}, -1)

ROUTE_ENV = ("STB_HB", "STB_HB_MIN_N", "STB_HB_MAX_SPINE", "STB_HB_MAX_MCELLS", "STB_CHAIN_MAX_COLS", "STB_CK", "STB_CK_MIN_MCELLS",
             "STB_CK_MAX_MCELLS", "STB_FILL_VARIANT", "STB_FILL_R", "STB_FILL_C", "STB_PC_CONSUMERS", "STB_FILLV_EXACT",
             "STB_FILLV_CHAIN", "STB_SHARED_GPU")


@contextlib.contextmanager
def setting(env, mode):
    """the route environment cleared but for `env`, the shared-GPU mode set; both put back afterwards"""
    L = capi.lib()
    saved = {k: os.environ.pop(k) for k in ROUTE_ENV if k in os.environ}
    os.environ.update(env)
    L.stb_set_shared_gpu(mode)
    try:
        yield L
    finally:
        L.stb_set_shared_gpu(-1)
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(saved)


def report(L, N, M, D):
    """[default variant, form code, C, R, launches, takes kind 1, 2, 3]"""
    c, r, n = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    code = L.stb_fill_tuning(N, M, D, C.byref(c), C.byref(r), C.byref(n))
    return [L.stb_default_variant(), code, c.value, r.value, n.value] + [L.stb_fill_takes_kind(N, M, D, k) for k in (1, 2, 3)]


def key(shape):
    return "%d,%d,%d" % shape


def record():
    out = {}
    for name, (env, mode) in SETTINGS.items():
        with setting(env, mode) as L:
            out[name] = {key(s): report(L, *s) for s in SHAPES}
    return out


def test_the_reports_keep_the_recorded_routes():
    with open(GOLDEN) as f:
        want = json.load(f)["routes"]
    assert sorted(want) == sorted(SETTINGS) and all(sorted(want[n]) == sorted(key(s) for s in SHAPES) for n in want)
    # what the recording must hold (seen on the recorded commit)
    assert want["default"]["512,512,1"][1:] == [6, 80, 48, 1, 1, 1, 1]
    assert want["default"]["511,511,1"][1:] == [3, 128, 511, 1, 0, 0, 0]
    assert want["default"]["10000,10000,32"][1:5] == [2, 4, 128, 79]
    assert want["STB_HB=1"]["300,300,1"][1] == 6 and want["STB_HB=1"]["300,300,1"][5:] == [0, 0, 0]
    for N, M, D in SHAPES:
        if N < 1 << 27:
            assert want["shared"][key((N, M, D))][1:] == [2, 4, 128, (N - 1 + 127) // 128, 0, 0, 0]
    got = record()
    bad = [(n, k, got[n][k], want[n][k]) for n in want for k in want[n] if got[n][k] != want[n][k]]
    assert not bad, "%d of %d rows differ, first (setting, shape, got, recorded): %r" % (len(bad), len(SETTINGS) * len(SHAPES), bad[:5])
    # not in the recording: three consumer waves leave a halo of 64 columns, so the producer/consumer form advances 64
    # rows a launch -- the report says what the fill does (it used to say 128 rows and half the launches)
    with setting({"STB_PC_CONSUMERS": "3"}, 1) as L:
        for N, M, D in SHAPES:
            if N < 1 << 27:
                assert report(L, N, M, D)[1:5] == [2, 4, 64, (N - 1 + 63) // 64], (N, M, D)
    with setting({"STB_PC_CONSUMERS": "3"}, -1) as L:
        assert report(L, 10000, 10000, 32)[1:5] == [2, 4, 64, 157]
