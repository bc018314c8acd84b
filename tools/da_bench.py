#!/usr/bin/env python3
"""Timings of the slope tables (MEASUREMENTS section D1): stb_fill_dS against stb_fill_S with STB_FILL_PC,
stb_groups_aterms_grad at D = 8, stb_groups_modea against stb_groups_samplea on the same set.

    python tools/da_bench.py            runs every step as a child process under its own time limit, stops at the first failure
    python tools/da_bench.py STEP ...   one step in this process (what the children run)
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS = [("fill", "4096", "1"), ("fill", "4096", "8"), ("fill", "10000", "1"), ("fill", "10000", "8"), ("grad",), ("modea",)]
LIMIT = {"fill": 120, "grad": 120, "modea": 180}


def med(f, sync, reps=7, warm=2):
    ts = []
    for i in range(warm + reps):
        sync()
        t0 = time.perf_counter()
        f()
        sync()
        if i >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def step_fill(N, D):
    import numpy as np
    import torch
    from libstb_amd import capi

    N, D = int(N), int(D)
    a = np.linspace(0.1, 0.9, D)
    g = capi.DeviceSlopeTables(N, N, D)
    ms_da = med(lambda: g.fill(a), torch.cuda.synchronize)
    del g
    s = capi.DeviceTables(N, N, D)
    ms_pc = med(lambda: s.fill(a, variant=capi.FILL_PC), torch.cuda.synchronize)
    return dict(step="fill", N=N, D=D, fill_dS_ms=round(ms_da, 3), fill_pc_ms=round(ms_pc, 3), ratio=round(ms_da / ms_pc, 2))


def _set(Dmax):
    import orc
    from libstb_amd import capi, synth

    g = synth.groups(1000, 100, n_max=4000, profile="realistic", seed=7, bpar=10.0)
    h = capi.lib().stb_groups_create(g.I, orc.i32p(g.K), orc.u32p(g.T), orc.u32p(g.n), orc.u16p(g.t), orc.dp(g.bpar), int(g.n.max()),
                                     int(g.t.max()), Dmax)
    assert h, capi.last_error()
    return g, h


def step_grad():
    import numpy as np
    from libstb_amd import capi

    g, h = _set(8)
    x = np.linspace(0.1, 0.9, 8)
    ms = med(lambda: capi.groups_aterms_grad(h, x), lambda: None)
    out = np.zeros(8)
    ms_val = med(lambda: capi.check(capi.lib().stb_groups_aterms(h, capi.dp(x), 8, capi.dp(out))), lambda: None)
    capi.lib().stb_groups_free(h)
    return dict(step="grad", pairs=int(g.pairs), N=int(g.n.max()), M=int(g.t.max()), D=8, aterms_grad_ms=round(ms, 3), aterms_ms=round(ms_val, 3))


def step_modea():
    from libstb_amd import capi

    g, h = _set(8)
    res = {}
    ms = med(lambda: res.update(r=capi.groups_modea(h, 0.01, 0.99, 1e-8, 32)), lambda: None)
    a_hat, curv, info = res["r"]
    ms_s = med(lambda: capi.groups_samplea(h, 0.5), lambda: None)
    capi.lib().stb_groups_free(h)
    return dict(step="modea", pairs=int(g.pairs), modea_ms=round(ms, 3), samplea_ms=round(ms_s, 3), a_hat=a_hat, curv=curv,
                rounds=info.rounds, evals=info.evals)


def main():
    if len(sys.argv) > 1:
        print(json.dumps(globals()["step_" + sys.argv[1]](*sys.argv[2:])))
        return 0
    for st in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT[st[0]]), sys.executable, os.path.abspath(__file__), *st])
        if r.returncode != 0:
            print(f"step {st} failed with status {r.returncode}: stopping", file=sys.stderr)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
