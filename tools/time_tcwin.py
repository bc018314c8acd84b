"""Time the windowed table-count sweep (stb_sample_tcounts_window, libstb_amd/csrc/tcwin.hip) at W = 1, 10, 30 against
the full sweep (stb_sample_tcounts) on the shapes of MEASUREMENTS.md section T1, in one run, alternating them; and a
single-core C restatement of the exact windowed sweep on the host (tools/tcwin_host.c).

  python tools/time_tcwin.py [--sweeps 20] [--shapes A-realistic,B] [--windows 1,10,30] [--out FILE]

Shapes from synth.groups: A = 1000 restaurants x 1000 pairs, n_max 4000 ("realistic"); B = 10^6 restaurants x 1 pair.
a = 0.5, h = 1, table M = N = max n, filled once.  Every variant sweeps its own copy of the state.  One warm-up sweep of
each, then `--sweeps` rounds of one sweep of each variant in turn, each between device events: median (min, max).
Span cells = sum over pairs of the span lo(t-W) .. hi(t+W) a visit reads (at the timed state's start).  The host sweeps a
slice of the restaurants once at the middle window, from the state the device's warm-up sweep starts from, and is scaled
by pairs; its draws are checked against the device's on that slice, and it counts the proposals that move t and the
share of them accepted.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libstb_amd import capi, synth  # noqa: E402

SHAPES = {"A-realistic": (1000, 1000, "realistic"), "B": (1000000, 1, "realistic")}


def host_lib():
    src = os.path.join(ROOT, "tools", "tcwin_host.c")
    out = os.path.join(ROOT, "tools", "build", "libtcwin_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, src, "-lm"], check=True)
    L = C.CDLL(out)
    vp, d, u, u64 = C.c_void_p, C.c_double, C.c_uint, C.c_uint64
    L.tcw_host_sweep.restype = d
    L.tcw_host_sweep.argtypes = [vp, vp, u, d, vp, C.c_int, C.c_int, vp, vp, vp, vp, u, u, u64, u64, vp]
    return L


def span_cells(n, t, M, W):
    Mt = np.minimum(n.astype(np.int64), M)
    tc = np.clip(t.astype(np.int64), 1, np.maximum(Mt, 1))
    lo, hi = np.maximum(1, tc - 2 * W), np.minimum(Mt, tc + 2 * W)
    return int(np.where(Mt >= 2, hi - lo + 1, 0).sum())


def run(name, sweeps, windows, a=0.5, seed=2025):
    import torch

    I, K, prof = SHAPES[name]
    g = synth.groups(I, K, 4000, prof)
    N = M = int(g.n.max())
    L = capi.lib()
    tabs = capi.DeviceTables(N, M)
    tabs.fill(a)
    tabs.status()
    koff_h = np.concatenate([[0], np.cumsum(g.K)]).astype(np.uint64)
    koff = torch.as_tensor(koff_h.view(np.int64), device="cuda")
    d_n = torch.as_tensor(g.n.view(np.int32), device="cuda")
    d_b = torch.as_tensor(g.bpar, device="cuda")
    variants = [("window", W) for W in windows] + [("full", 0)]
    state = {v: (torch.as_tensor(g.t.view(np.int16), device="cuda").clone(),
                 torch.as_tensor(g.T.view(np.int32), device="cuda").clone()) for v in variants}

    def sweep(v, s):
        d_t, d_T = state[v]
        if v[0] == "full":
            capi.check(L.stb_sample_tcounts(tabs.tables.data_ptr(), tabs.S1.data_ptr(), N, M, a, d_b.data_ptr(), I,
                                            koff.data_ptr(), d_n.data_ptr(), d_t.data_ptr(), d_T.data_ptr(), None, seed, s,
                                            capi.stream_ptr()))
        else:
            capi.check(L.stb_sample_tcounts_window(tabs.tables.data_ptr(), tabs.S1.data_ptr(), N, M, a, d_b.data_ptr(), I,
                                                   koff.data_ptr(), d_n.data_ptr(), d_t.data_ptr(), d_T.data_ptr(), None,
                                                   v[1], 0, seed, s, capi.stream_ptr()))

    for v in variants:
        sweep(v, 0)
    torch.cuda.synchronize()
    Wh = windows[len(windows) // 2]
    nslice = max(1, I // 50)
    G0 = int(koff_h[nslice])
    t_dev0 = state[("window", Wh)][0].cpu().numpy().view(np.uint16)[:G0].copy()
    t_start = {v: state[v][0].cpu().numpy().view(np.uint16).copy() for v in variants}
    ms = {v: [] for v in variants}
    for s in range(1, sweeps + 1):
        for v in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            sweep(v, s)
            e1.record()
            e1.synchronize()
            ms[v].append(e0.elapsed_time(e1))
    out = []
    for v in variants:
        med = float(np.median(ms[v]))
        r = {"shape": name, "I": I, "K": K, "G": g.pairs, "N": N, "M": M, "a": a, "kind": v[0], "W": v[1],
             "ms_median": med, "ms_min": float(min(ms[v])), "ms_max": float(max(ms[v])), "sweeps_timed": sweeps,
             "us_per_pair_step": med * 1e3 / K, "waves": int(os.environ.get("STB_TCWIN_WAVES", "4"))}
        if v[0] == "window":
            cells = span_cells(g.n, t_start[v], M, v[1])
            r.update({"span_cells": cells, "bound_span_8B_ms": cells * 8 / 8.0e12 * 1e3})
        else:
            r.update({"weights": int(np.minimum(g.n.astype(np.int64), M).sum())})
        out.append(r)
    # host: one core, the exact windowed sweep at W = Wh over the first restaurants, from the warm-up sweep's state
    H = host_lib()
    S1 = tabs.S1[0].cpu().numpy().copy()
    tab = tabs.packed_host(0)
    t_host, T_host = g.t.copy(), g.T.copy()
    moves = np.zeros(2, dtype=np.uint64)
    sec = H.tcw_host_sweep(S1.ctypes.data, tab.ctypes.data, M, a, g.bpar.ctypes.data, 0, nslice, koff_h.ctypes.data,
                           g.n.ctypes.data, t_host.ctypes.data, T_host.ctypes.data, Wh, 0, seed, 0, moves.ctypes.data)
    out.append({"shape": name, "kind": "host", "W": Wh, "host_slice_restaurants": nslice, "host_slice_pairs": G0,
                "host_slice_s": sec, "host_ms_scaled": sec * 1e3 * g.pairs / G0,
                "host_same_draws_on_slice": int(np.sum(t_host[:G0] == t_dev0)),
                "proposals_moving_t": int(moves[0]), "accepted_share": float(moves[1]) / max(1, int(moves[0]))})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--shapes", default="A-realistic,B")
    ap.add_argument("--windows", default="1,10,30")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert capi.lib().stb_device_count() > 0, "no GPU: " + capi.last_error()
    windows = [int(w) for w in args.windows.split(",")]
    out = []
    for s in args.shapes.split(","):
        for r in run(s, args.sweeps, windows):
            print(json.dumps(r), flush=True)
            out.append(r)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
