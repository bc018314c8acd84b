"""What temperatures buy: the spread of the held-out estimate of log p(document) over independent runs, for annealed
importance sampling against the particle filter at equal total visits, from the numpy replays (tests/ais_oracle.py,
tests/pf_oracle.py -- the device walks the same paths bit for bit).  Runs on the CPU.

  python tools/ais_spread.py [--lengths 50,200] [--runs 32] [--particles 16] [--temps 8] [--model flat|topics] [--out FILE]

tools/pf_spread.py's experiment: one document of N customers (1000 classes), K = 20 dishes, an empty restaurant, a = 0.3,
b = 2, h = 1 / K; --model flat or topics as there.  `runs` copies of the document in one call, each with its own indices,
so its own uniforms.  A particle filter of R particles visits every customer R times; a ladder of S temperatures and one
pass visits it S times a particle (the seating and S - 1 sweeps): AIS with R_a = max(1, R / S) particles and S
temperatures is set against the filter with R particles -- equal visits -- and AIS with R particles and S temperatures
against nothing (S times the visits; shown for the trend).  For every N: mean, standard deviation, minimum and maximum of
the estimate H over the runs, and the reference as in pf_spread.py (64 particles, tau = 0.5, log-mean-exp over the runs).
The dish sweep's V cells are the exact Stirling ratios (tests/ti_oracle.ExactV), which reach N = 150 in doubles at
a = 0.3; longer documents need the device's table.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ais_oracle as ao  # noqa: E402
import pf_oracle as pf  # noqa: E402
import st_oracle as sto  # noqa: E402
import ti_oracle as tio  # noqa: E402
from pf_spread import lme  # noqa: E402


def summary(H):
    return {"mean": float(H.mean()), "std": float(H.std(ddof=1)), "min": float(H.min()), "max": float(H.max()), "log_mean_exp": lme(H)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default="50,150")
    ap.add_argument("--runs", type=int, default=32)
    ap.add_argument("--particles", type=int, default=16)
    ap.add_argument("--temps", type=int, default=8)
    ap.add_argument("--model", default="flat", choices=("flat", "topics"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    K, rows, a, b = 20, 1000, 0.3, 2.0
    rng = np.random.default_rng(17)
    if args.model == "flat":
        lik = 0.05 + rng.random((rows, K))
    else:
        lik = np.maximum(rng.dirichlet(np.full(rows, 0.05), K).T * rows, 1e-6)
    out = []
    for N in (int(x) for x in args.lengths.split(",")):
        if args.model == "flat":
            doc = rng.integers(0, rows, size=N).astype(np.uint32)
        else:
            z = rng.choice([3, 11, 17], size=N, p=[0.6, 0.3, 0.1])
            phi = lik / lik.sum(axis=0)
            doc = np.array([rng.choice(rows, p=phi[:, k]) for k in z], dtype=np.uint32)
        I, R, S = args.runs, args.particles, args.temps
        Ks = np.full(I, K, dtype=np.int32)
        n, t, h = np.zeros(I * K, dtype=np.uint32), np.zeros(I * K, dtype=np.uint16), np.full(I * K, 1.0 / K)
        coff = (np.arange(I + 1) * N).astype(np.uint64)
        cls = np.tile(doc, I)
        bpar = np.full(I, b)
        vt = tio.ExactV(list(range(1, max(N, 3) + 1)), a)
        row = {"model": args.model, "customers": N, "dishes": K, "runs": I, "particles": R, "temperatures": S}
        for Rp, tau, name in ((64, 0.5, "ref"), (R, 0.5, "pf_tau0.5")):
            H = pf.replay(Ks, n, t, h, a, bpar, coff, cls, lik, 0, 7, 0, Rp, tau)["H"]
            row[name] = summary(H)
            print(N, name, json.dumps(row[name]), flush=True)
        for Ra, name in ((max(1, R // S), "ais_equal_visits"), (R, "ais_same_particles")):
            rp = ao.replay(Ks, h, a, bpar, coff, cls, lik, ao.numpy_tempered(lik, S), vt, max(N, 3), max(N, 3), 7, 0, Ra, S)
            H = sto.loglik_replay(rp["lw"])[0]
            row[name] = dict(summary(H), particles=Ra, dead=rp["dead"])
            print(N, name, json.dumps(row[name]), flush=True)
        out.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
