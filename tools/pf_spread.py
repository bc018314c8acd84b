"""What resampling buys: the spread of the held-out estimate of log p(document) over independent runs, with and without
resampling, from the numpy replay of the particle filter (tests/pf_oracle.py -- the device returns the same weights bit
for bit).  Runs on the CPU.

  python tools/pf_spread.py [--lengths 50,200,800] [--runs 64] [--particles 16] [--model flat|topics] [--out FILE]

One document of N customers (1000 classes at random), K = 20 dishes, an empty restaurant, a = 0.3, b = 2, h = 1 / K, a
random likelihood matrix 0.05 + U(0, 1) and classes at random (--model flat: tools/time_seat.py's model, in which no dish
explains a class much better than another); or (--model topics) every dish a sharp distribution over the classes
(Dirichlet(0.05), times the number of classes) and the document drawn from three of the dishes (weights 0.6, 0.3, 0.1):
a particle that has opened the right dishes early outweighs one that has not.  The `runs` replicates are `runs` copies of the document in one call: copy i's
customers have their own indices, so their own uniforms.  For every N: mean, standard deviation, minimum and maximum of
the estimate H over the runs at tau = 0 (the sequential method) and tau = 0.5, the resamplings a document, and the
reference: log of the mean over the runs of exp(H) at 64 particles and tau = 0.5 (the estimate of p is unbiased, so this
is the log of an average of runs x 64 particles' worth), with its own spread beside it.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pf_oracle as pf  # noqa: E402


def lme(H):
    m = H.max()
    return float(m + np.log(np.mean(np.exp(H - m))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default="50,200,800")
    ap.add_argument("--runs", type=int, default=64)
    ap.add_argument("--particles", type=int, default=16)
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
        I = args.runs
        Ks = np.full(I, K, dtype=np.int32)
        n, t, h = np.zeros(I * K, dtype=np.uint32), np.zeros(I * K, dtype=np.uint16), np.full(I * K, 1.0 / K)
        coff = (np.arange(I + 1) * N).astype(np.uint64)
        cls = np.tile(doc, I)
        row = {"model": args.model, "customers": N, "dishes": K, "runs": I, "particles": args.particles}
        for R, tau, name in ((64, 0.5, "ref"), (args.particles, 0.0, "tau0"), (args.particles, 0.5, "tau0.5")):
            rp = pf.replay(Ks, n, t, h, a, np.full(I, b), coff, cls, lik, 0, 7, 0, R, tau)
            H = rp["H"]
            row[name] = {"mean": float(H.mean()), "std": float(H.std(ddof=1)), "min": float(H.min()), "max": float(H.max()),
                         "log_mean_exp": lme(H), "resamplings_per_document": float(rp["res"].mean())}
            print(N, name, json.dumps(row[name]), flush=True)
        out.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
