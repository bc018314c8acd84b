"""A numpy replay of the class draw (include/stb_hip.h, "customers' classes drawn on the device": stb_sample_classes,
stb_tindic_sample_classes, stb_tindic_generate), written from the header's text; test infrastructure only.

  Cumulative sums of column k: rows in chunks of 256; pre_w the running sum inside a chunk in row order from the chunk's
  first row; S_j = pre at the chunk's last row; base_0 = 0, base_1 = S_0, base_{j+1} = base_j + S_j; cum_w = pre_w in chunk
  0, else base_j + pre_w; Z_k the last base (tl_oracle.chunk_sums' Z bit for bit).
  The draw: u = element 3C + 1 + c of the stream of ti_oracle.sweep_key(seed, sweep); thr = u Z_k; w* the smallest w with
  cum_w > thr, else the smallest w with cum_w >= Z_k.
  Left alone: cust[c] >= stride (skipped), Z_k not positive and finite (stuck), mask[c] == 0 (not counted).

numpy float64, one ufunc an operation: no contraction.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import st_oracle as sto  # noqa: E402
import ti_oracle as tio  # noqa: E402

CHUNK = 256
MUTS = ("plain", "u3", "ge")    # the wrong replays: a left-to-right column sum, u from u3's element, >= for >


def cum_columns(lik, plain: bool = False):
    """(cum (rows, stride), Z (stride)) in the header's association; plain: the wrong one, left to right"""
    lik = np.asarray(lik, dtype=np.float64)
    rows, stride = lik.shape
    if plain:
        cum = np.cumsum(lik, axis=0)
        return cum, cum[-1].copy()
    cum = np.empty((rows, stride))
    base = None
    for w0 in range(0, rows, CHUNK):
        w1 = min(rows, w0 + CHUNK)
        pre = np.empty((w1 - w0, stride))
        s = lik[w0].copy()
        pre[0] = s
        for w in range(w0 + 1, w1):
            s = s + lik[w]
            pre[w - w0] = s
        cum[w0:w1] = pre if base is None else base[None, :] + pre
        base = s if base is None else base + s
    return cum, base.copy()


def choose(cum_k, Z: float, u: float, ge: bool = False) -> int:
    """the rule on one column by binary search (cum_k non-decreasing, Z positive and finite)"""
    thr = u * Z
    if ge:
        w = int(np.searchsorted(cum_k, thr, side="left"))
    else:
        w = int(np.searchsorted(cum_k, thr, side="right"))          # the smallest w with cum_w > thr
    if w == len(cum_k):
        w = int(np.searchsorted(cum_k, Z, side="left"))             # the smallest w with cum_w >= Z
    return w


def choose_linear(cum_k, Z: float, u: float) -> int:
    """the rule as it is written: a scan"""
    thr = u * Z
    for w, x in enumerate(cum_k):
        if x > thr:
            return w
    for w, x in enumerate(cum_k):
        if x >= Z:
            return w
    raise AssertionError("cum never reaches Z")


def fallback_reached(Z: float, u: float) -> bool:
    """no cum_w exceeds thr: fl(u Z) >= Z"""
    return not (np.float64(u) * np.float64(Z) < np.float64(Z))


def uniforms(seed: int, sweep: int, C: int, first: int = 0, count=None, mut=None):
    """u of the flat customers first .. first + count - 1 of a call with C customers"""
    count = C - first if count is None else count
    c = np.arange(first, first + count, dtype=np.uint64)
    key = np.uint64(tio.sweep_key(seed, sweep))
    off = np.uint64(2 * C + 1) if mut == "u3" else np.uint64(3 * C + 1)
    return sto.unit(key, off + c)


def draw(cum, Z, dishes, u, ge: bool = False):
    """classes of customers at `dishes` (all < stride, all with a good Z) under uniforms u, vectorised a dish at a time"""
    dishes = np.asarray(dishes, dtype=np.int64)
    out = np.zeros(len(dishes), dtype=np.int64)
    rows = cum.shape[0]
    for k in np.unique(dishes):
        sel = np.flatnonzero(dishes == k)
        col = np.ascontiguousarray(cum[:, k])
        thr = u[sel] * Z[k]
        w = np.searchsorted(col, thr, side="left" if ge else "right")
        w = np.where(w == rows, np.searchsorted(col, Z[k], side="left"), w)
        out[sel] = w
    return out


def sample_classes(lik, cust, seed: int, sweep: int, cls, mask=None, mut=None):
    """stb_sample_classes: (cls after the call (uint32), (skipped, stuck, drawn))"""
    lik = np.asarray(lik, dtype=np.float64)
    cust = np.asarray(cust, dtype=np.int64)
    out = np.array(cls, dtype=np.uint32)
    C = len(cust)
    stride = lik.shape[1]
    cum, Z = cum_columns(lik, plain=(mut == "plain"))
    live = np.ones(C, dtype=bool) if mask is None else np.asarray(mask) != 0
    skip = live & (cust >= stride)
    kk = np.minimum(cust, stride - 1)
    good = (Z > 0.0) & np.isfinite(Z)
    stuck = live & ~skip & ~good[kk]
    go = np.flatnonzero(live & ~skip & ~stuck)
    u = uniforms(seed, sweep, C, mut=mut)
    out[go] = draw(cum, Z, cust[go], u[go], ge=(mut == "ge")).astype(np.uint32)
    return out, (int(skip.sum()), int(stuck.sum()), len(go))


def generate(K, h, a, bpar, coff, lik, M: int = 0, seed: int = 0, sweep: int = 0):
    """stb_tindic_generate: the seating's replay under the prior from empty restaurants, then every class.  The seating's
    dict (st_oracle.replay) with cls and cls_info added"""
    G = int(np.sum(K))
    rp = sto.replay(K, np.zeros(G, dtype=np.uint32), np.zeros(G, dtype=np.uint16), h, a, bpar, coff, None, None, M=M, seed=seed,
                    sweep=sweep)
    cls, info = sample_classes(lik, rp["cust"], seed, sweep, np.zeros(len(rp["cust"]), dtype=np.uint32))
    rp["cls"], rp["cls_info"] = cls, info
    return rp


# ---------------------------------------------------------------------------------------------------- the cases

def matrix_with_zeros(rows: int, stride: int, seed: int, zero_col=None):
    """random weights, about a quarter of the cells zero, the first and last rows of column 0 zero where there is room,
    column 1 (where there is one, and rows >= 3) a single positive cell; zero_col: a column of zeros"""
    rng = np.random.default_rng([seed, rows, stride])
    lik = rng.random((rows, stride)) * (rng.random((rows, stride)) > 0.25)
    if rows >= 3:
        lik[0, 0] = lik[-1, 0] = 0.0
        lik[rows // 2, 0] = 0.5
        if stride > 1:
            lik[:, 1] = 0.0
            lik[rows // 3, 1] = 0.25
    if zero_col is not None:
        lik[:, zero_col] = 0.0
    return lik


# the fixed case that tells the wrong replays apart (tests/test_classgen_host.py)
MUT_CASE = dict(rows=513, stride=5, C=400, seed=41, sweep=2)

# the law of the replay: 3 dishes over 1000 classes, columns ~ Dirichlet(0.5), 10^5 draws a dish.  The seed is chosen on the
# CPU so that the cells of expected count < 5 hold at most 2 % of each column (tests/test_classgen_host.py checks it)
LAW_ROWS, LAW_DISHES, LAW_DRAWS, LAW_SEED, LAW_SWEEP = 1000, 3, 100000, 7, 0


def law_matrix(seed: int = LAW_SEED):
    rng = np.random.default_rng([seed, 0xC1A55])
    return np.ascontiguousarray(rng.dirichlet(np.full(LAW_ROWS, 0.5), size=LAW_DISHES).T)


def merged_mass(p, total: int, floor: float = 5.0) -> float:
    """the mass of the cells st_oracle.chi2_p takes together"""
    p = np.asarray(p, dtype=np.float64)
    return float(p[(p > 0.0) & (total * p < floor)].sum())


def hist_p(cls, p, total: int) -> float:
    """chi-square p of the classes' histogram against the column p"""
    cnt = np.bincount(np.asarray(cls, dtype=np.int64), minlength=len(p))
    cells = {int(w): int(c) for w, c in enumerate(cnt) if c}
    return sto.chi2_p(cells, {int(w): float(q) for w, q in enumerate(p)}, total)


# the joint law: 20000 restaurants x 3 customers x 2 dishes x 2 classes
JOINT_I, JOINT_A, JOINT_B, JOINT_ROUNDS = 20000, 0.3, 1.5, 10
JOINT_H = (0.35, 0.65)
JOINT_LIK = ((0.7, 0.2), (0.3, 0.8))      # columns sum to 1: column k is dish k's law of the classes
JOINT_SEED = 5                            # chosen on the CPU so that the replays pass tests/test_classgen_host.py


def joint_case():
    """(K, h, bpar, coff, lik) of the joint-law case"""
    I = JOINT_I
    return (np.full(I, 2, dtype=np.int32), np.tile(np.array(JOINT_H), I), np.full(I, JOINT_B),
            (3 * np.arange(I + 1)).astype(np.uint64), np.array(JOINT_LIK))


def joint_law(lik=JOINT_LIK):
    """{(z, t, cls): probability}: P(z, t) prod_c lik[cls_c][z_c], P the prior of st_oracle.ujoint_states (L = 1)"""
    import itertools

    import td_oracle as tdo

    P = sto.ujoint_states(3, 2, JOINT_H, JOINT_A, JOINT_B)
    law = {}
    for (z, ts), pz in zip(tdo.states(3, 2), P):
        for cl in itertools.product(range(2), repeat=3):
            law[(tuple(z), tuple(ts), cl)] = float(pz) * math.prod(lik[cl[c]][z[c]] for c in range(3))
    tot = sum(law.values())
    assert abs(tot - 1.0) < 1e-12, tot
    return law


def joint_cells(cust, t, cls):
    """the states of the joint-law case as a dict {(z, t, cls): count}"""
    rows = np.concatenate([np.asarray(cust, dtype=np.int64).reshape(-1, 3), np.asarray(t, dtype=np.int64).reshape(-1, 2),
                           np.asarray(cls, dtype=np.int64).reshape(-1, 3)], axis=1)
    keys, cnt = np.unique(rows, axis=0, return_counts=True)
    return {(tuple(int(v) for v in k[:3]), tuple(int(v) for v in k[3:5]), tuple(int(v) for v in k[5:])): int(c)
            for k, c in zip(keys, cnt)}


def swapped(lik):
    """the matrix with its columns exchanged"""
    return tuple(tuple(reversed(r)) for r in lik)
