"""The cases of tests/test_samplers_truth_host.py and tests/test_gpu_samplers_truth.py: shapes placed on the boundaries
where k_tcounts, k_tcwin and k_partition change behaviour, and their truth replays (tests/hs_oracle.py), computed once a
process.  The seeds were chosen on the host so that no draw of any case is undecided (hs_oracle's eps)."""
from __future__ import annotations

import functools

import numpy as np

import hs_oracle as hs

A_SET = (0.0, 5e-324, 0.5, 0.999)
B_SET = (0.01, 1.0, 1e4)
H_SET = (1e-3, 1.0, 30.0)

# ---------------------------------------------------------------------------------------------------- k_tcounts
TC_N = 4100
TMAX = (2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 4100)
TC_THREADS = (64, 128, 512, 1024)
TC_TRUNC_M = (64, 257, 4096, 4097)


class Case:
    """pairs in the CSR layout of synth.Groups, the call's parameters, and the seed"""

    def __init__(self, name, K, n, t, h, a, bpar, M, seed, sweeps, W=0, ref=False):
        self.name = name
        self.K = np.asarray(K, dtype=np.int32)
        self.n = np.asarray(n, dtype=np.uint32)
        self.t = np.asarray(t, dtype=np.uint16)
        self.h = None if h is None else np.asarray(h, dtype=np.float64)
        self.a, self.bpar, self.seed, self.sweeps, self.W, self.ref = a, np.asarray(bpar, dtype=np.float64), seed, sweeps, W, ref
        self.N = max(int(self.n.max()), 3)
        self.M = M or int(self.n.max())  # as stb_tcounts_create: M = 0 is the largest n


def tc_boundary(seed=101):
    """rows with n = tmax on every chunk boundary of every workgroup size and either side of the LDS cap, each starting
    at t = 1, t = tmax and mid-row; N = M = 4100"""
    rng = np.random.default_rng(1)
    n = np.repeat(np.array(TMAX), 3)
    t = np.array([x for m in TMAX for x in (1, m, (m + 1) // 2)])
    h = 0.3 + 1.2 * rng.random(len(n))
    return Case("tc_boundary", [9] * 7, n, t, h, 0.5, [0.5, 1.0, 2.0, 3.0, 5.0, 10.0, 40.0], TC_N, seed, 3)


TC_TRUNC_SEED = {64: 111, 257: 112, 4096: 113, 4097: 114}


def tc_trunc(M):
    """n > M: draws from the conditional truncated at M (M = 4097: the truncated rows recompute)"""
    rng = np.random.default_rng(M)
    n = np.array([4100, M + 1, M, 300, 4097, M - 1, 65, 4100])
    tm = np.minimum(n, M)
    t = np.array([1, tm[1], tm[2] // 2, 7, tm[4], 1, tm[6], tm[7] // 3])
    h = 0.3 + 1.2 * rng.random(len(n))
    return Case(f"tc_trunc_M{M}", [4, 4], n, t, h, 0.5, [1.5, 20.0], M, TC_TRUNC_SEED[M], 3)


TC_PARAM_SEED = {(0.0, True): 121, (0.0, False): 122, (5e-324, True): 123, (5e-324, False): 124, (0.5, True): 125,
                 (0.5, False): 126, (0.999, True): 127, (0.999, False): 128}


def tc_params(a, with_h):
    """rows of 300 and 4097 over a x b x h (with_h False: h = None)"""
    n = np.array([300, 300, 300, 4097, 4097, 4097] * 3)
    t = np.array([1, 150, 300, 4097, 2000, 1] * 3)
    h = np.array(list(H_SET) * 6) if with_h else None
    return Case(f"tc_params_a{a:g}_{'h' if with_h else 'noh'}", [6, 6, 6], n, t, h, a, B_SET, 0, TC_PARAM_SEED[(a, with_h)], 2)


def tc_big_T(seed=131):
    """64 pairs with T about 1e5: T_ is large and the last pair's log terms sit near log(b + 1e5 a)"""
    rng = np.random.default_rng(3)
    return Case("tc_big_T", [64], np.full(64, TC_N), np.full(64, 1563), 0.5 + rng.random(64), 0.5, [1.0], TC_N, seed, 2)


def tc_cases():
    out = [tc_boundary()] + [tc_trunc(M) for M in TC_TRUNC_M]
    out += [tc_params(a, wh) for a in A_SET for wh in (True, False)] + [tc_big_T()]
    return out


@functools.lru_cache(maxsize=None)
def tc_cells():
    need = sorted({int(x) for c in tc_cases() for x in c.n})
    return hs.cells(A_SET, TC_N, TC_N, tuple(need))


# ---------------------------------------------------------------------------------------------------- k_tcwin
TCW_N = 600
TCW_W = (15, 16, 17, 31, 32)
TCW_ROWS = (40, 61, 64, 65, 66, 130, 600)


def _tcw_t(Mt, W):
    return [min(max(x, 1), Mt) for x in (1, 2 * W, 2 * W + 1, Mt // 2, Mt - 2 * W, Mt)]


TCW_SEED = {}


def tcw_main(W, ref, a=0.5, b=None, seed=None):
    """W either side of the one-chunk switch (4W+1 <= 64) on rows around 64, t where the span is clipped at 1 and at Mt"""
    rng = np.random.default_rng(W)
    n = np.repeat(np.array(TCW_ROWS), 6)
    t = np.array([x for m in TCW_ROWS for x in _tcw_t(m, W)])
    h = 0.3 + 1.2 * rng.random(len(n))
    bpar = [0.5, 1.0, 2.0, 3.0, 5.0, 10.0, 40.0] if b is None else [b] * 7
    name = f"tcw_W{W}_{'ref' if ref else 'mh'}" + ("" if b is None else f"_a{a:g}_b{b:g}")
    return Case(name, [6] * 7, n, t, h, a, bpar, 0, seed or 200 + W + 50 * ref, 2, W, ref)


def tcw_trunc(W, ref):
    """M = 65 < n = 600: Mt = 65"""
    rng = np.random.default_rng(100 + W)
    return Case(f"tcw_trunc_W{W}_{'ref' if ref else 'mh'}", [6], np.full(6, 600), _tcw_t(65, W), 0.3 + 1.2 * rng.random(6),
                0.5, [2.0], 65, 300 + W + 50 * ref, 2, W, ref)


def tcw_params(a, b):
    return tcw_main(16, False, a, b, 400 + 10 * A_SET.index(a) + B_SET.index(b))


def tcw_cases():
    out = [tcw_main(W, ref) for W in TCW_W for ref in (False, True)]
    out += [tcw_trunc(W, ref) for W in TCW_W for ref in (False, True)]
    out += [tcw_params(a, b) for a in A_SET for b in B_SET]
    return out


@functools.lru_cache(maxsize=None)
def tcw_cells():
    return hs.cells(A_SET, TCW_N, TCW_N, tuple(TCW_ROWS))


# ---------------------------------------------------------------------------------------------------- k_partition
PT_L = (1, 2, 63, 64, 65, 66, 127, 128, 129, 1023, 1024, 1025, 2000)
PT_T = (2, 3, 7, 60)
PT_N, PT_M = 2059, 60
PT_S = (2060, 1000)  # above and below STB_PT_LDS = 1024; with S = 2060 sizes on both sides of it are counted
PT_SEED = {0.0: 501, 5e-324: 502, 0.5: 503, 0.999: 504}


def pt_pairs():
    """first rounds with L = n - t + 1 on the chunk boundaries; later rounds cross them downward"""
    n = np.array([L + t - 1 for L in PT_L for t in PT_T], dtype=np.uint32)
    t = np.array([t for L in PT_L for t in PT_T], dtype=np.uint16)
    return n, t


@functools.lru_cache(maxsize=None)
def pt_cells():
    return hs.cells(A_SET, PT_N, PT_M, None)


# ---------------------------------------------------------------------------------------------------- the replays

@functools.lru_cache(maxsize=None)
def _tc_truth(name):
    c = {x.name: x for x in tc_cases()}[name]
    st, t, out = hs.Stats(), c.t, []
    for s in range(c.sweeps):
        t, T, _ = hs.sweep(c.K, c.n, t, c.h, c.a, c.bpar, c.M, tc_cells()[c.a], c.seed, s, st)
        out.append((t, T))
    return out, st


def tc_truth(c: Case):
    """([(t, T) after sweep s], Stats)"""
    return _tc_truth(c.name)


@functools.lru_cache(maxsize=None)
def _tcw_truth(name):
    c = {x.name: x for x in tcw_cases()}[name]
    st, t, out = hs.Stats(), c.t, []
    for s in range(c.sweeps):
        t, T, _ = hs.window_sweep(c.K, c.n, t, c.h, c.a, c.bpar, c.M, tcw_cells()[c.a], c.W, c.seed, s, c.ref, st)
        out.append((t, T))
    return out, st


def tcw_truth(c: Case):
    return _tcw_truth(c.name)


@functools.lru_cache(maxsize=None)
def pt_truth(a, S):
    """(cnt, sizes, Stats)"""
    n, t = pt_pairs()
    st = hs.Stats()
    cnt, sizes, _ = hs.partition(n, t, a, PT_N, PT_M, S, pt_cells()[a], PT_SEED[a], 0, st)
    return cnt, sizes, st
