"""numpy restatement of the table-size partition draw of stb_sample_partition / stb_tcounts_partition
(libstb_amd/csrc/partition.hip), the checker of tests/test_partition_host.py and tests/test_gpu_partition.py, and the
laws it is judged by: the truth enumerated from the definition, the recursion's sequential law, the replay's own law
integrated over u, and the law of the reference's walk (lib/samplea.c:295-320, kept by the drop-in samplea2).

Tables as in tests/tc_oracle.py, (S1, packed cells, M), read through a dense copy: dense(S1, tab, N, M)[n, m] = log S^n_m.
"""
from __future__ import annotations

import math
from collections import defaultdict

import numpy as np

import orc
import tc_oracle as tco

TIE = tco.TIE  # a round with |u W - C(l)| <= TIE W for some l is reported as a near-tie
_M64 = (1 << 64) - 1
_G = 0x9E3779B97F4A7C15


def _mix(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def unit_at(key: int, j: int) -> float:
    """element j of the stream with this key: top 53 bits of mix(key + j gamma) / 2^53"""
    return (_mix((key + j * _G) & _M64) >> 11) * (1.0 / 9007199254740992.0)


def round_u(key: int, g: int, r: int) -> float:
    return unit_at(key, g * 65536 + r + 1)


def S_at(S1, tab, M: int, n: int, tau: int) -> float:
    """log S^n_tau, stb_lookup_S's semantics (1 <= tau <= n, tau <= M)"""
    if tau == n:
        return 0.0
    if tau == 1:
        return float(S1[n - 1])
    return float(tab[orc.row_offset(n, M) + tau - 2])


def dense(S1, tab, N: int, M: int) -> np.ndarray:
    """D[n, m] = S_at(n, m) for 1 <= m <= min(n, M), n <= N (NaN elsewhere)"""
    D = np.full((N + 1, M + 1), np.nan)
    for n in range(1, N + 1):
        for m in range(1, min(n, M) + 1):
            if m == n:
                D[n, m] = 0.0
            elif m == 1:
                D[n, m] = S1[n - 1]
        hi = min(n - 1, M)
        if n >= 3 and hi >= 2:
            o = orc.row_offset(n, M)
            D[n, 2:hi + 1] = tab[o:o + hi - 1]
    return D


def _wave_scan(v: np.ndarray) -> np.ndarray:
    """the Hillis-Steele scan of a 64-lane chunk, as the kernel's stb_wave_scan (wave.h) adds"""
    v = v.copy()
    o = 1
    while o < 64:
        v[o:] = v[o:] + v[:-o]
        o <<= 1
    return v


def round_weights(Nr: int, Mc: int, a: float, D):
    """(C(l), l = 1 .. L) of one exact round, in the kernel's arithmetic (partition.hip's header)"""
    L = Nr - Mc
    ptot = D[Nr, Mc + 1]
    nc = (L + 63) // 64
    C = np.zeros(64 * nc)
    f = W = 0.0
    for k in range(nc):
        l = np.arange(64 * k + 1, 64 * k + 65)
        inn = l <= L
        x = np.zeros(64)
        m = inn & (l >= 2)
        lm = l[m].astype(np.float64)
        x[m] = np.log(((lm - 1.0 - a) * (Nr - lm + 1.0)) / (lm - 1.0))
        F = _wave_scan(x) + f
        f = F[63]
        w = np.zeros(64)
        Sv = D[Nr - l[inn], Mc]
        w[inn] = np.exp((F[inn] + Sv) - ptot)
        c = _wave_scan(w) + W
        W = c[63]
        C[64 * k:64 * k + 64] = c
    return C[:L]


def draw_round(C: np.ndarray, u: float):
    """(l, near-tie): the smallest l with C(l) > u W, else L"""
    W = C[-1]
    target = u * W
    hit = np.flatnonzero(C > target)
    l = int(hit[0]) + 1 if hit.size else len(C)
    return l, bool(np.any(np.abs(target - C) <= TIE * W))


def logminus(x: float, y: float) -> float:
    if y >= x:
        return -math.inf
    if y - x < -80:
        return x - math.exp(y - x)
    return x + math.log(1 - math.exp(y - x))


def ref_walk(n: int, t: int, a: float, u: float, D):
    """lib/samplea.c:295-320 for one pair (1 < t < n): the t sizes in draw order, the remainder last"""
    ptot = float(D[n, t])
    rem = ptot + (math.log(u) if u > 0 else -math.inf)
    Nr, out = n, []
    for Mc in range(t - 1, 0, -1):
        fact = 0.0
        l = 1
        while l <= Nr - Mc:
            if l > 1:
                fact += math.log((l - a) * (Nr - l + 1) / (l - 1))
            term = fact + float(D[Nr - l, Mc]) - ptot
            if term >= rem:
                break
            rem = logminus(rem, term)
            l += 1
        l = min(l, Nr - Mc)
        out.append(l)
        Nr -= l
    out.append(Nr)
    return out


def pair_sizes(n: int, t: int, a: float, D, key: int, g: int, ref: bool = False):
    """(sizes in draw order, near-ties) of a pair with 1 < t < n"""
    if ref:
        return ref_walk(n, t, a, round_u(key, g, 0), D), 0
    Nr, out, ties = n, [], 0
    for r in range(t - 1):
        Mc = t - 1 - r
        if Nr - Mc == 1:
            l = 1
        else:
            l, tie = draw_round(round_weights(Nr, Mc, a, D), round_u(key, g, r))
            ties += tie
        out.append(l)
        Nr -= l
    out.append(Nr)
    return out, ties


def replay(n, t, a, S1, tab, N: int, M: int, S: int, seed: int, sweep: int, ref: bool = False, D=None):
    """the whole call: (cnt[S], sizes per pair (a list; None where nothing is written), near-ties)"""
    key = tco.sweep_key(seed, sweep)
    if D is None:
        D = dense(S1, tab, N, M)
    cnt = np.zeros(S, dtype=np.int64)
    sizes, ties = [], 0
    for g in range(len(n)):
        ng, tg = int(n[g]), int(t[g])
        if ng == 0:
            sizes.append([] if tg == 0 else None)
            continue
        if tg == ng:
            sizes.append([1] * ng)
            continue
        if tg == 0 or tg > ng or ng >= S or (tg > 1 and (ng > N or tg > M)):
            cnt[0] += 1
            sizes.append(None)
            continue
        if tg == 1:
            sz = [ng]
        else:
            sz, tie = pair_sizes(ng, tg, a, D, key, g, ref)
            ties += tie
        for s in sz:
            cnt[s] += 1
        sizes.append(sz)
    return cnt, sizes, ties


def bin_sizes(sizes, S: int, left_out: int = 0) -> np.ndarray:
    """the histogram of a list of size lists, cnt[0] = left_out"""
    cnt = np.zeros(S, dtype=np.int64)
    cnt[0] = left_out
    for sz in sizes:
        for s in sz or []:
            cnt[s] += 1
    return cnt


# ---- laws ------------------------------------------------------------------------------------------------------

def rising(x: float, k: int) -> float:
    """(x)_k = x (x+1) .. (x+k-1)"""
    r = 1.0
    for j in range(k):
        r *= x + j
    return r


def partitions(n: int, t: int, smax=None):
    """multisets of t block sizes >= 1 summing to n, as non-increasing tuples"""
    smax = n if smax is None else smax
    if t == 0:
        if n == 0:
            yield ()
        return
    for s in range(min(n - t + 1, smax), 0, -1):
        if s * t < n:
            break
        for rest in partitions(n - s, t - 1, s):
            yield (s,) + rest


def truth(n: int, t: int, a: float) -> dict:
    """P(multiset of sizes) from the definition: n! / (prod s_j! prod mult_k!) prod (1-a)_{s_j-1}, normalised"""
    w = {}
    for p in partitions(n, t):
        mult = defaultdict(int)
        for s in p:
            mult[s] += 1
        v = math.factorial(n)
        for s in p:
            v /= math.factorial(s)
        for m in mult.values():
            v /= math.factorial(m)
        for s in p:
            v *= rising(1.0 - a, s - 1)
        w[p] = v
    Z = sum(w.values())
    return {p: v / Z for p, v in w.items()}


def stirling(nmax: int, a: float) -> np.ndarray:
    """S^n_m(a) in float64 (n, m <= nmax), S^{n+1}_m = S^n_{m-1} + (n - m a) S^n_m"""
    S = np.zeros((nmax + 1, nmax + 1))
    S[0, 0] = 1.0
    for n in range(nmax):
        for m in range(1, n + 2):
            S[n + 1, m] = S[n, m - 1] + (n - m * a) * S[n, m]
    return S


def _to_multiset(law_seq: dict) -> dict:
    out = defaultdict(float)
    for seq, p in law_seq.items():
        out[tuple(sorted(seq, reverse=True))] += p
    return dict(out)


def recursion_law(n: int, t: int, a: float) -> dict:
    """the law of the sequential draw with the exact weights C(N-1, l-1) (1-a)_{l-1} S^{N-l}_M / S^N_{M+1}"""
    S = stirling(n, a)
    law = {(): 1.0}
    for r in range(t - 1):
        Mc = t - 1 - r
        nxt = defaultdict(float)
        for seq, p in law.items():
            Nr = n - sum(seq)
            for l in range(1, Nr - Mc + 1):
                w = math.comb(Nr - 1, l - 1) * rising(1.0 - a, l - 1) * S[Nr - l, Mc] / S[Nr, Mc + 1]
                nxt[seq + (l,)] += p * w
        law = nxt
    return _to_multiset({seq + (n - sum(seq),): p for seq, p in law.items()})


def replay_law(n: int, t: int, a: float, S1, tab, M: int) -> dict:
    """the law of the replay's draw (the kernel's arithmetic) integrated exactly over u: P(l) = (C(l) - C(l-1)) / W"""
    D = dense(S1, tab, n, M)
    law = {(): 1.0}
    for r in range(t - 1):
        Mc = t - 1 - r
        nxt = defaultdict(float)
        for seq, p in law.items():
            Nr = n - sum(seq)
            if Nr - Mc == 1:
                nxt[seq + (1,)] += p
                continue
            C = round_weights(Nr, Mc, a, D)
            pl = np.diff(np.concatenate([[0.0], C])) / C[-1]
            for l in range(1, len(C) + 1):
                if pl[l - 1] > 0:
                    nxt[seq + (l,)] += p * pl[l - 1]
        law = nxt
    return _to_multiset({seq + (n - sum(seq),): p for seq, p in law.items()})


def ref_walk_law(n: int, t: int, a: float, S1, tab, M: int, K: int = 20000) -> dict:
    """the law of the reference's walk over its one uniform, on the midpoints of K equal cells of [0, 1)"""
    D = dense(S1, tab, n, M)
    law = defaultdict(float)
    for k in range(K):
        law[tuple(sorted(ref_walk(n, t, a, (k + 0.5) / K, D), reverse=True))] += 1.0 / K
    return dict(law)


def tv(p: dict, q: dict) -> float:
    keys = set(p) | set(q)
    return 0.5 * sum(abs(p.get(k, 0.0) - q.get(k, 0.0)) for k in keys)
