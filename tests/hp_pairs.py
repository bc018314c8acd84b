"""Pair sets for the `aterms` truth tests (test_gpu_hp.py, test_gpu_hp_shapes.py): the mirrored strip geometries of the
summing forms, (n, t) pairs placed where fused walks go wrong -- labelled by class, thinned to a density ceiling in a
stated order -- and their long-double truth (hp_oracle.py) with the bar, per set and per class, plus how far the nearest
neighbouring cell of any pair lies (the sensitivity condition).  Test infrastructure only."""
import ctypes as C

import numpy as np

import hp_oracle as hp
import orc
from libstb_amd import capi, synth

U = hp.U
XS = np.concatenate([[0.01, 0.5, 0.999, 0.99999, 0.37, 0.98, 3 * 2.0 ** -30], synth.discount_grid(64)])[:64]

CLASSES = ("strip edge", "halo edge", "block-boundary row", "group row", "column 1", "diagonal", "last row",
           "last column", "heavy cell")
STRIP, HALO, BLOCK, GROUP, COL1, DIAG, LASTROW, LASTCOL, HEAVY = range(len(CLASSES))
NEVER_DROPPED = (STRIP, HALO, BLOCK, COL1, DIAG, LASTROW, LASTCOL, HEAVY)
HEAVY_COUNT = 3000
GROUPS = (2, 4, 8, 12, 16, 24)   # rows of a group / staged-row periods of the summing forms (grid_hb.hip, HB_DOT_GR)


def _period_rows(N):
    """fill.hip stb_period_rows: the renormalisation period, which caps a block"""
    bits = 1
    while (1 << bits) < N:
        bits += 1
    return max(1, 1450 // (2 * bits + 1))


_MHL = {1: 32, 2: 25, 3: 17, 4: 13}   # fill_hb.hip hb_mhl: halo lanes at most


def hb_geometry(N, C):
    """(R, UC, HC) of the halo-block forms (fill_hb.hip hb_geometry) with C columns a lane: blocks of R rows (the state
    before block b is row 1 + b R), strip j's own columns from 2 + j UC, its halo the HC columns left of them"""
    R = min(48, _period_rows(N), (_MHL[C] - 1) * C) // 8 * 8
    if C == 3:
        R = R // 24 * 24
    HL = R // C
    return R, (64 - HL) * C, HL * C


def grid_geometry(N, C):
    """(R, UC, HC) of the grid form (grid_hb.hip stb_grid_geometry) with C columns a lane"""
    R = min(48, _period_rows(N)) // 8 * 8
    HL = R // C
    return R, (64 - HL) * C, HL * C


def mirrored_geometries(N):
    """every geometry the summing forms take at N rows: the halo-block form with 2, 3, 4 columns a lane (STB_HB_DOT_C, or
    stb_hb_sum_C's choice) and the grid form with 2, 4, 8 (STB_GRID_C, or stb_grid_shape's choice)"""
    return sorted({hb_geometry(N, c) for c in (2, 3, 4)} | {grid_geometry(N, c) for c in (2, 4, 8)})


def walk_geometry(N, M):
    """mirrored_geometries(N) and the group lengths, the mirrored formulas checked against what the library reports
    (stb_fill_tuning's blocks and strips, stb_grid_shape)"""
    L = capi.lib()
    Cw, Rw = C.c_int(), C.c_int()
    assert L.stb_fill_tuning(N, M, 1, C.byref(Cw), C.byref(Rw), None) == 6
    assert (Rw.value, Cw.value) in {hb_geometry(N, c)[:2] for c in (1, 2, 4)}, (Rw.value, Cw.value)
    geoms = mirrored_geometries(N)
    for D in (29, 64):
        gc, gg, gk = C.c_int(), C.c_int(), C.c_int()
        assert L.stb_grid_shape(N, M, D, C.byref(gc), C.byref(gg), C.byref(gk)) == 0
        assert grid_geometry(N, gc.value) in geoms
        assert gg.value in GROUPS and gk.value in GROUPS, (gg.value, gk.value)
    return geoms, sorted(GROUPS)


def table_cells(N, M):
    return hp.s_cells(N, M)


def boundary_rows(N, R, which="all"):
    """the rows 1 + b R and 2 + b R either side of the block boundaries b = 1 .. of blocks of R rows; which = "kept": of the
    first, a middle and the last boundary only"""
    bs = list(range(1, (N - 1) // R + 1))
    if which == "kept" and bs:
        bs = sorted({bs[0], bs[len(bs) // 2], bs[-1]})
    return sorted({r for b in bs for r in (1 + b * R, 2 + b * R) if 3 <= r <= N})


def edge_columns(N, M):
    """(strip-edge columns, halo-edge columns) of every mirrored geometry: c - 1, c for every strip start c = 2 + j UC,
    and c - HC - 1, c - HC"""
    cm = min(N - 1, M)
    strip, halo = set(), set()
    for R, UC, HC in mirrored_geometries(N):
        for c in range(2, cm + 1, UC):
            strip |= {c - 1, c}
            halo |= {c - HC - 1, c - HC}
    strip = {e for e in strip if 2 <= e <= cm}
    halo = {e for e in halo if 2 <= e <= cm} - strip
    return np.array(sorted(strip), dtype=np.int64), np.array(sorted(halo), dtype=np.int64)


class BudgetTooSmall(ValueError):
    """the pairs targeted_pairs never drops do not fit the density ceiling asked for"""


def _every(rows, k):
    return rows[::k] if k > 1 else rows


def targeted_pairs(N, M, seed=7, stride=1, rho=None):
    """(K, n, t, T, bpar, cls): (n, t) pairs on the cells where fused walks go wrong, for every mirrored geometry, and the
    class of each pair (an index into CLASSES):
      strip edge / halo edge   on every `stride`-th row, every block-boundary row kept and row N, the columns either side of
                               every strip start 2 + j UC / of its halo edge 2 + j UC - HC
      block-boundary row       whole rows 1 + b R and 2 + b R either side of every block boundary of every R
      group row                16 random columns (one from each sixteenth of the row) of every other row (groups of 2 .. 24 rows make every row a group's or a
                               staged row's neighbour)
      column 1, diagonal       t = 1 on every 37th row; (3, 2), t = n - 1 and t = n (log 1) on every 11th row
      last row, last column    row N whole; (n, M) on every 11th row below the diagonal, and the last stored cell of row N
      heavy cell               HEAVY_COUNT pairs on (N // 2, 7): a count no dense word holds
    rho: a ceiling G <= rho * cells.  The generator thins itself in this order until it fits: group rows (every 2nd, 4th,
    ... down to 8 rows), then the rows that carry edges alone (the stride doubled, down to 16 rows), then block-boundary
    rows other than those of the first, a middle and the last boundary of every R (every 2nd, 4th, ... of them).  The
    classes of NEVER_DROPPED are never thinned below what check_coverage asks, which is asserted here.  In that order the
    block-boundary rows keep 90 % and more of a 0.04 ceiling at the large shapes and the group rows go down to ~15 rows
    (4001 x 1001, 70000 x 130, 140000 x 90): the sparse sets hold almost no row from inside a block."""
    rng = np.random.default_rng(seed)
    geoms = mirrored_geometries(N)
    cm = min(N - 1, M)
    strip_cols, halo_cols = edge_columns(N, M)
    kept_block = sorted({r for R, _, _ in geoms for r in boundary_rows(N, R, "kept")})
    more_block = sorted({r for R, _, _ in geoms for r in boundary_rows(N, R)} - set(kept_block))
    block_all = set(kept_block) | set(more_block)
    edge_rows = [r for r in range(3, N + 1) if r % stride == 0 and r not in block_all]
    group_rows = [r for r in range(3, N + 1) if r not in block_all]

    def row_len(r):
        return min(r - 1, M)

    fixed = (sum(row_len(r) for r in kept_block) + 1 + len(range(2, N + 1, 37)) + 1 + sum(2 if r - 1 <= M else 1 for r in range(3, N + 1, 11)) + 1
             + min(N, M) + HEAVY_COUNT)
    budget = None if rho is None else int(rho * table_cells(N, M))

    def edge_cost(rows):
        r = np.asarray(rows, dtype=np.int64)
        lim = np.minimum(r - 1, M)
        return int(np.searchsorted(strip_cols, lim, side="right").sum() + np.searchsorted(halo_cols, lim, side="right").sum())

    def total(kg, ke, kb):
        return (fixed + sum(row_len(r) for r in _every(more_block, kb))
                + edge_cost(sorted(set(_every(edge_rows, ke)) | set(kept_block) | set(_every(more_block, kb)) | {N})) + sum(min(16, row_len(r) - 1) for r in _every(group_rows, kg) if row_len(r) >= 2))

    kg = ke = kb = 1
    if budget is not None:
        while total(kg, ke, kb) > budget and len(group_rows) // (2 * kg) >= 8:
            kg *= 2
        while total(kg, ke, kb) > budget and len(edge_rows) // (2 * ke) >= 16:
            ke *= 2
        while total(kg, ke, kb) > budget and kb <= len(more_block):
            kb *= 2
        if total(kg, ke, kb) > budget:
            raise BudgetTooSmall(f"{N} x {M}: what is never dropped is {total(kg, ke, kb)} pairs, above {rho} of the cells ({budget})")
    ns, ts, cs = [], [], []

    def add(n, t, c):
        t = np.atleast_1d(t)
        ns.append(np.full(t.shape[0], n))
        ts.append(t)
        cs.append(np.full(t.shape[0], c))

    for n in sorted(set(_every(edge_rows, ke)) | set(kept_block) | set(_every(more_block, kb)) | {N}):
        add(n, strip_cols[strip_cols <= row_len(n)], STRIP)
        add(n, halo_cols[halo_cols <= row_len(n)], HALO)
    for n in sorted(set(kept_block) | set(_every(more_block, kb))):
        add(n, np.arange(1, row_len(n) + 1), BLOCK)
    gr = np.array(_every(group_rows, kg), dtype=np.int64)
    gl = np.minimum(gr - 1, M)
    gr, gl = gr[gl >= 2], gl[gl >= 2]
    # (one draw from each sixteenth of the columns 2 .. L: their number does not depend on the seed)
    k16 = np.arange(16)[None, :]
    cols = 2 + ((k16 + rng.random((len(gr), 16))) * ((gl - 1)[:, None] / 16.0)).astype(np.int64)
    cols = np.where((gl - 1)[:, None] >= 16, np.minimum(cols, gl[:, None]), 2 + k16)
    take = (gl - 1)[:, None] > k16
    take |= (gl - 1)[:, None] >= 16
    ns.append(np.broadcast_to(gr[:, None], cols.shape)[take])
    ts.append(cols[take])
    cs.append(np.full(int(take.sum()), GROUP))
    add(2, 1, COL1)
    for n in range(2, N + 1, 37):
        add(n, 1, COL1)
    add(3, 2, DIAG)
    for n in range(3, N + 1, 11):
        if n - 1 <= M:
            add(n, n - 1, DIAG if n - 1 < M else LASTCOL)  # next to the diagonal
        add(n, min(n, M), DIAG if n <= M else LASTCOL)      # the diagonal (log 1), or the last column
    add(N, cm, LASTCOL)
    add(N, np.arange(1, min(N, M) + 1), LASTROW)            # the last row, whole
    add(N // 2, np.full(HEAVY_COUNT, 7), HEAVY)             # one cell carrying a huge count
    n = np.concatenate(ns).astype(np.uint32)
    t = np.concatenate(ts).astype(np.uint16)
    cls = np.concatenate(cs).astype(np.int8)
    assert int(np.concatenate(ts).max()) <= 65535 and np.all(t <= np.minimum(n, M)) and np.all(t >= 1)
    assert len(n) == total(kg, ke, kb), (len(n), total(kg, ke, kb))   # (the cost model the thinning went by is the generator's)
    assert budget is None or len(n) <= budget
    I = 37
    K = np.full(I, len(n) // I, dtype=np.int32)
    K[-1] += len(n) - int(K.sum())
    order = rng.permutation(len(n))
    n, t, cls = n[order].copy(), t[order].copy(), cls[order].copy()
    T = np.add.reduceat(t.astype(np.uint64), np.r_[0, np.cumsum(K)[:-1]]).astype(np.uint32)
    bpar = np.linspace(0.3, 40.0, I)
    check_coverage(N, M, n, t, cls)
    return K, n, t, T, bpar, cls


def check_coverage(N, M, n, t, cls):
    """what no thinning may drop, for every mirrored geometry: both columns either side of each strip start and halo edge
    (among the strip-edge / halo-edge pairs); both whole rows either side of the first, a middle and the last block
    boundary of every R; column 1; cell (3, 2); the diagonal neighbours; the last row, whole; the last column; the
    heavy cell.  A condition on the generator, checked on the CPU."""
    n = n.astype(np.int64)
    t = t.astype(np.int64)
    cm = min(N - 1, M)
    tcols = {c: set(np.unique(t[cls == c]).tolist()) for c in (STRIP, HALO)}
    for R, UC, HC in mirrored_geometries(N):
        for c in range(2, cm + 1, UC):
            for e in (c - 1, c):
                assert not 2 <= e <= cm or e in tcols[STRIP], ("strip edge", N, M, (R, UC, HC), e)
            for e in (c - HC - 1, c - HC):
                assert not 2 <= e <= cm or e in tcols[STRIP] or e in tcols[HALO], ("halo edge", N, M, (R, UC, HC), e)
        rows = boundary_rows(N, R, "kept")
        assert len(rows) >= 2 or N < R + 3, ("block boundaries", N, R)
        for r in rows:
            got = np.unique(t[(n == r) & (cls == BLOCK)])
            assert np.array_equal(got, np.arange(1, min(r - 1, M) + 1)), ("block-boundary row", N, M, R, r)
    for c in NEVER_DROPPED:                                 # (no halo-edge column exists where one strip holds the table)
        assert np.any(cls == c) or (c == HALO and not len(edge_columns(N, M)[1])), (CLASSES[c], N, M)
    assert np.any((n == 3) & (t == 2)) and np.any((t == 1) & (cls == COL1)) and np.any((t == n - 1) & (cls == DIAG))
    assert np.array_equal(np.unique(t[(n == N) & (cls == LASTROW)]), np.arange(1, min(N, M) + 1))
    assert np.any((t == cm) & (cls == LASTCOL)) and int(np.count_nonzero(cls == HEAVY)) == HEAVY_COUNT


CHUNKS = 64          # pieces the whole-row classes are handed over in at the tall shapes
CHUNK_FROM = 30000   # rows from which they are: below, a class of whole rows is one sum
BULK = (BLOCK, GROUP)
LOC = [0, 1, 4, 5]   # XS[LOC] = 0.01, 0.5, 0.37, 0.98: the discounts of the class-by-class hand-over
NO_SPARSE_SET = {(1250, 81), (1250, 82)}   # what is never dropped alone exceeds 0.04 of the cells


# The sums of the class-by-class hand-over whose bar is NOT below the nearest neighbouring cell's distance, by name:
# (N, M, set) -> {(class, discount): pieces}.  From the truth alone (test_hp_shapes_host.py asserts that these, and only
# these, fail the condition).  At a = 0.5 the smallest distance between neighbouring cells of a whole row shrinks with n
# and falls under the bar of ~2000 table rows' worth of whole rows from n ~ 35000 (47000 at 70000 x 130) on, and under the
# bar of the 90 pairs of row 140000 alone (which the restaurant terms' bar dominates); at a = 0.01 single pieces hold a row
# whose mode lies between two of its columns.
CANNOT_HOLD = {
    (70000, 130, "targeted"): {("block-boundary row", 0.01): [15], ("block-boundary row", 0.5): list(range(43, 64)),
                               ("group row", 0.01): [46], ("group row", 0.5): list(range(44, 64))},
    (140000, 90, "targeted"): {("block-boundary row", 0.01): [7, 23], ("block-boundary row", 0.5): list(range(18, 64)),
                               ("group row", 0.01): [7, 23], ("group row", 0.5): list(range(16, 64)),
                               ("last row", 0.5): [0]},
    (140000, 90, "sparse"): {("block-boundary row", 0.5): list(range(40, 64))},
}


def chunk_of(N, n, cls):
    """the piece a pair belongs to: 0, but for the block-boundary-row and group-row classes of a table of CHUNK_FROM rows
    and more, which are cut by row into CHUNKS pieces (rows (k N / CHUNKS, (k + 1) N / CHUNKS]) -- a sum of 10^6 pairs has
    a bar no single cell's neighbour exceeds, a sum of the whole rows of 2000 table rows does not"""
    ch = (n.astype(np.int64) - 1) * CHUNKS // N
    return np.where(np.isin(cls, BULK) & (N >= CHUNK_FROM), ch, 0)


class Truth:
    """per discount d and piece p = class * CHUNKS + chunk: psum[d, p] the long-double sum of log S over the pairs of the
    piece, pbar[d, p] the sum of their bars, near[d, p] the smallest |y(n,t) - y(n,t-1)| and |y(n,t) - y(n-1,t)| over them
    (inf where no neighbour exists), count[p] its pairs; rest[d] = (restaurant terms, their bar)"""

    def __init__(self, psum, pbar, near, count, rest):
        self.psum, self.pbar, self.near, self.count, self.rest = psum, pbar, near, count, rest

    def _cols(self, classes, chunk):
        cs = range(len(CLASSES)) if classes is None else classes
        return [c * CHUNKS + k for c in cs for k in (range(CHUNKS) if chunk is None else [chunk])]

    def chunks(self, c):
        """the pieces of class c that hold pairs"""
        return [k for k in range(CHUNKS) if self.count[c * CHUNKS + k]]

    def sums(self, classes=None, chunk=None):
        """[(the true sum, its bar)] per discount of the restaurant terms + the pairs of `classes` (None: all; chunk: that
        piece of them alone): sum of per-pair bars + restaurant-term bars + 4 u |sum|"""
        cs = self._cols(classes, chunk)
        out = []
        for d in range(self.psum.shape[0]):
            tot = self.rest[d][0] + self.psum[d, cs].sum()
            out.append((tot, float(self.pbar[d, cs].sum()) + self.rest[d][1] + 4 * U * abs(float(tot))))
        return out

    def margin(self, classes=None, chunk=None):
        """per discount: (the nearest neighbouring cell's distance over the pairs of the sum) / (the sum's bar); above 1,
        one pair answered from a neighbouring cell cannot hide under the bar"""
        cs = self._cols(classes, chunk)
        return np.array([float(self.near[d, cs].min()) / b for d, (_, b) in enumerate(self.sums(classes, chunk))])


_truths = {}


def aterms_truth_by_class(sets, x, N, M):
    """[Truth] for several pair sets (K, n, t, T, bpar, cls) of one shape in ONE pass over the truth's rows"""
    x = np.asarray(x, dtype=np.float64)
    D, NC = len(x), len(CLASSES) * CHUNKS
    slope = hp.K1 + hp.K2 / (1.0 - x)
    parts = []
    for s, (_, n, t, _, _, cls) in enumerate(sets):
        keep = n > 1
        piece = cls.astype(np.int64) * CHUNKS + chunk_of(N, n, cls)
        parts.append((n[keep].astype(np.int64), t[keep].astype(np.int64), piece[keep] + s * NC))
    nn = np.concatenate([p[0] for p in parts])
    tt = np.concatenate([p[1] for p in parts])
    bb = np.concatenate([p[2] for p in parts])
    order = np.lexsort((bb, nn))
    nn, tt, bb = nn[order], tt[order], bb[order]
    starts = np.searchsorted(nn, np.arange(N + 2))
    NB = NC * len(sets)
    psum = np.zeros((D, NB), dtype=hp.LD)
    pbar = np.zeros((D, NB))
    near = np.full((D, NB), np.inf)
    count = np.bincount(bb, minlength=NB)
    prev = np.full((D, M + 2), -np.inf)
    for r, v, e in hp.rows(x, N, M):
        lo, hi = starts[r], starts[r + 1]
        nxt = starts[r + 2] if r + 2 < len(starts) else hi
        if lo == hi and nxt == hi:
            continue
        lg = hp.logs(v, e)
        if lo < hi:
            tr, br = tt[lo:hi], bb[lo:hi]
            seg = np.r_[0, np.nonzero(np.diff(br))[0] + 1]
            ids = br[seg]
            y = lg[:, tr]                                    # (D, pairs of this row); t = n: log 1 = 0
            y64 = y.astype(np.float64)
            k = np.diff(np.r_[seg, len(br)])
            psum[:, ids] += np.add.reduceat(y, seg, axis=1)
            pbar[:, ids] += U * (slope[:, None] * r * k[None, :] + 4.0 * np.add.reduceat(np.abs(y64), seg, axis=1) + 16.0 * k[None, :])
            with np.errstate(invalid="ignore"):
                left = np.abs(y64 - lg[:, tr - 1].astype(np.float64))
                up = np.abs(y64 - prev[:, tr])
            d = np.fmin(np.where(np.isfinite(left), left, np.inf), np.where(np.isfinite(up), up, np.inf))
            near[:, ids] = np.minimum(near[:, ids], np.minimum.reduceat(d, seg, axis=1))
        prev[:] = -np.inf
        prev[:, :lg.shape[1]] = lg.astype(np.float64)
    out = []
    for s, (K, _, _, T, bpar, _) in enumerate(sets):
        rest = []
        for d in range(D):
            sv, bsum = hp.LD(0), 0.0
            for i in range(len(K)):
                val, b = hp.restaurant_term(x[d], int(T[i]), float(bpar[i]))
                sv += hp.LD(val)
                bsum += b
            rest.append((sv, bsum))
        sl = slice(s * NC, (s + 1) * NC)
        out.append(Truth(psum[:, sl], pbar[:, sl], near[:, sl], count[sl], rest))
    return out


def aterms_truth(K, n, t, T, bpar, x, N, M, cls=None):
    """per discount: (the true sum, its bar) -- sum of per-pair bars + restaurant-term bars + 4 u |sum|"""
    key = (n.tobytes(), t.tobytes(), tuple(x), N, M)
    if key not in _truths:
        c = np.zeros(len(n), dtype=np.int8) if cls is None else cls
        _truths[key] = aterms_truth_by_class([(K, n, t, T, bpar, c)], x, N, M)[0]
    return _truths[key].sums()


FORMS = [("fused", {}, (1, 3, 8, 16, 29, 64)),
         ("hb2", {"STB_HB_DOT_C": "2"}, (1, 3)), ("hb3", {"STB_HB_DOT_C": "3"}, (8,)), ("hb4", {"STB_HB_DOT_C": "4"}, (16,)),
         ("chain", {"STB_ATERMS_HB": "0"}, (3, 8)),
         ("grid2", {"STB_ATERMS_GRID": "1", "STB_GRID_C": "2"}, (3,)), ("grid4", {"STB_ATERMS_GRID": "1", "STB_GRID_C": "4"}, (8, 29)),
         ("grid4jobs", {"STB_ATERMS_GRID": "1", "STB_GRID_C": "4", "STB_GRID_HELP_NW": "1"}, (64,)),
         ("grid8", {"STB_ATERMS_GRID": "1", "STB_GRID_C": "8"}, (16,)),
         ("dense", {"STB_ATERMS_SPARSE": "0"}, (3,)),
         ("tables", {"STB_ATERMS_FUSED": "0"}, (8, 64))]


def _create(L, K, n, t, T, bpar, N, M, D):
    h = L.stb_groups_create(len(K), orc.i32p(K), orc.u32p(T), orc.u32p(n), orc.u16p(t), orc.dp(bpar), N, M, D)
    assert h, capi.last_error()
    return h


def _aterms(L, h, x, tables=False):
    out = np.zeros(len(x))
    f = L.stb_groups_aterms_tables if tables else L.stb_groups_aterms
    capi.check(f(h, capi.dp(np.ascontiguousarray(x)), len(x), capi.dp(out)))
    return out


def _note(form, a, ratio):
    """print a worst error / bar (the MEASUREMENTS table is read from these lines)"""
    print(f"{form} a={a!r}: worst error / bar {ratio:.3g}")


def _check_sums(form, got, want):
    for d, (g, (tv, b)) in enumerate(zip(got, want)):
        e = abs(float(hp.LD(g) - tv))
        _note(f"aterms-{form}", d, e / b)
        assert e <= b, (form, d, g, float(tv), e, b)


def last_form(L, h):
    """(fused, which, sparse, C, R) of the set's most recent evaluation (stb_groups_last_form)"""
    v = [C.c_int() for _ in range(5)]
    capi.check(L.stb_groups_last_form(h, *[C.byref(q) for q in v]))
    return tuple(q.value for q in v)


def expected_form(name, env, N):
    """what stb_groups_last_form must report for a case of FORMS at N rows: a dict of the fields the name pins (fused,
    which, sparse, C, R); the default form ("fused") pins fused = 1 and sparse = 1, and its strips whichever form it took"""
    if name.endswith("tables"):
        return {"fused": 0}
    if "STB_HB_DOT_C" in env:
        c = int(env["STB_HB_DOT_C"])
        return {"fused": 1, "which": 2, "sparse": 1, "C": c, "R": hb_geometry(N, c)[0]}
    if "STB_GRID_C" in env:
        c = int(env["STB_GRID_C"])
        return {"fused": 1, "which": {2: 3, 4: 4, 8: 5}[c], "sparse": 1, "C": c, "R": grid_geometry(N, c)[0]}
    if name == "chain":
        return {"fused": 1, "which": 0, "sparse": 1, "C": 0, "R": 0}
    if name == "dense":
        return {"fused": 1, "which": 0, "sparse": 0, "C": 0, "R": 0}
    return {"fused": 1, "sparse": 1}


def check_form(L, h, name, want, N):
    """print the form the library reported for the evaluation just made, and assert it is the one the case names; where
    strips were taken, (C, R) equals the mirrored geometry"""
    got = dict(zip(("fused", "which", "sparse", "C", "R"), last_form(L, h)))
    print(f"aterms-{name}: form {got}")
    for k, v in want.items():
        assert got[k] == v, (name, k, got, want)
    if got["fused"] and got["which"] == 2:
        assert got["C"] in (2, 3, 4) and got["R"] == hb_geometry(N, got["C"])[0], (name, got)
    if got["fused"] and got["which"] >= 3:
        assert got["C"] == {3: 2, 4: 4, 5: 8}[got["which"]] and got["R"] == grid_geometry(N, got["C"])[0], (name, got)
    return got


class Counters:
    """the fallback counters and the shared-GPU rule around a case: unchanged / off, or the case fails (with the library's
    last error: a walk that gave up on a busy machine is a counted fallback, not a silent pass)"""

    def __init__(self, L):
        self.L = L
        self.before = (L.stb_groups_fallbacks(), L.stb_fill_fallbacks())

    def check(self, what):
        now = (self.L.stb_groups_fallbacks(), self.L.stb_fill_fallbacks())
        assert now == self.before, (what, "fallbacks (groups, fill)", self.before, now, capi.last_error())
        assert self.L.stb_shared_gpu_mode() == 0, what
