// dirmult.hip -- the log marginal of independent multinomials under a Dirichlet prior, over a uint32 count matrix on the
// device (include/stb_hip.h, stb_dirmult_logml).  For a multinomial with counts c_j, weights w_j,
// W = sum_j w_j and C = sum_j c_j:
//     log ml = [lgamma(W) - lgamma(W + C)] + sum_j [lgamma(w_j + c_j) - lgamma(w_j)]
// STB_DM_ROWS: every row of the matrix is a multinomial over its cols cells and the weights run along the columns;
// STB_DM_COLUMNS: every column is a multinomial over its rows cells and the weights run along the rows.  Either way all
// the multinomials share one weight vector, so W is formed once.  It is the term a collapsed log joint integrates a
// Dirichlet-distributed vector out with: the groups' base weights over the table counts c_gk (rows), the dishes' class
// distributions over the (class, dish) counts (columns) -- stb_tindic_logjoint_collapsed (tindic_obj.hip).
//
//   k_dm_weights   one workgroup: W, lgamma(W) and the checks of the weights
//   k_dm_rows      rows orientation: a workgroup takes blocks of 256 rows grid-stride, a wave one row of the block at a
//                  time, lanes strided over its cells; the last workgroup to finish -- a ticket: nobody waits -- adds the blocks
//   k_dm_rows_split  the same for few or long rows: the grid's waves take the rows one by one and leave row values in
//                  scratch; the last workgroup runs the block trees.  Same values, same association, same bits
//   k_dm_cols      columns orientation: lanes along the columns, one thread a (chunk of 256 rows, column); the last
//                  workgroup to finish -- a ticket again -- adds every column's chunks, then the columns
//   k_dm_root      log p(r | gamma) of a root vector (one workgroup; the collapsed joint's STB_CJ_ROOT)
//
// The operations (FP64 throughout, no contraction anywhere; u32 / u64 integers are exact):
//   s          = d_scale ? *d_scale : scale
//   w_j        = s * d_w[j]                      one product (s = 1.0 changes no bit); d_w NULL: w = s * w0 for every j
//   rise(x, m) = log(x + 0.0) + log(x + 1.0) + ... + log(x + (double)(m - 1)), added in that order       (1 <= m <= 8)
//   cell term    0.0                                     c = 0: nothing is evaluated
//                rise(w, c)                              1 <= c <= 8
//                lgamma(w + (double)c) - lgamma(w)       c > 8
//   W            d_w NULL: (double)ncat * w, one product (ncat = cols for rows, rows for columns).  Else the categories are
//                cut into chunks of 256 (chunk j = categories 256 j .. 256 j + 255, 0.0 beyond the end), a chunk is summed
//                by k_logjoint's block tree -- (x[l] + x[l + 64]) + (x[l + 128] + x[l + 192]) per lane l, then the 64-lane
//                shuffle tree v += shfl_down(v, o), o = 32, 16, .. 1 -- and the chunk sums are added in order j = 0, 1, ..
//                in double-double (dd_add, stb_common.h): W = hi + lo.
//   normaliser   0.0                                     C = 0 (C is a uint64 sum of the counts)
//                -rise(W, C)                             1 <= C <= 8
//                lgW - lgamma(W + (double)C)             otherwise; lgW = lgamma(W), evaluated once
//   a multinomial's value  each = cells + normaliser, one plain addition (-inf when it holds an impossible cell)
// The associations:
//   rows     a row's cells are taken in chunks of 64, lane l the cell 64 j + l of chunk j (0.0 beyond cols); a chunk is
//            summed by the 64-lane shuffle tree; the chunk sums are added in order j = 0, 1, .. in double-double: cells =
//            hi + lo.  Over the rows, separately for the cell sums and the normalisers: rows 256 k .. 256 k + 255 (0.0
//            beyond the end) are block k, summed by the block tree above; the block sums are added in order k = 0, 1, .. in
//            double-double.
//   columns  rows are cut into chunks of 256 (stb_lik_loglik's); one thread owns a (chunk, column) and adds its cell terms
//            to 0.0 in row order; a column's chunk sums are added in chunk order in double-double: cells = hi + lo.  Over
//            the columns: columns 256 k .. 256 k + 255 are block k, exactly as the rows above.
//   info's cells and norms are hi + lo of their double-doubles; the total is hi + lo of the two merged in the order cells,
//   norms (dd_merge), as k_logjoint merges its components.
// So no bit of any output depends on the grid or the workgroup size: STB_DIRMULT_WAVES = 1, 2, 4 or 8 waves a workgroup
// (default 4) give the same bits.
//
// Weights that are not usable (the counters are u64, exact in any order):
//   zero_weight  w = 0 with c = 0 (an underflowed root coordinate): the cell contributes 0.0
//   impossible   w = 0 with c > 0: the cell adds nothing to the sums; its multinomial's value, `cells` and the total are
//                -inf.  Every sum stays finite until then, and no input >= 0 and finite ever gives a NaN.
//   error word   1: a weight (or the device's scale) is negative, NaN or infinite; 2: W is not positive and finite.  The
//                call fails after its wait with the outputs undefined.
//
// What sets the pace: the counts are read once, 4 bytes a cell, coalesced (lanes along a row of the matrix in both
// orientations); a zero cell costs the read and two compares, a non-zero cell up to eight logs or two lgammas.  On a
// sparse matrix the lanes of a wave diverge on the non-zero cells (MEASUREMENTS section C1).
//
// Bounds: a rows-orientation wave reads cnt[r stride + k] for r < rows, k < cols <= stride and d_w[k], k < cols; a
// columns-orientation thread the same cells and d_w[r], r < rows.  The scratch holds 2 doubles a block of 256 rows
// (k_dm_rows), 2 doubles a row (k_dm_rows_split), or a double and a u64 a (chunk, column) plus a flag word and 2 doubles a
// column (k_dm_cols).

#include "stb_common.h"
#include "dirmult.h"
#include "ticket.h"

#pragma clang fp contract(off)

#define DM_BLOCK 256  // multinomials of a block of the sums, rows of a chunk, categories of a chunk of W (part of the contract)
#define DM_MAXTHREADS 512
#define DM_STAGE 512  // block sums (x 2 components) the last workgroup stages in LDS at a time; chunk sums of W a stage
#define DM_GRID_PER_CU 8u  // workgroups a compute unit the rows kernels launch at most
#define DM_ERR_W 1u
#define DM_ERR_TOTAL 2u
// ctl (zeroed on the stream ahead of the launches): [0] ticket (u32); as u64 words 1 .. 4: nonzero, count, zero_weight,
// impossible; u32 word 16: the error word; as doubles 16, 17: W, lgamma(W)
#define DM_CTL_ERR 16
#define DM_CTL_W 16
// host (pinned): [0] total, [1] cells, [2] norms; as u64 3 .. 6: nonzero, count, zero_weight, impossible; 7: the error word

__device__ __forceinline__ double dm_rise(double x, unsigned m) {
#pragma clang fp contract(off)
  double s = log(x + 0.0);
  for (unsigned j = 1; j < m; j++) s = s + log(x + (double)j);
  return s;
}

__device__ __forceinline__ double dm_cell(double w, unsigned c) {
#pragma clang fp contract(off)
  if (c <= 8u) return dm_rise(w, c);
  return lgamma(w + (double)c) - lgamma(w);
}

__device__ __forceinline__ double dm_norm(double W, double lgW, unsigned long long C) {
#pragma clang fp contract(off)
  if (C == 0) return 0.0;
  if (C <= 8) return -dm_rise(W, (unsigned)C);
  return lgW - lgamma(W + (double)C);
}

// what a lane counts over everything it sees
struct dm_counts {
  unsigned long long nnz = 0, cnt = 0, zw = 0, imp = 0;
};

// one cell: its term (0.0 when it adds nothing); *bad is set for an impossible cell
__device__ __forceinline__ double dm_visit(double w, unsigned c, dm_counts &n, bool *bad) {
  if (c == 0) {
    if (w == 0.0) n.zw++;
    return 0.0;
  }
  n.nnz++;
  n.cnt += c;
  if (w > 0.0) return dm_cell(w, c);
  n.imp++;
  *bad = true;
  return 0.0;
}

__device__ __forceinline__ void dm_publish_counts(dm_counts n, unsigned lane, unsigned *ctl) {
  n.nnz = stb_wave_sum(n.nnz);
  n.cnt = stb_wave_sum(n.cnt);
  n.zw = stb_wave_sum(n.zw);
  n.imp = stb_wave_sum(n.imp);
  unsigned long long *cnt = (unsigned long long *)ctl;
  if (lane == 0) {
    if (n.nnz) __hip_atomic_fetch_add(&cnt[1], n.nnz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n.cnt) __hip_atomic_fetch_add(&cnt[2], n.cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n.zw) __hip_atomic_fetch_add(&cnt[3], n.zw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n.imp) __hip_atomic_fetch_add(&cnt[4], n.imp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// thread 0 of the last workgroup: the two double-doubles and the counters to the pinned words
__device__ __forceinline__ void dm_answer(dd_t cells, dd_t norms, unsigned *ctl, double *host) {
#pragma clang fp contract(off)
  unsigned long long *cnt = (unsigned long long *)ctl;
  const unsigned long long nnz = __hip_atomic_load(&cnt[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long sum = __hip_atomic_load(&cnt[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long zw = __hip_atomic_load(&cnt[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long imp = __hip_atomic_load(&cnt[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  dd_t tot{0.0, 0.0};
  dd_merge(tot, cells);
  dd_merge(tot, norms);
  host[0] = imp ? -HUGE_VAL : tot.hi + tot.lo;
  host[1] = imp ? -HUGE_VAL : cells.hi + cells.lo;
  host[2] = norms.hi + norms.lo;
  unsigned long long *hc = (unsigned long long *)host;
  hc[3] = nnz;
  hc[4] = sum;
  hc[5] = zw;
  hc[6] = imp;
  hc[7] = __hip_atomic_load(&ctl[DM_CTL_ERR], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(DM_BLOCK) void k_dm_weights(const double *wv, uint64_t ncat, double w0, double scale,
                                                         const double *d_scale, unsigned *ctl) {
#pragma clang fp contract(off)
  __shared__ double schunk[DM_STAGE];  // chunk sums, a stage at a time: a wave a chunk, thread 0 adds them in order
  const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const double s = d_scale ? *d_scale : scale;
  unsigned err = (s > 0.0 && isfinite(s)) ? 0u : DM_ERR_W;
  double W;
  if (!wv) {
    const double w = s * w0;
    if (!(w >= 0.0 && isfinite(w))) err |= DM_ERR_W;
    W = (double)ncat * w;
  } else {
    dd_t acc{0.0, 0.0};
    const uint64_t nchunks = (ncat + DM_BLOCK - 1) / DM_BLOCK;
    for (uint64_t c0 = 0; c0 < nchunks; c0 += DM_STAGE) {
      const unsigned cn = nchunks - c0 < DM_STAGE ? (unsigned)(nchunks - c0) : DM_STAGE;
      for (unsigned c = wave; c < cn; c += nw) {
        const uint64_t j0 = (c0 + c) * DM_BLOCK + lane;
        double x[4];
#pragma unroll
        for (unsigned q = 0; q < 4; q++) {
          x[q] = j0 + 64 * q < ncat ? s * wv[j0 + 64 * q] : 0.0;
          if (!(x[q] >= 0.0 && isfinite(x[q]))) err |= DM_ERR_W;
        }
        const double v = stb_wave_sum((x[0] + x[1]) + (x[2] + x[3]));
        if (lane == 0) schunk[c] = v;
      }
      __syncthreads();
      if (tid == 0)
        for (unsigned c = 0; c < cn; c++) dd_add(acc, schunk[c]);
      __syncthreads();
    }
    W = acc.hi + acc.lo;  // (thread 0's)
  }
  if (err) __hip_atomic_fetch_or(&ctl[DM_CTL_ERR], err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == 0) {
    if (!(W > 0.0 && isfinite(W))) __hip_atomic_fetch_or(&ctl[DM_CTL_ERR], DM_ERR_TOTAL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    double *wl = (double *)ctl + DM_CTL_W;
    wl[0] = W;
    wl[1] = lgamma(W);
  }
}

// the block's two sums (sx[0], sx[1] hold its 256 values), one fixed tree each, to out[0], out[1]
__device__ __forceinline__ void dm_block_sums(const double (*sx)[DM_BLOCK], unsigned wave, unsigned lane, unsigned nw, double *out) {
#pragma clang fp contract(off)
  for (unsigned q = wave; q < 2; q += nw) {
    const double *x = sx[q];
    const double v = stb_wave_sum((x[lane] + x[lane + 64]) + (x[lane + 128] + x[lane + 192]));
    if (lane == 0) out[q] = v;
  }
}

// one row by its wave, the code both rows kernels run (their bits must agree): the cells in chunks of 64, a chunk by the
// shuffle tree, the chunk sums in order in double-double.  Returns cells = hi + lo; *C the row's count, *any whether it
// holds an impossible cell (both valid in lane 0)
__device__ __forceinline__ double dm_row(const uint32_t *row, unsigned cols, const double *wv, double s, double wconst, unsigned lane,
                                         dm_counts &n, unsigned long long *C, bool *any) {
#pragma clang fp contract(off)
  dd_t acc{0.0, 0.0};
  unsigned long long sum = 0;
  bool bad = false;
  for (unsigned base = 0; base < cols; base += 64) {
    const unsigned k = base + lane;
    double x = 0.0;
    if (k < cols) {
      const unsigned c = row[k];
      const double w = wv ? s * wv[k] : wconst;
      sum += c;
      x = dm_visit(w, c, n, &bad);
    }
    dd_add(acc, stb_wave_sum(x));
    if (cols - base <= 64) break;  // (base + 64 may wrap)
  }
  *C = stb_wave_sum(sum);
  *any = __ballot(bad) != 0ull;
  return acc.hi + acc.lo;
}

__global__ __launch_bounds__(DM_MAXTHREADS) void k_dm_rows(const uint32_t *cnt, uint64_t rows, unsigned cols, unsigned stride,
                                                           const double *wv, double w0, double scale, const double *d_scale,
                                                           double *each, double *partial, unsigned nblk, unsigned *ctl,
                                                           double *host) {
#pragma clang fp contract(off)
  __shared__ double sx[2][DM_BLOCK];  // cells, normaliser of the block's rows
  __shared__ unsigned long long sC[DM_BLOCK];
  __shared__ unsigned sflag[DM_BLOCK];
  __shared__ double stage[2][DM_STAGE];
  __shared__ unsigned s_last;
  const unsigned nthr = blockDim.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nw = nthr >> 6;
  const double s = d_scale ? *d_scale : scale;
  const double wconst = s * w0;
  const double W = ((const double *)ctl)[DM_CTL_W], lgW = ((const double *)ctl)[DM_CTL_W + 1];
  dm_counts n;
  for (unsigned blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const uint64_t r0 = (uint64_t)blk * DM_BLOCK;
    // ---- the cells: a wave a row
    for (unsigned r = wave; r < DM_BLOCK && r0 + r < rows; r += nw) {
      unsigned long long C;
      bool any;
      const double cells = dm_row(cnt + (r0 + r) * stride, cols, wv, s, wconst, lane, n, &C, &any);
      if (lane == 0) {
        sx[0][r] = cells;
        sC[r] = C;
        sflag[r] = any ? 1u : 0u;
      }
    }
    __syncthreads();
    // ---- the normalisers: a lane a row
    for (unsigned r = tid; r < DM_BLOCK; r += nthr) {
      if (r0 + r < rows) {
        const double nm = dm_norm(W, lgW, sC[r]);
        sx[1][r] = nm;
        if (each) each[r0 + r] = sflag[r] ? -HUGE_VAL : sx[0][r] + nm;
      } else {
        sx[0][r] = 0.0;
        sx[1][r] = 0.0;
      }
    }
    __syncthreads();
    dm_block_sums(sx, wave, lane, nw, partial + (size_t)blk * 2);
    __syncthreads();
  }
  dm_publish_counts(n, lane, ctl);
  if (!stb_ticket_last(ctl, gridDim.x, &s_last)) return;
  dd_t acc{0.0, 0.0};  // threads 0, 1: one component each
  for (unsigned c0 = 0; c0 < nblk; c0 += DM_STAGE) {
    const unsigned cn = nblk - c0 < DM_STAGE ? nblk - c0 : DM_STAGE;
    for (unsigned e = tid; e < cn * 2; e += nthr) stage[e & 1][e >> 1] = partial[(size_t)c0 * 2 + e];
    __syncthreads();
    if (tid < 2)
      for (unsigned c = 0; c < cn; c++) dd_add(acc, stage[tid][c]);
    __syncthreads();
  }
  if (wave != 0) return;
  dd_t norms;
  norms.hi = __shfl(acc.hi, 1, 64);
  norms.lo = __shfl(acc.lo, 1, 64);
  if (tid == 0) dm_answer(acc, norms, ctl, host);
}

// rows orientation when the rows are few (fewer blocks than would fill the part): the waves of the whole grid take the rows
// one at a time, row values go to rowval[row][2], and the last workgroup to finish sums the blocks.  The same values in the
// same association as k_dm_rows: no bit differs (STB_DIRMULT_FORM = fused | split forces one of the two)
__global__ __launch_bounds__(DM_MAXTHREADS) void k_dm_rows_split(const uint32_t *cnt, uint64_t rows, unsigned cols, unsigned stride,
                                                                 const double *wv, double w0, double scale, const double *d_scale,
                                                                 double *each, double *rowval, unsigned nblk, unsigned *ctl,
                                                                 double *host) {
#pragma clang fp contract(off)
  __shared__ double stage[2][DM_STAGE];
  __shared__ unsigned s_last;
  const unsigned nthr = blockDim.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nw = nthr >> 6;
  const double s = d_scale ? *d_scale : scale;
  const double wconst = s * w0;
  const double W = ((const double *)ctl)[DM_CTL_W], lgW = ((const double *)ctl)[DM_CTL_W + 1];
  dm_counts n;
  for (uint64_t r = (uint64_t)blockIdx.x * nw + wave; r < rows; r += (uint64_t)gridDim.x * nw) {
    unsigned long long C;
    bool any;
    const double cells = dm_row(cnt + r * stride, cols, wv, s, wconst, lane, n, &C, &any);
    if (lane == 0) {
      const double nm = dm_norm(W, lgW, C);
      rowval[2 * r] = cells;
      rowval[2 * r + 1] = nm;
      if (each) each[r] = any ? -HUGE_VAL : cells + nm;
    }
  }
  dm_publish_counts(n, lane, ctl);
  if (!stb_ticket_last(ctl, gridDim.x, &s_last)) return;
  // the blocks' trees a wave each (its lanes read the block's 256 values themselves), a stage of block sums at a time;
  // threads 0 and 1 add a component each in block order
  dd_t acc{0.0, 0.0};
  for (unsigned c0 = 0; c0 < nblk; c0 += DM_STAGE) {
    const unsigned cn = nblk - c0 < DM_STAGE ? nblk - c0 : DM_STAGE;
    for (unsigned b = wave; b < cn; b += nw) {
      const uint64_t r0 = (uint64_t)(c0 + b) * DM_BLOCK + lane;
#pragma unroll
      for (unsigned q = 0; q < 2; q++) {
        double x[4];
#pragma unroll
        for (unsigned j = 0; j < 4; j++) x[j] = r0 + 64 * j < rows ? rowval[2 * (r0 + 64 * j) + q] : 0.0;
        const double v = stb_wave_sum((x[0] + x[1]) + (x[2] + x[3]));
        if (lane == 0) stage[q][b] = v;
      }
    }
    __syncthreads();
    if (tid < 2)
      for (unsigned c = 0; c < cn; c++) dd_add(acc, stage[tid][c]);
    __syncthreads();
  }
  if (wave != 0) return;
  dd_t norms;
  norms.hi = __shfl(acc.hi, 1, 64);
  norms.lo = __shfl(acc.lo, 1, 64);
  if (tid == 0) dm_answer(acc, norms, ctl, host);
}

// workgroup (x, y): the columns 64 x .. 64 x + 63; its wave v the chunks y nw + v, then + gridDim.y nw, ...
__global__ __launch_bounds__(DM_MAXTHREADS) void k_dm_cols(const uint32_t *cnt, uint64_t rows, unsigned cols, unsigned stride,
                                                           const double *wv, double w0, double scale, const double *d_scale,
                                                           double *each, double *csum, unsigned long long *ccnt,
                                                           unsigned *colflag, double *colval, unsigned nchunks, unsigned *ctl,
                                                           double *host) {
#pragma clang fp contract(off)
  __shared__ double sx[2][DM_BLOCK];
  __shared__ double sblk[2];
  __shared__ unsigned s_last;
  const unsigned nthr = blockDim.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nw = nthr >> 6;
  const double s = d_scale ? *d_scale : scale;
  const double wconst = s * w0;
  const unsigned k = blockIdx.x * 64 + lane;
  const bool live = k < cols;  // (no lane leaves: the ticket's barriers need them all)
  dm_counts n;
  bool bad = false;
  for (unsigned c = blockIdx.y * nw + wave; c < nchunks; c += gridDim.y * nw) {
    const uint64_t j0 = (uint64_t)c * DM_BLOCK, j1 = j0 + DM_BLOCK < rows ? j0 + DM_BLOCK : rows;
    double sum = 0.0;
    unsigned long long C = 0;
    if (live) {
      const uint32_t *p = cnt + j0 * stride + k;
      for (uint64_t j = j0; j < j1; j += 8, p += (size_t)8 * stride) {  // eight loads in flight ahead of the terms
        unsigned cc[8];
#pragma unroll
        for (unsigned q = 0; q < 8; q++) cc[q] = j + q < j1 ? p[(size_t)q * stride] : 0u;
#pragma unroll
        for (unsigned q = 0; q < 8; q++) {
          if (j + q >= j1) break;
          const double w = wv ? s * wv[j + q] : wconst;
          C += cc[q];
          if (cc[q])  // (a zero cell's 0.0 changes no bit of the sum)
            sum = sum + dm_visit(w, cc[q], n, &bad);
          else if (w == 0.0)
            n.zw++;
        }
      }
      csum[(size_t)c * cols + k] = sum;
      ccnt[(size_t)c * cols + k] = C;
    }
  }
  if (live && bad) __hip_atomic_fetch_or(&colflag[k], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  dm_publish_counts(n, lane, ctl);
  if (!stb_ticket_last(ctl, gridDim.x * gridDim.y, &s_last)) return;
  const double W = ((const double *)ctl)[DM_CTL_W], lgW = ((const double *)ctl)[DM_CTL_W + 1];
  dd_t accC{0.0, 0.0}, accN{0.0, 0.0};  // (thread 0's)
  // every column's value first, the threads strided over the columns; then the blocks of 256 columns
  for (unsigned kk = tid; kk < cols; kk += nthr) {
    dd_t acc{0.0, 0.0};
    unsigned long long C = 0;
#pragma unroll 8
    for (unsigned c = 0; c < nchunks; c++) {
      dd_add(acc, csum[(size_t)c * cols + kk]);
      C += ccnt[(size_t)c * cols + kk];
    }
    const double cells = acc.hi + acc.lo, nm = dm_norm(W, lgW, C);
    const unsigned flag = __hip_atomic_load(&colflag[kk], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (each) each[kk] = flag ? -HUGE_VAL : cells + nm;
    colval[2 * (size_t)kk] = cells;
    colval[2 * (size_t)kk + 1] = nm;
    if (cols - kk <= nthr) break;  // (kk + nthr may wrap)
  }
  __syncthreads();  // (colval is this workgroup's own: its stores are visible to it behind the barrier)
  for (unsigned k0 = 0; k0 < cols; k0 += DM_BLOCK) {
    for (unsigned r = tid; r < DM_BLOCK; r += nthr) {
      const bool in = r < cols - k0;
      sx[0][r] = in ? colval[2 * (size_t)(k0 + r)] : 0.0;
      sx[1][r] = in ? colval[2 * (size_t)(k0 + r) + 1] : 0.0;
    }
    __syncthreads();
    dm_block_sums(sx, wave, lane, nw, sblk);
    __syncthreads();
    if (tid == 0) {
      dd_add(accC, sblk[0]);
      dd_add(accN, sblk[1]);
    }
    if (cols - k0 <= DM_BLOCK) break;  // (k0 + 256 may wrap)
    __syncthreads();
  }
  if (tid == 0) dm_answer(accC, accN, ctl, host);
}

// log p(r | gamma) = lgamma(sum gamma) - sum lgamma(gamma_k) + sum (gamma_k - 1) log(r_k / R) of a root of K <= 1024 cells,
// one workgroup.  G = gamma_0 + gamma_1 + .. and R = r_0 + r_1 + .. in k order, plain; A = sum lgamma(gamma_k) and
// B = sum (gamma_k - 1.0) * log(r_k / R) in k order in double-double, hi + lo each; the value is (lgamma(G) - A) + B.
// Cells with r_k = 0 are left out of B and counted.  root NULL: every r_k is 1.0 / (double)K; gam NULL: every gamma_k
// is gamma0.  out[0] the value, out[1] (u64) the cells left out.
__global__ __launch_bounds__(DM_MAXTHREADS) void k_dm_root(unsigned K, const double *root, const double *gam, double gamma0,
                                                           double *out) {
#pragma clang fp contract(off)
  __shared__ double sa[STB_TD_MAXK], sb[STB_TD_MAXK];
  __shared__ double s_R;
  __shared__ unsigned s_left;
  const unsigned tid = threadIdx.x, nthr = blockDim.x;
  const double r0 = 1.0 / (double)K;
  if (tid == 0) {
    double R = root ? root[0] : r0;
    for (unsigned k = 1; k < K; k++) R = R + (root ? root[k] : r0);
    s_R = R;
    s_left = 0;
  }
  __syncthreads();
  const double R = s_R;
  unsigned left = 0;
  for (unsigned k = tid; k < K; k += nthr) {
    const double g = gam ? gam[k] : gamma0, r = root ? root[k] : r0;
    sa[k] = lgamma(g);
    if (r > 0.0) {
      sb[k] = (g - 1.0) * log(r / R);
    } else {
      sb[k] = 0.0;
      left++;
    }
  }
  if (left) atomicAdd(&s_left, left);
  __syncthreads();
  if (tid == 0) {
    double G = gam ? gam[0] : gamma0;
    for (unsigned k = 1; k < K; k++) G = G + (gam ? gam[k] : gamma0);
    dd_t A{0.0, 0.0}, B{0.0, 0.0};
    for (unsigned k = 0; k < K; k++) {
      dd_add(A, sa[k]);
      dd_add(B, sb[k]);
    }
    out[0] = (lgamma(G) - (A.hi + A.lo)) + (B.hi + B.lo);
    ((unsigned long long *)out)[1] = s_left;
  }
}

// ------------------------------------------------------------------------------------------------
// host side.  The scratch comes from the buffer cache and goes back behind the call's one wait.

struct dm_scratch {
  void *d = nullptr, *h = nullptr, *h_dev = nullptr;
  hipStream_t st = nullptr;
  bool queued = false;  // work that uses the buffers may be on st: wait before the cache hands them on
  ~dm_scratch() {
    if (queued) (void)hipStreamSynchronize(st);
    if (d) stb_pool_free(d);
    if (h) stb_pool_free(h);
  }
};

static size_t dm_up(size_t x) { return (x + 255) & ~(size_t)255; }

static unsigned dm_waves() {
  return (unsigned)stb_env_waves("STB_DIRMULT_WAVES", 4);
}

static void dm_clear(stb_dirmult_info_t *info) {
  if (info) memset(info, 0, sizeof(*info));
}

int stb_dm_check(const uint32_t *d_cnt, unsigned cols, unsigned stride, unsigned flags, const double *d_w, double w0, double scale,
                 const double *d_scale, const double *total_host, const char *who) {
  if (!d_cnt || !total_host) return stb_fail("%s: d_cnt and total_host are required", who);
  if (cols < 1 || cols > stride) return stb_fail("%s: cols=%u, stride=%u (1 <= cols <= stride)", who, cols, stride);
  if (flags != STB_DM_ROWS && flags != STB_DM_COLUMNS)
    return stb_fail("%s: flags=0x%x (exactly one of STB_DM_ROWS, STB_DM_COLUMNS)", who, flags);
  if (!d_w && (!(w0 > 0.0) || !std::isfinite(w0))) return stb_fail("%s: w0=%g (must be > 0 and finite)", who, w0);
  if (!d_scale && (!(scale > 0.0) || !std::isfinite(scale))) return stb_fail("%s: scale=%g (must be > 0 and finite)", who, scale);
  return 0;
}

int stb_dm_run(const uint32_t *d_cnt, uint64_t rows, unsigned cols, unsigned stride, unsigned flags, const double *d_w, double w0,
               double scale, const double *d_scale, double *d_each, double *total_host, stb_dirmult_info_t *info, hipStream_t st,
               const char *who) {
  if (rows == 0) {
    *total_host = 0.0;
    dm_clear(info);
    return 0;
  }
  if (stb_device_count() < 1) return stb_no_device(who);
  const bool by_rows = flags == STB_DM_ROWS;
  const uint64_t nunits = (rows + DM_BLOCK - 1) / DM_BLOCK;  // blocks of rows, or chunks of rows
  if (nunits > 0x7fffffffull) return stb_fail("%s: rows=%llu", who, (unsigned long long)rows);
  const unsigned nw = dm_waves(), cus = (unsigned)(stb_cu_count() > 0 ? stb_cu_count() : 1);
  // few rows: their blocks of 256 would leave most of the part idle, so the grid's waves take the rows one by one.  A row
  // then pays its normaliser on one lane, which long rows hide and short ones do not (MEASUREMENTS section C1: 10^5 rows
  // of 64 cells 0.21 ms fused, 0.41 ms split; of 1024 cells 2.34 ms fused, 1.92 ms split)
  const char *form = getenv("STB_DIRMULT_FORM");
  const bool few = nunits < cus / 4 || (cols > 256 && nunits < (uint64_t)DM_GRID_PER_CU * cus);
  const bool split = by_rows && (form && !strcmp(form, "split") ? true : form && !strcmp(form, "fused") ? false : few);
  // scratch: ctl (256 bytes) and, for columns, a flag word a column -- zeroed; then the block sums (split: the rows' values),
  // or the chunks' sums, their counts and the columns' values
  const size_t o_flag = 256, o_sum = o_flag + (by_rows ? 0 : dm_up(4 * (size_t)cols)),
               o_cnt = o_sum + dm_up(8 * (by_rows ? (split ? 2 * (size_t)rows : 2 * (size_t)nunits) : (size_t)nunits * cols)),
               o_val = o_cnt + (by_rows ? 0 : dm_up(8 * (size_t)nunits * cols)), bytes = o_val + (by_rows ? 0 : dm_up(16 * (size_t)cols));
  dm_scratch sc;
  sc.st = st;
  if (stb_pool_malloc(&sc.d, bytes) != hipSuccess || stb_pool_malloc(&sc.h, 256, 1) != hipSuccess ||
      hipHostGetDevicePointer(&sc.h_dev, sc.h, 0) != hipSuccess)
    return stb_fail("%s: out of memory for %zu bytes of scratch", who, bytes);
  char *d = (char *)sc.d;
  unsigned *ctl = (unsigned *)d, *colflag = (unsigned *)(d + o_flag);
  double *sums = (double *)(d + o_sum);
  unsigned long long *ccnt = (unsigned long long *)(d + o_cnt);
  volatile unsigned long long *hc = (volatile unsigned long long *)sc.h;
  hc[7] = 0xffffffffull;
  sc.queued = true;
  HIPCHK(hipMemsetAsync(d, 0, o_sum, st));
  STB_LAUNCH(k_dm_weights, dim3(1), dim3(DM_BLOCK), st, d_w, by_rows ? (uint64_t)cols : rows, w0, scale, d_scale, ctl);
  if (split) {
    const uint64_t want = (rows + nw - 1) / nw, cap = (uint64_t)DM_GRID_PER_CU * cus;
    STB_LAUNCH(k_dm_rows_split, dim3((unsigned)(want < cap ? want : cap)), dim3(64 * nw), st, d_cnt, rows, cols, stride, d_w, w0,
               scale, d_scale, d_each, sums, (unsigned)nunits, ctl, (double *)sc.h_dev);
  } else if (by_rows) {
    const unsigned nblk = (unsigned)nunits, cap = DM_GRID_PER_CU * cus, grid = nblk < cap ? nblk : cap;
    STB_LAUNCH(k_dm_rows, dim3(grid), dim3(64 * nw), st, d_cnt, rows, cols, stride, d_w, w0, scale, d_scale, d_each, sums, nblk,
               ctl, (double *)sc.h_dev);
  } else {
    const unsigned nchunks = (unsigned)nunits, cb = (cols + 63) / 64;
    // (the last workgroup takes the columns a thread each: eight waves where there are that many and nobody asked otherwise)
    const unsigned nwc = !getenv("STB_DIRMULT_WAVES") && cols >= 512 ? 8u : nw;
    const uint64_t want = ((uint64_t)nchunks + nwc - 1) / nwc, cap = (uint64_t)DM_GRID_PER_CU * cus / cb + 1;
    const uint64_t gy = want < cap ? want : cap;
    STB_LAUNCH(k_dm_cols, dim3(cb, (unsigned)(gy > 65535 ? 65535 : gy)), dim3(64 * nwc), st, d_cnt, rows, cols, stride, d_w, w0,
               scale, d_scale, d_each, sums, ccnt, colflag, (double *)(d + o_val), nchunks, ctl, (double *)sc.h_dev);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  sc.queued = false;
  const volatile double *h = (const volatile double *)sc.h;
  const unsigned err = (unsigned)hc[7];
  *total_host = h[0];
  if (info) {
    info->cells = h[1];
    info->norms = h[2];
    info->nonzero = hc[3];
    info->count = hc[4];
    info->zero_weight = hc[5];
    info->impossible = hc[6];
    info->error_word = err;
    info->reserved = 0;
  }
  if (err)
    return stb_fail("%s: failed, error word 0x%x (1: a weight or the scale is negative, NaN or infinite; 2: the sum of the "
                    "weights is not positive and finite); the outputs are undefined", who, err);
  return 0;
}

static_assert(STB_DM_CTL_ERR == DM_CTL_ERR && STB_DM_CTL_W == DM_CTL_W, "dirmult.h describes k_dm_weights' words");

int stb_dm_weights_queue(const double *d_w, uint64_t ncat, double w0, unsigned *ctl, hipStream_t st) {
  STB_LAUNCH(k_dm_weights, dim3(1), dim3(DM_BLOCK), st, d_w, ncat, w0, 1.0, (const double *)nullptr, ctl);
  HIPCHK(hipGetLastError());
  return 0;
}

int stb_dm_root_queue(unsigned K, const double *d_root, const double *d_gamma, double gamma0, double *out_dev, hipStream_t st) {
  const unsigned nw = dm_waves(), cb = (K + 63) / 64;
  STB_LAUNCH(k_dm_root, dim3(1), dim3(64 * (nw < cb ? nw : cb)), st, K, d_root, d_gamma, gamma0, out_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int stb_dirmult_logml(const uint32_t *d_cnt, uint64_t rows, unsigned cols, unsigned stride, unsigned flags,
                                 const double *d_w, double w0, double scale, const double *d_scale, double *d_each,
                                 double *total_host, stb_dirmult_info_t *info, void *stream) {
  STB_ENTRY;
  const char *who = "stb_dirmult_logml";
  if (stb_dm_check(d_cnt, cols, stride, flags, d_w, w0, scale, d_scale, total_host, who)) return 1;
  return stb_dm_run(d_cnt, rows, cols, stride, flags, d_w, w0, scale, d_scale, d_each, total_host, info, (hipStream_t)stream, who);
}
