// dirconc.hip -- the scale of Dirichlet weights shared by many multinomials, resampled on the device in one exact Gibbs
// step (include/stb_hip.h, stb_sample_dirconc).  Multinomial mu has counts c_mu,j under weights
// w_j = s v_j; V = sum_j v_j, n_mu = sum_j c_mu,j, the prior is s ~ Gamma(shape, scale):
//     p(s | c) ~ p(s) prod_mu Gamma(sV) / Gamma(sV + n_mu) prod_j Gamma(s v_j + c_mu,j) / Gamma(s v_j)
//     m_mu,j | c, s     Antoniak: [c >= 1] + sum_{i=1}^{c - 1} Bernoulli(s v_j / (s v_j + i))           (hg_cell.h)
//     B' | m, n         Teh's auxiliaries on B = sV, whose prior is Gamma(shape, scale V): stb_sample_bgroups with a = 0, a
//                       "restaurant" per multinomial (N = n_mu, T = M_mu = sum_j m_mu,j), one group, every b = B
//     s' = B' / V
// The count matrix is stb_dirmult_logml's: rows x stride uint32, the first cols columns the matrix; STB_DM_ROWS a
// multinomial a row (the table counts of groups of restaurants: the base weights' concentration), STB_DM_COLUMNS a
// multinomial a column over class-major rows (the (class, dish) counts: the class distributions' beta).
//
//   k_dm_weights       (dirmult.hip) V in stb_dirmult_logml's association, scale 1, and the checks of v
//   k_dc_totals        columns: n_mu, lanes along the columns, a wave a chunk of 256 rows, one atomic a (chunk, column);
//   k_dc_totals_rows   rows: a wave a row.  Both count the cells with v = 0 and flag those of them that hold a count
//   k_dc_prep          n_mu as hyperb's N and the 2^32 check, B for every multinomial, the one range, 1 / (scale V)
//   k_dc_aux_cols      m and M_mu, columns: lanes along the columns -- a matrix row is read coalesced -- a wave a chunk of
//                      256 rows; a zero cell costs its read; a cell with <= HG_TWAVE draws is its lane's, a larger one the
//                      whole wave's (k_hg_aux's ballot loop); a lane keeps its column's sum over the chunk, one atomic a
//                      (chunk, column); where the (chunk, column block) jobs are fewer than the waves that fit the part,
//                      each is taken by `parts` waves: a row of the chunk is one part's, but for its cells with more than
//                      DC_TSLICE draws, of which every part takes a slice
//   k_dc_aux_rows      the same, rows: k_hg_aux's shape, lanes along the categories, a wave a row
//   k_dc_finish        s' = B' / V, the totals, the error word to pinned words
// queued back to back with hyperb's three launches (hyperb.h) between prep and finish; one wait.  No kernel waits for
// another workgroup.  Once the error word is set -- a total above 2^32 - 1 above all: its draws would take hours -- the
// aux kernels return at once and make no draw.
//
// Streams: key = mix(seed + (sweep+1) gamma).  Cell e = mu cols + j (rows: stb_sample_hgroups' g Kmax + k) or j stride + mu
// (columns: stb_sample_lik's w stride + k) owns u_i = element i of mix(mix(key + (e+1) gamma) ^ HG_SALT_Y).  The
// concentration is hyperb's step on seed ^ HG_SALT_A.  FP64, no contraction: w = s v_j, B = s V, scale_B = scale V and
// 1.0 / scale_B are one operation each; s' = B' / V is one division.  m, M and n are integers (atomics), so no bit depends
// on STB_DIRCONC_WAVES = 1, 2, 4 or 8 waves a workgroup (default 4) or on STB_DIRCONC_FORM = lane | wave.
//
// Bounds: every kernel reads cnt[r stride + k] and writes m at the same index for r < rows, k < cols <= stride; d_w[r]
// (columns) or d_w[k] (rows); n, M, N32, B, L, Y at mu < the number of multinomials.

#include <climits>
#include <cmath>
#include <cstring>

#include "stb_common.h"
#include "dirmult.h"
#include "hyperb.h"
#include "hg_cell.h"
#include "dirconc.h"
#include "ticket.h"

#pragma clang fp contract(off)

#define DC_CHUNK 256u      // rows of a chunk (k_dm_cols')
#define DC_MAXTHREADS 512
#define DC_PARTS_MAX 64u   // waves that share a job at most
#define DC_TSLICE 16384u   // columns: a cell with more draws than this is cut into slices over the parts of its job
#define DC_ERR_W 1u        // (k_dm_weights' bits, as they are)
#define DC_ERR_V 2u
#define DC_ERR_ZERO 4u
#define DC_ERR_TOTAL 8u
// ctl (256 bytes, zeroed ahead of the launches): u32 [0] the error word; u64 [1] cells with v = 0 and c = 0; k_dm_weights'
// words (dirmult.h); doubles [18] 1 / (scale V), [19] B
#define DC_CTL_ZW 1
#define DC_CTL_INV 18
#define DC_CTL_B 19
// host (pinned), u64: [0] the error word, [1] s' (a double's bits), [2] sum n, [3] sum M, [4] multinomials with n > 0,
// [5] zero-weight cells

__device__ __forceinline__ void dc_publish(unsigned long long zw, bool bad, unsigned lane, unsigned *ctl) {
  zw = stb_wave_sum(zw);
  if (lane == 0 && zw) __hip_atomic_fetch_add(&((unsigned long long *)ctl)[DC_CTL_ZW], zw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (bad) __hip_atomic_fetch_or(&ctl[0], DC_ERR_ZERO, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// workgroup (x, y): the columns 64 x .. 64 x + 63; its wave v the chunks y nw + v, then + gridDim.y nw, ...
__global__ __launch_bounds__(DC_MAXTHREADS) void k_dc_totals(const uint32_t *cnt, uint64_t rows, unsigned cols, unsigned stride,
                                                             const double *wv, unsigned nchunks, unsigned long long *n,
                                                             unsigned *ctl) {
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const unsigned k = blockIdx.x * 64 + lane;
  const bool live = k < cols;
  unsigned long long zw = 0;
  bool bad = false;
  for (unsigned c = blockIdx.y * nw + wave; c < nchunks; c += gridDim.y * nw) {
    const uint64_t j0 = (uint64_t)c * DC_CHUNK, j1 = j0 + DC_CHUNK < rows ? j0 + DC_CHUNK : rows;
    unsigned long long sum = 0;
    if (live) {
      const uint32_t *p = cnt + j0 * stride + k;
      for (uint64_t j = j0; j < j1; j += 8, p += (size_t)8 * stride) {  // eight loads in flight
        unsigned cc[8];
#pragma unroll
        for (unsigned q = 0; q < 8; q++) cc[q] = j + q < j1 ? p[(size_t)q * stride] : 0u;
#pragma unroll
        for (unsigned q = 0; q < 8; q++) {
          if (j + q >= j1) break;
          sum += cc[q];
          if (wv && wv[j + q] == 0.0) {  // (uniform over the wave)
            if (cc[q]) bad = true; else zw++;
          }
        }
      }
      if (sum) atomicAdd(&n[k], sum);
    }
  }
  dc_publish(zw, bad, lane, ctl);
}

// wave v of the grid the rows v, v + the grid's waves, ...; lanes strided over the row's cells
__global__ __launch_bounds__(DC_MAXTHREADS) void k_dc_totals_rows(const uint32_t *cnt, uint64_t rows, unsigned cols, unsigned stride,
                                                                  const double *wv, unsigned long long *n, unsigned *ctl) {
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  unsigned long long zw = 0;
  bool bad = false;
  for (uint64_t r = (uint64_t)blockIdx.x * nw + wave; r < rows; r += (uint64_t)gridDim.x * nw) {
    const uint32_t *row = cnt + r * stride;
    unsigned long long sum = 0;
    for (unsigned base = 0; base < cols; base += 64) {
      const unsigned k = base + lane;
      if (k < cols) {
        const unsigned cc = row[k];
        sum += cc;
        if (wv && wv[k] == 0.0) {
          if (cc) bad = true; else zw++;
        }
      }
      if (cols - base <= 64) break;  // (base + 64 may wrap)
    }
    sum = stb_wave_sum(sum);
    if (lane == 0) n[r] = sum;
  }
  dc_publish(zw, bad, lane, ctl);
}

__global__ __launch_bounds__(256) void k_dc_prep(uint64_t nm, const unsigned long long *n, double s, double scale, uint32_t *N32,
                                                 double *B, uint64_t *goff1, unsigned *ctl) {
#pragma clang fp contract(off)
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const double V = ((const double *)ctl)[STB_DM_CTL_W];
  const double b = s * V;
  if (g == 0) {
    const double scale_B = scale * V;
    ((double *)ctl)[DC_CTL_INV] = 1.0 / scale_B;
    ((double *)ctl)[DC_CTL_B] = b;
    goff1[0] = 0;
    goff1[1] = nm;
    const unsigned e = ctl[STB_DM_CTL_ERR];
    if (e) __hip_atomic_fetch_or(&ctl[0], e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (g >= nm) return;
  const unsigned long long C = n[g];
  if (C > 0xffffffffull) __hip_atomic_fetch_or(&ctl[0], DC_ERR_TOTAL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  N32[g] = (uint32_t)C;
  B[g] = b;
}

// workgroup (x, y): the columns 64 x .. 64 x + 63; its wave v the jobs q = y nw + v, then + gridDim.y nw, ...; job q is
// part q % parts of chunk q / parts.  m arrives zeroed (null: not wanted)
__global__ __launch_bounds__(DC_MAXTHREADS) void k_dc_aux_cols(const uint32_t *cnt, uint64_t rows, unsigned cols, unsigned stride,
                                                               const double *wv, double w0, double s, uint64_t key,
                                                               unsigned twave, unsigned parts, unsigned nchunks,
                                                               const unsigned *ctl, uint32_t *m, uint32_t *M) {
#pragma clang fp contract(off)
  if (__hip_atomic_load(&ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return;  // (uniform: no draws)
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const unsigned k = blockIdx.x * 64 + lane;
  const bool live = k < cols;  // (no lane leaves: the wave's shuffles need them all)
  const double wconst = s * w0;
  for (uint64_t q = (uint64_t)blockIdx.y * nw + wave; q < (uint64_t)nchunks * parts; q += (uint64_t)gridDim.y * nw) {
    const uint64_t c = q / parts;
    const unsigned p = (unsigned)(q % parts);
    const uint64_t j0 = c * DC_CHUNK, j1 = j0 + DC_CHUNK < rows ? j0 + DC_CHUNK : rows;
    unsigned col = 0;  // (at most the column's total, which fits: k_dc_prep checked)
    for (uint64_t j = j0; j < j1; j += 8) {
      unsigned cc[8];
#pragma unroll
      for (unsigned r = 0; r < 8; r++) cc[r] = live && j + r < j1 ? cnt[(j + r) * stride + k] : 0u;
#pragma unroll
      for (unsigned r = 0; r < 8; r++) {
        if (j + r >= j1) break;  // (uniform)
        if (__ballot(cc[r] != 0u) == 0ull) continue;  // (uniform) a row of zero cells
        const double w = wv ? s * wv[j + r] : wconst;
        const uint64_t e = (j + r) * stride + k;
        const uint64_t ky = cc[r] >= 2 ? stb_mix64(stb_mix64(key + (e + 1) * STB_GAMMA) ^ HG_SALT_Y) : 0;
        // the row's cells go whole to part (row % parts), but for those with more than DC_TSLICE draws, which every part
        // takes a slice of: a dense chunk then costs a part its own rows, not every row's shuffles
        const bool huge = cc[r] >= 2 && cc[r] - 1 > DC_TSLICE;
        unsigned mm = 0;
        if (p == (unsigned)((j + r) % parts)) mm = hg_cell(huge ? 0u : cc[r], w, ky, 0u, 1u, twave, lane);  // (uniform)
        if (__ballot(huge) != 0ull) mm += hg_cell(huge ? cc[r] : 0u, w, ky, p, parts, twave, lane);
        if (mm && m) {
          if (parts == 1) m[e] = mm;
          else atomicAdd(&m[e], mm);
        }
        col += mm;
      }
    }
    if (live && col) atomicAdd(&M[k], col);
  }
}

// workgroup (x, y): the categories 64 x .. 64 x + 63; its wave v the jobs q = y nw + v, ...: part q % parts of row q / parts
__global__ __launch_bounds__(DC_MAXTHREADS) void k_dc_aux_rows(const uint32_t *cnt, uint64_t rows, unsigned cols, unsigned stride,
                                                               const double *wv, double w0, double s, uint64_t key,
                                                               unsigned twave, unsigned parts, const unsigned *ctl, uint32_t *m,
                                                               uint32_t *M) {
#pragma clang fp contract(off)
  if (__hip_atomic_load(&ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return;
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const unsigned k = blockIdx.x * 64 + lane;
  const bool live = k < cols;
  const double w = live ? s * (wv ? wv[k] : w0) : 1.0;
  for (uint64_t q = (uint64_t)blockIdx.y * nw + wave; q < rows * parts; q += (uint64_t)gridDim.y * nw) {
    const uint64_t g = q / parts;
    const unsigned p = (unsigned)(q % parts);
    const unsigned cc = live ? cnt[g * stride + k] : 0u;
    const uint64_t e = g * cols + k;
    const uint64_t ky = cc >= 2 ? stb_mix64(stb_mix64(key + (e + 1) * STB_GAMMA) ^ HG_SALT_Y) : 0;
    const unsigned mm = hg_cell(cc, w, ky, p, parts, twave, lane);
    if (mm && m) {
      if (parts == 1) m[g * stride + k] = mm;
      else atomicAdd(&m[g * stride + k], mm);
    }
    unsigned row = mm;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) row += __shfl_down(row, off, 64);
    if (lane == 0 && row) atomicAdd(&M[g], row);
  }
}

// one workgroup: the totals over the multinomials, s' = B' / V, then the words the host waits for
__global__ __launch_bounds__(256) void k_dc_finish(uint64_t nm, const unsigned long long *n, const uint32_t *M, const double *B,
                                                   const unsigned *ctl, unsigned long long *host_out) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_n, s_m, s_nz;
  if (threadIdx.x == 0) s_n = s_m = s_nz = 0;
  __syncthreads();
  unsigned long long ns = 0, ms = 0, nz = 0;
  for (uint64_t g = threadIdx.x; g < nm; g += 256) {
    ns += n[g];
    ms += M[g];
    nz += n[g] ? 1u : 0u;
  }
  if (ns) atomicAdd(&s_n, ns);
  if (ms) atomicAdd(&s_m, ms);
  if (nz) atomicAdd(&s_nz, nz);
  __syncthreads();
  if (threadIdx.x == 0) {
    const double V = ((const double *)ctl)[STB_DM_CTL_W];
    const double s1 = B[0] / V;
    host_out[0] = ctl[0];
    host_out[1] = (unsigned long long)__double_as_longlong(s1);
    host_out[2] = s_n;
    host_out[3] = s_m;
    host_out[4] = s_nz;
    host_out[5] = ((const unsigned long long *)ctl)[DC_CTL_ZW];
  }
}

// ------------------------------------------------------------------------------------------------
// host side.  The scratch comes from the buffer cache and goes back behind the call's one wait.

struct dc_scratch {
  void *d = nullptr, *h = nullptr, *h_dev = nullptr;
  hipStream_t st = nullptr;
  bool queued = false;  // work that uses the buffers may be on st: wait before the cache hands them on
  ~dc_scratch() {
    if (queued) (void)hipStreamSynchronize(st);
    if (d) stb_pool_free(d);
    if (h) stb_pool_free(h);
  }
};

static size_t dc_up(size_t x) { return (x + 255) & ~(size_t)255; }

int stb_dc_check(const uint32_t *d_cnt, uint64_t rows, unsigned cols, unsigned stride, unsigned flags, const double *d_w, double w0,
                 double s, double shape, double scale, const stb_dirconc_info_t *info, const char *who) {
  if (!d_cnt || !info) return stb_fail("%s: d_cnt and info are required", who);
  if (cols < 1 || cols > stride) return stb_fail("%s: cols=%u, stride=%u (1 <= cols <= stride)", who, cols, stride);
  if (flags != STB_DM_ROWS && flags != STB_DM_COLUMNS)
    return stb_fail("%s: flags=0x%x (exactly one of STB_DM_ROWS, STB_DM_COLUMNS)", who, flags);
  if (!d_w && (!(w0 > 0.0) || !std::isfinite(w0))) return stb_fail("%s: w0=%g (must be > 0 and finite)", who, w0);
  if (!(s > 0.0) || !std::isfinite(s)) return stb_fail("%s: s=%g (must be > 0 and finite)", who, s);
  if (!(shape > 0.0) || !std::isfinite(shape)) return stb_fail("%s: shape=%g (must be > 0 and finite)", who, shape);
  if (!(scale > 0.0) || !std::isfinite(scale)) return stb_fail("%s: scale=%g (must be > 0 and finite)", who, scale);
  if (rows < 1) return stb_fail("%s: rows=0 (a matrix without rows has no %s to draw from)", who,
                                flags == STB_DM_ROWS ? "multinomial" : "category");
  const uint64_t nm = flags == STB_DM_ROWS ? rows : (uint64_t)cols;
  if (nm > (uint64_t)INT_MAX) return stb_fail("%s: %llu multinomials (at most %d)", who, (unsigned long long)nm, INT_MAX);
  if ((rows + DC_CHUNK - 1) / DC_CHUNK > 0x7fffffffull) return stb_fail("%s: rows=%llu", who, (unsigned long long)rows);
  return 0;
}

int stb_dc_run(const uint32_t *d_cnt, uint64_t rows, unsigned cols, unsigned stride, unsigned flags, const double *d_w, double w0,
               double s, double shape, double scale, uint32_t *d_m, uint32_t *d_M, uint64_t seed, uint64_t sweep, hipStream_t st,
               stb_dirconc_info_t *info, const char *who) {
  if (stb_device_count() < 1) return stb_no_device(who);
  const bool by_rows = flags == STB_DM_ROWS;
  const size_t nm = by_rows ? (size_t)rows : (size_t)cols;
  const uint64_t ncat = by_rows ? (uint64_t)cols : rows;
  const unsigned nw = (unsigned)stb_env_waves("STB_DIRCONC_WAVES", 4);
  const char *form = getenv("STB_DIRCONC_FORM");
  const unsigned twave = form && !strcmp(form, "lane") ? 0xffffffffu : form && !strcmp(form, "wave") ? 0u : HG_TWAVE;
  // scratch.  Zeroed: ctl (256 bytes), n[nm], M[nm] unless the caller gave one.  Then N32[nm], B[nm], the range {0, nm},
  // hyperb's L[nm] and Y[nm]
  const size_t o_n = 256, o_M = o_n + dc_up(8 * nm), o_N = o_M + (d_M ? 0 : dc_up(4 * nm)), o_B = o_N + dc_up(4 * nm),
               o_go = o_B + dc_up(8 * nm), o_L = o_go + 256, o_Y = o_L + dc_up(8 * nm), bytes = o_Y + dc_up(4 * nm);
  dc_scratch sc;
  sc.st = st;
  if (stb_pool_malloc(&sc.d, bytes) != hipSuccess || stb_pool_malloc(&sc.h, 256, 1) != hipSuccess ||
      hipHostGetDevicePointer(&sc.h_dev, sc.h, 0) != hipSuccess)
    return stb_fail("%s: out of memory for %zu bytes of scratch", who, bytes);
  char *d = (char *)sc.d;
  unsigned *ctl = (unsigned *)d;
  unsigned long long *n = (unsigned long long *)(d + o_n);
  uint32_t *M = d_M ? d_M : (uint32_t *)(d + o_M), *N32 = (uint32_t *)(d + o_N), *Y = (uint32_t *)(d + o_Y);
  double *B = (double *)(d + o_B), *L = (double *)(d + o_L);
  uint64_t *goff1 = (uint64_t *)(d + o_go);
  volatile unsigned long long *h_out = (volatile unsigned long long *)sc.h;
  h_out[0] = 0xffffffffull;
  sc.queued = true;
  HIPCHK(hipMemsetAsync(d, 0, o_N, st));
  if (d_M) HIPCHK(hipMemsetAsync(d_M, 0, 4 * nm, st));
  if (d_m) HIPCHK(hipMemsetAsync(d_m, 0, 4 * (size_t)rows * stride, st));
  const uint64_t key = stb_mix64(seed + (sweep + 1) * STB_GAMMA);
  const unsigned cus = (unsigned)(stb_cu_count() > 0 ? stb_cu_count() : 1);
  const unsigned cb = (cols + 63) / 64;
  const uint64_t nchunks = (rows + DC_CHUNK - 1) / DC_CHUNK;
  // the jobs of a column block: chunks (columns) or rows.  Few jobs: each is cut into parts, so that the cells a wave
  // takes keep about 8 waves a compute unit busy
  const uint64_t jobs = by_rows ? rows : nchunks;
  const uint64_t cap_y = (uint64_t)8 * cus / cb + 1, fill = cap_y * nw;
  const uint64_t per = (fill + jobs - 1) / jobs;
  const unsigned parts = twave != 0xffffffffu && jobs < fill ? (unsigned)(per < DC_PARTS_MAX ? per : DC_PARTS_MAX) : 1u;
  const uint64_t want_aux = (jobs * parts + nw - 1) / nw, want_tot = (jobs + nw - 1) / nw;
  const uint64_t lim = cap_y < 65535 ? cap_y : 65535;
  const unsigned gy_aux = (unsigned)(want_aux < lim ? want_aux : lim), gy_tot = (unsigned)(want_tot < lim ? want_tot : lim);
  if (stb_dm_weights_queue(d_w, ncat, w0, ctl, st)) return 1;
  if (by_rows) {
    const uint64_t cap = (uint64_t)8 * cus;
    STB_LAUNCH(k_dc_totals_rows, dim3((unsigned)(want_tot < cap ? want_tot : cap)), dim3(64 * nw), st, d_cnt, rows, cols, stride, d_w,
               n, ctl);
  } else {
    STB_LAUNCH(k_dc_totals, dim3(cb, gy_tot), dim3(64 * nw), st, d_cnt, rows, cols, stride, d_w, (unsigned)nchunks, n, ctl);
  }
  STB_LAUNCH(k_dc_prep, dim3((unsigned)((nm + 255) / 256)), dim3(256), st, (uint64_t)nm, (const unsigned long long *)n, s, scale, N32, B,
             goff1, ctl);
  if (by_rows)
    STB_LAUNCH(k_dc_aux_rows, dim3(cb, gy_aux), dim3(64 * nw), st, d_cnt, rows, cols, stride, d_w, w0, s, key, twave, parts,
               (const unsigned *)ctl, d_m, M);
  else
    STB_LAUNCH(k_dc_aux_cols, dim3(cb, gy_aux), dim3(64 * nw), st, d_cnt, rows, cols, stride, d_w, w0, s, key, twave, parts,
               (unsigned)nchunks, (const unsigned *)ctl, d_m, M);
  if (stb_hb_bgroups_queue_dscale((const double *)ctl + DC_CTL_INV, shape, (int)nm, N32, M, 1, goff1, B, L, Y, seed ^ HG_SALT_A, sweep,
                                  st, who))
    return 1;
  STB_LAUNCH(k_dc_finish, dim3(1), dim3(256), st, (uint64_t)nm, (const unsigned long long *)n, (const uint32_t *)M, (const double *)B,
             (const unsigned *)ctl, (unsigned long long *)sc.h_dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  sc.queued = false;
  const unsigned err = (unsigned)h_out[0];
  const unsigned long long bits = h_out[1];
  memcpy(&info->s, &bits, sizeof(double));
  info->count = h_out[2];
  info->aux_tables = h_out[3];
  info->nonempty = h_out[4];
  info->zero_weight = h_out[5];
  info->error_word = err;
  info->reserved = 0;
  if (err) {
    info->s = NAN;
    return stb_fail("%s: failed, error word 0x%x (1: a weight is negative, NaN or infinite; 2: the sum of the weights is not "
                    "positive and finite; 4: a cell with weight 0 holds a count; 8: a multinomial has more than 2^32 - 1 counts) "
                    "(seed=%llu, sweep=%llu); no auxiliary table was drawn and the outputs are undefined",
                    who, err, (unsigned long long)seed, (unsigned long long)sweep);
  }
  stb_bgroups_info_t bi;
  if (stb_hb_bgroups_answer(1, &bi, who)) {
    info->s = NAN;
    return 1;
  }
  if (bi.kept_groups || !(info->s > 0.0) || !std::isfinite(info->s)) {
    info->s = NAN;
    return stb_fail("%s: the concentration's draw is not a positive finite double; the outputs are undefined", who);
  }
  return 0;
}

extern "C" int stb_sample_dirconc(const uint32_t *d_cnt, uint64_t rows, unsigned cols, unsigned stride, unsigned flags,
                                  const double *d_w, double w0, double s, double shape, double scale, uint32_t *d_m, uint32_t *d_M,
                                  uint64_t seed, uint64_t sweep, void *stream, stb_dirconc_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_sample_dirconc";
  if (stb_dc_check(d_cnt, rows, cols, stride, flags, d_w, w0, s, shape, scale, info, who)) return 1;
  return stb_dc_run(d_cnt, rows, cols, stride, flags, d_w, w0, s, shape, scale, d_m, d_M, seed, sweep, (hipStream_t)stream, info, who);
}
