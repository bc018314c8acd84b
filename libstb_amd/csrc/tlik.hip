// tlik.hip -- the uncollapsed steps that go with the dish sweep (tdish.hip), on the device: every dish's class
// distribution drawn from its Dirichlet posterior given the (class, dish) counts, the dishes' base weights h drawn from
// theirs given the table counts, and the data term log p(classes | dishes, likelihood) of the complete-data log joint
// (include/stb_hip.h, "the likelihood and the base weights").
//
//   k_tlik_draw    lg_wk = log Gamma(beta_w + cnt_wk) into the output matrix, and every column's maximum
//   k_tlik_exp     e_wk = exp(lg_wk - M_k) in place, a thread a cell
//   k_tlik_sum     the sums of chunks of 256 rows
//   k_tlik_z       Z_k = the chunk sums in chunk order
//   k_tlik_div     lik_wk = e_wk / Z_k
//   k_th_count     c_k = sum over restaurants of t_ik (integers: atomics)
//   k_th_draw      one workgroup: lg_k = log Gamma(gamma_k + c_k), their maximum, e_k, Z, h_k
//   k_th_scatter   h_k to every pair (i, k)
//   k_tlik_llchunk / k_tlik_llfinal   cnt log(lik) summed by chunk, then by column, then over the columns
//
// Uniforms (counter-based, the convention of hyperq.hip): key = mix(seed + (sweep+1) gamma); cell e owns the substream
// key_e = mix(key + (e+1) gamma) and takes its elements 1, 2, ... (gamma_dev.h's hq_unit) in the order of gamma_dev.h's
// recipe.  e = w stride + k for the likelihood (the matrix's own flat index), e = k for the base weights: the draws depend
// on (seed, sweep, e) alone.  The two steps share a stream for equal seeds; a caller gives them different seeds.
//
// Associations (FP64, no contraction; the header fixes them).  A column's M_k is a maximum: exact in any order, so it is
// gathered with an integer atomic on an order-preserving image of the double.  Rows are cut into chunks of 256 (chunk j =
// rows 256 j .. 256 j + 255); one thread owns a (chunk, column) and adds its e_wk in row order starting from the chunk's
// first; Z_k adds the chunk sums in chunk order; then one division a cell.  Lanes run along k, so matrix and counts are
// read and written in rows of 64 consecutive doubles.  Nothing depends on the launch geometry: STB_TLIK_WAVES = 1, 2, 4
// or 8 waves a workgroup (default 4) gives the same bits.  No kernel waits for another workgroup; the passes are ordered
// by the stream.
//
// What should set the pace, from the instruction counts alone (MEASUREMENTS section T5 has what was measured): the
// draw.  A variate costs about seven FP64 transcendentals (log u1, cos, sqrt, log v, log u, log d, and log u' under the
// boost) of 40 to 100 instructions each, against 4 bytes read and 8 written; a wave repeats the attempt while any lane
// rejects.  The exponentials run a thread a cell; only the additions of k_tlik_sum are sequential, 256 to a thread, which
// leaves that pass rows / 256 x stride threads.

#include "stb_common.h"
#include "gamma_dev.h"
#include "tlik.h"

#pragma clang fp contract(off)

#define TL_CHUNK 256       // rows of a chunk of the sums (part of the contract)
#define TL_RPT 16          // rows a thread draws per step of k_tlik_draw
#define TL_MAXTHREADS 512

// an image of a double that unsigned comparison orders as the doubles are ordered (0: nothing seen, decodes to a NaN)
__device__ __forceinline__ unsigned long long tl_key(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double tl_unkey(unsigned long long q) {
  return __longlong_as_double((long long)((q >> 63) ? (q & 0x7fffffffffffffffull) : ~q));
}

// ctl[1]: error word -- bit 0 a Gamma draw ran out of attempts, bit 1 a normaliser is not positive and finite
__global__ __launch_bounds__(TL_MAXTHREADS) void k_tlik_draw(const uint32_t *cnt, unsigned rows, unsigned stride,
                                                             const double *beta, double beta0, double *lik, uint64_t key,
                                                             unsigned long long *colmax, unsigned *ctl) {
  const unsigned nw = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned k = blockIdx.x * 64 + lane;
  if (k >= stride) return;
  const unsigned span = nw * TL_RPT;  // rows a workgroup draws per step: wave v the rows v, v + nw, ...
  const unsigned nsteps = (rows + span - 1) / span;
  bool bad = false;
  double mx = -INFINITY;
  for (unsigned s = blockIdx.y; s < nsteps; s += gridDim.y) {
    for (unsigned r = 0; r < TL_RPT; r++) {
      const uint64_t w = (uint64_t)s * span + wave + (uint64_t)r * nw;
      if (w >= rows) break;
      const uint64_t e = w * stride + k;
      const double alpha = (beta ? beta[w] : beta0) + (double)cnt[e];
      const uint64_t ke = stb_mix64(key + (e + 1) * STB_GAMMA);
      uint64_t j = 0;
      const double lg = hq_log_gamma(alpha, ke, j, bad);
      lik[e] = lg;
      if (lg > mx) mx = lg;  // (a NaN is never greater)
    }
  }
  if (mx > -INFINITY) atomicMax(&colmax[k], tl_key(mx));
  if (bad) __hip_atomic_fetch_or(&ctl[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_tlik_exp(uint64_t cells, unsigned stride, double *lik, const unsigned long long *colmax) {
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * 256)
    lik[e] = exp(lik[e] - tl_unkey(colmax[e % stride]));
}

// one thread a (chunk, column): wave v of workgroup (x, y) the chunks y nw + v, then + gridDim.y nw, ...
__global__ __launch_bounds__(TL_MAXTHREADS) void k_tlik_sum(unsigned rows, unsigned stride, const double *lik,
                                                            double *csum, unsigned nchunks) {
  const unsigned nw = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned k = blockIdx.x * 64 + lane;
  if (k >= stride) return;
  for (unsigned c = blockIdx.y * nw + wave; c < nchunks; c += gridDim.y * nw) {
    const uint64_t w0 = (uint64_t)c * TL_CHUNK, w1 = w0 + TL_CHUNK < rows ? w0 + TL_CHUNK : rows;
    const double *p = lik + w0 * stride + k;
    double s = *p;
    p += stride;
#pragma unroll 8
    for (uint64_t w = w0 + 1; w < w1; w++, p += stride) s = s + *p;
    csum[(uint64_t)c * stride + k] = s;
  }
}

__global__ __launch_bounds__(64) void k_tlik_z(unsigned stride, const double *csum, unsigned nchunks, double *Z, unsigned *ctl) {
  const unsigned k = blockIdx.x * 64 + threadIdx.x;
  if (k >= stride) return;
  double z = csum[k];
  for (unsigned c = 1; c < nchunks; c++) z = z + csum[(uint64_t)c * stride + k];
  Z[k] = z;
  if (!(z > 0.0 && isfinite(z))) __hip_atomic_fetch_or(&ctl[1], 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_tlik_div(uint64_t cells, unsigned stride, double *lik, const double *Z) {
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * 256)
    lik[e] = lik[e] / Z[e % stride];
}

// ---- the base weights ---------------------------------------------------------------------------------------------

// a wave a restaurant, lanes over its dishes
__global__ __launch_bounds__(256) void k_th_count(int I, const uint64_t *koff, const uint16_t *tv, unsigned Kmax,
                                                  unsigned long long *c) {
  const unsigned lane = threadIdx.x & 63;
  const uint64_t nwaves = (uint64_t)gridDim.x * 4;
  for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < (uint64_t)I; i += nwaves) {
    const uint64_t g0 = koff[i], K = koff[i + 1] - g0;
    for (uint64_t k = lane; k < K && k < Kmax; k += 64) {
      const unsigned t = tv[g0 + k];
      if (t) atomicAdd(&c[k], (unsigned long long)t);
    }
  }
}

__global__ __launch_bounds__(TL_MAXTHREADS) void k_th_draw(const unsigned long long *c, unsigned Kmax, const double *gam,
                                                           double gamma0, uint64_t key, double *hk, unsigned *ctl) {
  __shared__ double sv[STB_TD_MAXK];
  __shared__ double sred[TL_MAXTHREADS];
  __shared__ double s_M, s_Z;
  const unsigned nthr = blockDim.x, tid = threadIdx.x;
  bool bad = false;
  double mx = -INFINITY;
  for (unsigned k = tid; k < Kmax; k += nthr) {
    const double alpha = (gam ? gam[k] : gamma0) + (double)c[k];
    const uint64_t ke = stb_mix64(key + ((uint64_t)k + 1) * STB_GAMMA);
    uint64_t j = 0;
    const double lg = hq_log_gamma(alpha, ke, j, bad);
    sv[k] = lg;
    if (lg > mx) mx = lg;
  }
  sred[tid] = mx;
  __syncthreads();
  if (tid == 0) {
    double M = sred[0];
    for (unsigned q = 1; q < nthr; q++) M = sred[q] > M ? sred[q] : M;
    s_M = M;
  }
  __syncthreads();
  const double M = s_M;
  for (unsigned k = tid; k < Kmax; k += nthr) sv[k] = exp(sv[k] - M);
  __syncthreads();
  if (tid == 0) {
    double z = sv[0];
    for (unsigned k = 1; k < Kmax; k++) z = z + sv[k];
    s_Z = z;
    if (!(z > 0.0 && isfinite(z))) __hip_atomic_fetch_or(&ctl[1], 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const double Z = s_Z;
  for (unsigned k = tid; k < Kmax; k += nthr) hk[k] = sv[k] / Z;
  if (bad) __hip_atomic_fetch_or(&ctl[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_th_scatter(int I, const uint64_t *koff, unsigned Kmax, const double *hk, double *h) {
  const unsigned lane = threadIdx.x & 63;
  const uint64_t nwaves = (uint64_t)gridDim.x * 4;
  for (uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < (uint64_t)I; i += nwaves) {
    const uint64_t g0 = koff[i], K = koff[i + 1] - g0;
    for (uint64_t k = lane; k < K && k < Kmax; k += 64) h[g0 + k] = hk[k];
  }
}

// ---- the data term ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(TL_MAXTHREADS) void k_tlik_llchunk(const uint32_t *cnt, const double *lik, unsigned rows,
                                                                unsigned stride, double *csum, unsigned nchunks,
                                                                unsigned long long *imp) {
  const unsigned nw = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned k = blockIdx.x * 64 + lane;
  if (k >= stride) return;
  unsigned long long nimp = 0;
  for (unsigned c = blockIdx.y * nw + wave; c < nchunks; c += gridDim.y * nw) {
    const uint64_t w0 = (uint64_t)c * TL_CHUNK, w1 = w0 + TL_CHUNK < rows ? w0 + TL_CHUNK : rows;
    double s = 0.0;
#pragma unroll 4
    for (uint64_t w = w0; w < w1; w++) {
      const uint64_t e = w * stride + k;
      const unsigned n = cnt[e];
      double x = 0.0;
      if (n) {
        const double l = lik[e];
        x = (double)n * log(l);
        nimp += l == 0.0;
      }
      s = w == w0 ? x : s + x;
    }
    csum[(uint64_t)c * stride + k] = s;
  }
  if (nimp) atomicAdd(imp, nimp);
}

// one workgroup: the chunk sums of a column in chunk order, then the columns in k order; the answer to pinned memory
__global__ __launch_bounds__(256) void k_tlik_llfinal(unsigned stride, const double *csum, unsigned nchunks, double *col,
                                                      const unsigned long long *imp, double *host_out) {
  for (unsigned k = threadIdx.x; k < stride; k += 256) {
    double z = csum[k];
    for (unsigned c = 1; c < nchunks; c++) z = z + csum[(uint64_t)c * stride + k];
    col[k] = z;
  }
  __syncthreads();  // (col is this workgroup's own: its stores are visible to it behind the barrier)
  if (threadIdx.x == 0) {
    double t = col[0];
    for (unsigned k = 1; k < stride; k++) t = t + col[k];
    host_out[0] = t;
    ((unsigned long long *)host_out)[1] = *imp;
  }
}

// ------------------------------------------------------------------------------------------------
// host side.  Every call takes its scratch from the buffer cache and gives it back behind its one wait.

static unsigned tl_waves() {
  return (unsigned)stb_env_waves("STB_TLIK_WAVES", 4);
}

static unsigned tl_cap_y(uint64_t want) { return want < 1 ? 1u : (want > 65535u ? 65535u : (unsigned)want); }

struct tl_scratch {
  void *d = nullptr;   // device
  void *h = nullptr;   // pinned: 256 bytes of result words
  void *h_dev = nullptr;
  void *stage = nullptr;  // pinned: the caller's beta / gamma vector on its way to the device
  hipStream_t st = nullptr;
  bool queued = false;    // work that uses the buffers may be on st: wait before the cache hands them on
  ~tl_scratch() {
    if (queued) (void)hipStreamSynchronize(st);
    if (d) stb_pool_free(d);
    if (h) stb_pool_free(h);
    if (stage) stb_pool_free(stage);
  }
};

static int tl_take(tl_scratch &sc, size_t dev_bytes, size_t stage_bytes, hipStream_t st, const char *who) {
  sc.st = st;
  if (stb_pool_malloc(&sc.d, dev_bytes) != hipSuccess || stb_pool_malloc(&sc.h, 256, 1) != hipSuccess ||
      hipHostGetDevicePointer(&sc.h_dev, sc.h, 0) != hipSuccess ||
      (stage_bytes && stb_pool_malloc(&sc.stage, stage_bytes, 1) != hipSuccess))
    return stb_fail("%s: out of memory for %zu bytes of scratch", who, dev_bytes);
  return 0;
}

int stb_tl_check_prior(const double *v, uint64_t len, double v0, const char *name, const char *who) {
  if (!v) {
    if (!(v0 > 0.0) || !std::isfinite(v0)) return stb_fail("%s: %s0=%g (must be > 0 and finite)", who, name, v0);
    return 0;
  }
  for (uint64_t j = 0; j < len; j++)
    if (!(v[j] > 0.0) || !std::isfinite(v[j]))
      return stb_fail("%s: %s[%llu]=%g (must be > 0 and finite)", who, name, (unsigned long long)j, v[j]);
  return 0;
}

int stb_tl_sample_lik(const uint32_t *d_cnt, unsigned rows, unsigned stride, const double *beta_host, double beta0,
                      double *d_lik, uint64_t seed, uint64_t sweep, hipStream_t st, const char *who, bool *touched) {
  const unsigned nw = tl_waves(), nchunks = (rows + TL_CHUNK - 1) / TL_CHUNK, cb = (stride + 63) / 64;
  const uint64_t cells = (uint64_t)rows * stride;
  // scratch: ctl (256 bytes), colmax[stride], Z[stride], csum[nchunks x stride], beta[rows]
  const size_t o_max = 256, o_Z = o_max + 8 * (size_t)stride, o_cs = o_Z + 8 * (size_t)stride,
               o_beta = o_cs + 8 * (size_t)nchunks * stride, bytes = o_beta + (beta_host ? 8 * (size_t)rows : 0);
  tl_scratch sc;
  if (tl_take(sc, bytes, beta_host ? 8 * (size_t)rows : 0, st, who)) return 1;
  char *d = (char *)sc.d;
  unsigned *ctl = (unsigned *)d;
  unsigned long long *colmax = (unsigned long long *)(d + o_max);
  double *Z = (double *)(d + o_Z), *csum = (double *)(d + o_cs), *d_beta = beta_host ? (double *)(d + o_beta) : nullptr;
  volatile unsigned *h_err = (volatile unsigned *)sc.h;
  *h_err = 0xffffffffu;
  sc.queued = true;
  HIPCHK(hipMemsetAsync(d, 0, o_Z, st));  // ctl and the maxima's images
  if (beta_host) {
    memcpy(sc.stage, beta_host, 8 * (size_t)rows);
    HIPCHK(hipMemcpyAsync(d_beta, sc.stage, 8 * (size_t)rows, hipMemcpyHostToDevice, st));
  }
  const uint64_t key = stb_mix64(seed + (sweep + 1) * STB_GAMMA);
  const unsigned span = nw * TL_RPT;
  const uint64_t want = (cells + 255) / 256, cap = 64ull * (uint64_t)(stb_cu_count() > 0 ? stb_cu_count() : 1);
  const unsigned flat = (unsigned)(want < cap ? want : cap);
  if (touched) *touched = true;  // from here on d_lik is scratch until the last pass is through
  STB_LAUNCH(k_tlik_draw, dim3(cb, tl_cap_y((rows + span - 1) / span)), dim3(64 * nw), st, d_cnt, rows, stride, d_beta, beta0,
             d_lik, key, colmax, ctl);
  STB_LAUNCH(k_tlik_exp, dim3(flat), dim3(256), st, cells, stride, d_lik, colmax);
  STB_LAUNCH(k_tlik_sum, dim3(cb, tl_cap_y((nchunks + nw - 1) / nw)), dim3(64 * nw), st, rows, stride, d_lik, csum, nchunks);
  STB_LAUNCH(k_tlik_z, dim3(cb), dim3(64), st, stride, csum, nchunks, Z, ctl);
  STB_LAUNCH(k_tlik_div, dim3(flat), dim3(256), st, cells, stride, d_lik, Z);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(sc.h, ctl + 1, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  sc.queued = false;
  const unsigned err = *h_err;
  if (err & 1u)
    return stb_fail("%s: a Gamma draw was not accepted within %d attempts (seed=%llu, sweep=%llu); the matrix is undefined", who,
                    HQ_CAP, (unsigned long long)seed, (unsigned long long)sweep);
  if (err) return stb_fail("%s: a column's normaliser is not positive and finite; the matrix is undefined", who);
  return 0;
}

int stb_tl_sample_h(int I, const uint64_t *d_koff, const uint16_t *d_t, unsigned Kmax, const double *gamma_host, double gamma0,
                    double *d_h, uint64_t seed, uint64_t sweep, hipStream_t st, const char *who, bool *touched) {
  const unsigned nw = tl_waves();
  // scratch: ctl (256 bytes), c[Kmax] (uint64), hk[Kmax], gamma[Kmax]
  const size_t o_c = 256, o_hk = o_c + 8 * (size_t)Kmax, o_g = o_hk + 8 * (size_t)Kmax,
               bytes = o_g + (gamma_host ? 8 * (size_t)Kmax : 0);
  tl_scratch sc;
  if (tl_take(sc, bytes, gamma_host ? 8 * (size_t)Kmax : 0, st, who)) return 1;
  char *d = (char *)sc.d;
  unsigned *ctl = (unsigned *)d;
  unsigned long long *c = (unsigned long long *)(d + o_c);
  double *hk = (double *)(d + o_hk), *d_g = gamma_host ? (double *)(d + o_g) : nullptr;
  volatile unsigned *h_err = (volatile unsigned *)sc.h;
  *h_err = 0xffffffffu;
  sc.queued = true;
  HIPCHK(hipMemsetAsync(d, 0, o_hk, st));
  if (gamma_host) {
    memcpy(sc.stage, gamma_host, 8 * (size_t)Kmax);
    HIPCHK(hipMemcpyAsync(d_g, sc.stage, 8 * (size_t)Kmax, hipMemcpyHostToDevice, st));
  }
  const uint64_t key = stb_mix64(seed + (sweep + 1) * STB_GAMMA);
  const unsigned cap = 16u * (unsigned)(stb_cu_count() > 0 ? stb_cu_count() : 1), want = (unsigned)(((uint64_t)I + 3) / 4);
  const unsigned gx = want < cap ? want : cap;
  if (touched) *touched = true;
  STB_LAUNCH(k_th_count, dim3(gx), dim3(256), st, I, d_koff, d_t, Kmax, c);
  STB_LAUNCH(k_th_draw, dim3(1), dim3(64 * nw), st, c, Kmax, d_g, gamma0, key, hk, ctl);
  STB_LAUNCH(k_th_scatter, dim3(gx), dim3(256), st, I, d_koff, Kmax, hk, d_h);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(sc.h, ctl + 1, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  sc.queued = false;
  const unsigned err = *h_err;
  if (err & 1u)
    return stb_fail("%s: a Gamma draw was not accepted within %d attempts (seed=%llu, sweep=%llu); h is undefined", who, HQ_CAP,
                    (unsigned long long)seed, (unsigned long long)sweep);
  if (err) return stb_fail("%s: the normaliser is not positive and finite; h is undefined", who);
  return 0;
}

int stb_tl_loglik(const uint32_t *d_cnt, const double *d_lik, unsigned rows, unsigned stride, double *total_host,
                  uint64_t *impossible_host, hipStream_t st, const char *who) {
  const unsigned nw = tl_waves(), nchunks = (rows + TL_CHUNK - 1) / TL_CHUNK, cb = (stride + 63) / 64;
  // scratch: the impossible count (256 bytes), col[stride], csum[nchunks x stride]
  const size_t o_col = 256, o_cs = o_col + 8 * (size_t)stride, bytes = o_cs + 8 * (size_t)nchunks * stride;
  tl_scratch sc;
  if (tl_take(sc, bytes, 0, st, who)) return 1;
  char *d = (char *)sc.d;
  unsigned long long *imp = (unsigned long long *)d;
  double *col = (double *)(d + o_col), *csum = (double *)(d + o_cs);
  sc.queued = true;
  HIPCHK(hipMemsetAsync(d, 0, 256, st));
  STB_LAUNCH(k_tlik_llchunk, dim3(cb, tl_cap_y((nchunks + nw - 1) / nw)), dim3(64 * nw), st, d_cnt, d_lik, rows, stride, csum,
             nchunks, imp);
  STB_LAUNCH(k_tlik_llfinal, dim3(1), dim3(256), st, stride, csum, nchunks, col, imp, (double *)sc.h_dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  sc.queued = false;
  *total_host = ((volatile double *)sc.h)[0];
  if (impossible_host) *impossible_host = ((volatile unsigned long long *)sc.h)[1];
  return 0;
}

// ---- the raw layer ------------------------------------------------------------------------------------------------

extern "C" int stb_sample_lik(const uint32_t *d_cnt, unsigned rows, unsigned stride, const double *beta_host, double beta0,
                              double *d_lik, uint64_t seed, uint64_t sweep, void *stream) {
  STB_ENTRY;
  const char *who = "stb_sample_lik";
  if (!d_cnt || !d_lik) return stb_fail("%s: d_cnt and d_lik are required", who);
  if (rows < 1 || stride < 1) return stb_fail("%s: rows=%u stride=%u (both must be >= 1)", who, rows, stride);
  if (stb_tl_check_prior(beta_host, rows, beta0, "beta", who)) return 1;
  if (stb_device_count() < 1) return stb_no_device(who);
  return stb_tl_sample_lik(d_cnt, rows, stride, beta_host, beta0, d_lik, seed, sweep, (hipStream_t)stream, who, nullptr);
}

extern "C" int stb_lik_loglik(const uint32_t *d_cnt, const double *d_lik, unsigned rows, unsigned stride, double *total_host,
                              uint64_t *impossible_host, void *stream) {
  STB_ENTRY;
  const char *who = "stb_lik_loglik";
  if (!d_cnt || !d_lik || !total_host) return stb_fail("%s: d_cnt, d_lik and total_host are required", who);
  if (rows < 1 || stride < 1) return stb_fail("%s: rows=%u stride=%u (both must be >= 1)", who, rows, stride);
  if (stb_device_count() < 1) return stb_no_device(who);
  return stb_tl_loglik(d_cnt, d_lik, rows, stride, total_host, impossible_host, (hipStream_t)stream, who);
}
