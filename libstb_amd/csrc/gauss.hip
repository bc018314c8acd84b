// gauss.hip -- Gaussian observations for the dish sweep (tdish.hip), on the device: the dishes' sufficient statistics,
// every dish's mean and diagonal precision drawn from the Normal-Gamma posterior, the C x K matrix of Gaussian densities
// that k_tdish reads as its likelihood (one row per customer), the data term and the collapsed evidence
// (include/stb_hip.h, "Gaussian observations").
//
//   k_gs_sum_a / k_gs_sum_b   a thread a (chunk of 256 customers, dish): the chunk's members added in customer order, x in
//                             pass A, (x - mean)(x - mean) in pass B; 16 dimensions a launch row (blockIdx.z)
//   k_gs_fin_a / k_gs_fin_b   a thread a (dish, dimension): the chunk partials in chunk order in double-double; n and the
//                             mean, or Q
//   k_gs_draw                 a thread a cell e = k D + d: tau, then mu
//   k_gs_prep                 H_k, and mu, tau transposed so that lanes along k read them in whole rows
//   k_gs_lik                  a wave a customer row, lanes along k: l_ck, the row's maximum, exp
//   k_gs_loglik / k_gs_logml  blocks of 256 terms by k_logjoint's tree; the last workgroup (ticket.h) adds the block sums
//
// Associations (FP64, no contraction; the header fixes them).  No floating-point atomics and no sort: the members of a
// dish are found by comparing every customer's dish with the lane's own, so cust[c] and x_c[d] are wave-uniform and a
// customer costs the vector unit one compare and D masked adds.  The counts are integers: a chunk's are counted by the
// thread that sums it and added by k_gs_fin_a in u64.  Nothing depends on the launch geometry: STB_GAUSS_WAVES = 1, 2, 4
// or 8 waves a workgroup (default 4) gives the same bits.  No kernel waits for another workgroup; the passes are ordered
// by the stream.
//
// What sets the pace (MEASUREMENTS section GS1, K = 64, D = 16): the statistics, three times the matrix at 2 10^7 customers.
// The matrix reads 8 D bytes and writes 8 K bytes a customer, 4 D FP64 operations and one exp a cell, and runs at the
// store rate (1.2 TB/s).  The statistics read x twice, but every wave walks its 256 customers one after another, once per
// block of 64 dishes and 16 dimensions; the chunk partials are 8 D K bytes per 256 customers.

#include "stb_common.h"
#include "gamma_dev.h"
#include "ticket.h"
#include "gauss.h"

#pragma clang fp contract(off)

#define GS_DT 16            // dimensions a thread of the sums keeps in registers
#define GS_MAXTHREADS 512
#define GS_CAP 1024u        // workgroups along the strided axis of a grid at most
#define GS_STAGE 1024       // block sums the last workgroup stages in LDS at a time
#define GS_FIN_BATCH 16     // chunk partials k_gs_fin_* loads ahead of its ordered additions
#define GS_REG_D 16       // k_gs_lik keeps a block's mu and tau in registers up to this D (and K <= 64)

// ctl, u64 words zeroed on the stream ahead of a call: [0] the ticket (its low u32), [1] the error word -- bit 0 a Gamma
// draw ran out of attempts, bit 1 a tau is not positive and finite -- [2] skipped, [3] dead
#define GS_ERR 1
#define GS_SKIPPED 2
#define GS_DEAD 3

// ---- statistics ---------------------------------------------------------------------------------------------------

// wave v of workgroup (x, y, z): dishes 64 x .. 64 x + 63, dimensions 16 z .. 16 z + 15, chunks y nw + v, + gridDim.y nw, ...
template <bool CENTRED>
__device__ __forceinline__ void gs_sum(const double *__restrict__ x, unsigned D, const uint32_t *__restrict__ cust, uint64_t C,
                                       unsigned K, const double *__restrict__ mean, double *__restrict__ csum,
                                       uint32_t *__restrict__ ccnt, unsigned nchunks, unsigned long long *ctl) {
  const unsigned nw = blockDim.x >> 6, wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)),
                 lane = threadIdx.x & 63;
  const unsigned k = blockIdx.x * 64 + lane;
  const unsigned d0 = blockIdx.z * GS_DT, dn = D - d0 < GS_DT ? D - d0 : GS_DT;
  const bool count_skips = !CENTRED && blockIdx.x == 0 && blockIdx.z == 0;
  double mk[GS_DT];
#pragma unroll
  for (unsigned j = 0; j < GS_DT; j++) mk[j] = (CENTRED && j < dn && k < K) ? mean[(uint64_t)k * D + d0 + j] : 0.0;
  unsigned long long nskip = 0;
  for (unsigned ch = blockIdx.y * nw + wave; ch < nchunks; ch += gridDim.y * nw) {
    const uint64_t c0 = (uint64_t)ch * GS_CHUNK, c1 = c0 + GS_CHUNK < C ? c0 + GS_CHUNK : C;
    double acc[GS_DT];
#pragma unroll
    for (unsigned j = 0; j < GS_DT; j++) acc[j] = 0.0;
    unsigned m = 0;
    for (uint64_t c = c0; c < c1; c++) {
      if (cust[c] != k) continue;
      const double *xc = x + c * D + d0;
#pragma unroll
      for (unsigned j = 0; j < GS_DT; j++) {
        if (j < dn) {
          double v = xc[j];
          if (CENTRED) {
            const double t = v - mk[j];
            v = t * t;
          }
          acc[j] = m ? acc[j] + v : v;
        }
      }
      m++;
    }
    if (k < K) {
      if (!CENTRED && blockIdx.z == 0) ccnt[(uint64_t)ch * K + k] = m;
      if (m) {
#pragma unroll
        for (unsigned j = 0; j < GS_DT; j++)
          if (j < dn) csum[((uint64_t)ch * D + d0 + j) * K + k] = acc[j];
      }
    }
    if (count_skips)
      for (uint64_t c = c0 + lane; c < c1; c += 64) nskip += cust[c] >= K;
  }
  if (count_skips) {
    nskip = stb_wave_sum(nskip);
    if (lane == 0 && nskip) __hip_atomic_fetch_add(&ctl[GS_SKIPPED], nskip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(GS_MAXTHREADS) void k_gs_sum_a(const double *x, unsigned D, const uint32_t *cust, uint64_t C,
                                                            unsigned K, double *csum, uint32_t *ccnt, unsigned nchunks,
                                                            unsigned long long *ctl) {
  gs_sum<false>(x, D, cust, C, K, nullptr, csum, ccnt, nchunks, ctl);
}

__global__ __launch_bounds__(GS_MAXTHREADS) void k_gs_sum_b(const double *x, unsigned D, const uint32_t *cust, uint64_t C,
                                                            unsigned K, const double *mean, double *csum, uint32_t *ccnt,
                                                            unsigned nchunks) {
  gs_sum<true>(x, D, cust, C, K, mean, csum, ccnt, nchunks, nullptr);
}

// thread t = d K + k (lanes along k: the partials are read in rows)
template <bool CENTRED>
__device__ __forceinline__ void gs_fin(const double *__restrict__ csum, const uint32_t *__restrict__ ccnt, unsigned nchunks,
                                       unsigned K, unsigned D, uint32_t *nout, double *mean, double *Q) {
  const unsigned t = blockIdx.x * 256 + threadIdx.x;
  if (t >= K * D) return;
  const unsigned k = t % K, d = t / K;
  dd_t acc{0.0, 0.0};
  unsigned long long n = 0;
  // GS_FIN_BATCH chunks' counts and partials are loaded side by side (a skipped chunk's partial is scratch nobody wrote:
  // loaded, never used), then added in chunk order: the additions are a chain, the loads need not be
  for (unsigned c0 = 0; c0 < nchunks; c0 += GS_FIN_BATCH) {
    unsigned m[GS_FIN_BATCH];
    double v[GS_FIN_BATCH];
#pragma unroll
    for (unsigned j = 0; j < GS_FIN_BATCH; j++) {
      const unsigned ch = c0 + j < nchunks ? c0 + j : nchunks - 1;
      m[j] = c0 + j < nchunks ? ccnt[(uint64_t)ch * K + k] : 0u;
      v[j] = csum[((uint64_t)ch * D + d) * K + k];
    }
#pragma unroll
    for (unsigned j = 0; j < GS_FIN_BATCH; j++) {
      if (m[j]) {
        n += m[j];
        dd_add(acc, v[j]);
      }
    }
  }
  const uint64_t e = (uint64_t)k * D + d;
  if (!CENTRED) {
    if (d == 0) nout[k] = (uint32_t)n;
    mean[e] = n ? (acc.hi + acc.lo) / (double)(uint32_t)n : 0.0;
  } else {
    Q[e] = n ? acc.hi + acc.lo : 0.0;
  }
}

__global__ __launch_bounds__(256) void k_gs_fin_a(const double *csum, const uint32_t *ccnt, unsigned nchunks, unsigned K,
                                                  unsigned D, uint32_t *nout, double *mean) {
  gs_fin<false>(csum, ccnt, nchunks, K, D, nout, mean, nullptr);
}

__global__ __launch_bounds__(256) void k_gs_fin_b(const double *csum, const uint32_t *ccnt, unsigned nchunks, unsigned K,
                                                  unsigned D, double *Q) {
  gs_fin<true>(csum, ccnt, nchunks, K, D, nullptr, nullptr, Q);
}

// ---- the draw -----------------------------------------------------------------------------------------------------

struct gs_prior_dev {
  double kappa0, alpha0, beta00;
  const double *m0, *beta0;  // device, D each, or null
};

// what a cell's posterior is: the prior's values, nothing evaluated, for a dish without customers
__device__ __forceinline__ void gs_posterior(const gs_prior_dev &p, unsigned d, unsigned nk, double mean, double Q, double &kn,
                                             double &mn, double &an, double &bn) {
  const double m0 = p.m0 ? p.m0[d] : 0.0, b0 = p.beta0 ? p.beta0[d] : p.beta00;
  kn = p.kappa0;
  mn = m0;
  an = p.alpha0;
  bn = b0;
  if (nk) {
    const double n = (double)nk, dm = mean - m0;
    kn = p.kappa0 + n;
    mn = (p.kappa0 * m0 + n * mean) / kn;
    an = p.alpha0 + 0.5 * n;
    bn = (b0 + 0.5 * Q) + 0.5 * (((p.kappa0 * n) / kn) * (dm * dm));
  }
}

__global__ __launch_bounds__(GS_MAXTHREADS) void k_gs_draw(const uint32_t *n, const double *mean, const double *Q, unsigned K,
                                                           unsigned D, gs_prior_dev p, uint64_t key, double *mu, double *tau,
                                                           unsigned long long *ctl) {
  const unsigned e = blockIdx.x * blockDim.x + threadIdx.x;  // (K D <= 65536 cells: a thread a cell, no stride)
  if (e >= K * D) return;
  const unsigned k = e / D, d = e % D;
  double kn, mn, an, bn;
  gs_posterior(p, d, n[k], mean[e], Q[e], kn, mn, an, bn);
  const uint64_t ke = stb_mix64(key + ((uint64_t)e + 1) * STB_GAMMA);
  uint64_t j = 0;
  bool bad = false;
  const double lg = hq_log_gamma(an, ke, j, bad);
  const double lt = lg - log(bn);
  const double t = exp(lt);
  const double u1 = hq_unit(ke, ++j);
  const double u2 = hq_unit(ke, ++j);
  const double z = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
  tau[e] = t;
  mu[e] = mn + z / sqrt(kn * t);
  const unsigned err = (bad ? 1u : 0u) | (t > 0.0 && isfinite(t) ? 0u : 2u);
  if (err) __hip_atomic_fetch_or(&ctl[GS_ERR], (unsigned long long)err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the matrix ---------------------------------------------------------------------------------------------------

// a thread a dish: H_k = sum_d 0.5 log(tau_kd) from d = 0, and the transposed copies muT[d K + k], tauT[d K + k]
__global__ __launch_bounds__(256) void k_gs_prep(const double *mu, const double *tau, unsigned K, unsigned D, double *muT,
                                                 double *tauT, double *H) {
  const unsigned k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  double h = 0.0;
  for (unsigned d = 0; d < D; d++) {
    const double t = tau[(uint64_t)k * D + d], hl = 0.5 * log(t);
    h = d ? h + hl : hl;
    muT[(uint64_t)d * K + k] = mu[(uint64_t)k * D + d];
    tauT[(uint64_t)d * K + k] = t;
  }
  H[k] = h;
}

// wave v of workgroup g: rows g nw + v, + gridDim.x nw, ...  REG: K <= 64 and D <= GS_REG_D, the one block's mu and tau
// in registers; else they are read from the transposed copies (L1 / L2) and a row of more than one block keeps its l in
// the row itself until the maximum over all blocks is known (every lane reads back what it wrote)
template <bool REG>
__device__ __forceinline__ void gs_lik(const double *__restrict__ x, unsigned D, uint64_t C, const double *__restrict__ muT,
                                       const double *__restrict__ tauT, const double *__restrict__ H, unsigned K,
                                       double *__restrict__ lik, unsigned stride, unsigned long long *ctl) {
  const unsigned nw = blockDim.x >> 6, wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)),
                 lane = threadIdx.x & 63;
  const unsigned nb = (stride + 63) / 64;
  double mr[GS_REG_D], tr[GS_REG_D], hr = 0.0;
  if (REG) {
#pragma unroll
    for (unsigned d = 0; d < GS_REG_D; d++) {
      const bool in = d < D && lane < K;
      mr[d] = in ? muT[(uint64_t)d * K + lane] : 0.0;
      tr[d] = in ? tauT[(uint64_t)d * K + lane] : 0.0;
    }
    if (lane < K) hr = H[lane];
  }
  unsigned long long ndead = 0;
  for (uint64_t c = (uint64_t)blockIdx.x * nw + wave; c < C; c += (uint64_t)gridDim.x * nw) {
    const double *xc = x + c * D;
    double *row = lik + c * stride;
    double mx = -INFINITY, l0 = -INFINITY;
    for (unsigned b = 0; b < nb; b++) {
      const unsigned k = b * 64 + lane;
      double l = -INFINITY;
      if (k < K) {
        double q = 0.0;
        if (REG) {
#pragma unroll
          for (unsigned d = 0; d < GS_REG_D; d++) {
            if (d < D) {
              const double t = xc[d] - mr[d], s = (t * t) * tr[d];
              q = d ? q + s : s;
            }
          }
          l = hr - 0.5 * q;
        } else {
          for (unsigned d = 0; d < D; d++) {
            const double t = xc[d] - muT[(uint64_t)d * K + k], s = (t * t) * tauT[(uint64_t)d * K + k];
            q = d ? q + s : s;
          }
          l = H[k] - 0.5 * q;
        }
      }
      if (nb == 1) l0 = l;
      else if (k < stride) row[k] = l;
      if (l > mx) mx = l;  // (a NaN is never greater)
    }
    const double m = stb_wave_all_max(mx);
    const bool dead = !isfinite(m);
    for (unsigned b = 0; b < nb; b++) {
      const unsigned k = b * 64 + lane;
      if (k < stride) {
        const double l = nb == 1 ? l0 : row[k];
        row[k] = (dead || k >= K) ? 0.0 : exp(l - m);
      }
    }
    if (dead && lane == 0) ndead++;
  }
  if (ndead) __hip_atomic_fetch_add(&ctl[GS_DEAD], ndead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(GS_MAXTHREADS) void k_gs_lik_reg(const double *x, unsigned D, uint64_t C, const double *muT,
                                                              const double *tauT, const double *H, unsigned K, double *lik,
                                                              unsigned stride, unsigned long long *ctl) {
  gs_lik<true>(x, D, C, muT, tauT, H, K, lik, stride, ctl);
}

__global__ __launch_bounds__(GS_MAXTHREADS) void k_gs_lik(const double *x, unsigned D, uint64_t C, const double *muT,
                                                          const double *tauT, const double *H, unsigned K, double *lik,
                                                          unsigned stride, unsigned long long *ctl) {
  gs_lik<false>(x, D, C, muT, tauT, H, K, lik, stride, ctl);
}

// what an object that takes observations starts from: the identity classes and a matrix of ones
__global__ __launch_bounds__(256) void k_gs_init(uint32_t *cls, uint64_t C, double *lik, uint64_t cells) {
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * 256) {
    lik[e] = 1.0;
    if (e < C) cls[e] = (uint32_t)e;
  }
}

// ---- the data term and the evidence -------------------------------------------------------------------------------

// terms 256 b .. 256 b + 255 (0.0 beyond `count`) are block b, summed by k_logjoint's tree; the last workgroup to finish
// adds the block sums in order in double-double and answers host[0] = (hi + lo) + add, host[1] (u64) = ctl's skipped
template <class F>
__device__ __forceinline__ void gs_block_sums(F term, uint64_t count, double *partial, unsigned nblk, unsigned long long *ctl,
                                              double add, double *host) {
  __shared__ double sx[GS_BLOCK];
  __shared__ double stage[GS_STAGE];
  __shared__ unsigned s_last;
  const unsigned nthr = blockDim.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  unsigned long long nskip = 0;
  for (unsigned blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const uint64_t e0 = (uint64_t)blk * GS_BLOCK;
    for (unsigned r = tid; r < GS_BLOCK; r += nthr) sx[r] = e0 + r < count ? term(e0 + r, nskip) : 0.0;
    __syncthreads();
    if (wave == 0) {
      const double v = stb_wave_sum((sx[lane] + sx[lane + 64]) + (sx[lane + 128] + sx[lane + 192]));
      if (lane == 0) partial[blk] = v;
    }
    __syncthreads();
  }
  nskip = stb_wave_sum(nskip);
  if (lane == 0 && nskip) __hip_atomic_fetch_add(&ctl[GS_SKIPPED], nskip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!stb_ticket_last((unsigned *)ctl, gridDim.x, &s_last)) return;
  dd_t acc{0.0, 0.0};
  for (unsigned b0 = 0; b0 < nblk; b0 += GS_STAGE) {
    const unsigned bn = nblk - b0 < GS_STAGE ? nblk - b0 : GS_STAGE;
    for (unsigned e = tid; e < bn; e += nthr) stage[e] = partial[b0 + e];
    __syncthreads();
    if (tid == 0)
      for (unsigned e = 0; e < bn; e++) dd_add(acc, stage[e]);
    __syncthreads();
  }
  if (tid == 0) {
    host[0] = (acc.hi + acc.lo) + add;
    ((unsigned long long *)host)[1] = __hip_atomic_load(&ctl[GS_SKIPPED], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// a thread a customer: v_c = H_k - 0.5 q_ck at k = cust[c], the matrix's own operations
__global__ __launch_bounds__(GS_MAXTHREADS) void k_gs_loglik(const double *x, unsigned D, const uint32_t *cust, uint64_t C,
                                                             const double *mu, const double *tau, const double *H, unsigned K,
                                                             double *partial, unsigned nblk, unsigned long long *ctl,
                                                             double add, double *host) {
  gs_block_sums(
      [=](uint64_t c, unsigned long long &nskip) -> double {
        const unsigned k = cust[c];
        if (k >= K) {
          nskip++;
          return 0.0;
        }
        const double *xc = x + c * D, *mk = mu + (uint64_t)k * D, *tk = tau + (uint64_t)k * D;
        double q = 0.0;
        for (unsigned d = 0; d < D; d++) {
          const double t = xc[d] - mk[d], s = (t * t) * tk[d];
          q = d ? q + s : s;
        }
        return H[k] - 0.5 * q;
      },
      C, partial, nblk, ctl, add, host);
}

// a thread a cell e = k D + d of the collapsed evidence
__global__ __launch_bounds__(GS_MAXTHREADS) void k_gs_logml(const uint32_t *n, const double *mean, const double *Q, unsigned K,
                                                            unsigned D, gs_prior_dev p, double *partial, unsigned nblk,
                                                            unsigned long long *ctl, double *host) {
  gs_block_sums(
      [=](uint64_t e, unsigned long long &) -> double {
        const unsigned k = (unsigned)(e / D), d = (unsigned)(e % D), nk = n[k];
        if (!nk) return 0.0;
        double kn, mn, an, bn;
        gs_posterior(p, d, nk, mean[e], Q[e], kn, mn, an, bn);
        const double b0 = p.beta0 ? p.beta0[d] : p.beta00;
        return ((((lgamma(an) - lgamma(p.alpha0)) + p.alpha0 * log(b0)) - an * log(bn)) + 0.5 * (log(p.kappa0) - log(kn))) -
               (0.5 * (double)nk) * 1.8378770664093453;
      },
      (uint64_t)K * D, partial, nblk, ctl, 0.0, host);
}

// ------------------------------------------------------------------------------------------------
// host side.  Every call takes its scratch from the buffer cache and gives it back behind its one wait.

unsigned stb_gs_waves() {
  return (unsigned)stb_env_waves("STB_GAUSS_WAVES", 4);
}

static unsigned gs_cap(uint64_t want) { return want < 1 ? 1u : (want > GS_CAP ? GS_CAP : (unsigned)want); }

struct gs_scratch {
  void *d = nullptr;      // device: ctl (256 bytes) first
  void *h = nullptr;      // pinned: 256 bytes of result words
  void *h_dev = nullptr;
  void *stage = nullptr;  // pinned: the caller's m0 / beta0 on their way to the device
  hipStream_t st = nullptr;
  bool queued = false;    // work that uses the buffers may be on st: wait before the cache hands them on
  ~gs_scratch() {
    if (queued) (void)hipStreamSynchronize(st);
    if (d) stb_pool_free(d);
    if (h) stb_pool_free(h);
    if (stage) stb_pool_free(stage);
  }
};

static int gs_take(gs_scratch &sc, size_t dev_bytes, size_t stage_bytes, hipStream_t st, const char *who) {
  sc.st = st;
  if (stb_pool_malloc(&sc.d, dev_bytes) != hipSuccess || stb_pool_malloc(&sc.h, 256, 1) != hipSuccess ||
      hipHostGetDevicePointer(&sc.h_dev, sc.h, 0) != hipSuccess ||
      (stage_bytes && stb_pool_malloc(&sc.stage, stage_bytes, 1) != hipSuccess))
    return stb_fail("%s: out of memory for %zu bytes of scratch", who, dev_bytes);
  return 0;
}

int stb_gs_check_shape(unsigned K, unsigned D, const char *who) {
  if (D < 1 || D > STB_GS_MAXD) return stb_fail("%s: D=%u (1 .. %d)", who, D, STB_GS_MAXD);
  if (K < 1 || K > STB_TD_MAXK) return stb_fail("%s: K=%u (1 .. %d)", who, K, STB_TD_MAXK);
  return 0;
}

int stb_gs_check_prior(const stb_gauss_prior_t *p, unsigned D, const char *who) {
  if (!p) return stb_fail("%s: a prior is required", who);
  if (!(p->kappa0 > 0.0) || !std::isfinite(p->kappa0)) return stb_fail("%s: kappa0=%g (must be > 0 and finite)", who, p->kappa0);
  if (!(p->alpha0 > 0.0) || !std::isfinite(p->alpha0)) return stb_fail("%s: alpha0=%g (must be > 0 and finite)", who, p->alpha0);
  if (!p->beta0 && (!(p->beta00 > 0.0) || !std::isfinite(p->beta00)))
    return stb_fail("%s: beta00=%g (must be > 0 and finite)", who, p->beta00);
  for (unsigned d = 0; d < D; d++) {
    if (p->beta0 && (!(p->beta0[d] > 0.0) || !std::isfinite(p->beta0[d])))
      return stb_fail("%s: beta0[%u]=%g (must be > 0 and finite)", who, d, p->beta0[d]);
    if (p->m0 && !std::isfinite(p->m0[d])) return stb_fail("%s: m0[%u]=%g (must be finite)", who, d, p->m0[d]);
  }
  return 0;
}

// the prior's vectors through sc.stage to d_vec (2 D doubles of device scratch), queued on st
static int gs_prior_to_device(const stb_gauss_prior_t *p, unsigned D, gs_scratch &sc, double *d_vec, hipStream_t st,
                              gs_prior_dev *out) {
  *out = {p->kappa0, p->alpha0, p->beta00, nullptr, nullptr};
  if (!p->m0 && !p->beta0) return 0;
  double *stage = (double *)sc.stage;
  if (p->m0) memcpy(stage, p->m0, 8 * (size_t)D);
  if (p->beta0) memcpy(stage + D, p->beta0, 8 * (size_t)D);
  HIPCHK(hipMemcpyAsync(d_vec, stage, 16 * (size_t)D, hipMemcpyHostToDevice, st));
  if (p->m0) out->m0 = d_vec;
  if (p->beta0) out->beta0 = d_vec + D;
  return 0;
}

// ctl's words to the pinned words, one wait, info
static int gs_finish(gs_scratch &sc, unsigned long long *ctl, stb_gauss_info_t *info, unsigned long long *err, hipStream_t st) {
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(sc.h, ctl, 32, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  sc.queued = false;
  const volatile unsigned long long *h = (const volatile unsigned long long *)sc.h;
  if (err) *err = h[GS_ERR];
  if (info) {
    info->skipped = h[GS_SKIPPED];
    info->dead = h[GS_DEAD];
  }
  return 0;
}

// the statistics' scratch: csum[nchunks x D x K], ccnt[nchunks x K]
static size_t gs_stats_bytes(uint64_t C, unsigned K, unsigned D) {
  const size_t nchunks = (size_t)((C + GS_CHUNK - 1) / GS_CHUNK);
  return 8 * nchunks * D * K + 4 * nchunks * K;
}

// the four launches of the statistics on st; ws: gs_stats_bytes of device scratch
static void gs_queue_stats(const double *d_x, unsigned D, const uint32_t *d_cust, uint64_t C, unsigned K, uint32_t *d_n,
                           double *d_mean, double *d_Q, char *ws, unsigned long long *ctl, hipStream_t st) {
  const unsigned nw = stb_gs_waves(), nchunks = (unsigned)((C + GS_CHUNK - 1) / GS_CHUNK), cb = (K + 63) / 64,
                 dz = (D + GS_DT - 1) / GS_DT;
  double *csum = (double *)ws;
  uint32_t *ccnt = (uint32_t *)(ws + 8 * (size_t)nchunks * D * K);
  const dim3 gs(cb, gs_cap((nchunks + nw - 1) / nw), dz), gf((K * D + 255) / 256);
  if (nchunks) STB_LAUNCH(k_gs_sum_a, gs, dim3(64 * nw), st, d_x, D, d_cust, C, K, csum, ccnt, nchunks, ctl);
  STB_LAUNCH(k_gs_fin_a, gf, dim3(256), st, csum, ccnt, nchunks, K, D, d_n, d_mean);
  if (nchunks) STB_LAUNCH(k_gs_sum_b, gs, dim3(64 * nw), st, d_x, D, d_cust, C, K, d_mean, csum, ccnt, nchunks);
  STB_LAUNCH(k_gs_fin_b, gf, dim3(256), st, csum, ccnt, nchunks, K, D, d_Q);
}

int stb_gs_stats(const double *d_x, unsigned D, const uint32_t *d_cust, uint64_t C, unsigned K, uint32_t *d_n, double *d_mean,
                 double *d_Q, stb_gauss_info_t *info, hipStream_t st, const char *who) {
  gs_scratch sc;
  if (gs_take(sc, 256 + gs_stats_bytes(C, K, D), 0, st, who)) return 1;
  char *d = (char *)sc.d;
  unsigned long long *ctl = (unsigned long long *)d;
  sc.queued = true;
  HIPCHK(hipMemsetAsync(d, 0, 256, st));
  gs_queue_stats(d_x, D, d_cust, C, K, d_n, d_mean, d_Q, d + 256, ctl, st);
  return gs_finish(sc, ctl, info, nullptr, st);
}

static int gs_draw_failed(unsigned long long err, uint64_t seed, uint64_t sweep, const char *who) {
  if (err & 1u)
    return stb_fail("%s: a Gamma draw was not accepted within %d attempts (seed=%llu, sweep=%llu); mu and tau are undefined", who,
                    HQ_CAP, (unsigned long long)seed, (unsigned long long)sweep);
  if (err) return stb_fail("%s: a precision is not positive and finite; mu and tau are undefined", who);
  return 0;
}

int stb_gs_draw(const uint32_t *d_n, const double *d_mean, const double *d_Q, unsigned K, unsigned D,
                const stb_gauss_prior_t *prior, uint64_t seed, uint64_t sweep, double *d_mu, double *d_tau, hipStream_t st,
                const char *who) {
  const unsigned nw = stb_gs_waves();
  gs_scratch sc;
  if (gs_take(sc, 256 + 16 * (size_t)D, 16 * (size_t)D, st, who)) return 1;
  char *d = (char *)sc.d;
  unsigned long long *ctl = (unsigned long long *)d;
  sc.queued = true;
  HIPCHK(hipMemsetAsync(d, 0, 256, st));
  gs_prior_dev p;
  if (gs_prior_to_device(prior, D, sc, (double *)(d + 256), st, &p)) return 1;
  const uint64_t key = stb_mix64(seed + (sweep + 1) * STB_GAMMA);
  STB_LAUNCH(k_gs_draw, dim3((K * D + 64 * nw - 1) / (64 * nw)), dim3(64 * nw), st, d_n, d_mean, d_Q, K, D, p, key, d_mu,
             d_tau, ctl);
  unsigned long long err = 0;
  if (gs_finish(sc, ctl, nullptr, &err, st)) return 1;
  return gs_draw_failed(err, seed, sweep, who);
}

// k_gs_prep and the matrix's kernel on st; T: 2 K D + K doubles of device scratch
static void gs_queue_lik(const double *d_x, unsigned D, uint64_t C, const double *d_mu, const double *d_tau, unsigned K,
                         double *d_lik, unsigned stride, double *T, unsigned long long *ctl, hipStream_t st) {
  const unsigned nw = stb_gs_waves();
  double *muT = T, *tauT = T + (size_t)K * D, *H = tauT + (size_t)K * D;
  STB_LAUNCH(k_gs_prep, dim3((K + 255) / 256), dim3(256), st, d_mu, d_tau, K, D, muT, tauT, H);
  if (!C) return;
  const dim3 grid(gs_cap((C + nw - 1) / nw)), block(64 * nw);
  if (K <= 64 && stride <= 64 && D <= GS_REG_D)
    STB_LAUNCH(k_gs_lik_reg, grid, block, st, d_x, D, C, muT, tauT, H, K, d_lik, stride, ctl);
  else
    STB_LAUNCH(k_gs_lik, grid, block, st, d_x, D, C, muT, tauT, H, K, d_lik, stride, ctl);
}

// k_gs_prep alone on st, no wait: T as gs_queue_lik's
void stb_gs_queue_prep(const double *d_mu, const double *d_tau, unsigned K, unsigned D, double *T, hipStream_t st) {
  STB_LAUNCH(k_gs_prep, dim3((K + 255) / 256), dim3(256), st, d_mu, d_tau, K, D, T, T + (size_t)K * D, T + 2 * (size_t)K * D);
}

int stb_gs_lik(const double *d_x, unsigned D, uint64_t C, const double *d_mu, const double *d_tau, unsigned K, double *d_lik,
               unsigned stride, stb_gauss_info_t *info, hipStream_t st, const char *who) {
  gs_scratch sc;
  if (gs_take(sc, 256 + 8 * (2 * (size_t)K * D + K), 0, st, who)) return 1;
  char *d = (char *)sc.d;
  unsigned long long *ctl = (unsigned long long *)d;
  sc.queued = true;
  HIPCHK(hipMemsetAsync(d, 0, 256, st));
  gs_queue_lik(d_x, D, C, d_mu, d_tau, K, d_lik, stride, (double *)(d + 256), ctl, st);
  return gs_finish(sc, ctl, info, nullptr, st);
}

// statistics, draw and matrix on st behind one another, one wait: the raw calls' launches in their order, so the bits are
// those of stb_gauss_stats, stb_sample_gauss and stb_gauss_lik called one after another
int stb_gs_step(const double *d_x, unsigned D, const uint32_t *d_cust, uint64_t C, unsigned K, const stb_gauss_prior_t *prior,
                uint64_t seed, uint64_t sweep, uint32_t *d_n, double *d_mean, double *d_Q, double *d_mu, double *d_tau,
                double *d_lik, unsigned stride, stb_gauss_info_t *info, hipStream_t st, const char *who, bool *touched) {
  const unsigned nw = stb_gs_waves();
  // scratch: ctl (256 bytes), the prior's vectors (2 D), muT, tauT, H (2 K D + K), the statistics'
  const size_t o_v = 256, o_T = o_v + 16 * (size_t)D, o_s = o_T + 8 * (2 * (size_t)K * D + K), bytes = o_s + gs_stats_bytes(C, K, D);
  gs_scratch sc;
  if (gs_take(sc, bytes, 16 * (size_t)D, st, who)) return 1;
  char *d = (char *)sc.d;
  unsigned long long *ctl = (unsigned long long *)d;
  sc.queued = true;
  HIPCHK(hipMemsetAsync(d, 0, 256, st));
  gs_prior_dev p;
  if (gs_prior_to_device(prior, D, sc, (double *)(d + o_v), st, &p)) return 1;
  const uint64_t key = stb_mix64(seed + (sweep + 1) * STB_GAMMA);
  if (touched) *touched = true;  // from here on mu, tau and the matrix are scratch until the last launch is through
  gs_queue_stats(d_x, D, d_cust, C, K, d_n, d_mean, d_Q, d + o_s, ctl, st);
  STB_LAUNCH(k_gs_draw, dim3((K * D + 64 * nw - 1) / (64 * nw)), dim3(64 * nw), st, d_n, d_mean, d_Q, K, D, p, key, d_mu,
             d_tau, ctl);
  gs_queue_lik(d_x, D, C, d_mu, d_tau, K, d_lik, stride, (double *)(d + o_T), ctl, st);
  unsigned long long err = 0;
  if (gs_finish(sc, ctl, info, &err, st)) return 1;
  return gs_draw_failed(err, seed, sweep, who);
}

// cls[c] = c and a C x stride matrix of ones, queued on st (no wait)
int stb_gs_init(uint32_t *d_cls, uint64_t C, double *d_lik, unsigned stride, hipStream_t st) {
  const uint64_t cells = C * stride;
  if (!cells) return 0;
  STB_LAUNCH(k_gs_init, dim3(gs_cap((cells + 255) / 256)), dim3(256), st, d_cls, C, d_lik, cells);
  HIPCHK(hipGetLastError());
  return 0;
}

// grid and block sums of a ticket reduction over `count` terms
static unsigned gs_blocks(uint64_t count) { return (unsigned)((count + GS_BLOCK - 1) / GS_BLOCK); }
static unsigned gs_ticket_grid(unsigned nblk) {
  const unsigned want = 4u * (unsigned)(stb_cu_count() > 0 ? stb_cu_count() : 1);
  return nblk < want ? nblk : want;
}

int stb_gs_loglik(const double *d_x, unsigned D, const uint32_t *d_cust, uint64_t C, const double *d_mu, const double *d_tau,
                  unsigned K, double *total_host, stb_gauss_info_t *info, hipStream_t st, const char *who) {
  const double add = (double)(C * D) * (-0.9189385332046727);
  if (info) *info = {0, 0};
  if (!C) {
    *total_host = add;
    return 0;
  }
  const unsigned nw = stb_gs_waves(), nblk = gs_blocks(C);
  // scratch: ctl (256 bytes), muT, tauT (unused by the sum, written by k_gs_prep), H[K], partial[nblk]
  const size_t o_T = 256, o_p = o_T + 8 * (2 * (size_t)K * D + K), bytes = o_p + 8 * (size_t)nblk;
  gs_scratch sc;
  if (gs_take(sc, bytes, 0, st, who)) return 1;
  char *d = (char *)sc.d;
  unsigned long long *ctl = (unsigned long long *)d;
  double *T = (double *)(d + o_T), *H = T + 2 * (size_t)K * D, *partial = (double *)(d + o_p);
  sc.queued = true;
  HIPCHK(hipMemsetAsync(d, 0, 256, st));
  STB_LAUNCH(k_gs_prep, dim3((K + 255) / 256), dim3(256), st, d_mu, d_tau, K, D, T, T + (size_t)K * D, H);
  STB_LAUNCH(k_gs_loglik, dim3(gs_ticket_grid(nblk)), dim3(64 * nw), st, d_x, D, d_cust, C, d_mu, d_tau, H, K, partial, nblk, ctl,
             add, (double *)sc.h_dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  sc.queued = false;
  *total_host = ((volatile double *)sc.h)[0];
  if (info) info->skipped = ((volatile unsigned long long *)sc.h)[1];
  return 0;
}

int stb_gs_logml(const uint32_t *d_n, const double *d_mean, const double *d_Q, unsigned K, unsigned D,
                 const stb_gauss_prior_t *prior, double *total_host, hipStream_t st, const char *who) {
  const unsigned nw = stb_gs_waves(), nblk = gs_blocks((uint64_t)K * D);
  // scratch: ctl (256 bytes), the prior's vectors (2 D), partial[nblk]
  const size_t o_v = 256, o_p = o_v + 16 * (size_t)D, bytes = o_p + 8 * (size_t)nblk;
  gs_scratch sc;
  if (gs_take(sc, bytes, 16 * (size_t)D, st, who)) return 1;
  char *d = (char *)sc.d;
  unsigned long long *ctl = (unsigned long long *)d;
  sc.queued = true;
  HIPCHK(hipMemsetAsync(d, 0, 256, st));
  gs_prior_dev p;
  if (gs_prior_to_device(prior, D, sc, (double *)(d + o_v), st, &p)) return 1;
  STB_LAUNCH(k_gs_logml, dim3(gs_ticket_grid(nblk)), dim3(64 * nw), st, d_n, d_mean, d_Q, K, D, p, (double *)(d + o_p), nblk, ctl,
             (double *)sc.h_dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  sc.queued = false;
  *total_host = ((volatile double *)sc.h)[0];
  return 0;
}

// ---- the raw layer ------------------------------------------------------------------------------------------------

extern "C" int stb_gauss_stats(const double *d_x, unsigned D, const uint32_t *d_cust, uint64_t C, unsigned K, uint32_t *d_n,
                               double *d_mean, double *d_Q, stb_gauss_info_t *info, void *stream) {
  STB_ENTRY;
  const char *who = "stb_gauss_stats";
  if (!d_n || !d_mean || !d_Q) return stb_fail("%s: d_n, d_mean and d_Q are required", who);
  if (C > 0 && (!d_x || !d_cust)) return stb_fail("%s: d_x and d_cust are required", who);
  if (C > 0xffffffffull) return stb_fail("%s: C=%llu (n_k is a uint32: at most 2^32 - 1 customers)", who, (unsigned long long)C);
  if (stb_gs_check_shape(K, D, who)) return 1;
  if (stb_device_count() < 1) return stb_no_device(who);
  return stb_gs_stats(d_x, D, d_cust, C, K, d_n, d_mean, d_Q, info, (hipStream_t)stream, who);
}

extern "C" int stb_sample_gauss(const uint32_t *d_n, const double *d_mean, const double *d_Q, unsigned K, unsigned D,
                                const stb_gauss_prior_t *prior, uint64_t seed, uint64_t sweep, double *d_mu, double *d_tau,
                                void *stream) {
  STB_ENTRY;
  const char *who = "stb_sample_gauss";
  if (!d_n || !d_mean || !d_Q || !d_mu || !d_tau) return stb_fail("%s: d_n, d_mean, d_Q, d_mu and d_tau are required", who);
  if (stb_gs_check_shape(K, D, who) || stb_gs_check_prior(prior, D, who)) return 1;
  if (stb_device_count() < 1) return stb_no_device(who);
  return stb_gs_draw(d_n, d_mean, d_Q, K, D, prior, seed, sweep, d_mu, d_tau, (hipStream_t)stream, who);
}

extern "C" int stb_gauss_lik(const double *d_x, unsigned D, uint64_t C, const double *d_mu, const double *d_tau, unsigned K,
                             double *d_lik, unsigned stride, stb_gauss_info_t *info, void *stream) {
  STB_ENTRY;
  const char *who = "stb_gauss_lik";
  if (!d_mu || !d_tau) return stb_fail("%s: d_mu and d_tau are required", who);
  if (C > 0 && (!d_x || !d_lik)) return stb_fail("%s: d_x and d_lik are required", who);
  if (stb_gs_check_shape(K, D, who)) return 1;
  if (stride < K) return stb_fail("%s: stride=%u below K=%u", who, stride, K);
  if (stb_device_count() < 1) return stb_no_device(who);
  return stb_gs_lik(d_x, D, C, d_mu, d_tau, K, d_lik, stride, info, (hipStream_t)stream, who);
}

extern "C" int stb_gauss_loglik(const double *d_x, unsigned D, const uint32_t *d_cust, uint64_t C, const double *d_mu,
                                const double *d_tau, unsigned K, double *total_host, stb_gauss_info_t *info, void *stream) {
  STB_ENTRY;
  const char *who = "stb_gauss_loglik";
  if (!d_mu || !d_tau || !total_host) return stb_fail("%s: d_mu, d_tau and total_host are required", who);
  if (C > 0 && (!d_x || !d_cust)) return stb_fail("%s: d_x and d_cust are required", who);
  if (stb_gs_check_shape(K, D, who)) return 1;
  if (stb_device_count() < 1) return stb_no_device(who);
  return stb_gs_loglik(d_x, D, d_cust, C, d_mu, d_tau, K, total_host, info, (hipStream_t)stream, who);
}

extern "C" int stb_gauss_logml(const uint32_t *d_n, const double *d_mean, const double *d_Q, unsigned K, unsigned D,
                               const stb_gauss_prior_t *prior, double *total_host, void *stream) {
  STB_ENTRY;
  const char *who = "stb_gauss_logml";
  if (!d_n || !d_mean || !d_Q || !total_host) return stb_fail("%s: d_n, d_mean, d_Q and total_host are required", who);
  if (stb_gs_check_shape(K, D, who) || stb_gs_check_prior(prior, D, who)) return 1;
  if (stb_device_count() < 1) return stb_no_device(who);
  return stb_gs_logml(d_n, d_mean, d_Q, K, D, prior, total_host, (hipStream_t)stream, who);
}
