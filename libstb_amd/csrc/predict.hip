// predict.hip -- what a sampler state predicts: a restaurant's dish proportions, the probability of held-out customers
// under them, and the held-out log likelihood averaged over states (include/stb_hip.h, stb_predict_dishes and
// stb_heldout_loglik; an additive interface: the reference has no counterpart).
//
//     theta_ik = ((n_k - t_k a) + g_i h_k) / (b_i + N_i),   g_i = b_i + T_i a,   T_i = sum_k t_k,   N_i = sum_k n_k
//     p_c      = sum_k theta_ik lik[cls_c stride + k]        a held-out customer c of restaurant i
//     H_i      = sum_c log(p_c / samples)                    p_c accumulated over `samples` states
//
//   k_predict      a wave a restaurant, grid-stride; restaurants are independent: nobody waits for anybody
//   k_heldout_sum  k_logjoint's shape (logjoint.hip): blocks of 256 restaurants, a wave a restaurant, the block sums added
//                  by the last workgroup to finish (a ticket); geometry and ticket from ticket.h
//   k_gh_sum       the same body on log densities, or on log-domain accumulator pairs (gauss.hip's held-out points)
//
// The association (no contraction anywhere; FP64 throughout; u32 / u64 integers are exact) is the header's, word for
// word; tests/pr_oracle.py replays it.  In short:
//   k_predict  T_i, N_i: uint64 sums over the restaurant's pairs (no d_T is read).  T = (double)T_i, N = (double)N_i,
//       g = b + T a, den = b + N; per dish x = (double)n - (double)t a, theta = (x + g h) / den (h = 1 without d_h);
//       N_i = 0: theta = h.  Dishes in blocks of 64, lane l the dish 64 j + l, q = theta L (+0.0 past K_i); a block is
//       summed by the shuffle tree v += shfl_down(v, o), o = 32 .. 1, lane 0 taken; p = s_0, then p = p + s_j, j = 1, 2, ..
//   k_heldout_sum  x_c = log(p_c / (double)samples); a restaurant's customers in chunks of 64 in CSR order through the
//       same tree (+0.0 past the end and for impossible customers), the chunk sums added in order in double-double,
//       H_i = hi + lo; over restaurants k_logjoint's block tree and ordered double-double sum.
// So no output's bits depend on the grid or the workgroup size: STB_PREDICT_WAVES = 1, 2, 4 or 8 give the same bits.
//
// The form of k_predict is chosen per restaurant, wave-uniformly: K_i <= 64 keeps theta a lane a dish in a register,
// K_i > 64 keeps it in the wave's 8 KB of LDS (8 B a dish, lane l reads back what lane l wrote: no barrier).  The
// arithmetic is the same in both, so a restaurant's bits do not depend on which other restaurants share the call.
//
// What sets the pace: a held-out customer costs one gathered, coalesced 512-byte row load a block of dishes and one
// dependent six-step tree.  The wave loads the classes of 64 customers in one coalesced read, then takes the customers
// PR_CUST at a time: their row loads are issued together ahead of the first tree, and the PR_CUST trees are independent of
// each other, so their shuffles interleave.  The 64 results are gathered into lanes and stored (or added to p) coalesced;
// one lane owns a customer, so S accumulating calls give the bits of the S values added in call order.

#include "stb_common.h"
#include "predict.h"
#include "ticket.h"

#define PR_BLOCK STB_TG_BLOCK  // restaurants of a block sum in k_heldout_sum
#define PR_MAXTHREADS 512
#define PR_STAGE 1024  // block sums the last workgroup stages in LDS at a time
#define PR_CUST 4      // customers whose row loads are in flight before the first tree

// dynamic LDS: STB_TD_MAXK doubles a wave
__global__ __launch_bounds__(PR_MAXTHREADS) void k_predict(double a, const double *bpar, uint64_t I, const uint64_t *koff,
                                                           const uint32_t *nv, const uint16_t *tv, const double *hv,
                                                           double *theta, unsigned tstride, const uint64_t *hoff,
                                                           const uint32_t *hcls, const double *lik, unsigned rows,
                                                           unsigned stride, double *p, unsigned flags,
                                                           unsigned long long *skipped) {
#pragma clang fp contract(off)
  extern __shared__ double pr_lds[];
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  double *sth = pr_lds + (size_t)wave * STB_TD_MAXK;
  const bool accumulate = (flags & STB_PR_ACCUMULATE) != 0;
  unsigned long long nskip = 0;  // lane 0's count
  for (uint64_t i = (uint64_t)blockIdx.x * nw + wave; i < I; i += (uint64_t)gridDim.x * nw) {
    const uint64_t k0 = koff[i], K = koff[i + 1] - k0;
    const uint64_t c0 = hoff ? hoff[i] : 0, c1 = hoff ? hoff[i + 1] : 0;
    if (K > STB_TD_MAXK || (lik && K > stride) || (theta && K > tstride)) {
      nskip++;
      if (theta)
        for (unsigned k = lane; k < tstride; k += 64) theta[i * tstride + k] = 0.0;
      if (!accumulate)
        for (uint64_t c = c0 + lane; c < c1; c += 64) p[c] = 0.0;
      continue;
    }
    const unsigned Ki = (unsigned)K, nb = (Ki + 63) / 64;
    // ---- T_i and N_i, the kernel's own sums
    unsigned long long sT = 0, sN = 0;
    for (unsigned k = lane; k < Ki; k += 64) {
      sT += tv[k0 + k];
      sN += nv[k0 + k];
    }
    sT = __shfl(stb_wave_sum(sT), 0, 64);
    sN = __shfl(stb_wave_sum(sN), 0, 64);
    // ---- theta: a lane a dish
    const double b = bpar[i], Td = (double)sT, Nd = (double)sN;
    const double g = b + Td * a, den = b + Nd;
    double th0 = 0.0;
    for (unsigned j = 0; j < nb; j++) {
      const unsigned k = 64 * j + lane;
      double th = 0.0;
      if (k < Ki) {
        const double h = hv ? hv[k0 + k] : 1.0;
        if (sN == 0) {
          th = h;
        } else {
          const double x = (double)nv[k0 + k] - (double)tv[k0 + k] * a;
          th = (x + g * h) / den;
        }
      }
      if (nb == 1) th0 = th;
      else sth[k] = th;
      if (theta && k < tstride) theta[i * tstride + k] = th;
    }
    if (theta)
      for (unsigned k = 64 * nb + lane; k < tstride; k += 64) theta[i * tstride + k] = 0.0;
    // ---- the held-out customers, 64 at a time
    for (uint64_t cb = c0; cb < c1; cb += 64) {
      const unsigned cn = c1 - cb < 64 ? (unsigned)(c1 - cb) : 64u;
      const unsigned mycls = lane < cn ? hcls[cb + lane] : 0xffffffffu;
      double pv = 0.0;
      for (unsigned j0 = 0; j0 < cn; j0 += PR_CUST) {
        unsigned cls[PR_CUST];
        double acc[PR_CUST];
#pragma unroll
        for (int c = 0; c < PR_CUST; c++) {
          cls[c] = __shfl(mycls, (int)((j0 + c) & 63u), 64);  // (past cn: 0xffffffff, or a customer taken again -- dropped below)
          acc[c] = 0.0;
        }
        for (unsigned j = 0; j < nb; j++) {
          const unsigned k = 64 * j + lane;
          const double th = nb == 1 ? th0 : sth[k];
          double L[PR_CUST];
#pragma unroll
          for (int c = 0; c < PR_CUST; c++)
            L[c] = k < Ki ? (lik ? (cls[c] < rows ? lik[(size_t)cls[c] * stride + k] : 0.0) : 1.0) : 0.0;
#pragma unroll
          for (int c = 0; c < PR_CUST; c++) {
            const double s = stb_wave_sum(k < Ki ? th * L[c] : 0.0);
            acc[c] = j == 0 ? s : acc[c] + s;
          }
        }
#pragma unroll
        for (int c = 0; c < PR_CUST; c++) {
          const double r = __shfl(acc[c], 0, 64);
          if (lane == j0 + c) pv = r;
        }
      }
      if (lane < cn) p[cb + lane] = accumulate ? p[cb + lane] + pv : pv;
    }
  }
  if (lane == 0 && nskip && skipped) __hip_atomic_fetch_add(skipped, nskip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ctl: [0] ticket (u32); as u64 word 1: impossible customers -- zeroed on the stream ahead of the launch.
// host: [0] total, as u64 [1] impossible, [2] customers, [3] skipped (copied from skipped_in, 0 without one)
//
// The body serves two kernels that differ in what a customer's term x_c is taken from and in nothing else:
//   PR_X_P       k_heldout_sum: p holds probabilities, x_c = log(p_c / samples)
//   PR_X_LOG     k_gh_sum (stb_gauss_heldout_loglik): p holds log densities, x_c = p_c; not finite: impossible
//   PR_X_LOGACC  k_gh_sum: (p, A) hold the log-domain accumulator pairs (M_c, A_c), x_c = M_c + log(A_c / samples);
//                A_c / samples not positive and finite: impossible
struct pr_sum_lds {  // a kernel's one copy, whichever forms of the body it holds
  double sx[PR_BLOCK];  // H_i of the block's restaurants (the possible customers' sum)
  unsigned sflag[PR_BLOCK];
  double stage[PR_STAGE];
  unsigned s_last;
};
#define PR_X_P 0
#define PR_X_LOG 1
#define PR_X_LOGACC 2
template <int X>
__device__ __forceinline__ void pr_heldout_sum(const double *p, const double *A, const uint64_t *hoff, uint64_t I,
                                               double samples, double *Hi, double *partial, unsigned nblk, unsigned *ctl,
                                               double *host, const unsigned long long *skipped_in, pr_sum_lds &lds) {
#pragma clang fp contract(off)
  double *sx = lds.sx, *stage = lds.stage;
  unsigned *sflag = lds.sflag;
  const unsigned nthr = blockDim.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nw = nthr >> 6;
  unsigned long long c_imp = 0;  // per lane, over everything the lane sees
  for (unsigned blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const uint64_t i0 = (uint64_t)blk * PR_BLOCK;
    // ---- the customers: a wave a restaurant
    for (unsigned r = wave; r < PR_BLOCK && i0 + r < I; r += nw) {
      const uint64_t c0 = hoff[i0 + r], c1 = hoff[i0 + r + 1];
      dd_t acc{0.0, 0.0};
      unsigned bad = 0;
      for (uint64_t base = c0; base < c1; base += 64) {
        const uint64_t c = base + lane;
        double x = 0.0;
        if (c < c1) {
          bool ok;
          if (X == PR_X_P) {
            const double pc = p[c], q = pc / samples;
            ok = q > 0.0 && isfinite(pc);
            if (ok) x = log(q);
          } else if (X == PR_X_LOG) {
            const double l = p[c];
            ok = isfinite(l);
            if (ok) x = l;
          } else {
            const double q = A[c] / samples;
            ok = q > 0.0 && isfinite(q);
            if (ok) x = p[c] + log(q);
          }
          if (!ok) {
            bad = 1;
            c_imp++;
          }
        }
        dd_add(acc, stb_wave_sum(x));
      }
      const unsigned any = __ballot(bad) != 0ull ? 1u : 0u;
      if (lane == 0) {
        sx[r] = acc.hi + acc.lo;
        sflag[r] = any;
      }
    }
    __syncthreads();
    for (unsigned r = tid; r < PR_BLOCK; r += nthr) {
      const uint64_t i = i0 + r;
      if (i < I) {
        if (Hi) Hi[i] = sflag[r] ? -HUGE_VAL : sx[r];
      } else {
        sx[r] = 0.0;
      }
    }
    __syncthreads();
    // ---- the block's sum, the one fixed tree
    if (wave == 0) {
      const double v = stb_wave_sum((sx[lane] + sx[lane + 64]) + (sx[lane + 128] + sx[lane + 192]));
      if (lane == 0) partial[blk] = v;
    }
    __syncthreads();
  }
  c_imp = stb_wave_sum(c_imp);
  unsigned long long *cnt = (unsigned long long *)ctl;
  if (lane == 0 && c_imp) __hip_atomic_fetch_add(&cnt[1], c_imp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!stb_ticket_last(ctl, gridDim.x, &lds.s_last)) return;  // (ticket.h: the block sums and the counter are published)
  dd_t tot{0.0, 0.0};  // thread 0's
  for (unsigned b0 = 0; b0 < nblk; b0 += PR_STAGE) {
    const unsigned bn = nblk - b0 < PR_STAGE ? nblk - b0 : PR_STAGE;
    for (unsigned e = tid; e < bn; e += nthr) stage[e] = partial[(size_t)b0 + e];
    __syncthreads();
    if (tid == 0)
      for (unsigned e = 0; e < bn; e++) dd_add(tot, stage[e]);
    __syncthreads();
  }
  if (tid == 0) {
    const unsigned long long n_imp = __hip_atomic_load(&cnt[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    host[0] = n_imp ? -HUGE_VAL : tot.hi + tot.lo;
    unsigned long long *hc = (unsigned long long *)host;
    hc[1] = n_imp;
    hc[2] = hoff[I] - hoff[0];
    hc[3] = skipped_in ? *skipped_in : 0ull;
  }
}

__global__ __launch_bounds__(PR_MAXTHREADS) void k_heldout_sum(const double *p, const uint64_t *hoff, uint64_t I,
                                                               double samples, double *Hi, double *partial, unsigned nblk,
                                                               unsigned *ctl, double *host,
                                                               const unsigned long long *skipped_in) {
  __shared__ pr_sum_lds lds;
  pr_heldout_sum<PR_X_P>(p, nullptr, hoff, I, samples, Hi, partial, nblk, ctl, host, skipped_in, lds);
}

// A null: x holds log densities; else (x, A) the accumulator pairs of `samples` states
__global__ __launch_bounds__(PR_MAXTHREADS) void k_gh_sum(const double *x, const double *A, const uint64_t *hoff, uint64_t I,
                                                          double samples, double *Hi, double *partial, unsigned nblk,
                                                          unsigned *ctl, double *host) {
  __shared__ pr_sum_lds lds;
  if (A) pr_heldout_sum<PR_X_LOGACC>(x, A, hoff, I, samples, Hi, partial, nblk, ctl, host, nullptr, lds);
  else pr_heldout_sum<PR_X_LOG>(x, nullptr, hoff, I, samples, Hi, partial, nblk, ctl, host, nullptr, lds);
}

// ------------------------------------------------------------------------------------------------
// per calling thread: the block sums, the ticket and counter, and the pinned words k_heldout_sum answers in.  A call
// waits for its answer before it returns, so one set per thread is never in use twice.

static thread_local stb_tset pr;

extern "C" void stb_pr_release(void) {
  STB_ENTRY;
  stb_tset_drop(pr);
}

int stb_pr_check(double a, unsigned flags, int I, const char *who) {
  if (!(a >= 0.0 && a < 1.0)) return stb_fail("%s: discount a=%g outside [0, 1)", who, a);
  if (flags & ~STB_PR_ACCUMULATE) return stb_fail("%s: unknown flags 0x%x", who, flags);
  if (I < 0) return stb_fail("%s: I=%d", who, I);
  return 0;
}

int stb_pr_predict(const stb_rest_view &r, const stb_cnts_ro &c, const stb_cust_ro &held, const stb_lik_view &L,
                   const stb_pr_out &out, unsigned flags, hipStream_t st, const char *who) {
  const int I = r.I;
  if (I == 0) return 0;
  if (stb_device_count() < 1) return stb_no_device(who);
  int nw = stb_env_waves("STB_PREDICT_WAVES", 0);
  if (!nw) nw = 4;
  const int cus = stb_cu_count();
  const uint64_t want = 32ull * (uint64_t)(cus > 0 ? cus : 1), groups = ((uint64_t)I + nw - 1) / nw;
  const unsigned grid = (unsigned)(groups < want ? groups : want);
  STB_LAUNCH_SHM(k_predict, dim3(grid), dim3(64 * nw), sizeof(double) * STB_TD_MAXK * nw, st, r.a, r.bpar, (uint64_t)I, r.koff,
                 c.n, c.t, r.h, out.theta, out.tstride, held.off, held.cls, L.lik, L.rows, L.stride, out.p, flags,
                 (unsigned long long *)out.skipped);
  HIPCHK(hipGetLastError());
  return 0;
}

// log: k_gh_sum on (d_p, d_A) instead of k_heldout_sum on d_p
static int pr_heldout(bool log, const double *d_p, const double *d_A, const uint64_t *d_hoff, int I, unsigned samples,
                      double *d_Hi, double *Hi_host, double *total_host, stb_predict_info_t *info, const uint64_t *d_skipped,
                      hipStream_t st, const char *who) {
  if (I == 0) {
    if (total_host) *total_host = 0.0;
    if (info) memset(info, 0, sizeof(*info));
    return 0;
  }
  if (stb_device_count() < 1) return stb_no_device(who);
  stb_tgeom tg;  // k_logjoint's geometry; the workgroup size from STB_PREDICT_WAVES where it is set
  if (stb_ticket_geom(STB_GEOM_LOGJOINT, (uint64_t)I, 0, 0, stb_env_waves("STB_PREDICT_WAVES", 0), &tg))
    return stb_fail("%s: no launch geometry for I=%d", who, I);
  if (stb_tset_ready(pr, who) || stb_tset_room(pr, tg.need, STB_TG_CAP0_BLOCKS, sizeof(double), who)) return 1;
  HIPCHK(hipMemsetAsync(pr.d_ctl, 0, 64, st));
  if (log)
    STB_LAUNCH(k_gh_sum, dim3(tg.gx), dim3(64 * tg.waves), st, d_p, d_A, d_hoff, (uint64_t)I, (double)samples, d_Hi,
               (double *)pr.d_buf, tg.nblk, pr.d_ctl, pr.h_out_dev);
  else
    STB_LAUNCH(k_heldout_sum, dim3(tg.gx), dim3(64 * tg.waves), st, d_p, d_hoff, (uint64_t)I, (double)samples, d_Hi,
               (double *)pr.d_buf, tg.nblk, pr.d_ctl, pr.h_out_dev, (const unsigned long long *)d_skipped);
  HIPCHK(hipGetLastError());
  if (d_Hi && Hi_host) HIPCHK(hipMemcpyAsync(Hi_host, d_Hi, sizeof(double) * (size_t)I, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const volatile double *h = (const volatile double *)pr.h_out;
  const volatile uint64_t *hc = (const volatile uint64_t *)pr.h_out;
  if (total_host) *total_host = h[0];
  if (info) {
    info->impossible = hc[1];
    info->customers = hc[2];
    info->skipped = hc[3];
  }
  return 0;
}

int stb_pr_heldout(const double *d_p, const uint64_t *d_hoff, int I, unsigned samples, double *d_Hi, double *Hi_host,
                   double *total_host, stb_predict_info_t *info, const uint64_t *d_skipped, hipStream_t st, const char *who) {
  return pr_heldout(false, d_p, nullptr, d_hoff, I, samples, d_Hi, Hi_host, total_host, info, d_skipped, st, who);
}

int stb_pr_heldout_log(const double *d_x, const double *d_A, unsigned samples, const uint64_t *d_hoff, int I, double *d_Hi,
                       double *Hi_host, double *total_host, stb_predict_info_t *info, hipStream_t st, const char *who) {
  return pr_heldout(true, d_x, d_A, d_hoff, I, samples, d_Hi, Hi_host, total_host, info, nullptr, st, who);
}

extern "C" int stb_predict_dishes(double a, const double *d_bpar, int I, const uint64_t *d_koff, const uint32_t *d_n,
                                  const uint16_t *d_t, const double *d_h, double *d_theta, unsigned tstride,
                                  const uint64_t *d_hoff, const uint32_t *d_hcls, const double *d_lik, unsigned rows,
                                  unsigned stride, double *d_p, unsigned flags, uint64_t *d_skipped, void *stream) {
  STB_ENTRY;
  const char *who = "stb_predict_dishes";
  if (stb_pr_check(a, flags, I, who)) return 1;
  if (!d_koff || !d_n || !d_t) return stb_fail("%s: the pair offsets, n and t are required", who);
  if (I > 0 && !d_bpar) return stb_fail("%s: bpar is required", who);
  if (d_hoff && (!d_hcls || !d_p)) return stb_fail("%s: held-out offsets need their classes and p (d_hcls, d_p are required)", who);
  if (d_lik && (rows < 1 || stride < 1)) return stb_fail("%s: a likelihood of rows=%u stride=%u", who, rows, stride);
  if (d_theta && tstride < 1) return stb_fail("%s: theta with tstride=%u", who, tstride);
  const stb_rest_view r = {a, d_bpar, I, d_koff, d_h};
  const stb_cust_ro held = {d_hoff, d_hcls};
  const stb_lik_view L = {d_lik, rows, stride};
  const stb_pr_out out = {d_theta, tstride, d_p, d_skipped};
  return stb_pr_predict(r, {d_n, d_t}, held, L, out, flags, (hipStream_t)stream, who);
}

extern "C" int stb_heldout_loglik(const double *d_p, const uint64_t *d_hoff, int I, unsigned samples, double *d_Hi,
                                  double *total_host, stb_predict_info_t *info, void *stream) {
  STB_ENTRY;
  const char *who = "stb_heldout_loglik";
  if (I < 0) return stb_fail("%s: I=%d", who, I);
  if (samples < 1) return stb_fail("%s: samples=0", who);
  if (!total_host) return stb_fail("%s: total_host is required", who);
  if (I > 0 && (!d_p || !d_hoff)) return stb_fail("%s: p and the held-out offsets are required", who);
  return stb_pr_heldout(d_p, d_hoff, I, samples, d_Hi, nullptr, total_host, info, nullptr, (hipStream_t)stream, who);
}
