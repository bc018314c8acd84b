// gauss_heldout.hip -- held-out points under Gaussian observations: the log predictive density of a point under a state's
// dish proportions, its responsibilities, and the log-domain accumulator over states (include/stb_hip.h, "Held-out points
// under Gaussian observations").  The per-(point, dish) arithmetic is gauss.hip's k_gs_lik; the sum
// over points is predict.hip's k_gh_sum.
//
//   k_gh_point_reg / k_gh_point  a wave a held-out point, lanes along k
//   k_gh_reset                   an empty accumulator
//
// Built with machine LICM off (the Makefile): hoisted out of the loop over points, the polynomial constants of exp and log
// alone hold 28 registers across it, and k_gh_point_reg would need 152 where it now fits 128 with nothing spilled.

#include "stb_common.h"
#include "ticket.h"
#include "gauss.h"
#include "predict.h"

#pragma clang fp contract(off)

#define GS_MAXTHREADS 512
#define GS_CAP 1024u   // workgroups of a grid at most (gauss.hip's)
#define GS_REG_D 16    // k_gh_point_reg keeps the block's mu and tau in registers up to this D (and K <= 64), as k_gs_lik_reg

// ---- held-out points ----------------------------------------------------------------------------------------------

// wave v of workgroup g: held-out points hoff[0] + g nw + v, + gridDim.x nw, ... up to hoff[I] (read on the device: the
// call does not wait for it).  The point's restaurant is the last i with hoff[i] <= j, found by a binary search whose
// every word is wave-uniform (scalar loads), as y_j's are.  Lanes along k in blocks of 64:
//   pass 1   l_jk = H_k - 0.5 q_jk (k_gs_lik's operations), the maximum over the dishes with theta_ik > 0
//   pass 2   w_jk = theta_ik exp(l_jk - m_j), a block by the shuffle tree, the block sums in block order
//   pass 3   (with resp) r_jk = w_jk / s_j
// REG: K <= 64 and D <= GS_REG_D, the one block's mu and tau, l and w in registers.  Else mu and tau come from the
// transposed copies and a point's l, then its w, wait in the wave's 8 (64 nb) bytes of LDS `sl` (every lane reads back
// what it wrote: no barrier) -- an LDS round trip where recomputing l would cost the D-loop a second time.
// Lane 0 owns the point's ell and its accumulator pair: S calls give the bits of the S updates in call order.
template <bool REG>
__device__ __forceinline__ void gh_point(const double *__restrict__ theta, unsigned tstride, uint64_t I,
                                         const uint64_t *__restrict__ hoff, const double *__restrict__ y, unsigned D,
                                         const double *__restrict__ muT, const double *__restrict__ tauT,
                                         const double *__restrict__ H, unsigned K, double *__restrict__ ell,
                                         double *__restrict__ resp, unsigned rstride, double *__restrict__ accM,
                                         double *__restrict__ accA, double *sl) {
  const unsigned nw = blockDim.x >> 6, wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)),
                 lane = threadIdx.x & 63;
  const unsigned nb = REG ? 1u : (K + 63) / 64, nrb = (rstride + 63) / 64;
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
  const uint64_t c1 = hoff[I];
  for (uint64_t j = hoff[0] + (uint64_t)blockIdx.x * nw + wave; j < c1; j += (uint64_t)gridDim.x * nw) {
    uint64_t lo = 0, hi = I;  // hoff[lo] <= j < hoff[hi]
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (hoff[mid] <= j) lo = mid;
      else hi = mid;
    }
    const double *yj = y + j * D, *th = theta + lo * tstride;
    double mx = -INFINITY, l0 = -INFINITY, t0 = 0.0;
    for (unsigned b = 0; b < nb; b++) {
      const unsigned k = b * 64 + lane;
      double l = -INFINITY, t = 0.0;
      if (k < K) {
        t = th[k];
        double q = 0.0;
        if (REG) {
#pragma unroll
          for (unsigned d = 0; d < GS_REG_D; d++) {
            if (d < D) {
              const double v = yj[d] - mr[d], s = (v * v) * tr[d];
              q = d ? q + s : s;
            }
          }
          l = hr - 0.5 * q;
        } else {
          for (unsigned d = 0; d < D; d++) {
            const double v = yj[d] - muT[(uint64_t)d * K + k], s = (v * v) * tauT[(uint64_t)d * K + k];
            q = d ? q + s : s;
          }
          l = H[k] - 0.5 * q;
        }
      }
      if (REG) {
        l0 = l;
        t0 = t;
      } else {
        sl[k] = l;
      }
      if (t > 0.0 && l > mx) mx = l;  // (a NaN is never greater)
    }
    const double m = stb_wave_all_max(mx);
    const bool dead = !isfinite(m);
    double s = 0.0, w0 = 0.0;
    for (unsigned b = 0; b < nb; b++) {
      const unsigned k = b * 64 + lane;
      const double l = REG ? l0 : sl[k], t = REG ? t0 : (k < K ? th[k] : 0.0);
      const double w = (!dead && k < K && t > 0.0) ? t * exp(l - m) : 0.0;
      if (REG) w0 = w;
      else sl[k] = w;
      const double sb = stb_wave_sum(w);
      s = b ? s + sb : sb;
    }
    s = __shfl(s, 0, 64);
    const double e = dead ? -INFINITY : (m + log(s)) + (double)D * (-0.9189385332046727);
    if (lane == 0) {
      if (ell) ell[j] = e;
      if (accM && !dead) {
        double M = accM[j], A = accA[j];
        if (e > M) {
          A = M == -INFINITY ? 1.0 : A * exp(M - e) + 1.0;
          M = e;
        } else {
          A = A + exp(e - M);
        }
        accM[j] = M;
        accA[j] = A;
      }
    }
    if (resp) {
      double *row = resp + j * rstride;
      for (unsigned b = 0; b < nrb; b++) {
        const unsigned k = b * 64 + lane;
        if (k < rstride) {
          const double w = k < K ? (REG ? w0 : sl[k]) : 0.0;
          row[k] = dead ? 0.0 : w / s;
        }
      }
    }
  }
}

__global__ __launch_bounds__(GS_MAXTHREADS) void k_gh_point_reg(const double *theta, unsigned tstride, uint64_t I,
                                                                const uint64_t *hoff, const double *y, unsigned D,
                                                                const double *muT, const double *tauT, const double *H,
                                                                unsigned K, double *ell, double *resp, unsigned rstride,
                                                                double *accM, double *accA) {
  gh_point<true>(theta, tstride, I, hoff, y, D, muT, tauT, H, K, ell, resp, rstride, accM, accA, nullptr);
}

// dynamic LDS: 64 ceil(K / 64) doubles a wave
__global__ __launch_bounds__(GS_MAXTHREADS) void k_gh_point(const double *theta, unsigned tstride, uint64_t I,
                                                            const uint64_t *hoff, const double *y, unsigned D,
                                                            const double *muT, const double *tauT, const double *H, unsigned K,
                                                            double *ell, double *resp, unsigned rstride, double *accM,
                                                            double *accA) {
  extern __shared__ double gh_lds[];
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  gh_point<false>(theta, tstride, I, hoff, y, D, muT, tauT, H, K, ell, resp, rstride, accM, accA,
                  gh_lds + (size_t)wave * 64 * ((K + 63) / 64));
}

// an empty accumulator: (M, A) = (-inf, 0.0), standing for A e^M = 0
__global__ __launch_bounds__(256) void k_gh_reset(double *accM, double *accA, uint64_t n) {
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (uint64_t)gridDim.x * 256) {
    accM[e] = -INFINITY;
    accA[e] = 0.0;
  }
}

// ---- held-out points: the host side ---------------------------------------------------------------------------------

// per calling thread: muT, tauT and H of the call in flight (d_buf).  stb_gs_heldout queues and returns, so the buffer
// stays with the thread; calls of one thread are ordered by their stream (a thread that scores on two streams at once
// must wait for one before it queues on the other), and a buffer that has to grow waits for the stream first.
static thread_local stb_tset gh;

extern "C" void stb_gh_release(void) {
  STB_ENTRY;
  stb_tset_drop(gh);
}

int stb_gs_heldout(const double *d_theta, unsigned tstride, int I, const uint64_t *d_hoff, const double *d_y, unsigned D,
                   const double *d_mu, const double *d_tau, unsigned K, double *d_ell, double *d_resp, unsigned rstride,
                   double *d_accM, double *d_accA, hipStream_t st, const char *who) {
  if (I == 0) return 0;
  const unsigned nw = stb_gs_waves();
  const size_t need = 2 * (size_t)K * D + K;
  if (stb_tset_ready(gh, who, false)) return 1;
  if (need > gh.cap && gh.d_buf) HIPCHK(hipStreamSynchronize(st));
  if (stb_tset_room(gh, need, 0, sizeof(double), who)) return 1;
  double *muT = (double *)gh.d_buf, *tauT = muT + (size_t)K * D, *H = tauT + (size_t)K * D;
  stb_gs_queue_prep(d_mu, d_tau, K, D, muT, st);
  // (the number of points is hoff[I], on the device: the capped grid, whose idle waves leave at once)
  const dim3 grid(GS_CAP), block(64 * nw);
  if (K <= 64 && D <= GS_REG_D)
    STB_LAUNCH(k_gh_point_reg, grid, block, st, d_theta, tstride, (uint64_t)I, d_hoff, d_y, D, muT, tauT, H, K, d_ell, d_resp,
               rstride, d_accM, d_accA);
  else
    STB_LAUNCH_SHM(k_gh_point, grid, block, sizeof(double) * 64 * ((K + 63) / 64) * nw, st, d_theta, tstride, (uint64_t)I, d_hoff,
                   d_y, D, muT, tauT, H, K, d_ell, d_resp, rstride, d_accM, d_accA);
  HIPCHK(hipGetLastError());
  return 0;
}

int stb_gs_heldout_reset(double *d_accM, double *d_accA, uint64_t n, hipStream_t st) {
  if (!n) return 0;
  STB_LAUNCH(k_gh_reset, dim3((unsigned)((n + 255) / 256 < GS_CAP ? (n + 255) / 256 : GS_CAP)), dim3(256), st, d_accM, d_accA, n);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int stb_gauss_heldout(const double *d_theta, unsigned tstride, int I, const uint64_t *d_hoff, const double *d_y,
                                 unsigned D, const double *d_mu, const double *d_tau, unsigned K, double *d_ell, double *d_resp,
                                 unsigned rstride, double *d_accM, double *d_accA, unsigned flags, void *stream) {
  STB_ENTRY;
  const char *who = "stb_gauss_heldout";
  if (flags & ~STB_GH_ACCUMULATE) return stb_fail("%s: unknown flags 0x%x", who, flags);
  if (I < 0) return stb_fail("%s: I=%d", who, I);
  if (!d_theta || !d_hoff || !d_y || !d_mu || !d_tau) return stb_fail("%s: d_theta, d_hoff, d_y, d_mu and d_tau are required", who);
  if (stb_gs_check_shape(K, D, who)) return 1;
  if (tstride < K) return stb_fail("%s: tstride=%u below K=%u", who, tstride, K);
  if (d_resp && rstride < K) return stb_fail("%s: rstride=%u below K=%u", who, rstride, K);
  const bool accumulate = (flags & STB_GH_ACCUMULATE) != 0;
  if (accumulate && (!d_accM || !d_accA)) return stb_fail("%s: STB_GH_ACCUMULATE needs both accumulator arrays (d_accM, d_accA)", who);
  if (stb_device_count() < 1) return stb_no_device(who);
  return stb_gs_heldout(d_theta, tstride, I, d_hoff, d_y, D, d_mu, d_tau, K, d_ell, d_resp, d_resp ? rstride : 0,
                        accumulate ? d_accM : nullptr, accumulate ? d_accA : nullptr, (hipStream_t)stream, who);
}

extern "C" int stb_gauss_heldout_loglik(const double *d_ell, const double *d_accM, const double *d_accA, unsigned samples,
                                        const uint64_t *d_hoff, int I, double *d_Hi, double *total_host,
                                        stb_predict_info_t *info, void *stream) {
  STB_ENTRY;
  const char *who = "stb_gauss_heldout_loglik";
  if (I < 0) return stb_fail("%s: I=%d", who, I);
  if (!total_host) return stb_fail("%s: total_host is required", who);
  if ((d_accM != nullptr) != (d_accA != nullptr)) return stb_fail("%s: the accumulator is a pair (d_accM, d_accA)", who);
  if (d_accM && samples < 1) return stb_fail("%s: samples=0", who);
  if (!d_accM && !d_ell) return stb_fail("%s: d_ell, or the accumulator pair, is required", who);
  if (!d_hoff) return stb_fail("%s: the held-out offsets are required", who);
  return stb_pr_heldout_log(d_accM ? d_accM : d_ell, d_accM ? d_accA : nullptr, d_accM ? samples : 1u, d_hoff, I, d_Hi, nullptr,
                            total_host, info, (hipStream_t)stream, who);
}
