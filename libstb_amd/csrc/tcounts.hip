// tcounts.hip -- the table-count step of a Pitman-Yor Gibbs sampler on the device: a collapsed Gibbs sweep that
// redraws every t[i][k] from its conditional given the other table counts of its restaurant.
//
//   k_tcounts   one workgroup per restaurant; its pairs in order, the tau range of a pair across the workgroup
//
// For a pair (n, t, h) of restaurant i with concentration b, discount a and T_ = T_i - t, the conditional is
//     log w(tau) = S_S(n, tau) + (tau-1) log h + sum_{s=T_+1}^{T_+tau-1} log(b + s a),   tau = 1 .. min(n, M)
// from the PYP joint (b|a)_T prod_k S^{n_k}_{t_k,a} h_k^{t_k}: the factor aterms evaluates (lib/samplea.c:65-67) times
// the S_S cells aterms gathers (lib/samplea.c:68-80).  The draw is the smallest tau whose cumulative weight exceeds
// u W, the weights scaled by exp(-max log w) and W their sum.  With M < n the draw is from the conditional
// truncated at M (exact when M >= max n).  This is test/check.c's SampleCT without its early stop.
//
// A pair visit is three passes over tau in chunks of one workgroup (tau = base + thread + 1):
//   1. log(b + (T_+tau-1) a) turned into a prefix sum by a workgroup scan carried across chunks; with the S row
//      (contiguous: coalesced loads) and (tau-1) log h that is log w; its maximum.
//   2. w = exp(log w - max), again a scan carried across chunks: the cumulative weights C(tau); W = C(tau_max).
//   3. the first tau with C(tau) > u W (each thread its first, then the workgroup's minimum).
// Rows up to STB_TC_CAP values keep log w, then C, in LDS between the passes; longer rows recompute passes 1 and 2
// chunk by chunk (the same operations in the same order: the same bits) and stop at the chunk holding the draw.
// T_i is a register of every thread; t and T are written back in place.  No workgroup waits for another.
//
// Uniforms are counter-based (libstb_amd/synth.py's splitmix64): sweep s, flat pair index g:
//     key_s = mix(seed + (s+1) gamma),  u = top 53 bits of mix(key_s + (g+1) gamma) / 2^53
// so the draws depend on (seed, sweep, g) alone, not on launch geometry or timing.
//
// The stb_tcounts_* object that drives this sweep, the windowed one and the steps on its counts is tcounts_obj.hip's.

#include "stb_common.h"
#include "tcounts.h"

#define STB_TC_CAP 4096      // tau values a workgroup keeps in LDS (32 KB); longer rows recompute
#define STB_TC_MAXWAVES 16

// ---- workgroup collectives (nw = waves of the workgroup; every thread gets the same bits); the wave's part of each is
// wave.h's ----

struct tc_shared {
  double wsum[STB_TC_MAXWAVES];
  unsigned wmin[STB_TC_MAXWAVES];
};

// inclusive prefix sum over the workgroup in thread order; *total = the sum over all threads
__device__ __forceinline__ double tc_scan(double v, int nw, tc_shared &sh, double *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = stb_wave_scan(v, (unsigned)lane);
  if (nw == 1) {
    *total = __shfl(v, 63, 64);
    return v;
  }
  if (lane == 63) sh.wsum[wave] = v;
  __syncthreads();
  double pre = 0.0, tot = 0.0;
  for (int w = 0; w < nw; w++) {
    const double x = sh.wsum[w];
    if (w < wave) pre += x;
    tot += x;
  }
  __syncthreads();
  *total = tot;
  return pre + v;
}

__device__ __forceinline__ double tc_max(double v, int nw, tc_shared &sh) {
  v = stb_wave_all_max(v);
  if (nw == 1) return v;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh.wsum[wave] = v;
  __syncthreads();
  double m = sh.wsum[0];
  for (int w = 1; w < nw; w++) m = fmax(m, sh.wsum[w]);
  __syncthreads();
  return m;
}

__device__ __forceinline__ unsigned tc_min(unsigned v, int nw, tc_shared &sh) {
  v = stb_wave_all_min(v);
  if (nw == 1) return v;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh.wmin[wave] = v;
  __syncthreads();
  unsigned m = sh.wmin[0];
  for (int w = 1; w < nw; w++) m = min(m, sh.wmin[w]);
  __syncthreads();
  return m;
}

// one chunk of pass 1: log w at tau (-inf outside 1..tmax); *carry advances by the chunk's sum of log terms
__device__ __forceinline__ double tc_logw(const double *row, const double *S1, unsigned n, unsigned tau,
                                          unsigned tmax, double lb_base, double a, double b, double logh, int nw,
                                          tc_shared &sh, double *carry) {
  const bool ok = tau <= tmax;
  const double term = (ok && tau >= 2) ? log(b + (lb_base + (double)(tau - 1)) * a) : 0.0;
  double tot;
  const double pre = tc_scan(term, nw, sh, &tot) + *carry;
  *carry += tot;
  return ok ? tc_S(row, S1, n, tau) + (double)(tau - 1) * logh + pre : -HUGE_VAL;
}

__global__ __launch_bounds__(1024) void k_tcounts(const double *table, const double *S1, unsigned N, unsigned M, double a,
                                                  const double *bpar, int I, const uint64_t *koff, const uint32_t *nv,
                                                  uint16_t *tv, uint32_t *Tv, const double *hv, uint64_t seed,
                                                  uint64_t sweep0, int nsweeps, unsigned cap) {
  extern __shared__ double lds[];  // [cap]: log w, then C, of the pair being visited
  __shared__ tc_shared sh;
  const int i = blockIdx.x;
  if (i >= I) return;
  const int nt = blockDim.x, nw = nt >> 6, tid = threadIdx.x;
  const uint64_t k0 = koff[i], k1 = koff[i + 1];
  const double b = bpar[i];
  uint32_t T = Tv[i];
  for (int s = 0; s < nsweeps; s++) {
    const uint64_t key = stb_mix64(seed + (sweep0 + (uint64_t)s + 1) * STB_GAMMA);
    for (uint64_t g = k0; g < k1; g++) {
      const unsigned n = nv[g], told = tv[g];
      if (nw > 1) __syncthreads();  // (every thread has read t[g] before thread 0 rewrites it)
      if (n == 0 || n > N) continue;  // (n > N: outside the table -- the pair keeps its t)
      unsigned tnew = 1;
      const unsigned tmax = n < M ? n : M;
      if (tmax >= 2) {
        const double logh = hv ? log(hv[g]) : 0.0;
        const double lb_base = (double)(T - told);  // T_: the log terms are log(b + (T_ + tau - 1) a), tau >= 2
        const double *row = table + stb_row_offset(n, M);
        const bool cached = tmax <= cap;
        // pass 1: log w and its maximum
        double carry = 0.0, mx = -HUGE_VAL;
        for (unsigned base = 0; base < tmax; base += nt) {
          const unsigned tau = base + tid + 1;
          const double lw = tc_logw(row, S1, n, tau, tmax, lb_base, a, b, logh, nw, sh, &carry);
          mx = fmax(mx, lw);
          if (cached && tau <= tmax) lds[tau - 1] = lw;
        }
        mx = tc_max(mx, nw, sh);
        // pass 2: the cumulative weights; W = C(tmax)
        double c1 = 0.0, c2 = 0.0;
        for (unsigned base = 0; base < tmax; base += nt) {
          const unsigned tau = base + tid + 1;
          double lw;
          if (cached) lw = tau <= tmax ? lds[tau - 1] : -HUGE_VAL;
          else lw = tc_logw(row, S1, n, tau, tmax, lb_base, a, b, logh, nw, sh, &c1);
          double tot;
          const double c = tc_scan(exp(lw - mx), nw, sh, &tot) + c2;
          c2 += tot;
          if (cached && tau <= tmax) lds[tau - 1] = c;
        }
        const double u = stb_unit(key, g + 1);
        const double target = u * c2;
        // pass 3: the first tau with C(tau) > u W
        unsigned first = 0xffffffffu;
        if (cached) {
          for (unsigned tau = tid + 1; tau <= tmax; tau += nt)
            if (lds[tau - 1] > target) {
              first = tau;
              break;
            }
          first = tc_min(first, nw, sh);
        } else {
          c1 = 0.0;
          c2 = 0.0;
          for (unsigned base = 0; base < tmax && first == 0xffffffffu; base += nt) {
            const unsigned tau = base + tid + 1;
            const double lw = tc_logw(row, S1, n, tau, tmax, lb_base, a, b, logh, nw, sh, &c1);
            double tot;
            const double c = tc_scan(exp(lw - mx), nw, sh, &tot) + c2;
            c2 += tot;
            first = tc_min((tau <= tmax && c > target) ? tau : 0xffffffffu, nw, sh);
          }
        }
        tnew = first <= tmax ? first : tmax;  // (C(tmax) = W > u W: always found)
      }
      T = T - told + tnew;
      if (tid == 0 && tnew != told) tv[g] = (uint16_t)tnew;
      if (nw > 1) __syncthreads();  // (the store is seen by the next sweep's reads; the LDS row is free again)
    }
  }
  if (tid == 0) Tv[i] = T;
}

static int tc_threads(void) {
  const int v = stb_env_int("STB_TCOUNTS_THREADS", 256);
  return (v == 64 || v == 128 || v == 256 || v == 512 || v == 1024) ? v : 256;
}

int stb_tc_launch(const stb_table_view &S, const stb_rest_view &r, const stb_cnts_tT &c, const stb_draw_key &k, int nsweeps,
                  unsigned tau_max, hipStream_t st) {
  if (r.I <= 0 || nsweeps <= 0) return 0;
  const int nt = tc_threads();
  unsigned cap = tau_max < STB_TC_CAP ? tau_max : STB_TC_CAP;
  if (cap < 1) cap = 1;
  STB_LAUNCH_SHM(k_tcounts, dim3((unsigned)r.I), dim3(nt), sizeof(double) * cap, st, S.tab, S.S1, S.N, S.M, r.a, r.bpar, r.I,
                 r.koff, c.n, c.t, c.T, r.h, k.seed, k.sweep, nsweeps, cap);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int stb_sample_tcounts(const double *d_table, const double *d_S1, unsigned N, unsigned M, double a,
                                  const double *d_bpar, int I, const uint64_t *d_koff, const uint32_t *d_n, uint16_t *d_t,
                                  uint32_t *d_T, const double *d_h, uint64_t seed, uint64_t sweep, void *stream) {
  STB_ENTRY;
  if (!(a >= 0.0 && a < 1.0)) return stb_fail("stb_sample_tcounts: discount a=%g outside [0, 1)", a);
  if (N < 1 || M < 1) return stb_fail("stb_sample_tcounts: table bounds N=%u M=%u", N, M);
  if (I < 0) return stb_fail("stb_sample_tcounts: I=%d", I);
  const stb_table_view S = {d_table, N, M, d_S1};
  const stb_rest_view r = {a, d_bpar, I, d_koff, d_h};
  const stb_cnts_tT c = {d_n, d_t, d_T};
  return stb_tc_launch(S, r, c, {seed, sweep}, 1, N < M ? N : M, (hipStream_t)stream);
}
