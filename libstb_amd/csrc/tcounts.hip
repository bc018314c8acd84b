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

#include <vector>

#include "stb_common.h"
#include "groups.h"
#include "tcounts.h"
#include "hyperq.h"
#include "hyperb.h"
#include "hyperj.h"
#include "logjoint.h"

#define STB_TC_CAP 4096      // tau values a workgroup keeps in LDS (32 KB); longer rows recompute
#define STB_TC_MAXWAVES 16

// ---- workgroup collectives (nw = waves of the workgroup; every thread gets the same bits) ----

struct tc_shared {
  double wsum[STB_TC_MAXWAVES];
  unsigned wmin[STB_TC_MAXWAVES];
};

// inclusive prefix sum over the workgroup in thread order; *total = the sum over all threads
__device__ __forceinline__ double tc_scan(double v, int nw, tc_shared &sh, double *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
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
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = fmax(v, __shfl_xor(v, o, 64));
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
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = min(v, (unsigned)__shfl_xor((int)v, o, 64));
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
        const double u = tc_unit(key, g + 1);
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

static int tc_launch(const double *d_table, const double *d_S1, unsigned N, unsigned M, double a, const double *d_bpar, int I,
                     const uint64_t *d_koff, const uint32_t *d_n, uint16_t *d_t, uint32_t *d_T, const double *d_h,
                     uint64_t seed, uint64_t sweep, int nsweeps, unsigned tau_max, hipStream_t st) {
  if (I <= 0 || nsweeps <= 0) return 0;
  const int nt = tc_threads();
  unsigned cap = tau_max < STB_TC_CAP ? tau_max : STB_TC_CAP;
  if (cap < 1) cap = 1;
  STB_LAUNCH_SHM(k_tcounts, dim3((unsigned)I), dim3(nt), sizeof(double) * cap, st, d_table, d_S1, N, M, a, d_bpar, I, d_koff,
                 d_n, d_t, d_T, d_h, seed, sweep, nsweeps, cap);
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
  return tc_launch(d_table, d_S1, N, M, a, d_bpar, I, d_koff, d_n, d_t, d_T, d_h, seed, sweep, 1, N < M ? N : M,
                   (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// the object: pairs, totals, weights, its own table for the current discount, its own stream

struct stb_tcounts {
  int dev;
  int I;
  uint64_t G;
  unsigned N, M;        // table bounds: N = the largest n (at least 3), M = the column bound the draws are truncated at
  unsigned maxn;
  uint64_t sumn;        // sum of n over the pairs (the partition's histogram bins are uint32)
  bool need_table;      // some pair can have 2 or more tables (min(max n, M) >= 2); otherwise every draw is t = 1
  uint64_t *d_koff;
  uint32_t *d_n, *d_T;
  uint32_t *d_N;        // customers per restaurant (the sum of n over its pairs), built once at create: sampleb's N
  uint16_t *d_t;
  double *d_h;          // null: every h is 1
  double *d_bpar;
  double *h_bpar[2];    // pinned staging of bpar, used in turn: a sweep does not wait for the one before it
  hipEvent_t ev_bpar[2];  // the copy out of h_bpar[k] is through
  int slot;
  std::vector<double> last_bpar;  // what d_bpar holds (empty: nothing yet, or a device step wrote it)
  stb_hb_obj hb;        // the per-group concentration step (hyperb.hip): ranges, L, Y, and whether d_bpar holds anything
  double *d_table, *d_S1;
  uint64_t tstride;
  void *d_ws;
  size_t ws_bytes;
  double a_filled;      // the discount the table holds (NaN: none yet)
  hipStream_t st;
};

static void tc_release(stb_tcounts_t *s) {
  stb_hb_obj_release(&s->hb);
  void *dev[] = {s->d_koff, s->d_n, s->d_T, s->d_N, s->d_t, s->d_h, s->d_bpar, s->d_table, s->d_S1, s->d_ws};
  for (void *p : dev)
    if (p) (void)hipFree(p);
  for (int k = 0; k < 2; k++) {
    if (s->h_bpar[k]) (void)hipHostFree(s->h_bpar[k]);
    if (s->ev_bpar[k]) (void)hipEventDestroy(s->ev_bpar[k]);
  }
  if (s->st) (void)hipStreamDestroy(s->st);
  delete s;
}

static int tc_check_h(const double *h, uint64_t G, const char *who) {
  for (uint64_t g = 0; g < G; g++)
    if (!(h[g] > 0.0) || !std::isfinite(h[g])) return stb_fail("%s: h[%llu]=%g (must be > 0 and finite)", who, (unsigned long long)g, h[g]);
  return 0;
}

static stb_tcounts_t *tc_create_here(int I, const int *K, const uint32_t *nflat, const uint16_t *tflat, const double *hflat,
                                     unsigned M) {
  if (stb_device_count() < 1) {
    stb_fail("stb_tcounts_create: no HIP device (libstb_amd has no CPU path)");
    return nullptr;
  }
  if (I < 1 || !K || !nflat || !tflat) {
    stb_fail("stb_tcounts_create: I=%d and K, n, t are required", I);
    return nullptr;
  }
  std::vector<uint64_t> koff((size_t)I + 1, 0);
  for (int i = 0; i < I; i++) {
    if (K[i] < 0) {
      stb_fail("stb_tcounts_create: K[%d]=%d", i, K[i]);
      return nullptr;
    }
    koff[i + 1] = koff[i] + (uint64_t)K[i];
  }
  const uint64_t G = koff[I];
  unsigned maxn = 0;
  for (uint64_t g = 0; g < G; g++) maxn = nflat[g] > maxn ? nflat[g] : maxn;
  if (M == 0 && maxn > 65535u) {
    stb_fail("stb_tcounts_create: the largest n is %u; t is a uint16, so pass M <= 65535 (the draws are then from the "
             "conditional truncated at M)", maxn);
    return nullptr;
  }
  if (M == 0) M = maxn > 0 ? maxn : 1;
  if (M > 65535u) {
    stb_fail("stb_tcounts_create: M=%u (t is a uint16: at most 65535)", M);
    return nullptr;
  }
  std::vector<uint32_t> T(I, 0);
  for (int i = 0; i < I; i++)
    for (uint64_t g = koff[i]; g < koff[i + 1]; g++) {
      const unsigned n = nflat[g], t = tflat[g], tm = n < M ? n : M;
      if (n == 0 ? t != 0 : (t < 1 || t > tm)) {
        stb_fail("stb_tcounts_create: pair %llu has n=%u t=%u (t = 0 exactly when n = 0, else 1 <= t <= min(n, M=%u))",
                 (unsigned long long)g, n, t, M);
        return nullptr;
      }
      T[i] += t;
    }
  if (hflat && tc_check_h(hflat, G, "stb_tcounts_create")) return nullptr;
  stb_tcounts_t *s = new stb_tcounts_t();
  s->I = I;
  s->G = G;
  s->maxn = maxn;
  for (uint64_t g = 0; g < G; g++) s->sumn += nflat[g];
  for (int i = 0; i < I; i++) {  // (N_i is a uint32, as sampleb's N[])
    uint64_t ni = 0;
    for (uint64_t g = koff[i]; g < koff[i + 1]; g++) ni += nflat[g];
    if (ni >= (1ull << 32)) {
      stb_fail("stb_tcounts_create: restaurant %d holds %llu customers (fewer than 2^32)", i, (unsigned long long)ni);
      delete s;
      return nullptr;
    }
  }
  s->N = maxn < 3 ? 3 : maxn;
  s->M = M;
  s->a_filled = NAN;
  s->need_table = (maxn < M ? maxn : M) >= 2;
  const size_t Gs = G ? G : 1;
  int rc = 0;
  if (hipGetDevice(&s->dev) != hipSuccess || hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc((void **)&s->d_koff, sizeof(uint64_t) * (I + 1)) != hipSuccess ||
      hipMalloc((void **)&s->d_n, sizeof(uint32_t) * Gs) != hipSuccess || hipMalloc((void **)&s->d_t, sizeof(uint16_t) * Gs) != hipSuccess ||
      hipMalloc((void **)&s->d_T, sizeof(uint32_t) * I) != hipSuccess || hipMalloc((void **)&s->d_bpar, sizeof(double) * I) != hipSuccess ||
      hipMalloc((void **)&s->d_N, sizeof(uint32_t) * I) != hipSuccess ||
      hipHostMalloc((void **)&s->h_bpar[0], sizeof(double) * I) != hipSuccess ||
      hipHostMalloc((void **)&s->h_bpar[1], sizeof(double) * I) != hipSuccess ||
      hipEventCreateWithFlags(&s->ev_bpar[0], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&s->ev_bpar[1], hipEventDisableTiming) != hipSuccess ||
      (hflat && hipMalloc((void **)&s->d_h, sizeof(double) * Gs) != hipSuccess))
    rc = stb_fail("stb_tcounts_create: %s", hipGetErrorString(hipGetLastError()));
  // (no table where no draw reads one: every pair has n <= 1, or M = 1)
  s->tstride = s->need_table ? (stb_table_elems(s->N, s->M) + 31) & ~31ull : 0;
  s->ws_bytes = s->need_table ? stb_fill_workspace_bytes(s->N, s->M, 1) : 0;
  if (!rc && s->need_table && (hipMalloc((void **)&s->d_table, sizeof(double) * s->tstride) != hipSuccess ||
              hipMalloc((void **)&s->d_S1, sizeof(double) * s->N) != hipSuccess || hipMalloc(&s->d_ws, s->ws_bytes ? s->ws_bytes : 1) != hipSuccess))
    rc = stb_fail("stb_tcounts_create: out of device memory for a %u x %u table", s->N, s->M);
  if (!rc && (hipMemcpy(s->d_koff, koff.data(), sizeof(uint64_t) * (I + 1), hipMemcpyHostToDevice) != hipSuccess ||
              (G && hipMemcpy(s->d_n, nflat, sizeof(uint32_t) * G, hipMemcpyHostToDevice) != hipSuccess) ||
              (G && hipMemcpy(s->d_t, tflat, sizeof(uint16_t) * G, hipMemcpyHostToDevice) != hipSuccess) ||
              hipMemcpy(s->d_T, T.data(), sizeof(uint32_t) * I, hipMemcpyHostToDevice) != hipSuccess ||
              (hflat && G && hipMemcpy(s->d_h, hflat, sizeof(double) * G, hipMemcpyHostToDevice) != hipSuccess)))
    rc = stb_fail("stb_tcounts_create: %s", hipGetErrorString(hipGetLastError()));
  // customers per restaurant: a segmented sum of n over the pair offsets, once (the b step reads it: stb_tcounts_sampleb)
  if (!rc) rc = stb_hq_segsum(s->d_koff, s->d_n, I, s->d_N, s->st);
  if (!rc && hipStreamSynchronize(s->st) != hipSuccess) rc = stb_fail("stb_tcounts_create: %s", hipGetErrorString(hipGetLastError()));
  if (rc) {
    tc_release(s);
    return nullptr;
  }
  return s;
}

// The object lives on the device stb_get_device() names, like a group set; every later call switches to it.
extern "C" stb_tcounts_t *stb_tcounts_create(int I, const int *K, const uint32_t *nflat, const uint16_t *tflat,
                                             const double *hflat, unsigned M) {
  STB_ENTRY;
  const int prev = stb_device_enter(stb_get_device());
  stb_tcounts_t *s = tc_create_here(I, K, nflat, tflat, hflat, M);
  stb_device_leave(prev);
  return s;
}

extern "C" void stb_tcounts_free(stb_tcounts_t *s) {
  STB_ENTRY;
  if (!s) return;
  const int prev = stb_device_enter(s->dev);
  (void)hipStreamSynchronize(s->st);
  tc_release(s);
  stb_device_leave(prev);
}

extern "C" int stb_tcounts_set_h(stb_tcounts_t *s, const double *hflat) {
  STB_ENTRY;
  if (!s) return stb_fail("stb_tcounts_set_h: null object");
  if (hflat && tc_check_h(hflat, s->G, "stb_tcounts_set_h")) return 1;
  const int prev = stb_device_enter(s->dev);
  int rc = 0;
  if (hipStreamSynchronize(s->st) != hipSuccess) rc = stb_fail("stb_tcounts_set_h: %s", hipGetErrorString(hipGetLastError()));
  if (!rc && !hflat && s->d_h) {
    (void)hipFree(s->d_h);
    s->d_h = nullptr;
  } else if (!rc && hflat && s->G) {
    if (!s->d_h && hipMalloc((void **)&s->d_h, sizeof(double) * s->G) != hipSuccess) rc = stb_fail("stb_tcounts_set_h: out of device memory");
    if (!rc && hipMemcpy(s->d_h, hflat, sizeof(double) * s->G, hipMemcpyHostToDevice) != hipSuccess)
      rc = stb_fail("stb_tcounts_set_h: %s", hipGetErrorString(hipGetLastError()));
  }
  stb_device_leave(prev);
  return rc;
}

// what every sweep of the object checks before anything changes: a failure leaves the state as it was
static int tc_check_sweep(stb_tcounts_t *s, double a, const double *bpar, int nsweeps, const char *who) {
  if (!s) return stb_fail("%s: null object", who);
  if (!(a >= 0.0 && a < 1.0)) return stb_fail("%s: discount a=%g outside [0, 1)", who, a);
  if (!bpar) return stb_fail("%s: bpar is required", who);
  if (nsweeps < 0) return stb_fail("%s: nsweeps=%d", who, nsweeps);
  if (bpar == STB_BPAR_RESIDENT) return stb_hb_obj_resident(&s->hb, a, who);  // (what the object holds, by its lower bound)
  for (int i = 0; i < s->I; i++)
    if (!(bpar[i] > -a) || !std::isfinite(bpar[i])) return stb_fail("%s: bpar[%d]=%g (must be > -a = %g)", who, i, bpar[i], -a);
  return 0;
}

// new concentrations through the staging buffer used two calls ago (its copy is long through); unchanged ones stay
static int tc_stage_bpar(stb_tcounts_t *s, const double *bpar, const char *who) {
  int rc = 0;
  if (bpar == STB_BPAR_RESIDENT) return rc;  // (tc_check_sweep saw that the object holds some)
  const bool same_b = s->last_bpar.size() == (size_t)s->I && memcmp(s->last_bpar.data(), bpar, sizeof(double) * s->I) == 0;
  if (!same_b) {
    const int k = s->slot ^= 1;
    s->last_bpar.clear();
    if (hipEventSynchronize(s->ev_bpar[k]) != hipSuccess) rc = stb_fail("%s: %s", who, hipGetErrorString(hipGetLastError()));
    if (!rc) {
      memcpy(s->h_bpar[k], bpar, sizeof(double) * s->I);
      if (hipMemcpyAsync(s->d_bpar, s->h_bpar[k], sizeof(double) * s->I, hipMemcpyHostToDevice, s->st) != hipSuccess ||
          hipEventRecord(s->ev_bpar[k], s->st) != hipSuccess)
        rc = stb_fail("%s: %s", who, hipGetErrorString(hipGetLastError()));
    }
    if (!rc) s->last_bpar.assign(bpar, bpar + s->I);
    if (!rc) stb_hb_obj_uploaded(&s->hb, bpar, s->I);
  }
  return rc;
}

// what every sweep of the object needs queued before its kernel (on the object's device): the table for `a` and the
// concentrations bpar on the device
static int tc_stage(stb_tcounts_t *s, double a, const double *bpar, const char *who) {
  int rc = 0;
  if (s->need_table && !(a == s->a_filled)) {  // (refilled only when the discount changes; the refill is checked: a wait)
    s->a_filled = NAN;
    rc = stb_fill_S(&a, 1, s->N, s->M, s->d_table, s->tstride, s->d_S1, s->N, s->d_ws, s->ws_bytes, stb_default_variant(), s->st);
    if (!rc) rc = stb_fill_status();
    if (!rc) s->a_filled = a;
  }
  if (!rc) rc = tc_stage_bpar(s, bpar, who);
  return rc;
}

extern "C" int stb_tcounts_set_bpar(stb_tcounts_t *s, const double *bpar) {
  STB_ENTRY;
  const char *who = "stb_tcounts_set_bpar";
  if (!s) return stb_fail("%s: null object", who);
  if (!bpar || bpar == STB_BPAR_RESIDENT) return stb_fail("%s: bpar (host, I values) is required", who);
  for (int i = 0; i < s->I; i++)
    if (!std::isfinite(bpar[i])) return stb_fail("%s: bpar[%d]=%g (must be finite)", who, i, bpar[i]);
  const int prev = stb_device_enter(s->dev);
  const int rc = tc_stage_bpar(s, bpar, who);
  stb_device_leave(prev);
  return rc;
}

extern "C" int stb_tcounts_get_bpar(stb_tcounts_t *s, double *bpar_out) {
  STB_ENTRY;
  const char *who = "stb_tcounts_get_bpar";
  if (!s || !bpar_out) return stb_fail("%s: null %s", who, s ? "output" : "object");
  if (!s->hb.resident) return stb_fail("%s: the object holds no concentrations yet", who);
  const int prev = stb_device_enter(s->dev);
  int rc = 0;
  if (hipMemcpyAsync(bpar_out, s->d_bpar, sizeof(double) * s->I, hipMemcpyDeviceToHost, s->st) != hipSuccess ||
      hipStreamSynchronize(s->st) != hipSuccess)
    rc = stb_fail("%s: %s", who, hipGetErrorString(hipGetLastError()));
  stb_device_leave(prev);
  return rc;
}

extern "C" int stb_tcounts_set_bgroups(stb_tcounts_t *s, int G, const uint64_t *goff_host) {
  STB_ENTRY;
  if (!s) return stb_fail("stb_tcounts_set_bgroups: null object");
  const int prev = stb_device_enter(s->dev);
  const int rc = stb_hb_obj_set_groups(&s->hb, s->I, G, goff_host, s->st, "stb_tcounts_set_bgroups");
  stb_device_leave(prev);
  return rc;
}

// the per-group concentration step (hyperb.hip) on the object's T, N and concentrations, queued behind its sweeps.  The
// step writes d_bpar: the host copy that spares an upload no longer describes it
extern "C" int stb_tcounts_sampleb_groups(stb_tcounts_t *s, double a, double shape, double scale, uint64_t seed, uint64_t sweep,
                                          double *bgrp_host, stb_bgroups_info_t *info) {
  STB_ENTRY;
  if (!s) return stb_fail("stb_tcounts_sampleb_groups: null object");
  const int prev = stb_device_enter(s->dev);
  const int rc = stb_hb_obj_step(&s->hb, a, shape, scale, s->I, s->d_N, nullptr, s->d_T, s->d_bpar, seed, sweep, s->st, bgrp_host,
                                 info, "stb_tcounts_sampleb_groups");
  if (s->hb.resident) s->last_bpar.clear();
  stb_device_leave(prev);
  return rc;
}

extern "C" int stb_tcounts_sweep(stb_tcounts_t *s, double a, const double *bpar, uint64_t seed, uint64_t sweep, int nsweeps) {
  STB_ENTRY;
  if (tc_check_sweep(s, a, bpar, nsweeps, "stb_tcounts_sweep")) return 1;
  if (nsweeps == 0) return 0;
  const int prev = stb_device_enter(s->dev);
  int rc = tc_stage(s, a, bpar, "stb_tcounts_sweep");
  if (!rc)
    rc = tc_launch(s->d_table, s->d_S1, s->N, s->M, a, s->d_bpar, s->I, s->d_koff, s->d_n, s->d_t, s->d_T, s->d_h, seed, sweep,
                   nsweeps, s->maxn < s->M ? s->maxn : s->M, s->st);
  stb_device_leave(prev);
  return rc;
}

// the windowed sweep (tcwin.hip) on the same object: the same table, concentrations, stream and checks
extern "C" int stb_tcounts_sweep_window(stb_tcounts_t *s, double a, const double *bpar, unsigned W, unsigned flags,
                                        uint64_t seed, uint64_t sweep, int nsweeps) {
  STB_ENTRY;
  if (W == 0) return stb_fail("stb_tcounts_sweep_window: window W=0 (must be >= 1)");
  if (flags & ~STB_TC_REF_WINDOW_FLAG) return stb_fail("stb_tcounts_sweep_window: unknown flags 0x%x", flags);
  if (tc_check_sweep(s, a, bpar, nsweeps, "stb_tcounts_sweep_window")) return 1;
  if (nsweeps == 0) return 0;
  const int prev = stb_device_enter(s->dev);
  int rc = tc_stage(s, a, bpar, "stb_tcounts_sweep_window");
  if (!rc)
    rc = stb_tcw_launch(s->d_table, s->d_S1, s->N, s->M, a, s->d_bpar, s->I, s->d_koff, s->d_n, s->d_t, s->d_T, s->d_h, W,
                        flags, seed, sweep, nsweeps, s->st);
  stb_device_leave(prev);
  return rc;
}

extern "C" int stb_tcounts_get(stb_tcounts_t *s, uint16_t *t_out, uint32_t *T_out) {
  STB_ENTRY;
  if (!s) return stb_fail("stb_tcounts_get: null object");
  const int prev = stb_device_enter(s->dev);
  int rc = 0;
  if ((t_out && s->G && hipMemcpyAsync(t_out, s->d_t, sizeof(uint16_t) * s->G, hipMemcpyDeviceToHost, s->st) != hipSuccess) ||
      (T_out && hipMemcpyAsync(T_out, s->d_T, sizeof(uint32_t) * s->I, hipMemcpyDeviceToHost, s->st) != hipSuccess) ||
      hipStreamSynchronize(s->st) != hipSuccess)
    rc = stb_fail("stb_tcounts_get: %s", hipGetErrorString(hipGetLastError()));
  stb_device_leave(prev);
  return rc;
}

// the pairs and T to a group set of the same shape, device to device (what stb_groups_update_pairs +
// stb_groups_update_restaurants do from host arrays)
extern "C" int stb_tcounts_to_groups(stb_tcounts_t *s, stb_groups_t *g, const double *bpar) {
  STB_ENTRY;
  if (!s || !g) return stb_fail("stb_tcounts_to_groups: null object");
  if (g->I != s->I || g->G != s->G)
    return stb_fail("stb_tcounts_to_groups: the group set has I=%d, G=%llu; the counts I=%d, G=%llu", g->I,
                    (unsigned long long)g->G, s->I, (unsigned long long)s->G);
  if (g->dev != s->dev) return stb_fail("stb_tcounts_to_groups: the group set is on device %d, the counts on %d", g->dev, s->dev);
  if (g->pending == 1) return stb_fail("stb_tcounts_to_groups: an evaluation queued with stb_groups_aterms_async has not been waited for");
  if (g->putting) return stb_fail("stb_tcounts_to_groups: the group set is between stb_groups_pairs_begin and _commit");
  if (bpar == STB_BPAR_RESIDENT && !s->hb.resident)
    return stb_fail("stb_tcounts_to_groups: STB_BPAR_RESIDENT, but the object holds no concentrations yet");
  const int prev = stb_device_enter(s->dev);
  int rc = 0;
  // the bounds the new pairs can need, known without looking at them: n up to max n, t up to min(max n, M)
  unsigned N = g->have_bounds ? g->N : 0, M = g->have_bounds ? g->M : 0;
  if (N < s->maxn) N = s->maxn;
  const unsigned tcap = s->maxn < s->M ? s->maxn : s->M;
  if (M < tcap) M = tcap;
  if (N < 1) N = 1;
  if (M < 1) M = 1;
  hipEvent_t ev = nullptr;
  if (!rc && hipStreamSynchronize(g->st) != hipSuccess) rc = stb_fail("stb_tcounts_to_groups: %s", hipGetErrorString(hipGetLastError()));
  if (!rc) rc = stb_groups_set_bounds(g, N, M);  // (re-sizes what depends on the bounds when they grow)
  if (!rc && (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(ev, s->st) != hipSuccess ||
              hipStreamWaitEvent(g->st, ev, 0) != hipSuccess))
    rc = stb_fail("stb_tcounts_to_groups: %s", hipGetErrorString(hipGetLastError()));
  if (!rc && ((s->G && (hipMemcpyAsync(g->d_n, s->d_n, sizeof(uint32_t) * s->G, hipMemcpyDeviceToDevice, g->st) != hipSuccess ||
                        hipMemcpyAsync(g->d_t, s->d_t, sizeof(uint16_t) * s->G, hipMemcpyDeviceToDevice, g->st) != hipSuccess)) ||
              hipMemcpyAsync(g->d_T, s->d_T, sizeof(uint32_t) * s->I, hipMemcpyDeviceToDevice, g->st) != hipSuccess))
    rc = stb_fail("stb_tcounts_to_groups: %s", hipGetErrorString(hipGetLastError()));
  if (!rc && bpar == STB_BPAR_RESIDENT) {  // (g->st waits for the object's stream above)
    for (int i = 0; i < g->I; i++) g->h_bpar[i] = NAN;  // (the host's copy no longer says what the set holds)
    if (hipMemcpyAsync(g->d_bpar, s->d_bpar, sizeof(double) * g->I, hipMemcpyDeviceToDevice, g->st) != hipSuccess)
      rc = stb_fail("stb_tcounts_to_groups: %s", hipGetErrorString(hipGetLastError()));
  } else if (!rc && bpar) {
    memcpy(g->h_bpar, bpar, sizeof(double) * (size_t)g->I);  // (g->st was idle above: its staging area is free)
    if (hipMemcpyAsync(g->d_bpar, g->h_bpar, sizeof(double) * g->I, hipMemcpyHostToDevice, g->st) != hipSuccess)
      rc = stb_fail("stb_tcounts_to_groups: %s", hipGetErrorString(hipGetLastError()));
  }
  // the sweep's later work must not overwrite the pairs before the set has its copy
  if (!rc && (hipEventRecord(ev, g->st) != hipSuccess || hipStreamWaitEvent(s->st, ev, 0) != hipSuccess))
    rc = stb_fail("stb_tcounts_to_groups: %s", hipGetErrorString(hipGetLastError()));
  if (ev) (void)hipEventDestroy(ev);
  if (!rc) {  // as stb_groups_pairs_commit: new pairs, cell lists rebuilt and the pairs sorted again on first need
    stb_lists_drop(g, true);
    g->sorted = 0;
    g->have_pairs = 1;
    g->reused = 1;  // (as stb_groups_update_restaurants marks: a set that serves sweep after sweep)
  }
  stb_device_leave(prev);
  return rc;
}

// stage 1 of the S-free discount step (partition.hip) on the object's pairs: the table-size histogram into h, T and bpar
// to h, all on the device, queued behind the object's earlier work; h's later work waits for it
extern "C" int stb_tcounts_partition(stb_tcounts_t *s, double a, stb_hist_t *h, const double *bpar, uint64_t seed,
                                     uint64_t sweep) {
  STB_ENTRY;
  const char *who = "stb_tcounts_partition";
  if (tc_check_sweep(s, a, bpar, 0, who)) return 1;
  stb_hist_view v;
  if (!h || stb_hist_view_of(h, &v)) return stb_fail("%s: null histogram", who);
  if (v.dev != s->dev) return stb_fail("%s: the histogram is on device %d, the counts on %d", who, v.dev, s->dev);
  if (v.I != s->I) return stb_fail("%s: the histogram has I=%d, the counts I=%d", who, v.I, s->I);
  if (v.S <= s->maxn) return stb_fail("%s: histogram length S=%u (must exceed the largest n, %u)", who, v.S, s->maxn);
  if (s->sumn >= (1ull << 32))
    return stb_fail("%s: the pairs hold %llu customers (the bins are uint32: fewer than 2^32)", who,
                    (unsigned long long)s->sumn);
  if (stb_pt_check(a, s->N, s->M, s->G, v.S, 0u, who)) return 1;
  const int prev = stb_device_enter(s->dev);
  int rc = tc_stage(s, a, bpar, who);
  hipEvent_t ev = nullptr;
  if (!rc && (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(ev, v.st) != hipSuccess ||
              hipStreamWaitEvent(s->st, ev, 0) != hipSuccess))
    rc = stb_fail("%s: %s", who, hipGetErrorString(hipGetLastError()));
  if (!rc)
    rc = stb_pt_launch(s->d_table, s->d_S1, s->N, s->M, a, s->G, s->d_n, s->d_t, v.d_cnt, v.S, nullptr, nullptr, 0u, seed,
                       sweep, s->st);
  if (!rc && (hipMemcpyAsync(v.d_T, s->d_T, sizeof(uint32_t) * s->I, hipMemcpyDeviceToDevice, s->st) != hipSuccess ||
              hipMemcpyAsync(v.d_bpar, s->d_bpar, sizeof(double) * s->I, hipMemcpyDeviceToDevice, s->st) != hipSuccess ||
              hipEventRecord(ev, s->st) != hipSuccess || hipStreamWaitEvent(v.st, ev, 0) != hipSuccess))
    rc = stb_fail("%s: %s", who, hipGetErrorString(hipGetLastError()));
  if (ev) (void)hipEventDestroy(ev);
  stb_device_leave(prev);
  return rc;
}

// the concentration step on the object's counts (hyperq.hip, sampleb.c): Q from N on the device, T read in place, queued
// behind the object's sweeps; the call waits for Q and for the sampler's evaluations only.  t and T are not written.
extern "C" double stb_tcounts_sampleb(stb_tcounts_t *s, double b_in, double shape, double scale, double a, void *rng, int loops,
                                      int verbose, uint64_t seed, uint64_t sweep) {
  // (no rand() guard across the call: ARMS draws from the caller's rand() stream, as in sampleb)
  if (!s) {
    stb_fail("stb_tcounts_sampleb: null object");
    return NAN;
  }
  const int prev = stb_device_enter(s->dev);
  const double b = stb_sampleb_device_ex(b_in, s->I, shape, scale, s->d_N, nullptr, s->d_T, a, rng, loops, verbose, seed, sweep,
                                         s->st, "stb_tcounts_sampleb");
  stb_device_leave(prev);
  return b;
}

// the joint step for a and b on the object's counts (hyperj.hip): the pairs and T to the set, device to device, then the
// step with the object's N, queued behind its sweeps.  Nothing per restaurant crosses to the host; t and T are not written.
extern "C" int stb_tcounts_samplejoint(stb_tcounts_t *s, stb_groups_t *g, const stb_joint_opts_t *opts, double a_in, double b_in,
                                   double *a_out, double *b_out, stb_joint_info_t *info) {
  if (!s || !g) return stb_fail("stb_tcounts_samplejoint: null object");
  if (stb_tcounts_to_groups(s, g, nullptr)) return 1;
  return stb_hj_samplejoint(g, s->d_N, nullptr, opts, a_in, b_in, a_out, b_out, info, "stb_tcounts_samplejoint");
}

// the log joint of the object's state (logjoint.hip) from its own S table, queued behind its sweeps; t and T are not
// written.  Objects without a table read none: S^n_1 (M = 1) is evaluated in place, as the fill would.
extern "C" int stb_tcounts_logjoint(stb_tcounts_t *s, double a, const double *bpar, unsigned flags, double *total,
                                    double *Li_host, stb_logjoint_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_tcounts_logjoint";
  if (!s) return stb_fail("%s: null object", who);
  if (stb_lj_check(a, flags, s->I, who)) return 1;
  if (!total) return stb_fail("%s: total is required", who);
  if (tc_check_sweep(s, a, bpar, 0, who)) return 1;
  const int prev = stb_device_enter(s->dev);
  int rc = tc_stage(s, a, bpar, who);
  double *d_Li = nullptr;
  if (!rc && Li_host && stb_pool_malloc((void **)&d_Li, sizeof(double) * (size_t)s->I) != hipSuccess)
    rc = stb_fail("%s: out of device memory for %d values", who, s->I);
  if (!rc)
    rc = stb_lj_run(s->d_table, s->d_S1, s->N, s->M, a, s->d_bpar, s->I, s->d_koff, s->d_n, s->d_t, s->d_T, s->d_h, flags, d_Li,
                    Li_host, total, info, s->st, who);
  if (d_Li) {
    if (rc) (void)hipStreamSynchronize(s->st);  // (the cache may hand the buffer on at once)
    stb_pool_free(d_Li);
  }
  stb_device_leave(prev);
  return rc;
}
