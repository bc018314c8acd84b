// seat_ais.hip -- annealed importance sampling for unseen documents: a ladder of temperatures between the prior seating
// and the posterior, climbed by every particle on a private copy of its restaurant (include/stb_hip.h, "annealed
// importance sampling"; the law is DESIGN.md section 6).  The seating is k_seat's and the moves are k_tdish's, both as they
// stand, on a replicated problem: replica j = i R + r is a restaurant of its own.  What this file adds is the ladder.
//
//   k_ais_expand   the replicated problem: offsets, b, h and classes of every replica, empty pairs, the skip flags
//   k_ais_temper   lik^beta, a cell a thread: the matrix the sweeps of one temperature read
//   k_ais_weight   D_j = sum_c log L[cls_c][z_c] of replica j's present seating and lw_j += dbeta * D_j; a wave a replica
//
// Nobody waits for anybody: the kernels are queued one after another on the caller's stream, and the stream orders them.
// The bits of lw depend on the replica's own customers and nothing else -- a lane takes customers q = lane, lane + 64, ..
// of its replica in that order, and the lanes are added in lane order -- so neither the waves of a workgroup
// (STB_AIS_WAVES = 1, 2, 4 or 8) nor the grid nor who shares the launch can move them.

#include <climits>
#include <vector>

#include "stb_common.h"
#include "seat.h"
#include "seat_ais.h"
#include "tindic.h"

#pragma clang fp contract(off)

#define AIS_MAXTHREADS 512
#define AIS_MAXGRID 4096u  // workgroups of k_ais_expand and k_ais_weight at most: the waves stride over the replicas

struct ais_args {
  // the caller's problem
  uint64_t I, G, C;
  unsigned R, rows, stride, N, cap;
  const uint64_t *koff, *coff;
  const double *bpar, *h, *lik;
  const uint32_t *cls;
  // the replicated one
  uint64_t *koff2, *coff2;
  double *bpar2, *h2, *lw;
  uint32_t *n2, *cust2, *cls2;
  uint16_t *t2;
  unsigned char *skip;            // [I] 1: the restaurant is left out
  unsigned long long *info;       // the caller's three words (skipped, dead, stuck), or null
  const unsigned long long *inner;  // k_seat's three words and k_tdish's two behind them
};

__global__ __launch_bounds__(AIS_MAXTHREADS) void k_ais_expand(ais_args A) {
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const uint64_t items = A.I * (uint64_t)A.R;
  const bool agree = A.koff[A.I] == A.G && A.coff[A.I] == A.C;
  unsigned long long n_skip = 0;  // wave-uniform
  for (uint64_t w = (uint64_t)blockIdx.x * nw + wave; w < items; w += (uint64_t)gridDim.x * nw) {
    const uint64_t i = w / A.R;
    const unsigned r = (unsigned)(w % A.R);
    if (!agree) {  // the caller's G or C is not the arrays': replicas without pairs or customers, every restaurant left out
      if (lane == 0) {
        A.koff2[w] = 0;
        A.coff2[w] = 0;
        A.bpar2[w] = 1.0;
        if (r == 0) A.skip[i] = 1;
        if (w == items - 1) A.koff2[items] = 0, A.coff2[items] = 0;
      }
      if (r == 0) n_skip++;
      continue;
    }
    const uint64_t k0 = A.koff[i], K = A.koff[i + 1] - k0, c0 = A.coff[i], Nc = A.coff[i + 1] - c0;
    const bool skipped = K > A.cap || K > A.stride || (K == 0 && Nc > 0) || Nc > A.N;
    const uint64_t kb = k0 * A.R + r * K, cb = c0 * A.R + r * Nc;
    if (lane == 0) {
      A.koff2[w] = kb;
      A.coff2[w] = cb;
      A.bpar2[w] = A.bpar[i];
      if (r == 0) A.skip[i] = skipped ? 1 : 0;
      if (w == items - 1) A.koff2[items] = kb + K, A.coff2[items] = cb + Nc;
    }
    if (r == 0 && skipped) n_skip++;
    if (K <= A.cap)  // (a K past the cap may be an offset array that runs backwards: nothing of it is addressed)
      for (uint64_t k = lane; k < K; k += 64) {
        A.n2[kb + k] = 0;
        A.t2[kb + k] = 0;
        if (A.h) A.h2[kb + k] = A.h[k0 + k];
      }
    if (!skipped)
      for (uint64_t q = lane; q < Nc; q += 64) A.cls2[cb + q] = A.cls[c0 + q];
  }
  if (lane == 0 && n_skip && A.info) __hip_atomic_fetch_add(&A.info[0], n_skip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_ais_temper(const double *lik, uint64_t cells, double beta, double *out) {
#pragma clang fp contract(off)
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= cells) return;
  const double L = lik[e];
  double v = 0.0;
  if (L != 0.0) {
    const double x = log(L);
    const double y = beta * x;
    v = exp(y);
  }
  out[e] = v;
}

// lw arrives holding the prior seating's own log weight (k_seat's: 0 for what it skipped).  first: a restaurant left out
// gets its lw = 0 here, whatever the seating made of its replicas; last: the ladder's top -- the dead particles are counted
// and the stuck visits of the seating and the sweeps handed on
__global__ __launch_bounds__(AIS_MAXTHREADS) void k_ais_weight(ais_args A, double dbeta, int first, int last) {
#pragma clang fp contract(off)
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const uint64_t items = A.I * (uint64_t)A.R;
  unsigned long long n_dead = 0;  // lane 0's
  for (uint64_t w = (uint64_t)blockIdx.x * nw + wave; w < items; w += (uint64_t)gridDim.x * nw) {
    if (A.skip[w / A.R]) {
      if (first && lane == 0) A.lw[w] = 0.0;
      continue;
    }
    const uint64_t c0 = A.coff2[w], c1 = A.coff2[w + 1];
    dd_t acc{0.0, 0.0};
    for (uint64_t c = c0 + lane; c < c1; c += 64) {
      const unsigned cl = A.cls2[c], k = A.cust2[c];
      const double L = cl < A.rows && k < A.stride ? A.lik[(uint64_t)cl * A.stride + k] : 0.0;
      dd_add(acc, L > 0.0 ? log(L) : -HUGE_VAL);
    }
    const unsigned nl = c1 - c0 < 64 ? (unsigned)(c1 - c0) : 64u;  // (a lane without customers holds 0: adding it changes no bit)
    dd_t tot{0.0, 0.0};
    for (unsigned l = 0; l < nl; l++) {
      dd_t o;
      o.hi = stb_wave_rld(acc.hi, l);
      o.lo = stb_wave_rld(acc.lo, l);
      dd_merge(tot, o);
    }
    const double D = tot.hi + tot.lo;
    if (lane == 0) {
      const double step = dbeta * D;
      const double v = A.lw[w] + step;
      A.lw[w] = v;
      if (last && v == -HUGE_VAL) n_dead++;
    }
  }
  if (lane == 0 && A.info) {
    if (n_dead) __hip_atomic_fetch_add(&A.info[1], n_dead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (last && blockIdx.x == 0 && wave == 0) {
      const unsigned long long stuck = A.inner[2] + A.inner[4];
      if (stuck) __hip_atomic_fetch_add(&A.info[2], stuck, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// the workspace: the replicated problem, the tempered matrix, the inner kernels' counters

namespace {

struct ais_plan {
  size_t koff2, coff2, bpar2, h2, tlik, n2, T2, cust2, cls2, t2, skip, inner, bytes;
};

ais_plan ais_layout(uint64_t I, uint64_t G, uint64_t C, unsigned R, unsigned rows, unsigned stride) {
  const size_t I2 = (size_t)I * R, G2 = (size_t)G * R, C2 = (size_t)C * R;
  ais_plan p;
  size_t o = 0;
  auto seg = [&o](size_t bytes) {
    const size_t at = o;
    o = stb_align_up(o + (bytes ? bytes : 1), 256);
    return at;
  };
  p.koff2 = seg(sizeof(uint64_t) * (I2 + 1));
  p.coff2 = seg(sizeof(uint64_t) * (I2 + 1));
  p.bpar2 = seg(sizeof(double) * I2);
  p.h2 = seg(sizeof(double) * G2);
  p.tlik = seg(sizeof(double) * (size_t)rows * stride);
  p.n2 = seg(sizeof(uint32_t) * G2);
  p.T2 = seg(sizeof(uint32_t) * I2);
  p.cust2 = seg(sizeof(uint32_t) * C2);
  p.cls2 = seg(sizeof(uint32_t) * C2);
  p.t2 = seg(sizeof(uint16_t) * G2);
  p.skip = seg((size_t)I);
  p.inner = seg(sizeof(unsigned long long) * 8);
  p.bytes = o;
  return p;
}

// the ladder 0 < beta_1 < ... < beta_S = 1 (0, or 1 with stb_last_error() set)
int ais_ladder(unsigned S, const double *betas_host, std::vector<double> *out, const char *who) {
  double prev = 0.0;
  for (unsigned s = 1; s <= S; s++) {
    const double be = betas_host ? betas_host[s - 1] : (s == S ? 1.0 : (double)s / (double)S);
    if (!(be > prev) || !(be <= 1.0))
      return stb_fail("%s: betas[%u]=%g (strictly increasing inside (0, 1]; the one before is %g)", who, s - 1, be, prev);
    if (out) out->push_back(be);
    prev = be;
  }
  if (prev != 1.0) return stb_fail("%s: the last beta is %.17g (the ladder ends at exactly 1.0)", who, prev);
  return 0;
}

int ais_temper_launch(const double *d_lik, unsigned rows, unsigned stride, double beta, double *d_out, hipStream_t st) {
  const uint64_t cells = (uint64_t)rows * stride;
  if (cells == 0) return 0;
  STB_LAUNCH(k_ais_temper, dim3((unsigned)((cells + 255) / 256)), dim3(256), st, d_lik, cells, beta, d_out);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // namespace

int stb_seat_anneal_check(double a, unsigned N, unsigned M, unsigned particles, unsigned S, const double *betas_host,
                          unsigned passes, int I, const char *who) {
  if (stb_seat_check(a, M, particles, 0, I, who)) return 1;
  if (N < 1 || M < 1) return stb_fail("%s: table bounds N=%u M=%u", who, N, M);
  if (S < 1) return stb_fail("%s: S=0 (at least one temperature: beta = 1)", who);
  if (passes < 1 || passes > (unsigned)INT_MAX) return stb_fail("%s: passes=%u (at least 1)", who, passes);
  if (ais_ladder(S, betas_host, nullptr, who)) return 1;
  if ((uint64_t)I * particles > (uint64_t)INT_MAX)
    return stb_fail("%s: %d restaurants x %u particles (at most %d replicas a call: split the restaurants)", who, I, particles, INT_MAX);
  return 0;
}

int stb_seat_anneal_launch(const stb_table_view &V, const stb_rest_view &r, const stb_cust_ro &cu, const stb_lik_view &L,
                           unsigned particles, const stb_ais_ladder &ld, const stb_draw_key &k, const stb_ais_out &out,
                           void *d_ws, size_t ws_bytes, hipStream_t st, const char *who) {
  const int I = r.I;
  const unsigned S = ld.S, passes = ld.passes, maxK = r.maxK;
  if (I == 0) return 0;
  if (stb_device_count() < 1) return stb_no_device(who);
  std::vector<double> beta;
  if (ais_ladder(S, ld.betas_host, &beta, who)) return 1;
  const ais_plan p = ais_layout((uint64_t)I, r.G, cu.C, particles, L.rows, L.stride);
  if (!d_ws || ws_bytes < p.bytes)
    return stb_fail("%s: the workspace holds %zu bytes, the call needs %zu (stb_seat_anneal_workspace_bytes)", who,
                    d_ws ? ws_bytes : (size_t)0, p.bytes);
  char *ws = (char *)d_ws;
  // the cap the sweeps will hold the restaurants to (stb_td_launch's), so that what they would skip is left out here
  const unsigned tdcap = maxK == 0 || maxK > STB_TD_MAXK ? STB_TD_MAXK : maxK;
  ais_args A;
  A.I = (uint64_t)I;
  A.G = r.G;
  A.C = cu.C;
  A.R = particles;
  A.rows = L.rows;
  A.stride = L.stride;
  A.N = V.N;
  A.cap = tdcap <= 64 ? 64u : (tdcap + 63u) & ~63u;
  A.koff = r.koff;
  A.coff = cu.off;
  A.bpar = r.bpar;
  A.h = r.h;
  A.lik = L.lik;
  A.cls = cu.cls;
  A.koff2 = (uint64_t *)(ws + p.koff2);
  A.coff2 = (uint64_t *)(ws + p.coff2);
  A.bpar2 = (double *)(ws + p.bpar2);
  A.h2 = r.h ? (double *)(ws + p.h2) : nullptr;
  A.lw = out.lw;
  A.n2 = out.pn ? out.pn : (uint32_t *)(ws + p.n2);
  A.t2 = out.pt ? out.pt : (uint16_t *)(ws + p.t2);
  A.cust2 = out.pcust ? out.pcust : (uint32_t *)(ws + p.cust2);
  A.cls2 = (uint32_t *)(ws + p.cls2);
  A.skip = (unsigned char *)(ws + p.skip);
  A.info = (unsigned long long *)out.info;
  unsigned long long *inner = (unsigned long long *)(ws + p.inner);
  A.inner = inner;
  double *d_tlik = (double *)(ws + p.tlik);

  const int nw = stb_env_waves("STB_AIS_WAVES", 4);
  const uint64_t items = (uint64_t)I * particles, groups = (items + nw - 1) / nw;
  const unsigned grid = (unsigned)(groups < AIS_MAXGRID ? groups : AIS_MAXGRID);
  // the replicated problem: I x particles restaurants, each with the pairs and the customers of its original.  (tdcap is
  // at most 64 exactly when maxK is 1 .. 64: the seating takes its register form as it would under maxK)
  const stb_rest_view r2 = {r.a, A.bpar2, (int)items, A.koff2, A.h2, tdcap};
  const stb_cnts_rw c2 = {A.n2, A.t2, (uint32_t *)(ws + p.T2)};
  const stb_cust_rw cu2 = {A.coff2, A.cls2, A.cust2};
  HIPCHK(hipMemsetAsync(inner, 0, sizeof(unsigned long long) * 8, st));
  STB_LAUNCH(k_ais_expand, dim3(grid), dim3(64 * nw), st, A);
  HIPCHK(hipGetLastError());
  // x_0 ~ prior: the committed seating of one particle a replica, no matrix.  Its own log weight is where lw starts: the
  // log of a product of sums of theta, 0 up to rounding -- but under a truncation M the sums fall short of 1 and the
  // seating is a weighted draw from the truncated prior (the header's statement), which is what the ladder needs
  // (without a matrix the seating reads no class)
  if (stb_seat_launch(r2, c2, V.M, cu2, stb_lik_view{}, 1, STB_SEAT_COMMIT, k, {out.lw, nullptr, (uint64_t *)inner}, st, who))
    return 1;
  const stb_lik_view tempered = {d_tlik, L.rows, L.stride};
  for (unsigned s = 1; s <= S; s++) {
    const double be = beta[s - 1], dbeta = be - (s >= 2 ? beta[s - 2] : 0.0);
    if (s < S && ais_temper_launch(L.lik, L.rows, L.stride, be, d_tlik, st)) return 1;
    STB_LAUNCH(k_ais_weight, dim3(grid), dim3(64 * nw), st, A, dbeta, s == 1 ? 1 : 0, s == S ? 1 : 0);
    HIPCHK(hipGetLastError());
    const stb_draw_key ks = {k.seed, k.sweep + 1 + (uint64_t)(s - 1) * passes};
    if (s < S && stb_td_launch(V, r2, c2, cu2, tempered, ks, (int)passes, inner + 3, st)) return 1;
  }
  return 0;
}

extern "C" size_t stb_seat_anneal_workspace_bytes(int I, uint64_t G, uint64_t C, unsigned particles, unsigned rows,
                                                  unsigned stride) {
  if (I < 0) return 0;
  return ais_layout((uint64_t)I, G, C, particles ? particles : 1, rows, stride).bytes;
}

extern "C" int stb_lik_temper(const double *d_lik, unsigned rows, unsigned stride, double beta, double *d_out, void *stream) {
  STB_ENTRY;
  const char *who = "stb_lik_temper";
  if (!d_lik || !d_out) return stb_fail("%s: the matrix and the output are required", who);
  if (!(beta >= 0.0) || !std::isfinite(beta)) return stb_fail("%s: beta=%g", who, beta);
  if ((uint64_t)rows * stride > ((uint64_t)1 << 39)) return stb_fail("%s: %u x %u cells", who, rows, stride);
  if (stb_device_count() < 1) return stb_no_device(who);
  return ais_temper_launch(d_lik, rows, stride, beta, d_out, (hipStream_t)stream);
}

extern "C" int stb_seat_anneal(const double *d_vtable, unsigned N, unsigned M, double a, const double *d_bpar, int I,
                               const uint64_t *d_koff, const double *d_h, const uint64_t *d_coff, const uint32_t *d_cls,
                               const double *d_lik, unsigned rows, unsigned stride, uint64_t G, uint64_t C, unsigned particles,
                               unsigned S, const double *betas_host, unsigned passes, uint64_t seed, uint64_t sweep,
                               double *d_lw, uint32_t *d_pn, uint16_t *d_pt, uint32_t *d_pcust, uint64_t *d_info, void *d_ws,
                               size_t ws_bytes, void *stream) {
  STB_ENTRY;
  const char *who = "stb_seat_anneal";
  if (stb_seat_anneal_check(a, N, M, particles, S, betas_host, passes, I, who)) return 1;
  if (!d_koff || !d_coff) return stb_fail("%s: the pair offsets and the customer offsets are required", who);
  if (I > 0 && !d_bpar) return stb_fail("%s: bpar is required", who);
  if (!d_lw) return stb_fail("%s: d_lw is required", who);
  if (!d_lik || !d_cls) return stb_fail("%s: the matrix and the classes are required (the prior alone has nothing to anneal to)", who);
  if (rows < 1 || stride < 1) return stb_fail("%s: a likelihood needs rows >= 1 and stride >= 1 (rows=%u, stride=%u)", who, rows, stride);
  if ((uint64_t)rows * stride > ((uint64_t)1 << 39)) return stb_fail("%s: %u x %u cells", who, rows, stride);
  if (!d_vtable && N >= 2 && M >= 2 && S >= 2) return stb_fail("%s: the V table is required (the sweeps read it)", who);
  const stb_table_view V = {d_vtable, N, M};
  stb_rest_view r = {a, d_bpar, I, d_koff, d_h};
  r.G = G;
  stb_cust_ro cu = {d_coff, d_cls};
  cu.C = C;
  const stb_lik_view L = {d_lik, rows, stride};
  const stb_ais_out out = {d_lw, d_info, d_pn, d_pt, d_pcust};
  return stb_seat_anneal_launch(V, r, cu, L, particles, {S, betas_host, passes}, {seed, sweep}, out, d_ws, ws_bytes,
                                (hipStream_t)stream, who);
}
