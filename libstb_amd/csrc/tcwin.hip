// tcwin.hip -- the windowed table-count sweep (test/check.c's SampleCTW) made exact: a pair's t is proposed from the
// conditional restricted to the window [t-W, t+W] and the move is accepted with probability min(1, Z(t) / Z(tau')),
// Z(x) the weight of x's window.  O(W) work a pair instead of the O(min(n, M)) of k_tcounts.
//
//   k_tcwin   one wave per restaurant, several independent waves per workgroup; no workgroup barrier
//
// For a pair (n, t, h) of restaurant i the weights are k_tcounts' (tcounts.hip): log w(tau) = S_S(n, tau) +
// (tau-1) log h + sum_{s=T_+1}^{T_+tau-1} log(b + s a), T_ = T_i - t.  With Mt = min(n, M), lo(x) = max(1, x-W),
// hi(x) = min(Mt, x+W), a visit reads the span lo(t-W) .. hi(t+W) (at most 4W+1 tau values: both windows a move can
// compare lie in it), one tau a lane, in chunks of 64:
//   - spans of one chunk: log w relative to w(t), the log terms summed by two segmented wave scans that start at t --
//     upward over tau > t, downward over tau < t; log w stays in a register for the passes below;
//   - longer spans: log w relative to the span's first tau, one scan carried across chunks, recomputed every pass
//     (the same operations in the same order: the same bits).
// Then the proposal (max over win(t), exp, a scan, Z(t), the first tau whose cumulative weight exceeds u1 Z(t), by
// ballot) and, when tau' != t, the acceptance: the max over win(t) u win(tau'), exp, and Z(t), Z(tau') on that scale
// (xor-butterfly sums: every lane holds the same bits); accept iff u2 Z(tau') < Z(t).  Only T_i carries from a pair to
// the next, so pair g+1's S cells and pair g+2's (n, t, h) are loaded while pair g is drawn.  Every lane stores the new
// t (the same value): a later sweep's load of it is then ordered after the store by each lane's own program order.
//
// Uniforms: tindic.hip's convention on the flat pair index g: u1 = element 2g+1, u2 = element 2g+2 of sweep s's
// stream (key = mix(seed + (s+1) gamma)); the draws depend on (seed, sweep, g) alone, not on STB_TCWIN_WAVES.

#include "stb_common.h"
#include "tcounts.h"

#define STB_TCW_MAXWAVES 8   // (launch bounds: the kernel needs ~150 VGPRs)

struct tcw_pair {
  unsigned n, t;
  double h;
};

__device__ __forceinline__ tcw_pair tcw_load(const uint32_t *nv, const uint16_t *tv, const double *hv, uint64_t g, uint64_t k1) {
  tcw_pair p = {0u, 0u, 1.0};
  if (g < k1) {
    p.n = nv[g];
    p.t = tv[g];
    if (hv) p.h = hv[g];
  }
  return p;
}

// where a pair's visit reads: Mt = min(n, M), tc = t clamped to [1, Mt], the span [slo, shi] = [lo(tc-W), hi(tc+W)]
struct tcw_geom {
  unsigned Mt, tc, slo, shi;
};

__device__ __forceinline__ unsigned tcw_lo(unsigned x, unsigned W) { return x > W ? x - W : 1u; }
__device__ __forceinline__ unsigned tcw_hi(unsigned x, unsigned W, unsigned Mt) {
  return (uint64_t)x + W < Mt ? x + W : Mt;
}

__device__ __forceinline__ tcw_geom tcw_span(unsigned n, unsigned t, unsigned M, unsigned W) {
  tcw_geom q;
  q.Mt = n < M ? n : M;
  q.tc = t < 1 ? 1 : (t > q.Mt ? q.Mt : t);
  const uint64_t W2 = 2ull * W;
  q.slo = q.tc > W2 ? (unsigned)(q.tc - W2) : 1u;
  q.shi = q.tc + W2 < q.Mt ? (unsigned)(q.tc + W2) : q.Mt;
  return q;
}

// S_S(n, tau) of the lane's tau in chunk k of the span (0 outside it; only pairs that draw, 2 <= Mt, n <= N, read)
__device__ __forceinline__ double tcw_cell(const double *table, const double *S1, unsigned n, unsigned M, const tcw_geom &q,
                                           unsigned k, unsigned lane) {
  const unsigned tau = q.slo + 64u * k + lane;
  if (tau > q.shi) return 0.0;
  return tc_S(table + stb_row_offset(n, M), S1, n, tau);
}

// (the wave collectives -- the all-lanes max and sum, the scan: every lane gets the same bits -- are wave.h's)

// the log weights of the span a pair visit reads, relative to a constant (which the scale exp(-max) removes)
struct tcw_row {
  const double *table, *S1;
  unsigned n, M, nc;
  tcw_geom q;
  double a, b, Tm, logh;
  double cell0;  // the lane's S cell of chunk 0 (prefetched)
  double lw1;    // nc == 1: the lane's log w, computed once
  double carry;  // nc > 1: the log terms summed over the chunks before this one (pass by pass, chunks in order)

  __device__ double term(unsigned tau) const {  // log(b + (T_ + tau - 1) a), as k_tcounts writes it
    return log(b + (Tm + (double)(tau - 1)) * a);
  }

  // nc == 1: log w(tau) - log w(tc); the log terms summed outward from tc in both directions
  __device__ void one_chunk(unsigned lane) {
#pragma clang fp contract(off)
    const unsigned tau = q.slo + lane, tc = q.tc;
    const bool in = tau <= q.shi;
    const double x = (in && tau > q.slo) ? term(tau) : 0.0;
    double up = tau > tc && in ? x : 0.0;
    double dn = __shfl_down(x, 1, 64);  // term(tau + 1): tau < tc has tau + 1 <= tc in the span
    if (!(tau < tc)) dn = 0.0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double u = __shfl_up(up, o, 64), d = __shfl_down(dn, o, 64);
      if (lane >= (unsigned)o && tau - o > tc) up += u;
      if (lane + o < 64 && tau + o < tc) dn += d;
    }
    const double D = tau > tc ? up : (tau < tc ? -dn : 0.0);
    lw1 = in ? cell0 + (double)((int)tau - (int)tc) * logh + D : -HUGE_VAL;
  }

  // log w of the lane's tau in chunk k (-inf outside the span)
  __device__ double lw(unsigned k, unsigned lane) {
#pragma clang fp contract(off)
    if (nc == 1) return lw1;
    if (k == 0) carry = 0.0;
    const unsigned tau = q.slo + 64u * k + lane;
    const bool in = tau <= q.shi;
    const double x = (in && tau > q.slo) ? term(tau) : 0.0;
    const double P = stb_wave_scan(x, lane) + carry;
    carry = __shfl(P, 63, 64);
    if (!in) return -HUGE_VAL;
    const double S = k == 0 ? cell0 : tcw_cell(table, S1, n, M, q, k, lane);
    return S + (double)((int)tau - (int)q.tc) * logh + P;
  }
};

// one visit of a pair that draws (2 <= Mt, n <= N): the new t
__device__ __forceinline__ unsigned tcw_visit(tcw_row &r, unsigned W, bool ref, double u1, double u2, unsigned lane) {
#pragma clang fp contract(off)
  const unsigned tc = r.q.tc, Mt = r.q.Mt, slo = r.q.slo;
  if (r.nc == 1) r.one_chunk(lane);
  const unsigned lo1 = tcw_lo(tc, W), hi1 = tcw_hi(tc, W, Mt);
  // the proposal: w on win(tc) scaled by exp(-its max)
  double m1 = -HUGE_VAL;
  for (unsigned k = 0; k < r.nc; k++) {
    const unsigned tau = slo + 64u * k + lane;
    const double lw = r.lw(k, lane);
    m1 = fmax(m1, tau >= lo1 && tau <= hi1 ? lw : -HUGE_VAL);
  }
  m1 = stb_wave_all_max(m1);
  double Z1 = 0.0, c1 = 0.0;
  for (unsigned k = 0; k < r.nc; k++) {
    const unsigned tau = slo + 64u * k + lane;
    const double lw = r.lw(k, lane);
    const double c = stb_wave_scan(tau >= lo1 && tau <= hi1 ? exp(lw - m1) : 0.0, lane) + Z1;
    Z1 = __shfl(c, 63, 64);
    c1 = c;  // (nc == 1: the cumulative weights, kept for the crossing)
  }
  const double target = u1 * Z1;
  unsigned tp = hi1;  // (C(hi1) = Z(tc) > u1 Z(tc): always found)
  if (r.nc == 1) {
    const unsigned tau = slo + lane;
    const unsigned long long m = __ballot(tau >= lo1 && tau <= hi1 && c1 > target);
    if (m) tp = slo + (unsigned)__ffsll(m) - 1;
  } else {
    double C = 0.0;
    for (unsigned k = 0; k < r.nc; k++) {
      const unsigned tau = slo + 64u * k + lane;
      const double lw = r.lw(k, lane);
      const double c = stb_wave_scan(tau >= lo1 && tau <= hi1 ? exp(lw - m1) : 0.0, lane) + C;
      C = __shfl(c, 63, 64);
      const unsigned long long m = __ballot(tau >= lo1 && tau <= hi1 && c > target);
      if (m) {
        tp = slo + 64u * k + (unsigned)__ffsll(m) - 1;
        break;
      }
    }
  }
  if (ref || tp == tc) return tp;
  // the acceptance: Z(tc) and Z(tp) on one scale, exp(-max over win(tc) u win(tp))
  const unsigned lo2 = tcw_lo(tc < tp ? tc : tp, W), hi2 = tcw_hi(tc < tp ? tp : tc, W, Mt);
  const unsigned lop = tcw_lo(tp, W), hip = tcw_hi(tp, W, Mt);
  double m2 = -HUGE_VAL;
  for (unsigned k = 0; k < r.nc; k++) {
    const unsigned tau = slo + 64u * k + lane;
    const double lw = r.lw(k, lane);
    m2 = fmax(m2, tau >= lo2 && tau <= hi2 ? lw : -HUGE_VAL);
  }
  m2 = stb_wave_all_max(m2);
  double Zt = 0.0, Zp = 0.0;
  for (unsigned k = 0; k < r.nc; k++) {
    const unsigned tau = slo + 64u * k + lane;
    const double lw = r.lw(k, lane);
    const double e = tau >= lo2 && tau <= hi2 ? exp(lw - m2) : 0.0;
    Zt += stb_wave_all_sum(tau >= lo1 && tau <= hi1 ? e : 0.0);
    Zp += stb_wave_all_sum(tau >= lop && tau <= hip ? e : 0.0);
  }
  return u2 * Zp < Zt ? tp : tc;
}

__global__ __launch_bounds__(64 * STB_TCW_MAXWAVES) void k_tcwin(const double *table, const double *S1, unsigned N,
                                                                 unsigned M, double a, const double *bpar, int I,
                                                                 const uint64_t *koff, const uint32_t *nv, uint16_t *tv,
                                                                 uint32_t *Tv, const double *hv, unsigned W, unsigned flags,
                                                                 uint64_t seed, uint64_t sweep0, int nsweeps) {
  const unsigned lane = threadIdx.x & 63;
  const int i = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (i >= I) return;  // (a whole wave: nothing waits for it)
  const bool ref = (flags & STB_TC_REF_WINDOW_FLAG) != 0;
  const uint64_t k0 = koff[i], k1 = koff[i + 1];
  const double b = bpar[i];
  uint32_t T = Tv[i];
  for (int s = 0; s < nsweeps; s++) {
    const uint64_t key = stb_mix64(seed + (sweep0 + (uint64_t)s + 1) * STB_GAMMA);
    // the pipeline (restarted every sweep: the next sweep's pairs are this sweep's stores): pair g+1's (n, t, h) and
    // its chunk-0 S cell, pair g+2's (n, t, h)
    tcw_pair p1 = tcw_load(nv, tv, hv, k0, k1), p2 = tcw_load(nv, tv, hv, k0 + 1, k1);
    tcw_geom q1 = tcw_span(p1.n, p1.t, M, W);
    double s1 = (p1.n <= N && q1.Mt >= 2) ? tcw_cell(table, S1, p1.n, M, q1, 0, lane) : 0.0;
    for (uint64_t g = k0; g < k1; g++) {
      const tcw_pair p = p1;
      const tcw_geom q = q1;
      const double cell = s1;
      p1 = p2;
      q1 = tcw_span(p1.n, p1.t, M, W);
      s1 = (p1.n <= N && q1.Mt >= 2) ? tcw_cell(table, S1, p1.n, M, q1, 0, lane) : 0.0;
      p2 = tcw_load(nv, tv, hv, g + 2, k1);
      if (p.n == 0 || p.n > N) continue;  // (n > N: outside the table -- the pair keeps its t)
      unsigned tnew = 1;
      if (q.Mt >= 2) {
        tcw_row r;
        r.table = table;
        r.S1 = S1;
        r.n = p.n;
        r.M = M;
        r.q = q;
        r.nc = (q.shi - q.slo + 64u) / 64u;
        r.a = a;
        r.b = b;
        r.Tm = (double)(T - p.t);  // T_ = T_i - t
        r.logh = hv ? log(p.h) : 0.0;
        r.cell0 = cell;
        r.lw1 = 0.0;
        r.carry = 0.0;
        tnew = tcw_visit(r, W, ref, stb_unit(key, 2 * g + 1), stb_unit(key, 2 * g + 2), lane);
      }
      T = T - p.t + tnew;
      if (tnew != p.t) tv[g] = (uint16_t)tnew;  // (every lane: the same value)
    }
  }
  if (lane == 0) Tv[i] = T;
}

int stb_tcw_launch(const stb_table_view &S, const stb_rest_view &r, const stb_cnts_tT &c, unsigned W, unsigned flags,
                   const stb_draw_key &k, int nsweeps, hipStream_t st) {
  if (r.I <= 0 || nsweeps <= 0) return 0;
  const int wpb = stb_env_waves("STB_TCWIN_WAVES", 4);
  STB_LAUNCH(k_tcwin, dim3((unsigned)((r.I + wpb - 1) / wpb)), dim3(64 * wpb), st, S.tab, S.S1, S.N, S.M, r.a, r.bpar, r.I,
             r.koff, c.n, c.t, c.T, r.h, W, flags, k.seed, k.sweep, nsweeps);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int stb_sample_tcounts_window(const double *d_table, const double *d_S1, unsigned N, unsigned M, double a,
                                         const double *d_bpar, int I, const uint64_t *d_koff, const uint32_t *d_n,
                                         uint16_t *d_t, uint32_t *d_T, const double *d_h, unsigned W, unsigned flags,
                                         uint64_t seed, uint64_t sweep, void *stream) {
  STB_ENTRY;
  if (!(a >= 0.0 && a < 1.0)) return stb_fail("stb_sample_tcounts_window: discount a=%g outside [0, 1)", a);
  if (N < 1 || M < 1) return stb_fail("stb_sample_tcounts_window: table bounds N=%u M=%u", N, M);
  if (M > 65535u) return stb_fail("stb_sample_tcounts_window: M=%u (t is a uint16: at most 65535)", M);
  if (W == 0) return stb_fail("stb_sample_tcounts_window: window W=0 (must be >= 1)");
  if (flags & ~STB_TC_REF_WINDOW_FLAG) return stb_fail("stb_sample_tcounts_window: unknown flags 0x%x", flags);
  if (I < 0) return stb_fail("stb_sample_tcounts_window: I=%d", I);
  const stb_table_view S = {d_table, N, M, d_S1};
  const stb_rest_view r = {a, d_bpar, I, d_koff, d_h};
  const stb_cnts_tT c = {d_n, d_t, d_T};
  return stb_tcw_launch(S, r, c, W, flags, {seed, sweep}, 1, (hipStream_t)stream);
}
