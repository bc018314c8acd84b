/* seat_visit.h -- private: one visit of the forward seating (include/stb_hip.h, "seating customers one by one", steps
 * 1 to 4), shared by the kernels that seat: k_seat (seat.hip: a wave a particle, nobody waits) and k_seat_pf
 * (seat_pf.hip: a workgroup a restaurant, the particles meet after every customer).  The arithmetic is the header's, word
 * for word; whoever includes this seats by the same bits.  st_args fills the kernels' arguments for both launches.
 *
 * Moved out (MEASUREMENTS O6): the scan, the 64-bit readlane and the register form's choice are wave.h's, and this header
 * takes the readlanes from there, not from tindic.h.
 * Stayed out: the customer walk (the next chunk's classes and the next customer's row of L, prefetched) is written out
 * twice, in seat_item (seat.hip) and in k_seat_pf.  Written once here and called from both, it cost k_seat_pf 0.7 to 1.3 % at
 * every tau of tools/time_seat_pf.py, outside the parent's own spread (its code moved though no count did: 2664 lines
 * before and after, the same registers); k_seat stayed inside its spread, but a walk with one caller shares nothing. */
#ifndef STB_SEAT_VISIT_H
#define STB_SEAT_VISIT_H
#include "stb_common.h"
#include "uniforms.h"
#include "views.h"
#include "wave.h"

struct seat_args {
  double a;
  const double *bpar;
  uint64_t I;
  const uint64_t *koff;
  uint32_t *nv;
  uint16_t *tv;
  uint32_t *Tv;
  const double *hv;
  unsigned M;
  const uint64_t *coff;
  const uint32_t *cls;
  uint32_t *cust;
  const double *lik;
  unsigned rows, stride, R, flags;
  uint64_t seed, sweep;
  double *lw, *p;
  unsigned long long *info;
};

// what both launches fill alike, from the view records they hold: a seating that commits nothing, weighs nothing and
// writes no state (Tv, cust, lw and p null, flags 0).  stb_seat_launch sets those five; stb_seat_pf_launch none.  (n and
// t lose their const here: k_seat stores to them under STB_SEAT_COMMIT alone, whose caller holds them writable, and
// k_seat_pf never)
static inline seat_args st_args(const stb_rest_view &r, const stb_cnts_ro &c, unsigned M, const stb_cust_ro &cu,
                                const stb_lik_view &L, unsigned particles, const stb_draw_key &k, uint64_t *info) {
  seat_args A;
  A.a = r.a;
  A.bpar = r.bpar;
  A.I = (uint64_t)r.I;
  A.koff = r.koff;
  A.nv = const_cast<uint32_t *>(c.n);
  A.tv = const_cast<uint16_t *>(c.t);
  A.Tv = nullptr;
  A.hv = r.h;
  A.M = M ? M : 65535u;
  A.coff = cu.off;
  A.cls = cu.cls;
  A.cust = nullptr;
  A.lik = L.lik;
  A.rows = L.rows;
  A.stride = L.stride;
  A.R = particles;
  A.flags = 0;
  A.seed = k.seed;
  A.sweep = k.sweep;
  A.lw = nullptr;
  A.p = nullptr;
  A.info = (unsigned long long *)info;
  return A;
}

// x, y and theta of a pair (n, t, h) in a restaurant with g = b + T a, den = b + N
__device__ __forceinline__ double st_theta(unsigned n, unsigned t, double h, double a, double g, double den, bool empty, unsigned M,
                                           double &x, double &y) {
#pragma clang fp contract(off)
  const double ta = (double)t * a;
  x = (double)n - ta;
  const double gh = g * h;
  y = (n >= 1 && t + 1 > M) ? 0.0 : gh;
  return empty ? h : (x + y) / den;
}

// One customer of class cl (lrow: cl < rows) on one particle's state, before -> after.  REG: a dish a lane, the pair in
// rn, rt, rh and the customer's row of L in Lcur (K <= 64, nblk = 1); else n and t in ln, lt (the wave's own), h and L
// read through the cache.  kg: the restaurant's first pair; b, T, N: its concentration and the particle's sums.  Out:
// ks the dish, pc the visit's p (0: impossible, then dead is set and n_imp counts; n_stuck: seated at dish 0).
template <bool REG>
__device__ __forceinline__ void st_visit(const seat_args &A, uint64_t kg, unsigned K, unsigned nblk, double a, double b, unsigned M,
                                         unsigned lane,
                                         uint32_t *ln, uint16_t *lt, unsigned &rn, unsigned &rt, double rh, double Lcur,
                                         unsigned cl, bool lrow, double u2, double u3, unsigned long long &T_io,
                                         unsigned long long &N_io, unsigned &ks_out, double &pc_out, bool &dead,
                                         unsigned long long &n_imp, unsigned long long &n_stuck) {
#pragma clang fp contract(off)
  const double *hv = A.hv, *lik = A.lik;
  unsigned long long T = T_io, N = N_io;  // (locals: a reference that is stored to on two paths survives inlining as memory)
  // ---- 1. weights, 2. their cumulative sums
  const bool empty = N == 0;
  const double g = b + (double)T * a, den = b + (double)N;
  double Z = 0.0, cum = 0.0, th0 = 0.0;
  uint64_t pos = 0;    // register form: dishes with q > 0; LDS form: lane j holds block j's
  double basev = 0.0;  // LDS form: lane j holds the base of block j
  if (REG) {
    double x, y;
    th0 = lane < K ? st_theta(rn, rt, rh, a, g, den, empty, M, x, y) : 0.0;
    const double q = lane < K ? th0 * (lik ? Lcur : 1.0) : 0.0;
    cum = 0.0 + stb_wave_scan(q, lane);
    pos = __ballot(q > 0.0);
    Z = stb_wave_rld(cum, 63);
  } else {
    double base = 0.0;
    for (unsigned blk = 0; blk < nblk; blk++) {
      const unsigned k = blk * 64 + lane;
      double q = 0.0;
      if (k < K) {
        double x, y;
        const double th = st_theta(ln[k], lt[k], hv ? hv[kg + k] : 1.0, a, g, den, empty, M, x, y);
        q = th * (lik ? (lrow ? lik[(uint64_t)cl * A.stride + k] : 0.0) : 1.0);
      }
      const double cm = base + stb_wave_scan(q, lane);
      const uint64_t pm = __ballot(q > 0.0);
      if (lane == blk) pos = pm, basev = base;
      base = stb_wave_rld(cm, 63);
    }
    Z = base;
  }
  bool useL = true;
  bool nowhere = false;
  double pc = Z;
  if (!(Z > 0.0 && isfinite(Z))) {
    // ---- 3. impossible: the weight is 0; the customer is seated on theta alone, with the same u3
    pc = 0.0;
    dead = true;
    n_imp++;
    useL = false;
    if (REG) {
      const double q = lane < K ? th0 : 0.0;
      cum = 0.0 + stb_wave_scan(q, lane);
      pos = __ballot(q > 0.0);
      Z = stb_wave_rld(cum, 63);
    } else {
      double base = 0.0;
      pos = 0;
      for (unsigned blk = 0; blk < nblk; blk++) {
        const unsigned k = blk * 64 + lane;
        double q = 0.0;
        if (k < K) {
          double x, y;
          q = st_theta(ln[k], lt[k], hv ? hv[kg + k] : 1.0, a, g, den, empty, M, x, y);
        }
        const double cm = base + stb_wave_scan(q, lane);
        const uint64_t pm = __ballot(q > 0.0);
        if (lane == blk) pos = pm, basev = base;
        base = stb_wave_rld(cm, 63);
      }
      Z = base;
    }
    if (!(Z > 0.0 && isfinite(Z))) {
      nowhere = true;
      n_stuck++;
    }
  }
  // ---- the choice: the smallest k with q_k > 0 and cum_k > thr, else the largest k with q_k > 0
  unsigned ks = 0;
  if (!nowhere) {
    const double thr = u3 * Z;
    if (REG) {
      ks = stb_wave_choice(pos, cum, thr, lane);
    } else {
      bool found = false;
      unsigned lastb = 0;
      uint64_t lastm = 1;
      for (unsigned blk = 0; blk < nblk && !found; blk++) {
        const uint64_t pm = stb_wave_rl64(pos, blk);
        if (!pm) continue;
        const unsigned k = blk * 64 + lane;
        double q = 0.0;
        if (k < K) {
          double x, y;
          const double th = st_theta(ln[k], lt[k], hv ? hv[kg + k] : 1.0, a, g, den, empty, M, x, y);
          q = useL ? th * (lik ? (lrow ? lik[(uint64_t)cl * A.stride + k] : 0.0) : 1.0) : th;
        }
        const double cm = stb_wave_rld(basev, blk) + stb_wave_scan(q, lane);
        const uint64_t hit = __ballot(((pm >> lane) & 1) && cm > thr);
        if (hit) {
          ks = blk * 64 + (unsigned)__builtin_ctzll(hit);
          found = true;
        }
        lastb = blk, lastm = pm;
      }
      if (!found) ks = lastb * 64 + 63u - (unsigned)__builtin_clzll(lastm);
    }
  }
  // ---- 4. the head, from the chosen dish's own x and y
  const unsigned ns = REG ? stb_wave_rl(rn, ks) : ln[ks], ts = REG ? stb_wave_rl(rt, ks) : (unsigned)lt[ks];
  const double hs = REG ? stb_wave_rld(rh, ks) : (hv ? hv[kg + ks] : 1.0);
  double xs, ys;
  (void)st_theta(ns, ts, hs, a, g, den, empty, M, xs, ys);
  const bool isnew = ns == 0 || u2 * (xs + ys) < ys;
  if (REG) {
    if (lane == ks) rn = ns + 1, rt = ts + (isnew ? 1u : 0u);
  } else {
    ln[ks] = ns + 1;
    if (isnew) lt[ks] = (uint16_t)(ts + 1);
  }
  N++;
  if (isnew) T++;
  T_io = T;
  N_io = N;
  ks_out = ks;
  pc_out = pc;
}

#endif
