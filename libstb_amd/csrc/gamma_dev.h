// gamma_dev.h -- the device's log-Gamma variates, shared by hyperq.hip (the concentration step's auxiliaries) and tlik.hip
// (the Dirichlet draws of the likelihood and the base weights): one copy, so the two draw the same bits from the same
// uniforms.
//
// Uniforms: element k = 1, 2, ... of the substream `key` is m 2^-53 with m the top 53 bits of mix(key + k gamma), and
// 2^-54 in place of m = 0: always inside the open interval (0, 1), so every log is finite.
//
// log of a Gamma(alpha) variate, alpha >= 1 (Marsaglia & Tsang 2000): d = alpha - 1/3, c = 1 / sqrt(9 d); an attempt
// takes u1, u2, the normal x = sqrt(-2 log u1) cos(2 pi u2) (Box-Muller's cosine member; the sine member is not used),
// w = 1 + c x; w <= 0 ends the attempt; else v = w w w, a third uniform u, and the attempt is accepted when
//     log u < ((x x / 2 + d) - d v) + d log v          (evaluated as written, no contraction)
// with log G = log d + log v.  For alpha < 1 the boost in the log domain: log G = log G' + log(u') / alpha with
// G' ~ Gamma(alpha + 1) as above and one more uniform u' after it.  At most HQ_CAP attempts a variate (acceptance is
// above 0.95 an attempt): a lane that runs out sets `bad` and returns NaN; the caller raises its error word.
#ifndef STB_GAMMA_DEV_H
#define STB_GAMMA_DEV_H

#include "stb_common.h"
#include "tcounts.h"

#define HQ_CAP 64

#if defined(__HIPCC__)
__device__ __forceinline__ double hq_unit(uint64_t key, uint64_t k) {
  const uint64_t m = stb_mix64(key + k * STB_GAMMA) >> 11;
  return m ? (double)m * (1.0 / 9007199254740992.0) : (1.0 / 18014398509481984.0);
}

// log of a Gamma(alpha) variate, alpha >= 1; k counts the uniforms taken from the substream
__device__ __forceinline__ double hq_log_gamma_ge1(double alpha, uint64_t key, uint64_t &k, bool &bad) {
#pragma clang fp contract(off)
  const double d = alpha - 1.0 / 3.0;
  const double c = 1.0 / sqrt(9.0 * d);
  for (int it = 0; it < HQ_CAP; it++) {
    const double u1 = hq_unit(key, ++k);
    const double u2 = hq_unit(key, ++k);
    const double x = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
    const double w = 1.0 + c * x;
    if (!(w > 0.0)) continue;
    const double v = w * w * w;
    const double u = hq_unit(key, ++k);
    const double lv = log(v);
    if (log(u) < ((0.5 * (x * x) + d) - d * v) + d * lv) return log(d) + lv;
  }
  bad = true;
  return NAN;
}

__device__ __forceinline__ double hq_log_gamma(double alpha, uint64_t key, uint64_t &k, bool &bad) {
#pragma clang fp contract(off)
  if (alpha >= 1.0) return hq_log_gamma_ge1(alpha, key, k, bad);
  const double lg = hq_log_gamma_ge1(alpha + 1.0, key, k, bad);
  const double u = hq_unit(key, ++k);
  return lg + log(u) / alpha;
}

// L = -log q, q ~ Beta(b, Ni), for restaurant i of the sweep `key` (hyperq.hip's header: log G_b first, then log G_N, from
// the restaurant's substream key_i = mix(key + (i+1) gamma)); shared by hyperq.hip and hyperb.hip, so the two draw the
// same bits
__device__ __forceinline__ double hq_draw_L(double b, double Ni, uint64_t key, uint64_t i, bool &bad) {
#pragma clang fp contract(off)
  const uint64_t ki = stb_mix64(key + (i + 1) * STB_GAMMA);
  uint64_t k = 0;
  const double lgb = hq_log_gamma(b, ki, k, bad);
  const double lgn = hq_log_gamma(Ni, ki, k, bad);
  const double D = lgn - lgb;
  return D > 0.0 ? D + log1p(exp(-D)) : log1p(exp(D));
}
#endif  // __HIPCC__

#endif
