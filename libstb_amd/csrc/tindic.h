// tindic.h -- what tindic.hip (the indicator sweep), tdish.hip (the dish sweep) and tindic_obj.hip (the object) share: the counter-based uniforms, the V
// cell look-up and the two decisions of a visit.  Both kernels evaluate a visit with these functions, so a dish visit whose
// customer stays in its dish gives the indicator visit's bits.  Moved out (MEASUREMENTS O6): the wave's readlane helpers,
// ti_rl and ti_rld, are wave.h's stb_wave_rl and stb_wave_rld; this header includes it.
#ifndef STB_TINDIC_H
#define STB_TINDIC_H

#include "stb_common.h"
#include "views.h"
#include "wave.h"
#include "uniforms.h"  // u1 of customer c is element j = 2c+1 of the sweep's stream, u2 is j = 2c+2

#define STB_TI_REF_ODDS_FLAG 1u

// V^n_m with stb_lookup_V's semantics for the cells a visit can address (2 <= n <= N): 0 outside 2 <= m <= min(n, M)
__device__ __forceinline__ double ti_V(const double *vt, unsigned M, unsigned n, unsigned m) {
  if (m < 2 || m > M || m > n) return 0.0;
  return vt[stb_vrow_offset(n, M) + (m - 2)];
}

__device__ __forceinline__ bool ti_remove(unsigned n, unsigned t, double u1) {
  return t > 1 && (double)(n - 1) * u1 < (double)(t - 1);
}

// t, T after the removal; t < n
__device__ __forceinline__ bool ti_add(unsigned n, unsigned t, uint32_t T, double h, double a, double b, double V, double u2,
                                       bool ref) {
#pragma clang fp contract(off)
  const double odds = h * (b + (double)T * a) * (double)t / (double)(ref ? n - t + 1 : n - t) * V;
  const double p = isinf(odds) ? 1.0 : odds / (odds + 1.0);
  return u2 < p;
}

// the indicator sweep's launch (tindic.hip): nsweeps sweeps from k.sweep on; r.maxK = dishes a wave keeps in LDS; of cu the
// offsets and the dishes are read
int stb_ti_launch(const stb_table_view &V, const stb_rest_view &r, const stb_cnts_tT &c, const stb_cust_ro &cu, unsigned flags,
                  const stb_draw_key &k, int nsweeps, hipStream_t st);
// the dish sweep's launch (tdish.hip): nsweeps sweeps from k.sweep on; r.maxK = dishes a wave holds (the largest K_i, at
// most STB_TD_MAXK); d_info: two uint64 (skipped, stuck), added to
int stb_td_launch(const stb_table_view &V, const stb_rest_view &r, const stb_cnts_rw &c, const stb_cust_rw &cu,
                  const stb_lik_view &L, const stb_draw_key &k, int nsweeps, unsigned long long *d_info, hipStream_t st);
// customers per (class, dish): cnt[rows x stride] += 1 at (cu.cls[c], cu.cust[c]) for c < cu.C
int stb_td_class_counts(const stb_cust_ro &cu, unsigned rows, unsigned stride, uint32_t *d_cnt, hipStream_t st);

#endif
