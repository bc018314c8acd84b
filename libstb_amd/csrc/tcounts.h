// tcounts.h -- what the table-count sweeps share: the counter-based uniforms (uniforms.h) and the S-row read (tcounts.hip,
// tcwin.hip), and the launches that the stb_tcounts_* object of tcounts_obj.hip drives.
#pragma once

#include "stb_common.h"
#include "uniforms.h"
#include "views.h"
#include "wave.h"  // the scan and the butterflies of k_tcounts, k_tcwin and k_partition

// S_S(n, tau) for 1 <= tau <= min(n, M): dev_S_S of sweep_terms.hip for the cells a draw can address
// (n <= N: the kernels leave pairs with n > N alone)
__device__ __forceinline__ double tc_S(const double *row, const double *S1, unsigned n, unsigned tau) {
  if (tau == n) return 0.0;
  if (tau == 1) return S1[n - 1];
  return row[tau - 2];
}

// the sweep's launch (tcounts.hip): nsweeps sweeps from k.sweep on, tau_max = the longest tau range a pair can have (sizes
// the LDS row); the arguments are checked by the caller
int stb_tc_launch(const stb_table_view &S, const stb_rest_view &r, const stb_cnts_tT &c, const stb_draw_key &k, int nsweeps,
                  unsigned tau_max, hipStream_t st);

#define STB_TC_REF_WINDOW_FLAG 1u

// nsweeps windowed sweeps (include/stb_hip.h, stb_sample_tcounts_window); the arguments are checked by the caller
int stb_tcw_launch(const stb_table_view &S, const stb_rest_view &r, const stb_cnts_tT &c, unsigned W, unsigned flags,
                   const stb_draw_key &k, int nsweeps, hipStream_t st);

#define STB_PT_REF_WALK_FLAG 1u

// the partition draw (partition.hip, include/stb_hip.h stb_sample_partition): zeroes cnt[S] on st, then fills it from the
// G pairs' n and t; d_sizes and d_soff go together
int stb_pt_launch(const stb_table_view &S, double a, uint64_t G, const stb_cnts_ro &c, uint32_t *d_cnt, unsigned Sh,
                  unsigned flags, const stb_draw_key &k, hipStream_t st, uint16_t *d_sizes = nullptr,
                  const uint64_t *d_soff = nullptr);
// the checks of the raw call that the object's call shares (0, or 1 with stb_last_error() set)
int stb_pt_check(double a, unsigned N, unsigned M, uint64_t G, unsigned S, unsigned flags, const char *who);

// what the object layer needs of a histogram (sweep_terms.hip)
struct stb_hist_view {
  int dev, I;
  unsigned S;
  uint32_t *d_cnt, *d_T;
  double *d_bpar;
  hipStream_t st;
};
int stb_hist_view_of(stb_hist_t *h, stb_hist_view *v);
