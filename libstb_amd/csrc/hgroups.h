// hgroups.h -- private: what the object layer (tindic_obj.hip) needs of hgroups.hip beyond include/stb_hip.h.
#ifndef STB_HGROUPS_H
#define STB_HGROUPS_H

#include "stb_common.h"
#include "../../include/stb_hip.h"

// opts' alpha, gamma, flags and (with STB_HG_SAMPLE_ALPHA) prior positive and finite, Kmax inside 1 .. STB_TD_MAXK; 0, or 1
// with stb_last_error() set
int stb_hg_check_opts(const stb_hgroups_opts_t *opts, unsigned Kmax, const char *who);
// stb_sample_hgroups behind its checks: the caller has checked the arrays, Kmax, opts (stb_hg_check_opts) and the ranges
// (d_goff: 0 = goff[0] <= ... <= goff[G] = I, or null with G = I).  Queues every launch on st, waits once, fills *info.
// *touched (may be null) is set once the first launch that writes d_root / d_h is queued: a call that fails with it unset
// has left them as they were
int stb_hg_sample(int I, const uint64_t *d_koff, const uint16_t *d_t, unsigned Kmax, int G, const uint64_t *d_goff,
                  const stb_hgroups_opts_t *opts, double *d_root, double *d_h, double *d_hgrp, uint32_t *d_c, uint32_t *d_m,
                  uint64_t seed, uint64_t sweep, hipStream_t st, stb_hgroups_info_t *info, const char *who, bool *touched);
// the step's first launch alone: c_gk (d_c[G Kmax]) and C_g (d_Cg[G]) are added to -- the caller zeroes them on st first --
// by k_hg_count with the geometry stb_hg_sample gives it.  d_goff null: G = I.  Queued on st; no wait
int stb_hg_count_queue(int I, const uint64_t *d_koff, const uint16_t *d_t, unsigned Kmax, int G, const uint64_t *d_goff,
                       uint32_t *d_c, unsigned long long *d_Cg, hipStream_t st);
// two more launches of the step alone, for the tree step (htree.hip); nw = 1, 2, 4 or 8 waves a workgroup.  Queued on st; no wait.
// The root's row: d_root[k] ~ Dirichlet(gamma_k + d_s[k]) (d_gam[Kmax], or null for gamma0) on mix(key ^ HG_SALT_R)'s cells, the
// error bits or-ed into d_ctl[0]
int stb_hg_root_queue(unsigned Kmax, const unsigned long long *d_s, const double *d_gam, double gamma0, uint64_t key,
                      double *d_root, unsigned *d_ctl, unsigned nw, hipStream_t st);
// the scatter: d_hgrp's row of restaurant i's range to its pairs
int stb_hg_scatter_queue(int I, const uint64_t *d_koff, unsigned Kmax, int G, const uint64_t *d_goff, const double *d_hgrp,
                         double *d_h, unsigned nw, hipStream_t st);

#endif
