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

#endif
