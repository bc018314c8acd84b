// hgroups.h -- private: what the object layer (tindic_obj.hip) and the tree step (htree.hip) need of hgroups.hip beyond
// include/stb_hip.h.
#ifndef STB_HGROUPS_H
#define STB_HGROUPS_H

#include "stb_common.h"
#include "../../include/stb_hip.h"

// the step's error word (ctl[0] on the device, info->error_word)
#define HG_ERR_CAP 1u
#define HG_ERR_Z 2u
#define HG_ERR_SHAPE 4u
#define HG_ERR_TOTAL 8u

// the launches' geometry: nw = 1, 2, 4 or 8 waves a workgroup; a cell with more than twave Bernoulli draws goes to its wave
struct stb_hg_geom {
  unsigned nw, twave;
};
// from a pair of environment names: waves = 1 | 2 | 4 | 8 (anything else, or unset: 4), form = lane | wave (unset: HG_TWAVE)
stb_hg_geom stb_hg_geom_env(const char *waves_name, const char *form_name);

// opts' alpha, gamma, flags and (with STB_HG_SAMPLE_ALPHA) prior positive and finite, Kmax inside 1 .. STB_TD_MAXK; 0, or 1
// with stb_last_error() set
int stb_hg_check_opts(const stb_hgroups_opts_t *opts, unsigned Kmax, const char *who);
// what that and stb_ht_check_opts share: Kmax, the flags, alpha[levels] (named alpha[l] when indexed), gamma, the prior
int stb_hg_check_common(unsigned flags, const double *alpha, int levels, bool indexed, double gamma0, const double *gamma_host,
                        double shape, double scale, unsigned Kmax, const char *who);
// what a call that has not run says: alpha NaN, the rest 0 (null: nothing)
void stb_hg_clear(stb_hgroups_info_t *info);
// stb_sample_hgroups behind its checks: the caller has checked the arrays, Kmax, opts (stb_hg_check_opts) and the ranges
// (d_goff: 0 = goff[0] <= ... <= goff[G] = I, or null with G = I).  The tree's step (htree.h) on one level, with
// STB_HGROUPS_WAVES and _FORM: queues every launch on st, waits once, fills *info.  *touched (may be null) is set once the
// first launch that writes d_root / d_h is queued: a call that fails with it unset has left them as they were
int stb_hg_sample(int I, const uint64_t *d_koff, const uint16_t *d_t, unsigned Kmax, int G, const uint64_t *d_goff,
                  const stb_hgroups_opts_t *opts, double *d_root, double *d_h, double *d_hgrp, uint32_t *d_c, uint32_t *d_m,
                  uint64_t seed, uint64_t sweep, hipStream_t st, stb_hgroups_info_t *info, const char *who, bool *touched);

// the step's launches one by one, queued on st without a wait; nw is stb_hg_geom's.
// Level 1's counts: c_gk (d_c[G Kmax]) and C_g (d_Cg[G]) are added to -- the caller zeroes them on st first.  d_goff null: G = I
int stb_hg_count_queue(int I, const uint64_t *d_koff, const uint16_t *d_t, unsigned Kmax, int G, const uint64_t *d_goff,
                       uint32_t *d_c, unsigned long long *d_Cg, unsigned nw, hipStream_t st);
// a level's auxiliary tables on key: m (d_m[G Kmax], or null) and M_v (d_Mv[G], added to) from d_c[G Kmax] with w = alpha
// base_k, base the row of d_base that d_poff[Gp + 1] gives the row's parent (null: row 0); the parents' counts are added to
// d_cpar[Gp Kmax] and d_Cpar[Gp], or, both null, to d_s[Kmax]
int stb_hg_aux_queue(unsigned Kmax, uint64_t G, const uint32_t *d_c, uint64_t Gp, const uint64_t *d_poff, const double *d_base,
                     double alpha, uint64_t key, stb_hg_geom geo, uint32_t *d_m, uint32_t *d_Mv, uint32_t *d_cpar,
                     unsigned long long *d_Cpar, unsigned long long *d_s, hipStream_t st);
// the root's row: d_root[k] ~ Dirichlet(gamma_k + d_s[k]) (d_gam[Kmax], or null for gamma0) on mix(key ^ HG_SALT_R)'s cells, the
// error bits or-ed into d_ctl[0]
int stb_hg_root_queue(unsigned Kmax, const unsigned long long *d_s, const double *d_gam, double gamma0, uint64_t key,
                      double *d_root, unsigned *d_ctl, unsigned nw, hipStream_t st);
// a level's rows on key: d_out[v] ~ Dirichlet(*d_factor base_k + d_c[v Kmax + k]), base as for the auxiliary tables
int stb_hg_rows_queue(uint64_t G, unsigned Kmax, const uint32_t *d_c, uint64_t Gp, const uint64_t *d_poff, const double *d_base,
                      const double *d_factor, uint64_t key, double *d_out, unsigned *d_ctl, unsigned nw, hipStream_t st);
// the scatter: d_hgrp's row of restaurant i's range to its pairs
int stb_hg_scatter_queue(int I, const uint64_t *d_koff, unsigned Kmax, int G, const uint64_t *d_goff, const double *d_hgrp,
                         double *d_h, unsigned nw, hipStream_t st);

#endif
