// htree.h -- private: what the object layer (tindic_obj.hip) and the grouped step (hgroups.hip) need of htree.hip beyond
// include/stb_hip.h.
#ifndef STB_HTREE_H
#define STB_HTREE_H

#include "hgroups.h"

#define HT_SALT_L 0x3C6EF372FE94F82Bull  // level l >= 2 (level 1 is the leaves' own): key_l = mix(key ^ (HT_SALT_L + l))

// levels, every alpha, gamma (unless STB_HT_KEEP_ROOT), the prior (with STB_HT_SAMPLE_ALPHA) and the flags, Kmax inside
// 1 .. STB_TD_MAXK; alpha[levels] stands in for opts->alpha (the object's own when the caller gave none).  0, or 1 with
// stb_last_error() set
int stb_ht_check_opts(const stb_htree_opts_t *opts, const double *alpha, unsigned Kmax, const char *who);
// 0 = off[0] <= ... <= off[G] = below, on the host; 0, or 1 with stb_last_error() set
int stb_ht_check_ranges(int level, int G, const uint64_t *off_host, uint64_t below, const char *who);
// what a call that has not run says: every alpha NaN, the rest 0 (null: nothing)
void stb_ht_clear(stb_htree_info_t *info);
// stb_sample_htree behind its checks, and stb_sample_hgroups' step (hgroups.h): the caller has checked the arrays, Kmax, opts
// (stb_ht_check_opts) and every level's ranges.  alpha[levels] is read in place of opts->alpha.  d_off[0] may be null: every
// restaurant is its own level-1 node, G_host[0] = I.  Queues every launch on st with geo's geometry, waits once, fills
// *info.  *touched (may be null) is set once the first launch that writes d_root / d_h / a stored row is queued
int stb_ht_sample(int I, const uint64_t *d_koff, const uint16_t *d_t, unsigned Kmax, const int *G_host, const uint64_t *const *d_off,
                  const stb_htree_opts_t *opts, const double *alpha, double *d_root, double *const *d_hnode, double *d_h,
                  uint32_t *const *d_c, uint32_t *const *d_m, uint64_t seed, uint64_t sweep, hipStream_t st, stb_htree_info_t *info,
                  stb_hg_geom geo, const char *who, bool *touched);

#endif
