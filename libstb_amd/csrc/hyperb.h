/* hyperb.h -- private: what the object layers (tcounts.hip, tindic_obj.hip) and the tests need of hyperb.hip beyond
 * include/stb_hip.h. */
#ifndef STB_HYPERB_H
#define STB_HYPERB_H
#include <stdint.h>
#include "../../include/stb_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
/* stb_sample_bgroups with one more output: d_rate (G doubles, or NULL) receives every group's rate 1/scale + sum L_i, the
 * sum whose association the header fixes (for tests) */
int stb_hb_bgroups(double a, double shape, double scale, int I, const uint32_t *d_N, const uint64_t *d_coff, const uint32_t *d_T,
                   int G, const uint64_t *d_goff, double *d_bpar, double *d_bgrp, double *d_L, uint32_t *d_Y, double *d_rate,
                   uint64_t seed, uint64_t sweep, void *stream, stb_bgroups_info_t *info, const char *who);
/* the same step in two halves, for a caller that queues it among launches of its own and waits once (hgroups.hip):
 * _queue checks the arguments and queues the launches on `stream` (customers as d_N; no d_bgrp, no d_rate) without waiting;
 * _answer reads the pinned words of the calling thread's last _queue once that stream has been waited for, fills *info and
 * fails as stb_hb_bgroups does.  Between the two the thread makes no other stb_hb_* call */
int stb_hb_bgroups_queue(double a, double shape, double scale, int I, const uint32_t *d_N, const uint32_t *d_T, int G,
                         const uint64_t *d_goff, double *d_bpar, double *d_L, uint32_t *d_Y, uint64_t seed, uint64_t sweep,
                         void *stream, const char *who);
int stb_hb_bgroups_answer(int G, stb_bgroups_info_t *info, const char *who);
/* _queue with a = 0 over ranges whose prior's 1/scale is a device word that an earlier launch on `stream` leaves
 * (dirconc.hip: the scale is a product with a sum formed on the device); every other operation, stream and bit is _queue's */
int stb_hb_bgroups_queue_dscale(const double *d_inv_scale, double shape, int I, const uint32_t *d_N, const uint32_t *d_T, int G,
                                const uint64_t *d_goff, double *d_bpar, double *d_L, uint32_t *d_Y, uint64_t seed, uint64_t sweep,
                                void *stream, const char *who);
/* frees the calling thread's words and scratch (stb_sampler_cache_clear) */
void stb_hb_release(void);
#ifdef __cplusplus
}

/* what an object (stb_tcounts, stb_tindic) keeps for the step: its ranges and the step's L, Y and b_g, on its device */
struct stb_hb_obj {
  int G = 0;                  /* groups (0: every restaurant its own) */
  uint64_t *d_goff = nullptr; /* [G + 1], or null */
  double *d_L = nullptr;      /* [I] */
  uint32_t *d_Y = nullptr;    /* [I] */
  double *d_bgrp = nullptr;   /* [G or I] */
  bool resident = false;      /* the object's d_bpar holds concentrations (an upload, stb_*_set_bpar or a step put them there) */
  double min_b = 0.0;         /* a lower bound of what it holds: the smallest of the last upload, DBL_MIN after a step */
};
/* the staging helpers call this once bpar[I] is on its way to the object's d_bpar */
void stb_hb_obj_uploaded(stb_hb_obj *o, const double *bpar, int I);
/* STB_BPAR_RESIDENT in a call with discount a: 0 when the object holds concentrations and all are > -a (what the
 * host-side check of a host bpar asks); else 1 with stb_last_error() set */
int stb_hb_obj_resident(const stb_hb_obj *o, double a, const char *who);
/* all on the current device (the object's); 0, or 1 with stb_last_error() set */
int stb_hb_obj_set_groups(stb_hb_obj *o, int I, int G, const uint64_t *goff_host, void *stream, const char *who);
int stb_hb_obj_step(stb_hb_obj *o, double a, double shape, double scale, int I, const uint32_t *d_N, const uint64_t *d_coff,
                    const uint32_t *d_T, double *d_bpar, uint64_t seed, uint64_t sweep, void *stream, double *bgrp_host,
                    stb_bgroups_info_t *info, const char *who);
void stb_hb_obj_release(stb_hb_obj *o);
#endif
#endif
