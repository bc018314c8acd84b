/* hyperb.h -- private: what the object layers (tcounts_obj.hip, tindic_obj.hip) and the tests need of hyperb.hip beyond
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

#include <vector>
#include <hip/hip_runtime.h>

/* what an object (stb_tcounts, stb_tindic) keeps for its concentrations d_bpar[I]: the staging of host values on their way
 * there and what is known of the values it holds; and for the step its ranges and the step's L, Y and b_g, on its device */
struct stb_hb_obj {
  int G = 0;                  /* groups (0: every restaurant its own) */
  uint64_t *d_goff = nullptr; /* [G + 1], or null */
  double *d_L = nullptr;      /* [I] */
  uint32_t *d_Y = nullptr;    /* [I] */
  double *d_bgrp = nullptr;   /* [G or I] */
  bool resident = false;      /* the object's d_bpar holds concentrations (an upload, stb_*_set_bpar or a step put them there) */
  double min_b = 0.0;         /* a lower bound of what it holds: the smallest of the last upload, DBL_MIN after a step */
  double *h_bpar[2] = {nullptr, nullptr};     /* pinned staging of bpar, used in turn: a sweep does not wait for the one before it */
  hipEvent_t ev_bpar[2] = {nullptr, nullptr}; /* the copy out of h_bpar[k] is through */
  int slot = 0;
  std::vector<double> last_bpar;              /* the host values d_bpar holds (empty: nothing yet, or a device step wrote it) */
};
/* the staging area for I concentrations, once, from the object's create (which releases the object when this fails) */
int stb_hb_obj_init(stb_hb_obj *o, int I, const char *who);
/* bpar on the device before what is queued on st next: STB_BPAR_RESIDENT is what d_bpar holds (refused when it holds nothing);
 * I host values go through the staging buffer used two calls ago (its copy is long through), unchanged ones stay */
int stb_hb_obj_stage(stb_hb_obj *o, int I, double *d_bpar, const double *bpar, hipStream_t st, const char *who);
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
