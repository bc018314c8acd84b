/* seat_pf.h -- private: what the object layer (tindic_obj.hip) needs of seat_pf.hip, beyond include/stb_hip.h. */
#ifndef STB_SEAT_PF_H
#define STB_SEAT_PF_H
#include <stdint.h>
#include "../../include/stb_hip.h"

#if defined(__HIPCC__)
/* the checks stb_seat_filter and the object's call share: stb_seat_check's, particles 1 .. STB_PF_MAXR, tau in [0, 1]
 * (0, or 1 with stb_last_error() set) */
int stb_seat_pf_check(double a, unsigned M, unsigned particles, double tau, int I, const char *who);
/* k_seat_pf on st, no wait; arguments checked by the caller.  maxK: the largest K_i where the caller knows it (the launch
 * then takes the LDS that needs, when it is inside the budget), else 0: the whole budget.  d_info: five uint64 (skipped,
 * impossible, stuck, dead, resamplings), added to */
int stb_seat_pf_launch(double a, const double *d_bpar, int I, const uint64_t *d_koff, const uint32_t *d_n, const uint16_t *d_t,
                       const double *d_h, unsigned M, const uint64_t *d_coff, const uint32_t *d_cls, const double *d_lik,
                       unsigned rows, unsigned stride, unsigned particles, double tau, uint64_t seed, uint64_t sweep, double *d_Hi,
                       double *d_w, int64_t *d_E, uint32_t *d_res, uint32_t *d_pn, uint16_t *d_pt, uint64_t *d_info, unsigned maxK,
                       hipStream_t st, const char *who);
#endif
#endif
