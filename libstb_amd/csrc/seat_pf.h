/* seat_pf.h -- private: what the object layer (tindic_obj.hip) needs of seat_pf.hip, beyond include/stb_hip.h. */
#ifndef STB_SEAT_PF_H
#define STB_SEAT_PF_H
#include <stdint.h>
#include "../../include/stb_hip.h"

#if defined(__HIPCC__)
#include "views.h"
/* the checks stb_seat_filter and the object's call share: stb_seat_check's, particles 1 .. STB_PF_MAXR, tau in [0, 1]
 * (0, or 1 with stb_last_error() set) */
int stb_seat_pf_check(double a, unsigned M, unsigned particles, double tau, int I, const char *who);
/* what k_seat_pf writes: H_i, five uint64 (skipped, impossible, stuck, dead, resamplings) that are added to, and for who
 * asks the slots' last weights, exponents, resampling counts and states (stb_seat_filter's d_w, d_E, d_res, d_pn, d_pt) */
struct stb_pf_out {
  double *Hi;
  uint64_t *info = nullptr;
  double *w = nullptr; int64_t *E = nullptr; uint32_t *res = nullptr, *pn = nullptr; uint16_t *pt = nullptr;
};
/* k_seat_pf on st, no wait; arguments checked by the caller.  r.maxK: the largest K_i where the caller knows it (the
 * launch then takes the LDS that needs, when it is inside the budget), else 0: the whole budget.  M: the truncation of t
 * (0: none).  Of cu the offsets and the classes are read */
int stb_seat_pf_launch(const stb_rest_view &r, const stb_cnts_ro &c, unsigned M, const stb_cust_ro &cu, const stb_lik_view &L,
                       unsigned particles, double tau, const stb_draw_key &k, const stb_pf_out &out, hipStream_t st,
                       const char *who);
#endif
#endif
