/* seat.h -- private: what the object layer (tindic_obj.hip) and the samplers' cache need of seat.hip, beyond
 * include/stb_hip.h. */
#ifndef STB_SEAT_H
#define STB_SEAT_H
#include <stdint.h>
#include "../../include/stb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* frees the calling thread's block sums, counters and result words (stb_sampler_cache_clear) */
void stb_seat_release(void);
#ifdef __cplusplus
}
#endif

#if defined(__HIPCC__)
#include "views.h"
/* the checks stb_seat_customers and the object's calls share (0, or 1 with stb_last_error() set) */
int stb_seat_check(double a, unsigned M, unsigned particles, unsigned flags, int I, const char *who);
/* what k_seat writes besides the state: the log weights (I x particles), a committed seating's p per customer, and three
 * uint64 (skipped, impossible, stuck) that are added to */
struct stb_seat_out { double *lw, *p = nullptr; uint64_t *info = nullptr; };
/* k_seat on st, no wait; arguments checked by the caller.  r.maxK: the largest K_i where the caller knows it (at most
 * 64: the launch takes no LDS), else 0.  M: the truncation of t (0: none).  c.T and cu.cust are written by a committed
 * seating only */
int stb_seat_launch(const stb_rest_view &r, const stb_cnts_rw &c, unsigned M, const stb_cust_rw &cu, const stb_lik_view &L,
                    unsigned particles, unsigned flags, const stb_draw_key &k, const stb_seat_out &out, hipStream_t st,
                    const char *who);
/* k_seat_sum on st, the copy of d_Hi to Hi_host (when both are given) and the wait.  d_info (or NULL): k_seat's three
 * words, copied into info->skipped, ->impossible, ->stuck; without it info->impossible is the number of restaurants
 * whose H_i is -inf and the other two are 0.  info->customers is left alone. */
int stb_seat_sum(const double *d_lw, int I, unsigned particles, double *d_Hi, double *Hi_host, double *total_host,
                 stb_seat_info_t *info, const uint64_t *d_info, hipStream_t st, const char *who);
#endif
#endif
