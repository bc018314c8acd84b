/* predict.h -- private: what the object layer (tindic_obj.hip) and the samplers' cache need of predict.hip, beyond
 * include/stb_hip.h. */
#ifndef STB_PREDICT_H
#define STB_PREDICT_H
#include <stdint.h>
#include "../../include/stb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* frees the calling thread's block sums, counters and result words (stb_sampler_cache_clear) */
void stb_pr_release(void);
/* the same for the held-out points' transposed parameters (gauss.hip) */
void stb_gh_release(void);
#ifdef __cplusplus
}
#endif

#if defined(__HIPCC__)
#include "views.h"
/* the checks stb_predict_dishes and the object's calls share (0, or 1 with stb_last_error() set) */
int stb_pr_check(double a, unsigned flags, int I, const char *who);
/* what k_predict writes: the proportions (I x tstride), the held-out customers' p, one uint64 that is added to */
struct stb_pr_out { double *theta = nullptr; unsigned tstride = 0; double *p = nullptr; uint64_t *skipped = nullptr; };
/* k_predict on st, no wait; arguments checked by the caller.  held: the held-out customers' offsets and classes
 * (stb_cust_ro{}: none), under L */
int stb_pr_predict(const stb_rest_view &r, const stb_cnts_ro &c, const stb_cust_ro &held, const stb_lik_view &L,
                   const stb_pr_out &out, unsigned flags, hipStream_t st, const char *who);
/* k_heldout_sum on st, the copy of d_Hi to Hi_host (when both are given) and the wait; d_skipped (or NULL: 0) is a
 * device word whose value goes into info->skipped */
int stb_pr_heldout(const double *d_p, const uint64_t *d_hoff, int I, unsigned samples, double *d_Hi, double *Hi_host,
                   double *total_host, stb_predict_info_t *info, const uint64_t *d_skipped, hipStream_t st, const char *who);
/* k_gh_sum: the same sum over x_c = d_x[c] (d_A null: log densities; a value that is not finite is impossible), or over
 * x_c = d_x[c] + log(d_A[c] / samples) (the log-domain accumulator pairs of gauss.hip's held-out points) */
int stb_pr_heldout_log(const double *d_x, const double *d_A, unsigned samples, const uint64_t *d_hoff, int I, double *d_Hi,
                       double *Hi_host, double *total_host, stb_predict_info_t *info, hipStream_t st, const char *who);
#endif
#endif
