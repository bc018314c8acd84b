/* logjoint.h -- private: what the object layers (tcounts_obj.hip, tindic_obj.hip) and the samplers' cache need of
 * logjoint.hip, beyond include/stb_hip.h. */
#ifndef STB_LOGJOINT_H
#define STB_LOGJOINT_H
#include <stdint.h>
#include "../../include/stb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* frees the calling thread's block sums, counters and result words (stb_sampler_cache_clear) */
void stb_lj_release(void);
#ifdef __cplusplus
}
#endif

#if defined(__HIPCC__)
#include "views.h"
/* the checks stb_logjoint and the objects' calls share (0, or 1 with stb_last_error() set) */
int stb_lj_check(double a, unsigned flags, int I, const char *who);
/* the launch on st, the copy of d_Li to Li_host (when both are given) and the wait; arguments checked by the caller */
int stb_lj_run(const stb_table_view &S, const stb_rest_view &r, const stb_cnts_ro &c, unsigned flags, double *d_Li,
               double *Li_host, double *total_host, stb_logjoint_info_t *info, hipStream_t st, const char *who);
#endif
#endif
