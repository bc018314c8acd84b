/* hyperj.h -- private: what the object layers (tcounts_obj.hip, tindic_obj.hip) and the samplers' cache need of hyperj.hip,
 * beyond include/stb_hip.h. */
#ifndef STB_HYPERJ_H
#define STB_HYPERJ_H
#include <stdint.h>
#include "../../include/stb_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
/* stb_groups_samplejoint with the customers per restaurant given either way: d_N[I] (uint32), or d_coff[I+1] (uint64
 * prefix sums: N_i = d_coff[i+1] - d_coff[i]); exactly one of the two is non-NULL.  `who` names the caller in messages. */
int stb_hj_samplejoint(stb_groups_t *g, const uint32_t *d_N, const uint64_t *d_coff, const stb_joint_opts_t *opts, double a_in,
                       double b_in, double *a_out, double *b_out, stb_joint_info_t *info, const char *who);
/* stb_joint_terms with the customers per restaurant given either way, as above (the objects' steps take d_coff) */
int stb_hj_joint_terms(const double *a_host, int D, const double *b_host, int J, const uint32_t *d_T, const uint32_t *d_N,
                       const uint64_t *d_coff, uint64_t I, double *d_out, void *stream);
/* frees the calling thread's block sums, stage buffers and result words (stb_sampler_cache_clear) */
void stb_hj_release(void);
#ifdef __cplusplus
}
#endif
#endif
