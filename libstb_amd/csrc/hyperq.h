/* hyperq.h -- private: what the device b step's host control flow (sampleb.c, C) needs of hyperq.hip and of the
 * object layers (tcounts_obj.hip, tindic_obj.hip), beyond include/stb_hip.h. */
#ifndef STB_HYPERQ_H
#define STB_HYPERQ_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* stb_sample_logq with the customers per restaurant given either way: d_N[I] (uint32), or d_coff[I+1] (uint64 prefix
 * sums: N_i = d_coff[i+1] - d_coff[i]); exactly one of the two is non-NULL */
int stb_hq_logq(double b, double scale, int I, const uint32_t *d_N, const uint64_t *d_coff, double *d_L, double *Q_host,
                uint64_t seed, uint64_t sweep, void *stream);
/* *sum_host = sum of d_T[0..I), queued on `stream` and waited for */
int stb_hq_sum_u32(const uint32_t *d_T, int I, uint64_t *sum_host, void *stream);
/* d_N[i] = sum of d_n over the pairs d_koff[i] .. d_koff[i+1] of restaurant i; queued on `stream` */
int stb_hq_segsum(const uint64_t *d_koff, const uint32_t *d_n, int I, uint32_t *d_N, void *stream);
/* frees the calling thread's block sums and result words (stb_sampler_cache_clear) */
void stb_hq_release(void);
/* records msg for stb_last_error(); returns 1 */
int stb_fail_msg(const char *msg);
/* sampleb.c: stb_sampleb_device with N given either way (see stb_hq_logq) */
double stb_sampleb_device_ex(double b_in, int I, double shape, double scale, const uint32_t *d_N, const uint64_t *d_coff,
                             const uint32_t *d_T, double a, void *rng, int loops, int verbose, uint64_t seed,
                             uint64_t sweep, void *stream, const char *who);
#ifdef __cplusplus
}
#endif
#endif
