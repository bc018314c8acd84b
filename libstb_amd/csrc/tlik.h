// tlik.h -- private: what the object layer (tindic_obj.hip) needs of tlik.hip beyond include/stb_hip.h.  Each call queues its
// launches on st, waits once and returns 0, or 1 with stb_last_error() set; the arguments are checked by the caller.
#ifndef STB_TLIK_H
#define STB_TLIK_H

#include "stb_common.h"

// *touched (may be null) is set once the first launch that writes d_lik / d_h is queued: a call that fails with it unset
// has left the output as it was
// v[len] (or, when v is null, v0) positive and finite
int stb_tl_check_prior(const double *v, uint64_t len, double v0, const char *name, const char *who);
int stb_tl_sample_lik(const uint32_t *d_cnt, unsigned rows, unsigned stride, const double *beta_host, double beta0,
                      double *d_lik, uint64_t seed, uint64_t sweep, hipStream_t st, const char *who, bool *touched);
// dish k is local pair k of every restaurant; Kmax the largest K_i (1 <= Kmax <= STB_TD_MAXK); d_h[G] is written
int stb_tl_sample_h(int I, const uint64_t *d_koff, const uint16_t *d_t, unsigned Kmax, const double *gamma_host, double gamma0,
                    double *d_h, uint64_t seed, uint64_t sweep, hipStream_t st, const char *who, bool *touched);
int stb_tl_loglik(const uint32_t *d_cnt, const double *d_lik, unsigned rows, unsigned stride, double *total_host,
                  uint64_t *impossible_host, hipStream_t st, const char *who);

#endif
