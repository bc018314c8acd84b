// gauss.h -- private: what gauss.hip's callers inside the library need beyond include/stb_hip.h.  Each call queues its
// launches on st, waits once and returns 0, or 1 with stb_last_error() set; the arguments are checked by the caller.
#ifndef STB_GAUSS_H
#define STB_GAUSS_H

#include "stb_common.h"

#define GS_CHUNK 256u  // customers of a chunk of the statistics' sums (part of the contract)
#define GS_BLOCK 256u  // terms of a block sum of the data term and the evidence (k_logjoint's block: part of the contract)

// kappa0, alpha0 and every beta0 positive and finite, every m0 finite
int stb_gs_check_prior(const stb_gauss_prior_t *prior, unsigned D, const char *who);
// 1 <= D <= STB_GS_MAXD, 1 <= K <= STB_TD_MAXK
int stb_gs_check_shape(unsigned K, unsigned D, const char *who);

int stb_gs_stats(const double *d_x, unsigned D, const uint32_t *d_cust, uint64_t C, unsigned K, uint32_t *d_n, double *d_mean,
                 double *d_Q, stb_gauss_info_t *info, hipStream_t st, const char *who);
int stb_gs_draw(const uint32_t *d_n, const double *d_mean, const double *d_Q, unsigned K, unsigned D,
                const stb_gauss_prior_t *prior, uint64_t seed, uint64_t sweep, double *d_mu, double *d_tau, hipStream_t st,
                const char *who);
// statistics, draw and matrix behind one another with one wait.  *touched (may be null) is set once the first launch that
// writes mu, tau or the matrix is queued: a call that fails with it unset has left them as they were
int stb_gs_step(const double *d_x, unsigned D, const uint32_t *d_cust, uint64_t C, unsigned K, const stb_gauss_prior_t *prior,
                uint64_t seed, uint64_t sweep, uint32_t *d_n, double *d_mean, double *d_Q, double *d_mu, double *d_tau,
                double *d_lik, unsigned stride, stb_gauss_info_t *info, hipStream_t st, const char *who, bool *touched);
// cls[c] = c and a C x stride matrix of ones, queued on st: no wait
int stb_gs_init(uint32_t *d_cls, uint64_t C, double *d_lik, unsigned stride, hipStream_t st);
int stb_gs_lik(const double *d_x, unsigned D, uint64_t C, const double *d_mu, const double *d_tau, unsigned K, double *d_lik,
               unsigned stride, stb_gauss_info_t *info, hipStream_t st, const char *who);
int stb_gs_loglik(const double *d_x, unsigned D, const uint32_t *d_cust, uint64_t C, const double *d_mu, const double *d_tau,
                  unsigned K, double *total_host, stb_gauss_info_t *info, hipStream_t st, const char *who);
int stb_gs_logml(const uint32_t *d_n, const double *d_mean, const double *d_Q, unsigned K, unsigned D,
                 const stb_gauss_prior_t *prior, double *total_host, hipStream_t st, const char *who);
// STB_GAUSS_WAVES (1, 2, 4 or 8; default 4)
unsigned stb_gs_waves();
// k_gs_prep alone on st, no wait: T holds muT, tauT (K D each) and H (K)
void stb_gs_queue_prep(const double *d_mu, const double *d_tau, unsigned K, unsigned D, double *T, hipStream_t st);
// held-out points (gauss_heldout.hip, stb_gauss_heldout): k_gs_prep and the point kernel queued on st, no wait.  d_accM null: no accumulation;
// d_resp null: no responsibilities
int stb_gs_heldout(const double *d_theta, unsigned tstride, int I, const uint64_t *d_hoff, const double *d_y, unsigned D,
                   const double *d_mu, const double *d_tau, unsigned K, double *d_ell, double *d_resp, unsigned rstride,
                   double *d_accM, double *d_accA, hipStream_t st, const char *who);
// (M, A) = (-inf, 0.0) on n points, queued on st: no wait
int stb_gs_heldout_reset(double *d_accM, double *d_accA, uint64_t n, hipStream_t st);

#endif
