/* seat_ais.h -- private: what the object layer (tindic_obj.hip) needs of seat_ais.hip, beyond include/stb_hip.h. */
#ifndef STB_SEAT_AIS_H
#define STB_SEAT_AIS_H
#include <stdint.h>
#include "../../include/stb_hip.h"

#if defined(__HIPCC__)
/* the checks stb_seat_anneal and the object's call share: stb_seat_check's on (a, M, particles, I), the table bounds as
 * stb_sample_tdishes, S >= 1, passes >= 1, the ladder (betas_host NULL: the even one), I * particles inside an int
 * (0, or 1 with stb_last_error() set) */
int stb_seat_anneal_check(double a, unsigned N, unsigned M, unsigned particles, unsigned S, const double *betas_host,
                          unsigned passes, int I, const char *who);
/* the whole ladder on st, no wait; arguments checked by the caller.  maxK: the largest K_i where the caller knows it
 * (the seating and the sweeps then take the register form when it is at most 64), else 0.  d_info: three uint64
 * (skipped, dead, stuck), added to */
int stb_seat_anneal_launch(const double *d_vt, unsigned N, unsigned M, double a, const double *d_bpar, int I,
                           const uint64_t *d_koff, const double *d_h, const uint64_t *d_coff, const uint32_t *d_cls,
                           const double *d_lik, unsigned rows, unsigned stride, uint64_t G, uint64_t C, unsigned particles,
                           unsigned S, const double *betas_host, unsigned passes, uint64_t seed, uint64_t sweep, double *d_lw,
                           uint32_t *d_pn, uint16_t *d_pt, uint32_t *d_pcust, uint64_t *d_info, void *d_ws, size_t ws_bytes,
                           unsigned maxK, hipStream_t st, const char *who);
#endif
#endif
