/* seat_ais.h -- private: what the object layer (tindic_obj.hip) needs of seat_ais.hip, beyond include/stb_hip.h. */
#ifndef STB_SEAT_AIS_H
#define STB_SEAT_AIS_H
#include <stdint.h>
#include "../../include/stb_hip.h"

#if defined(__HIPCC__)
#include "views.h"
/* the checks stb_seat_anneal and the object's call share: stb_seat_check's on (a, M, particles, I), the table bounds as
 * stb_sample_tdishes, S >= 1, passes >= 1, the ladder (betas_host NULL: the even one), I * particles inside an int
 * (0, or 1 with stb_last_error() set) */
int stb_seat_anneal_check(double a, unsigned N, unsigned M, unsigned particles, unsigned S, const double *betas_host,
                          unsigned passes, int I, const char *who);
/* the temperatures: S of them (betas_host NULL: the even ladder), `passes` dish sweeps after each but the last */
struct stb_ais_ladder { unsigned S; const double *betas_host; unsigned passes; };
/* what the ladder writes: the log weights (I x particles), three uint64 (skipped, dead, stuck) that are added to, and for
 * who asks the replicas' last states (stb_seat_anneal's d_pn, d_pt, d_pcust) */
struct stb_ais_out { double *lw; uint64_t *info = nullptr; uint32_t *pn = nullptr; uint16_t *pt = nullptr; uint32_t *pcust = nullptr; };
/* the whole ladder on st, no wait; arguments checked by the caller.  r.G and cu.C are read; r.maxK: the largest K_i where
 * the caller knows it (the seating and the sweeps then take the register form when it is at most 64), else 0.  Of cu
 * the offsets and the classes are read */
int stb_seat_anneal_launch(const stb_table_view &V, const stb_rest_view &r, const stb_cust_ro &cu, const stb_lik_view &L,
                           unsigned particles, const stb_ais_ladder &ld, const stb_draw_key &k, const stb_ais_out &out,
                           void *d_ws, size_t ws_bytes, hipStream_t st, const char *who);
#endif
#endif
