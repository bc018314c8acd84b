// dirconc.h -- private: what the object layer (tindic_obj.hip) needs of dirconc.hip beyond include/stb_hip.h.
#ifndef STB_DIRCONC_H
#define STB_DIRCONC_H

#include "stb_common.h"
#include "../../include/stb_hip.h"

// the checks stb_sample_dirconc makes before anything is queued (0, or 1 with stb_last_error() set)
int stb_dc_check(const uint32_t *d_cnt, uint64_t rows, unsigned cols, unsigned stride, unsigned flags, const double *d_w, double w0,
                 double s, double shape, double scale, const stb_dirconc_info_t *info, const char *who);
// stb_sample_dirconc behind its checks: every launch on st, the one wait, *info
int stb_dc_run(const uint32_t *d_cnt, uint64_t rows, unsigned cols, unsigned stride, unsigned flags, const double *d_w, double w0,
               double s, double shape, double scale, uint32_t *d_m, uint32_t *d_M, uint64_t seed, uint64_t sweep, hipStream_t st,
               stb_dirconc_info_t *info, const char *who);

#endif
