// dirmult.h -- private: what the object layer (tindic.hip) needs of dirmult.hip beyond include/stb_hip.h.
#ifndef STB_DIRMULT_H
#define STB_DIRMULT_H

#include "stb_common.h"
#include "../../include/stb_hip.h"

// the checks stb_dirmult_logml makes before anything is queued (0, or 1 with stb_last_error() set)
int stb_dm_check(const uint32_t *d_cnt, unsigned cols, unsigned stride, unsigned flags, const double *d_w, double w0, double scale,
                 const double *d_scale, const double *total_host, const char *who);
// stb_dirmult_logml behind its checks: the launches on st and the one wait
int stb_dm_run(const uint32_t *d_cnt, uint64_t rows, unsigned cols, unsigned stride, unsigned flags, const double *d_w, double w0,
               double scale, const double *d_scale, double *d_each, double *total_host, stb_dirmult_info_t *info, hipStream_t st,
               const char *who);
// log p(r | gamma) of a root of K <= STB_TD_MAXK cells (d_root NULL: 1 / K each; d_gamma NULL: gamma0 each), queued on st:
// out_dev[0] the value, out_dev[1] (as uint64) the cells with r_k = 0, which are left out.  No wait
int stb_dm_root_queue(unsigned K, const double *d_root, const double *d_gamma, double gamma0, double *out_dev, hipStream_t st);

#endif
