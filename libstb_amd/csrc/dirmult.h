// dirmult.h -- private: what the object layer (tindic_obj.hip) needs of dirmult.hip beyond include/stb_hip.h.
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
// k_dm_weights alone with scale 1, queued on st, for a caller that needs the weights' total in dirmult's association
// (dirconc.hip): ctl is 256 bytes the caller zeroed on st.  Behind the launch its u32 word STB_DM_CTL_ERR holds the error
// bits (1: a weight is negative, NaN or infinite; 2: the total is not positive and finite) and its doubles STB_DM_CTL_W,
// STB_DM_CTL_W + 1 the total W and lgamma(W).  No wait
#define STB_DM_CTL_ERR 16
#define STB_DM_CTL_W 16
int stb_dm_weights_queue(const double *d_w, uint64_t ncat, double w0, unsigned *ctl, hipStream_t st);

#endif
