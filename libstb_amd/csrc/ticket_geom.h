/* ticket_geom.h -- private: the launch geometry of the three ticket reductions (k_logq of hyperq.hip, k_joint_terms of
 * hyperj.hip, k_logjoint of logjoint.hip) in one place.  The three launch sites compute grid, workgroup size and the
 * room for block sums from stb_ticket_geom, and stb_reduce_geometry (include/stb_hip.h) answers from the same function:
 * what the query says is what is launched.  No device work beyond stb_tg_cps, which the kernels share. */
#ifndef STB_TICKET_GEOM_H
#define STB_TICKET_GEOM_H
#include "stb_common.h"

#define STB_TG_BLOCK 256u        // restaurants of a block sum: HQ_CHUNK, HJ_CHUNK and LJ_BLOCK are defined as this
#define STB_TG_CAP0_BLOCKS 4096u // block sums k_logq's and k_logjoint's first buffer holds
#define STB_TG_CAP0_HJ 65536u    // doubles k_joint_terms' first buffer holds

// blocks a workgroup of nthr threads takes per step in k_logq and k_joint_terms (eight waves: two): the kernels and
// stb_ticket_geom both call this
__host__ __device__ static inline unsigned stb_tg_cps(unsigned nthr) { return nthr > STB_TG_BLOCK ? nthr / STB_TG_BLOCK : 1u; }

struct stb_tgeom {
  unsigned nblk;       // blocks of 256 restaurants
  unsigned waves;      // waves a workgroup
  unsigned cps;        // blocks a workgroup takes per step
  unsigned steps;      // steps in all: a workgroup takes step blockIdx.x, + gridDim.x, ...
  unsigned gx, gy;     // the grid
  size_t need, cap0;   // what the call needs of `partial` and what the first allocation holds (block sums; doubles for
                       // k_joint_terms, whose block sum is D J doubles)
};

// waves = 0: the kernel's environment variable, else its default.  I >= 1; D, J are read for STB_GEOM_JOINT_TERMS alone.
static inline int stb_ticket_geom(int which, uint64_t I, int D, int J, int waves, stb_tgeom *g) {
  if (which != STB_GEOM_LOGQ && which != STB_GEOM_JOINT_TERMS && which != STB_GEOM_LOGJOINT) return 1;
  if (!(waves == 0 || waves == 1 || waves == 2 || waves == 4 || waves == 8) || I < 1) return 1;
  const int cus = stb_cu_count();
  unsigned want = 4u * (unsigned)(cus > 0 ? cus : 1);
  g->nblk = (unsigned)((I + STB_TG_BLOCK - 1) / STB_TG_BLOCK);
  int nw = waves;
  if (!nw) {
    nw = stb_env_int(which == STB_GEOM_LOGQ ? "STB_HYPERQ_WAVES" : which == STB_GEOM_JOINT_TERMS ? "STB_HYPERJ_WAVES" : "STB_LOGJOINT_WAVES", 0);
    if (!(nw == 1 || nw == 2 || nw == 4 || nw == 8))
      nw = which == STB_GEOM_LOGJOINT && g->nblk < 2u * (unsigned)(cus > 0 ? cus : 1) ? 8 : 4;
  }
  g->waves = (unsigned)nw;
  // k_logq and k_joint_terms: a workgroup of eight waves takes 512 restaurants a step; k_logjoint always one block
  g->cps = which != STB_GEOM_LOGJOINT ? stb_tg_cps(64u * (unsigned)nw) : 1u;
  g->steps = (g->nblk + g->cps - 1) / g->cps;
  g->gx = g->steps < want ? g->steps : want;
  g->gy = 1;
  g->need = g->nblk;
  g->cap0 = STB_TG_CAP0_BLOCKS;
  if (which == STB_GEOM_JOINT_TERMS) {  // what x leaves of the chip goes to j
    if (D < 1 || J < 1) return 1;
    g->gy = want / g->gx;
    if (g->gy < 1) g->gy = 1;
    if (g->gy > (unsigned)J) g->gy = (unsigned)J;
    g->need = (size_t)g->nblk * (size_t)D * (size_t)J;
    g->cap0 = STB_TG_CAP0_HJ;
  }
  return 0;
}
#endif
