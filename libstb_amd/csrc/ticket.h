/* ticket.h -- private: what the ticket reductions share.  A ticket reduction leaves block sums in global memory, every
 * workgroup takes a ticket when it is through, and the last one to take one adds the block sums; nobody waits.
 *
 *   geometry         stb_ticket_geom, stb_tg_cps, STB_TG_*: k_logq (hyperq.hip), k_joint_terms (hyperj.hip), k_logjoint
 *                    (logjoint.hip), k_heldout_sum (predict.hip) and k_seat_sum (seat.hip; both k_logjoint's geometry).
 *                    The launch sites compute grid, workgroup size and the room for block sums from stb_ticket_geom, and
 *                    stb_reduce_geometry (include/stb_hip.h) answers from the same function: what the query says is
 *                    what is launched.
 *   stb_wave_sum     the 64-lane shuffle tree of a double or a 64-bit count.  Moved out to wave.h, which this header
 *                    includes (MEASUREMENTS O6); its callers are still listed here: k_logjoint, k_predict, k_heldout_sum,
 *                    k_seat and k_seat_sum, the k_dm_* (dirmult.hip), k_dc_totals and k_dc_totals_rows (dirconc.hip), k_hg_count (hgroups.hip).  The
 *                    same tree stays written out in k_logq, k_sum_u32, k_joint_terms, k_hb_group_wg (hyperb.hip) and
 *                    k_eval_tail (groups.hip): there the call compiles to other code than the loop (MEASUREMENTS O3)
 *   stb_ticket_last  the ticket: the five kernels above and k_dm_rows, k_dm_rows_split, k_dm_cols (dirmult.hip)
 *   stb_tset         what a calling thread keeps for a ticket kernel: hq (hyperq.hip), lj (logjoint.hip), pr (predict.hip),
 *                    sq (seat.hip); hj (hyperj.hip) and hb (hyperb.hip) hold one next to what is theirs alone
 */
#ifndef STB_TICKET_H
#define STB_TICKET_H
#include "stb_common.h"
#include "wave.h"

#define STB_TG_BLOCK 256u        // restaurants of a block sum: HQ_CHUNK, HJ_CHUNK, LJ_BLOCK and PR_BLOCK are defined as this
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
    nw = stb_env_waves(which == STB_GEOM_LOGQ ? "STB_HYPERQ_WAVES" : which == STB_GEOM_JOINT_TERMS ? "STB_HYPERJ_WAVES" : "STB_LOGJOINT_WAVES", 0);
    if (!nw)
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

// ------------------------------------------------------------------------------------------------
// device

// the ticket, called by all threads of every workgroup (ngroups of them): every store of the workgroup is published by
// an agent-scope release ahead of it; true in the last workgroup to take one, which has acquired what the others published
__device__ __forceinline__ bool stb_ticket_last(unsigned *ticket, unsigned ngroups, unsigned *s_last) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    *s_last = __hip_atomic_fetch_add(&ticket[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ngroups - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (!*s_last) return false;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  return true;
}

// ------------------------------------------------------------------------------------------------
// host: what a calling thread keeps for one family of ticket kernels, on one device.  One set per family and thread (a
// family may queue a launch and return: a set shared with another family could have its words zeroed under that launch).

struct stb_tset {
  int dev = -1;
  unsigned *d_ctl = nullptr;                      // 256 bytes: the ticket, the kernel's counters and error word
  double *h_out = nullptr, *h_out_dev = nullptr;  // 256 pinned bytes the kernel answers in, and their device alias
  void *d_buf = nullptr;                          // the buffer that grows: block sums (hyperb.hip: its y)
  size_t cap = 0;                                 // elements d_buf holds
};

static inline void stb_tset_drop(stb_tset &s) {
  if (s.dev < 0) return;
  stb_device_scope dev(s.dev);
  if (s.d_buf) stb_pool_free(s.d_buf);
  if (s.d_ctl) stb_pool_free(s.d_ctl);
  if (s.h_out) stb_pool_free(s.h_out);
  s = stb_tset();
}

// the set on the thread's current device (one made for another device is dropped): the control words, and with `words`
// the pinned result words
static inline int stb_tset_ready(stb_tset &s, const char *who, bool words = true) {
  int dev = -1;
  HIPCHK(hipGetDevice(&dev));
  if (s.dev >= 0 && s.dev != dev) stb_tset_drop(s);
  if (s.dev >= 0) return 0;
  s.dev = dev;
  if (stb_pool_malloc((void **)&s.d_ctl, 256) != hipSuccess ||
      (words && (stb_pool_malloc((void **)&s.h_out, 256, 1) != hipSuccess ||
                 hipHostGetDevicePointer((void **)&s.h_out_dev, s.h_out, 0) != hipSuccess))) {
    stb_tset_drop(s);
    return stb_fail("%s: out of memory for the control and result words", who);
  }
  return 0;
}

// room for `need` elements of `elem` bytes in d_buf; a new buffer holds `floor` elements at least.  Nothing the old
// buffer held is kept
static inline int stb_tset_room(stb_tset &s, size_t need, size_t floor, size_t elem, const char *who) {
  if (need <= s.cap) return 0;
  if (s.d_buf) stb_pool_free(s.d_buf);
  s.d_buf = nullptr;
  s.cap = 0;
  const size_t want = need < floor ? floor : need;
  if (stb_pool_malloc(&s.d_buf, elem * want) != hipSuccess)
    return stb_fail("%s: out of device memory for %zu elements of %zu bytes", who, want, elem);
  s.cap = want;
  return 0;
}
#endif
