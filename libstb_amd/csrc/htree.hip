// htree.hip -- base weights on a tree of nested groups, drawn on the device (include/stb_hip.h, stb_sample_htree; DESIGN.md
// section 6).  hgroups.hip's two layers made L: level 1 cuts the restaurants into contiguous ranges, level l + 1 cuts the nodes
// of level l, the root sits above level L; node v of level l has h_v | h_par(v) ~ Dirichlet(alpha_l h_par(v)).  One step:
//     up, l = 1 .. L      m_vk | c, alpha_l, h_par(v)   Antoniak (hg_cell.h) with w = alpha_l h_par(v),k on the stored row of
//                         level l + 1 (the root at l = L); the parent's counts are the integer sums of its children's m
//     r' | s              Dirichlet(gamma_k + s_k), s the sums handed up by level L
//     alpha'_l            Teh's auxiliaries for all levels in one hyperb step: every node a "restaurant" (N = C_v, T = M_v),
//                         a range a level
//     down, l = L .. 1    h'_v ~ Dirichlet(alpha'_l h'_par(v),k + c_vk), the parent's new row
// stb_ht_sample is that step for every caller, stb_sample_hgroups (L = 1) included.  It queues hgroups.hip's kernels through
// hgroups.h's entries -- k_hg_count, a k_hg_aux a level, the root's k_hg_rows, a k_hg_rows a level, k_hg_scatter -- and
// between them
//   k_ht_prep     every node's C as hyperb's N (and the 2^32 check), its level's alpha, the L ranges
//   k_ht_finish   error word, the L concentrations, the totals of every level to pinned words
// and hyperb's three launches; the call waits once.  No kernel waits for another workgroup.  The streams, the FP64
// associations and why no bit depends on the launch geometry are stated in hgroups.hip's header.

#include <cmath>
#include <cstring>
#include <vector>

#include "stb_common.h"
#include "hyperb.h"
#include "htree.h"
#include "hg_cell.h"  // HG_SALT_A

struct ht_levels {  // by value to k_ht_prep and k_ht_finish
  double alpha[STB_HT_MAXL];
  uint64_t noff[STB_HT_MAXL + 1];  // level l's nodes are noff[l] .. noff[l+1] - 1 of the concatenation
  unsigned L;
};

__global__ __launch_bounds__(256) void k_ht_prep(ht_levels lv, const unsigned long long *Cv, uint32_t *N32, double *al, uint64_t *loff,
                                                 unsigned *ctl) {
  const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (v <= lv.L) loff[v] = lv.noff[v];
  if (v >= lv.noff[lv.L]) return;
  unsigned l = 0;
  while (l + 1 < lv.L && lv.noff[l + 1] <= v) l++;
  const unsigned long long C = Cv[v];
  if (C > 0xffffffffull) __hip_atomic_fetch_or(&ctl[0], HG_ERR_TOTAL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  N32[v] = (uint32_t)C;
  al[v] = lv.alpha[l];
}

// one workgroup: every level's totals, then the words the host waits for: [0] the error word, [1 + l] alpha'_l's bits,
// [1 + MAXL + l] sum C_v, [1 + 2 MAXL + l] sum M_v
__global__ __launch_bounds__(256) void k_ht_finish(ht_levels lv, const unsigned long long *Cv, const uint32_t *Mv, const double *al,
                                                   const unsigned *ctl, unsigned long long *host_out) {
  __shared__ unsigned long long s_c[STB_HT_MAXL], s_m[STB_HT_MAXL];
  if (threadIdx.x < STB_HT_MAXL) s_c[threadIdx.x] = s_m[threadIdx.x] = 0;
  __syncthreads();
  for (unsigned l = 0; l < lv.L; l++) {
    unsigned long long cs = 0, ms = 0;
    for (uint64_t v = lv.noff[l] + threadIdx.x; v < lv.noff[l + 1]; v += 256) {
      cs += Cv[v];
      ms += Mv[v];
    }
    if (cs) atomicAdd(&s_c[l], cs);
    if (ms) atomicAdd(&s_m[l], ms);
  }
  __syncthreads();
  if (threadIdx.x == 0) host_out[0] = ctl[0];
  if (threadIdx.x < lv.L) {
    const unsigned l = threadIdx.x;
    host_out[1 + l] = (unsigned long long)__double_as_longlong(al[lv.noff[l]]);
    host_out[1 + STB_HT_MAXL + l] = s_c[l];
    host_out[1 + 2 * STB_HT_MAXL + l] = s_m[l];
  }
}

// ------------------------------------------------------------------------------------------------
// host side.  The scratch comes from the buffer cache and goes back behind the call's one wait.

struct ht_scratch {
  void *d = nullptr, *h = nullptr, *h_dev = nullptr, *stage = nullptr;
  hipStream_t st = nullptr;
  bool queued = false;  // work that uses the buffers may be on st: wait before the cache hands them on
  ~ht_scratch() {
    if (queued) (void)hipStreamSynchronize(st);
    if (d) stb_pool_free(d);
    if (h) stb_pool_free(h);
    if (stage) stb_pool_free(stage);
  }
};

static size_t ht_up(size_t x) { return (x + 255) & ~(size_t)255; }

void stb_ht_clear(stb_htree_info_t *info) {
  if (!info) return;
  for (int l = 0; l < STB_HT_MAXL; l++) {
    info->alpha[l] = NAN;
    info->tables[l] = info->aux_tables[l] = 0;
  }
  info->error_word = info->reserved = 0;
}

int stb_ht_check_opts(const stb_htree_opts_t *opts, const double *alpha, unsigned Kmax, const char *who) {
  if (!opts) return stb_fail("%s: opts is required", who);
  if (opts->levels < 1 || opts->levels > STB_HT_MAXL) return stb_fail("%s: levels=%d (1 to STB_HT_MAXL = %d)", who, opts->levels, STB_HT_MAXL);
  return stb_hg_check_common(opts->flags, alpha, opts->levels, true, opts->gamma0, opts->gamma_host, opts->shape, opts->scale, Kmax, who);
}

int stb_ht_check_ranges(int level, int G, const uint64_t *off, uint64_t below, const char *who) {
  if (off[0] != 0 || off[G] != below)
    return stb_fail("%s: level %d's ranges run from %llu to %llu; the level below has %llu", who, level + 1,
                    (unsigned long long)off[0], (unsigned long long)off[G], (unsigned long long)below);
  for (int g = 0; g < G; g++)
    if (off[g] > off[g + 1]) return stb_fail("%s: level %d: off[%d] > off[%d]", who, level + 1, g, g + 1);
  return 0;
}

int stb_ht_sample(int I, const uint64_t *d_koff, const uint16_t *d_t, unsigned Kmax, const int *G_host, const uint64_t *const *d_off,
                  const stb_htree_opts_t *opts, const double *alpha, double *d_root, double *const *d_hnode, double *d_h,
                  uint32_t *const *d_c, uint32_t *const *d_m, uint64_t seed, uint64_t sweep, hipStream_t st, stb_htree_info_t *info,
                  stb_hg_geom geo, const char *who, bool *touched) {
  stb_ht_clear(info);
  const unsigned L = (unsigned)opts->levels, nw = geo.nw;
  const bool keep_root = (opts->flags & STB_HT_KEEP_ROOT) != 0, draw_alpha = (opts->flags & STB_HT_SAMPLE_ALPHA) != 0;
  const bool gvec = !keep_root && opts->gamma_host;
  ht_levels lv;
  memset(&lv, 0, sizeof lv);
  lv.L = L;
  for (unsigned l = 0; l < L; l++) {
    lv.alpha[l] = alpha[l];
    lv.noff[l + 1] = lv.noff[l] + (uint64_t)G_host[l];
  }
  const size_t NV = (size_t)lv.noff[L];
  // scratch.  Zeroed: ctl (256 bytes), s[Kmax], Cv[NV], Mv[NV] -- and every level's c.  Then N32[NV], al[NV], the L ranges,
  // hyperb's L[NV] and Y[NV], gamma[Kmax], and whichever of c and level 1's rows the caller did not give
  const size_t o_s = 256, o_Cv = o_s + ht_up(8 * (size_t)Kmax), o_Mv = o_Cv + ht_up(8 * NV), o_N = o_Mv + ht_up(4 * NV),
               o_al = o_N + ht_up(4 * NV), o_lo = o_al + ht_up(8 * NV), o_L = o_lo + 256,
               o_Y = o_L + (draw_alpha ? ht_up(8 * NV) : 0), o_gam = o_Y + (draw_alpha ? ht_up(4 * NV) : 0);
  size_t bytes = o_gam + (gvec ? ht_up(8 * (size_t)Kmax) : 0);
  size_t o_c[STB_HT_MAXL];
  for (unsigned l = 0; l < L; l++) {
    const size_t cells = (size_t)G_host[l] * Kmax;
    o_c[l] = bytes;
    if (!(d_c && d_c[l])) bytes += ht_up(4 * cells);
  }
  const size_t o_h1 = bytes;
  if (!d_hnode[0]) bytes += ht_up(8 * (size_t)G_host[0] * Kmax);
  ht_scratch sc;
  sc.st = st;
  if (stb_pool_malloc(&sc.d, bytes) != hipSuccess || stb_pool_malloc(&sc.h, 256, 1) != hipSuccess ||
      hipHostGetDevicePointer(&sc.h_dev, sc.h, 0) != hipSuccess ||
      (gvec && stb_pool_malloc(&sc.stage, 8 * (size_t)Kmax, 1) != hipSuccess))
    return stb_fail("%s: out of memory for %zu bytes of scratch", who, bytes);
  char *d = (char *)sc.d;
  unsigned *ctl = (unsigned *)d;
  unsigned long long *s = (unsigned long long *)(d + o_s), *Cv = (unsigned long long *)(d + o_Cv);
  uint32_t *Mv = (uint32_t *)(d + o_Mv), *N32 = (uint32_t *)(d + o_N), *Y = (uint32_t *)(d + o_Y);
  double *al = (double *)(d + o_al), *Lh = (double *)(d + o_L), *d_gam = gvec ? (double *)(d + o_gam) : nullptr;
  uint64_t *loff = (uint64_t *)(d + o_lo);
  uint32_t *c[STB_HT_MAXL], *m[STB_HT_MAXL];
  for (unsigned l = 0; l < L; l++) {
    c[l] = d_c && d_c[l] ? d_c[l] : (uint32_t *)(d + o_c[l]);
    m[l] = d_m && d_m[l] ? d_m[l] : nullptr;  // (m is handed up as it is drawn: nobody else reads it)
  }
  double *h1 = d_hnode[0] ? d_hnode[0] : (double *)(d + o_h1);
  volatile unsigned long long *h_out = (volatile unsigned long long *)sc.h;
  h_out[0] = 0xffffffffull;
  sc.queued = true;
  HIPCHK(hipMemsetAsync(d, 0, o_N, st));
  for (unsigned l = 0; l < L; l++) HIPCHK(hipMemsetAsync(c[l], 0, 4 * (size_t)G_host[l] * Kmax, st));
  if (gvec) {
    memcpy(sc.stage, opts->gamma_host, 8 * (size_t)Kmax);
    HIPCHK(hipMemcpyAsync(d_gam, sc.stage, 8 * (size_t)Kmax, hipMemcpyHostToDevice, st));
  }
  const uint64_t key = stb_mix64(seed + (sweep + 1) * STB_GAMMA);
  uint64_t keys[STB_HT_MAXL];
  for (unsigned l = 0; l < L; l++) keys[l] = l == 0 ? key : stb_mix64(key ^ (HT_SALT_L + (uint64_t)(l + 1)));
  // level l's parents: the nodes of level l + 1 and their stored rows, or, above the top level, the root alone
  auto Gp = [&](unsigned l) { return l + 1 == L ? (uint64_t)1 : (uint64_t)G_host[l + 1]; };
  auto poff = [&](unsigned l) { return l + 1 == L ? (const uint64_t *)nullptr : d_off[l + 1]; };
  auto base = [&](unsigned l) { return l + 1 == L ? (const double *)d_root : (const double *)d_hnode[l + 1]; };
  if (stb_hg_count_queue(I, d_koff, d_t, Kmax, G_host[0], d_off[0], c[0], Cv, nw, st)) return 1;
  for (unsigned l = 0; l < L; l++) {  // up
    const bool top = l + 1 == L;
    if (stb_hg_aux_queue(Kmax, (uint64_t)G_host[l], c[l], Gp(l), poff(l), base(l), alpha[l], keys[l], geo, m[l], Mv + lv.noff[l],
                         top ? nullptr : c[l + 1], top ? nullptr : Cv + lv.noff[l + 1], s, st))
      return 1;
  }
  if (touched) *touched = true;
  if (!keep_root && stb_hg_root_queue(Kmax, s, d_gam, opts->gamma0, key, d_root, ctl, nw, st)) return 1;
  STB_LAUNCH(k_ht_prep, dim3((unsigned)((NV + 256) / 256)), dim3(256), st, lv, (const unsigned long long *)Cv, N32, al, loff, ctl);
  if (draw_alpha && stb_hb_bgroups_queue(0.0, opts->shape, opts->scale, (int)NV, N32, Mv, (int)L, loff, al, Lh, Y, seed ^ HG_SALT_A,
                                         sweep, st, who))
    return 1;
  for (unsigned l = L; l-- > 0;)  // down
    if (stb_hg_rows_queue((uint64_t)G_host[l], Kmax, c[l], Gp(l), poff(l), base(l), al + lv.noff[l], keys[l], l == 0 ? h1 : d_hnode[l],
                          ctl, nw, st))
      return 1;
  if (stb_hg_scatter_queue(I, d_koff, Kmax, G_host[0], d_off[0], h1, d_h, nw, st)) return 1;
  STB_LAUNCH(k_ht_finish, dim3(1), dim3(256), st, lv, (const unsigned long long *)Cv, (const uint32_t *)Mv, (const double *)al,
             (const unsigned *)ctl, (unsigned long long *)sc.h_dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  sc.queued = false;
  const unsigned err = (unsigned)h_out[0];
  if (info) {
    for (unsigned l = 0; l < L; l++) {
      const unsigned long long bits = h_out[1 + l];
      memcpy(&info->alpha[l], &bits, sizeof(double));
      info->tables[l] = h_out[1 + STB_HT_MAXL + l];
      info->aux_tables[l] = h_out[1 + 2 * STB_HT_MAXL + l];
    }
    info->error_word = err;
  }
  if (err)
    return stb_fail("%s: failed, error word 0x%x (1: a Gamma draw was not accepted within %d attempts; 2: a normaliser is not "
                    "positive and finite; 4: a shape alpha base_k + c_k (base the row above, the root at the top) is negative, "
                    "infinite or NaN; 8: a group or node has more than 2^32 - 1 tables) (seed=%llu, sweep=%llu); the outputs are "
                    "undefined",
                    who, err, HQ_CAP, (unsigned long long)seed, (unsigned long long)sweep);
  if (draw_alpha) {
    stb_bgroups_info_t bi;
    if (stb_hb_bgroups_answer((int)L, &bi, who)) return 1;
    if (bi.kept_groups) return stb_fail("%s: a concentration's draw is not a positive finite double; the outputs are undefined", who);
  }
  return 0;
}

// ---- the raw layer ------------------------------------------------------------------------------------------------

extern "C" int stb_sample_htree(int I, const uint64_t *d_koff, const uint16_t *d_t, unsigned Kmax, const int *G_host,
                                const uint64_t *const *d_off, const stb_htree_opts_t *opts, double *d_root, double *const *d_hnode,
                                double *d_h, uint32_t *const *d_c, uint32_t *const *d_m, uint64_t seed, uint64_t sweep, void *stream,
                                stb_htree_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_sample_htree";
  stb_ht_clear(info);
  if (!d_koff || !d_t || !d_root || !d_h || !G_host || !d_off || !d_hnode)
    return stb_fail("%s: d_koff, d_t, G_host, d_off, d_root, d_hnode and d_h are required", who);
  if (I < 1) return stb_fail("%s: I=%d (must be >= 1)", who, I);
  if (stb_ht_check_opts(opts, opts ? opts->alpha : nullptr, Kmax, who)) return 1;
  const int L = opts->levels;
  for (int l = 0; l < L; l++) {
    if (G_host[l] < 1) return stb_fail("%s: G[%d]=%d (must be >= 1)", who, l, G_host[l]);
    if (!d_off[l]) return stb_fail("%s: d_off[%d] is required", who, l);
    if (l >= 1 && !d_hnode[l]) return stb_fail("%s: d_hnode[%d] is required (the rows of level %d)", who, l, l + 1);
  }
  if (stb_device_count() < 1) return stb_no_device(who);
  hipStream_t st = (hipStream_t)stream;
  // the ranges steer stores: they are read back and checked before anything is queued
  std::vector<std::vector<uint64_t>> off((size_t)L);
  for (int l = 0; l < L; l++) {
    off[l].resize((size_t)G_host[l] + 1);
    HIPCHK(hipMemcpyAsync(off[l].data(), d_off[l], 8 * ((size_t)G_host[l] + 1), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  for (int l = 0; l < L; l++)
    if (stb_ht_check_ranges(l, G_host[l], off[l].data(), l == 0 ? (uint64_t)I : (uint64_t)G_host[l - 1], who)) return 1;
  return stb_ht_sample(I, d_koff, d_t, Kmax, G_host, d_off, opts, opts->alpha, d_root, d_hnode, d_h, d_c, d_m, seed, sweep, st, info,
                       stb_hg_geom_env("STB_HTREE_WAVES", "STB_HTREE_FORM"), who, nullptr);
}
