// htree.hip -- base weights on a tree of nested groups, drawn on the device (include/stb_hip.h, stb_sample_htree; DESIGN.md
// section 6).  hgroups.hip's two layers made L: level 1 cuts the restaurants into contiguous ranges, level l + 1 cuts the nodes
// of level l, the root sits above level L; node v of level l has h_v | h_par(v) ~ Dirichlet(alpha_l h_par(v)).  One step:
//     up, l = 1 .. L      m_vk | c, alpha_l, h_par(v)   Antoniak (hg_cell.h) with w = alpha_l h_par(v),k on the stored row of
//                         level l + 1 (the root at l = L); the parent's counts are the integer sums of its children's m
//     r' | s              Dirichlet(gamma_k + s_k), s the sums handed up by level L
//     alpha'_l            Teh's auxiliaries for all levels in one hyperb step: every node a "restaurant" (N = C_v, T = M_v),
//                         a range a level
//     down, l = L .. 1    h'_v ~ Dirichlet(alpha'_l h'_par(v),k + c_vk), the parent's new row
//
//   k_hg_count    (hgroups.hip) level 1's c and C
//   k_ht_aux      a level's m, M_v, and its parents' c and C: lanes along k, a wave a run of successive rows; the parent's
//                 column sums stay in registers while the parent does not change (integers: atomics)
//   k_hg_rows     (hgroups.hip) the root's row
//   k_ht_prep     every node's C as hyperb's N (and the 2^32 check), its level's alpha, the L ranges
//   k_ht_rows     a Dirichlet row a workgroup, its base row the parent's
//   k_hg_scatter  (hgroups.hip) level 1's rows to the pairs
//   k_ht_finish   error word, the L concentrations, the totals of every level to pinned words
// All are queued back to back, hyperb's three launches among them; the call waits once.  No kernel waits for another
// workgroup.
//
// Streams: key = mix(seed + (sweep+1) gamma); key_1 = key, key_l = mix(key ^ (HT_SALT_L + l)) for l >= 2.  Cell e = v Kmax + k
// of level l owns mix(key_l + (e+1) gamma) and its Bernoulli draws that key's ^ HG_SALT_Y substream; the root and the
// concentration as hgroups.hip's.  Associations are hgroups.hip's (FP64, no contraction): w = alpha_l base_k one product, a
// row's shapes alpha'_l base'_k + (double)c.  With L = 1 every launch computes what stb_sample_hgroups' does.  Counts and m are
// integers, so no bit depends on STB_HTREE_WAVES = 1, 2, 4 or 8 or on STB_HTREE_FORM = lane | wave.

#include <cmath>
#include <cstring>
#include <vector>

#include "stb_common.h"
#include "gamma_dev.h"
#include "hyperb.h"
#include "hgroups.h"
#include "htree.h"
#include "hg_cell.h"

#pragma clang fp contract(off)

#define HT_MAXTHREADS 512
#define HT_ERR_CAP 1u
#define HT_ERR_Z 2u
#define HT_ERR_SHAPE 4u
#define HT_ERR_TOTAL 8u

struct ht_levels {  // by value to k_ht_prep and k_ht_finish
  double alpha[STB_HT_MAXL];
  uint64_t noff[STB_HT_MAXL + 1];  // level l's nodes are noff[l] .. noff[l+1] - 1 of the concatenation
  unsigned L;
};

// the last range that starts at or before i (empty ranges in front of it start there too)
__device__ __forceinline__ uint64_t ht_range_of(const uint64_t *off, uint64_t G, uint64_t i) {
  uint64_t lo = 0, hi = G;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// what a wave holds of parent `par`: its lanes' column sums, and (lane 0) the rows' totals
__device__ __forceinline__ void ht_flush(unsigned long long &acc, unsigned long long &tot, uint64_t par, unsigned Kmax, unsigned k,
                                         bool live, unsigned lane, uint32_t *cpar, unsigned long long *Cpar, unsigned long long *s) {
  if (live && acc) {
    if (cpar) atomicAdd(&cpar[par * Kmax + k], (unsigned)acc);  // (a wrap shows in C_par > 2^32 - 1: error 8)
    else atomicAdd(&s[k], acc);
  }
  acc = 0;
  if (lane == 0 && tot && Cpar) atomicAdd(&Cpar[par], tot);
  tot = 0;
}

// workgroup (x, y): the columns 64 x .. 64 x + 63.  The G rows, each cut into `parts` (hg_cell.h), are dealt to the grid's
// waves in runs of successive (row, part).  poff[Gp + 1] cuts the rows into their parents' ranges (null: one parent, row 0 of
// base).  The parents' counts go to cpar[Gp Kmax] and Cpar[Gp], or, above the top level, to s[Kmax] (cpar and Cpar null).
// m may be null; with parts > 1 it arrives zeroed
__global__ __launch_bounds__(HT_MAXTHREADS) void k_ht_aux(unsigned Kmax, uint64_t G, const uint32_t *c, uint64_t Gp, const uint64_t *poff,
                                                          const double *base, double alpha, uint64_t key, unsigned twave, unsigned parts,
                                                          uint32_t *m, uint32_t *Mv, uint32_t *cpar, unsigned long long *Cpar,
                                                          unsigned long long *s) {
  const unsigned lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (what follows from it stays in scalar registers)
  const unsigned k = blockIdx.x * 64 + lane;
  const bool live = k < Kmax;  // (no lane leaves: the wave's shuffles need them all)
  const uint64_t total = G * parts, waves = (uint64_t)gridDim.y * nw, run = (total + waves - 1) / waves;
  const uint64_t q0 = ((uint64_t)blockIdx.y * nw + wave) * run;
  if (q0 >= total) return;  // (the whole wave)
  const uint64_t q1 = q0 + run < total ? q0 + run : total;
  uint64_t par = poff ? ht_range_of(poff, Gp, q0 / parts) : 0;
  unsigned long long acc = 0, tot = 0;
  for (uint64_t q = q0; q < q1; q++) {
    const uint64_t g = q / parts;
    const unsigned p = (unsigned)(q % parts);
    if (poff) {
      uint64_t pn = par;
      while (pn + 1 < Gp && poff[pn + 1] <= g) pn++;
      if (pn != par) {  // (uniform over the wave)
        ht_flush(acc, tot, par, Kmax, k, live, lane, cpar, Cpar, s);
        par = pn;
      }
    }
    const uint64_t e = g * Kmax + k;
    const unsigned cc = live ? c[e] : 0u;
    const double w = live ? alpha * base[par * Kmax + k] : 1.0;
    const uint64_t ky = stb_mix64(stb_mix64(key + (e + 1) * STB_GAMMA) ^ HG_SALT_Y);
    const unsigned mm = hg_cell(cc, w, ky, p, parts, twave, lane);
    if (live && m) {
      if (parts == 1) m[e] = mm;
      else if (mm) atomicAdd(&m[e], mm);
    }
    acc += mm;
    unsigned row = mm;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) row += __shfl_down(row, off, 64);
    if (lane == 0 && row) atomicAdd(&Mv[g], row);
    tot += row;  // (lane 0's is the row's)
  }
  ht_flush(acc, tot, par, Kmax, k, live, lane, cpar, Cpar, s);
}

__global__ __launch_bounds__(256) void k_ht_prep(ht_levels lv, const unsigned long long *Cv, uint32_t *N32, double *al, uint64_t *loff,
                                                 unsigned *ctl) {
  const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (v <= lv.L) loff[v] = lv.noff[v];
  if (v >= lv.noff[lv.L]) return;
  unsigned l = 0;
  while (l + 1 < lv.L && lv.noff[l + 1] <= v) l++;
  const unsigned long long C = Cv[v];
  if (C > 0xffffffffull) __hip_atomic_fetch_or(&ctl[0], HT_ERR_TOTAL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  N32[v] = (uint32_t)C;
  al[v] = lv.alpha[l];
}

// k_hg_rows with a base row per output row: a workgroup a row (rows r = blockIdx.x, + gridDim.x, ...), its threads strided
// over k: shape_k = f base[par(r) Kmax + k] + (double)cnt[r Kmax + k], f = *factor; par(r) from poff[Gp + 1] (null: row 0);
// cell e = r Kmax + k
__global__ __launch_bounds__(HT_MAXTHREADS) void k_ht_rows(uint64_t rows, unsigned Kmax, const uint32_t *cnt, uint64_t Gp,
                                                           const uint64_t *poff, const double *base, const double *factor, uint64_t key,
                                                           double *out, unsigned *ctl) {
  __shared__ double sv[STB_TD_MAXK];
  __shared__ double s_max[HT_MAXTHREADS / 64];
  __shared__ double s_Z;
  const unsigned nthr = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
  const double f = *factor;
  unsigned err = 0;
  for (uint64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    const double *brow = base + (poff ? ht_range_of(poff, Gp, r) : 0) * Kmax;
    bool bad = false;
    double mx = -INFINITY;
    for (unsigned k = tid; k < Kmax; k += nthr) {
      const uint64_t e = r * Kmax + k;
      const double shape = f * brow[k] + (double)cnt[e];
      double lg = NAN;
      if (shape > 0.0 && isfinite(shape)) {
        const uint64_t ke = stb_mix64(key + (e + 1) * STB_GAMMA);
        uint64_t j = 0;
        lg = hq_log_gamma(shape, ke, j, bad);
      } else {
        err |= HT_ERR_SHAPE;
      }
      sv[k] = lg;
      if (lg > mx) mx = lg;  // (a NaN is never greater)
    }
    if (bad) err |= HT_ERR_CAP;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double o = __shfl_xor(mx, off, 64);
      mx = o > mx ? o : mx;
    }
    if (lane == 0) s_max[wave] = mx;
    __syncthreads();
    double M = s_max[0];
    for (unsigned q = 1; q < nw; q++) M = s_max[q] > M ? s_max[q] : M;
    for (unsigned k = tid; k < Kmax; k += nthr) sv[k] = exp(sv[k] - M);
    __syncthreads();
    if (tid == 0) {
      double z = sv[0];
      for (unsigned k = 1; k < Kmax; k++) z = z + sv[k];
      s_Z = z;
      if (!(z > 0.0 && isfinite(z))) err |= HT_ERR_Z;
    }
    __syncthreads();
    const double Z = s_Z;
    for (unsigned k = tid; k < Kmax; k += nthr) out[r * Kmax + k] = sv[k] / Z;
    __syncthreads();  // (sv, s_max and s_Z are the next row's)
  }
  if (err) __hip_atomic_fetch_or(&ctl[0], err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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

static void ht_clear(stb_htree_info_t *info) {
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
  if (Kmax < 1 || Kmax > STB_TD_MAXK) return stb_fail("%s: Kmax=%u (1 to STB_TD_MAXK = %d)", who, Kmax, STB_TD_MAXK);
  if (opts->flags & ~(STB_HT_KEEP_ROOT | STB_HT_SAMPLE_ALPHA)) return stb_fail("%s: unknown flags 0x%x", who, opts->flags);
  if (!alpha) return stb_fail("%s: opts->alpha is required", who);
  for (int l = 0; l < opts->levels; l++)
    if (!(alpha[l] > 0.0) || !std::isfinite(alpha[l]))
      return stb_fail("%s: alpha[%d]=%g (must be > 0 and finite)", who, l, alpha[l]);
  if (!(opts->flags & STB_HT_KEEP_ROOT)) {
    if (opts->gamma_host) {
      for (unsigned k = 0; k < Kmax; k++)
        if (!(opts->gamma_host[k] > 0.0) || !std::isfinite(opts->gamma_host[k]))
          return stb_fail("%s: gamma[%u]=%g (must be > 0 and finite)", who, k, opts->gamma_host[k]);
    } else if (!(opts->gamma0 > 0.0) || !std::isfinite(opts->gamma0)) {
      return stb_fail("%s: gamma0=%g (must be > 0 and finite)", who, opts->gamma0);
    }
  }
  if (opts->flags & STB_HT_SAMPLE_ALPHA) {
    if (!(opts->shape > 0.0) || !std::isfinite(opts->shape))
      return stb_fail("%s: shape=%g (must be > 0 and finite)", who, opts->shape);
    if (!(opts->scale > 0.0) || !std::isfinite(opts->scale))
      return stb_fail("%s: scale=%g (must be > 0 and finite)", who, opts->scale);
  }
  return 0;
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
                  const char *who, bool *touched) {
  ht_clear(info);
  const unsigned L = (unsigned)opts->levels;
  const bool keep_root = (opts->flags & STB_HT_KEEP_ROOT) != 0, draw_alpha = (opts->flags & STB_HT_SAMPLE_ALPHA) != 0;
  const bool gvec = !keep_root && opts->gamma_host;
  int nwi = stb_env_int("STB_HTREE_WAVES", 4);
  const unsigned nw = nwi == 1 || nwi == 2 || nwi == 4 || nwi == 8 ? (unsigned)nwi : 4u;
  const char *form = getenv("STB_HTREE_FORM");
  const unsigned twave = form && !strcmp(form, "lane") ? 0xffffffffu : form && !strcmp(form, "wave") ? 0u : HG_TWAVE;
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
  const unsigned cus = (unsigned)(stb_cu_count() > 0 ? stb_cu_count() : 1);
  const unsigned cb = (Kmax + 63) / 64;
  const unsigned thr_row = 64u * nw < 64u * cb ? 64u * nw : 64u * cb;  // (no more waves than the row has columns for)
  const uint64_t cap_y = (uint64_t)8 * cus / cb + 1, fill = cap_y * nw, cap_rows = (uint64_t)32 * cus;
  if (stb_hg_count_queue(I, d_koff, d_t, Kmax, G_host[0], d_off[0], c[0], Cv, st)) return 1;
  for (unsigned l = 0; l < L; l++) {  // up
    const size_t Gs = (size_t)G_host[l];
    // few rows: each is cut into parts, so that the cells a wave takes keep about 8 waves a compute unit busy -- a high node
    // collects the auxiliary tables of a whole subtree in one cell
    const unsigned parts = twave != 0xffffffffu && Gs < fill ? (unsigned)((fill + Gs - 1) / Gs < 1024 ? (fill + Gs - 1) / Gs : 1024) : 1u;
    const uint64_t want_y = (Gs * parts + nw - 1) / nw;
    const unsigned gy = (unsigned)(want_y < cap_y ? want_y : cap_y);
    const bool top = l + 1 == L;
    if (parts > 1 && m[l]) HIPCHK(hipMemsetAsync(m[l], 0, 4 * Gs * Kmax, st));
    STB_LAUNCH(k_ht_aux, dim3(cb, gy), dim3(64 * nw), st, Kmax, (uint64_t)Gs, (const uint32_t *)c[l],
               top ? (uint64_t)1 : (uint64_t)G_host[l + 1], top ? (const uint64_t *)nullptr : d_off[l + 1],
               top ? (const double *)d_root : (const double *)d_hnode[l + 1], alpha[l], keys[l], twave, parts, m[l],
               Mv + lv.noff[l], top ? (uint32_t *)nullptr : c[l + 1], top ? (unsigned long long *)nullptr : Cv + lv.noff[l + 1], s);
  }
  if (touched) *touched = true;
  if (!keep_root && stb_hg_root_queue(Kmax, s, d_gam, opts->gamma0, key, d_root, ctl, nw, st)) return 1;
  STB_LAUNCH(k_ht_prep, dim3((unsigned)((NV + 256) / 256)), dim3(256), st, lv, (const unsigned long long *)Cv, N32, al, loff, ctl);
  if (draw_alpha && stb_hb_bgroups_queue(0.0, opts->shape, opts->scale, (int)NV, N32, Mv, (int)L, loff, al, Lh, Y, seed ^ HG_SALT_A,
                                         sweep, st, who))
    return 1;
  for (unsigned l = L; l-- > 0;) {  // down
    const size_t Gs = (size_t)G_host[l];
    const bool top = l + 1 == L;
    const unsigned gx = (unsigned)(Gs < cap_rows ? Gs : cap_rows);
    STB_LAUNCH(k_ht_rows, dim3(gx), dim3(thr_row), st, (uint64_t)Gs, Kmax, (const uint32_t *)c[l],
               top ? (uint64_t)1 : (uint64_t)G_host[l + 1], top ? (const uint64_t *)nullptr : d_off[l + 1],
               top ? (const double *)d_root : (const double *)d_hnode[l + 1], (const double *)(al + lv.noff[l]), keys[l],
               l == 0 ? h1 : d_hnode[l], ctl);
  }
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
                    "positive and finite; 4: a shape alpha h_k + c_vk is not positive and finite; 8: a node has more than "
                    "2^32 - 1 tables) (seed=%llu, sweep=%llu); the outputs are undefined",
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
  ht_clear(info);
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
  if (stb_device_count() < 1) return stb_fail("%s: no HIP device (libstb_amd has no CPU path)", who);
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
  return stb_ht_sample(I, d_koff, d_t, Kmax, G_host, d_off, opts, opts->alpha, d_root, d_hnode, d_h, d_c, d_m, seed, sweep, st, info, who,
                       nullptr);
}
