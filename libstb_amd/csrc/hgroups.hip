// hgroups.hip -- base weights per group of restaurants under a shared root, drawn on the device (include/stb_hip.h,
// stb_sample_hgroups), and the kernels of that step on a tree of nested groups (htree.hip), of which it
// is the one-level case.  Restaurants are cut into G contiguous ranges; the root r ~ Dirichlet(gamma), group g's weights
// h_g | r ~ Dirichlet(alpha r), every table of a restaurant of group g draws its dish from h_g, and c_gk counts the tables of
// group g that serve dish k.  One step, h integrated out until its own draw:
//     m_gk | c, alpha, r     Antoniak: [c_gk >= 1] + sum_{j=1}^{c_gk - 1} Bernoulli(alpha r_k / (alpha r_k + j))
//     r' | m                 Dirichlet(gamma_k + sum_g m_gk)
//     alpha' | m, c          Teh's auxiliaries: stb_sample_bgroups with a = 0, a "restaurant" per group (N = C_g, T = M_g)
//     h_g | r', alpha', c    Dirichlet(alpha' r'_k + c_gk)
// On a tree a level's rows are the groups, the level above holds their base rows (the root above the top level), and a
// parent's counts are the integer sums of its children's m.
//
//   k_hg_count    level 1's c and C: a wave a run of HG_RUN restaurants, lanes over the dishes, sums kept in registers while
//                 the group does not change (integers: atomics)
//   k_hg_aux      a level's m, M_v, and its parents' c and C (above the top level: s_k): lanes along k, a wave a run of
//                 successive rows, the parent's column sums kept in registers while the parent does not change (one parent:
//                 the rows strided over the waves); a cell with
//                 many draws is taken by its whole wave, and where the rows are few by several waves, each a slice of the
//                 draws (integers: atomics)
//   k_hg_rows     a Dirichlet row a workgroup: the root (one row), and a level's rows on their parents' new rows
//   k_hg_scatter  level 1's rows to the pairs of their restaurants
// stb_ht_sample (htree.hip) queues them back to back with its own k_ht_prep and k_ht_finish and the concentration's three
// launches (hyperb.hip, through hyperb.h's queue entry); the call waits once.  No kernel waits for another workgroup.
//
// Streams (gamma_dev.h's uniforms): key = mix(seed + (sweep+1) gamma); key_1 = key, key_l = mix(key ^ (HT_SALT_L + l)) for a
// level l >= 2.  Cell e = v Kmax + k of level l owns key_e = mix(key_l + (e+1) gamma): its row's variate takes key_e's
// elements 1, 2, ... as tlik.hip's k_th_draw does with e = k, its Bernoulli draws take u_j = element j of
// mix(key_e ^ HG_SALT_Y), hyperb.hip's y substream.  Root cell k owns mix(key_R + (k+1) gamma), key_R = mix(key ^ HG_SALT_R).
// The concentrations are one hyperb step with seed ^ HG_SALT_A, a range a level.
//
// Associations (FP64, no contraction).  w = alpha_l base_k is one product, base the parent's stored row (the root r at the top);
// a Bernoulli is u_j (w + (double)j) < w.  A row's shapes are alpha'_l base'_k + (double)c on the parent's new row (the
// root's gamma_k + (double)s_k); M = the largest lg_k (exact in any order), e_k = exp(lg_k - M), Z adds the e_k one after
// another in k order (one thread), h_k = e_k / Z: stb_tindic_sample_h's.  Counts and m are integers.  So no bit depends on
// the waves a workgroup (1, 2, 4 or 8; default 4) or on who takes a cell's Bernoulli draws (lane | wave; default: its wave
// when c - 1 > HG_TWAVE): STB_HGROUPS_WAVES and STB_HGROUPS_FORM for the grouped entry points, STB_HTREE_WAVES and
// STB_HTREE_FORM for the tree's.
//
// What should set the pace, from the counts alone (MEASUREMENTS section H1 has what was measured): G Kmax Gamma variates
// of about seven FP64 transcendentals each in k_hg_rows, against 12 bytes read and 8 written a cell; the Bernoulli draws
// are one multiply-add-compare and a 64-bit mix each, as many as there are tables.

#include <cmath>
#include <cstring>
#include <vector>

#include "stb_common.h"
#include "gamma_dev.h"
#include "hgroups.h"
#include "htree.h"
#include "ticket.h"
#include "hg_cell.h"  // HG_SALT_Y, HG_SALT_A, HG_TWAVE, hg_y, hg_cell: the cell's draw, shared with dirconc.hip

#pragma clang fp contract(off)

#define HG_SALT_R 0x6A09E667F3BCC909ull  // the root's key: mix(key ^ HG_SALT_R)
#define HG_MAXTHREADS 512
#define HG_RUN 32u     // restaurants a wave counts (or scatters) in a row
#define HG_KREG (STB_TD_MAXK / 64)
static_assert(STB_HG_KEEP_ROOT == STB_HT_KEEP_ROOT && STB_HG_SAMPLE_ALPHA == STB_HT_SAMPLE_ALPHA, "the grouped step hands its flags on");

// the last range that starts at or before restaurant i (empty ranges in front of it start there too)
__device__ __forceinline__ uint64_t hg_group_of(const uint64_t *goff, uint64_t G, uint64_t i) {
  uint64_t lo = 0, hi = G;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (goff[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void hg_flush(unsigned (&acc)[HG_KREG], unsigned long long &tot, uint64_t g, unsigned Kmax,
                                         unsigned lane, uint32_t *c, unsigned long long *Cg) {
#pragma unroll
  for (unsigned j = 0; j < HG_KREG; j++) {
    const unsigned k = lane + 64u * j;
    if (k < Kmax && acc[j]) atomicAdd(&c[g * Kmax + k], acc[j]);
    acc[j] = 0;
  }
  tot = stb_wave_sum(tot);
  if (lane == 0 && tot) atomicAdd(&Cg[g], tot);
  tot = 0;
}

// wave v of the grid the restaurants HG_RUN v .. HG_RUN v + HG_RUN - 1; goff null: restaurant i is group i
__global__ __launch_bounds__(HG_MAXTHREADS) void k_hg_count(uint64_t I, const uint64_t *koff, const uint16_t *tv, unsigned Kmax,
                                                            uint64_t G, const uint64_t *goff, uint32_t *c,
                                                            unsigned long long *Cg) {
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const uint64_t i0 = ((uint64_t)blockIdx.x * nw + wave) * HG_RUN;
  if (i0 >= I) return;  // (the whole wave)
  const uint64_t i1 = i0 + HG_RUN < I ? i0 + HG_RUN : I;
  uint64_t g = goff ? hg_group_of(goff, G, i0) : i0;
  unsigned acc[HG_KREG];
#pragma unroll
  for (unsigned j = 0; j < HG_KREG; j++) acc[j] = 0;
  unsigned long long tot = 0;
  for (uint64_t i = i0; i < i1; i++) {
    uint64_t gi = i;
    if (goff) {
      gi = g;
      while (gi + 1 < G && goff[gi + 1] <= i) gi++;
    }
    if (gi != g) {  // (uniform over the wave)
      hg_flush(acc, tot, g, Kmax, lane, c, Cg);
      g = gi;
    }
    const uint64_t p0 = koff[i], K = koff[i + 1] - p0;
#pragma unroll
    for (unsigned j = 0; j < HG_KREG; j++) {
      const unsigned k = lane + 64u * j;
      if (k < K && k < Kmax) {
        const unsigned t = tv[p0 + k];
        acc[j] += t;  // (at most HG_RUN x 65535)
        tot += t;
      }
    }
  }
  hg_flush(acc, tot, g, Kmax, lane, c, Cg);
}

// what a wave holds of parent `par`: its lanes' column sums, and (lane 0) the rows' totals
__device__ __forceinline__ void hg_hand_up(unsigned long long &acc, unsigned long long &tot, uint64_t par, unsigned Kmax, unsigned k,
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
// waves in runs of successive (row, part), or strided (below).  poff[Gp + 1] cuts the rows into their parents' ranges (null:
// one parent, row 0 of base).  The parents' counts go to cpar[Gp Kmax] and Cpar[Gp], or, above the top level, to s[Kmax] (cpar
// and Cpar null).  m may be null; with parts > 1 it arrives zeroed
__global__ __launch_bounds__(HG_MAXTHREADS) void k_hg_aux(unsigned Kmax, uint64_t G, const uint32_t *c, uint64_t Gp, const uint64_t *poff,
                                                          const double *base, double alpha, uint64_t key, unsigned twave, unsigned parts,
                                                          uint32_t *m, uint32_t *Mv, uint32_t *cpar, unsigned long long *Cpar,
                                                          unsigned long long *s) {
  const unsigned lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (what follows from it stays in scalar registers)
  const unsigned k = blockIdx.x * 64 + lane;
  const bool live = k < Kmax;  // (no lane leaves: the wave's shuffles need them all)
  const uint64_t total = G * parts, waves = (uint64_t)gridDim.y * nw, run = (total + waves - 1) / waves;
  const uint64_t gw = (uint64_t)blockIdx.y * nw + wave;
  // (uniform over the grid) one parent: nothing to keep from row to row, so wave gw strides, gw, gw + waves, ..., and the
  // waves of a workgroup read neighbouring rows
  const bool runs = poff != nullptr;
  const uint64_t q0 = runs ? gw * run : gw, step = runs ? 1 : waves;
  if (q0 >= total) return;  // (the whole wave)
  const uint64_t q1 = runs && q0 + run < total ? q0 + run : total;
  uint64_t par = poff ? hg_group_of(poff, Gp, q0 / parts) : 0;
  const double w1 = live ? alpha * base[k] : 1.0;  // (one parent: every row's w, kept out of the loop's loads)
  unsigned long long acc = 0, tot = 0;
  for (uint64_t q = q0; q < q1; q += step) {
    const uint64_t g = q / parts;
    const unsigned p = (unsigned)(q % parts);
    if (poff) {
      uint64_t pn = par;
      while (pn + 1 < Gp && poff[pn + 1] <= g) pn++;
      if (pn != par) {  // (uniform over the wave)
        hg_hand_up(acc, tot, par, Kmax, k, live, lane, cpar, Cpar, s);
        par = pn;
      }
    }
    const uint64_t e = g * Kmax + k;
    const unsigned cc = live ? c[e] : 0u;
    const double w = !poff ? w1 : live ? alpha * base[par * Kmax + k] : 1.0;
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
  hg_hand_up(acc, tot, par, Kmax, k, live, lane, cpar, Cpar, s);
}

// a workgroup a row (rows r = blockIdx.x, + gridDim.x, ...), its threads strided over k: shape_k = f base_k + count, f = *factor
// (1 when null), count = cnt32[r Kmax + k] or cnt64[k]; base_k = base0 when base is null, else base[par(r) Kmax + k] with
// par(r) from poff[Gp + 1] (null: row 0).  Cell e = r Kmax + k.  The root's row: rows = 1, cnt64 = s, no factor, no poff
__global__ __launch_bounds__(HG_MAXTHREADS) void k_hg_rows(uint64_t rows, unsigned Kmax, const uint32_t *cnt32,
                                                           const unsigned long long *cnt64, uint64_t Gp, const uint64_t *poff,
                                                           const double *base, double base0, const double *factor, uint64_t key,
                                                           double *out, unsigned *ctl) {
  __shared__ double sv[STB_TD_MAXK];
  __shared__ double s_max[HG_MAXTHREADS / 64];
  __shared__ double s_Z;
  const unsigned nthr = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
  const double f = factor ? *factor : 1.0;
  unsigned err = 0;
  for (uint64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    const double *brow = base ? base + (poff ? hg_group_of(poff, Gp, r) : 0) * Kmax : nullptr;
    bool bad = false;
    double mx = -INFINITY;
    for (unsigned k = tid; k < Kmax; k += nthr) {
      const uint64_t e = r * Kmax + k;
      const double cnt = cnt32 ? (double)cnt32[e] : (double)cnt64[k];
      const double shape = f * (brow ? brow[k] : base0) + cnt;
      double lg = NAN;
      if (shape > 0.0 && isfinite(shape)) {
        const uint64_t ke = stb_mix64(key + (e + 1) * STB_GAMMA);
        uint64_t j = 0;
        lg = hq_log_gamma(shape, ke, j, bad);
      } else if (shape == 0.0) {
        lg = -INFINITY;  // an underflowed base weight under no count: the coordinate is 0, and no uniform is taken
      } else {
        err |= HG_ERR_SHAPE;
      }
      sv[k] = lg;
      if (lg > mx) mx = lg;  // (a NaN is never greater)
    }
    if (bad) err |= HG_ERR_CAP;
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
      if (!(z > 0.0 && isfinite(z))) err |= HG_ERR_Z;
    }
    __syncthreads();
    const double Z = s_Z;
    for (unsigned k = tid; k < Kmax; k += nthr) out[r * Kmax + k] = sv[k] / Z;
    __syncthreads();  // (sv, s_max and s_Z are the next row's)
  }
  if (err) __hip_atomic_fetch_or(&ctl[0], err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(HG_MAXTHREADS) void k_hg_scatter(uint64_t I, const uint64_t *koff, unsigned Kmax, uint64_t G,
                                                              const uint64_t *goff, const double *hgrp, double *h) {
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const uint64_t i0 = ((uint64_t)blockIdx.x * nw + wave) * HG_RUN;
  if (i0 >= I) return;
  const uint64_t i1 = i0 + HG_RUN < I ? i0 + HG_RUN : I;
  uint64_t g = goff ? hg_group_of(goff, G, i0) : i0;
  for (uint64_t i = i0; i < i1; i++) {
    if (goff)
      while (g + 1 < G && goff[g + 1] <= i) g++;
    else
      g = i;
    const uint64_t p0 = koff[i], K = koff[i + 1] - p0;
    const double *row = hgrp + g * Kmax;
    for (uint64_t k = lane; k < K && k < Kmax; k += 64) h[p0 + k] = row[k];
  }
}

// ------------------------------------------------------------------------------------------------
// host side: the checks, the launches one by one (the step that queues them is htree.hip's stb_ht_sample), the grouped step

stb_hg_geom stb_hg_geom_env(const char *waves_name, const char *form_name) {
  const char *form = getenv(form_name);
  stb_hg_geom geo;
  geo.nw = (unsigned)stb_env_waves(waves_name, 4);
  geo.twave = form && !strcmp(form, "lane") ? 0xffffffffu : form && !strcmp(form, "wave") ? 0u : HG_TWAVE;
  return geo;
}

int stb_hg_check_common(unsigned flags, const double *alpha, int levels, bool indexed, double gamma0, const double *gamma_host,
                        double shape, double scale, unsigned Kmax, const char *who) {
  if (Kmax < 1 || Kmax > STB_TD_MAXK) return stb_fail("%s: Kmax=%u (1 to STB_TD_MAXK = %d)", who, Kmax, STB_TD_MAXK);
  if (flags & ~(STB_HG_KEEP_ROOT | STB_HG_SAMPLE_ALPHA)) return stb_fail("%s: unknown flags 0x%x", who, flags);
  if (!alpha) return stb_fail("%s: opts->alpha is required", who);
  for (int l = 0; l < levels; l++)
    if (!(alpha[l] > 0.0) || !std::isfinite(alpha[l]))
      return indexed ? stb_fail("%s: alpha[%d]=%g (must be > 0 and finite)", who, l, alpha[l])
                     : stb_fail("%s: alpha=%g (must be > 0 and finite)", who, alpha[l]);
  if (!(flags & STB_HG_KEEP_ROOT)) {
    if (gamma_host) {
      for (unsigned k = 0; k < Kmax; k++)
        if (!(gamma_host[k] > 0.0) || !std::isfinite(gamma_host[k]))
          return stb_fail("%s: gamma[%u]=%g (must be > 0 and finite)", who, k, gamma_host[k]);
    } else if (!(gamma0 > 0.0) || !std::isfinite(gamma0)) {
      return stb_fail("%s: gamma0=%g (must be > 0 and finite)", who, gamma0);
    }
  }
  if (flags & STB_HG_SAMPLE_ALPHA) {
    if (!(shape > 0.0) || !std::isfinite(shape)) return stb_fail("%s: shape=%g (must be > 0 and finite)", who, shape);
    if (!(scale > 0.0) || !std::isfinite(scale)) return stb_fail("%s: scale=%g (must be > 0 and finite)", who, scale);
  }
  return 0;
}

int stb_hg_check_opts(const stb_hgroups_opts_t *opts, unsigned Kmax, const char *who) {
  if (!opts) return stb_fail("%s: opts is required", who);
  return stb_hg_check_common(opts->flags, &opts->alpha, 1, false, opts->gamma0, opts->gamma_host, opts->shape, opts->scale, Kmax, who);
}

void stb_hg_clear(stb_hgroups_info_t *info) {
  if (!info) return;
  info->alpha = NAN;
  info->tables = info->aux_tables = 0;
  info->error_word = info->reserved = 0;
}

int stb_hg_count_queue(int I, const uint64_t *d_koff, const uint16_t *d_t, unsigned Kmax, int G, const uint64_t *d_goff,
                       uint32_t *d_c, unsigned long long *d_Cg, unsigned nw, hipStream_t st) {
  const uint64_t runs = ((uint64_t)I + HG_RUN - 1) / HG_RUN;
  STB_LAUNCH(k_hg_count, dim3((unsigned)((runs + nw - 1) / nw)), dim3(64 * nw), st, (uint64_t)I, d_koff, d_t, Kmax, (uint64_t)G,
             d_goff, d_c, d_Cg);
  HIPCHK(hipGetLastError());
  return 0;
}

int stb_hg_aux_queue(unsigned Kmax, uint64_t G, const uint32_t *d_c, uint64_t Gp, const uint64_t *d_poff, const double *d_base,
                     double alpha, uint64_t key, stb_hg_geom geo, uint32_t *d_m, uint32_t *d_Mv, uint32_t *d_cpar,
                     unsigned long long *d_Cpar, unsigned long long *d_s, hipStream_t st) {
  const unsigned cus = (unsigned)stb_cu_count(), cb = (Kmax + 63) / 64, nw = geo.nw;
  // few rows: each is cut into parts, so that the cells a wave takes keep about 8 waves a compute unit busy -- a group of
  // many restaurants has tens of thousands of draws a cell, a high node collects the auxiliary tables of a whole subtree
  const uint64_t cap_y = (uint64_t)8 * cus / cb + 1, fill = cap_y * nw;
  const unsigned parts = geo.twave != 0xffffffffu && G < fill ? (unsigned)((fill + G - 1) / G < 1024 ? (fill + G - 1) / G : 1024) : 1u;
  // whole rows are light: two a wave, so that half as many waves add their sums to the same s_k or parent
  const uint64_t per = parts > 1 ? 1 : 2, want_y = (G * parts + nw * per - 1) / (nw * per);
  if (parts > 1 && d_m) HIPCHK(hipMemsetAsync(d_m, 0, 4 * (size_t)G * Kmax, st));
  STB_LAUNCH(k_hg_aux, dim3(cb, (unsigned)(want_y < cap_y ? want_y : cap_y)), dim3(64 * nw), st, Kmax, G, d_c, Gp, d_poff, d_base,
             alpha, key, geo.twave, parts, d_m, d_Mv, d_cpar, d_Cpar, d_s);
  HIPCHK(hipGetLastError());
  return 0;
}

static unsigned hg_row_threads(unsigned Kmax, unsigned nw) {  // (no more waves than the row has columns for)
  const unsigned cb = (Kmax + 63) / 64;
  return 64u * (nw < cb ? nw : cb);
}

int stb_hg_root_queue(unsigned Kmax, const unsigned long long *d_s, const double *d_gam, double gamma0, uint64_t key,
                      double *d_root, unsigned *d_ctl, unsigned nw, hipStream_t st) {
  STB_LAUNCH(k_hg_rows, dim3(1), dim3(hg_row_threads(Kmax, nw)), st, (uint64_t)1, Kmax, (const uint32_t *)nullptr, d_s, (uint64_t)1,
             (const uint64_t *)nullptr, d_gam, gamma0, (const double *)nullptr, stb_mix64(key ^ HG_SALT_R), d_root, d_ctl);
  HIPCHK(hipGetLastError());
  return 0;
}

int stb_hg_rows_queue(uint64_t G, unsigned Kmax, const uint32_t *d_c, uint64_t Gp, const uint64_t *d_poff, const double *d_base,
                      const double *d_factor, uint64_t key, double *d_out, unsigned *d_ctl, unsigned nw, hipStream_t st) {
  const uint64_t cap_rows = (uint64_t)32 * (unsigned)stb_cu_count();
  STB_LAUNCH(k_hg_rows, dim3((unsigned)(G < cap_rows ? G : cap_rows)), dim3(hg_row_threads(Kmax, nw)), st, G, Kmax, d_c,
             (const unsigned long long *)nullptr, Gp, d_poff, d_base, 0.0, d_factor, key, d_out, d_ctl);
  HIPCHK(hipGetLastError());
  return 0;
}

int stb_hg_scatter_queue(int I, const uint64_t *d_koff, unsigned Kmax, int G, const uint64_t *d_goff, const double *d_hgrp,
                         double *d_h, unsigned nw, hipStream_t st) {
  const uint64_t runs = ((uint64_t)I + HG_RUN - 1) / HG_RUN;
  STB_LAUNCH(k_hg_scatter, dim3((unsigned)((runs + nw - 1) / nw)), dim3(64 * nw), st, (uint64_t)I, d_koff, Kmax, (uint64_t)G, d_goff,
             d_hgrp, d_h);
  HIPCHK(hipGetLastError());
  return 0;
}

// the grouped step is the tree's with one level: the ranges (or none) are level 1's, the root sits right above
int stb_hg_sample(int I, const uint64_t *d_koff, const uint16_t *d_t, unsigned Kmax, int G, const uint64_t *d_goff,
                  const stb_hgroups_opts_t *opts, double *d_root, double *d_h, double *d_hgrp, uint32_t *d_c, uint32_t *d_m,
                  uint64_t seed, uint64_t sweep, hipStream_t st, stb_hgroups_info_t *info, const char *who, bool *touched) {
  stb_hg_clear(info);
  stb_htree_opts_t o;
  memset(&o, 0, sizeof o);
  o.levels = 1;
  o.gamma0 = opts->gamma0;
  o.shape = opts->shape;
  o.scale = opts->scale;
  o.gamma_host = opts->gamma_host;
  o.flags = opts->flags;  // (STB_HG_KEEP_ROOT and _SAMPLE_ALPHA are STB_HT_'s)
  stb_htree_info_t ti;
  const int rc = stb_ht_sample(I, d_koff, d_t, Kmax, &G, &d_goff, &o, &opts->alpha, d_root, &d_hgrp, d_h, &d_c, &d_m, seed, sweep, st, &ti,
                               stb_hg_geom_env("STB_HGROUPS_WAVES", "STB_HGROUPS_FORM"), who, touched);
  if (info) {
    info->alpha = ti.alpha[0];
    info->tables = ti.tables[0];
    info->aux_tables = ti.aux_tables[0];
    info->error_word = ti.error_word;
  }
  return rc;
}

// ---- the raw layer ------------------------------------------------------------------------------------------------

extern "C" int stb_sample_hgroups(int I, const uint64_t *d_koff, const uint16_t *d_t, unsigned Kmax, int G, const uint64_t *d_goff,
                                  const stb_hgroups_opts_t *opts, double *d_root, double *d_h, double *d_hgrp, uint32_t *d_c,
                                  uint32_t *d_m, uint64_t seed, uint64_t sweep, void *stream, stb_hgroups_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_sample_hgroups";
  stb_hg_clear(info);
  if (!d_koff || !d_t || !d_root || !d_h) return stb_fail("%s: d_koff, d_t, d_root and d_h are required", who);
  if (I < 1) return stb_fail("%s: I=%d (must be >= 1)", who, I);
  if (stb_hg_check_opts(opts, Kmax, who)) return 1;
  if (G < 1) return stb_fail("%s: G=%d (must be >= 1)", who, G);
  if (!d_goff && G != I) return stb_fail("%s: without ranges every restaurant is its own group: G=%d, I=%d", who, G, I);
  if (stb_device_count() < 1) return stb_no_device(who);
  hipStream_t st = (hipStream_t)stream;
  if (d_goff) {  // the ranges steer stores: they are read back and checked before anything is queued
    std::vector<uint64_t> goff((size_t)G + 1);
    HIPCHK(hipMemcpyAsync(goff.data(), d_goff, 8 * ((size_t)G + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (goff[0] != 0 || goff[G] != (uint64_t)I)
      return stb_fail("%s: the ranges run from %llu to %llu; there are I=%d restaurants", who, (unsigned long long)goff[0],
                      (unsigned long long)goff[G], I);
    for (int g = 0; g < G; g++)
      if (goff[g] > goff[g + 1]) return stb_fail("%s: goff[%d] > goff[%d]", who, g, g + 1);
  }
  return stb_hg_sample(I, d_koff, d_t, Kmax, G, d_goff, opts, d_root, d_h, d_hgrp, d_c, d_m, seed, sweep, st, info, who, nullptr);
}
