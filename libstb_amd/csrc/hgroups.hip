// hgroups.hip -- base weights per group of restaurants under a shared root, drawn on the device (include/stb_hip.h,
// stb_sample_hgroups).  Restaurants are cut into G contiguous ranges; the root r ~ Dirichlet(gamma),
// group g's weights h_g | r ~ Dirichlet(alpha r), every table of a restaurant of group g draws its dish from h_g, and
// c_gk counts the tables of group g that serve dish k.  One step, h integrated out until its own draw:
//     m_gk | c, alpha, r     Antoniak: [c_gk >= 1] + sum_{j=1}^{c_gk - 1} Bernoulli(alpha r_k / (alpha r_k + j))
//     r' | m                 Dirichlet(gamma_k + sum_g m_gk)
//     alpha' | m, c          Teh's auxiliaries: stb_sample_bgroups with a = 0, a "restaurant" per group (N = C_g, T = M_g)
//     h_g | r', alpha', c    Dirichlet(alpha' r'_k + c_gk)
//
//   k_hg_count    c_gk and C_g: a wave a run of HG_RUN restaurants, lanes over the dishes, sums kept in registers while
//                 the group does not change (integers: atomics)
//   k_hg_aux      m_gk, M_g, s_k: lanes along k, a wave a group row; a cell with many draws is taken by its whole wave,
//                 and where the rows are few by several waves, each a slice of the draws (integers: atomics)
//   k_hg_prep     C_g as hyperb's N (and the 2^32 check), alpha for every group, the one range {0, G}
//   k_hg_rows     a Dirichlet row a workgroup: the root (one row) and the groups (G rows)
//   k_hg_scatter  h_g to the pairs of its restaurants
//   k_hg_finish   error word, alpha', the totals to pinned words
// All are queued back to back, the concentration's three launches (hyperb.hip, through hyperb.h's queue entry) among
// them; alpha' stays in a device word between them; the call waits once.  No kernel waits for another workgroup.
//
// Streams (gamma_dev.h's uniforms): key = mix(seed + (sweep+1) gamma).  Cell e = g Kmax + k owns key_e = mix(key + (e+1)
// gamma): its group variate takes key_e's elements 1, 2, ... as tlik.hip's k_th_draw does with e = k, its Bernoulli draws
// take u_j = element j of mix(key_e ^ HG_SALT_Y), hyperb.hip's y substream.  Root cell k owns mix(key_R + (k+1) gamma),
// key_R = mix(key ^ HG_SALT_R).  The concentration is hyperb's own step with seed ^ HG_SALT_A.
//
// Associations (FP64, no contraction).  w = alpha r_k is one product; a Bernoulli is u_j (w + (double)j) < w.  A row's
// shapes are w + (double)c (the root's gamma_k + (double)s_k); M = the largest lg_k (exact in any order), e_k = exp(lg_k -
// M), Z adds the e_k one after another in k order (one thread), h_k = e_k / Z: stb_tindic_sample_h's.  Counts and m are
// integers.  So no bit depends on STB_HGROUPS_WAVES = 1, 2, 4 or 8 waves a workgroup (default 4) or on
// STB_HGROUPS_FORM = lane | wave (who takes a cell's Bernoulli draws; default: its wave when c_gk - 1 > HG_TWAVE).
//
// What should set the pace, from the counts alone (MEASUREMENTS section H1 has what was measured): G Kmax Gamma variates
// of about seven FP64 transcendentals each in k_hg_rows, against 12 bytes read and 8 written a cell; the Bernoulli draws
// are one multiply-add-compare and a 64-bit mix each, as many as there are tables.

#include <cmath>
#include <cstring>
#include <vector>

#include "stb_common.h"
#include "gamma_dev.h"
#include "hyperb.h"
#include "hgroups.h"
#include "ticket.h"
#include "hg_cell.h"  // HG_SALT_Y, HG_SALT_A, HG_TWAVE, hg_y, hg_cell: the cell's draw, shared with dirconc.hip

#pragma clang fp contract(off)

#define HG_SALT_R 0x6A09E667F3BCC909ull  // the root's key: mix(key ^ HG_SALT_R)
#define HG_MAXTHREADS 512
#define HG_RUN 32u     // restaurants a wave counts (or scatters) in a row
#define HG_KREG (STB_TD_MAXK / 64)
#define HG_ERR_CAP 1u
#define HG_ERR_Z 2u
#define HG_ERR_SHAPE 4u
#define HG_ERR_TOTAL 8u
// ctl[0]: the error word

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

// workgroup (x, y): the columns 64 x .. 64 x + 63; its wave v the rows y nw + v, then + gridDim.y nw, ...
__global__ __launch_bounds__(HG_MAXTHREADS) void k_hg_aux(unsigned Kmax, uint64_t G, const uint32_t *c, const double *root,
                                                          double alpha, uint64_t key, unsigned twave, unsigned parts,
                                                          uint32_t *m, uint32_t *Mg, unsigned long long *s) {
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const unsigned k = blockIdx.x * 64 + lane;
  const bool live = k < Kmax;  // (no lane leaves: the wave's shuffles need them all)
  const double w = live ? alpha * root[k] : 1.0;
  unsigned long long sk = 0;
  // a row is taken by `parts` waves: part 0 the cells a lane draws alone and every cell's first table, part p the draws
  // j = 1 + 64 p + lane, + 64 parts, ... of the cells a wave takes.  With parts > 1 m arrives zeroed and is added to
  for (uint64_t q = (uint64_t)blockIdx.y * nw + wave; q < G * parts; q += (uint64_t)gridDim.y * nw) {
    const uint64_t g = q / parts;
    const unsigned p = (unsigned)(q % parts);
    const uint64_t e = g * Kmax + k;
    const unsigned cc = live ? c[e] : 0u;
    const uint64_t ky = stb_mix64(stb_mix64(key + (e + 1) * STB_GAMMA) ^ HG_SALT_Y);
    const unsigned mm = hg_cell(cc, w, ky, p, parts, twave, lane);
    if (live) {
      if (parts == 1) m[e] = mm;
      else if (mm) atomicAdd(&m[e], mm);
    }
    sk += mm;
    unsigned row = mm;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) row += __shfl_down(row, off, 64);
    if (lane == 0 && row) atomicAdd(&Mg[g], row);
  }
  if (live && sk) atomicAdd(&s[k], sk);
}

__global__ __launch_bounds__(256) void k_hg_prep(uint64_t G, const unsigned long long *Cg, double alpha, uint32_t *N32,
                                                 double *al, uint64_t *goff1, unsigned *ctl) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  const unsigned long long C = Cg[g];
  if (C > 0xffffffffull) __hip_atomic_fetch_or(&ctl[0], HG_ERR_TOTAL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  N32[g] = (uint32_t)C;
  al[g] = alpha;
  if (g == 0) {
    goff1[0] = 0;
    goff1[1] = G;
  }
}

// a workgroup a row (rows r = blockIdx.x, + gridDim.x, ...), its threads strided over k: shape_k = f base_k + count,
// f = *factor (1 when null), base_k = base[k] (base0 when null), count = cnt32[r Kmax + k] or cnt64[k]; cell e = r Kmax + k
__global__ __launch_bounds__(HG_MAXTHREADS) void k_hg_rows(uint64_t rows, unsigned Kmax, const uint32_t *cnt32,
                                                           const unsigned long long *cnt64, const double *base, double base0,
                                                           const double *factor, uint64_t key, double *out, unsigned *ctl) {
  __shared__ double sv[STB_TD_MAXK];
  __shared__ double s_max[HG_MAXTHREADS / 64];
  __shared__ double s_Z;
  const unsigned nthr = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
  const double f = factor ? *factor : 1.0;
  unsigned err = 0;
  for (uint64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    bool bad = false;
    double mx = -INFINITY;
    for (unsigned k = tid; k < Kmax; k += nthr) {
      const uint64_t e = r * Kmax + k;
      const double cnt = cnt32 ? (double)cnt32[e] : (double)cnt64[k];
      const double shape = f * (base ? base[k] : base0) + cnt;
      double lg = NAN;
      if (shape > 0.0 && isfinite(shape)) {
        const uint64_t ke = stb_mix64(key + (e + 1) * STB_GAMMA);
        uint64_t j = 0;
        lg = hq_log_gamma(shape, ke, j, bad);
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

// one workgroup: the totals over the groups, then the words the host waits for
__global__ __launch_bounds__(256) void k_hg_finish(uint64_t G, const unsigned long long *Cg, const uint32_t *Mg, const double *al,
                                                   const unsigned *ctl, unsigned long long *host_out) {
  __shared__ unsigned long long s_c, s_m;
  if (threadIdx.x == 0) s_c = s_m = 0;
  __syncthreads();
  unsigned long long cs = 0, ms = 0;
  for (uint64_t g = threadIdx.x; g < G; g += 256) {
    cs += Cg[g];
    ms += Mg[g];
  }
  if (cs) atomicAdd(&s_c, cs);
  if (ms) atomicAdd(&s_m, ms);
  __syncthreads();
  if (threadIdx.x == 0) {
    host_out[0] = ctl[0];
    host_out[1] = (unsigned long long)__double_as_longlong(al[0]);
    host_out[2] = s_c;
    host_out[3] = s_m;
  }
}

// ------------------------------------------------------------------------------------------------
// host side.  The scratch comes from the buffer cache and goes back behind the call's one wait.

struct hg_scratch {
  void *d = nullptr, *h = nullptr, *h_dev = nullptr, *stage = nullptr;
  hipStream_t st = nullptr;
  bool queued = false;  // work that uses the buffers may be on st: wait before the cache hands them on
  ~hg_scratch() {
    if (queued) (void)hipStreamSynchronize(st);
    if (d) stb_pool_free(d);
    if (h) stb_pool_free(h);
    if (stage) stb_pool_free(stage);
  }
};

static size_t hg_up(size_t x) { return (x + 255) & ~(size_t)255; }

int stb_hg_check_opts(const stb_hgroups_opts_t *opts, unsigned Kmax, const char *who) {
  if (!opts) return stb_fail("%s: opts is required", who);
  if (Kmax < 1 || Kmax > STB_TD_MAXK) return stb_fail("%s: Kmax=%u (1 to STB_TD_MAXK = %d)", who, Kmax, STB_TD_MAXK);
  if (opts->flags & ~(STB_HG_KEEP_ROOT | STB_HG_SAMPLE_ALPHA)) return stb_fail("%s: unknown flags 0x%x", who, opts->flags);
  if (!(opts->alpha > 0.0) || !std::isfinite(opts->alpha))
    return stb_fail("%s: alpha=%g (must be > 0 and finite)", who, opts->alpha);
  if (!(opts->flags & STB_HG_KEEP_ROOT)) {
    if (opts->gamma_host) {
      for (unsigned k = 0; k < Kmax; k++)
        if (!(opts->gamma_host[k] > 0.0) || !std::isfinite(opts->gamma_host[k]))
          return stb_fail("%s: gamma[%u]=%g (must be > 0 and finite)", who, k, opts->gamma_host[k]);
    } else if (!(opts->gamma0 > 0.0) || !std::isfinite(opts->gamma0)) {
      return stb_fail("%s: gamma0=%g (must be > 0 and finite)", who, opts->gamma0);
    }
  }
  if (opts->flags & STB_HG_SAMPLE_ALPHA) {
    if (!(opts->shape > 0.0) || !std::isfinite(opts->shape))
      return stb_fail("%s: shape=%g (must be > 0 and finite)", who, opts->shape);
    if (!(opts->scale > 0.0) || !std::isfinite(opts->scale))
      return stb_fail("%s: scale=%g (must be > 0 and finite)", who, opts->scale);
  }
  return 0;
}

static void hg_clear(stb_hgroups_info_t *info) {
  if (!info) return;
  info->alpha = NAN;
  info->tables = info->aux_tables = 0;
  info->error_word = info->reserved = 0;
}

int stb_hg_sample(int I, const uint64_t *d_koff, const uint16_t *d_t, unsigned Kmax, int G, const uint64_t *d_goff,
                  const stb_hgroups_opts_t *opts, double *d_root, double *d_h, double *d_hgrp, uint32_t *d_c, uint32_t *d_m,
                  uint64_t seed, uint64_t sweep, hipStream_t st, stb_hgroups_info_t *info, const char *who, bool *touched) {
  hg_clear(info);
  const bool keep_root = (opts->flags & STB_HG_KEEP_ROOT) != 0, draw_alpha = (opts->flags & STB_HG_SAMPLE_ALPHA) != 0;
  const bool gvec = !keep_root && opts->gamma_host;
  int nwi = stb_env_int("STB_HGROUPS_WAVES", 4);
  const unsigned nw = nwi == 1 || nwi == 2 || nwi == 4 || nwi == 8 ? (unsigned)nwi : 4u;
  const char *form = getenv("STB_HGROUPS_FORM");
  const unsigned twave = form && !strcmp(form, "lane") ? 0xffffffffu : form && !strcmp(form, "wave") ? 0u : HG_TWAVE;
  const size_t Gs = (size_t)G, cells = Gs * Kmax;
  // scratch.  Zeroed: ctl (256 bytes), s[Kmax], Cg[G], Mg[G] -- and c.  Then N32[G], al[G], the range {0, G}, hyperb's L[G]
  // and Y[G], gamma[Kmax], and whichever of c, m, hgrp the caller did not give
  const size_t o_s = 256, o_Cg = o_s + hg_up(8 * (size_t)Kmax), o_Mg = o_Cg + hg_up(8 * Gs), o_N = o_Mg + hg_up(4 * Gs),
               o_al = o_N + hg_up(4 * Gs), o_go = o_al + hg_up(8 * Gs), o_L = o_go + 256,
               o_Y = o_L + (draw_alpha ? hg_up(8 * Gs) : 0), o_gam = o_Y + (draw_alpha ? hg_up(4 * Gs) : 0),
               o_c = o_gam + (gvec ? hg_up(8 * (size_t)Kmax) : 0), o_m = o_c + (d_c ? 0 : hg_up(4 * cells)),
               o_hg = o_m + (d_m ? 0 : hg_up(4 * cells)), bytes = o_hg + (d_hgrp ? 0 : hg_up(8 * cells));
  hg_scratch sc;
  sc.st = st;
  if (stb_pool_malloc(&sc.d, bytes) != hipSuccess || stb_pool_malloc(&sc.h, 256, 1) != hipSuccess ||
      hipHostGetDevicePointer(&sc.h_dev, sc.h, 0) != hipSuccess ||
      (gvec && stb_pool_malloc(&sc.stage, 8 * (size_t)Kmax, 1) != hipSuccess))
    return stb_fail("%s: out of memory for %zu bytes of scratch", who, bytes);
  char *d = (char *)sc.d;
  unsigned *ctl = (unsigned *)d;
  unsigned long long *s = (unsigned long long *)(d + o_s), *Cg = (unsigned long long *)(d + o_Cg);
  uint32_t *Mg = (uint32_t *)(d + o_Mg), *N32 = (uint32_t *)(d + o_N), *Y = (uint32_t *)(d + o_Y);
  double *al = (double *)(d + o_al), *L = (double *)(d + o_L), *d_gam = gvec ? (double *)(d + o_gam) : nullptr;
  uint64_t *goff1 = (uint64_t *)(d + o_go);
  uint32_t *c = d_c ? d_c : (uint32_t *)(d + o_c), *m = d_m ? d_m : (uint32_t *)(d + o_m);
  double *hgrp = d_hgrp ? d_hgrp : (double *)(d + o_hg);
  volatile unsigned long long *h_out = (volatile unsigned long long *)sc.h;
  h_out[0] = 0xffffffffull;
  sc.queued = true;
  HIPCHK(hipMemsetAsync(d, 0, o_N, st));
  HIPCHK(hipMemsetAsync(c, 0, 4 * cells, st));
  if (gvec) {
    memcpy(sc.stage, opts->gamma_host, 8 * (size_t)Kmax);
    HIPCHK(hipMemcpyAsync(d_gam, sc.stage, 8 * (size_t)Kmax, hipMemcpyHostToDevice, st));
  }
  const uint64_t key = stb_mix64(seed + (sweep + 1) * STB_GAMMA), keyR = stb_mix64(key ^ HG_SALT_R);
  const unsigned cus = (unsigned)(stb_cu_count() > 0 ? stb_cu_count() : 1);
  const uint64_t runs = ((uint64_t)I + HG_RUN - 1) / HG_RUN;
  const unsigned gx_rest = (unsigned)((runs + nw - 1) / nw), cb = (Kmax + 63) / 64;
  // few rows: each is cut into parts, so that the cells a wave takes (a group of many restaurants has tens of thousands
  // of draws a cell) keep about 8 waves a compute unit busy
  const uint64_t cap_y = (uint64_t)8 * cus / cb + 1, fill = cap_y * nw;
  const unsigned parts = twave != 0xffffffffu && Gs < fill ? (unsigned)((fill + Gs - 1) / Gs < 1024 ? (fill + Gs - 1) / Gs : 1024) : 1u;
  const uint64_t want_y = (Gs * parts + nw - 1) / nw;
  const unsigned gy_aux = (unsigned)(want_y < cap_y ? want_y : cap_y);
  const unsigned thr_row = 64u * nw < 64u * cb ? 64u * nw : 64u * cb;  // (no more waves than the row has columns for)
  const uint64_t cap_rows = (uint64_t)32 * cus;
  const unsigned gx_rows = (unsigned)(Gs < cap_rows ? Gs : cap_rows);
  if (parts > 1) HIPCHK(hipMemsetAsync(m, 0, 4 * cells, st));
  if (stb_hg_count_queue(I, d_koff, d_t, Kmax, G, d_goff, c, Cg, st)) return 1;
  STB_LAUNCH(k_hg_aux, dim3(cb, gy_aux), dim3(64 * nw), st, Kmax, (uint64_t)G, (const uint32_t *)c, (const double *)d_root,
             opts->alpha, key, twave, parts, m, Mg, s);
  if (touched) *touched = true;
  if (!keep_root)
    STB_LAUNCH(k_hg_rows, dim3(1), dim3(thr_row), st, (uint64_t)1, Kmax, (const uint32_t *)nullptr, (const unsigned long long *)s,
               (const double *)d_gam, opts->gamma0, (const double *)nullptr, keyR, d_root, ctl);
  STB_LAUNCH(k_hg_prep, dim3((unsigned)((Gs + 255) / 256)), dim3(256), st, (uint64_t)G, (const unsigned long long *)Cg,
             opts->alpha, N32, al, goff1, ctl);
  if (draw_alpha &&
      stb_hb_bgroups_queue(0.0, opts->shape, opts->scale, G, N32, Mg, 1, goff1, al, L, Y, seed ^ HG_SALT_A, sweep, st, who))
    return 1;
  STB_LAUNCH(k_hg_rows, dim3(gx_rows), dim3(thr_row), st, (uint64_t)G, Kmax, (const uint32_t *)c,
             (const unsigned long long *)nullptr, (const double *)d_root, 0.0, (const double *)al, key, hgrp, ctl);
  STB_LAUNCH(k_hg_scatter, dim3(gx_rest), dim3(64 * nw), st, (uint64_t)I, d_koff, Kmax, (uint64_t)G, d_goff,
             (const double *)hgrp, d_h);
  STB_LAUNCH(k_hg_finish, dim3(1), dim3(256), st, (uint64_t)G, (const unsigned long long *)Cg, (const uint32_t *)Mg,
             (const double *)al, (const unsigned *)ctl, (unsigned long long *)sc.h_dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  sc.queued = false;
  const unsigned err = (unsigned)h_out[0];
  if (info) {
    const unsigned long long bits = h_out[1];
    memcpy(&info->alpha, &bits, sizeof(double));
    info->tables = h_out[2];
    info->aux_tables = h_out[3];
    info->error_word = err;
  }
  if (err)
    return stb_fail("%s: failed, error word 0x%x (1: a Gamma draw was not accepted within %d attempts; 2: a normaliser is not "
                    "positive and finite; 4: a shape alpha r_k + c_gk is not positive and finite; 8: a group has more than "
                    "2^32 - 1 tables) (seed=%llu, sweep=%llu); the outputs are undefined",
                    who, err, HQ_CAP, (unsigned long long)seed, (unsigned long long)sweep);
  if (draw_alpha) {
    stb_bgroups_info_t bi;
    if (stb_hb_bgroups_answer(1, &bi, who)) return 1;
    if (bi.kept_groups) return stb_fail("%s: the concentration's draw is not a positive finite double; the outputs are undefined", who);
  }
  return 0;
}

// k_hg_count as stb_hg_sample launches it, for a caller that wants the counts alone (the collapsed log joint, tindic_obj.hip)
int stb_hg_count_queue(int I, const uint64_t *d_koff, const uint16_t *d_t, unsigned Kmax, int G, const uint64_t *d_goff,
                       uint32_t *d_c, unsigned long long *d_Cg, hipStream_t st) {
  const int nwi = stb_env_int("STB_HGROUPS_WAVES", 4);
  const unsigned nw = nwi == 1 || nwi == 2 || nwi == 4 || nwi == 8 ? (unsigned)nwi : 4u;
  const uint64_t runs = ((uint64_t)I + HG_RUN - 1) / HG_RUN;
  STB_LAUNCH(k_hg_count, dim3((unsigned)((runs + nw - 1) / nw)), dim3(64 * nw), st, (uint64_t)I, d_koff, d_t, Kmax, (uint64_t)G,
             d_goff, d_c, d_Cg);
  HIPCHK(hipGetLastError());
  return 0;
}

// the root's row and the scatter as stb_hg_sample launches them, for the tree step (htree.hip)
int stb_hg_root_queue(unsigned Kmax, const unsigned long long *d_s, const double *d_gam, double gamma0, uint64_t key,
                      double *d_root, unsigned *d_ctl, unsigned nw, hipStream_t st) {
  const unsigned cb = (Kmax + 63) / 64, thr_row = 64u * nw < 64u * cb ? 64u * nw : 64u * cb;
  STB_LAUNCH(k_hg_rows, dim3(1), dim3(thr_row), st, (uint64_t)1, Kmax, (const uint32_t *)nullptr, d_s, d_gam, gamma0,
             (const double *)nullptr, stb_mix64(key ^ HG_SALT_R), d_root, d_ctl);
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

// ---- the raw layer ------------------------------------------------------------------------------------------------

extern "C" int stb_sample_hgroups(int I, const uint64_t *d_koff, const uint16_t *d_t, unsigned Kmax, int G, const uint64_t *d_goff,
                                  const stb_hgroups_opts_t *opts, double *d_root, double *d_h, double *d_hgrp, uint32_t *d_c,
                                  uint32_t *d_m, uint64_t seed, uint64_t sweep, void *stream, stb_hgroups_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_sample_hgroups";
  hg_clear(info);
  if (!d_koff || !d_t || !d_root || !d_h) return stb_fail("%s: d_koff, d_t, d_root and d_h are required", who);
  if (I < 1) return stb_fail("%s: I=%d (must be >= 1)", who, I);
  if (stb_hg_check_opts(opts, Kmax, who)) return 1;
  if (G < 1) return stb_fail("%s: G=%d (must be >= 1)", who, G);
  if (!d_goff && G != I) return stb_fail("%s: without ranges every restaurant is its own group: G=%d, I=%d", who, G, I);
  if (stb_device_count() < 1) return stb_fail("%s: no HIP device (libstb_amd has no CPU path)", who);
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
