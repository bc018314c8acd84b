// hyperb.hip -- one concentration per group of restaurants, resampled on the device by Teh's auxiliary variables
// (include/stb_hip.h, stb_sample_bgroups).  Group g shares b > 0 with the prior Gamma(shape, scale);
// restaurant i of it has T_i tables and N_i customers, the discount is a in [0, 1):
//     q_i | b ~ Beta(b, N_i) (N_i > 0),  L_i = -log q_i;     y_ik | b ~ Bernoulli(b / (b + k a)), k = 1 .. T_i - 1,
//     Y_i = [T_i >= 1] + sum_k y_ik;     b | q, y ~ Gamma(shape + sum_i Y_i, rate = 1/scale + sum_i L_i).
//
//   k_hb_rest        pass 1, a lane per restaurant: L_i, Y_i and the checks of b_i; restaurants with many tables are
//                    handed to the workgroup's waves, one wave a restaurant, k strided over its lanes
//   k_hb_group_wg    pass 2 over ranges: a workgroup per group sums L and Y, draws b_g, scatters it
//   k_hb_group_lane  pass 2 without ranges (every restaurant its own group): a lane per group
//   k_hb_finish      the counts, the error word and (one group) b to pinned words
// All three are queued back to back on the caller's stream; the call waits once, for the pinned words.  The two halves
// are also entries of their own (hyperb.h: stb_hb_bgroups_queue, _answer) for a caller that queues the step among
// launches of its own and waits once for all of them (hgroups.hip); _queue_dscale is _queue with the prior's 1/scale read
// from a device word an earlier launch left (dirconc.hip), pass 2 over ranges being the one kernel that reads it.
//
// Streams: key = mix(seed + (sweep+1) gamma); restaurant i owns key_i = mix(key + (i+1) gamma).  L_i is hq_draw_L
// (gamma_dev.h) on key_i unchanged: with every b_i equal it is stb_sample_logq's L to the bit.  The y take the substream
// mix(key_i ^ HB_SALT_Y): y_ik = [u_k (b + k a) < b] with u_k its element k (hq_unit's open interval), so they do not depend
// on how many uniforms the Beta draw took.  Group g's Gamma variate takes mix(key' + (g+1) gamma), key' = mix(key ^
// HB_SALT_G), through hq_log_gamma.  Y is a sum of integers: any order is exact, so both forms of pass 1 give the same bits.
//
// sum L has one association, relative to the group's first restaurant: blocks of 256 restaurants (0 beyond the group's
// end), inside a block k_logq's tree (four quarters per lane, then the shuffle tree of a 64-lane wave), the block sums
// lane-strided in double-double (lane l the blocks l, l + 64, ...), merged by the same tree, 1/scale added last.  One
// group of equal b therefore has stb_sample_logq's Q as its rate, to the bit, and a group of one restaurant has
// L_i + 1/scale in double-double whichever kernel draws it.  STB_HYPERB_WAVES = 1, 2, 4 or 8 waves a workgroup (default
// 4) and STB_HYPERB_FORM = lane | wave (pass 1; default: a wave for T_i - 1 > HB_TWAVE) change no bit.
//
// Error word (pass 1; any bit fails the call and pass 2 then writes nothing): 1 a rejection loop ran out, 2 a b_i is
// not a positive finite double, 4 a b_i differs from its group's first restaurant's, 8 the ranges are not 0 = goff[0]
// <= ... <= goff[G] = I.  A group whose draw is not a positive finite double keeps its b and is counted.

#include <cfloat>

#include "stb_common.h"
#include "tcounts.h"
#include "hyperb.h"
#include "gamma_dev.h"  // hq_unit, hq_log_gamma, hq_draw_L, HQ_CAP
#include "ticket.h"

#define HB_SALT_Y 0x59B1D5A7C3E9F24Dull  // the y substream of a restaurant: mix(key_i ^ HB_SALT_Y)
#define HB_SALT_G 0x6A09E667F3BCC909ull  // the groups' key: mix(key ^ HB_SALT_G)
#define HB_MAXTHREADS 512
#define HB_BLOCK 256u   // restaurants of a block sum (k_logq's)
#define HB_ROUND 512u   // block sums held in LDS at a time (a multiple of 64: lane l keeps the blocks l, l + 64, ...)
#define HB_TWAVE 256u   // a restaurant with more Bernoulli draws than this goes to a wave
#define HB_ERR_CAP 1u
#define HB_ERR_B 2u
#define HB_ERR_UNEQUAL 4u
#define HB_ERR_GOFF 8u
// ctl words (device): [0] error word, [1] bad restaurants, [2] kept groups, [4..5] group 0's b (a double)

__device__ __forceinline__ unsigned hb_y(double b, double a, uint64_t ky, uint64_t k) {
#pragma clang fp contract(off)
  return hq_unit(ky, k) * (b + (double)k * a) < b ? 1u : 0u;
}

__global__ __launch_bounds__(HB_MAXTHREADS) void k_hb_rest(double a, uint64_t I, const uint32_t *Nv, const uint64_t *coff,
                                                           const uint32_t *Tv, uint64_t G, const uint64_t *goff,
                                                           const double *bpar, double *Lout, uint32_t *Yout, uint64_t key,
                                                           unsigned twave, unsigned *ctl) {
  __shared__ unsigned short s_list[HB_MAXTHREADS];
  __shared__ unsigned s_n;
  const unsigned nthr = blockDim.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = nthr >> 6;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * nthr, i = base + threadIdx.x;
  unsigned err = 0;
  if (goff && i < G) {
    if (goff[i] > goff[i + 1]) err |= HB_ERR_GOFF;
    if (i == 0 && (goff[0] != 0 || goff[G] != I)) err |= HB_ERR_GOFF;
  }
  if (i < I) {
    const double b = bpar[i];
    const uint64_t Ni = Nv ? (uint64_t)Nv[i] : coff[i + 1] - coff[i];
    const uint32_t Ti = Tv[i];
    double L = 0.0;
    uint32_t Y = Ti >= 1 ? 1u : 0u;
    unsigned mine = 0;
    if (!(b > 0.0) || !isfinite(b)) {
      mine = HB_ERR_B;
      L = NAN;
      Y = 0;
    } else {
      if (goff) {  // the last range that starts at or before i (empty ranges in front of it start there too)
        uint64_t lo = 0, hi = G;
        while (hi - lo > 1) {
          const uint64_t mid = lo + (hi - lo) / 2;
          if (goff[mid] <= i) lo = mid; else hi = mid;
        }
        const uint64_t first = goff[lo];
        if (first > i || goff[lo + 1] <= i) err |= HB_ERR_GOFF;  // (ranges out of order; never addressed beyond I)
        else if (bpar[first] != b) mine |= HB_ERR_UNEQUAL;
      }
      bool bad = false;
      if (Ni > 0) L = hq_draw_L(b, (double)Ni, key, i, bad);
      if (bad) mine |= HB_ERR_CAP;
      if (Ti >= 2) {
        if (Ti - 1 > twave) {
          s_list[atomicAdd(&s_n, 1u)] = (unsigned short)threadIdx.x;
        } else {
          const uint64_t ky = stb_mix64(stb_mix64(key + (i + 1) * STB_GAMMA) ^ HB_SALT_Y);
          for (uint64_t k = 1; k < Ti; k++) Y += hb_y(b, a, ky, k);
        }
      }
    }
    Lout[i] = L;
    Yout[i] = Y;
    if (mine) atomicAdd(&ctl[1], 1u);
    err |= mine;
  }
  if (err) __hip_atomic_fetch_or(&ctl[0], err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const unsigned nl = s_n;  // (the same for every wave: the loop below is uniform over the workgroup)
  for (unsigned e = wave; e < nl; e += nw) {
    const uint64_t j = base + s_list[e];
    const double b = bpar[j];
    const uint64_t Tj = Tv[j];
    const uint64_t ky = stb_mix64(stb_mix64(key + (j + 1) * STB_GAMMA) ^ HB_SALT_Y);
    unsigned cnt = 0;
    for (uint64_t k = 1 + lane; k < Tj; k += 64) cnt += hb_y(b, a, ky, k);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if (lane == 0) Yout[j] = 1u + cnt;
  }
}

// the group's draw from its sums: acc the block sums in double-double, ysum the y.  Returns b_g (NaN when the variate's
// loop ran out)
__device__ __forceinline__ double hb_draw_b(dd_t acc, double inv_scale, double shape, unsigned long long ysum, uint64_t keyG,
                                            uint64_t g, double *rate_out) {
#pragma clang fp contract(off)
  dd_add(acc, inv_scale);
  const double rate = acc.hi + acc.lo;
  if (rate_out) *rate_out = rate;
  const uint64_t kg = stb_mix64(keyG + (g + 1) * STB_GAMMA);
  uint64_t k = 0;
  bool bad = false;
  const double lg = hq_log_gamma(shape + (double)ysum, kg, k, bad);
  return bad ? NAN : exp(lg - log(rate));
}

// d_inv_scale (may be null): a device word an earlier launch on the stream left, read in place of inv_scale
__global__ __launch_bounds__(HB_MAXTHREADS) void k_hb_group_wg(double inv_scale, const double *d_inv_scale, double shape,
                                                               const uint64_t *goff,
                                                               const double *Lv, const uint32_t *Yv, double *bpar,
                                                               double *bgrp, double *rate_out, uint64_t keyG, unsigned *ctl) {
  __shared__ double sblk[HB_ROUND];
  __shared__ unsigned long long s_y;
  __shared__ double s_b;
  if (__hip_atomic_load(&ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return;  // (uniform: pass 1 failed)
  const unsigned nthr = blockDim.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = nthr >> 6;
  const uint64_t g = blockIdx.x, s0 = goff[g], s1 = goff[g + 1];
  const uint64_t n = s1 - s0, nblk = (n + HB_BLOCK - 1) / HB_BLOCK;
  if (threadIdx.x == 0) s_y = 0;
  dd_t acc{0.0, 0.0};
  unsigned long long y = 0;
  for (uint64_t cb = 0; cb < nblk; cb += HB_ROUND) {
    const uint64_t ce = cb + HB_ROUND < nblk ? cb + HB_ROUND : nblk;
    for (uint64_t c = cb + wave; c < ce; c += nw) {
      const uint64_t r = s0 + c * HB_BLOCK + lane;
      double p[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint64_t rq = r + 64u * q;
        p[q] = rq < s1 ? Lv[rq] : 0.0;
        y += rq < s1 ? Yv[rq] : 0u;
      }
      double v = (p[0] + p[1]) + (p[2] + p[3]);
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
      if (lane == 0) sblk[c - cb] = v;
    }
    __syncthreads();
    if (wave == 0)
      for (uint64_t c = cb + lane; c < ce; c += 64) dd_add(acc, sblk[c - cb]);
    __syncthreads();
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) y += __shfl_down(y, off, 64);
  if (lane == 0 && y) atomicAdd(&s_y, y);
  if (wave == 0) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      dd_t o;
      o.hi = __shfl_down(acc.hi, off, 64);
      o.lo = __shfl_down(acc.lo, off, 64);
      dd_merge(acc, o);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double b = hb_draw_b(acc, d_inv_scale ? *d_inv_scale : inv_scale, shape, s_y, keyG, g, rate_out ? rate_out + g : nullptr);
    bool keep = !(b > 0.0) || !isfinite(b);
    if (keep) {
      atomicAdd(&ctl[2], 1u);
      b = n ? bpar[s0] : NAN;
    }
    if (bgrp) bgrp[g] = b;
    if (g == 0) *(double *)(ctl + 4) = b;
    s_b = keep ? NAN : b;
  }
  __syncthreads();
  const double b = s_b;
  if (b == b)
    for (uint64_t r = s0 + threadIdx.x; r < s1; r += nthr) bpar[r] = b;
}

__global__ __launch_bounds__(256) void k_hb_group_lane(double inv_scale, double shape, uint64_t G, const double *Lv,
                                                       const uint32_t *Yv, double *bpar, double *bgrp, double *rate_out,
                                                       uint64_t keyG, unsigned *ctl) {
  if (__hip_atomic_load(&ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return;
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  // a block of one restaurant sums to L itself ((L + 0) + (0 + 0), then zeros up the tree), and so do the merges
  dd_t acc{0.0, 0.0};
  dd_add(acc, Lv[g]);
  double b = hb_draw_b(acc, inv_scale, shape, Yv[g], keyG, g, rate_out ? rate_out + g : nullptr);
  if (!(b > 0.0) || !isfinite(b)) {
    atomicAdd(&ctl[2], 1u);
    b = bpar[g];
  } else {
    bpar[g] = b;
  }
  if (bgrp) bgrp[g] = b;
  if (g == 0) *(double *)(ctl + 4) = b;
}

__global__ void k_hb_finish(const unsigned *ctl, unsigned long long *host_out) {
  host_out[0] = ctl[0];
  host_out[1] = ctl[1];
  host_out[2] = ctl[2];
  host_out[3] = *(const unsigned long long *)(ctl + 4);
}

// ------------------------------------------------------------------------------------------------
// per calling thread: the device words, the pinned words the last kernel answers in, and Y where the caller keeps none.
// A call waits for its answer before it returns, so one set per thread is never in use twice.

static thread_local stb_tset hb;  // h_out: four u64 words (k_hb_finish); d_buf: uint32 y, no floor

extern "C" void stb_hb_release(void) {
  STB_ENTRY;
  stb_tset_drop(hb);
}

// the checks and the launches of a step, nothing waited for: *queued says whether hb_answer has words to read
static int hb_queue(double a, double shape, double scale, int I, const uint32_t *d_N, const uint64_t *d_coff,
                    const uint32_t *d_T, int G, const uint64_t *d_goff, double *d_bpar, double *d_bgrp, double *d_L,
                    uint32_t *d_Y, double *d_rate, uint64_t seed, uint64_t sweep, void *stream, stb_bgroups_info_t *info,
                    const char *who, bool *queued, const double *d_inv_scale = nullptr) {
  *queued = false;
  if (info) {
    info->bad_restaurants = info->kept_groups = 0;
    info->error_word = 0;
    info->b = NAN;
  }
  if (!(a >= 0.0 && a < 1.0)) return stb_fail("%s: discount a=%g outside [0, 1)", who, a);
  if (!(shape > 0.0) || !std::isfinite(shape)) return stb_fail("%s: shape=%g (must be > 0, finite)", who, shape);
  if (!(scale > 0.0) || !std::isfinite(scale)) return stb_fail("%s: scale=%g (must be > 0, finite)", who, scale);
  if (I < 0 || G < 0) return stb_fail("%s: I=%d, G=%d", who, I, G);
  if (!d_goff && G != I) return stb_fail("%s: without ranges every restaurant is its own group: G=%d, I=%d", who, G, I);
  if (d_goff && I > 0 && G < 1) return stb_fail("%s: G=%d ranges cannot hold I=%d restaurants", who, G, I);
  if (I > 0 && !d_N == !d_coff) return stb_fail("%s: the customers per restaurant are required, as d_N or as d_coff", who);
  if (I > 0 && (!d_T || !d_bpar || !d_L)) return stb_fail("%s: d_T, d_bpar and d_L are required", who);
  if (G == 0) return 0;
  if (stb_device_count() < 1) return stb_no_device(who);
  if (stb_tset_ready(hb, who) || stb_tset_room(hb, d_Y || I == 0 ? 0 : (size_t)I, 0, sizeof(uint32_t), who)) return 1;
  if (!d_Y) d_Y = (uint32_t *)hb.d_buf;
  hipStream_t st = (hipStream_t)stream;
  int nw = stb_env_waves("STB_HYPERB_WAVES", 0);
  const bool nw_given = nw != 0;
  if (!nw_given) nw = 4;
  const unsigned nthr = 64u * (unsigned)nw;
  // pass 2 over ranges: a group's sums are one workgroup's, so large groups get the most waves a workgroup can hold
  const unsigned nthr2 = !nw_given && d_goff && (uint64_t)I / (uint64_t)G >= 4096u ? HB_MAXTHREADS : nthr;
  const char *form = getenv("STB_HYPERB_FORM");
  const unsigned twave = form && !strcmp(form, "lane") ? 0xffffffffu : form && !strcmp(form, "wave") ? 0u : HB_TWAVE;
  const uint64_t key = stb_mix64(seed + (sweep + 1) * STB_GAMMA), keyG = stb_mix64(key ^ HB_SALT_G);
  HIPCHK(hipMemsetAsync(hb.d_ctl, 0, 8 * sizeof(unsigned), st));
  const uint64_t cover = d_goff && (uint64_t)G > (uint64_t)I ? (uint64_t)G : (uint64_t)I;
  STB_LAUNCH(k_hb_rest, dim3((unsigned)((cover + nthr - 1) / nthr)), dim3(nthr), st, a, (uint64_t)I, d_N, d_coff, d_T, (uint64_t)G,
             d_goff, (const double *)d_bpar, d_L, d_Y, key, twave, hb.d_ctl);
  if (d_goff)
    STB_LAUNCH(k_hb_group_wg, dim3((unsigned)G), dim3(nthr2), st, 1.0 / scale, d_inv_scale, shape, d_goff, (const double *)d_L,
               (const uint32_t *)d_Y, d_bpar, d_bgrp, d_rate, keyG, hb.d_ctl);
  else
    STB_LAUNCH(k_hb_group_lane, dim3((unsigned)((G + 255) / 256)), dim3(256), st, 1.0 / scale, shape, (uint64_t)G,
               (const double *)d_L, (const uint32_t *)d_Y, d_bpar, d_bgrp, d_rate, keyG, hb.d_ctl);
  STB_LAUNCH(k_hb_finish, dim3(1), dim3(1), st, (const unsigned *)hb.d_ctl, (unsigned long long *)hb.h_out_dev);
  HIPCHK(hipGetLastError());
  *queued = true;
  return 0;
}

// the pinned words of the step hb_queue queued last on this thread, once its stream has been waited for
static int hb_answer(int G, stb_bgroups_info_t *info, const char *who) {
  const volatile unsigned long long *h = (const volatile unsigned long long *)hb.h_out;
  const unsigned err = (unsigned)h[0];
  if (info) {
    info->error_word = err;
    info->bad_restaurants = h[1];
    info->kept_groups = h[2];
  }
  if (err)
    return stb_fail("%s: refused, error word 0x%x over %llu restaurants (1: a Gamma draw was not accepted within %d attempts; "
                    "2: a b_i is not a positive finite double; 4: a b_i differs from its group's first; 8: the ranges are not "
                    "0 = goff[0] <= ... <= goff[G] = I); nothing was written",
                    who, err, (unsigned long long)h[1], HQ_CAP);
  if (info && G == 1) {
    const unsigned long long bits = h[3];
    memcpy(&info->b, &bits, sizeof(double));
  }
  return 0;
}

extern "C" int stb_hb_bgroups(double a, double shape, double scale, int I, const uint32_t *d_N, const uint64_t *d_coff,
                              const uint32_t *d_T, int G, const uint64_t *d_goff, double *d_bpar, double *d_bgrp, double *d_L,
                              uint32_t *d_Y, double *d_rate, uint64_t seed, uint64_t sweep, void *stream,
                              stb_bgroups_info_t *info, const char *who) {
  STB_ENTRY;
  bool queued = false;
  if (hb_queue(a, shape, scale, I, d_N, d_coff, d_T, G, d_goff, d_bpar, d_bgrp, d_L, d_Y, d_rate, seed, sweep, stream, info, who,
               &queued))
    return 1;
  if (!queued) return 0;
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return hb_answer(G, info, who);
}

extern "C" int stb_hb_bgroups_queue(double a, double shape, double scale, int I, const uint32_t *d_N, const uint32_t *d_T, int G,
                                    const uint64_t *d_goff, double *d_bpar, double *d_L, uint32_t *d_Y, uint64_t seed,
                                    uint64_t sweep, void *stream, const char *who) {
  STB_ENTRY;
  bool queued = false;
  return hb_queue(a, shape, scale, I, d_N, nullptr, d_T, G, d_goff, d_bpar, nullptr, d_L, d_Y, nullptr, seed, sweep, stream,
                  nullptr, who, &queued);
}

extern "C" int stb_hb_bgroups_queue_dscale(const double *d_inv_scale, double shape, int I, const uint32_t *d_N,
                                           const uint32_t *d_T, int G, const uint64_t *d_goff, double *d_bpar, double *d_L,
                                           uint32_t *d_Y, uint64_t seed, uint64_t sweep, void *stream, const char *who) {
  STB_ENTRY;
  bool queued = false;
  if (!d_inv_scale || !d_goff) return stb_fail("%s: the device's 1/scale and the ranges are required", who);
  return hb_queue(0.0, shape, 1.0, I, d_N, nullptr, d_T, G, d_goff, d_bpar, nullptr, d_L, d_Y, nullptr, seed, sweep, stream, nullptr,
                  who, &queued, d_inv_scale);
}

extern "C" int stb_hb_bgroups_answer(int G, stb_bgroups_info_t *info, const char *who) {
  STB_ENTRY;
  if (info) {
    info->bad_restaurants = info->kept_groups = 0;
    info->error_word = 0;
    info->b = NAN;
  }
  return hb_answer(G, info, who);
}

extern "C" int stb_sample_bgroups(double a, double shape, double scale, int I, const uint32_t *d_N, const uint64_t *d_coff,
                                  const uint32_t *d_T, int G, const uint64_t *d_goff, double *d_bpar, double *d_bgrp, double *d_L,
                                  uint32_t *d_Y, uint64_t seed, uint64_t sweep, void *stream, stb_bgroups_info_t *info) {
  return stb_hb_bgroups(a, shape, scale, I, d_N, d_coff, d_T, G, d_goff, d_bpar, d_bgrp, d_L, d_Y, nullptr, seed, sweep, stream,
                        info, "stb_sample_bgroups");
}

// ------------------------------------------------------------------------------------------------
// what the objects keep for the step

void stb_hb_obj_release(stb_hb_obj *o) {
  void *dev[] = {o->d_goff, o->d_L, o->d_Y, o->d_bgrp};
  for (void *p : dev)
    if (p) (void)hipFree(p);
  for (int k = 0; k < 2; k++) {
    if (o->h_bpar[k]) (void)hipHostFree(o->h_bpar[k]);
    if (o->ev_bpar[k]) (void)hipEventDestroy(o->ev_bpar[k]);
  }
  *o = stb_hb_obj();
}

int stb_hb_obj_init(stb_hb_obj *o, int I, const char *who) {
  for (int k = 0; k < 2; k++)
    if (hipHostMalloc((void **)&o->h_bpar[k], sizeof(double) * (size_t)I) != hipSuccess ||
        hipEventCreateWithFlags(&o->ev_bpar[k], hipEventDisableTiming) != hipSuccess)
      return STB_STREAM_FAIL(who);
  return 0;
}

int stb_hb_obj_set_groups(stb_hb_obj *o, int I, int G, const uint64_t *goff_host, void *stream, const char *who) {
  if (goff_host) {
    if (G < 1) return stb_fail("%s: G=%d", who, G);
    if (goff_host[0] != 0 || goff_host[G] != (uint64_t)I)
      return stb_fail("%s: the ranges run from %llu to %llu; the object has I=%d restaurants", who,
                      (unsigned long long)goff_host[0], (unsigned long long)goff_host[G], I);
    for (int g = 0; g < G; g++)
      if (goff_host[g] > goff_host[g + 1]) return stb_fail("%s: goff[%d] > goff[%d]", who, g, g + 1);
  }
  // the new ranges first: a call that fails leaves the object with the ranges it had
  uint64_t *d_new = nullptr;
  if (goff_host) {
    if (hipMalloc((void **)&d_new, sizeof(uint64_t) * ((size_t)G + 1)) != hipSuccess)
      return stb_fail("%s: out of device memory for %d ranges", who, G);
    if (hipMemcpy(d_new, goff_host, sizeof(uint64_t) * ((size_t)G + 1), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(d_new);
      return stb_fail("%s: %s", who, hipGetErrorString(hipGetLastError()));
    }
  }
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {  // (a queued step may still read the old ranges)
    if (d_new) (void)hipFree(d_new);
    return stb_fail("%s: %s", who, hipGetErrorString(hipGetLastError()));
  }
  if (o->d_goff) (void)hipFree(o->d_goff);
  if (o->d_bgrp) (void)hipFree(o->d_bgrp);
  o->d_goff = d_new;
  o->d_bgrp = nullptr;
  o->G = goff_host ? G : 0;
  return 0;
}

int stb_hb_obj_stage(stb_hb_obj *o, int I, double *d_bpar, const double *bpar, hipStream_t st, const char *who) {
  if (bpar == STB_BPAR_RESIDENT)  // what the object holds: nothing to upload
    return o->resident ? 0 : stb_fail("%s: STB_BPAR_RESIDENT, but the object holds no concentrations yet", who);
  if (o->last_bpar.size() == (size_t)I && memcmp(o->last_bpar.data(), bpar, sizeof(double) * I) == 0) return 0;
  const int k = o->slot ^= 1;
  o->last_bpar.clear();
  if (hipEventSynchronize(o->ev_bpar[k]) != hipSuccess) return STB_STREAM_FAIL(who);
  memcpy(o->h_bpar[k], bpar, sizeof(double) * I);
  if (hipMemcpyAsync(d_bpar, o->h_bpar[k], sizeof(double) * I, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipEventRecord(o->ev_bpar[k], st) != hipSuccess)
    return STB_STREAM_FAIL(who);
  o->last_bpar.assign(bpar, bpar + I);
  double m = INFINITY;
  for (int i = 0; i < I; i++) m = bpar[i] < m ? bpar[i] : m;
  o->min_b = m;
  o->resident = true;
  return 0;
}

int stb_hb_obj_resident(const stb_hb_obj *o, double a, const char *who) {
  if (!o->resident) return stb_fail("%s: STB_BPAR_RESIDENT, but the object holds no concentrations yet", who);
  if (!(o->min_b > -a))
    return stb_fail("%s: STB_BPAR_RESIDENT, but the object holds a concentration %g (must be > -a = %g)", who, o->min_b, -a);
  return 0;
}

int stb_hb_obj_step(stb_hb_obj *o, double a, double shape, double scale, int I, const uint32_t *d_N, const uint64_t *d_coff,
                    const uint32_t *d_T, double *d_bpar, uint64_t seed, uint64_t sweep, void *stream, double *bgrp_host,
                    stb_bgroups_info_t *info, const char *who) {
  if (!o->resident) return stb_fail("%s: the object holds no concentrations yet (stb_*_set_bpar, or a call that takes bpar)", who);
  o->last_bpar.clear();  // (from here on the step can have written d_bpar: the host values no longer describe it)
  const int G = o->d_goff ? o->G : I;
  if ((!o->d_L && hipMalloc((void **)&o->d_L, sizeof(double) * (size_t)I) != hipSuccess) ||
      (!o->d_Y && hipMalloc((void **)&o->d_Y, sizeof(uint32_t) * (size_t)I) != hipSuccess) ||
      (bgrp_host && !o->d_bgrp && hipMalloc((void **)&o->d_bgrp, sizeof(double) * (size_t)G) != hipSuccess))
    return stb_fail("%s: out of device memory for the step's %d values", who, I);
  stb_bgroups_info_t mine;
  if (!info) info = &mine;
  if (stb_hb_bgroups(a, shape, scale, I, d_N, d_coff, d_T, G, o->d_goff, d_bpar, bgrp_host ? o->d_bgrp : nullptr, o->d_L, o->d_Y,
                     nullptr, seed, sweep, stream, info, who))
    return 1;
  o->min_b = DBL_MIN;  // (the step refuses a b_i <= 0 and writes positive values only: every entry is positive now)
  if (bgrp_host) {
    if (G == 1) bgrp_host[0] = info->b;  // (from the pinned words: no copy)
    else HIPCHK(hipMemcpy(bgrp_host, o->d_bgrp, sizeof(double) * (size_t)G, hipMemcpyDeviceToHost));
  }
  return 0;
}
