// hyperq.hip -- the auxiliary variables of the concentration step on the device (reference lib/sampleb.c:90-99): for
// every restaurant i with N_i > 0 customers, q_i ~ Beta(b, N_i), L_i = -log q_i, and Q = 1/scale + sum_i L_i.
//
//   k_logq      one lane per restaurant, grid-strided over blocks of 256 restaurants; the block sums and Q
//   k_sum_u32   sum of T over the restaurants (the a = 0 branch's Gamma shape)
//   k_segsum    customers per restaurant from the pairs (stb_tcounts' N, built once)
//
// Uniforms (counter-based, the convention of tcounts.hip): key = mix(seed + (sweep+1) gamma); restaurant i owns the
// substream key_i = mix(key + (i+1) gamma); its k-th uniform, k = 1, 2, ..., is m 2^-53 with m the top 53 bits of
// mix(key_i + k gamma), and 2^-54 in place of m = 0: always inside the open interval (0, 1), so every log is finite.
// They are consumed in the order written below; the draws depend on (seed, sweep, i) alone.
//
// log of a Gamma(alpha) variate, alpha >= 1 (Marsaglia & Tsang 2000): d = alpha - 1/3, c = 1 / sqrt(9 d); an attempt
// takes u1, u2, the normal x = sqrt(-2 log u1) cos(2 pi u2) (Box-Muller's cosine member; the sine member is not used),
// w = 1 + c x; w <= 0 ends the attempt; else v = w w w, a third uniform u, and the attempt is accepted when
//     log u < ((x x / 2 + d) - d v) + d log v          (evaluated as written, no contraction)
// with log G = log d + log v.  For alpha < 1 the boost in the log domain: log G = log G' + log(u') / alpha with
// G' ~ Gamma(alpha + 1) as above and one more uniform u' after it.  At most HQ_CAP attempts a variate (acceptance is
// above 0.95 an attempt): a lane that runs out sets the error word, writes NaN and goes on; the call then fails.
// A restaurant draws log G_b (shape b) first, then log G_N (shape N_i); with D = log G_N - log G_b
//     L_i = log1p(exp D)  (D <= 0),   D + log1p(exp(-D))  (D > 0)
// which is -log(G_b / (G_b + G_N)) without ever forming q: q underflows for small b where L_i stays an ordinary number.
//
// Q does not depend on launch geometry: the L of restaurants 256 c .. 256 c + 255 (0 beyond I) are summed in one fixed
// tree (four quarters per lane, then the shuffle tree of a 64-lane wave), and the last workgroup to finish -- a ticket --
// adds the block sums in a fixed order as well (lane l the blocks l, l + 64, ... in double-double, then the same tree)
// to 1/scale.  Q and the error word go to pinned host memory from the kernel: one launch, one wait, no copy.
// STB_HYPERQ_WAVES = 1, 2, 4 or 8 waves a workgroup (default 4); the bits are the same for each.
//
// What sets the pace: FP64 transcendentals.  A restaurant costs two variates, each attempt five of them (log u1, cos,
// sqrt, log v, log u) plus log d, and exp / log1p at the end -- about 14 calls of 40 to 100 FP64 instructions, against
// 4 bytes read and 8 written.  Lanes diverge only in the attempt loop (a wave repeats while any lane rejects: with
// acceptance above 0.95, 64 lanes need two rounds more often than not and almost never four) and between b < 1 and
// b >= 1, which is uniform over the launch.

#include "stb_common.h"
#include "tcounts.h"
#include "hyperq.h"
#include "gamma_dev.h"  // hq_unit, hq_log_gamma, hq_draw_L, HQ_CAP
#include "ticket.h"

#define HQ_CHUNK STB_TG_BLOCK  // (one constant for the kernel, the launch and stb_reduce_geometry)
#define HQ_MAXTHREADS 512

// ctl[0] ticket, ctl[1] error word (both zeroed on the stream ahead of the launch); host_out[0] = Q, host_out[1] = error
__global__ __launch_bounds__(HQ_MAXTHREADS) void k_logq(double b, double inv_scale, uint64_t I, const uint32_t *Nv,
                                                        const uint64_t *coff, double *Lout, uint64_t key, double *partial,
                                                        unsigned nchunks, unsigned *ctl, double *host_out) {
  __shared__ double sL[HQ_MAXTHREADS];
  __shared__ unsigned s_last;
  const unsigned nthr = blockDim.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned cps = stb_tg_cps(nthr);   // blocks of 256 a workgroup takes per step
  const unsigned span = cps * HQ_CHUNK;    // ... which are this many restaurants
  const unsigned nsteps = (nchunks + cps - 1) / cps;
  bool bad = false;
  for (unsigned s = blockIdx.x; s < nsteps; s += gridDim.x) {
    const uint64_t base = (uint64_t)s * span;
    for (unsigned o = threadIdx.x; o < span; o += nthr) {
      const uint64_t i = base + o;
      double L = 0.0;
      if (i < I) {
        const uint64_t Ni = Nv ? (uint64_t)Nv[i] : coff[i + 1] - coff[i];
        if (Ni > 0) L = hq_draw_L(b, (double)Ni, key, i, bad);
        if (Lout) Lout[i] = L;
      }
      sL[o] = L;
    }
    __syncthreads();
    if (wave < cps) {  // (cps <= the number of waves: 1 up to four waves, 2 with eight)
      const double *p = sL + wave * HQ_CHUNK;
      double v = (p[lane] + p[lane + 64]) + (p[lane + 128] + p[lane + 192]);
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
      const unsigned c = s * cps + wave;
      if (lane == 0 && c < nchunks) partial[c] = v;
    }
    __syncthreads();
  }
  if (bad) __hip_atomic_fetch_or(&ctl[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!stb_ticket_last(ctl, gridDim.x, &s_last) || wave != 0) return;  // (ticket.h)
  dd_t acc{0.0, 0.0};
  for (unsigned c = lane; c < nchunks; c += 64) dd_add(acc, partial[c]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    dd_t o;
    o.hi = __shfl_down(acc.hi, off, 64);
    o.lo = __shfl_down(acc.lo, off, 64);
    dd_merge(acc, o);
  }
  if (lane == 0) {
    dd_add(acc, inv_scale);
    host_out[0] = acc.hi + acc.lo;
    host_out[1] = (double)__hip_atomic_load(&ctl[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(256) void k_sum_u32(const uint32_t *T, uint64_t I, unsigned long long *host_out) {
  __shared__ unsigned long long sw[4];
  unsigned long long v = 0;  // (integers: exact in any order)
  for (uint64_t i = threadIdx.x; i < I; i += 256) v += T[i];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) *host_out = sw[0] + sw[1] + sw[2] + sw[3];
}

__global__ __launch_bounds__(256) void k_segsum(const uint64_t *koff, const uint32_t *n, int I, uint32_t *Nout) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I) return;
  uint32_t v = 0;
  for (uint64_t g = koff[i]; g < koff[i + 1]; g++) v += n[g];
  Nout[i] = v;
}

// ------------------------------------------------------------------------------------------------
// per calling thread: the block sums, the ticket and error words, and the pinned words the kernels answer in.  A call
// waits for its answer before it returns, so one set per thread is never in use twice.

static thread_local stb_tset hq;  // h_out: [0] Q, [1] error word, [2] (as uint64) sum of T

extern "C" void stb_hq_release(void) {
  STB_ENTRY;
  stb_tset_drop(hq);
}

extern "C" int stb_hq_logq(double b, double scale, int I, const uint32_t *d_N, const uint64_t *d_coff, double *d_L,
                           double *Q_host, uint64_t seed, uint64_t sweep, void *stream) {
  STB_ENTRY;
  if (!(b > 0.0) || !std::isfinite(b)) return stb_fail("stb_sample_logq: b=%g (a Beta(b, N) draw needs b > 0, finite)", b);
  if (!(scale > 0.0) || !std::isfinite(scale)) return stb_fail("stb_sample_logq: scale=%g (must be > 0, finite)", scale);
  if (I < 0) return stb_fail("stb_sample_logq: I=%d", I);
  if (!Q_host) return stb_fail("stb_sample_logq: Q_host is required");
  if (I > 0 && !d_N == !d_coff) return stb_fail("stb_sample_logq: the customers per restaurant are required");
  if (I == 0) {
    *Q_host = 1.0 / scale;
    return 0;
  }
  if (stb_device_count() < 1) return stb_no_device("stb_sample_logq");
  hipStream_t st = (hipStream_t)stream;
  stb_tgeom tg;
  if (stb_ticket_geom(STB_GEOM_LOGQ, (uint64_t)I, 0, 0, 0, &tg)) return stb_fail("stb_sample_logq: no launch geometry for I=%d", I);
  if (stb_tset_ready(hq, "stb_sample_logq") || stb_tset_room(hq, tg.need, STB_TG_CAP0_BLOCKS, sizeof(double), "stb_sample_logq")) return 1;
  const unsigned nchunks = tg.nblk, grid = tg.gx;
  const int nthr = 64 * (int)tg.waves;
  const uint64_t key = stb_mix64(seed + (sweep + 1) * STB_GAMMA);
  HIPCHK(hipMemsetAsync(hq.d_ctl, 0, 2 * sizeof(unsigned), st));
  STB_LAUNCH(k_logq, dim3(grid), dim3(nthr), st, b, 1.0 / scale, (uint64_t)I, d_N, d_coff, d_L, key, (double *)hq.d_buf, nchunks,
             hq.d_ctl, hq.h_out_dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  const double Q = ((volatile double *)hq.h_out)[0], err = ((volatile double *)hq.h_out)[1];
  if (err != 0.0)
    return stb_fail("stb_sample_logq: a Gamma draw was not accepted within %d attempts (b=%g, seed=%llu, sweep=%llu)", HQ_CAP, b,
                    (unsigned long long)seed, (unsigned long long)sweep);
  *Q_host = Q;
  return 0;
}

extern "C" int stb_sample_logq(double b, double scale, int I, const uint32_t *d_N, double *d_L, double *Q_host, uint64_t seed,
                               uint64_t sweep, void *stream) {
  if (I > 0 && !d_N) return stb_fail("stb_sample_logq: d_N is required");
  return stb_hq_logq(b, scale, I, d_N, nullptr, d_L, Q_host, seed, sweep, stream);
}

extern "C" int stb_hq_sum_u32(const uint32_t *d_T, int I, uint64_t *sum_host, void *stream) {
  STB_ENTRY;
  if (I < 0 || !sum_host || (I > 0 && !d_T)) return stb_fail("stb_sampleb_device: I=%d and T are required", I);
  if (I == 0) {
    *sum_host = 0;
    return 0;
  }
  if (stb_tset_ready(hq, "stb_sampleb_device")) return 1;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long *out_dev = (unsigned long long *)(hq.h_out_dev + 2);
  STB_LAUNCH(k_sum_u32, dim3(1), dim3(256), st, d_T, (uint64_t)I, out_dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  *sum_host = *(volatile unsigned long long *)(hq.h_out + 2);
  return 0;
}

extern "C" int stb_hq_segsum(const uint64_t *d_koff, const uint32_t *d_n, int I, uint32_t *d_N, void *stream) {
  if (I <= 0) return 0;
  STB_LAUNCH(k_segsum, dim3((unsigned)((I + 255) / 256)), dim3(256), (hipStream_t)stream, d_koff, d_n, I, d_N);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int stb_fail_msg(const char *msg) { return stb_fail("%s", msg); }
