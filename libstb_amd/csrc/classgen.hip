// classgen.hip -- customers' classes drawn on the device given their dishes: cls_c ~ lik[.][z_c] / Z_{z_c}, the one
// conditional of the joint the other steps leave to the caller (include/stb_hip.h, "customers' classes drawn on the
// device").
//
//   k_cls_pre    the running sums inside chunks of 256 rows (pre), and every chunk's sum
//   k_cls_base   the chunk sums of a column added in chunk order, in place: E_j = cum at chunk j's last row
//   k_cls_draw   a lane a customer: thr = u Z, binary search over the E_j, then over the chunk's pre
//
// Association (FP64, no contraction; the header fixes it): tlik.hip's.  One thread owns a (chunk, column) and adds its
// cells in row order from the chunk's first; the chunk sums are added in chunk order, so the last E is stb_sample_lik's Z
// of the same cells bit for bit.  cum_w = pre_w in chunk 0, else E_{j-1} + pre_w: at a chunk's last row that is E_j
// itself, so the search over the chunks and the search inside one see the same numbers.  Lanes run along k in the first
// two kernels: the matrix is read and pre written in rows of 64 consecutive doubles.
//
// Nothing depends on the launch geometry: STB_CLS_WAVES = 1, 2, 4 or 8 waves a workgroup (default 4) gives the same bits;
// the draw's grid is capped at CG_GRID_CAP workgroups and strides.  No kernel waits for another workgroup; the passes are
// ordered by the stream.
//
// What should set the pace, from the counts alone (MEASUREMENTS section G2 has what was measured): the draw.  The cumulative pass
// reads and writes the matrix once.  A customer costs one uniform (two 64-bit multiplies a mix) and about
// log2(chunks) + 8 dependent loads a column apart, from a scratch that stays in L2 while the matrix is a few megabytes.

#include "stb_common.h"
#include "uniforms.h"
#include "ticket.h"
#include "classgen.h"

#pragma clang fp contract(off)

#define CG_CHUNK 256        // rows of a chunk of the sums (part of the contract: tlik.hip's TL_CHUNK)
#define CG_MAXTHREADS 512
#define CG_GRID_CAP 2048u   // workgroups of k_cls_draw at most (tests/test_gpu_classgen.py names it)

// one thread a (chunk, column): wave v of workgroup (x, y) the chunks y nw + v, then + gridDim.y nw, ...
__global__ __launch_bounds__(CG_MAXTHREADS) void k_cls_pre(unsigned rows, unsigned stride, const double *lik, double *pre,
                                                           double *ends, unsigned nchunks) {
  const unsigned nw = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned k = blockIdx.x * 64 + lane;
  if (k >= stride) return;
  for (unsigned c = blockIdx.y * nw + wave; c < nchunks; c += gridDim.y * nw) {
    const uint64_t w0 = (uint64_t)c * CG_CHUNK, w1 = w0 + CG_CHUNK < rows ? w0 + CG_CHUNK : rows;
    const double *p = lik + w0 * stride + k;
    double *q = pre + w0 * stride + k;
    double s = *p;
    *q = s;
    p += stride, q += stride;
#pragma unroll 8
    for (uint64_t w = w0 + 1; w < w1; w++, p += stride, q += stride) {
      s = s + *p;
      *q = s;
    }
    ends[(uint64_t)c * stride + k] = s;
  }
}

__global__ __launch_bounds__(64) void k_cls_base(unsigned stride, double *ends, unsigned nchunks) {
  const unsigned k = blockIdx.x * 64 + threadIdx.x;
  if (k >= stride) return;
  double z = ends[k];
  for (unsigned c = 1; c < nchunks; c++) {
    z = z + ends[(uint64_t)c * stride + k];
    ends[(uint64_t)c * stride + k] = z;
  }
}

// info: NULL, or {skipped, stuck, drawn}, added to: a wave sums its lanes' counts, the workgroup's first thread adds them
__global__ __launch_bounds__(CG_MAXTHREADS) void k_cls_draw(const double *pre, const double *ends, unsigned rows, unsigned stride,
                                                            unsigned nchunks, const uint32_t *cust, const uint8_t *mask,
                                                            uint64_t C, uint64_t key, uint32_t *cls, unsigned long long *info) {
  __shared__ unsigned long long s_cnt[CG_MAXTHREADS / 64][3];
  unsigned long long nskip = 0, nstuck = 0, ndrawn = 0;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < C; c += step) {
    if (mask && !mask[c]) continue;
    const unsigned k = cust[c];
    if (k >= stride) {
      nskip++;
      continue;
    }
    const double *E = ends + k;
    const double Z = E[(uint64_t)(nchunks - 1) * stride];
    if (!(Z > 0.0 && isfinite(Z))) {
      nstuck++;
      continue;
    }
    const double thr = stb_unit(key, 3 * C + 1 + c) * Z;
    // the rule's first form where some cum exceeds thr (the last one is Z), else its second; either holds at the last row
    const bool strict = Z > thr;
    unsigned lo = 0, hi = nchunks - 1;
    while (lo < hi) {
      const unsigned mid = (lo + hi) >> 1;
      const double x = E[(uint64_t)mid * stride];
      if (strict ? x > thr : x >= Z) hi = mid;
      else lo = mid + 1;
    }
    const unsigned j = lo;
    const double base = j ? E[(uint64_t)(j - 1) * stride] : 0.0;
    const uint64_t w0 = (uint64_t)j * CG_CHUNK, left = rows - w0;
    const double *P = pre + w0 * stride + k;
    lo = 0, hi = (left < CG_CHUNK ? (unsigned)left : CG_CHUNK) - 1;  // rows of the chunk, from its first
    while (lo < hi) {
      const unsigned mid = (lo + hi) >> 1;
      double x = P[(uint64_t)mid * stride];
      if (j) x = base + x;
      if (strict ? x > thr : x >= Z) hi = mid;
      else lo = mid + 1;
    }
    cls[c] = (uint32_t)w0 + lo;
    ndrawn++;
  }
  if (!info) return;
  const unsigned nw = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  nskip = stb_wave_sum(nskip);
  nstuck = stb_wave_sum(nstuck);
  ndrawn = stb_wave_sum(ndrawn);
  if (lane == 0) s_cnt[wave][0] = nskip, s_cnt[wave][1] = nstuck, s_cnt[wave][2] = ndrawn;
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long v = 0;
    for (unsigned w = 0; w < nw; w++) v += s_cnt[w][threadIdx.x];
    if (v) atomicAdd(&info[threadIdx.x], v);
  }
}

// ------------------------------------------------------------------------------------------------
// host side

static unsigned cg_chunks(unsigned rows) { return (unsigned)(((uint64_t)rows + CG_CHUNK - 1) / CG_CHUNK); }

size_t stb_cg_scratch_bytes(unsigned rows, unsigned stride) {
  return sizeof(double) * ((size_t)rows + cg_chunks(rows)) * stride;
}

int stb_cg_launch(const stb_lik_view &L, const uint32_t *d_cust, const uint8_t *d_mask, uint64_t C, const stb_draw_key &k,
                  uint32_t *d_cls, uint64_t *d_info, void *d_scratch, hipStream_t st, const char *who) {
  if (C == 0) return 0;
  const unsigned rows = L.rows, stride = L.stride;
  const unsigned nw = (unsigned)stb_env_waves("STB_CLS_WAVES", 4), nchunks = cg_chunks(rows), cb = (stride + 63) / 64;
  double *pre = (double *)d_scratch, *ends = pre + (size_t)rows * stride;
  const uint64_t wanty = (nchunks + nw - 1) / nw, wantx = (C + 64 * nw - 1) / (64 * nw);
  const unsigned gy = wanty > 65535u ? 65535u : (unsigned)wanty, gx = wantx > CG_GRID_CAP ? CG_GRID_CAP : (unsigned)wantx;
  const uint64_t key = stb_mix64(k.seed + (k.sweep + 1) * STB_GAMMA);
  STB_LAUNCH(k_cls_pre, dim3(cb, gy), dim3(64 * nw), st, rows, stride, L.lik, pre, ends, nchunks);
  if (nchunks > 1) STB_LAUNCH(k_cls_base, dim3(cb), dim3(64), st, stride, ends, nchunks);
  STB_LAUNCH(k_cls_draw, dim3(gx), dim3(64 * nw), st, (const double *)pre, (const double *)ends, rows, stride, nchunks, d_cust,
             d_mask, C, key, d_cls, (unsigned long long *)d_info);
  if (hipGetLastError() != hipSuccess) return STB_STREAM_FAIL(who);
  return 0;
}

// ---- the raw layer ------------------------------------------------------------------------------------------------

extern "C" int stb_sample_classes(const double *d_lik, unsigned rows, unsigned stride, const uint32_t *d_cust,
                                  const uint8_t *d_mask, uint64_t C, uint64_t seed, uint64_t sweep, uint32_t *d_cls,
                                  uint64_t *d_info, void *stream) {
  STB_ENTRY;
  const char *who = "stb_sample_classes";
  if (!d_lik || (C && (!d_cls || !d_cust))) return stb_fail("%s: d_lik, d_cust and d_cls are required", who);
  if (rows < 1 || stride < 1) return stb_fail("%s: rows=%u stride=%u (both must be >= 1)", who, rows, stride);
  if (stb_device_count() < 1) return stb_no_device(who);
  if (C == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  void *d_scratch = nullptr;
  if (stb_pool_malloc(&d_scratch, stb_cg_scratch_bytes(rows, stride)) != hipSuccess)
    return stb_fail("%s: out of device memory for a %u x %u scratch", who, rows, stride);
  int rc = stb_cg_launch({d_lik, rows, stride}, d_cust, d_mask, C, {seed, sweep}, d_cls, d_info, d_scratch, st, who);
  // (the cache may hand the scratch on at once: the one wait)
  if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = STB_STREAM_FAIL(who);
  stb_pool_free(d_scratch);
  return rc;
}
