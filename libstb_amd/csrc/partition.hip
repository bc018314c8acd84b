// partition.hip -- stage 1 of the S-free discount step (samplea2) on the device: for every pair (n, t) draw how the n
// customers split over the t tables, and bin the table sizes into the histogram aterms2 reads (stb_hist_aterms2).
//
//   k_partition   one wave per pair, several independent waves per workgroup, pairs grid-strided over the waves
//
// The law.  A pair is drawn in rounds r = 0 .. t-2, round r with M = t-1-r tables still to open after this one and N the
// customers still unplaced (N = n at r = 0): the size l of the next table, l = 1 .. L = N-M, with probability
//     w(l) = C(N-1, l-1) (1-a)_{l-1} S^{N-l}_M / S^N_{M+1}
// (the recursion S^N_{M+1} = sum_l C(N-1, l-1) (1-a)_{l-1} S^{N-l}_M: the weights sum to 1); N -= l.  The last table
// takes the remaining N.  S is read with stb_lookup_S's semantics: column 1 from S1, S^N_N = 1, other cells from the
// packed row of tcounts.h (tc_S).  A round with L = 1 takes l = 1 and reads nothing.
//
// The arithmetic, exactly (contraction off; one lane per candidate l, l = 64k + lane + 1 in chunk k):
//   x(l) = log((((double)(l-1) - a) * (double)(N-l+1)) / (double)(l-1))   for l >= 2, x(1) = 0, x = 0 past L
//   F(l) = log(C(N-1, l-1) (1-a)_{l-1}): a prefix sum of x, the Hillis-Steele wave scan (for o = 1, 2, .., 32 a lane
//          adds the value o lanes below, lanes >= o) of the chunk's x, plus the previous chunk's F(64k) (F = 0 before
//          chunk 0): scan + carry
//   w(l) = exp((F(l) + S^{N-l}_M) - S^N_{M+1})   (w = 0 past L; the scale is the law's own total S^N_{M+1}: every
//          w <= 1 up to rounding, so nothing overflows and no maximum pass is needed)
//   C(l) = the same wave scan of the chunk's w, plus C(64k): scan + carry; W = C(L)
// and l = the smallest l <= L with C(l) > u W, or L when rounding leaves u W at or above every C(l) (stb_tcounts' rule).
// A pair whose L fits one chunk keeps C in a register; longer ones recompute the chunks (the same operations in the same
// order: the same bits) and stop at the chunk holding the crossing.
//
// Uniforms: the splitmix64 convention of the other device samplers.  key = mix(seed + (sweep+1) gamma); round r of pair g
// uses u = element g 65536 + r + 1 of the stream (top 53 bits of mix(key + (g 65536 + r + 1) gamma) / 2^53): the
// draws depend on (seed, sweep, g, r) alone, not on the launch geometry.
//
// STB_PT_REF_WALK: lib/samplea.c:295-320 as the drop-in samplea2 runs it (deviation 12): one
// uniform a pair (r = 0's), rem = log S^n_t + log u, each round walks l = 1, 2, .. with the factor (l - a) (N-l+1) /
// (l-1), compares fact + S^{N-l}_M - log S^n_t >= rem and otherwise rem = logminus(rem, term), and clamps l to N-M.  One
// serial walk, every lane computing the same values.
//
// The output.  cnt[s] (s = 2 .. S-1): tables with s customers -- stb_hist's layout; cnt[1]: singleton tables (aterms2
// ignores them); cnt[0]: pairs left out.  A pair with n = 0 or t = n counts nothing; t = 1 counts one table of n (no
// table read); 1 < t < n draws.  Left out (cnt[0]): t = 0, t > n, n >= S, and a pair with 1 < t < n whose n > N or
// t > M (outside the table).  Every count is an integer atomic add, so the histogram does not depend on the order: sizes
// below STB_PT_LDS are counted in the workgroup's LDS copy and flushed once, larger sizes go straight to global memory.
// With d_sizes, pair g's t sizes are written in draw order at d_sizes[d_soff[g]] (the remainder last; t = 1: n; t = n:
// n ones) when its slot d_soff[g+1] - d_soff[g] holds at least t entries; pairs left out, and shorter slots, get none.

#include "stb_common.h"
#include "tcounts.h"

#define STB_PT_MAXWAVES 8
#define STB_PT_LDS 1024u  // sizes 0 .. 1023 counted in LDS (4 KB)
#define STB_PT_GRID 8192u // workgroups at most (pairs are grid-strided)

__device__ __forceinline__ double pt_S(const double *table, const double *S1, unsigned M, unsigned n, unsigned tau) {
  return tc_S(table + stb_row_offset(n, M), S1, n, tau);
}

// round's candidate l = 64k + lane + 1 (k given): its w, the wave's F carry advanced
__device__ __forceinline__ double pt_weight(const double *table, const double *S1, unsigned TM, unsigned Nr, unsigned Mc,
                                            unsigned L, double a, double ptot, unsigned k, unsigned lane, double &fcarry) {
#pragma clang fp contract(off)
  const unsigned l = 64u * k + lane + 1u;
  const bool in = l <= L;
  const double x = (in && l >= 2u) ? log((((double)(l - 1u) - a) * (double)(Nr - l + 1u)) / (double)(l - 1u)) : 0.0;
  const double F = stb_wave_scan(x, lane) + fcarry;
  fcarry = __shfl(F, 63, 64);
  return in ? exp((F + pt_S(table, S1, TM, Nr - l, Mc)) - ptot) : 0.0;
}

// one exact round: the size of the next table of Nr customers with Mc >= 1 tables to open after it
__device__ unsigned pt_round(const double *table, const double *S1, unsigned TM, unsigned Nr, unsigned Mc, double a, double u,
                             unsigned lane) {
#pragma clang fp contract(off)
  const unsigned L = Nr - Mc;
  if (L == 1u) return 1u;
  const double ptot = pt_S(table, S1, TM, Nr, Mc + 1u);
  const unsigned nc = (L + 63u) / 64u;
  double f = 0.0, W = 0.0, c1 = 0.0;
  for (unsigned k = 0; k < nc; k++) {
    const double c = stb_wave_scan(pt_weight(table, S1, TM, Nr, Mc, L, a, ptot, k, lane, f), lane) + W;
    W = __shfl(c, 63, 64);
    c1 = c;
  }
  const double target = u * W;
  if (nc == 1u) {
    const unsigned long long m = __ballot(lane + 1u <= L && c1 > target);
    return m ? (unsigned)__ffsll(m) : L;
  }
  f = 0.0;
  double C = 0.0;
  for (unsigned k = 0; k < nc; k++) {
    const double c = stb_wave_scan(pt_weight(table, S1, TM, Nr, Mc, L, a, ptot, k, lane, f), lane) + C;
    C = __shfl(c, 63, 64);
    const unsigned long long m = __ballot(64u * k + lane + 1u <= L && c > target);
    if (m) return 64u * k + (unsigned)__ffsll(m);
  }
  return L;
}

// lib/samplea.c:232-238
__device__ __forceinline__ double pt_logminus(double x, double y) {
#pragma clang fp contract(off)
  if (y >= x) return -HUGE_VAL;
  if (y - x < -80) return x - exp(y - x);
  return x + log(1 - exp(y - x));
}

__device__ __forceinline__ void pt_count(unsigned *lh, uint32_t *cnt, uint32_t s) {
  if (s < STB_PT_LDS) atomicAdd(&lh[s], 1u);
  else atomicAdd(&cnt[s], 1u);
}

__global__ __launch_bounds__(64 * STB_PT_MAXWAVES) void k_partition(const double *table, const double *S1, unsigned N,
                                                                    unsigned M, double a, uint64_t G, const uint32_t *nv,
                                                                    const uint16_t *tv, uint32_t *cnt, unsigned S,
                                                                    uint16_t *sizes, const uint64_t *soff, unsigned flags,
                                                                    uint64_t seed, uint64_t sweep) {
  __shared__ unsigned lh[STB_PT_LDS];
  const unsigned lane = threadIdx.x & 63u, wpb = blockDim.x >> 6;
  const bool ref = (flags & STB_PT_REF_WALK_FLAG) != 0;
  const unsigned SL = S < STB_PT_LDS ? S : STB_PT_LDS;
  for (unsigned s = threadIdx.x; s < SL; s += blockDim.x) lh[s] = 0u;
  __syncthreads();
  const uint64_t key = stb_mix64(seed + (sweep + 1ull) * STB_GAMMA);
  const uint64_t stride = (uint64_t)gridDim.x * wpb;
  for (uint64_t g = (uint64_t)blockIdx.x * wpb + (threadIdx.x >> 6); g < G; g += stride) {
    const unsigned n = nv[g], t = tv[g];
    uint16_t *out = nullptr;
    if (sizes) {
      const uint64_t o0 = soff[g], o1 = soff[g + 1];
      if (o1 >= o0 && o1 - o0 >= t) out = sizes + o0;
    }
    if (n == 0u) continue;
    if (t == n) {  // n tables of one: counts nothing
      if (out)
        for (unsigned j = lane; j < n; j += 64u) out[j] = 1;
      continue;
    }
    if (t == 0u || t > n || n >= S || (t > 1u && (n > N || t > M))) {
      if (lane == 0) pt_count(lh, cnt, 0u);
      continue;
    }
    if (t == 1u) {
      if (lane == 0) {
        pt_count(lh, cnt, n);
        if (out) out[0] = (uint16_t)n;
      }
      continue;
    }
    unsigned Nr = n;
    if (!ref) {
      for (unsigned r = 0; r + 1u < t; r++) {
        const unsigned l = pt_round(table, S1, M, Nr, t - 1u - r, a, stb_unit(key, g * 65536ull + r + 1u), lane);
        if (lane == 0) {
          pt_count(lh, cnt, l);
          if (out) out[r] = (uint16_t)l;
        }
        Nr -= l;
      }
    } else {
#pragma clang fp contract(off)
      const double ptot = pt_S(table, S1, M, n, t);
      double rem = ptot + log(stb_unit(key, g * 65536ull + 1u));
      for (unsigned Mc = t - 1u; Mc >= 1u; Mc--) {
        double fact = 0.0;
        unsigned l;
        for (l = 1; l <= Nr - Mc; l++) {
          if (l > 1u) fact += log(((double)l - a) * (double)(Nr - l + 1u) / (double)(l - 1u));
          const double term = fact + pt_S(table, S1, M, Nr - l, Mc) - ptot;
          if (term >= rem) break;
          rem = pt_logminus(rem, term);
        }
        if (l > Nr - Mc) l = Nr - Mc;
        if (lane == 0) {
          pt_count(lh, cnt, l);
          if (out) out[t - 1u - Mc] = (uint16_t)l;
        }
        Nr -= l;
      }
    }
    if (lane == 0) {  // the last table: the customers left
      pt_count(lh, cnt, Nr);
      if (out) out[t - 1u] = (uint16_t)Nr;
    }
  }
  __syncthreads();
  for (unsigned s = threadIdx.x; s < SL; s += blockDim.x) {
    const unsigned c = lh[s];
    if (c) atomicAdd(&cnt[s], c);
  }
}

int stb_pt_launch(const stb_table_view &S, double a, uint64_t G, const stb_cnts_ro &c, uint32_t *d_cnt, unsigned Sh,
                  unsigned flags, const stb_draw_key &k, hipStream_t st, uint16_t *d_sizes, const uint64_t *d_soff) {
  HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(uint32_t) * Sh, st));
  if (G == 0) return 0;
  const unsigned wpb = (unsigned)stb_env_waves("STB_PARTITION_WAVES", 4);
  const uint64_t want = (G + wpb - 1) / wpb;
  const unsigned grid = want < STB_PT_GRID ? (unsigned)want : STB_PT_GRID;
  STB_LAUNCH(k_partition, dim3(grid), dim3(64 * wpb), st, S.tab, S.S1, S.N, S.M, a, G, c.n, c.t, d_cnt, Sh, d_sizes, d_soff,
             flags, k.seed, k.sweep);
  HIPCHK(hipGetLastError());
  return 0;
}

int stb_pt_check(double a, unsigned N, unsigned M, uint64_t G, unsigned S, unsigned flags, const char *who) {
  if (!(a >= 0.0 && a < 1.0)) return stb_fail("%s: discount a=%g outside [0, 1)", who, a);
  if (N < 1 || M < 1) return stb_fail("%s: table bounds N=%u M=%u", who, N, M);
  if (S < 2) return stb_fail("%s: histogram length S=%u (must be >= 2)", who, S);
  if (G >= (1ull << 47)) return stb_fail("%s: G=%llu pairs (at most 2^47)", who, (unsigned long long)G);
  if (flags & ~STB_PT_REF_WALK_FLAG) return stb_fail("%s: unknown flags 0x%x", who, flags);
  return 0;
}

extern "C" int stb_sample_partition(const double *d_table, const double *d_S1, unsigned N, unsigned M, double a, uint64_t G,
                                    const uint32_t *d_n, const uint16_t *d_t, uint32_t *d_cnt, unsigned S,
                                    uint16_t *d_sizes, const uint64_t *d_soff, unsigned flags, uint64_t seed,
                                    uint64_t sweep, void *stream) {
  STB_ENTRY;
  if (stb_pt_check(a, N, M, G, S, flags, "stb_sample_partition")) return 1;
  if (!d_cnt || (G && (!d_n || !d_t))) return stb_fail("stb_sample_partition: d_cnt, and d_n, d_t when G > 0, are required");
  if (!d_sizes != !d_soff) return stb_fail("stb_sample_partition: d_sizes and d_soff go together (both or neither)");
  const stb_table_view tab = {d_table, N, M, d_S1};
  return stb_pt_launch(tab, a, G, {d_n, d_t}, d_cnt, S, flags, {seed, sweep}, (hipStream_t)stream, d_sizes, d_soff);
}
