/* wave.h -- private: what one wave of 64 lanes does with its own registers, no LDS and no memory.  The sampler kernels
 * took these from one another by copy (MEASUREMENTS O6); they are written here once, and the other private headers
 * (tindic.h, ticket.h, seat_visit.h, tcounts.h) include this one.
 *
 *   stb_wave_rl, stb_wave_rld, stb_wave_rl64
 *                    lane j's 32-bit word, double or 64-bit word, j the same in every lane: k_tindic (tindic.hip), k_tdish
 *                    (tdish.hip), k_seat and k_seat_sum (seat.hip), k_seat_pf (seat_pf.hip), k_ais_weight (seat_ais.hip)
 *   stb_wave_scan    the inclusive Kogge-Stone scan, lane l adding lane l - d for d = 1, 2, .. 32: k_tdish, k_seat and
 *                    k_seat_pf (through st_visit, seat_visit.h; k_seat_pf's weight sums too), k_partition (partition.hip),
 *                    k_tcwin (tcwin.hip), k_tcounts (tcounts.hip: the wave's part of tc_scan).  groups.h keeps the
 *                    `unsigned` scan of the list builders, and k_tcwin's one-chunk rows their two segmented scans (up
 *                    and down from t in one loop: another operation)
 *   stb_wave_all_max, stb_wave_all_sum, stb_wave_all_min
 *                    xor butterflies, offsets 1, 2, .. 32, every lane the same bits: the max in k_tcwin, k_tcounts (the
 *                    wave's part of tc_max) and k_seat_sum; the sum in k_tcwin; the min over `unsigned` in k_tcounts (the
 *                    wave's part of tc_min)
 *   stb_wave_sum     the shuffle tree v += shfl_down(v, o), o = 32, 16, .. 1, the result lane 0's: the callers are listed
 *                    in ticket.h, with the five kernels that keep the tree written out
 *   stb_wave_choice  the dish a threshold picks among 64 cumulative weights: k_tdish<true>, and st_visit<true> in k_seat
 *                    and k_seat_pf.  The block forms (k_tdish<false>, st_visit<false>) keep their loops: theirs stops at the
 *                    first block that holds a hit and remembers the last block with weight, which is no call of this
 *
 * Left as they are, because a call there compiles to other code than the loop (ticket.h, MEASUREMENTS O3): the trees of
 * k_logq, k_sum_u32, k_joint_terms, k_hb_group_wg and k_eval_tail, those of hg_cell.h, hgroups.hip and lists.hip, and
 * everything in the fill and grid kernels.
 */
#ifndef STB_WAVE_H
#define STB_WAVE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#if defined(__HIPCC__)

// ---- readlanes: every lane of a wave walks the same chain on the same values ----

__device__ __forceinline__ unsigned stb_wave_rl(unsigned v, unsigned j) {
  return (unsigned)__builtin_amdgcn_readlane((int)v, (int)__builtin_amdgcn_readfirstlane((int)j));
}
__device__ __forceinline__ double stb_wave_rld(double v, unsigned j) {
  const int jj = __builtin_amdgcn_readfirstlane((int)j);
  const uint64_t x = (uint64_t)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, jj);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), jj);
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
__device__ __forceinline__ uint64_t stb_wave_rl64(uint64_t v, unsigned j) {
  return ((uint64_t)stb_wave_rl((unsigned)(v >> 32), j) << 32) | stb_wave_rl((unsigned)v, j);
}

// ---- the inclusive scan: lane l gets x_0 + .. + x_l in the Kogge-Stone association (no contraction: it only adds) ----

__device__ __forceinline__ double stb_wave_scan(double x, unsigned lane) {
#pragma clang fp contract(off)
#pragma unroll
  for (unsigned d = 1; d < 64; d <<= 1) {
    const double y = __shfl_up(x, d, 64);
    if (lane >= d) x = x + y;
  }
  return x;
}

// ---- all-lanes butterflies ----

__device__ __forceinline__ double stb_wave_all_max(double v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ double stb_wave_all_sum(double v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);  // (x + y and y + x: the same bits in both lanes)
  return v;
}

__device__ __forceinline__ unsigned stb_wave_all_min(unsigned v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = min(v, (unsigned)__shfl_xor((int)v, o, 64));
  return v;
}

// ---- the sum over the 64 lanes, v += shfl_down(v, o) for o = 32, 16, .. 1; the result is lane 0's ----

__device__ __forceinline__ double stb_wave_sum(double v) {
#pragma clang fp contract(off)
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__device__ __forceinline__ unsigned long long stb_wave_sum(unsigned long long v) {  // (integers: exact in any order)
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// ---- the choice: the smallest lane with weight (its bit in pos) whose cumulative sum exceeds thr, else the largest lane
// with weight.  pos != 0 ----

__device__ __forceinline__ unsigned stb_wave_choice(uint64_t pos, double cum, double thr, unsigned lane) {
  const uint64_t hit = __ballot(((pos >> lane) & 1) && cum > thr);
  return hit ? (unsigned)__builtin_ctzll(hit) : 63u - (unsigned)__builtin_clzll(pos);
}

#endif  // __HIPCC__
#endif
