// hg_cell.h -- private: the Antoniak auxiliary-table draw of one count cell, the one copy hgroups.hip (k_hg_aux, for the grouped and the
// tree step) and dirconc.hip (k_dc_aux_rows, k_dc_aux_cols) share.  A cell with count c and weight w owns the substream ky =
// mix(key_e ^ HG_SALT_Y) and draws
//     m = [c >= 1] + sum_{j=1}^{c-1} [u_j (w + (double)j) < w],     u_j = element j of ky (hq_unit's open interval)
// in FP64 as written, no contraction.  m is an integer, so who adds which Bernoulli changes no bit.
#ifndef STB_HG_CELL_H
#define STB_HG_CELL_H

#include "stb_common.h"
#include "gamma_dev.h"

#define HG_SALT_Y 0x59B1D5A7C3E9F24Dull  // a cell's Bernoulli substream: mix(key_e ^ HG_SALT_Y)
#define HG_SALT_A 0xA54FF53A5F1D36F1ull  // the concentration step's seed: seed ^ HG_SALT_A
#define HG_TWAVE 256u  // a cell with more Bernoulli draws than this goes to its wave

__device__ __forceinline__ unsigned hg_y(double w, uint64_t ky, uint64_t j) {
#pragma clang fp contract(off)
  return hq_unit(ky, j) * (w + (double)j) < w ? 1u : 0u;
}

// every lane of a wave calls this with a cell of its own (cc = 0: none).  The wave is one of `parts` that take the same
// cells: part 0 the cells a lane draws alone (cc - 1 <= twave) and every cell's first table, part p the draws j = 1 + 64 p +
// lane, + 64 parts, ... of the cells a wave takes.  Returns what this part adds to the lane's own m.  ky is read only
// where cc >= 2
__device__ __forceinline__ unsigned hg_cell(unsigned cc, double w, uint64_t ky, unsigned p, unsigned parts, unsigned twave,
                                            unsigned lane) {
  unsigned mm = p == 0 && cc >= 1 ? 1u : 0u;
  const bool big = cc >= 2 && cc - 1 > twave;
  if (p == 0 && cc >= 2 && !big)
    for (uint64_t j = 1; j < cc; j++) mm += hg_y(w, ky, j);
  unsigned long long todo = __ballot(big);
  while (todo) {  // (uniform over the wave) the cell of lane src, its draws strided over the lanes
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const unsigned cs = __shfl(cc, src, 64);
    const double ws = __shfl(w, src, 64);
    const uint64_t kys = (uint64_t)__shfl((unsigned long long)ky, src, 64);
    unsigned cnt = 0;
    for (uint64_t j = 1 + 64ull * p + lane; j < cs; j += 64ull * parts) cnt += hg_y(ws, kys, j);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if ((int)lane == src) mm += cnt;
  }
  return mm;
}

#endif
