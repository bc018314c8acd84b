// lists_sorted.hip -- the sort-based builder of the cell lists (struct stb_cell_list, groups.h): the pairs keyed by
// (item, position), a radix sort, a run-length encoding for the distinct cells and their counts, the CSR row pointer by
// binary search; for the grid form the dense words and, on the host, the helper jobs.  Four host round trips: taken where
// the count slab does not apply (stb_lists_build, lists.hip); decides by the distinct cells that a set is too dense for lists.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>

#include "groups.h"

#define STB_KEY_OTHER 0xfffffffffffffffeull  // a pair that addresses no table cell (t = 1, t = n, out of bounds)
#define STB_KEY_SKIP 0xffffffffffffffffull   // n <= 1: contributes nothing (lib/samplea.c:78)

// key of a pair: (item index << 9) | (row in trip << 6) | column in slice, item = trip * nsg + slice
__global__ void k_item_keys(const uint32_t *n, const uint16_t *t, uint64_t G, unsigned N, unsigned M, unsigned nsg,
                            unsigned col0, uint64_t *key, uint32_t *payload) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const unsigned nn = n[g], tt = t[g];
  uint64_t k;
  if (nn <= 1) k = STB_KEY_SKIP;
  else if (nn == tt || tt <= 1 || nn < tt || tt > M || nn > N) k = STB_KEY_OTHER;
  else {
    const unsigned trip = (nn - 3) >> 3, u = (nn - 3) & 7, sg = (tt - col0) >> 6, ln = (tt - col0) & 63;  // (tt >= 2)
    k = (((uint64_t)trip * nsg + sg) << 9) | (u << 6) | ln;
  }
  key[g] = k;
  payload[g] = (uint32_t)g;
}

// the same for the tiles of k_fill_hb: key = (item << 11) | (row in group << 8) | element of the wave (halo included),
// item = (record index of tile (strip, block)) * NQ + group of H.G rows; row n belongs to block (n - 2) / R
__global__ void k_item_keys_hb(const uint32_t *n, const uint16_t *t, uint64_t G, unsigned N, unsigned M, hb_dot_info H,
                               uint64_t *key, uint32_t *payload) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const unsigned nn = n[g], tt = t[g];
  uint64_t k;
  // (column 1 -- t = 1 -- is a cell too: the last element of strip 0's halo, which that strip's tiles compute along;
  // a pair with t = n contributes log 1 = 0; what is left as "other" has S_S = log 0, lib/stable.c:948-949)
  if (nn <= 1 || nn == tt) k = STB_KEY_SKIP;
  else if (tt == 0 || nn < tt || tt > M || nn > N) k = STB_KEY_OTHER;
  else {
    unsigned j = 0, cw = (unsigned)H.HC - 1u;  // t = 1
    if (tt >= 2) {
      const unsigned e = tt - 2;
      j = e / (unsigned)H.UC;
      cw = (unsigned)H.HC + (e - j * (unsigned)H.UC);
    }
    const unsigned b = (nn - 2) / (unsigned)H.R, r = (nn - 2) - b * (unsigned)H.R;
    const unsigned b0 = (unsigned)(((unsigned long long)j * (unsigned)H.UC) / (unsigned)H.R);
    const unsigned rec = H.rec_off[j + 1] + (b - b0);  // (b >= b0: the cell lies on or below the diagonal)
    const unsigned q = r / (unsigned)H.G;
    k = ((((uint64_t)rec * (unsigned)H.NQ) + q) << 11) | ((uint64_t)(r - q * (unsigned)H.G) << 8) | cw;
  }
  key[g] = k;
  payload[g] = (uint32_t)g;
}

// ... and for the strips of the grid form (grid_hb.hip): key = (item << 13) | (row in group << 8) | element of the wave,
// item = (record index of tile (strip, block)) * NQ + group of G rows.  Column 1 (t = 1) is a cell too -- the last
// element of strip 0's halo, which that strip computes along -- and a pair with t = n contributes log 1 = 0: what is
// left as "other" are the pairs whose S_S is log 0 (lib/stable.c:948-949).
__global__ void k_item_keys_hb2(const uint32_t *n, const uint16_t *t, uint64_t G, unsigned N, unsigned M, hb_dot_info H, int posbits,
                                uint64_t *key, uint32_t *payload) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const unsigned nn = n[g], tt = t[g];
  uint64_t k;
  if (nn <= 1 || nn == tt) k = STB_KEY_SKIP;
  else if (tt == 0 || nn < tt || tt > M || nn > N) k = STB_KEY_OTHER;
  else {
    unsigned j = 0, cw = (unsigned)H.HC - 1u;  // t = 1
    if (tt >= 2) {
      const unsigned e = tt - 2;
      j = e / (unsigned)H.UC;
      cw = (unsigned)H.HC + (e - j * (unsigned)H.UC);
    }
    const unsigned b = (nn - 2) / (unsigned)H.R, r = (nn - 2) - b * (unsigned)H.R;
    const unsigned b0 = (unsigned)(((unsigned long long)j * (unsigned)H.UC) / (unsigned)H.R);
    const unsigned rec = H.rec_off[j + 1] + (b - b0);
    const unsigned q = r / (unsigned)H.G;
    k = ((((uint64_t)rec * (unsigned)H.NQ) + q) << (posbits + 5)) | ((uint64_t)(r - q * (unsigned)H.G) << posbits) | cw;
  }
  key[g] = k;
  payload[g] = (uint32_t)g;
}

// counts[0] = keys below STB_KEY_OTHER (table cells), counts[1] = keys equal to it
__global__ void k_key_bounds(const uint64_t *key, uint64_t G, uint64_t *counts) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint64_t lo = 0, hi = G;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) / 2;
    if (key[mid] < STB_KEY_OTHER) lo = mid + 1;
    else hi = mid;
  }
  const uint64_t a = lo;
  hi = G;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) / 2;
    if (key[mid] <= STB_KEY_OTHER) lo = mid + 1;
    else hi = mid;
  }
  counts[0] = a;
  counts[1] = lo - a;
}

__global__ void k_gather_pairs(const uint32_t *n, const uint16_t *t, const uint32_t *idx, uint64_t cnt, uint32_t *n2,
                               uint16_t *t2) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g < cnt) {
    n2[g] = n[idx[g]];
    t2[g] = t[idx[g]];
  }
}

__global__ void k_split_runs(const uint64_t *ukey, const unsigned *runs, unsigned short *pos, unsigned *item, int posbits) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < *runs) {
    pos[r] = (unsigned short)(ukey[r] & ((1u << posbits) - 1u));
    item[r] = (unsigned)(ukey[r] >> posbits);
  }
}

// The grid form's dense layout.  A listed cell is one word, position | count << 13; a (tile, group of rows) holds its
// cells in NW words per lane -- NW the same for the NQ groups of a tile: the most any of them needs -- at an address that
// needs no look-up beyond the tile's own entry of `tinfo` (first word / 64 << 6 | NW), which the walking wave asks for a
// block ahead: a group's cells are coalesced loads issued ahead of their use, whether it holds 20 cells or 2000 (the
// pairs of a 10^4 x 10^4 table thin out like 1 / n: its first 4000 rows hold more than 63 cells per group of 12 x 208).
// NW = 63 marks a tile taken from the CSR lists instead (a count of 2^19 or more, or more words than STB_DENSE_NWMAX).
__global__ void k_tile_words(const unsigned *item_ptr, const unsigned *cnt, unsigned n_tiles, unsigned NQ, int wbits, unsigned *tnw, unsigned *twords) {
  const unsigned t = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
  if (t >= n_tiles) return;
  const unsigned e0 = item_ptr[(size_t)t * NQ], e1 = item_ptr[(size_t)t * NQ + NQ];
  unsigned nw = 0;
  for (unsigned q = 0; q < NQ; q++) {
    const unsigned c = item_ptr[(size_t)t * NQ + q + 1] - item_ptr[(size_t)t * NQ + q];
    nw = max(nw, (c + 63) / 64);
  }
  bool big = false;
  for (unsigned e = e0 + lane; e < e1; e += 64) big = big || cnt[e] >= (1u << (32 - wbits));  // (a word is position | count << wbits)
  if (__any(big) || nw > STB_DENSE_NWMAX) nw = STB_DENSE_CSR;
  if (lane == 0) {
    tnw[t] = nw;
    twords[t] = (nw == STB_DENSE_CSR) ? 0u : nw * NQ;
  }
}

__global__ void k_dense_fill(const unsigned *item_ptr, const unsigned short *pos, const unsigned *cnt, unsigned nitems, unsigned NQ, int wbits,
                             const unsigned *tnw, const unsigned *toff, unsigned *dense, unsigned *tinfo) {
  const unsigned i = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
  if (i >= nitems) return;
  const unsigned t = i / NQ, q = i - t * NQ;
  const unsigned nw = tnw[t];
  if (q == 0 && lane == 0) tinfo[t] = (toff[t] << 6) | nw;
  if (nw == STB_DENSE_CSR) return;
  const unsigned e0 = item_ptr[i], e1 = item_ptr[i + 1];
  unsigned *dst = dense + ((size_t)toff[t] + (size_t)q * nw) * 64;
  for (unsigned k = lane; k < nw * 64; k += 64) dst[k] = (e0 + k < e1) ? ((unsigned)pos[e0 + k] | (cnt[e0 + k] << wbits)) : 0u;
}

// item_ptr[i] = first run whose item index is >= i
__global__ void k_item_ptr(const unsigned *item, const unsigned *runs, unsigned nitems, unsigned *ptr) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > nitems) return;
  unsigned lo = 0, hi = *runs;
  while (lo < hi) {
    const unsigned mid = (lo + hi) / 2;
    if (item[mid] < i) lo = mid + 1;
    else hi = mid;
  }
  ptr[i] = lo;
}

// what one build takes from the buffer cache: given back when the build ends, behind a wait for the stream (st null:
// the owner's code has waited itself, or has queued nothing on them)
struct sort_scratch {
  hipStream_t st;
  void *p[12];
  int n = 0;
  template <class T>
  bool take(T **out, size_t bytes) {
    if (n == 12 || stb_pool_malloc((void **)out, bytes) != hipSuccess) return false;
    p[n++] = (void *)*out;
    return true;
  }
  ~sort_scratch() {
    if (st) (void)hipStreamSynchronize(st);
    for (int k = 0; k < n; k++) stb_pool_free(p[k]);
  }
};

// a step failed: the runtime's error, where it has one, is the message
static int sort_failed(const char *msg = nullptr) {
  if (msg) stb_fail("%s", msg);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) stb_fail("stb_groups_aterms: sparse set-up failed: %s", hipGetErrorString(e));
  return 1;
}

// the grid form's dense layout from the CSR lists: words per tile, their prefix sum, the words the walk reads; then the
// tiles left to helper jobs, chosen on the host.  The stream has been waited for when this returns true.
static bool sort_dense_words(stb_groups_t *g, int which, int D, const hb_dot_info &H, const grid_geom &gg, unsigned nitems) {
  stb_cell_list &l = g->lists[which];
  const unsigned n_tiles = H.n_tiles, NQ = (unsigned)H.NQ;
  sort_scratch sc{nullptr};
  unsigned *tnw = nullptr, *twords = nullptr, *toff = nullptr;
  void *tmp2 = nullptr;
  size_t b3 = 0;
  bool ok = sc.take(&tnw, 4 * (size_t)(n_tiles + 1)) && sc.take(&twords, 4 * (size_t)(n_tiles + 1)) && sc.take(&toff, 4 * (size_t)(n_tiles + 1)) &&
            stb_pool_malloc((void **)&l.tinfo, 4 * (size_t)(n_tiles + 1)) == hipSuccess;
  unsigned h_last[2] = {0, 0};
  if (ok && n_tiles) {
    hipLaunchKernelGGL(k_tile_words, dim3((n_tiles + 3) / 4), dim3(256), 0, g->st, l.item_ptr, l.ent_cnt, n_tiles, NQ, stb_pos_bits(H.C) + 5, tnw, twords);
    ok = rocprim::exclusive_scan(nullptr, b3, twords, toff, 0u, (size_t)n_tiles, rocprim::plus<unsigned>(), g->st) == hipSuccess &&
         sc.take(&tmp2, b3 ? b3 : 1) &&
         rocprim::exclusive_scan(tmp2, b3, twords, toff, 0u, (size_t)n_tiles, rocprim::plus<unsigned>(), g->st) == hipSuccess &&
         hipMemcpyAsync(&h_last[0], toff + (n_tiles - 1), 4, hipMemcpyDeviceToHost, g->st) == hipSuccess &&
         hipMemcpyAsync(&h_last[1], twords + (n_tiles - 1), 4, hipMemcpyDeviceToHost, g->st) == hipSuccess &&
         hipStreamSynchronize(g->st) == hipSuccess;
  }
  const size_t words = (size_t)h_last[0] + h_last[1];  // in units of 64 dwords
  ok = ok && words < (1u << 26);                       // (a tile's first word / 64 goes into 26 bits of its entry)
  ok = ok && stb_pool_malloc((void **)&l.dense, 256 * (words ? words : 1)) == hipSuccess;
  if (ok && nitems)
    hipLaunchKernelGGL(k_dense_fill, dim3((nitems + 3) / 4), dim3(256), 0, g->st, l.item_ptr, l.ent_pos, l.ent_cnt, nitems, NQ, stb_pos_bits(H.C) + 5, tnw, toff,
                       l.dense, l.tinfo);
  if (ok) ok = hipStreamSynchronize(g->st) == hipSuccess;
  l.n_jobs = 0;
  if (ok && n_tiles) {
    std::vector<unsigned> h_nw(n_tiles);
    ok = hipMemcpy(h_nw.data(), tnw, 4 * (size_t)n_tiles, hipMemcpyDeviceToHost) == hipSuccess && stb_lists_jobs_from(g, which, D, gg, h_nw.data()) == 0;
  }
  return ok;
}

// the lists of layout `which` (resolved, with its geometry H / gg) by sorting the pairs; returns what stb_lists_build returns
int stb_lists_sort_build(stb_groups_t *g, int which, int D, const hb_dot_info &H, const grid_geom &gg) {
  stb_cell_list &l = g->lists[which];
  const unsigned N = g->N, M = g->M;
  const uint64_t G = g->G;
  if (!g->fused_ready) g->sparse = 0;
  if (G == 0 || G >= 0xffffffffull) return 0;
  const unsigned nsg = (M + 63) / 64 + 4;
  const unsigned trips = (N - 2 + 7) / 8;
  const uint64_t nitems64 = (which >= 2) ? (uint64_t)H.n_rec * (unsigned)H.NQ : (uint64_t)trips * nsg;
  if (nitems64 >= (1ull << 31)) return 0;
  const unsigned nitems = (unsigned)nitems64;
  sort_scratch sc{g->st};
  uint64_t *k0 = nullptr, *k1 = nullptr, *uk = nullptr, *d_counts = nullptr;
  uint32_t *p0 = nullptr, *p1 = nullptr;
  unsigned *cnt = nullptr, *runs = nullptr, *item = nullptr;
  void *tmp = nullptr;
  const unsigned blocks = (unsigned)((G + 255) / 256);
  if (!sc.take(&k0, 8 * G) || !sc.take(&k1, 8 * G) || !sc.take(&p0, 4 * G) || !sc.take(&p1, 4 * G) || !sc.take(&uk, 8 * G) || !sc.take(&cnt, 4 * G) ||
      !sc.take(&item, 4 * G) || !sc.take(&runs, 64) || !sc.take(&d_counts, 64))
    return sort_failed("stb_groups_aterms: out of device memory");
  if (which >= 3)
    hipLaunchKernelGGL(k_item_keys_hb2, dim3(blocks), dim3(256), 0, g->st, g->d_n, g->d_t, G, N, M, H, stb_pos_bits(H.C), k0, p0);
  else if (which == 2)
    hipLaunchKernelGGL(k_item_keys_hb, dim3(blocks), dim3(256), 0, g->st, g->d_n, g->d_t, G, N, M, H, k0, p0);
  else
    hipLaunchKernelGGL(k_item_keys, dim3(blocks), dim3(256), 0, g->st, g->d_n, g->d_t, G, N, M, nsg, which ? 2u : 1u, k0, p0);
  size_t b1 = 0, b2 = 0;
  if (rocprim::radix_sort_pairs(nullptr, b1, k0, k1, p0, p1, (size_t)G, 0, 64, g->st) != hipSuccess) return sort_failed();
  if (rocprim::run_length_encode(nullptr, b2, k1, (unsigned)G, uk, cnt, runs, g->st) != hipSuccess) return sort_failed();
  const size_t tmp_bytes = b1 > b2 ? b1 : b2;
  if (!sc.take(&tmp, tmp_bytes ? tmp_bytes : 1)) return sort_failed("stb_groups_aterms: out of device memory");
  size_t bb = tmp_bytes;
  if (rocprim::radix_sort_pairs(tmp, bb, k0, k1, p0, p1, (size_t)G, 0, 64, g->st) != hipSuccess) return sort_failed();
  hipLaunchKernelGGL(k_key_bounds, dim3(1), dim3(1), 0, g->st, k1, G, d_counts);
  uint64_t h_counts[2] = {0, 0};
  if (hipMemcpyAsync(h_counts, d_counts, 16, hipMemcpyDeviceToHost, g->st) != hipSuccess || hipStreamSynchronize(g->st) != hipSuccess) return sort_failed();
  const uint64_t n_in = h_counts[0], n_other = h_counts[1];
  // dense enough that every cell's log might as well be computed: leave it to the count slab
  if (n_in * 3 > stb_table_cells(N, M)) return 0;
  // the pairs outside the table, in their sorted order (the same whichever layout is built first; the
  // self-summing form has none but those whose S_S is log 0, which it only counts)
  if (which >= 2) {
    g->n_inf = n_other;
  } else if (!g->d_n2) {
    g->G2 = n_other;
    if (stb_pool_malloc((void **)&g->d_n2, 4 * (n_other ? n_other : 1)) != hipSuccess || stb_pool_malloc((void **)&g->d_t2, 2 * (n_other ? n_other : 1)) != hipSuccess)
      return sort_failed("stb_groups_aterms: out of device memory");
    if (n_other)
      hipLaunchKernelGGL(k_gather_pairs, dim3((unsigned)((n_other + 255) / 256)), dim3(256), 0, g->st, g->d_n, g->d_t, p1 + n_in, n_other, g->d_n2, g->d_t2);
  }
  // distinct cells with their counts
  unsigned h_runs = 0;
  if (n_in) {
    bb = tmp_bytes;
    if (rocprim::run_length_encode(tmp, bb, k1, (unsigned)n_in, uk, cnt, runs, g->st) != hipSuccess) return sort_failed();
    if (hipMemcpyAsync(&h_runs, runs, 4, hipMemcpyDeviceToHost, g->st) != hipSuccess || hipStreamSynchronize(g->st) != hipSuccess) return sort_failed();
  } else if (hipMemsetAsync(runs, 0, 4, g->st) != hipSuccess) {
    return sort_failed();
  }
  // sized exactly: what another build sized -- the slab builder's capacity among it -- goes
  stb_list_release(l, false);
  if (stb_pool_malloc((void **)&l.ent_pos, 2 * (size_t)(h_runs ? h_runs : 1)) != hipSuccess || stb_pool_malloc((void **)&l.ent_cnt, 4 * (size_t)(h_runs ? h_runs : 1)) != hipSuccess ||
      stb_pool_malloc((void **)&l.item_ptr, 4 * ((size_t)nitems + 2)) != hipSuccess)
    return sort_failed("stb_groups_aterms: out of device memory");
  if (h_runs) {
    hipLaunchKernelGGL(k_split_runs, dim3((h_runs + 255) / 256), dim3(256), 0, g->st, uk, runs, l.ent_pos, item, which >= 3 ? stb_pos_bits(H.C) + 5 : (which == 2 ? 11 : 9));
    if (hipMemcpyAsync(l.ent_cnt, cnt, 4 * (size_t)h_runs, hipMemcpyDeviceToDevice, g->st) != hipSuccess) return sort_failed();
  }
  hipLaunchKernelGGL(k_item_ptr, dim3((nitems + 1 + 255) / 256), dim3(256), 0, g->st, item, runs, nitems, l.item_ptr);
  if (which >= 3 && !sort_dense_words(g, which, D, H, gg, nitems)) return sort_failed("stb_groups_aterms: out of device memory (or a dense list beyond 2^32 bytes)");
  if (!g->d_dotp && stb_groups_alloc_dotp(g)) return sort_failed();
  if (hipStreamSynchronize(g->st) != hipSuccess || hipGetLastError() != hipSuccess) return sort_failed();
  g->nsg = nsg;
  g->sparse = 1;
  l.ready = 1;
  l.R = H.R;
  l.G = H.G;
  g->fused_ready = 1;
  return 0;
}
