// lists.hip -- the cell lists of the fused evaluation (struct stb_cell_list, groups.h): their lifetime, the builder that
// makes them on the device from a COUNT SLAB without a sort and without a host round trip, the helper jobs of the grid
// form.  stb_lists_build is the way in; where the slab builder does not apply, lists_sorted.hip's sort-based one does.
//
// Why.  The reference's callers change the counts between two samplea calls (test/demo.c:405-445 rewrites t[j][i] and
// T[j] in every Gibbs iteration, then :478-480 resamples a): a set of pairs is used for ONE samplea call, i.e. ~8
// posterior evaluations, and whatever is done once per set is paid on every call.  Rounds 2-4 sorted the pairs twice
// per set (rocPRIM: 23 launches, 0.24 ms, by (n,t) for the gather; 21 launches + run-length encoding, 0.33 ms, by
// (tile, group, cell) for the lists of the fused form) with four host round trips in between, and the host copied the
// ragged arrays twice: 3.1-3.8 ms a call where an unchanged set took 1.57.  The copies: pairs.hip.  Here:
//   * the lists come from a COUNT SLAB: one word per cell of every (tile, group of rows) item in the order the walk
//     looks cells up, i.e. the table's cells once over (33 MB for N = M = 4096, 205 MB for 10^4), zero between builds.
//     k_count_cells adds every pair to its word -- ONE device-scope atomic per pair: this part hands out 24 G of them a
//     second whatever they return and however large the slab (tools/ubench/scatter.hip: 42 us for 10^6), an integer, so
//     the result does not depend on the order of the pairs; k_item_count reads the slab for every item's distinct cells;
//     a prefix sum of those is the CSR row pointer; k_emit_cells has a wave per item compact the item's words -- in position
//     order, the order the sort produced, so the lists are THE SAME BYTES as the sort-based builder's -- and puts every
//     word it read back to zero: the slab is clean for the next set without a memset.  For the grid form the prefix sums and
//     the tiles' entries are one single-workgroup kernel (k_scan_lists), the compaction writes the dense words the walk
//     reads along with the CSR entries (k_emit_both), and the tiles left to helper jobs are chosen by k_jobs_build,
//     which leaves their number in the list for the kernels to read.  No host synchronisation anywhere: the
//     evaluation is queued right behind (N = 4096, halo-block form: 75 us; N = 10^4, grid form: 166 us; the radix sort +
//     run-length encoding they replace: 330-600 us and four host round trips).
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "groups.h"

// ------------------------------------------------------------------------------------------------
// count slab -> CSR lists

// the word of the slab a pair falls on: 0 nothing (n <= 1 or t = n: log 1), 1 its S_S is log 0 (lib/stable.c:948-949), 2 a cell
__device__ __forceinline__ int slab_word(unsigned nn, unsigned tt, unsigned N, unsigned M, const slab_info &H, unsigned &item, size_t &idx) {
  if (nn <= 1 || nn == tt) return 0;
  if (tt == 0 || nn < tt || tt > M || nn > N) return 1;
  unsigned j = 0, col = 0;  // t = 1: the last element of strip 0's halo, word 0 of the row
  if (tt >= 2) {
    const unsigned e = tt - 2;
    j = e / (unsigned)H.UC;
    col = 1 + (e - j * (unsigned)H.UC);
  }
  const unsigned b = (nn - 2) / (unsigned)H.R, r = (nn - 2) - b * (unsigned)H.R;
  const unsigned b0 = (j * (unsigned)H.UC) / (unsigned)H.R;  // (j < 2^16, UC <= 256)
  const unsigned rec = H.rec_off[j + 1] + (b - b0);  // (b >= b0: the cell lies on or below the diagonal)
  const unsigned q = r / (unsigned)H.G;
  item = rec * (unsigned)H.NQ + q;
  idx = ((size_t)item * (unsigned)H.G + (r - q * (unsigned)H.G)) * H.UCp + col;
  return 2;
}

// (device-scope atomics run at 24 G a second on this part whatever they return and however large the slab
// -- tools/ubench/scatter.hip, profiles/r05_ubench_scatter.txt: 42 us for 10^6 -- so there is ONE per pair: the items'
// distinct cells are counted from the slab afterwards, by reading it)
__global__ __launch_bounds__(256) void k_count_cells(const uint32_t *n, const uint16_t *t, uint64_t G, unsigned N, unsigned M, slab_info H,
                                                     unsigned *slab, unsigned long long *ninf) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int kind = 0;
  unsigned item = 0;
  size_t idx = 0;
  if (g < G) kind = slab_word(n[g], t[g], N, M, H, item, idx);
  if (kind == 2) __hip_atomic_fetch_add(&slab[idx], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long m = __ballot(kind == 1);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(ninf, (unsigned long long)__popcll(m));
}

// a wave per item: how many of its words are not zero
__global__ __launch_bounds__(256) void k_item_count(const unsigned *slab, unsigned nitems, unsigned len, unsigned *icnt) {
  const unsigned item = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (item >= nitems) return;
  const unsigned *w = slab + (size_t)item * len;
  unsigned c = 0;
  unsigned k = lane * 4;
  // (four words a lane and load while the item's start is 16-byte aligned -- len is odd for most shapes: word by word then)
  if ((((size_t)item * len) & 3u) == 0) {
    for (; k + 3 < len; k += 256) {
      const uint4 v = *reinterpret_cast<const uint4 *>(w + k);
      c += (v.x != 0u) + (v.y != 0u) + (v.z != 0u) + (v.w != 0u);
    }
    for (unsigned i = (len & ~3u) + lane; i < len; i += 64) c += w[i] != 0u;
  } else {
    for (unsigned i = lane; i < len; i += 64) c += w[i] != 0u;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0) icnt[item] = c;
}

// a wave per item: its words, in order, become its list; what was read goes back to zero.  A lane takes four
// consecutive words a step (one 16-byte load where the item starts on a 16-byte boundary: its length is a multiple of 8
// words), the next step's load in flight while this one's words are placed; the order of the entries is the order of the
// words.
__global__ __launch_bounds__(256) void k_emit_cells(unsigned *slab, const unsigned *item_ptr, unsigned nitems, slab_info H, unsigned short *ent_pos,
                                                    unsigned *ent_cnt) {
  const unsigned item = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (item >= nitems) return;
  unsigned out = item_ptr[item];
  const unsigned end = item_ptr[item + 1];
  if (out == end) return;  // (nothing of this item occurs: its words are zero, nobody reads them)
  const unsigned len = (unsigned)H.G * H.UCp;
  unsigned *w = slab + (size_t)item * len;
  const unsigned long long below = (1ull << lane) - 1ull;
  if ((((size_t)item * len) & 3u) == 0 && (len & 3u) == 0) {
    auto load4 = [&](unsigned i) -> uint4 { return (i + 3 < len) ? *reinterpret_cast<const uint4 *>(w + i) : uint4{0u, 0u, 0u, 0u}; };
    uint4 nx = load4(lane * 4);
    for (unsigned k = 0; k < len && out < end; k += 256) {
      const unsigned i = k + lane * 4;
      const uint4 c = nx;
      if (k + 256 < len) nx = load4(i + 256);
      const unsigned cc[4] = {c.x, c.y, c.z, c.w};
      // entries before this lane's first word: the non-zero words of the lanes below it
      const unsigned mine = (cc[0] != 0u) + (cc[1] != 0u) + (cc[2] != 0u) + (cc[3] != 0u);
      unsigned before = 0, total = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const unsigned long long m = __ballot(cc[j] != 0u);
        before += (unsigned)__popcll(m & below);
        total += (unsigned)__popcll(m);
      }
      if (mine) {
        unsigned o = out + before;
        bool any = false;
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (cc[j] != 0u) {
            const unsigned ii = i + j, r = ii / H.UCp, col = ii - r * H.UCp;
            ent_pos[o] = (unsigned short)((r << H.PB) | ((unsigned)H.HC - 1u + col));
            ent_cnt[o] = cc[j];
            o++;
            any = true;
          }
        if (any) *reinterpret_cast<uint4 *>(w + i) = uint4{0u, 0u, 0u, 0u};
      }
      out += total;
    }
    return;
  }
  // (an item that does not start on a 16-byte boundary: word by word, two pieces of 64 words in flight)
  unsigned c0 = (lane < len) ? w[lane] : 0u;
  for (unsigned k = 0; k < len && out < end; k += 64) {
    const unsigned i = k + lane;
    const unsigned c = c0;
    if (k + 64 < len) c0 = (i + 64 < len) ? w[i + 64] : 0u;
    const unsigned long long m = __ballot(c != 0u);
    if (c != 0u) {
      const unsigned o = out + (unsigned)__popcll(m & below);
      const unsigned r = i / H.UCp, col = i - r * H.UCp;
      ent_pos[o] = (unsigned short)((r << H.PB) | ((unsigned)H.HC - 1u + col));
      ent_cnt[o] = c;
      w[i] = 0u;
    }
    out += (unsigned)__popcll(m);
  }
}

// ---- the grid form: CSR lists AND the dense words the walk reads, in one pass over the slab ----
// One workgroup: the exclusive scan of the items' distinct cells (the CSR row pointer) and, per tile, the words per lane
// its groups get in the dense layout (the most any of them needs; 63: more than the layout takes, the tile is read from
// the CSR lists), their prefix sum and the tile's entry -- what two library scans, k_tile_words and a launch gap did.
__global__ __launch_bounds__(1024) void k_scan_lists(const unsigned *icnt, unsigned nitems, unsigned n_tiles, unsigned NQ, unsigned *item_ptr, unsigned *tnw,
                                                     unsigned *toff, unsigned *tinfo) {
  __shared__ unsigned s_scan[17];
  const unsigned tid = threadIdx.x;
  auto block_exclusive = [&](unsigned mine) -> unsigned { return stb_block_exclusive_1024(mine, s_scan, nullptr); };
  {
    const unsigned per = (nitems + 1 + 1023u) / 1024u, i0 = tid * per, i1 = min(i0 + per, nitems + 1);
    unsigned sum = 0;
    for (unsigned i = i0; i < i1; i++) sum += (i < nitems) ? icnt[i] : 0u;
    unsigned run = block_exclusive(sum);
    for (unsigned i = i0; i < i1; i++) {
      item_ptr[i] = run;
      run += (i < nitems) ? icnt[i] : 0u;
    }
  }
  {
    const unsigned per = (n_tiles + 1023u) / 1024u, t0 = tid * per, t1 = min(t0 + per, n_tiles);
    unsigned sum = 0;
    for (unsigned t = t0; t < t1; t++) {
      unsigned nw = 0;
      for (unsigned q = 0; q < NQ; q++) nw = max(nw, (icnt[(size_t)t * NQ + q] + 63u) / 64u);
      if (nw > STB_DENSE_NWMAX) nw = 63u;
      tnw[t] = nw;
      sum += (nw == 63u) ? 0u : nw * NQ;
    }
    unsigned run = block_exclusive(sum);
    for (unsigned t = t0; t < t1; t++) {
      const unsigned nw = tnw[t];
      toff[t] = run;
      tinfo[t] = (run << 6) | nw;
      run += (nw == 63u) ? 0u : nw * NQ;
    }
  }
}

// a wave per item, as k_emit_cells; every entry also goes to its place among the tile's dense words (position | count <<
// wbits, group q of the tile at words [first + q NW, first + (q + 1) NW) x 64 lanes, filled from the front, zeros behind).
// A count that does not fit a word marks its tile as one read from the CSR lists (NW := 63).
__global__ __launch_bounds__(256) void k_emit_both(unsigned *slab, const unsigned *item_ptr, unsigned nitems, slab_info H, unsigned short *ent_pos, unsigned *ent_cnt,
                                                   unsigned NQ, int wbits, unsigned *tnw, const unsigned *toff, unsigned *tinfo, unsigned *dense) {
  const unsigned item = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (item >= nitems) return;
  const unsigned tile = item / NQ, q = item - tile * NQ;
  const unsigned first = item_ptr[item], end = item_ptr[item + 1];
  const unsigned nw = tinfo[tile] & 63u;  // (as k_scan_lists left it: another wave's "63" for a big count comes later or never)
  unsigned *dw = (nw != 0u && nw != 63u) ? dense + ((size_t)toff[tile] + (size_t)q * nw) * 64 : nullptr;
  const unsigned room = nw * 64u;
  if (first != end) {
    unsigned out = first;
    const unsigned len = (unsigned)H.G * H.UCp;
    unsigned *w = slab + (size_t)item * len;
    const unsigned long long below = (1ull << lane) - 1ull;
    const bool wide = (((size_t)item * len) & 3u) == 0 && (len & 3u) == 0;
    auto place = [&](unsigned o, unsigned ii, unsigned c) {
      const unsigned r = ii / H.UCp, col = ii - r * H.UCp;
      const unsigned pos = (r << H.PB) | ((unsigned)H.HC - 1u + col);
      ent_pos[o] = (unsigned short)pos;
      ent_cnt[o] = c;
      if (dw) dw[o - first] = pos | (c << wbits);
      if (c >= (1u << (32 - wbits))) {  // (does not fit a dense word: this tile is read from the CSR lists)
        atomicOr(&tinfo[tile], 63u);
        atomicMax(&tnw[tile], 63u);
      }
    };
    if (wide) {
      auto load4 = [&](unsigned i) -> uint4 { return (i + 3 < len) ? *reinterpret_cast<const uint4 *>(w + i) : uint4{0u, 0u, 0u, 0u}; };
      uint4 nx = load4(lane * 4);
      for (unsigned k = 0; k < len && out < end; k += 256) {
        const unsigned i = k + lane * 4;
        const uint4 c = nx;
        if (k + 256 < len) nx = load4(i + 256);
        const unsigned cc[4] = {c.x, c.y, c.z, c.w};
        unsigned before = 0, total = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const unsigned long long m = __ballot(cc[j] != 0u);
          before += (unsigned)__popcll(m & below);
          total += (unsigned)__popcll(m);
        }
        if ((cc[0] | cc[1] | cc[2] | cc[3]) != 0u) {
          unsigned o = out + before;
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (cc[j] != 0u) place(o++, i + j, cc[j]);
          *reinterpret_cast<uint4 *>(w + i) = uint4{0u, 0u, 0u, 0u};
        }
        out += total;
      }
    } else {
      for (unsigned k = 0; k < len && out < end; k += 64) {
        const unsigned i = k + lane;
        const unsigned c = (i < len) ? w[i] : 0u;
        const unsigned long long m = __ballot(c != 0u);
        if (c != 0u) {
          place(out + (unsigned)__popcll(m & below), i, c);
          w[i] = 0u;
        }
        out += (unsigned)__popcll(m);
      }
    }
  }
  // the words behind the group's last cell: zero (the first empty word ends a group's look-ups)
  if (dw)
    for (unsigned k = (end - first) + lane; k < room; k += 64) dw[k] = 0u;
}

static void free_z(void *&p) {
  stb_pool_free(p);
  p = nullptr;
}
#define FREE_Z(x) free_z(reinterpret_cast<void *&>(x))

void stb_list_release(stb_cell_list &l, bool with_shape) {
  void **sized[] = {(void **)&l.item_ptr, (void **)&l.ent_pos, (void **)&l.ent_cnt, (void **)&l.dense, (void **)&l.tinfo, (void **)&l.jobs, (void **)&l.tjob};
  for (void **p : sized) free_z(*p);
  l.ent_cap = l.dense_cap = 0;
  if (!with_shape) return;
  void **shaped[] = {(void **)&l.tile_off, (void **)&l.tnw, (void **)&l.toff};
  for (void **p : shaped) free_z(*p);
  l.n_jobs = 0;
  l.ready = 0;
}

// New pairs (keep_capacity) or new table bounds: what was built from the old ones goes.  With keep_capacity the buffers
// the slab builder sized for the most a set of G pairs can need stay; those the sort-based builder sized exactly go.
void stb_lists_drop(stb_groups_t *g, bool keep_capacity) {
  for (stb_cell_list &l : g->lists) {
    if (!keep_capacity || !stb_list_from_slab(l)) stb_list_release(l, true);
    l.ready = 0;
    l.n_jobs = 0;
  }
  // the forms that read the pairs outside the table and the dense count slab of the chain form
  FREE_Z(g->d_n2);
  FREE_Z(g->d_t2);
  FREE_Z(g->d_cnt);
  g->G2 = 0;
  g->n_inf = 0;
  g->fused_ready = 0;
  g->sparse = 0;
  if (!keep_capacity) {
    FREE_Z(g->d_slab);
    FREE_Z(g->d_icnt);
    FREE_Z(g->d_scan_tmp);
    FREE_Z(g->d_dotp);
    g->slab_elems = 0;
    g->slab_which = 0;
    g->scan_tmp_bytes = 0;
    g->dotp_elems = 0;
  }
}

// the list of layout `which` as a launcher takes it, with the strip shape it was built for (halo-block and grid forms)
void stb_list_request(const stb_groups_t *g, int which, dot_request *req) {
  const stb_cell_list &l = g->lists[which];
  req->item_ptr = l.item_ptr;
  req->ent_pos = l.ent_pos;
  req->ent_cnt = l.ent_cnt;
  req->nsg = g->nsg;
  req->col0 = which >= 3 ? 4 : which + 1;
  if (which == 2) req->geom_C = g->hb_sum_C;  // (the strip shape the set's lists were built for)
  if (which >= 3) {
    req->geom_C = stb_which_C(which);
    req->geom_R = l.R;
    req->geom_G = l.G;
    req->tile_off = l.tile_off;
    req->dense = l.dense;
    req->tinfo = l.tinfo;
    req->jobs = l.jobs;
    req->tjob = l.tjob;
  }
}

static size_t slab_limit_bytes() { return (size_t)stb_env_int("STB_SLAB_MB", 4096) << 20; }

// Returns 0 with the lists of layout `which` queued on the set's stream (the list is ready: an evaluation may be queued
// behind them), 2 when this builder does not apply (the caller takes the sort-based one), 1 on error.
int stb_lists_slab_build(stb_groups_t *g, int which, int D, const hb_dot_info &H, const grid_geom &gg) {
  if (which < 2 || !stb_env_int("STB_LISTS_SLAB", 1)) return 2;
  stb_cell_list &l = g->lists[which];
  const unsigned N = g->N, M = g->M;
  const uint64_t G = g->G;
  if (G == 0 || G >= 0xffffffffull) return 2;
  // (pairs that could fill a third of the table: the sort-based builder decides by the distinct cells whether the
  // count slab of the chain form serves better)
  if (G * 3 > stb_table_cells(N, M)) return 2;
  slab_info S;
  S.R = H.R;
  S.G = H.G;
  S.NQ = H.NQ;
  S.UC = H.UC;
  S.HC = H.HC;
  S.UCp = (unsigned)H.UC + 1u;
  S.rec_off = H.rec_off;
  const uint64_t nitems64 = (uint64_t)H.n_rec * (unsigned)H.NQ;
  const uint64_t elems64 = nitems64 * (unsigned)H.G * S.UCp;
  if (nitems64 >= (1ull << 31) || elems64 * 4 > slab_limit_bytes()) return 2;
  S.PB = which >= 3 ? stb_pos_bits(H.C) : 8;
  if (H.G > 32 || H.HC - 1 + (int)S.UCp > (1 << S.PB)) return 2;  // (a position is row << PB | element)
  // (the grid form's dense words are sized for the worst case; where that is beyond a 32-bit offset the sort-based builder,
  // which sizes exactly, takes over -- decided here, before anything is queued)
  if (which >= 3 && (size_t)H.NQ * ((size_t)(g->G / 64) + H.n_tiles + 1) >= (1u << 26)) return 2;
  const unsigned nitems = (unsigned)nitems64;
  const size_t elems = (size_t)elems64;
  hipStream_t st = g->st;
  // the slab: laid out for ONE layout at a time (a set is evaluated in one form call after call; another form asks
  // for another slab)
  if (!g->d_slab || g->slab_elems < elems || g->slab_which != which || g->slab_R != H.R || g->slab_G != H.G || g->slab_UCp != (int)S.UCp ||
      g->slab_items != nitems) {
    if (g->d_slab) HIPCHK(hipStreamSynchronize(st));
    if (!g->d_slab || g->slab_elems < elems) {
      FREE_Z(g->d_slab);
      g->slab_elems = 0;
      if (stb_pool_malloc((void **)&g->d_slab, 4 * elems) != hipSuccess) return stb_fail("stb_groups_aterms: out of device memory (count slab, %zu MB)", (4 * elems) >> 20);
      g->slab_elems = elems;
      g->slab_clean = 0;
    }
    FREE_Z(g->d_icnt);
    if (stb_pool_malloc((void **)&g->d_icnt, 4 * ((size_t)nitems + 2)) != hipSuccess || (!g->d_ninf && stb_pool_malloc((void **)&g->d_ninf, 64) != hipSuccess))
      return stb_fail("stb_groups_aterms: out of device memory");
    HIPCHK(hipMemsetAsync(g->d_icnt, 0, 4 * ((size_t)nitems + 2), st));
    size_t need = 0;
    if (rocprim::exclusive_scan(nullptr, need, g->d_icnt, g->d_icnt, 0u, (size_t)nitems + 1, rocprim::plus<unsigned>(), st) != hipSuccess)
      return stb_fail("stb_groups_aterms: exclusive_scan (size query) failed");
    if (which >= 3) {  // (... and the scan over the tiles' word counts)
      size_t need2 = 0;
      if (rocprim::exclusive_scan(nullptr, need2, g->d_icnt, g->d_icnt, 0u, (size_t)H.n_tiles + 1, rocprim::plus<unsigned>(), st) != hipSuccess)
        return stb_fail("stb_groups_aterms: exclusive_scan (size query) failed");
      if (need2 > need) need = need2;
    }
    if (need > g->scan_tmp_bytes) {
      FREE_Z(g->d_scan_tmp);
      if (stb_pool_malloc(&g->d_scan_tmp, need ? need : 1) != hipSuccess) return stb_fail("stb_groups_aterms: out of device memory");
      g->scan_tmp_bytes = need ? need : 1;
    }
    g->slab_which = which;
    g->slab_R = H.R;
    g->slab_G = H.G;
    g->slab_UCp = (int)S.UCp;
    g->slab_items = nitems;
  }
  if (!g->slab_clean) HIPCHK(hipMemsetAsync(g->d_slab, 0, 4 * g->slab_elems, st));
  // the list buffers, for the most G pairs can ask for
  if (l.ent_cap < G || !l.item_ptr) {
    if (l.ent_pos) HIPCHK(hipStreamSynchronize(st));
    FREE_Z(l.ent_pos);
    FREE_Z(l.ent_cnt);
    FREE_Z(l.item_ptr);
    if (stb_pool_malloc((void **)&l.ent_pos, 2 * (size_t)G + 256) != hipSuccess || stb_pool_malloc((void **)&l.ent_cnt, 4 * (size_t)G + 256) != hipSuccess ||
        stb_pool_malloc((void **)&l.item_ptr, 4 * ((size_t)nitems + 2)) != hipSuccess)
      return stb_fail("stb_groups_aterms: out of device memory");
    l.ent_cap = (size_t)G;
  }
  g->slab_clean = 0;
  // (counting the pieces of a hand-over while the next ones still arrive -- on the guess that layout and bounds stay --
  // was built and measured: in the copies' stream the DMA engine waits for every count, the hand-over ends 55 us LATER; on a
  // stream of its own it ends 20 us later still (tools/ab_spec.py in the history of this file): removed)
  HIPCHK(hipMemsetAsync(g->d_ninf, 0, 8, st));
  hipLaunchKernelGGL(k_count_cells, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, st, g->d_n, g->d_t, G, N, M, S, g->d_slab, g->d_ninf);
  hipLaunchKernelGGL(k_item_count, dim3((nitems + 3) / 4), dim3(256), 0, st, g->d_slab, nitems, (unsigned)H.G * S.UCp, g->d_icnt);
  // (the log-0 pairs of a layout built here are counted on the device, d_ninf, and added by k_eval_tail to g->n_inf, which
  // is what a layout built by the sort counted on the host and stays: the two may count the same pairs twice, which is
  // still "not zero"; stb_lists_drop zeroes it with the pairs)
  if (which < 3) {
    size_t tb = g->scan_tmp_bytes;
    if (rocprim::exclusive_scan(g->d_scan_tmp, tb, g->d_icnt, l.item_ptr, 0u, (size_t)nitems + 1, rocprim::plus<unsigned>(), st) != hipSuccess)
      return stb_fail("stb_groups_aterms: exclusive_scan failed");
    hipLaunchKernelGGL(k_emit_cells, dim3((nitems + 3) / 4), dim3(256), 0, st, g->d_slab, l.item_ptr, nitems, S, l.ent_pos,
                       l.ent_cnt);
    HIPCHK(hipGetLastError());
    g->slab_clean = 1;  // (once the stream has come this far; every later use is queued behind it)
  } else {
    // the grid form: CSR lists and the dense words the walk reads in ONE pass over the slab, the scans by one workgroup,
    // then the tiles left to helper jobs -- all on the device, the evaluation queued right behind
    const unsigned n_tiles = H.n_tiles, NQ = (unsigned)H.NQ;
    const size_t words_cap = (size_t)NQ * ((size_t)(G / 64) + n_tiles + 1);  // in units of 64 words: sum over tiles of NQ * ceil(most cells of a group / 64)
    if (words_cap >= (1u << 26)) return stb_fail("stb_groups_aterms: a dense list beyond 2^32 bytes");
    {
      unsigned **bufs[] = {&l.tnw, &l.toff, &l.tinfo};
      for (unsigned **q : bufs)
        if (!*q && stb_pool_malloc((void **)q, 4 * (size_t)(n_tiles + 2)) != hipSuccess) return stb_fail("stb_groups_aterms: out of device memory");
    }
    if (l.dense_cap < words_cap || !l.dense) {
      if (l.dense) HIPCHK(hipStreamSynchronize(st));
      FREE_Z(l.dense);
      if (stb_pool_malloc((void **)&l.dense, 256 * words_cap) != hipSuccess) return stb_fail("stb_groups_aterms: out of device memory");
      l.dense_cap = words_cap;
    }
    hipLaunchKernelGGL(k_scan_lists, dim3(1), dim3(1024), 0, st, g->d_icnt, nitems, n_tiles, NQ, l.item_ptr, l.tnw, l.toff,
                       l.tinfo);
    hipLaunchKernelGGL(k_emit_both, dim3((nitems + 3) / 4), dim3(256), 0, st, g->d_slab, l.item_ptr, nitems, S, l.ent_pos,
                       l.ent_cnt, NQ, S.PB + 5, l.tnw, l.toff, l.tinfo, l.dense);
    HIPCHK(hipGetLastError());
    g->slab_clean = 1;
    if (stb_lists_jobs_device(g, which, D, gg, l.tnw)) return 1;
  }
  if (!g->d_dotp && stb_groups_alloc_dotp(g)) return 1;
  g->sparse = 1;
  l.ready = 1;
  l.R = H.R;
  l.G = H.G;
  g->fused_ready = 1;
  g->nsg = (M + 63) / 64 + 4;
  return 0;
}

// ---- the grid form's helper jobs.  The tiles whose listed cells the strip's own wave does not look up: every strip of a table moves at the pace of
// the strips to its left, and those hold most of the pairs (t uniform below n: columns like log) -- several
// passes a group where the average strip has one.  Such a tile is only walked by its strip, which leaves the
// state of its wave before the block as a record; waves whose strips the diagonal has not reached yet take the
// tiles as jobs once their own strips have ended.  Which: all tiles of NWH passes a group and more (the lists in CSR
// form among them), NWH chosen here (returned) and raised until the records fit (grid_geom::job_cap at Dmax discounts);
// *jlim: the strips from the left that may have jobs.
static unsigned jobs_rule(const grid_geom &gg, int D, int *jlim) {
  // NWH at the least: what a job takes off the critical path it adds to the chip's work (the tile is walked twice),
  // which the fuller chip can afford less (MI355X, 10^6 pairs, N = 10^4, kernel ms without jobs / NWH = 3 / 4 / 6 /
  // 8 / 12: 32 discounts 1.21 / 1.00 / 0.96 / 1.01 / 1.04 / 1.09, 40: 1.26 / 1.10 / 1.02 / 1.05 / 1.08 / 1.12,
  // 48: 1.26 / 1.30 / 1.14 / 1.09 / 1.10 / 1.15, 64: 1.36 / 1.59 / 1.39 / 1.29 / 1.28 / 1.29)
  unsigned nwh = (unsigned)stb_env_int("STB_GRID_HELP_NW", 0);
  if (nwh < 1) {
    const double waves_per_simd = (double)gg.JW * D / (4.0 * stb_cu_count());
    nwh = waves_per_simd <= 1.9 ? 4 : (waves_per_simd <= 2.7 ? 6 : 8);
  }
  // (a job is taken by a wave of a workgroup further right -- one with a higher ticket, for which the strip's own
  // workgroup is running or through: the strips of a table's last workgroup have no jobs; GH_JQ = 64 queues)
  *jlim = ((gg.JW - 1) / gg.P) * gg.P;
  if (*jlim > 64) *jlim = 64;
  return nwh;
}
// room for the most jobs there can be, kept from set to set
static int jobs_room(stb_cell_list &l, unsigned n_tiles) {
  if (!l.jobs && stb_pool_malloc((void **)&l.jobs, 4 * ((size_t)n_tiles + 128 + 1)) != hipSuccess) return stb_fail("stb_groups_aterms: out of device memory");
  if (!l.tjob && stb_pool_malloc((void **)&l.tjob, 4 * (size_t)(n_tiles + 1)) != hipSuccess) return stb_fail("stb_groups_aterms: out of device memory");
  return 0;
}

// The choice made ON the device (round 5: a set whose pairs are new gets its lists without a host round trip): one
// workgroup; the tiles' words per group in, the job list in the layout of grid_hb.hip out (queue starts, number of jobs,
// jobs in tile order = strip after strip, a strip's by block) together with every tile's place in it.
__global__ __launch_bounds__(1024) void k_jobs_build(const unsigned *tnw, unsigned n_tiles, const unsigned *tile_off, int JW, int jlim, int R, int UC, int NB,
                                                     unsigned cap, unsigned nwh0, unsigned *jobs, unsigned *tjob) {
  __shared__ unsigned hist[64], s_nwh, s_scan[17], s_off[1024];
  const unsigned tid = threadIdx.x;
  if (tid < 64) hist[tid] = 0;
  // (the strips' first tiles, looked at a dozen times per tile below: in LDS where they fit)
  const bool off_lds = JW + 2 <= 1024;
  if (off_lds)
    for (int i = (int)tid; i < JW + 2; i += 1024) s_off[i] = tile_off[i];
  __syncthreads();
  const unsigned *toffp = off_lds ? s_off : tile_off;
  for (unsigned t = tid; t < n_tiles; t += 1024) atomicAdd(&hist[min(tnw[t], 63u)], 1u);
  __syncthreads();
  if (tid == 0) {
    // the smallest threshold from nwh0 on whose tiles fit (the tiles at or above a threshold grow as it falls): one pass
    // from the top; 64 = none fits
    unsigned nwh = 64, c = 0;
    for (int k = 63; k >= (int)nwh0; k--) {
      c += hist[k];
      if (c > cap) break;
      nwh = (unsigned)k;
    }
    s_nwh = nwh;
  }
  __syncthreads();
  const unsigned nwh = s_nwh;
  // strip of a tile: tile_off[j + 1] is the first tile of strip j (entry 0 holds the total)
  auto strip_of = [&](unsigned t) -> int {
    int lo = 0, hi = JW - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) / 2;
      if (toffp[mid + 1] <= t) lo = mid;
      else hi = mid - 1;
    }
    return lo;
  };
  const int jend = JW < jlim ? JW : jlim;  // strips that may have jobs
  const unsigned per = (n_tiles + 1023u) / 1024u, t0 = tid * per, t1 = min(t0 + per, n_tiles);
  unsigned mine = 0;
  if (nwh <= 63)
    for (unsigned t = t0; t < t1; t++) mine += (tnw[t] >= nwh && strip_of(t) < jend) ? 1u : 0u;
  unsigned total = 0;
  unsigned k = stb_block_exclusive_1024(mine, s_scan, &total);
  for (unsigned t = t0; t < t1; t++) {
    const int j = strip_of(t);
    if (t == toffp[j + 1] && j <= GH_JQ_HOST) jobs[j] = (j < jend) ? k : total;  // the first tile of strip j: its queue starts here
    if (nwh <= 63 && tnw[t] >= nwh && j < jend) {
      const int b = (int)(((long long)j * UC) / R) + (int)(t - toffp[j + 1]);
      jobs[128 + k] = (unsigned)j | ((unsigned)b << 16);
      tjob[t] = k;
      k++;
    } else {
      tjob[t] = 0xffffffffu;
    }
  }
  // queue starts of the strips there are not (or that may have no jobs), and the number of jobs
  for (int j = (int)tid; j <= GH_JQ_HOST; j += 1024)
    if (j >= jend) jobs[j] = total;
  if (tid == 0) jobs[GH_JQ_HOST + 1] = total;
}

// queued on the set's stream behind the kernels that produced `tnw`; no host synchronisation
int stb_lists_jobs_device(stb_groups_t *g, int which, int D, const grid_geom &gg, const unsigned *tnw) {
  stb_cell_list &l = g->lists[which];
  const unsigned n_tiles = gg.n_tiles;
  l.n_jobs = 0;
  const unsigned cap = stb_grid_job_cap(gg.C, g->Dmax, n_tiles, gg.phases);
  if (!cap || !n_tiles) {
    if (l.jobs) HIPCHK(hipMemsetAsync(l.jobs, 0, 4 * 128, g->st));
    return 0;
  }
  int jlim;
  const unsigned nwh = jobs_rule(gg, D, &jlim);
  if (jobs_room(l, n_tiles)) return 1;
  hipLaunchKernelGGL(k_jobs_build, dim3(1), dim3(1024), 0, g->st, tnw, n_tiles, l.tile_off, gg.JW, jlim, gg.R, gg.U * gg.C, gg.NB, cap, nwh, l.jobs, l.tjob);
  HIPCHK(hipGetLastError());
  l.n_jobs = cap;  // (at most; the number itself stays on the device)
  return 0;
}

// The same choice on the host, for the sort-based builder.  h_nw: words per group of every tile (host).  The lists go to
// the device on the set's stream.
int stb_lists_jobs_from(stb_groups_t *g, int which, int D, const grid_geom &gg, const unsigned *h_nw) {
  stb_cell_list &l = g->lists[which];
  const unsigned n_tiles = gg.n_tiles;
  l.n_jobs = 0;
  const unsigned cap = stb_grid_job_cap(gg.C, g->Dmax, n_tiles, gg.phases);
  if (!cap || !n_tiles) {
    // (no jobs: a list left by an earlier build must say so -- the kernels read the number of jobs from it)
    if (l.jobs && (hipMemsetAsync(l.jobs, 0, 4 * 128, g->st) != hipSuccess || hipStreamSynchronize(g->st) != hipSuccess))
      return stb_fail("stb_groups_aterms: %s", hipGetErrorString(hipGetLastError()));
    return 0;
  }
  unsigned hist[65] = {0};  // (an upper bound: the tiles of all strips)
  for (unsigned t = 0; t < n_tiles; t++) hist[h_nw[t] > 63 ? 63 : h_nw[t]]++;
  int jlim;
  unsigned nwh = jobs_rule(gg, D, &jlim);
  for (; nwh <= 63; nwh++) {
    unsigned c = 0;
    for (unsigned k = nwh; k <= 63; k++) c += hist[k];
    if (c <= cap) break;
  }
  std::vector<unsigned> jobs, tjob(n_tiles, 0xffffffffu), off;
  stb_grid_tile_offsets(gg, off);
  const int UCg = gg.U * gg.C;
  std::vector<unsigned> qoff(64 + 1, 0u);
  if (nwh <= 63) {
    // strip after strip, a strip's tiles by block: a queue per strip
    for (int j = 0; j < gg.JW && j < jlim; j++) {
      const int b00 = (int)(((long long)j * UCg) / gg.R);
      qoff[j] = (unsigned)jobs.size();
      for (int b = b00; b < gg.NB; b++)
        if (h_nw[off[j + 1] + (unsigned)(b - b00)] >= nwh) {
          tjob[off[j + 1] + (unsigned)(b - b00)] = (unsigned)jobs.size();
          jobs.push_back((unsigned)j | ((unsigned)b << 16));
        }
    }
    for (int j = (gg.JW < jlim ? gg.JW : jlim); j <= 64; j++) qoff[j] = (unsigned)jobs.size();
    if (jobs.size() > cap) {  // (the bound above counted every strip's tiles: cannot happen)
      jobs.clear();
      std::fill(tjob.begin(), tjob.end(), 0xffffffffu);
      std::fill(qoff.begin(), qoff.end(), 0u);
    }
  }
  const size_t nj = jobs.size();
  {
    // the list as the kernels read it (grid_hb.hip: GH_JQ + 1 queue starts, the number of jobs at word 65, jobs from word 128)
    std::vector<unsigned> lay(128, 0u);
    for (int j = 0; j <= 64; j++) lay[(size_t)j] = qoff[(size_t)j];
    lay[65] = (unsigned)nj;
    lay.insert(lay.end(), jobs.begin(), jobs.end());
    jobs.swap(lay);
  }
  // (the copies are synchronous: the vectors above go away)
  if (jobs_room(l, n_tiles)) return 1;
  if (hipMemcpyAsync(l.tjob, tjob.data(), 4 * (size_t)n_tiles, hipMemcpyHostToDevice, g->st) != hipSuccess ||
      hipMemcpyAsync(l.jobs, jobs.data(), 4 * jobs.size(), hipMemcpyHostToDevice, g->st) != hipSuccess || hipStreamSynchronize(g->st) != hipSuccess)
    return stb_fail("stb_groups_aterms: %s", hipGetErrorString(hipGetLastError()));
  l.n_jobs = (unsigned)nj;
  return 0;
}

// ---- the way in: the layout an evaluation of D discounts in the form `which` reads, with the geometry of its items
// (for the grid forms H is filled from gg; H.rec_off is left to match_strip_shape)
static int resolve_layout(const stb_groups_t *g, int &which, int D, hb_dot_info &H, grid_geom &gg) {
  memset(&H, 0, sizeof(H));
  memset(&gg, 0, sizeof(gg));
  if (which == 2 && stb_hb_dot_info(g->N, g->M, g->Dmax, &H, g->hb_sum_C)) return stb_fail("stb_groups_aterms: no halo-block geometry for N=%u M=%u", g->N, g->M);
  if (which < 3) return 0;
  // (the strip shape of the grid form depends on the number of discounts: a list per shape)
  if (stb_grid_geometry(g->N, g->M, D, &gg)) return stb_fail("stb_groups_aterms: no grid geometry for N=%u M=%u", g->N, g->M);
  which = stb_grid_which(gg.C);
  H.R = gg.R;
  H.UC = gg.U * gg.C;
  H.HC = gg.HL * gg.C;
  H.NB = gg.NB;
  H.JW = gg.JW;
  H.NQ = gg.NQ;
  H.G = gg.G;
  H.C = gg.C;
  H.n_tiles = H.n_rec = gg.n_tiles;
  return 0;
}

// a grid layout's list serves one strip shape: what was built for another goes, and the tile offsets of this one are there
static int match_strip_shape(stb_groups_t *g, stb_cell_list &l, hb_dot_info &H, const grid_geom &gg) {
  if ((l.ready || l.tile_off) && (l.R != H.R || l.G != H.G)) {
    (void)hipStreamSynchronize(g->st);
    stb_list_release(l, true);
  }
  if (!l.ready && !l.tile_off) {
    std::vector<unsigned> off;
    stb_grid_tile_offsets(gg, off);
    if (stb_pool_malloc((void **)&l.tile_off, off.size() * sizeof(unsigned)) != hipSuccess ||
        hipMemcpy(l.tile_off, off.data(), off.size() * sizeof(unsigned), hipMemcpyHostToDevice) != hipSuccess)
      return stb_fail("stb_groups_aterms: out of device memory");
  }
  H.rec_off = l.tile_off;
  return 0;
}

int stb_lists_build(stb_groups_t *g, int which, int D) {
  hb_dot_info H;
  grid_geom gg;
  if (resolve_layout(g, which, D, H, gg)) return 1;
  stb_cell_list &l = g->lists[which];
  if (which >= 3 && match_strip_shape(g, l, H, gg)) return 1;
  if (l.ready) return 0;
  // from the count slab: no sort, no host round trip; where it does not apply, the sort
  const int rc = stb_lists_slab_build(g, which, D, H, gg);
  return rc != 2 ? rc : stb_lists_sort_build(g, which, D, H, gg);
}
