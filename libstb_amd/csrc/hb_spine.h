// hb_spine.h -- the halo-block spine, what k_fill_hb (fill_hb.hip) and k_grid_hb (grid_hb.hip) both walk with: the record
// format, the row, the renormalisation, a strip's first block -- and, on the host, the strip shape, the wait settings and
// the timeline file.
//
// THE RECORD.  What a spine wave leaves in HBM of a block for another workgroup (the right workgroup's fetcher, the tile
// workers) is, per lane, C words of significands and one word of lane exponent.  A word is its own flag: 0 means "not
// written yet".  Significands are never negative and travel with the sign bit set (HB_WRITTEN); exponents travel with
// 2^30 added (HB_EOFF32).  Records are written with write-through stores (sc1) and read with L1-bypassing loads at agent
// scope.  This is the one place that format is written down; whoever changes it changes both kernels.
//
// WHAT IS NOT HERE.  Everything below left every instantiation of both kernels instruction for instruction as it was
// (tools/isa_diff.py).  Three pieces that did not are still written out where they were, untimed (MEASUREMENTS O8): the
// fetcher wave's loop, the same in both kernels but for where a record lies, which ring it fills, the last block and the
// exponent offset; hb_row's body in k_fill_hb's summing worker (as a call it moves k_fill_hb<2, 1, 0>: 5972 -> 5954
// instructions); the worker's two "give up" blocks (as one lambda they move all twelve k_fill_hb).
#ifndef STB_HB_SPINE_H
#define STB_HB_SPINE_H

#include <vector>

#include "fill_chain.h"

#define HB_PMAX 7          // spine waves of a workgroup at most
#define HB_MAXHL 32        // halo lanes at most
#define HB_EOFF32 (1u << 30)
#define HB_WRITTEN 0x8000000000000000ull  // a record's significands (never negative) travel with the sign bit set
#define HB_SPIN 48         // looks at a neighbour's counter, ~0.1 us apart, before the out-of-line wait
// ... per strip shape: blocks have at most 48 rows with 2 or 4 columns per lane (+ a lane for the V table), 32 with one -- what
// the fill's hand-over rings in LDS are sized by (4 columns: 23 KB instead of 57)
__host__ __device__ constexpr int hb_mhl(int C) { return C == 1 ? HB_MAXHL : (C == 2 ? 25 : (C == 3 ? 17 : 13)); }

typedef double hb_double2 __attribute__((ext_vector_type(2)));

// aligned 16-byte store at (wave-uniform base) + (per-lane byte offset); see store_sbase
__device__ __forceinline__ void hb_store16(const void *sbase, unsigned byte_off, double x, double y) {
  unsigned long long base_copy;
  hb_double2 v2 = {x, y};
  asm volatile("s_mov_b64 %0, %3\n\tglobal_store_dwordx4 %1, %2, %0\n\ts_nop 1"
               : "=&s"(base_copy)
               : "v"(byte_off), "v"(v2), "s"(sbase)
               : "memory");
}

// two record words with one write-through store (what __hip_atomic_store at agent scope compiles to, 16 bytes wide)
__device__ __forceinline__ void hb_store_wt16(unsigned long long *p, unsigned long long a, unsigned long long b) {
  typedef unsigned long long hb_u64x2 __attribute__((ext_vector_type(2)));
  const hb_u64x2 v2 = {a, b};
  // (s_nop: a store of more than 8 bytes reads its data a cycle or two after it issues, and the compiler does
  // not look into an asm statement for the VALU write of those registers that may follow)
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v2) : "memory");
}

// the record of a spine block: C words per lane (each with the sign bit set) behind `p`, written through, by the lanes of
// `mask` only -- the mask goes into exec and comes out again inside the statement: no branch round the stores (the
// compiler's own masked region moved them out of line, two taken branches a block on the lone wave's path)
// (s_and_saveexec_b64 writes SCC, which the statements say)
template <int C>
__device__ __forceinline__ void hb_store_record(unsigned long long mask, unsigned long long *p, const double (&v)[C]) {
  typedef unsigned long long hb_u64x2 __attribute__((ext_vector_type(2)));
  unsigned long long saved;
  if constexpr (C == 1) {
    const unsigned long long a = (unsigned long long)__double_as_longlong(v[0]) | HB_WRITTEN;
    asm volatile("s_and_saveexec_b64 %0, %1\n\tglobal_store_dwordx2 %2, %3, off sc1\n\ts_mov_b64 exec, %0" : "=&s"(saved) : "s"(mask), "v"(p), "v"(a) : "memory", "scc");
  } else if constexpr (C == 2) {
    const hb_u64x2 a = {(unsigned long long)__double_as_longlong(v[0]) | HB_WRITTEN, (unsigned long long)__double_as_longlong(v[1]) | HB_WRITTEN};
    asm volatile("s_and_saveexec_b64 %0, %1\n\tglobal_store_dwordx4 %2, %3, off sc1\n\ts_nop 0\n\ts_mov_b64 exec, %0" : "=&s"(saved) : "s"(mask), "v"(p), "v"(a) : "memory", "scc");
  } else if constexpr (C == 3) {
    const hb_u64x2 a = {(unsigned long long)__double_as_longlong(v[0]) | HB_WRITTEN, (unsigned long long)__double_as_longlong(v[1]) | HB_WRITTEN};
    const unsigned long long c = (unsigned long long)__double_as_longlong(v[2]) | HB_WRITTEN;
    asm volatile("s_and_saveexec_b64 %0, %1\n\tglobal_store_dwordx4 %2, %3, off sc1\n\tglobal_store_dwordx2 %2, %4, off offset:16 sc1\n\ts_nop 0\n\ts_mov_b64 exec, %0"
                 : "=&s"(saved) : "s"(mask), "v"(p), "v"(a), "v"(c) : "memory", "scc");
  } else {
    static_assert(C == 4, "columns per lane");
    const hb_u64x2 a = {(unsigned long long)__double_as_longlong(v[0]) | HB_WRITTEN, (unsigned long long)__double_as_longlong(v[1]) | HB_WRITTEN};
    const hb_u64x2 c = {(unsigned long long)__double_as_longlong(v[2]) | HB_WRITTEN, (unsigned long long)__double_as_longlong(v[3]) | HB_WRITTEN};
    asm volatile("s_and_saveexec_b64 %0, %1\n\tglobal_store_dwordx4 %2, %3, off sc1\n\tglobal_store_dwordx4 %2, %4, off offset:16 sc1\n\ts_nop 0\n\ts_mov_b64 exec, %0"
                 : "=&s"(saved) : "s"(mask), "v"(p), "v"(a), "v"(c) : "memory", "scc");
  }
}

// renormalise a lane: the largest of its C significands (none is negative) back to 2^-PC_BIAS * [0.5,1)
template <int C>
__device__ __forceinline__ void hb_renorm(double (&v)[C], int &ep) {
  double vmax = v[0];
#pragma unroll
  for (int i = 1; i < C; i++) vmax = fmax(vmax, v[i]);
  const int sh = (vmax != 0.0) ? __builtin_amdgcn_frexp_exp(vmax) + PC_BIAS : 0;
#pragma unroll
  for (int i = 0; i < C; i++) v[i] = ldexp(v[i], -sh);
  ep += sh;
}

// ... in two steps: the shift (from the lane as it stands) and its application (possibly to the lane a few rows later: any
// shift that keeps the significands in range is as good as any other -- the arithmetic is scale-free and the logs are taken
// from exponent field + lane exponent together)
template <int C>
__device__ __forceinline__ int hb_renorm_shift(const double (&v)[C]) {
  // (v_max_f64 as written: fmax() first quiets its operands, an instruction each -- nothing here is a NaN)
  double vmax = v[0];
#pragma unroll
  for (int i = 1; i < C; i++) asm("v_max_f64 %0, %1, %2" : "=v"(vmax) : "v"(vmax), "v"(v[i]));
  int sh = (vmax != 0.0) ? __builtin_amdgcn_frexp_exp(vmax) + PC_BIAS : 0;
  asm volatile("" : "+v"(sh));  // (here, not where it is used)
  return sh;
}
template <int C>
__device__ __forceinline__ void hb_renorm_apply(double (&v)[C], int &ep, int sh) {
#pragma unroll
  for (int i = 0; i < C; i++) v[i] = ldexp(v[i], -sh);
  ep += sh;
}

// what a lane's first column takes from the lane to its left is under that lane's exponent: the factor 2^(e_left - e),
// clamped to what a double holds (an exponent that far off belongs to a lane of zeros)
__device__ __forceinline__ double hb_left_scale(int e_left, int e) { return ldexp(1.0, min(max(e_left - e, -1100), 220)); }
// ... with the left lane's exponent fetched (lane 0: its own -- the factor is 1)
__device__ __forceinline__ double hb_left_scale(int ep) { return hb_left_scale(wave_shr1(ep, ep), ep); }

// a row of the recurrence: lane l takes the last column of lane l - 1 (lane 0: nothing), scaled
// by s = 2^(exponent of lane l-1 - exponent of lane l), frozen for the block
template <int C>
__device__ __forceinline__ void hb_row(double (&v)[C], double (&coef)[C], double s) {
  const double t0 = wave_shr1_zero(v[C - 1]) * s;
#pragma unroll
  for (int i = C - 1; i >= 1; i--) v[i] = fma(coef[i], v[i], v[i - 1]);
  v[0] = fma(coef[0], v[0], t0);
#pragma unroll
  for (int i = 0; i < C; i++) coef[i] += 1.0;
}

// A spine wave's wait for an LDS counter of its workgroup to reach `need`.  Neighbours reach a block's end within a
// fraction of a microsecond of each other: a short wait is spun out here -- the out-of-line wait is a call, and a call
// waits for every store under way.  A wait that is given up (timeout, or another wave gave up) sets `aborted`, and every
// later one returns at once: the wave runs to its end on stale halos, the header says `code` and `who`.
__device__ __forceinline__ void hb_wait_ge(const int *cnt, int need, unsigned code, bool &aborted, int *s_abort, unsigned *hdr,
                                           unsigned long long timeout, unsigned who) {
  if (aborted) return;
  for (int k = 0; k < HB_SPIN; k++) {
    if (lds_peek(cnt) >= need) {
      asm volatile("" ::: "memory");  // (what the counter guards is read or written after it)
      return;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  if (!chain_wait_slow(cnt, need, s_abort, hdr, timeout, code, who, 1)) aborted = true;
  asm volatile("" ::: "memory");
}

// first block of strip j: the state before it has nothing in the strip's own columns (2 + j U C and up)
__host__ __device__ static inline int hb_first_block(int j, int UC, int R) { return (int)(((long long)j * UC) / R); }

// ------------------------------------------------------------------------------------------------
// host side

// The shape of the strips of a table of N rows whose columns 2 .. cmax hold cells, walked with C columns per lane in blocks
// of R rows (halo_extra: the V table's lane more, see hb_geometry): halo and own lanes, strips, blocks -- and the tiles,
// a strip's being its blocks from its first one on.  ok: every strip has one (column 2 + j U C <= N - 1: always).
struct hb_strip {
  int HL, U, JW, NB;
  uint64_t tiles;
  bool ok;
};
static inline hb_strip hb_strip_shape(unsigned N, unsigned cmax, int C, int R, int halo_extra) {
  hb_strip s;
  s.HL = R / C + halo_extra;
  s.U = 64 - s.HL;
  const int UC = s.U * C;
  s.JW = (int)((cmax - 1 + UC - 1) / UC);
  if (s.JW < 1) s.JW = 1;
  s.NB = (int)((N - 1 + R - 1) / R);  // the state before block b is row 1 + b R
  s.tiles = 0;
  s.ok = true;
  for (int j = 0; j < s.JW; j++) {
    const int b0 = hb_first_block(j, UC, R);
    if (b0 < s.NB)
      s.tiles += (uint64_t)(s.NB - b0);
    else
      s.ok = false;
  }
  return s;
}
// ... and where every strip's tiles start when they are laid out strip after strip from `first` on: out[0 .. JW - 1];
// returns the end
static inline unsigned hb_strip_starts(int UC, int R, int JW, int NB, unsigned first, unsigned *out) {
  for (int j = 0; j < JW; j++) {
    out[j] = first;
    first += (unsigned)(NB - hb_first_block(j, UC, R));
  }
  return first;
}

// how long a wait of either kernel may last (wall_clock64 ticks: 100 MHz) and what a fetcher sleeps between two polls
struct hb_wait_settings {
  unsigned long long timeout;
  int poll_nap;
};
static inline hb_wait_settings hb_wait_env() {
  hb_wait_settings w;
  w.timeout = (unsigned long long)stb_env_int("STB_CHAIN_TIMEOUT_MS", 2000) * 100000ull;
  w.poll_nap = stb_env_int("STB_HB_POLL_NAP", 4);
  if (w.poll_nap < 1) w.poll_nap = 1;
  return w;
}

// STB_HB_TIMELINE=file: the stamps of a launch (tools/timeline_hb.py, fine_hb.py, hop_hb.py read the file: 8 ints of
// header, the tile order if there is one, the stamps).  Owns the device buffer: whichever way the launch function is left,
// the buffer goes with it.  (In an unnamed namespace: a header's class would export its members from the library.)
namespace {
struct hb_timeline {
  const char *file = nullptr;
  unsigned long long *dbg = nullptr;
  size_t words = 0;
  hb_timeline() = default;
  hb_timeline(const hb_timeline &) = delete;
  hb_timeline &operator=(const hb_timeline &) = delete;
  ~hb_timeline() {
    if (dbg) (void)hipFree(dbg);
  }
  // the buffer, zeroed on the stream, when the variable names a file; *out stays null otherwise
  int open(size_t n_words, hipStream_t st, unsigned long long **out) {
    file = getenv("STB_HB_TIMELINE");
    if (!file || !*file) return 0;
    words = n_words;
    HIPCHK(hipMalloc((void **)&dbg, words * 8));
    HIPCHK(hipMemsetAsync(dbg, 0, words * 8, st));
    *out = dbg;
    return 0;
  }
  // after the launch: waits for it and writes the file (order: n_order words on the device, or null)
  int write(const int (&hd)[8], const unsigned *order, unsigned n_order, hipStream_t st) {
    if (!dbg) return 0;
    HIPCHK(hipStreamSynchronize(st));
    std::vector<unsigned long long> h(words);
    HIPCHK(hipMemcpy(h.data(), dbg, words * 8, hipMemcpyDeviceToHost));
    std::vector<unsigned> ord(order ? n_order : 0);
    if (order) HIPCHK(hipMemcpy(ord.data(), order, (size_t)n_order * sizeof(unsigned), hipMemcpyDeviceToHost));
    FILE *f = fopen(file, "wb");
    if (f) {
      fwrite(hd, sizeof(int), 8, f);
      if (order) fwrite(ord.data(), sizeof(unsigned), n_order, f);
      fwrite(h.data(), 8, words, f);
      fclose(f);
    }
    return 0;
  }
};
}  // namespace

#endif
