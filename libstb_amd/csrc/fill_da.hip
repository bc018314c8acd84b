// fill_da.hip -- k_fill_da: tables of g(n, m) = d log S^n_m / da, and k_ds1_da: d log S^n_1 / da.
//
// The reference has no such table: its only derivative of log S is S_approx_da (lib/sapprox.c:76-114), for m <= 4, and
// wrong at m = 4.  With E = -dS/da the derivative has a recurrence of the table's own shape,
//     E^n_m = (n - 1 - m a) E^{n-1}_m + m S^{n-1}_m + E^{n-1}_{m-1},   E^1_1 = 0,
// every term non-negative, so it rides on the producer/consumer form of the fill (fill_pc.hip): launched per block of
// rows, one producer wave a column block walks the recurrence behind a recomputed halo, consumer waves finish and store,
// no waits between workgroups (the kernel boundary publishes the frontier), blockIdx.y = discount.
//
// The producer carries (v, w) = (S, E) per column, four columns a lane, under ONE exponent a lane.  Per row and column,
// right to left inside the lane so that every operand is still the previous row's:
//     w = fma(coef, w, fma(m, v, w_left));     // inner fma first: m v_prev + w_left, one rounding; then one more
//     v = fma(coef, v, v_left);                // k_fill_pc's own step, the same bits
//     coef += 1.0
// with coef = (double)(n - 1) - (double)m * a formed once per period and m = (double)column exact.  The left neighbour of
// a lane's first column comes from the lane below (DPP) times the frozen power of two s: exact.  The consumers read both
// significands from LDS and store g = -w / v, ONE FP64 division, no contraction; the exponent cancels, so they need
// neither it nor a log table.  tests/hd_oracle.py derives the bar of a cell from exactly these roundings.
//
// Three things checked before this was written:
//  * headroom of the shared exponent.  E / S <= n / (2 (1 - a)) (exact rationals, n <= 60, and it is what the sum of
//    n rows of m / coef <= 1 / (1 - a) gives within a factor 2): 2.5 10^6 = 2^21.3 at n = 10^5, a = 0.98; 2^27 2^53 = 2^80
//    for the largest n the block-floating forms take and the discount next to 1.  k_fill_pc lets a significand climb from
//    2^-700 through 1450 bits and bounds the scaled cross-lane input by 2^970; w needs 80 bits more, which 1024 does not
//    leave.  So a period here spends DA_BITS = 1340 bits: w stays below 2^(640 + 80) in a lane and 2^(860 + 80) across
//    lanes.  Downwards nothing changes: w >= v / n wherever it is not an exact zero (the diagonal).  (As in k_fill_pc the
//    coefficient is formed anew at a period's first row and carried by coef += 1.0 inside it, which rounds at binade
//    crossings: the bits depend on the period and on the rows per launch -- STB_FILL_P, STB_FILL_R -- and on nothing else;
//    not on D.)
//  * the LDS ring holds two values a cell: 2 slots x DA_U rows x 128 columns x 16 B.  With k_fill_pc's 8 rows a trip that
//    is 32 KB, four workgroups a compute unit; DA_U = 4 makes it 16 KB, and the 8 workgroups (24 waves) of k_fill_pc's
//    target fit 160 KB again.  (No exponent buffer and no log table: g needs neither.)
//  * registers: the producer holds v, w, coef, m of four columns (32) + the scale, addresses and the DPP temporaries; the
//    consumers one division.  The launch bound asks for k_fill_pc's six waves a SIMD, i.e. at most 80 registers;
//    tools/kernel_regs.py (make regs) reports what the build took.
//
// log S itself, where the caller asks for it, is written by k_fill_pc launches queued on the same stream (stb_fill_S
// with STB_FILL_PC): the same bits by construction.  Column 1 does not come from the recurrence: k_ds1_da.

#include "stb_common.h"

#define DA_U 4          // rows between two barriers
#define DA_NCW 2        // consumer waves
#define DA_OW (64 * DA_NCW)
#define DA_H (256 - DA_OW)
#define DA_BITS 1340    // bits a significand may climb in a period (see above)
#define DA_CHUNK 64     // terms of a chunk of k_ds1_da's sum

struct da_args {
  const double *a;     // [D]
  double *gt;          // D slabs, S layout
  uint64_t gstride;
  double *fm, *fw;     // frontier: S significands and E in units of 2^fe: [D][2][W]
  int *fe;             // frontier exponents [D][2][W]
  unsigned W, N, M;
  int R;               // rows per launch (<= DA_H)
};

__global__ __launch_bounds__(64 * (1 + DA_NCW), 6) void k_fill_da(da_args A, int k, int P) {
  constexpr int C = 4;
  constexpr int OW = DA_OW, H = DA_H;
  __shared__ __attribute__((aligned(16))) double vbuf[2][DA_U][OW];
  __shared__ __attribute__((aligned(16))) double wbuf[2][DA_U][OW];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int j = blockIdx.x;
  const int d = blockIdx.y;
  const unsigned N = A.N, M = A.M;
  const int n0 = 2 + k * A.R;
  const int n1 = min((int)N, n0 + A.R - 1);
  const int nf = n0 - 1;
  const int cmin = 2 + j * OW - H;
  double *table = A.gt + (uint64_t)d * A.gstride;

  double v[C], w[C], ca[C], mc[C], s = 1.0;
  int ep = 1 + PC_BIAS;
  const int c0 = cmin + lane * C;
  const bool owned = lane * C >= H;
  if (wave == 0) {
    const double a = A.a[d];
    const uint64_t fbase = ((uint64_t)d * 2 + (uint64_t)(k & 1)) * A.W;
    const int cmax_f = min(nf, (int)M);
    double m[C], mw[C];
    int e[C], E = STB_EZ;
#pragma unroll
    for (int i = 0; i < C; i++) {
      const int c = c0 + i;
      m[i] = 0.0;
      mw[i] = 0.0;
      e[i] = STB_EZ;
      if (k == 0) {
        if (c == 1) {  // S^1_1 = 1, E^1_1 = 0
          m[i] = 0.5;
          e[i] = 1;
        }
      } else if (c >= 1 && c <= cmax_f) {
        m[i] = A.fm[fbase + c];
        mw[i] = A.fw[fbase + c];
        e[i] = A.fe[fbase + c];
      }
      if (m[i] != 0.0) E = max(E, e[i]);
      ca[i] = (double)c * a;
      mc[i] = (double)c;
    }
    if (E == STB_EZ) E = 1;
#pragma unroll
    for (int i = 0; i < C; i++) {
      const int sh = max(e[i] - E, -1000) - PC_BIAS;
      v[i] = (m[i] != 0.0) ? ldexp(m[i], sh) : 0.0;
      w[i] = (m[i] != 0.0) ? ldexp(mw[i], sh) : 0.0;
    }
    ep = E + PC_BIAS;
  }
  const int ridx = (wave - 1) * 64 + lane;  // consumers: my slot in the ring
  const int cc = 2 + j * OW + ridx;         // ... and my column

  for (int nb = n0; nb <= n1; nb += P) {
    const int ne = min(n1, nb + P - 1);
    const int ns = max(nb, max(cmin, 3));  // rows above the block's first column are all zero
    if (wave == 0) {
      const int epl = wave_shr1(ep, ep);
      s = ldexp(1.0, min(max(epl - ep, -1100), 220));
      if (nb == 2 && cmin < 3) {  // row 2 (nothing is stored for it)
        const double t0 = wave_shr1_zero(v[3]) * s, u0 = wave_shr1_zero(w[3]) * s;
#pragma unroll
        for (int i = C - 1; i >= 0; i--) {
          const double cf = 1.0 - ca[i];
          w[i] = fma(cf, w[i], fma(mc[i], v[i], i ? w[i - 1] : u0));
          v[i] = fma(cf, v[i], i ? v[i - 1] : t0);
        }
      }
    }
    if (ns <= ne) {
      double coef[C];
      if (wave == 0) {
#pragma unroll
        for (int i = 0; i < C; i++) coef[i] = (double)(ns - 1) - ca[i];
      }
      double *rowbase = table + stb_row_offset((unsigned)ns, M);
      const int trips = (ne - ns + 1 + DA_U - 1) / DA_U;
      // trip q: the producer computes rows ns + U q .., the consumers emit the rows of trip q - 1
      for (int q = 0; q <= trips; q++) {
        if (wave == 0) {
          if (q < trips) {
            const int r0 = ns + q * DA_U;
            const int cnt = min(DA_U, ne - r0 + 1);
            for (int u = 0; u < cnt; u++) {
              const double t0 = wave_shr1_zero(v[3]) * s, u0 = wave_shr1_zero(w[3]) * s;
#pragma unroll
              for (int i = C - 1; i >= 0; i--) {
                w[i] = fma(coef[i], w[i], fma(mc[i], v[i], i ? w[i - 1] : u0));
                v[i] = fma(coef[i], v[i], i ? v[i - 1] : t0);
                coef[i] += 1.0;
              }
              if (owned) {
                const int o = lane * C - H;
                *(double2 *)&vbuf[q & 1][u][o] = make_double2(v[0], v[1]);
                *(double2 *)&vbuf[q & 1][u][o + 2] = make_double2(v[2], v[3]);
                *(double2 *)&wbuf[q & 1][u][o] = make_double2(w[0], w[1]);
                *(double2 *)&wbuf[q & 1][u][o + 2] = make_double2(w[2], w[3]);
              }
            }
          }
        } else if (q > 0) {
          const int r0 = ns + (q - 1) * DA_U;
          const int cnt = min(DA_U, ne - r0 + 1);
          for (int u = 0; u < cnt; u++) {
            const int r = r0 + u;
            // row r stores columns 2 .. min(r - 1, M); nothing else of the slab is written
            if (cc <= min(r - 1, (int)M)) {
#pragma clang fp contract(off)
              rowbase[cc - 2] = -wbuf[(q - 1) & 1][u][ridx] / vbuf[(q - 1) & 1][u][ridx];
            }
            rowbase += stb_row_pitch((unsigned)r, M);
          }
        }
        lds_barrier();
      }
    }
    if (wave == 0) {
      // renormalise the lane by the largest S significand (E follows it within 2^80)
      int kmax = -4000;
#pragma unroll
      for (int i = 0; i < C; i++)
        if (v[i] != 0.0) kmax = max(kmax, __builtin_amdgcn_frexp_exp(v[i]));
      if (kmax > -4000) {
#pragma unroll
        for (int i = 0; i < C; i++) {
          v[i] = ldexp(v[i], -kmax - PC_BIAS);
          w[i] = ldexp(w[i], -kmax - PC_BIAS);
        }
        ep += kmax + PC_BIAS;
      }
    }
  }

  if (wave == 0 && n1 < (int)N) {
    const uint64_t fbase = ((uint64_t)d * 2 + (uint64_t)((k + 1) & 1)) * A.W;
#pragma unroll
    for (int i = 0; i < C; i++) {
      const int c = c0 + i;
      const bool mine = owned || (j == 0 && c == 1);
      if (mine && c >= 1 && c <= (int)M) {
        const int ke = __builtin_amdgcn_frexp_exp(v[i]);
        A.fm[fbase + c] = __builtin_amdgcn_frexp_mant(v[i]);
        A.fw[fbase + c] = (v[i] != 0.0) ? ldexp(w[i], -ke) : 0.0;  // E in units of 2^fe: exact
        A.fe[fbase + c] = (v[i] != 0.0) ? ep + ke : STB_EZ;
      }
    }
  }
}

// dS1[n-1] = d/da [lgamma(n - a) - lgamma(1 - a)] = -sum_{k=1}^{n-1} 1 / (k - a), n = 1 .. N.
// The order of the sum is fixed by DA_CHUNK alone, not by the launch: terms k = 64 c + 1 .. 64 c + 64 form chunk c;
// chunk sums add their terms in ascending k from 0; B_c is the sum of the chunk sums before c, added in ascending c from
// 0; the value at k is B_c plus the chunk's terms up to k, added in ascending k.  One workgroup a discount: the chunks
// strided over its threads, the chunk bases by one thread (N / 64 additions), then the running sums.
__global__ __launch_bounds__(256) void k_ds1_da(const double *a, double *dS1, uint64_t stride, unsigned N, double *chunks, unsigned nch) {
#pragma clang fp contract(off)
  const int d = blockIdx.x;
  const double ad = a[d];
  double *cs = chunks + (uint64_t)d * nch;
  double *out = dS1 + (uint64_t)d * stride;
  const unsigned K = N - 1;  // terms
  for (unsigned c = threadIdx.x; c < nch; c += 256) {
    double acc = 0.0;
    const unsigned k1 = min(K, c * DA_CHUNK + DA_CHUNK);
    for (unsigned k = c * DA_CHUNK + 1; k <= k1; k++) acc += 1.0 / ((double)k - ad);
    cs[c] = acc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double run = 0.0;
    for (unsigned c = 0; c < nch; c++) {
      const double t = cs[c];
      cs[c] = run;
      run += t;
    }
    out[0] = 0.0;
  }
  __syncthreads();
  for (unsigned c = threadIdx.x; c < nch; c += 256) {
    double acc = cs[c];
    const unsigned k1 = min(K, c * DA_CHUNK + DA_CHUNK);
    for (unsigned k = c * DA_CHUNK + 1; k <= k1; k++) {
      acc += 1.0 / ((double)k - ad);
      out[k] = -acc;
    }
  }
}

__global__ void k_da_set_a(stb_a64 av, double *a, int D) {
  if ((int)threadIdx.x < D) a[threadIdx.x] = av.v[threadIdx.x];
}

static unsigned da_pitch(unsigned M) { return (unsigned)stb_align_up((size_t)M + 2, 64); }
static unsigned da_chunks(unsigned N) { return N > 1 ? (N - 1 + DA_CHUNK - 1) / DA_CHUNK : 1; }
static size_t da_own_bytes(unsigned N, unsigned M, int D) {
  const size_t W = da_pitch(M);
  return stb_align_up((size_t)D * sizeof(double), 256) + stb_align_up((size_t)D * 2 * W * (2 * sizeof(double) + sizeof(int)), 256) +
         stb_align_up((size_t)D * da_chunks(N) * sizeof(double), 256);
}

extern "C" size_t stb_fill_dS_workspace_bytes(unsigned N, unsigned M, int D) {
  if (D < 1 || N < 2 || M < 2) return 0;
  return da_own_bytes(N, M, D) + stb_fill_workspace_bytes(N, M, D);  // (the second part: the log S slabs, when asked for)
}

extern "C" int stb_fill_dS(const double *a_host, int D, unsigned N, unsigned M, double *d_gtables, uint64_t gtable_stride, double *d_dS1,
                           uint64_t ds1_stride, double *d_tables, uint64_t table_stride, double *d_S1, uint64_t s1_stride, void *d_ws,
                           size_t ws_bytes, void *stream) {
  STB_ENTRY;
  const char *who = "stb_fill_dS";
  hipStream_t st = (hipStream_t)stream;
  if (D < 1 || D > 64) return stb_fail("%s: D=%d (1..64)", who, D);
  if (N < 2 || M < 2) return stb_fail("%s: bounds N=%u M=%u too small", who, N, M);
  if (N >= (1u << 27)) return stb_fail("%s: N=%u (the block-floating recurrence takes N < 2^27)", who, N);
  if (!a_host || !d_gtables || !d_dS1 || !d_ws) return stb_fail("%s: null pointer", who);
  if ((d_tables == nullptr) != (d_S1 == nullptr)) return stb_fail("%s: the log S slab and its S1 vector come together or not at all", who);
  if (ws_bytes < stb_fill_dS_workspace_bytes(N, M, D)) return stb_fail("%s: workspace %zu < %zu", who, ws_bytes, stb_fill_dS_workspace_bytes(N, M, D));
  const uint64_t need = stb_table_elems(N, M);
  if (gtable_stride < need || ds1_stride < N || (d_tables && (table_stride < need || s1_stride < N))) return stb_fail("%s: strides too small", who);
  if (D > 1 && ((gtable_stride & 1) || (d_tables && (table_stride & 1)))) return stb_fail("%s: table stride must be even", who);
  for (int d = 0; d < D; d++)
    if (!(a_host[d] >= 0.0 && a_host[d] < 1.0)) return stb_fail("%s: discount %g outside [0,1)", who, a_host[d]);

  da_args A;
  memset(&A, 0, sizeof(A));
  char *ws = (char *)d_ws;
  double *d_a = (double *)ws;
  ws += stb_align_up((size_t)D * sizeof(double), 256);
  A.a = d_a;
  A.W = da_pitch(M);
  const size_t fr = (size_t)D * 2 * A.W;
  A.fm = (double *)ws;
  A.fw = A.fm + fr;
  A.fe = (int *)(A.fw + fr);
  ws += stb_align_up(fr * (2 * sizeof(double) + sizeof(int)), 256);
  double *chunks = (double *)ws;
  A.gt = d_gtables;
  A.gstride = gtable_stride;
  A.N = N;
  A.M = M;
  A.R = stb_env_int("STB_FILL_R", DA_H);
  if (A.R > DA_H) A.R = DA_H;
  if (A.R < 1) A.R = 1;

  stb_a64 av;
  for (int d = 0; d < D; d++) av.v[d] = a_host[d];
  hipLaunchKernelGGL(k_da_set_a, dim3(1), dim3(64), 0, st, av, d_a, D);
  hipLaunchKernelGGL(k_ds1_da, dim3(D), dim3(256), 0, st, A.a, d_dS1, ds1_stride, N, chunks, da_chunks(N));

  // equal-length renormalisation periods inside a launch, as stb_launch_pc cuts them, from DA_BITS
  const int R = A.R;
  const int P = [&] {
    int bits = 1;
    while ((1ull << bits) < (unsigned long long)N) bits++;
    int p = DA_BITS / (2 * bits + 1);
    if (p < 1) p = 1;
    const int penv = stb_env_int("STB_FILL_P", 0);
    if (penv > 0 && penv < p) p = penv;
    if (p >= R) return R;
    const int per = (R + p - 1) / p;
    return (R + per - 1) / per;
  }();
  const int nlaunch = ((int)N - 1 + R - 1) / R;
  for (int k = 0; k < nlaunch; k++) {
    int n1 = 2 + (k + 1) * R - 1;
    if (n1 > (int)N) n1 = (int)N;
    int ncols = (n1 < (int)M ? n1 : (int)M) - 1;
    if (ncols < 1) ncols = 1;
    STB_LAUNCH(k_fill_da, dim3((ncols + DA_OW - 1) / DA_OW, D), dim3(64 * (1 + DA_NCW)), st, A, k, P);
  }
  HIPCHK(hipGetLastError());
  if (d_tables)
    return stb_fill_S(a_host, D, N, M, d_tables, table_stride, d_S1, s1_stride, (char *)d_ws + da_own_bytes(N, M, D),
                      ws_bytes - da_own_bytes(N, M, D), STB_FILL_PC, stream);
  return 0;
}

// the constants a test takes its shapes from: rows per launch, owned columns and halo columns of a column block, rows
// between two barriers, rows of a renormalisation period for N rows (before STB_FILL_P)
extern "C" void stb_fill_dS_geometry(unsigned N, int *rows_per_launch, int *owned_cols, int *halo_cols, int *trip_rows, int *period_rows) {
  int bits = 1;
  while ((1ull << bits) < (unsigned long long)N) bits++;
  int p = DA_BITS / (2 * bits + 1);
  if (p < 1) p = 1;
  if (rows_per_launch) *rows_per_launch = DA_H;
  if (owned_cols) *owned_cols = DA_OW;
  if (halo_cols) *halo_cols = DA_H;
  if (trip_rows) *trip_rows = DA_U;
  if (period_rows) *period_rows = p;
}
