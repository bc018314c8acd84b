// tindic.hip -- the table-indicator step of a Pitman-Yor Gibbs sampler on the device: every customer's indicator
// ("heads a table of its dish") is removed and drawn again given the rest of its restaurant (test/demo.c:405-436,
// SampleTI of test/check.c:843-866), one customer after another.
//
//   k_tindic_lane   one lane per restaurant: many short restaurants
//   k_tindic_wave   one wave per restaurant: few long ones (t in LDS, the next 64 customers' V cells prefetched)
//
// A visit to a customer of pair (n, t, h) of restaurant i (total T, concentration b, discount a):
//   n <= 1 or n > N: nothing.  Remove: t > 1 and (n-1) u1 < t-1 -> t--, T--.  Then, with V = V^n_{t+1} (0 when t+1 > M)
//     odds = h (b + T a) t / (n - t) V        (STB_TI_REF_ODDS: / (n - t + 1), the reference's factor)
//   and t++, T++ when u2 < odds / (odds + 1).
// Given one indicator held at 1 and the other n-1 uniform given t, the prior ratio of t+1 to t tables is
// C(n-1, t-1) / C(n-1, t) = t / (n-t): with it the step leaves the PYP joint (b|a)_T prod_k S^{n_k}_{t_k,a} h_k^{t_k}
// invariant; the reference's t / (n-t+1) does not.
//
// Both forms evaluate a visit with the same functions (ti_remove, ti_add; no contraction) on the same V cells, so
// they give the same bits.  Uniforms are counter-based as in tcounts.hip: sweep s, flat customer index c,
//     key_s = mix(seed + (s+1) gamma),  u1 = unit(mix(key_s + (2c+1) gamma)),  u2 = unit(mix(key_s + (2c+2) gamma))
// so the draws depend on (seed, sweep, c) alone.  No workgroup waits for another.  (The object that holds a state and
// queues these sweeps, stb_tindic_t, is tindic_obj.hip.)

#include "stb_common.h"
#include "tindic.h"

#define STB_TI_LDS_CAP 4096  // dishes whose t a wave keeps in LDS (8 KB); restaurants with more keep t in global memory
// ---- lane form -------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(64) void k_tindic_lane(const double *vt, unsigned N, unsigned M, double a, const double *bpar,
                                                    int I, const uint64_t *koff, const uint32_t *nv, uint16_t *tv,
                                                    uint32_t *Tv, const double *hv, const uint64_t *coff,
                                                    const uint32_t *cust, unsigned flags, uint64_t seed, uint64_t sweep0,
                                                    int nsweeps) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= I) return;
  const bool ref = (flags & STB_TI_REF_ODDS_FLAG) != 0;
  const uint64_t k0 = koff[i], k1 = koff[i + 1], c0 = coff[i], c1 = coff[i + 1];
  const double b = bpar[i];
  uint32_t T = Tv[i];
  for (int s = 0; s < nsweeps; s++) {
    const uint64_t key = stb_mix64(seed + (sweep0 + (uint64_t)s + 1) * STB_GAMMA);
    if (cust) {
      for (uint64_t c = c0; c < c1; c++) {  // (t through global memory: this lane's own stores)
        const uint64_t g = k0 + cust[c];
        const unsigned n = nv[g];
        if (n <= 1 || n > N) continue;
        unsigned t = tv[g];
        if (ti_remove(n, t, stb_unit(key, 2 * c + 1))) t--, T--;
        const double h = hv ? hv[g] : 1.0;
        if (ti_add(n, t, T, h, a, b, ti_V(vt, M, n, t + 1), stb_unit(key, 2 * c + 2), ref)) t++, T++;
        tv[g] = (uint16_t)t;
      }
    } else {  // pair order: a pair's customers are consecutive, its t stays in a register
      uint64_t c = c0;
      for (uint64_t g = k0; g < k1; g++) {
        const unsigned n = nv[g];
        if (n <= 1 || n > N) {
          c += n;
          continue;
        }
        const double h = hv ? hv[g] : 1.0;
        const unsigned t0 = tv[g];
        unsigned t = t0;
        for (unsigned r = 0; r < n; r++, c++) {
          if (ti_remove(n, t, stb_unit(key, 2 * c + 1))) t--, T--;
          if (ti_add(n, t, T, h, a, b, ti_V(vt, M, n, t + 1), stb_unit(key, 2 * c + 2), ref)) t++, T++;
        }
        if (t != t0) tv[g] = (uint16_t)t;
      }
    }
  }
  Tv[i] = T;
}

// ---- wave form -------------------------------------------------------------------------------------------------
// Every lane walks the same chain on the same values (read with readlane), so each lane's own loads and stores are
// all the ordering the chain needs; the per-lane work is the loads of the next 64 customers and their V cells.

__global__ __launch_bounds__(64) void k_tindic_wave(const double *vt, unsigned N, unsigned M, double a, const double *bpar,
                                                    int I, const uint64_t *koff, const uint32_t *nv, uint16_t *tv,
                                                    uint32_t *Tv, const double *hv, const uint64_t *coff,
                                                    const uint32_t *cust, unsigned flags, uint64_t seed, uint64_t sweep0,
                                                    int nsweeps, unsigned cap) {
  extern __shared__ uint16_t lt[];  // [cap]: t of the restaurant's dishes, customer order with K_i <= cap
  const int i = blockIdx.x;
  if (i >= I) return;
  const unsigned lane = threadIdx.x;
  const bool ref = (flags & STB_TI_REF_ODDS_FLAG) != 0;
  const uint64_t k0 = koff[i], k1 = koff[i + 1], c0 = coff[i], c1 = coff[i + 1];
  const double b = bpar[i];
  uint32_t T = Tv[i];
  const bool inlds = cust && k1 - k0 <= cap;
  if (inlds)
    for (uint64_t k = lane; k < k1 - k0; k += 64) lt[k] = tv[k0 + k];
  __syncthreads();
  for (int s = 0; s < nsweeps; s++) {
    const uint64_t key = stb_mix64(seed + (sweep0 + (uint64_t)s + 1) * STB_GAMMA);
    if (cust) {
      for (uint64_t cb = c0; cb < c1; cb += 64) {
        const unsigned L = c1 - cb < 64 ? (unsigned)(c1 - cb) : 64u;
        // this lane's customer of the chunk: its dish, n, h, and V(n, t0), V(n, t0+1) at the chunk's start t0 --
        // the two cells the dish's first visit in the chunk can read
        unsigned mk = 0, mn = 0, mt0 = 0;
        double mh = 1.0, v0 = 0.0, v1 = 0.0;
        if (lane < L) {
          mk = cust[cb + lane];
          const uint64_t g = k0 + mk;
          mn = nv[g];
          if (mn >= 2 && mn <= N) {
            mh = hv ? hv[g] : 1.0;
            mt0 = inlds ? lt[mk] : tv[g];
            v0 = ti_V(vt, M, mn, mt0);
            v1 = ti_V(vt, M, mn, mt0 + 1);
          }
        }
        for (unsigned j = 0; j < L; j++) {
          const unsigned n = stb_wave_rl(mn, j);
          if (n <= 1 || n > N) continue;
          const unsigned k = stb_wave_rl(mk, j), t0 = stb_wave_rl(mt0, j);
          const uint64_t c = cb + j;
          unsigned t = inlds ? lt[k] : tv[k0 + k];
          if (ti_remove(n, t, stb_unit(key, 2 * c + 1))) t--, T--;
          const unsigned m = t + 1;
          // (an earlier visit in this chunk may have moved the dish's t out of the prefetched pair: a direct load)
          const double V = m == t0 ? stb_wave_rld(v0, j) : (m == t0 + 1 ? stb_wave_rld(v1, j) : ti_V(vt, M, n, m));
          if (ti_add(n, t, T, stb_wave_rld(mh, j), a, b, V, stb_unit(key, 2 * c + 2), ref)) t++, T++;
          if (inlds) lt[k] = (uint16_t)t;  // (every lane stores the same value)
          else tv[k0 + k] = (uint16_t)t;
        }
      }
    } else {  // pair order: 64 pairs loaded at a time, a window of 64 cells of the row around t per pair
      uint64_t c = c0;
      for (uint64_t pb = k0; pb < k1; pb += 64) {
        const unsigned P = k1 - pb < 64 ? (unsigned)(k1 - pb) : 64u;
        unsigned mn = 0, mt = 0;
        double mh = 1.0;
        if (lane < P) {
          mn = nv[pb + lane];
          mt = tv[pb + lane];
          mh = hv ? hv[pb + lane] : 1.0;
        }
        for (unsigned j = 0; j < P; j++) {
          const unsigned n = stb_wave_rl(mn, j);
          if (n <= 1 || n > N) {
            c += n;
            continue;
          }
          const unsigned t0 = stb_wave_rl(mt, j);
          const double h = stb_wave_rld(mh, j);
          unsigned t = t0;
          unsigned wb = t0 > 32 ? t0 - 32 : 0;  // the window holds m = wb .. wb+63
          double win = ti_V(vt, M, n, wb + lane);
          for (unsigned r = 0; r < n; r++, c++) {
            if (ti_remove(n, t, stb_unit(key, 2 * c + 1))) t--, T--;
            const unsigned m = t + 1;
            if (m - wb >= 64u) {
              wb = m > 32 ? m - 32 : 0;
              win = ti_V(vt, M, n, wb + lane);
            }
            if (ti_add(n, t, T, h, a, b, stb_wave_rld(win, m - wb), stb_unit(key, 2 * c + 2), ref)) t++, T++;
          }
          if (t != t0) tv[pb + j] = (uint16_t)t;
        }
      }
    }
  }
  if (inlds) {
    __syncthreads();
    for (uint64_t k = lane; k < k1 - k0; k += 64) tv[k0 + k] = lt[k];
  }
  if (lane == 0) Tv[i] = T;
}

// ---- launch ------------------------------------------------------------------------------------------------------

// the wave form below this many restaurants (MEASUREMENTS.md section T2), the lane form from it on;
// STB_TINDIC_FORM=lane|wave forces one
#define STB_TI_WAVE_BELOW 2048

static int ti_form(int I) {
  const char *e = getenv("STB_TINDIC_FORM");
  if (e && !strcmp(e, "lane")) return 0;
  if (e && !strcmp(e, "wave")) return 1;
  return I < STB_TI_WAVE_BELOW ? 1 : 0;
}

// r.maxK: dishes a wave keeps in LDS (the largest K_i when it is known and smaller than STB_TI_LDS_CAP)
int stb_ti_launch(const stb_table_view &V, const stb_rest_view &r, const stb_cnts_tT &c, const stb_cust_ro &cu, unsigned flags,
                  const stb_draw_key &k, int nsweeps, hipStream_t st) {
  const int I = r.I;
  if (I <= 0 || nsweeps <= 0) return 0;
  if (ti_form(I) == 0) {
    STB_LAUNCH(k_tindic_lane, dim3((unsigned)((I + 63) / 64)), dim3(64), st, V.tab, V.N, V.M, r.a, r.bpar, I, r.koff, c.n, c.t,
               c.T, r.h, cu.off, cu.cust, flags, k.seed, k.sweep, nsweeps);
  } else {
    unsigned cap = r.maxK;
    if (cap > STB_TI_LDS_CAP) cap = STB_TI_LDS_CAP;
    if (!cu.cust) cap = 0;
    STB_LAUNCH_SHM(k_tindic_wave, dim3((unsigned)I), dim3(64), sizeof(uint16_t) * (cap ? cap : 1), st, V.tab, V.N, V.M, r.a,
                   r.bpar, I, r.koff, c.n, c.t, c.T, r.h, cu.off, cu.cust, flags, k.seed, k.sweep, nsweeps, cap);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int stb_sample_tindic(const double *d_vtable, unsigned N, unsigned M, double a, const double *d_bpar, int I,
                                 const uint64_t *d_koff, const uint32_t *d_n, uint16_t *d_t, uint32_t *d_T, const double *d_h,
                                 const uint64_t *d_coff, const uint32_t *d_cust, unsigned flags, uint64_t seed, uint64_t sweep,
                                 void *stream) {
  STB_ENTRY;
  if (!(a >= 0.0 && a < 1.0)) return stb_fail("stb_sample_tindic: discount a=%g outside [0, 1)", a);
  if (N < 1 || M < 1) return stb_fail("stb_sample_tindic: table bounds N=%u M=%u", N, M);
  if (M > 65535u) return stb_fail("stb_sample_tindic: M=%u (t is a uint16: at most 65535)", M);
  if (flags & ~STB_TI_REF_ODDS_FLAG) return stb_fail("stb_sample_tindic: unknown flags 0x%x", flags);
  if (I < 0) return stb_fail("stb_sample_tindic: I=%d", I);
  const stb_table_view V = {d_vtable, N, M};
  const stb_rest_view r = {a, d_bpar, I, d_koff, d_h, STB_TI_LDS_CAP};
  const stb_cnts_tT c = {d_n, d_t, d_T};
  const stb_cust_ro cu = {d_coff, nullptr, d_cust};
  return stb_ti_launch(V, r, c, cu, flags, {seed, sweep}, 1, (hipStream_t)stream);
}
