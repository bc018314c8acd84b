// tdish.hip -- the step of a Pitman-Yor Gibbs sampler that moves data, on the device: every customer leaves its dish and
// is seated again, at any dish of its restaurant, under a likelihood that is a fixed table during the sweep
// (include/stb_hip.h, "dishes"; the derivation is DESIGN.md section 6).  The likelihood being fixed, restaurants stay
// independent: one wave per restaurant, lanes over dishes, no workgroup waits for another.
//
//   k_tdish<true>    K_i <= 64: a dish a lane; n, t, h, A, B in registers
//   k_tdish<false>   K_i <= STB_TD_MAXK: n, t, A, B and the cumulative weights in LDS, 64 dishes a trip
//
// A pair's seating weight is z = L (A + g B), g = b + T a, with A (an old table) and B (a new one, but for g) functions of
// the pair's own (n, t, h): they are kept with the pair and evaluated again only for the dish left and the dish entered,
// the two V cells each needs read by every lane at once.  The cumulative sums are taken in the association the header
// fixes -- a Kogge-Stone scan inside a block of 64 dishes, block bases added in sequence -- so the draws depend on
// neither form nor launch geometry.  The removal and the new-table decision are tindic.h's ti_remove and ti_add on the
// cells stb_sample_tindic reads: a customer that can only stay in its dish gets that sweep's bits.

#include "stb_common.h"
#include "tindic.h"

#pragma clang fp contract(off)

// V^n_m, 0 where the table has no such row (n > N cannot happen while sum_k n_k = N_i <= N; a raw caller's counts that
// break this read nothing out of bounds)
__device__ __forceinline__ double td_V(const double *vt, unsigned N, unsigned M, unsigned n, unsigned m) {
  if (n > N) return 0.0;
  return ti_V(vt, M, n, m);
}

// A and B of a pair (n, t, h): Vt = V^n_t, Vt1 = V^n_{t+1}
__device__ __forceinline__ void td_AB(unsigned n, unsigned t, double h, double a, unsigned M, double Vt, double Vt1, double &A,
                                      double &B) {
#pragma clang fp contract(off)
  if (n == 0) {
    A = 0.0;
    B = h;
    return;
  }
  const double dn = (double)n;
  const double U = t == 1 ? dn - a : (dn - (double)t * a) + 1.0 / Vt;
  A = U * (double)(n - t + 1) / dn;
  const double R = t + 1 > M ? 0.0 : (t == n ? 1.0 : (dn - (double)(t + 1) * a) * Vt1 + 1.0);
  B = h * (double)t * R / dn;
}

__device__ __forceinline__ double td_z(double L, double A, double g, double B) {
#pragma clang fp contract(off)
  const double gB = g * B;
  return L * (A + gB);
}

// (the inclusive Kogge-Stone scan, the readlanes and the choice are wave.h's)

template <bool REG>
__global__ __launch_bounds__(64) void k_tdish(const double *vt, unsigned N, unsigned M, double a, const double *bpar, int I,
                                              const uint64_t *koff, uint32_t *nv, uint16_t *tv, uint32_t *Tv, const double *hv,
                                              const uint64_t *coff, uint32_t *cust, const uint32_t *cls, const double *lik,
                                              unsigned rows, unsigned stride, uint64_t seed, uint64_t sweep0, int nsweeps,
                                              unsigned cap, unsigned long long *info) {
  extern __shared__ double td_lds[];  // LDS form: A[cap], B[cap], cum[cap], then n[cap] (uint32), t[cap] (uint16)
  const int i = blockIdx.x;
  if (i >= I) return;
  const unsigned lane = threadIdx.x;
  const uint64_t kg = koff[i], Kl = koff[i + 1] - kg, c0 = coff[i], c1 = coff[i + 1], C = coff[I];
  if (c1 - c0 > (uint64_t)N || Kl > (uint64_t)cap || (lik && Kl > (uint64_t)stride)) {
    if (lane == 0 && info) atomicAdd(&info[0], 1ull);
    return;
  }
  if (c1 == c0) return;
  const unsigned K = (unsigned)Kl;
  double *lA = td_lds, *lB = lA + cap, *lcum = lB + cap;
  uint32_t *ln = (uint32_t *)(lcum + cap);
  uint16_t *lt = (uint16_t *)(ln + cap);
  const double b = bpar[i];
  uint32_t T = Tv[i];
  unsigned long long stuck = 0;

  // this lane's dish (register form)
  unsigned rn = 0, rt = 0;
  double rh = 0.0, rA = 0.0, rB = 0.0;
  if (REG) {
    if (lane < K) {
      rn = nv[kg + lane];
      rt = tv[kg + lane];
      rh = hv ? hv[kg + lane] : 1.0;
      td_AB(rn, rt, rh, a, M, td_V(vt, N, M, rn, rt), td_V(vt, N, M, rn, rt + 1), rA, rB);
    }
  } else {
    for (unsigned k = lane; k < K; k += 64) {
      const unsigned n = nv[kg + k], t = tv[kg + k];
      double A, B;
      td_AB(n, t, hv ? hv[kg + k] : 1.0, a, M, td_V(vt, N, M, n, t), td_V(vt, N, M, n, t + 1), A, B);
      ln[k] = n;
      lt[k] = (uint16_t)t;
      lA[k] = A;
      lB[k] = B;
    }
    __syncthreads();
  }
  const unsigned nblk = (K + 63) / 64;

  for (int s = 0; s < nsweeps; s++) {
    const uint64_t key = stb_mix64(seed + (sweep0 + (uint64_t)s + 1) * STB_GAMMA);
    for (uint64_t cb = c0; cb < c1; cb += 64) {
      const unsigned Lc = c1 - cb < 64 ? (unsigned)(c1 - cb) : 64u;
      unsigned mk = 0, mc = 0;  // this lane's customer of the chunk: its dish and class
      if (lane < Lc) {
        mk = cust[cb + lane];
        mc = cls && lik ? cls[cb + lane] : 0;
      }
      const unsigned mk_in = mk;
      for (unsigned j = 0; j < Lc; j++) {
        const unsigned k0 = stb_wave_rl(mk, j), cl = stb_wave_rl(mc, j);
        const uint64_t c = cb + j;
        if (k0 >= K) continue;  // (not a dish of this restaurant: a raw caller's error, nothing is touched)
        // ---- 1. remove
        const unsigned n0 = REG ? stb_wave_rl(rn, k0) : ln[k0], t0 = REG ? stb_wave_rl(rt, k0) : lt[k0];
        if (n0 == 0 || T == 0) continue;  // (counts that do not hold the customer: likewise)
        const double A0 = REG ? stb_wave_rld(rA, k0) : lA[k0], B0 = REG ? stb_wave_rld(rB, k0) : lB[k0];
        const double h0 = REG ? stb_wave_rld(rh, k0) : (hv ? hv[kg + k0] : 1.0);
        const uint32_t T0 = T;
        unsigned n = n0, t = t0;
        if (n >= 2) {
          if (ti_remove(n, t, stb_unit(key, 2 * c + 1))) t--, T--;
          n--;
        } else {
          n = 0, t = 0, T--;
        }
        {
          double A, B;
          td_AB(n, t, h0, a, M, td_V(vt, N, M, n, t), td_V(vt, N, M, n, t + 1), A, B);
          if (REG) {
            if (lane == k0) rn = n, rt = t, rA = A, rB = B;
          } else {
            ln[k0] = n, lt[k0] = (uint16_t)t, lA[k0] = A, lB[k0] = B;
          }
        }
        // ---- 2. weights, 3. their cumulative sums
        const double g = b + (double)T * a;
        const bool lrow = lik && cl < rows;  // (a class outside the matrix: every L is 0, the customer stays)
        double Z, cum = 0.0;
        uint64_t pos = 0;  // register form: dishes with z > 0; LDS form: lane j holds block j's
        if (REG) {
          const double Lk = lik ? (lrow && lane < K ? lik[(uint64_t)cl * stride + lane] : 0.0) : 1.0;
          const double z = lane < K ? td_z(Lk, rA, g, rB) : 0.0;
          cum = 0.0 + stb_wave_scan(z, lane);
          pos = __ballot(z > 0.0);
          Z = stb_wave_rld(cum, 63);
        } else {
          double base = 0.0;
          for (unsigned blk = 0; blk < nblk; blk++) {
            const unsigned k = blk * 64 + lane;
            const double Lk = lik ? (lrow && k < K ? lik[(uint64_t)cl * stride + k] : 0.0) : 1.0;
            const double z = k < K ? td_z(Lk, lA[k], g, lB[k]) : 0.0;
            const double cm = base + stb_wave_scan(z, lane);
            lcum[k] = cm;  // (cap is a multiple of 64)
            const uint64_t pm = __ballot(z > 0.0);
            if (lane == blk) pos = pm;
            base = stb_wave_rld(cm, 63);
          }
          Z = base;
        }
        if (!(Z > 0.0 && isfinite(Z))) {  // nowhere to go: back to k0 as it was
          if (REG) {
            if (lane == k0) rn = n0, rt = t0, rA = A0, rB = B0;
          } else {
            ln[k0] = n0, lt[k0] = (uint16_t)t0, lA[k0] = A0, lB[k0] = B0;
          }
          T = T0;
          stuck++;
          continue;
        }
        const double thr = stb_unit(key, 2 * C + 1 + c) * Z;
        unsigned ks = 0;
        if (REG) {
          ks = stb_wave_choice(pos, cum, thr, lane);
        } else {
          bool found = false;
          unsigned lastb = 0;
          uint64_t lastm = 0;
          for (unsigned blk = 0; blk < nblk && !found; blk++) {
            const uint64_t pm = stb_wave_rl64(pos, blk);
            const uint64_t hit = __ballot(((pm >> lane) & 1) && lcum[blk * 64 + lane] > thr);
            if (hit) {
              ks = blk * 64 + (unsigned)__builtin_ctzll(hit);
              found = true;
            }
            if (pm) lastb = blk, lastm = pm;
          }
          if (!found) ks = lastb * 64 + 63u - (unsigned)__builtin_clzll(lastm);
        }
        // ---- 4. seat
        n = REG ? stb_wave_rl(rn, ks) : ln[ks];
        t = REG ? stb_wave_rl(rt, ks) : lt[ks];
        const double hs = REG ? stb_wave_rld(rh, ks) : (hv ? hv[kg + ks] : 1.0);
        if (n == 0) {
          n = 1, t = 1, T++;
        } else {
          n++;
          if (ti_add(n, t, T, hs, a, b, td_V(vt, N, M, n, t + 1), stb_unit(key, 2 * c + 2), false)) t++, T++;
        }
        {
          double A, B;
          td_AB(n, t, hs, a, M, td_V(vt, N, M, n, t), td_V(vt, N, M, n, t + 1), A, B);
          if (REG) {
            if (lane == ks) rn = n, rt = t, rA = A, rB = B;
          } else {
            ln[ks] = n, lt[ks] = (uint16_t)t, lA[ks] = A, lB[ks] = B;
          }
        }
        if (lane == j) mk = ks;
      }
      if (lane < Lc && mk != mk_in) cust[cb + lane] = mk;
    }
  }
  if (REG) {
    if (lane < K) {
      nv[kg + lane] = rn;
      tv[kg + lane] = (uint16_t)rt;
    }
  } else {
    __syncthreads();
    for (unsigned k = lane; k < K; k += 64) {
      nv[kg + k] = ln[k];
      tv[kg + k] = lt[k];
    }
  }
  if (lane == 0) {
    Tv[i] = T;
    if (stuck && info) atomicAdd(&info[1], stuck);
  }
}

__global__ __launch_bounds__(256) void k_td_class_counts(const uint32_t *cust, const uint32_t *cls, uint64_t C, unsigned rows,
                                                         unsigned stride, uint32_t *cnt) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const unsigned r = cls[c], k = cust[c];
  if (r < rows && k < stride) atomicAdd(&cnt[(uint64_t)r * stride + k], 1u);
}

int stb_td_launch(const stb_table_view &V, const stb_rest_view &r, const stb_cnts_rw &c, const stb_cust_rw &cu,
                  const stb_lik_view &L, const stb_draw_key &k, int nsweeps, unsigned long long *d_info, hipStream_t st) {
  const int I = r.I;
  if (I <= 0 || nsweeps <= 0) return 0;
  unsigned cap = r.maxK;
  if (cap > STB_TD_MAXK) cap = STB_TD_MAXK;
  if (cap <= 64) {
    STB_LAUNCH(k_tdish<true>, dim3((unsigned)I), dim3(64), st, V.tab, V.N, V.M, r.a, r.bpar, I, r.koff, c.n, c.t, c.T, r.h,
               cu.off, cu.cust, cu.cls, L.lik, L.rows, L.stride, k.seed, k.sweep, nsweeps, 64u, d_info);
  } else {
    cap = (cap + 63u) & ~63u;
    const size_t shm = (size_t)cap * (3 * sizeof(double) + sizeof(uint32_t) + sizeof(uint16_t));
    STB_LAUNCH_SHM(k_tdish<false>, dim3((unsigned)I), dim3(64), shm, st, V.tab, V.N, V.M, r.a, r.bpar, I, r.koff, c.n, c.t, c.T,
                   r.h, cu.off, cu.cust, cu.cls, L.lik, L.rows, L.stride, k.seed, k.sweep, nsweeps, cap, d_info);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int stb_td_class_counts(const stb_cust_ro &cu, unsigned rows, unsigned stride, uint32_t *d_cnt, hipStream_t st) {
  if (cu.C == 0) return 0;
  STB_LAUNCH(k_td_class_counts, dim3((unsigned)((cu.C + 255) / 256)), dim3(256), st, cu.cust, cu.cls, cu.C, rows, stride, d_cnt);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int stb_sample_tdishes(const double *d_vtable, unsigned N, unsigned M, double a, const double *d_bpar, int I,
                                  const uint64_t *d_koff, uint32_t *d_n, uint16_t *d_t, uint32_t *d_T, const double *d_h,
                                  const uint64_t *d_coff, uint32_t *d_cust, const uint32_t *d_cls, const double *d_lik,
                                  unsigned rows, unsigned stride, uint64_t seed, uint64_t sweep, uint64_t *d_info, void *stream) {
  STB_ENTRY;
  const char *who = "stb_sample_tdishes";
  if (!(a >= 0.0 && a < 1.0)) return stb_fail("%s: discount a=%g outside [0, 1)", who, a);
  if (N < 1 || M < 1) return stb_fail("%s: table bounds N=%u M=%u", who, N, M);
  if (M > 65535u) return stb_fail("%s: M=%u (t is a uint16: at most 65535)", who, M);
  if (I < 0) return stb_fail("%s: I=%d", who, I);
  if (!d_cust) return stb_fail("%s: d_cust is required (a customer's dish is what the sweep writes)", who);
  if (!d_bpar || !d_koff || !d_n || !d_t || !d_T || !d_coff) return stb_fail("%s: bpar, koff, n, t, T and coff are required", who);
  if (d_lik && (!d_cls || rows < 1 || stride < 1))
    return stb_fail("%s: a likelihood needs d_cls, rows >= 1 and stride >= 1 (rows=%u, stride=%u)", who, rows, stride);
  const stb_table_view V = {d_vtable, N, M};
  const stb_rest_view r = {a, d_bpar, I, d_koff, d_h, STB_TD_MAXK};
  const stb_cnts_rw c = {d_n, d_t, d_T};
  const stb_cust_rw cu = {d_coff, d_cls, d_cust};
  const stb_lik_view L = {d_lik, rows, stride};
  return stb_td_launch(V, r, c, cu, L, {seed, sweep}, 1, (unsigned long long *)d_info, (hipStream_t)stream);
}
