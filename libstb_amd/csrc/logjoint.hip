// logjoint.hip -- the log joint probability of a sampler state, from the counts the sweeps hold on the device
// (include/stb_hip.h, stb_logjoint; an additive interface: the reference computes only fragments, test/check.c:195-209).
//
//     log p(n, t | a, b, h) = sum_i L_i,     L_i = P_i + H_i + R_i   (+ B_i with STB_LJ_INDICATORS)
//     P_i = sum_k S_S_a(n_ik, t_ik)                        pairs with n >= 1 (n = 0, t = 0 contributes 0)
//     H_i = sum_k t_ik log h_ik                            0 when h is NULL
//     R_i = log (b_i|a)_{T_i} - log (b_i)_{N_i}            T_i = sum_k t_ik, N_i = sum_k n_ik; 0 when N_i = 0
//     B_i = - sum_k log C(n_ik - 1, t_ik - 1)              the table-indicator representation: one indicator of a pair is
//                                                          held at 1 and the other n - 1 are uniform given t, as
//                                                          stb_sample_tindic draws them (tindic.hip's header)
//
//   k_logjoint   one pass over the pairs, one table gather a pair; a workgroup takes blocks of 256 restaurants grid-stride,
//                a wave one restaurant of the block at a time; nobody waits for anybody
//
// The association (no contraction anywhere; FP64 throughout; u32 / u64 integers are exact):
//   pair terms  (n, t, h) of a pair that enters the sums (see "left out" below), tc_S's cases (tcounts.h):
//       p = 0                                t = n
//           S1[n-1]                          t = 1 < n    (d_S1 NULL: lgamma((double)n - a) - lgamma(1.0 - a), what the
//                                                          fill writes into S1 -- fill_pc.hip, k_s1)
//           table[row_offset(n, M) + t - 2]  1 < t < n
//       q = (double)t * log(h)                                                          (h given)
//       c = -((lgamma((double)n) - lgamma((double)t)) - lgamma((double)(n - t) + 1.0)),  0.0 when t = 1 or t = n    (flag)
//   a restaurant's pairs are taken in chunks of 64 in CSR order, lane l the pair 64 j + l of chunk j (0.0 beyond K_i and
//       for pairs left out); a chunk is summed by the 64-lane shuffle tree v += shfl_down(v, o), o = 32, 16, .. 1; the
//       chunk sums are added in order j = 0, 1, .. in double-double (dd_add, stb_common.h), separately for p, q and c:
//       P_i = hi + lo, H_i = hi + lo, B_i = hi + lo.  T_i and N_i are summed as uint64 over ALL the restaurant's pairs.
//   R_i by one lane, T = (double)T_i, N = (double)N_i, b = b_i, la = log(a) from the host's libm (as k_joint_terms):
//       0.0                                                                    N_i = 0
//       (T la + (lgamma(T + b / a) - lgamma(b / a))) - (lgamma(b + N) - lgamma(b))      a > 0, b != 0
//       ((T - 1.0) la + lgamma(T)) - lgamma(N)                                 a > 0, b = 0, T_i >= 1 (the factor b of both
//                                                                              rising factorials cancelled; 0.0 at T_i = 0)
//       T log(b) - (lgamma(b + N) - lgamma(b))                                 a = 0
//     lgamma is log |Gamma|.  The sign of Gamma matters only for -a < b < 0 (a > 0): then -1 < b / a < 0 and -1 < b < 0, so
//     Gamma(b / a) and Gamma(b) are both negative while Gamma(T + b / a) and Gamma(b + N) are positive for T_i, N_i >= 1
//     (b + N_i and b lie on opposite sides of zero exactly when b / a + T_i and b / a do; a second sign change cannot
//     happen for b > -a > -1).  Both rising factorials carry the one negative factor b, their quotient is positive, and
//     the difference of the log |Gamma| values is its logarithm.
//   L_i = ((P_i + H_i) + R_i) + B_i in plain doubles, -inf when the restaurant holds an impossible pair.
//   Over restaurants, separately for P, H, R and B: restaurants 256 k .. 256 k + 255 (0.0 beyond I) are block k, summed in
//       one fixed tree: (x[l] + x[l + 64]) + (x[l + 128] + x[l + 192]) per lane l, then the shuffle tree (32 .. 1).  The
//       block sums go to partial[k][4]; the last workgroup to finish -- a ticket, as in k_joint_terms: nobody waits -- adds
//       the blocks k = 0, 1, 2, .. in double-double, one lane a component; info's components are hi + lo of each, and the
//       total is hi + lo of the four double-doubles merged in the order P, H, R, B.
// So the bits of every output depend on neither the grid nor the workgroup size: STB_LOGJOINT_WAVES = 1, 2, 4 or 8 waves a
// workgroup give the same bits (default: 4, and 8 where the blocks are fewer than twice the compute units).
//
// Left out and impossible (counted in u64, exact in any order):
//   impossible  S_S is log 0 -- t = 0 with n > 0, or t > n -- or h is not a positive finite number.  The pair adds
//               nothing to the sums; its restaurant's L_i, the component it belongs to (pairs, or base for a bad h) and
//               the total are -inf.  Every sum stays finite until then: no NaN is ever produced.
//   outside     the table cannot answer: n > N, or 1 < t < n with t > M or without a table (d_table NULL).  The pair is
//               left out of P, H and B (stb_sample_partition's cnt[0] convention); it still counts in T_i and N_i.
//   t_mismatch  d_T given and d_T[i] != the kernel's own sum of t: the kernel's sum is the one used.
//
// What sets the pace: a restaurant of K pairs costs one coalesced read of (n, t, h) and one gathered table cell a pair,
// three shuffle trees a chunk at most, and four lgamma evaluations for R_i -- which the threads of the workgroup take for
// the block's 256 restaurants side by side, one restaurant a lane, after the waves have left P_i, H_i, B_i, T_i and N_i in
// LDS.  The last workgroup stages the block sums in LDS so that the ordered double-double sum reads no global memory.

#include "stb_common.h"
#include "tcounts.h"
#include "logjoint.h"
#include "ticket.h"

#define LJ_BLOCK STB_TG_BLOCK  // (one constant for the kernel, the launch and stb_reduce_geometry)
#define LJ_MAXTHREADS 512
#define LJ_STAGE 1024  // block sums (x 4 components) the last workgroup stages in LDS at a time

#define LJ_IMP_P 1u
#define LJ_IMP_H 2u

// ctl: [0] ticket (u32); as u64 words 1 .. 4: outside, impossible (S), impossible (h), t_mismatch -- zeroed on the stream
// ahead of the launch.  host: [0..3] pairs, base, restaurants, binom, [4] total, [5..7] (as u64) outside, impossible, t_mismatch
__global__ __launch_bounds__(LJ_MAXTHREADS) void k_logjoint(const double *table, const double *S1, unsigned N, unsigned M,
                                                            double a, double la, const double *bpar, uint64_t I,
                                                            const uint64_t *koff, const uint32_t *nv, const uint16_t *tv,
                                                            const uint32_t *Tv, const double *hv, unsigned flags, double *Li,
                                                            double *partial, unsigned nblk, unsigned *ctl, double *host) {
#pragma clang fp contract(off)
  __shared__ double sx[4][LJ_BLOCK];  // P_i, H_i, R_i, B_i of the block's restaurants
  __shared__ unsigned long long sT[LJ_BLOCK], sN[LJ_BLOCK];
  __shared__ unsigned sflag[LJ_BLOCK];
  __shared__ double stage[4][LJ_STAGE];
  __shared__ unsigned s_last;
  const unsigned nthr = blockDim.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nw = nthr >> 6;
  const bool want_b = (flags & STB_LJ_INDICATORS) != 0;
  unsigned long long c_out = 0, c_imp_p = 0, c_imp_h = 0, c_mis = 0;  // per lane, over everything the lane sees
  for (unsigned blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const uint64_t i0 = (uint64_t)blk * LJ_BLOCK;
    // ---- the pairs: a wave a restaurant
    for (unsigned r = wave; r < LJ_BLOCK && i0 + r < I; r += nw) {
      const uint64_t i = i0 + r;
      const uint64_t k0 = koff[i], k1 = koff[i + 1];
      dd_t accP{0.0, 0.0}, accH{0.0, 0.0}, accB{0.0, 0.0};
      unsigned long long sumT = 0, sumN = 0;
      unsigned imp = 0;
      for (uint64_t base = k0; base < k1; base += 64) {
        const uint64_t g = base + lane;
        double p = 0.0, q = 0.0, c = 0.0;
        if (g < k1) {
          const unsigned n = nv[g], t = tv[g];
          sumT += t;
          sumN += n;
          if (n == 0 ? t != 0 : (t == 0 || t > n)) {
            imp |= LJ_IMP_P;
            c_imp_p++;
          } else if (n != 0) {
            bool in = true;
            if (n > N) in = false;
            else if (t == n) p = 0.0;
            else if (t == 1) p = S1 ? S1[n - 1] : lgamma((double)n - a) - lgamma(1.0 - a);
            else if (t > M || !table) in = false;
            else p = table[stb_row_offset(n, M) + (t - 2)];
            if (!in) {
              c_out++;
            } else if (hv) {
              const double h = hv[g];
              if (h > 0.0 && isfinite(h)) {
                q = (double)t * log(h);
              } else {
                imp |= LJ_IMP_H;
                c_imp_h++;
                p = 0.0;
                in = false;
              }
            }
            if (in && want_b && t != n && t != 1)
              c = -((lgamma((double)n) - lgamma((double)t)) - lgamma((double)(n - t) + 1.0));
          }
        }
        dd_add(accP, stb_wave_sum(p));
        if (hv) dd_add(accH, stb_wave_sum(q));
        if (want_b) dd_add(accB, stb_wave_sum(c));
      }
      sumT = stb_wave_sum(sumT);
      sumN = stb_wave_sum(sumN);
      const unsigned any_p = __ballot(imp & LJ_IMP_P) != 0ull ? LJ_IMP_P : 0u;
      const unsigned any_h = __ballot(imp & LJ_IMP_H) != 0ull ? LJ_IMP_H : 0u;
      if (lane == 0) {
        sx[0][r] = accP.hi + accP.lo;
        sx[1][r] = accH.hi + accH.lo;
        sx[3][r] = accB.hi + accB.lo;
        sT[r] = sumT;
        sN[r] = sumN;
        sflag[r] = any_p | any_h;
      }
    }
    __syncthreads();
    // ---- the restaurants' own terms: a lane a restaurant
    for (unsigned r = tid; r < LJ_BLOCK; r += nthr) {
      const uint64_t i = i0 + r;
      if (i < I) {
        const unsigned long long Ti = sT[r], Ni = sN[r];
        if (Tv && (unsigned long long)Tv[i] != Ti) c_mis++;
        double R = 0.0;
        if (Ni > 0) {
          const double T = (double)Ti, Nd = (double)Ni, b = bpar[i];
          if (a > 0.0) {
            if (b != 0.0) {
              const double cc = b / a;
              R = (T * la + (lgamma(T + cc) - lgamma(cc))) - (lgamma(b + Nd) - lgamma(b));
            } else {
              R = Ti > 0 ? ((T - 1.0) * la + lgamma(T)) - lgamma(Nd) : 0.0;
            }
          } else {
            R = T * log(b) - (lgamma(b + Nd) - lgamma(b));
          }
        }
        sx[2][r] = R;
        if (Li) Li[i] = sflag[r] ? -HUGE_VAL : ((sx[0][r] + sx[1][r]) + R) + sx[3][r];
      } else {
        sx[0][r] = 0.0;
        sx[1][r] = 0.0;
        sx[2][r] = 0.0;
        sx[3][r] = 0.0;
      }
    }
    __syncthreads();
    // ---- the block's four sums, one fixed tree each
    for (unsigned q = wave; q < 4; q += nw) {
      const double *x = sx[q];
      const double v = stb_wave_sum((x[lane] + x[lane + 64]) + (x[lane + 128] + x[lane + 192]));
      if (lane == 0) partial[(size_t)blk * 4 + q] = v;
    }
    __syncthreads();
  }
  // the counters: integers, exact in any order
  c_out = stb_wave_sum(c_out);
  c_imp_p = stb_wave_sum(c_imp_p);
  c_imp_h = stb_wave_sum(c_imp_h);
  c_mis = stb_wave_sum(c_mis);
  unsigned long long *cnt = (unsigned long long *)ctl;
  if (lane == 0) {
    if (c_out) __hip_atomic_fetch_add(&cnt[1], c_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (c_imp_p) __hip_atomic_fetch_add(&cnt[2], c_imp_p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (c_imp_h) __hip_atomic_fetch_add(&cnt[3], c_imp_h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (c_mis) __hip_atomic_fetch_add(&cnt[4], c_mis, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!stb_ticket_last(ctl, gridDim.x, &s_last)) return;  // (ticket.h: the block sums and the counters are published)
  dd_t acc{0.0, 0.0};  // lanes 0 .. 3 of wave 0: one component each
  for (unsigned c0 = 0; c0 < nblk; c0 += LJ_STAGE) {
    const unsigned cn = nblk - c0 < LJ_STAGE ? nblk - c0 : LJ_STAGE;
    for (unsigned e = tid; e < cn * 4; e += nthr) stage[e & 3][e >> 2] = partial[(size_t)c0 * 4 + e];
    __syncthreads();
    if (tid < 4)
      for (unsigned c = 0; c < cn; c++) dd_add(acc, stage[tid][c]);
    __syncthreads();
  }
  if (wave != 0) return;
  // the total: the four double-doubles merged in the order P, H, R, B (lane 0 gathers them)
  dd_t tot{0.0, 0.0};
  double comp[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    dd_t o;
    o.hi = __shfl(acc.hi, q, 64);
    o.lo = __shfl(acc.lo, q, 64);
    comp[q] = o.hi + o.lo;
    dd_merge(tot, o);
  }
  if (tid == 0) {
    const unsigned long long n_out = __hip_atomic_load(&cnt[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long n_imp_p = __hip_atomic_load(&cnt[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long n_imp_h = __hip_atomic_load(&cnt[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long n_mis = __hip_atomic_load(&cnt[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    host[0] = n_imp_p ? -HUGE_VAL : comp[0];
    host[1] = n_imp_h ? -HUGE_VAL : comp[1];
    host[2] = comp[2];
    host[3] = comp[3];
    host[4] = (n_imp_p | n_imp_h) ? -HUGE_VAL : tot.hi + tot.lo;
    unsigned long long *hc = (unsigned long long *)(host + 5);
    hc[0] = n_out;
    hc[1] = n_imp_p + n_imp_h;
    hc[2] = n_mis;
  }
}

// ------------------------------------------------------------------------------------------------
// per calling thread: the block sums, the ticket and counters, and the pinned words the kernel answers in.  A call
// waits for its answer before it returns, so one set per thread is never in use twice.

static thread_local stb_tset lj;  // d_buf: block sums of four doubles

extern "C" void stb_lj_release(void) {
  STB_ENTRY;
  stb_tset_drop(lj);
}

int stb_lj_check(double a, unsigned flags, int I, const char *who) {
  if (!(a >= 0.0 && a < 1.0)) return stb_fail("%s: discount a=%g outside [0, 1)", who, a);
  if (flags & ~STB_LJ_INDICATORS) return stb_fail("%s: unknown flags 0x%x", who, flags);
  if (I < 0) return stb_fail("%s: I=%d", who, I);
  return 0;
}

// one launch on st, the copy of d_Li to Li_host (when both are given), one wait; the arguments are checked by the caller
int stb_lj_run(const stb_table_view &S, const stb_rest_view &r, const stb_cnts_ro &c, unsigned flags, double *d_Li,
               double *Li_host, double *total_host, stb_logjoint_info_t *info, hipStream_t st, const char *who) {
  const int I = r.I;
  const double a = r.a;
  if (I == 0) {
    if (total_host) *total_host = 0.0;
    if (info) memset(info, 0, sizeof(*info));
    return 0;
  }
  if (stb_device_count() < 1) return stb_no_device(who);
  stb_tgeom tg;
  if (stb_ticket_geom(STB_GEOM_LOGJOINT, (uint64_t)I, 0, 0, 0, &tg)) return stb_fail("%s: no launch geometry for I=%d", who, I);
  if (stb_tset_ready(lj, who) || stb_tset_room(lj, tg.need, STB_TG_CAP0_BLOCKS, 4 * sizeof(double), who)) return 1;
  const unsigned nblk = tg.nblk, grid = tg.gx;
  const int nw = (int)tg.waves;
  HIPCHK(hipMemsetAsync(lj.d_ctl, 0, 64, st));
  STB_LAUNCH(k_logjoint, dim3(grid), dim3(64 * nw), st, S.tab, S.S1, S.N, S.M, a, a > 0.0 ? log(a) : 0.0, r.bpar,
             (uint64_t)I, r.koff, c.n, c.t, c.T, r.h, flags, d_Li, (double *)lj.d_buf, nblk, lj.d_ctl, lj.h_out_dev);
  HIPCHK(hipGetLastError());
  if (d_Li && Li_host) HIPCHK(hipMemcpyAsync(Li_host, d_Li, sizeof(double) * (size_t)I, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const volatile double *h = (const volatile double *)lj.h_out;
  const volatile uint64_t *hc = (const volatile uint64_t *)(lj.h_out + 5);
  if (total_host) *total_host = h[4];
  if (info) {
    info->pairs = h[0];
    info->base = h[1];
    info->restaurants = h[2];
    info->binom = h[3];
    info->outside = hc[0];
    info->impossible = hc[1];
    info->t_mismatch = hc[2];
  }
  return 0;
}

extern "C" int stb_reduce_geometry(int which, uint64_t I, int D, int J, int waves, stb_reduce_geom_t *out) {
  STB_ENTRY;
  if (!out) return stb_fail("stb_reduce_geometry: null argument");
  if (which == STB_GEOM_JOINT_TERMS && (D < 1 || J < 1 || D > 64 || J > 64))
    return stb_fail("stb_reduce_geometry: a grid of %d x %d (1..64 each way)", D, J);
  if (stb_device_count() < 1) return stb_no_device("stb_reduce_geometry");
  stb_tgeom tg;
  if (stb_ticket_geom(which, I, D, J, waves, &tg))
    return stb_fail("stb_reduce_geometry: which=%d, I=%llu, waves=%d (which 0..2, I >= 1, waves 0, 1, 2, 4 or 8)", which,
                    (unsigned long long)I, waves);
  out->grid_x = tg.gx;
  out->grid_y = tg.gy;
  out->steps = tg.steps;
  out->chunks = tg.cps;
  out->blocks = tg.nblk;
  out->waves = tg.waves;
  out->need = tg.need;
  out->cap0 = tg.cap0;
  return 0;
}

extern "C" int stb_logjoint(const double *d_table, const double *d_S1, unsigned N, unsigned M, double a, const double *d_bpar,
                            int I, const uint64_t *d_koff, const uint32_t *d_n, const uint16_t *d_t, const uint32_t *d_T,
                            const double *d_h, unsigned flags, double *d_Li, double *total_host, stb_logjoint_info_t *info,
                            void *stream) {
  STB_ENTRY;
  if (stb_lj_check(a, flags, I, "stb_logjoint")) return 1;
  if (N < 1 || M < 1) return stb_fail("stb_logjoint: table bounds N=%u M=%u", N, M);
  if (!d_koff || !d_n || !d_t) return stb_fail("stb_logjoint: the pair offsets, n and t are required");
  if (I > 0 && !d_bpar) return stb_fail("stb_logjoint: bpar is required");
  if (!total_host) return stb_fail("stb_logjoint: total_host is required");
  const stb_table_view S = {d_table, N, M, d_S1};
  const stb_rest_view r = {a, d_bpar, I, d_koff, d_h};
  return stb_lj_run(S, r, {d_n, d_t, d_T}, flags, d_Li, nullptr, total_host, info, (hipStream_t)stream, "stb_logjoint");
}
