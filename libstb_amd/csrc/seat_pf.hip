// seat_pf.hip -- the forward seating as a particle filter: the R particles of a restaurant seat its customers side by
// side, and after any customer those with negligible weight may be replaced by copies of the heavy ones (systematic
// resampling, triggered by the effective sample size).  include/stb_hip.h, stb_seat_filter; the law and the bars are
// DESIGN.md section 6, the replay is tests/pf_oracle.py.  An additive interface: the reference has no counterpart.
//
//   k_seat_pf   a workgroup a restaurant, W = 1, 2, 4 or 8 waves; slot r is wave r mod W's.  The slots' n and t live in
//               LDS in two buffers (dynamic: 2 x R x K' x 6 bytes, K' = K_i rounded up to even), T and N beside them.  A
//               visit is seat_visit.h's st_visit on one slot: K_i <= 64 takes the pair into registers for the visit (a
//               dish a lane, h and the customer's row of L loaded once a wave, not once a slot), larger K_i works on the
//               slot's LDS as k_seat<false> does on its wave's.
//
// Between customers the waves meet once.  Every wave writes its slots' new weights w_r p_c(r) to LDS (two vectors, by the
// customer's parity, so that a fast wave's next weights never land on what a slow wave still reads), the workgroup
// barrier makes them visible, and then every wave does the whole of steps 2 to 5 redundantly on the same 64 values, a
// slot a lane: the rescaling, the two scans, the decision, the ancestors.  The waves therefore agree on everything with
// no second barrier, and w, Zm, E and the counters live in registers.  A resampling copies slot A_j of the current buffer
// to slot j of the other one, each wave for its own j, and the buffers swap: nobody writes the buffer that is read from,
// and a wave writes only its own slots of the other.  The next copy in the opposite direction lies behind the next
// barrier.  When the decision is no, nothing is copied.
//
// Only + - x /, comparisons, conversions, ilogb and ldexp by integers decide the path, so states, w, E and the counts are
// bit-equal to the replay whatever W is; H_i holds the one logarithm.

#include <climits>

#include "stb_common.h"
#include "seat.h"
#include "seat_pf.h"
#include "seat_visit.h"
#include "ticket.h"

#pragma clang fp contract(off)

#define PF_MAXTHREADS 512
#define PF_LDS_TOTAL 65536u                    // what a workgroup takes at most: no more than the other kernels assume
#define PF_LDS_FIXED 4096u                     // kept for the static part: T, N (2 x 2 x 64 x 8) and the weights (2 x 64 x 8)
#define PF_LDS_DYN (PF_LDS_TOTAL - PF_LDS_FIXED)
#define PF_LN2 0.6931471805599453094

struct pf_args {
  double tau;
  double *Hi, *w;
  long long *E;
  uint32_t *res, *pn;
  uint16_t *pt;
};

// dishes of a slot as laid out: even, so that the uint16 rows keep the uint32 rows behind them aligned
__host__ __device__ static inline unsigned pf_kp(unsigned K) { return K < 2 ? 2u : (K + 1u) & ~1u; }

__host__ __device__ static inline unsigned pf_budget(unsigned K) {
  const unsigned r = PF_LDS_DYN / (12u * pf_kp(K));
  return r > STB_PF_MAXR ? (unsigned)STB_PF_MAXR : r;
}

__global__ __launch_bounds__(PF_MAXTHREADS) void k_seat_pf(seat_args A, pf_args P) {
  extern __shared__ unsigned char pf_lds[];
  __shared__ unsigned long long s_T[2][64], s_N[2][64];
  __shared__ double s_w[2][64];
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6, R = A.R, M = A.M;
  const double a = A.a, tau = P.tau;
  const double *hv = A.hv, *lik = A.lik;
  const uint64_t C = A.coff[A.I];
  // lane r: the key of slot r's stream (sweep + r, as particle r of k_seat)
  const uint64_t keyv = stb_mix64(A.seed + (A.sweep + (uint64_t)lane + 1) * STB_GAMMA);
  unsigned long long n_skip = 0, n_imp = 0, n_stuck = 0, n_dead = 0, n_res = 0;  // wave-uniform; the last two and the first are wave 0's

  for (uint64_t i = blockIdx.x; i < A.I; i += gridDim.x) {
    __syncthreads();  // the last restaurant's copies and weights are read
    const uint64_t kg = A.koff[i], K64 = A.koff[i + 1] - kg, c0 = A.coff[i], c1 = A.coff[i + 1];
    if (K64 > (uint64_t)STB_TD_MAXK || (lik && K64 > A.stride) || (K64 == 0 && c1 > c0) || R > pf_budget((unsigned)K64)) {
      if (wave == 0) n_skip++;
      if (threadIdx.x == 0) P.Hi[i] = 0.0;
      continue;
    }
    const unsigned K = (unsigned)K64, Kp = pf_kp(K), nblk = (K + 63) / 64;
    const bool reg = K <= 64;
    const size_t bufbytes = (size_t)R * Kp * 6u;
    const double b = A.bpar[i];
    auto np = [&](unsigned buf, unsigned r) { return (uint32_t *)(pf_lds + buf * bufbytes) + (size_t)r * Kp; };
    auto tp = [&](unsigned buf, unsigned r) { return (uint16_t *)(pf_lds + buf * bufbytes + (size_t)R * Kp * 4u) + (size_t)r * Kp; };

    // ---- the start state into this wave's slots of buffer 0; T and N are the kernel's own sums
    {
      unsigned long long sT = 0, sN = 0;
      for (unsigned k = lane; k < K; k += 64) {
        const unsigned n = A.nv[kg + k], t = A.tv[kg + k];
        for (unsigned r = wave; r < R; r += nw) np(0, r)[k] = n, tp(0, r)[k] = (uint16_t)t;
        sT += t;
        sN += n;
      }
      const unsigned long long T = __shfl(stb_wave_sum(sT), 0, 64), N = __shfl(stb_wave_sum(sN), 0, 64);
      for (unsigned r = wave; r < R; r += nw) s_T[0][r] = T, s_N[0][r] = N;  // (every lane the same value: each reads its own)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    const double rh = reg && lane < K ? (hv ? hv[kg + lane] : 1.0) : 0.0;

    unsigned cur = 0, res = 0;
    double wv = lane < R ? 1.0 : 0.0, Zm = 1.0, S1 = (double)R;
    long long E = 0;
    bool rdead = false;

    unsigned mcn = 0;  // the next chunk's classes, a lane a customer
    if (lik && c0 + lane < c1) mcn = A.cls[c0 + lane];
    double Lnext = 1.0;  // register form: the next customer's row of L, a lane a dish
    if (reg && lik && c0 < c1) {
      const unsigned cl = stb_wave_rl(mcn, 0);
      Lnext = cl < A.rows && lane < K ? lik[(uint64_t)cl * A.stride + lane] : 0.0;
    }
    for (uint64_t cb = c0; cb < c1; cb += 64) {
      const unsigned Lc = c1 - cb < 64 ? (unsigned)(c1 - cb) : 64u;
      const unsigned mc = mcn;
      mcn = 0;
      if (lik && cb + 64 + lane < c1) mcn = A.cls[cb + 64 + lane];
      for (unsigned j = 0; j < Lc; j++) {
        const uint64_t c = cb + j;
        const unsigned par = (unsigned)(c - c0) & 1u;
        const unsigned cl = stb_wave_rl(mc, j);
        const bool lrow = lik && cl < A.rows;
        const double Lcur = Lnext;
        if (reg && lik) {
          const unsigned cn = j + 1 < Lc ? stb_wave_rl(mc, j + 1) : stb_wave_rl(mcn, 0);
          const bool more = c + 1 < c1;
          Lnext = more && cn < A.rows && lane < K ? lik[(uint64_t)cn * A.stride + lane] : 0.0;
        }
        // ---- every slot of this wave seats customer c: st_visit, and 1. the weight
        for (unsigned r = wave; r < R; r += nw) {
          const uint64_t key = stb_wave_rl64(keyv, r);
          const double u2 = stb_unit(key, 2 * c + 2), u3 = stb_unit(key, 2 * C + 1 + c);
          uint32_t *ln = np(cur, r);
          uint16_t *lt = tp(cur, r);
          unsigned long long T = s_T[cur][r], N = s_N[cur][r];
          unsigned ks;
          double pc;
          bool imp = false;
          if (reg) {
            unsigned rn = lane < K ? ln[lane] : 0u, rt = lane < K ? (unsigned)lt[lane] : 0u;
            st_visit<true>(A, kg, K, 1u, a, b, M, lane, nullptr, nullptr, rn, rt, rh, Lcur, cl, lrow, u2, u3, T, N, ks, pc, imp,
                           n_imp, n_stuck);
            if (lane == ks) ln[ks] = rn, lt[ks] = (uint16_t)rt;
          } else {
            unsigned rn = 0, rt = 0;
            st_visit<false>(A, kg, K, nblk, a, b, M, lane, ln, lt, rn, rt, 0.0, 0.0, cl, lrow, u2, u3, T, N, ks, pc, imp, n_imp,
                            n_stuck);
          }
          s_T[cur][r] = T;
          s_N[cur][r] = N;
          if (!rdead) {
            const double wr = stb_wave_rld(wv, r) * pc;
            if (lane == 0) s_w[par][r] = wr;
          }
        }
        if (rdead) continue;  // (a dead restaurant is still seated; its slots never meet again)
        __syncthreads();
        // ---- 2. the rescaling by an exact power of two, every wave on the same 64 values
        double w = lane < R ? s_w[par][lane] : 0.0;
        const int ex = w > 0.0 ? ilogb(w) : INT_MIN;
        int e = ex;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
          const int o = __shfl_xor(e, off, 64);
          e = o > e ? o : e;
        }
        if (e == INT_MIN) {
          rdead = true;
          wv = w;
          if (wave == 0) n_dead++;
          continue;
        }
        w = (w > 0.0 && (long long)ex >= (long long)e - 1000) ? ldexp(w, -e) : 0.0;
        E += e;
        // ---- 3. the sums, 4. the decision
        const double cum = 0.0 + stb_wave_scan(w, lane);
        S1 = stb_wave_rld(cum, 63);
        const double S2 = stb_wave_rld(0.0 + stb_wave_scan(w * w, lane), 63);
        if (c + 1 < c1 && S1 * S1 < (tau * (double)R) * S2) {
          // ---- 5. systematic resampling on slot 0's u4
          Zm = Zm * (S1 / (double)R);
          const int ez = ilogb(Zm);
          Zm = ldexp(Zm, -ez);
          E += ez;
          const double u4 = stb_unit(stb_wave_rl64(keyv, 0), 2 * c + 1);
          const double thr = (((double)lane + u4) / (double)R) * S1;  // lane j: slot j's threshold
          const uint64_t pos = __ballot(w > 0.0);
          unsigned anc = 63u - (unsigned)__builtin_clzll(pos);
          bool found = false;
          for (unsigned r = 0; r < R; r++) {
            const double cr = stb_wave_rld(cum, r);
            if (!found && ((pos >> r) & 1) && cr > thr) anc = r, found = true;
          }
          for (unsigned jj = wave; jj < R; jj += nw) {
            const unsigned aj = stb_wave_rl(anc, jj);
            const uint32_t *sn = np(cur, aj);
            const uint16_t *st = tp(cur, aj);
            uint32_t *dn = np(cur ^ 1u, jj);
            uint16_t *dt = tp(cur ^ 1u, jj);
            for (unsigned k = lane; k < K; k += 64) dn[k] = sn[k], dt[k] = st[k];
            s_T[cur ^ 1u][jj] = s_T[cur][aj];
            s_N[cur ^ 1u][jj] = s_N[cur][aj];
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          cur ^= 1u;
          w = lane < R ? 1.0 : 0.0;
          res++;
        }
        wv = w;
      }
    }
    // ---- 6. the finish, and what the caller asked for
    if (wave == 0) {
      n_res += res;
      double H = 0.0;
      if (c1 > c0) {
        const double v = Zm * (S1 / (double)R);
        H = rdead || !(v > 0.0) ? -HUGE_VAL : log(v) + (double)E * PF_LN2;
      }
      if (lane == 0) {
        P.Hi[i] = H;
        if (P.E) P.E[i] = E;
        if (P.res) P.res[i] = res;
      }
      if (P.w && lane < R) P.w[i * R + lane] = wv;
    }
    if (P.pn || P.pt)
      for (unsigned r = wave; r < R; r += nw) {
        const uint32_t *ln = np(cur, r);
        const uint16_t *lt = tp(cur, r);
        const uint64_t o = kg * R + (uint64_t)r * K;
        for (unsigned k = lane; k < K; k += 64) {
          if (P.pn) P.pn[o + k] = ln[k];
          if (P.pt) P.pt[o + k] = lt[k];
        }
      }
  }
  if (lane == 0 && A.info) {
    if (n_skip) __hip_atomic_fetch_add(&A.info[0], n_skip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n_imp) __hip_atomic_fetch_add(&A.info[1], n_imp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n_stuck) __hip_atomic_fetch_add(&A.info[2], n_stuck, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n_dead) __hip_atomic_fetch_add(&A.info[3], n_dead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n_res) __hip_atomic_fetch_add(&A.info[4], n_res, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ------------------------------------------------------------------------------------------------

extern "C" unsigned stb_seat_filter_budget(unsigned K) { return pf_budget(K); }

int stb_seat_pf_check(double a, unsigned M, unsigned particles, double tau, int I, const char *who) {
  if (particles < 1 || particles > STB_PF_MAXR) return stb_fail("%s: particles=%u (1 to %d: a slot a lane)", who, particles, STB_PF_MAXR);
  if (stb_seat_check(a, M, particles, 0, I, who)) return 1;
  if (!(tau >= 0.0 && tau <= 1.0)) return stb_fail("%s: tau=%g outside [0, 1]", who, tau);
  return 0;
}

int stb_seat_pf_launch(const stb_rest_view &r, const stb_cnts_ro &c, unsigned M, const stb_cust_ro &cu, const stb_lik_view &L,
                       unsigned particles, double tau, const stb_draw_key &k, const stb_pf_out &out, hipStream_t st,
                       const char *who) {
  if (r.I == 0) return 0;
  if (stb_device_count() < 1) return stb_no_device(who);
  int nw = stb_env_waves("STB_SEAT_WAVES", 0);
  if (!nw) {
    // sixteen slots a wave: every wave repeats the weight step of a customer, so that step is paid once per wave and
    // customer whatever the wave seats; at R = 16 one wave beat two, four and eight (MEASUREMENTS.md section F1)
    nw = 1;
    while (nw < 8 && 16u * (unsigned)nw < particles) nw *= 2;
  }
  const seat_args A = st_args(r, c, M, cu, L, particles, k, out.info);  // (read only: the kernel stores to neither n nor t)
  pf_args P;
  P.tau = tau;
  P.Hi = out.Hi;
  P.w = out.w;
  P.E = (long long *)out.E;
  P.res = out.res;
  P.pn = out.pn;
  P.pt = out.pt;
  // the largest K_i where the caller knows it and it fits: the launch takes what that needs; else the whole budget
  size_t shm = PF_LDS_DYN;
  if (r.maxK >= 1 && particles <= pf_budget(r.maxK)) shm = (size_t)12u * particles * pf_kp(r.maxK);
  const unsigned grid = (unsigned)((uint64_t)r.I < (1ull << 20) ? (uint64_t)r.I : (1ull << 20));
  STB_LAUNCH_SHM(k_seat_pf, dim3(grid), dim3(64 * nw), shm, st, A, P);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int stb_seat_filter(double a, const double *d_bpar, int I, const uint64_t *d_koff, const uint32_t *d_n,
                               const uint16_t *d_t, const double *d_h, unsigned M, const uint64_t *d_coff, const uint32_t *d_cls,
                               const double *d_lik, unsigned rows, unsigned stride, unsigned particles, double tau, uint64_t seed,
                               uint64_t sweep, double *d_Hi, double *d_w, int64_t *d_E, uint32_t *d_res, uint32_t *d_pn,
                               uint16_t *d_pt, uint64_t *d_info, void *stream) {
  STB_ENTRY;
  const char *who = "stb_seat_filter";
  if (stb_seat_pf_check(a, M, particles, tau, I, who)) return 1;
  if (!d_koff || !d_n || !d_t || !d_coff) return stb_fail("%s: the pair offsets, n, t and the customer offsets are required", who);
  if (I > 0 && !d_bpar) return stb_fail("%s: bpar is required", who);
  if (!d_Hi) return stb_fail("%s: d_Hi is required", who);
  if (d_lik && (!d_cls || rows < 1 || stride < 1))
    return stb_fail("%s: a likelihood needs d_cls, rows >= 1 and stride >= 1 (rows=%u, stride=%u)", who, rows, stride);
  const stb_rest_view r = {a, d_bpar, I, d_koff, d_h};
  const stb_cust_ro cu = {d_coff, d_cls};
  const stb_lik_view L = {d_lik, rows, stride};
  const stb_pf_out out = {d_Hi, d_info, d_w, d_E, d_res, d_pn, d_pt};
  return stb_seat_pf_launch(r, {d_n, d_t}, M, cu, L, particles, tau, {seed, sweep}, out, (hipStream_t)stream, who);
}
