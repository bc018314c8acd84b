// seat.hip -- the Chinese-restaurant seating itself, run forwards on the device: customers are seated one after another
// in restaurants whose pairs (n, t, h) are a start state, each drawn from the state's one-step predictive under a
// likelihood, and the product of the predictives is the particle's weight (include/stb_hip.h, stb_seat_customers and
// stb_seat_loglik; an additive interface: the reference has no counterpart; the law is DESIGN.md section 6).
//
//   k_seat<true>    every K_i <= 64 (the object layer knows): a dish a lane, n, t, h in registers, no LDS
//   k_seat<false>   the form is chosen per restaurant, wave-uniformly: K_i <= 64 as above, K_i <= STB_TD_MAXK keeps n and t
//                   in the wave's 6 KB of LDS (h is read through the cache: eight waves of n, t and h would not fit the
//                   64 KB a workgroup may take)
//   k_seat_sum      k_heldout_sum's shape (predict.hip): blocks of 256 restaurants, a wave a restaurant, the block sums
//                   added by the last workgroup to finish (a ticket); geometry and ticket from ticket.h
//
// A wave is one (restaurant, particle); nobody waits for anybody and the state is touched by no atomic.  The arithmetic
// of a visit is the header's, word for word (FP64, no contraction; tests/st_oracle.py replays it): theta as k_predict,
// the cumulative sums and the choice as k_tdish (a Kogge-Stone scan inside a block of 64 dishes, block bases added in
// sequence), the head from the chosen dish's own x and y.  The LDS form keeps no cumulative sums: it takes Z in one pass
// over the blocks, remembering every block's base and positive lanes in a lane, and evaluates the blocks again up to
// the one that holds the threshold -- the same operations on the same values, so the same bits.
//
// What sets the pace: a restaurant is a serial chain of customers, each one scan (six dependent shuffle steps a block)
// and a handful of readlanes.  So the chain carries nothing it need not: a chunk's 64 classes come in one coalesced load
// with the next chunk's already on the way, the register form loads the next customer's row of L while the current one is
// decided, the uniforms are counter-based (computed, not fetched), and log p_c leaves the chain -- a lane keeps its
// customer's p, the 64 logs are taken at once at the end of the chunk and added in seating order in double-double.

#include "stb_common.h"
#include "seat.h"
#include "seat_visit.h"
#include "ticket.h"

#pragma clang fp contract(off)

#define ST_BLOCK STB_TG_BLOCK  // restaurants of a block sum in k_seat_sum
#define ST_MAXTHREADS 512
#define ST_STAGE 1024          // block sums the last workgroup stages in LDS at a time
#define ST_MAXPART 4096u
#define ST_LDS_WAVE ((size_t)STB_TD_MAXK * (sizeof(uint32_t) + sizeof(uint16_t)))

// (seat_args, theta and one visit -- steps 1 to 4 -- are seat_visit.h's, shared with seat_pf.hip; the scan is wave.h's)

// one (restaurant, particle); counters: lane-uniform counts of this wave
template <bool REG>
__device__ __forceinline__ void seat_item(const seat_args &A, uint64_t i, unsigned r, unsigned lane, uint32_t *ln, uint16_t *lt,
                                          unsigned long long &n_imp, unsigned long long &n_stuck) {
#pragma clang fp contract(off)
  const uint64_t kg = A.koff[i], c0 = A.coff[i], c1 = A.coff[i + 1], C = A.coff[A.I];
  const unsigned K = (unsigned)(A.koff[i + 1] - kg), nblk = REG ? 1u : (K + 63) / 64, M = A.M;
  const bool commit = (A.flags & STB_SEAT_COMMIT) != 0;
  const double a = A.a, b = A.bpar[i];
  const uint64_t key = stb_mix64(A.seed + (A.sweep + (uint64_t)r + 1) * STB_GAMMA);
  const double *hv = A.hv, *lik = A.lik;

  // ---- the start state: this lane's dish (register form) or the wave's LDS; T and N are the kernel's own sums
  unsigned rn = 0, rt = 0;
  double rh = 0.0;
  unsigned long long sT = 0, sN = 0;
  if (REG) {
    if (lane < K) {
      rn = A.nv[kg + lane];
      rt = A.tv[kg + lane];
      rh = hv ? hv[kg + lane] : 1.0;
    }
    sT = rt;
    sN = rn;
  } else {
    for (unsigned k = lane; k < K; k += 64) {
      const unsigned n = A.nv[kg + k], t = A.tv[kg + k];
      ln[k] = n;
      lt[k] = (uint16_t)t;
      sT += t;
      sN += n;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  unsigned long long T = __shfl(stb_wave_sum(sT), 0, 64), N = __shfl(stb_wave_sum(sN), 0, 64);

  dd_t acc{0.0, 0.0};
  bool dead = false;

  unsigned mcn = 0;  // the next chunk's classes, a lane a customer
  if (lik && c0 + lane < c1) mcn = A.cls[c0 + lane];
  double Lnext = 1.0;  // register form: the next customer's row of L, a lane a dish
  if (REG && lik && c0 < c1) {
    const unsigned cl = stb_wave_rl(mcn, 0);
    Lnext = cl < A.rows && lane < K ? lik[(uint64_t)cl * A.stride + lane] : 0.0;
  }
  for (uint64_t cb = c0; cb < c1; cb += 64) {
    const unsigned Lc = c1 - cb < 64 ? (unsigned)(c1 - cb) : 64u;
    const unsigned mc = mcn;
    mcn = 0;
    if (lik && cb + 64 + lane < c1) mcn = A.cls[cb + 64 + lane];
    unsigned mk = 0;   // this lane's customer of the chunk: its dish
    double mp = 1.0;   // and its p (1 past the chunk's end: log 1 = 0 is never added)
    for (unsigned j = 0; j < Lc; j++) {
      const uint64_t c = cb + j;
      const unsigned cl = stb_wave_rl(mc, j);
      const bool lrow = lik && cl < A.rows;
      const double Lcur = Lnext;
      if (REG && lik) {  // the next customer's row, on its way while this one is decided
        const unsigned cn = j + 1 < Lc ? stb_wave_rl(mc, j + 1) : stb_wave_rl(mcn, 0);
        const bool more = c + 1 < c1;
        Lnext = more && cn < A.rows && lane < K ? lik[(uint64_t)cn * A.stride + lane] : 0.0;
      }
      const double u2 = stb_unit(key, 2 * c + 2), u3 = stb_unit(key, 2 * C + 1 + c);
      unsigned ks;
      double pc;
      st_visit<REG>(A, kg, K, nblk, a, b, M, lane, ln, lt, rn, rt, rh, Lcur, cl, lrow, u2, u3, T, N, ks, pc, dead, n_imp, n_stuck);
      if (lane == j) mk = ks, mp = pc;
    }
    // ---- the chunk's results, coalesced; 5. the log weight, in seating order
    if (commit && lane < Lc) {
      A.cust[cb + lane] = mk;
      if (A.p) A.p[cb + lane] = mp;
    }
    const double xl = mp > 0.0 ? log(mp) : 0.0;
    for (unsigned j = 0; j < Lc; j++) dd_add(acc, stb_wave_rld(xl, j));
  }
  if (commit) {
    if (REG) {
      if (lane < K) {
        A.nv[kg + lane] = rn;
        A.tv[kg + lane] = (uint16_t)rt;
      }
    } else {
      for (unsigned k = lane; k < K; k += 64) {
        A.nv[kg + k] = ln[k];
        A.tv[kg + k] = lt[k];
      }
    }
    if (lane == 0 && A.Tv) A.Tv[i] = (uint32_t)T;
  }
  if (lane == 0) A.lw[i * A.R + r] = dead ? -HUGE_VAL : acc.hi + acc.lo;
}

// dynamic LDS (k_seat<false>): ST_LDS_WAVE bytes a wave
template <bool REG>
__global__ __launch_bounds__(ST_MAXTHREADS) void k_seat(seat_args A) {
  extern __shared__ unsigned char st_lds[];
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  uint32_t *ln = nullptr;
  uint16_t *lt = nullptr;
  if (!REG) {
    ln = (uint32_t *)(st_lds + (size_t)wave * ST_LDS_WAVE);
    lt = (uint16_t *)(ln + STB_TD_MAXK);
  }
  const uint64_t items = A.I * (uint64_t)A.R;
  unsigned long long n_skip = 0, n_imp = 0, n_stuck = 0;  // wave-uniform
  for (uint64_t w = (uint64_t)blockIdx.x * nw + wave; w < items; w += (uint64_t)gridDim.x * nw) {
    const uint64_t i = w / A.R;
    const unsigned r = (unsigned)(w % A.R);
    const uint64_t K = A.koff[i + 1] - A.koff[i];
    if (K > (REG ? 64u : (unsigned)STB_TD_MAXK) || (A.lik && K > A.stride) || (K == 0 && A.coff[i + 1] > A.coff[i])) {
      if (r == 0) n_skip++;
      if (lane == 0) A.lw[w] = 0.0;
      continue;
    }
    if (REG || K <= 64)
      seat_item<true>(A, i, r, lane, nullptr, nullptr, n_imp, n_stuck);
    else
      seat_item<false>(A, i, r, lane, ln, lt, n_imp, n_stuck);
  }
  if (lane == 0 && A.info) {
    if (n_skip) __hip_atomic_fetch_add(&A.info[0], n_skip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n_imp) __hip_atomic_fetch_add(&A.info[1], n_imp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n_stuck) __hip_atomic_fetch_add(&A.info[2], n_stuck, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ctl: [0] ticket (u32); as u64 word 1: restaurants whose H_i is -inf -- zeroed on the stream ahead of the launch.
// host: [0] total, as u64 [1] those restaurants, [2 .. 4] info_in's three words (0 without one)
__global__ __launch_bounds__(ST_MAXTHREADS) void k_seat_sum(const double *lw, uint64_t I, unsigned R, double *Hi, double *partial,
                                                            unsigned nblk, unsigned *ctl, double *host,
                                                            const unsigned long long *info_in) {
#pragma clang fp contract(off)
  __shared__ double sx[ST_BLOCK];
  __shared__ double stage[ST_STAGE];
  __shared__ unsigned s_last;
  const unsigned nthr = blockDim.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nw = nthr >> 6;
  unsigned long long c_bad = 0;  // lane 0's
  for (unsigned blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const uint64_t i0 = (uint64_t)blk * ST_BLOCK;
    // ---- the particles: a wave a restaurant
    for (unsigned q = wave; q < ST_BLOCK && i0 + q < I; q += nw) {
      const double *row = lw + (i0 + q) * R;
      double m = -HUGE_VAL;
      for (unsigned r = lane; r < R; r += 64) m = fmax(m, row[r]);
      m = stb_wave_all_max(m);
      double H = -HUGE_VAL;
      if (m > -HUGE_VAL) {
        double s = 0.0;
        for (unsigned base = 0; base < R; base += 64) {
          const unsigned cn = R - base < 64 ? R - base : 64u;
          const double e = lane < cn ? exp(row[base + lane] - m) : 0.0;
          for (unsigned j = 0; j < cn; j++) s = s + stb_wave_rld(e, j);
        }
        H = m + log(s / (double)R);
      } else if (lane == 0) {
        c_bad++;
      }
      if (lane == 0) {
        sx[q] = m > -HUGE_VAL ? H : 0.0;
        if (Hi) Hi[i0 + q] = H;
      }
    }
    __syncthreads();
    for (unsigned q = tid; q < ST_BLOCK; q += nthr)
      if (i0 + q >= I) sx[q] = 0.0;
    __syncthreads();
    // ---- the block's sum, the one fixed tree
    if (wave == 0) {
      const double v = stb_wave_sum((sx[lane] + sx[lane + 64]) + (sx[lane + 128] + sx[lane + 192]));
      if (lane == 0) partial[blk] = v;
    }
    __syncthreads();
  }
  unsigned long long *cnt = (unsigned long long *)ctl;
  if (lane == 0 && c_bad) __hip_atomic_fetch_add(&cnt[1], c_bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!stb_ticket_last(ctl, gridDim.x, &s_last)) return;  // (ticket.h: the block sums and the counter are published)
  dd_t tot{0.0, 0.0};  // thread 0's
  for (unsigned b0 = 0; b0 < nblk; b0 += ST_STAGE) {
    const unsigned bn = nblk - b0 < ST_STAGE ? nblk - b0 : ST_STAGE;
    for (unsigned e = tid; e < bn; e += nthr) stage[e] = partial[(size_t)b0 + e];
    __syncthreads();
    if (tid == 0)
      for (unsigned e = 0; e < bn; e++) dd_add(tot, stage[e]);
    __syncthreads();
  }
  if (tid == 0) {
    const unsigned long long n_bad = __hip_atomic_load(&cnt[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    host[0] = n_bad ? -HUGE_VAL : tot.hi + tot.lo;
    unsigned long long *hc = (unsigned long long *)host;
    hc[1] = n_bad;
    for (int e = 0; e < 3; e++) hc[2 + e] = info_in ? info_in[e] : 0ull;
  }
}

// ------------------------------------------------------------------------------------------------
// per calling thread: the block sums, the ticket and counter, and the pinned words k_seat_sum answers in.  A call waits
// for its answer before it returns, so one set per thread is never in use twice.

static thread_local stb_tset sq;

extern "C" void stb_seat_release(void) {
  STB_ENTRY;
  stb_tset_drop(sq);
}

int stb_seat_check(double a, unsigned M, unsigned particles, unsigned flags, int I, const char *who) {
  if (!(a >= 0.0 && a < 1.0)) return stb_fail("%s: discount a=%g outside [0, 1)", who, a);
  if (flags & ~STB_SEAT_COMMIT) return stb_fail("%s: unknown flags 0x%x", who, flags);
  if (I < 0) return stb_fail("%s: I=%d", who, I);
  if (M > 65535u) return stb_fail("%s: M=%u (t is a uint16: at most 65535)", who, M);
  if (particles < 1 || particles > ST_MAXPART) return stb_fail("%s: particles=%u (1 to %u)", who, particles, ST_MAXPART);
  if ((flags & STB_SEAT_COMMIT) && particles != 1)
    return stb_fail("%s: STB_SEAT_COMMIT with particles=%u (a committed seating is one particle)", who, particles);
  return 0;
}

int stb_seat_launch(const stb_rest_view &r, const stb_cnts_rw &c, unsigned M, const stb_cust_rw &cu, const stb_lik_view &L,
                    unsigned particles, unsigned flags, const stb_draw_key &k, const stb_seat_out &out, hipStream_t st,
                    const char *who) {
  if (r.I == 0) return 0;
  if (stb_device_count() < 1) return stb_no_device(who);
  const int nw = stb_env_waves("STB_SEAT_WAVES", 4);
  const bool commit = (flags & STB_SEAT_COMMIT) != 0;
  seat_args A = st_args(r, c, M, cu, L, particles, k, out.info);
  A.Tv = commit ? c.T : nullptr;
  A.cust = cu.cust;
  A.lw = out.lw;
  A.p = commit ? out.p : nullptr;
  A.flags = flags;
  const uint64_t items = (uint64_t)r.I * particles, groups = (items + nw - 1) / nw;
  const unsigned grid = (unsigned)(groups < (1ull << 20) ? groups : (1ull << 20));
  if (r.maxK >= 1 && r.maxK <= 64) {
    STB_LAUNCH(k_seat<true>, dim3(grid), dim3(64 * nw), st, A);
  } else {
    STB_LAUNCH_SHM(k_seat<false>, dim3(grid), dim3(64 * nw), ST_LDS_WAVE * nw, st, A);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int stb_seat_sum(const double *d_lw, int I, unsigned particles, double *d_Hi, double *Hi_host, double *total_host,
                 stb_seat_info_t *info, const uint64_t *d_info, hipStream_t st, const char *who) {
  if (info) info->skipped = info->impossible = info->stuck = 0;
  if (I == 0) {
    if (total_host) *total_host = 0.0;
    return 0;
  }
  if (stb_device_count() < 1) return stb_no_device(who);
  stb_tgeom tg;  // k_logjoint's geometry; the workgroup size from STB_SEAT_WAVES where it is set
  if (stb_ticket_geom(STB_GEOM_LOGJOINT, (uint64_t)I, 0, 0, stb_env_waves("STB_SEAT_WAVES", 0), &tg))
    return stb_fail("%s: no launch geometry for I=%d", who, I);
  if (stb_tset_ready(sq, who) || stb_tset_room(sq, tg.need, STB_TG_CAP0_BLOCKS, sizeof(double), who)) return 1;
  HIPCHK(hipMemsetAsync(sq.d_ctl, 0, 64, st));
  STB_LAUNCH(k_seat_sum, dim3(tg.gx), dim3(64 * tg.waves), st, d_lw, (uint64_t)I, particles, d_Hi, (double *)sq.d_buf, tg.nblk,
             sq.d_ctl, sq.h_out_dev, (const unsigned long long *)d_info);
  HIPCHK(hipGetLastError());
  if (d_Hi && Hi_host) HIPCHK(hipMemcpyAsync(Hi_host, d_Hi, sizeof(double) * (size_t)I, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const volatile double *h = (const volatile double *)sq.h_out;
  const volatile uint64_t *hc = (const volatile uint64_t *)sq.h_out;
  if (total_host) *total_host = h[0];
  if (info) {
    info->skipped = d_info ? hc[2] : 0;
    info->impossible = d_info ? hc[3] : hc[1];
    info->stuck = d_info ? hc[4] : 0;
  }
  return 0;
}

extern "C" int stb_seat_customers(double a, const double *d_bpar, int I, const uint64_t *d_koff, uint32_t *d_n, uint16_t *d_t,
                                  uint32_t *d_T, const double *d_h, unsigned M, const uint64_t *d_coff, const uint32_t *d_cls,
                                  uint32_t *d_cust, const double *d_lik, unsigned rows, unsigned stride, unsigned particles,
                                  unsigned flags, uint64_t seed, uint64_t sweep, double *d_lw, double *d_p, uint64_t *d_info,
                                  void *stream) {
  STB_ENTRY;
  const char *who = "stb_seat_customers";
  if (stb_seat_check(a, M, particles, flags, I, who)) return 1;
  if (!d_koff || !d_n || !d_t || !d_coff) return stb_fail("%s: the pair offsets, n, t and the customer offsets are required", who);
  if (I > 0 && !d_bpar) return stb_fail("%s: bpar is required", who);
  if (!d_lw) return stb_fail("%s: d_lw is required", who);
  if (d_lik && (!d_cls || rows < 1 || stride < 1))
    return stb_fail("%s: a likelihood needs d_cls, rows >= 1 and stride >= 1 (rows=%u, stride=%u)", who, rows, stride);
  if ((flags & STB_SEAT_COMMIT) && (!d_T || !d_cust)) return stb_fail("%s: STB_SEAT_COMMIT writes d_T and d_cust (both are required)", who);
  const stb_rest_view r = {a, d_bpar, I, d_koff, d_h};
  const stb_cnts_rw c = {d_n, d_t, d_T};
  const stb_cust_rw cu = {d_coff, d_cls, d_cust};
  const stb_lik_view L = {d_lik, rows, stride};
  return stb_seat_launch(r, c, M, cu, L, particles, flags, {seed, sweep}, {d_lw, d_p, d_info}, (hipStream_t)stream, who);
}

extern "C" int stb_seat_loglik(const double *d_lw, int I, unsigned particles, double *d_Hi, double *total_host,
                               stb_seat_info_t *info, void *stream) {
  STB_ENTRY;
  const char *who = "stb_seat_loglik";
  if (I < 0) return stb_fail("%s: I=%d", who, I);
  if (particles < 1 || particles > ST_MAXPART) return stb_fail("%s: particles=%u (1 to %u)", who, particles, ST_MAXPART);
  if (!total_host) return stb_fail("%s: total_host is required", who);
  if (I > 0 && !d_lw) return stb_fail("%s: d_lw is required", who);
  if (info) info->customers = 0;
  return stb_seat_sum(d_lw, I, particles, d_Hi, nullptr, total_host, info, nullptr, (hipStream_t)stream, who);
}
