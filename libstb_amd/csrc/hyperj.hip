// hyperj.hip -- the joint step for the discount a and the concentration b on the device (DESIGN.md section 6,
// deviation 14: an additive algorithm, not the reference's).  All restaurants share one a and one b; with beta = log b
//     L(a, beta) = W(a) + R(a, b) + ((shape - 1) beta - b / scale) + beta
//     W(a)    = sum over pairs with n > 1 of S_S_a(n, t)                       (stb_groups_ssum, groups.hip)
//     R(a, b) = sum_i [ T_i log a + lgamma(T_i + b/a) - lgamma(b/a) - lgamma(b + N_i) + lgamma(b) ]
//
//   k_joint_terms   R[d][j] over a D x J grid (D, J <= 64) from device-resident T[I] and N[I]
//   k_joint_draw    one workgroup: L = (W[d] + R[d][j]) + P[j], the stage's maximum, floored weights, their total, the
//                   box, the cell picked for u1 and the weight of one queried cell, written to pinned host memory
//   k_joint_final   the weights of the proposed point's cells in every stage, and the four sums of the two points
//
// k_joint_terms, the association (no contraction anywhere).  With T = (double)T_i, N = (double)N_i, c = b_j / a_d,
// la_d = log a_d (host libm, one per abscissa, as stb_restaurant_terms does):
//     lgc_dj = lgamma(c)                 once per (d, j) and workgroup
//     lgb_j  = lgamma(b_j)               once per j and workgroup
//     gN_ij  = lgamma(b_j + N) - lgb_j   once per restaurant and j, reused over d
//     term   = (T la_d + (lgamma(T + c) - lgc_dj)) - gN_ij         (0 for a restaurant with N_i = 0)
// (a restaurant with T_i = 0 gets lgamma(c) - lgc_dj = 0 exactly: the same call on the same argument.)
// Restaurants 256 k .. 256 k + 255 (terms 0 beyond I) are block k; its terms for one cell are summed in one fixed tree:
// (p[l] + p[l + 64]) + (p[l + 128] + p[l + 192]) per lane l, then the shuffle tree of a 64-lane wave (offsets 32, 16,
// ... 1).  The block sums go to partial[k][d J + j]; the last workgroup to finish -- a ticket, nobody waits -- adds, one
// lane per cell, the blocks k = 0, 1, 2, ... in double-double, and writes hi + lo.  So the bits of R depend on neither the
// grid nor the workgroup size: STB_HYPERJ_WAVES = 1, 2, 4 or 8 waves a workgroup (default 4) give the same bits.
//
// What a lane carries: HJ_CT = 4 cells (d0 .. d0 + 3, j) of its restaurant at a time -- four independent lgamma chains,
// which is what hides the latency of the FP64 pipe at two or three waves a SIMD -- written to LDS (4 x 512 doubles) and
// summed there by the waves, one (cell, block) each.  More cells a lane add registers (an lgamma evaluation holds about
// 30 live doubles) without adding anything the four chains do not already give; fewer leave a barrier per lgamma.
// Workgroups split the work by block of restaurants (x) and by j (y): a set of 1000 restaurants still fills the chip.

#include "groups.h"
#include "tcounts.h"
#include "hyperj.h"
#include "ticket.h"
#include "../../include/psample.h"

#include <vector>

#define HJ_CHUNK STB_TG_BLOCK  // (one constant for the kernel, the launch and stb_reduce_geometry)
#define HJ_CT 4
#define HJ_MAXTHREADS 512
#define HJ_DMAX 64
#define HJ_CELLS (HJ_DMAX * HJ_DMAX)
#define HJ_STAGES 5
#define HJ_HOST_STRIDE (16 + HJ_CELLS)  // doubles of pinned memory a stage answers in

struct hj_args {
  double a[HJ_DMAX], la[HJ_DMAX], b[HJ_DMAX];
  int D, J;
};

template <int RPT>
__global__ __launch_bounds__(HJ_MAXTHREADS) void k_joint_terms(hj_args A, uint64_t I, const uint32_t *T, const uint32_t *Nv,
                                                               const uint64_t *coff, double *partial, unsigned nchunks,
                                                               unsigned *ctl, double *out) {
#pragma clang fp contract(off)
  __shared__ double sL[HJ_CT][HJ_MAXTHREADS];
  __shared__ double s_lgc[HJ_DMAX];
  __shared__ double s_lgb;
  __shared__ unsigned s_last;
  const unsigned nthr = blockDim.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nw = nthr >> 6;
  const unsigned span = nthr * RPT;       // restaurants a workgroup takes per step: 256, or 512 with eight waves
  const unsigned cps = stb_tg_cps(nthr);  // ... which are this many blocks of 256 (the launch pairs RPT with nthr so)
  const unsigned nsteps = (nchunks + cps - 1) / cps;
  const int D = A.D, J = A.J, DJ = D * J;
  for (unsigned s = blockIdx.x; s < nsteps; s += gridDim.x) {
    double Tr[RPT], Nr[RPT];
#pragma unroll
    for (int r = 0; r < RPT; r++) {
      const uint64_t i = (uint64_t)s * span + tid + (unsigned)r * nthr;
      Tr[r] = 0.0;
      Nr[r] = 0.0;
      if (i < I) {
        const uint64_t Ni = Nv ? (uint64_t)Nv[i] : coff[i + 1] - coff[i];
        Nr[r] = (double)Ni;
        if (Ni > 0) Tr[r] = (double)T[i];
      }
    }
    for (int j = blockIdx.y; j < J; j += gridDim.y) {
      const double bj = A.b[j];
      __syncthreads();  // (the readers of the last j's s_lgc are through)
      if ((int)tid < D) s_lgc[tid] = lgamma(bj / A.a[tid]);
      if (tid == 0) s_lgb = lgamma(bj);
      __syncthreads();
      const double lgb = s_lgb;
      double gN[RPT];
#pragma unroll
      for (int r = 0; r < RPT; r++) gN[r] = Nr[r] > 0.0 ? lgamma(bj + Nr[r]) - lgb : 0.0;
      for (int d0 = 0; d0 < D; d0 += HJ_CT) {
#pragma unroll
        for (int ct = 0; ct < HJ_CT; ct++) {
          const int d = d0 + ct;
          if (d < D) {
            const double c = bj / A.a[d], la = A.la[d], lgc = s_lgc[d];
#pragma unroll
            for (int r = 0; r < RPT; r++)
              sL[ct][tid + (unsigned)r * nthr] = Nr[r] > 0.0 ? (Tr[r] * la + (lgamma(Tr[r] + c) - lgc)) - gN[r] : 0.0;
          }
        }
        __syncthreads();
        for (unsigned q = wave; q < HJ_CT * cps; q += nw) {
          const int d = d0 + (int)(q / cps);
          const unsigned w = q % cps, chunk = s * cps + w;
          if (d < D && chunk < nchunks) {
            const double *p = sL[q / cps] + w * HJ_CHUNK;
            double v = (p[lane] + p[lane + 64]) + (p[lane + 128] + p[lane + 192]);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane == 0) partial[(size_t)chunk * DJ + d * J + j] = v;
          }
        }
        __syncthreads();
      }
    }
  }
  if (!stb_ticket_last(ctl, gridDim.x * gridDim.y, &s_last)) return;  // (ticket.h)
  for (int cell = tid; cell < DJ; cell += nthr) {
    dd_t acc{0.0, 0.0};
    for (unsigned c = 0; c < nchunks; c++) dd_add(acc, partial[(size_t)c * DJ + cell]);
    out[cell] = acc.hi + acc.lo;
  }
}

// ------------------------------------------------------------------------------------------------
// one stage of the draw.  host[0] max, [1] Z, [2] the cell picked (d J + j), [3] / [4] the cumulative weight before /
// with it, [5..8] the box (d lo, d hi, j lo, j hi: cells, inclusive), [9] the weight of cell q0 (q0 < 0: none),
// [11] error word (1: a NaN or +inf among the L, or no finite L at all), [16 ..) the L when asked
struct hj_draw_args {
  double P[HJ_DMAX];  // ((shape - 1) beta_j - b_j / scale) + beta_j
  double u1;
  int D, J, q0, want_L;
};

__global__ __launch_bounds__(256) void k_joint_draw(hj_draw_args A, const double *W, const double *R, double *Lout, double *host) {
#pragma clang fp contract(off)
  __shared__ double sw[HJ_CELLS];
  __shared__ double red[256];
  __shared__ int s_box[4], s_bad, s_pick;
  __shared__ double s_Z;
  const int tid = threadIdx.x, D = A.D, J = A.J, DJ = D * J;
  if (tid == 0) {
    s_box[0] = D;
    s_box[1] = -1;
    s_box[2] = J;
    s_box[3] = -1;
    s_bad = 0;
    s_pick = DJ;
  }
  __syncthreads();
  double mx = -HUGE_VAL;
  bool bad = false;
  for (int k = tid; k < DJ; k += 256) {
    const double L = (W[k / J] + R[k]) + A.P[k % J];
    sw[k] = L;
    Lout[k] = L;
    if (A.want_L) host[16 + k] = L;
    if (L != L || L == HUGE_VAL) bad = true;
    mx = fmax(mx, L);
  }
  if (bad) atomicOr(&s_bad, 1);
  red[tid] = mx;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if (tid < off) red[tid] = fmax(red[tid], red[tid + off]);
    __syncthreads();
  }
  mx = red[0];
  __syncthreads();
  if (s_bad || mx == -HUGE_VAL) {
    if (tid == 0) host[11] = 1.0;
    return;
  }
  // floored weights and the box; thread t owns the cells [t per, (t + 1) per) of the d-major order
  const int per = (DJ + 255) / 256, k0 = tid * per, k1 = k0 + per < DJ ? k0 + per : DJ;
  double seg = 0.0;
  for (int k = k0; k < k1; k++) {
    const double L = sw[k];
    if (L >= mx - 40.0) {
      atomicMin(&s_box[0], k / J);
      atomicMax(&s_box[1], k / J);
      atomicMin(&s_box[2], k % J);
      atomicMax(&s_box[3], k % J);
    }
    const double w = exp(fmax(L - mx, -60.0));
    sw[k] = w;
    seg += w;
  }
  red[tid] = seg;
  __syncthreads();
  if (tid == 0) {  // (256 additions in thread order: the cumulative weight of a cell is one fixed sequence)
    double run = 0.0;
    for (int t = 0; t < 256; t++) {
      const double v = red[t];
      red[t] = run;
      run += v;
    }
    s_Z = run;
  }
  __syncthreads();
  const double Z = s_Z, target = A.u1 * Z;
  {
    double run = red[tid];
    for (int k = k0; k < k1; k++) {
      run += sw[k];
      if (run > target) {
        atomicMin(&s_pick, k);
        break;
      }
    }
  }
  __syncthreads();
  const int pick = s_pick < DJ ? s_pick : DJ - 1;
  if (pick >= k0 && pick < k1) {
    double run = red[tid];
    for (int k = k0; k < pick; k++) run += sw[k];
    host[3] = run;
    host[4] = run + sw[pick];
  }
  if (tid == 0) {
    int b0 = s_box[0] - 1, b1 = s_box[1] + 1, b2 = s_box[2] - 1, b3 = s_box[3] + 1;  // padded by one cell, clipped
    host[0] = mx;
    host[1] = Z;
    host[2] = (double)pick;
    host[5] = (double)(b0 < 0 ? 0 : b0);
    host[6] = (double)(b1 > D - 1 ? D - 1 : b1);
    host[7] = (double)(b2 < 0 ? 0 : b2);
    host[8] = (double)(b3 > J - 1 ? J - 1 : b3);
    host[9] = A.q0 >= 0 ? sw[A.q0] : 0.0;
    host[11] = 0.0;
  }
}

// after the last stage: host[s] = the weight of the proposed point's cell in stage s (0 where it lies outside the stage's
// rectangle), host[8..11] = W(a_cur), W(a'), R(x_cur), R(x')
struct hj_final_args {
  double mx[HJ_STAGES];
  int cell[HJ_STAGES];
  int S;
};

__global__ __launch_bounds__(64) void k_joint_final(hj_final_args A, const double *Lall, const double *Wcur, const double *pt, double *host) {
#pragma clang fp contract(off)
  const int s = threadIdx.x;
  if (s < A.S) host[s] = A.cell[s] >= 0 ? exp(fmax(Lall[(size_t)s * HJ_CELLS + A.cell[s]] - A.mx[s], -60.0)) : 0.0;
  if (s == 0) {
    host[8] = Wcur[0];
    host[9] = pt[1];
    host[10] = pt[2];
    host[11] = pt[3];
  }
}

// ------------------------------------------------------------------------------------------------
// per calling thread: block sums, ticket, the stage buffers and the pinned words the kernels answer in.  A step waits
// for its answers before it returns, so one set per thread is never in use twice.

struct hj_ctx {
  stb_tset set;             // d_buf: doubles of block sums; its pinned words are not used (the stages have their own)
  double *d_buf = nullptr;  // [HJ_STAGES][HJ_CELLS] L, then R [HJ_CELLS], W [HJ_DMAX], pt [4]
  double *h_out = nullptr, *h_out_dev = nullptr;  // [HJ_STAGES + 1][HJ_HOST_STRIDE]
  std::vector<double> keepL;
};
static thread_local hj_ctx hj;

static void hj_drop() {
  if (hj.set.dev < 0) return;
  stb_device_scope dev(hj.set.dev);
  if (hj.d_buf) stb_pool_free(hj.d_buf);
  if (hj.h_out) stb_pool_free(hj.h_out);
  hj.d_buf = nullptr;
  hj.h_out = hj.h_out_dev = nullptr;
  stb_tset_drop(hj.set);
}

extern "C" void stb_hj_release(void) {
  STB_ENTRY;
  hj_drop();
}

static int hj_ready(size_t partials, bool stages) {
  int dev = -1;
  HIPCHK(hipGetDevice(&dev));
  if (hj.set.dev >= 0 && hj.set.dev != dev) hj_drop();  // (the stage buffers go with the set)
  if (stb_tset_ready(hj.set, "stb_joint_terms", false)) return 1;
  if (stages && !hj.d_buf) {
    if (stb_pool_malloc((void **)&hj.d_buf, sizeof(double) * ((HJ_STAGES + 1) * HJ_CELLS + HJ_DMAX + 8)) != hipSuccess ||
        stb_pool_malloc((void **)&hj.h_out, sizeof(double) * (HJ_STAGES + 1) * HJ_HOST_STRIDE, 1) != hipSuccess ||
        hipHostGetDevicePointer((void **)&hj.h_out_dev, hj.h_out, 0) != hipSuccess) {
      hj_drop();
      return stb_fail("stb_groups_samplejoint: out of memory for the stage buffers");
    }
  }
  // (a launch queued earlier may still write the old buffer, and the cache may hand it to another thread at once)
  if (partials > hj.set.cap && hj.set.d_buf) HIPCHK(hipDeviceSynchronize());
  return stb_tset_room(hj.set, partials, STB_TG_CAP0_HJ, sizeof(double), "stb_joint_terms");
}

// R over the grid, queued on st; N given either way (d_N uint32, or d_coff uint64 prefix sums)
static int hj_terms(const double *a, int D, const double *b, int J, const uint32_t *d_T, const uint32_t *d_N, const uint64_t *d_coff,
                    uint64_t I, double *d_out, hipStream_t st, const char *who) {
  if (D < 1 || J < 1 || D > HJ_DMAX || J > HJ_DMAX) return stb_fail("%s: a grid of %d x %d (1..%d each way)", who, D, J, HJ_DMAX);
  if (!a || !b || !d_out) return stb_fail("%s: null argument", who);
  if (I > 0 && (!d_T || (!d_N == !d_coff))) return stb_fail("%s: T and the customers per restaurant are required", who);
  hj_args A;
  memset(&A, 0, sizeof(A));
  A.D = D;
  A.J = J;
  for (int d = 0; d < D; d++) {
    if (!(a[d] > 0.0 && a[d] < 1.0)) return stb_fail("%s: a=%g outside (0, 1)", who, a[d]);
    A.a[d] = a[d];
    A.la[d] = log(a[d]);  // host libm: one scalar per abscissa, as stb_restaurant_terms
  }
  for (int j = 0; j < J; j++) {
    if (!(b[j] > 0.0) || !std::isfinite(b[j])) return stb_fail("%s: b=%g (must be > 0, finite)", who, b[j]);
    A.b[j] = b[j];
  }
  if (I == 0) {
    HIPCHK(hipMemsetAsync(d_out, 0, sizeof(double) * D * J, st));
    return 0;
  }
  if (stb_device_count() < 1) return stb_no_device(who);
  const uint64_t nch64 = (I + HJ_CHUNK - 1) / HJ_CHUNK;
  if (nch64 * (uint64_t)(D * J) > (1ull << 28)) return stb_fail("%s: %llu restaurants x %d cells: more block sums than 2 GB hold", who, (unsigned long long)I, D * J);
  stb_tgeom tg;
  if (stb_ticket_geom(STB_GEOM_JOINT_TERMS, I, D, J, 0, &tg)) return stb_fail("%s: no launch geometry for I=%llu", who, (unsigned long long)I);
  if (hj_ready(tg.need, false)) return 1;
  const unsigned nchunks = tg.nblk, gx = tg.gx, gy = tg.gy;
  const int nw = (int)tg.waves, nthr = 64 * nw;
  HIPCHK(hipMemsetAsync(hj.set.d_ctl, 0, sizeof(unsigned), st));
  if (nw == 1)
    STB_LAUNCH(k_joint_terms<4>, dim3(gx, gy), dim3(nthr), st, A, I, d_T, d_N, d_coff, (double *)hj.set.d_buf, nchunks, hj.set.d_ctl, d_out);
  else if (nw == 2)
    STB_LAUNCH(k_joint_terms<2>, dim3(gx, gy), dim3(nthr), st, A, I, d_T, d_N, d_coff, (double *)hj.set.d_buf, nchunks, hj.set.d_ctl, d_out);
  else
    STB_LAUNCH(k_joint_terms<1>, dim3(gx, gy), dim3(nthr), st, A, I, d_T, d_N, d_coff, (double *)hj.set.d_buf, nchunks, hj.set.d_ctl, d_out);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int stb_joint_terms(const double *a_host, int D, const double *b_host, int J, const uint32_t *d_T, const uint32_t *d_N,
                               uint64_t I, double *d_out, void *stream) {
  STB_ENTRY;
  return hj_terms(a_host, D, b_host, J, d_T, d_N, nullptr, I, d_out, (hipStream_t)stream, "stb_joint_terms");
}

// stb_joint_terms with the customers per restaurant given either way (hyperj.h)
extern "C" int stb_hj_joint_terms(const double *a_host, int D, const double *b_host, int J, const uint32_t *d_T, const uint32_t *d_N,
                                  const uint64_t *d_coff, uint64_t I, double *d_out, void *stream) {
  STB_ENTRY;
  return hj_terms(a_host, D, b_host, J, d_T, d_N, d_coff, I, d_out, (hipStream_t)stream, "stb_joint_terms");
}

// ------------------------------------------------------------------------------------------------
// the step (the law: DESIGN.md section 6, deviation 14; tests/hj_oracle.py replays it)

struct hj_stage {
  double alo, ahi, blo, bhi, da, db;  // the stage's rectangle in (a, beta) and its cell sizes
  double mx, Z, wcur;
  int qcur, cell, box[4];
};

// the cell of x in a stage (d J + j), or -1 outside its rectangle
static int hj_cell_of(const hj_stage &s, int D, int J, double a, double beta) {
#pragma clang fp contract(off)
  if (!(a >= s.alo && a <= s.ahi && beta >= s.blo && beta <= s.bhi)) return -1;
  int d = (int)floor((a - s.alo) / s.da), j = (int)floor((beta - s.blo) / s.db);
  if (d > D - 1) d = D - 1;
  if (j > J - 1) j = J - 1;
  if (d < 0) d = 0;
  if (j < 0) j = 0;
  return d * J + j;
}

static double hj_prior(double shape, double scale, double beta, double b) {
#pragma clang fp contract(off)
  return ((shape - 1.0) * beta - b / scale) + beta;
}

extern "C" int stb_hj_samplejoint(stb_groups_t *g, const uint32_t *d_N, const uint64_t *d_coff, const stb_joint_opts_t *o, double a_in,
                                  double b_in, double *a_out, double *b_out, stb_joint_info_t *info, const char *who) {
#pragma clang fp contract(off)
  STB_ENTRY;
  if (!g) return stb_fail("%s: null group set", who);
  if (!o || !a_out || !b_out) return stb_fail("%s: null argument", who);
  if (!(o->a_lo >= A_MIN && o->a_lo < o->a_hi && o->a_hi <= A_MAX && o->b_lo >= B_MIN && o->b_lo < o->b_hi && o->b_hi <= B_MAX))
    return stb_fail("%s: the rectangle [%g, %g] x [%g, %g] must satisfy %g <= a_lo < a_hi <= %g and %g <= b_lo < b_hi <= %g", who, o->a_lo,
                    o->a_hi, o->b_lo, o->b_hi, (double)A_MIN, (double)A_MAX, (double)B_MIN, (double)B_MAX);
  const int D = o->D ? o->D : 24, J = o->J ? o->J : 24;
  if (D < 1 || D > HJ_DMAX - 1 || J < 1 || J > HJ_DMAX) return stb_fail("%s: a grid of %d x %d (D 1..%d, J 1..%d)", who, D, J, HJ_DMAX - 1, HJ_DMAX);
  if (!(o->scale > 0.0) || !std::isfinite(o->scale) || !std::isfinite(o->shape)) return stb_fail("%s: shape=%g, scale=%g (finite, scale > 0)", who, o->shape, o->scale);
  if (!(a_in >= o->a_lo && a_in <= o->a_hi && b_in >= o->b_lo && b_in <= o->b_hi))
    return stb_fail("%s: the state (a=%g, b=%g) lies outside the rectangle [%g, %g] x [%g, %g]", who, a_in, b_in, o->a_lo, o->a_hi, o->b_lo, o->b_hi);
  if (g->Dmax < D + 1) return stb_fail("%s: the set takes Dmax=%d discounts; a grid of %d needs Dmax >= %d", who, g->Dmax, D, D + 1);
  if (g->I > 0 && (!d_N == !d_coff)) return stb_fail("%s: the customers per restaurant are required", who);
  // (the step does not read bpar -- b is the argument; the host's copy of what the set's concentrations were last set to
  // only has to agree with the model of one shared b.  Never set -- all NaN since create -- agrees.)
  for (int i = 1; i < g->I; i++) {
    const double x = g->h_bpar[i], y = g->h_bpar[0];
    if (!(x == y) && !(x != x && y != y))
      return stb_fail("%s: the set's bpar are not all equal (bpar[%d]=%g, bpar[0]=%g): one shared concentration only", who, i, x, y);
  }
  stb_device_scope dev(g->dev);  // (to the end of the call: what follows the last wait is host arithmetic)
  // (the block sums of the largest grid of this step, before anything is queued: the 1 x 1 calls then never replace them)
  int rc = hj_ready((size_t)(((uint64_t)(g->I > 0 ? g->I : 0) + HJ_CHUNK - 1) / HJ_CHUNK) * D * J, true);
  hipStream_t st = g->st;
  double *d_L = hj.d_buf, *d_R = d_L + HJ_STAGES * HJ_CELLS, *d_W = d_R + HJ_CELLS, *d_pt = d_W + HJ_DMAX;
  const uint64_t key = stb_mix64(o->seed + (o->sweep + 1) * STB_GAMMA);
  double u[6];
  for (int k = 1; k <= 5; k++)  // element k of the sweep's stream (libstb_amd/synth.py: unit(., key)[k])
    u[k] = stb_unit(key, (uint64_t)k + 1);
  const double beta_in = log(b_in);
  hj_stage S[HJ_STAGES];
  int nst = 0;
  const bool keep = (o->flags & STB_JOINT_KEEP_L) != 0;
  if (keep) hj.keepL.assign((size_t)HJ_STAGES * D * J, 0.0);
  // R at the current point: a 1 x 1 call, queued ahead of the stages
  if (!rc) rc = hj_terms(&a_in, 1, &b_in, 1, g->d_T, d_N, d_coff, (uint64_t)g->I, d_pt + 2, st, who);
  double ralo = o->a_lo, rahi = o->a_hi, rblo = log(o->b_lo), rbhi = log(o->b_hi);
  int evals = 0;
  for (int s = 0; s < HJ_STAGES && !rc; s++) {
    hj_stage &Q = S[s];
    Q.alo = ralo;
    Q.ahi = rahi;
    Q.blo = rblo;
    Q.bhi = rbhi;
    Q.da = (rahi - ralo) / (double)D;
    Q.db = (rbhi - rblo) / (double)J;
    double x[HJ_DMAX], bm[HJ_DMAX];
    hj_draw_args A;
    memset(&A, 0, sizeof(A));
    for (int d = 0; d < D; d++) x[d] = Q.alo + ((double)d + 0.5) * Q.da;
    x[D] = a_in;  // W(a_cur) rides along
    for (int j = 0; j < J; j++) {
      const double beta = Q.blo + ((double)j + 0.5) * Q.db;
      bm[j] = exp(beta);
      A.P[j] = hj_prior(o->shape, o->scale, beta, bm[j]);
    }
    A.D = D;
    A.J = J;
    A.u1 = u[1];
    A.q0 = Q.qcur = hj_cell_of(Q, D, J, a_in, beta_in);
    A.want_L = keep ? 1 : 0;
    double *host = hj.h_out + (size_t)s * HJ_HOST_STRIDE, *host_dev = hj.h_out_dev + (size_t)s * HJ_HOST_STRIDE;
    rc = stb_groups_ssum_device(g, x, D + 1, d_W, st);
    if (rc) break;
    evals++;
    rc = hj_terms(x, D, bm, J, g->d_T, d_N, d_coff, (uint64_t)g->I, d_R, st, who);
    if (!rc) {
      STB_LAUNCH(k_joint_draw, dim3(1), dim3(256), st, A, d_W, d_R, d_L + (size_t)s * HJ_CELLS, host_dev);
      if (hipGetLastError() != hipSuccess) rc = stb_fail("%s: launch failed", who);
    }
    const unsigned fb = stb_groups_fallbacks();
    if (stb_groups_wait(g)) rc = 1;  // (always: what was queued is waited for)
    if (!rc && stb_groups_fallbacks() != fb) {  // the walk was redone through stored tables and W rewritten: the stage's draw again
      STB_LAUNCH(k_joint_draw, dim3(1), dim3(256), st, A, d_W, d_R, d_L + (size_t)s * HJ_CELLS, host_dev);
      if (hipGetLastError() != hipSuccess) rc = stb_fail("%s: launch failed", who);
    }
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = stb_fail("%s: %s", who, hipGetErrorString(hipGetLastError()));
    if (rc) break;
    const volatile double *h = host;
    if (h[11] != 0.0) {
      rc = stb_fail("%s: non-finite log-posterior on the grid of stage %d", who, s + 1);
      break;
    }
    Q.mx = h[0];
    Q.Z = h[1];
    Q.cell = (int)h[2];
    for (int k = 0; k < 4; k++) Q.box[k] = (int)h[5 + k];
    Q.wcur = h[9];
    if (keep)
      for (int k = 0; k < D * J; k++) hj.keepL[(size_t)s * D * J + k] = h[16 + k];
    nst = s + 1;
    const int nd = Q.box[1] - Q.box[0] + 1, nj = Q.box[3] - Q.box[2] + 1;
    if (!((2 * nd <= D || 2 * nj <= J) && s + 1 < HJ_STAGES)) break;
    // the box is the next stage's rectangle (an edge on the stage's own edge keeps its bits)
    ralo = Q.alo + (double)Q.box[0] * Q.da;
    rahi = Q.box[1] == D - 1 ? Q.ahi : Q.alo + (double)(Q.box[1] + 1) * Q.da;
    rblo = Q.blo + (double)Q.box[2] * Q.db;
    rbhi = Q.box[3] == J - 1 ? Q.bhi : Q.blo + (double)(Q.box[3] + 1) * Q.db;
  }
  double a_new = a_in, b_new = b_in, beta_new = beta_in, log_alpha = 0.0, L_cur = 0.0, L_new = 0.0;
  int pick = 0, accepted = 0;
  if (!rc) {
    // the stage from u5: eps = 1/64 for every stage but the last, which takes the rest
    double cum = 0.0;
    pick = nst - 1;
    for (int s = 0; s < nst - 1; s++) {
      cum += 1.0 / 64.0;
      if (u[5] < cum) {
        pick = s;
        break;
      }
    }
    const hj_stage &Q = S[pick];
    const int d = Q.cell / J, j = Q.cell % J;
    a_new = Q.alo + ((double)d + u[2]) * Q.da;
    beta_new = Q.blo + ((double)j + u[3]) * Q.db;
    if (a_new > Q.ahi) a_new = Q.ahi;
    if (beta_new > Q.bhi) beta_new = Q.bhi;
    b_new = exp(beta_new);
    hj_final_args F;
    memset(&F, 0, sizeof(F));
    F.S = nst;
    for (int s = 0; s < nst; s++) {
      F.mx[s] = S[s].mx;
      F.cell[s] = hj_cell_of(S[s], D, J, a_new, beta_new);
    }
    double *host = hj.h_out + (size_t)HJ_STAGES * HJ_HOST_STRIDE, *host_dev = hj.h_out_dev + (size_t)HJ_STAGES * HJ_HOST_STRIDE;
    rc = stb_groups_ssum_device(g, &a_new, 1, d_pt + 1, st);
    if (!rc) {
      evals++;
      rc = hj_terms(&a_new, 1, &b_new, 1, g->d_T, d_N, d_coff, (uint64_t)g->I, d_pt + 3, st, who);
      if (!rc) {
        STB_LAUNCH(k_joint_final, dim3(1), dim3(64), st, F, d_L, d_W + D, d_pt, host_dev);
        if (hipGetLastError() != hipSuccess) rc = stb_fail("%s: launch failed", who);
      }
      const unsigned fb = stb_groups_fallbacks();
      if (stb_groups_wait(g)) rc = 1;
      if (!rc && stb_groups_fallbacks() != fb) {
        STB_LAUNCH(k_joint_final, dim3(1), dim3(64), st, F, d_L, d_W + D, d_pt, host_dev);
        if (hipGetLastError() != hipSuccess) rc = stb_fail("%s: launch failed", who);
      }
      if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = stb_fail("%s: %s", who, hipGetErrorString(hipGetLastError()));
    }
    if (!rc) {
      const volatile double *h = host;
      L_cur = (h[8] + h[10]) + hj_prior(o->shape, o->scale, beta_in, b_in);
      L_new = (h[9] + h[11]) + hj_prior(o->shape, o->scale, beta_new, b_new);
      if (!std::isfinite(L_cur)) rc = stb_fail("%s: the log-posterior at the current state (a=%g, b=%g) is not finite", who, a_in, b_in);
      if (!rc && L_new != L_new) rc = stb_fail("%s: the log-posterior at the proposed point (a=%g, b=%g) is not a number", who, a_new, b_new);
      if (!rc) {
        // q = sum_s eps_s w_s(cell) / (Z_s da_s db_s) over the stages whose rectangle holds the point
        double q_cur = 0.0, q_new = 0.0;
        for (int s = 0; s < nst; s++) {
          const double eps = s < nst - 1 ? 1.0 / 64.0 : 1.0 - (double)(nst - 1) / 64.0;
          const double dens = eps / (S[s].Z * (S[s].da * S[s].db));
          if (S[s].qcur >= 0) q_cur += dens * S[s].wcur;
          if (F.cell[s] >= 0) q_new += dens * h[s];
        }
        log_alpha = (L_new - L_cur) + (log(q_cur) - log(q_new));
        accepted = log(u[4]) < log_alpha ? 1 : 0;
      }
    }
  }
  if (rc) return 1;
  if (info) {
    memset(info, 0, sizeof(*info));
    info->stages = nst;
    info->accepted = accepted;
    info->evals = evals;
    info->log_alpha = log_alpha;
    info->rect[0] = S[nst - 1].alo;
    info->rect[1] = S[nst - 1].ahi;
    info->rect[2] = S[nst - 1].blo;
    info->rect[3] = S[nst - 1].bhi;
    info->stage_pick = pick + 1;
    info->a_prop = a_new;
    info->b_prop = b_new;
    info->L_cur = L_cur;
    info->L_prop = L_new;
    for (int s = 0; s < nst; s++) {
      info->cell[s] = S[s].cell;
      for (int k = 0; k < 4; k++) info->box[s][k] = S[s].box[k];
    }
    info->L = keep ? hj.keepL.data() : nullptr;
  }
  *a_out = accepted ? a_new : a_in;
  *b_out = accepted ? b_new : b_in;
  return 0;
}

extern "C" int stb_groups_samplejoint(stb_groups_t *g, const uint32_t *d_N, const stb_joint_opts_t *opts, double a_in, double b_in,
                                      double *a_out, double *b_out, stb_joint_info_t *info) {
  if (g && g->I > 0 && !d_N) return stb_fail("stb_groups_samplejoint: d_N is required");
  return stb_hj_samplejoint(g, d_N, nullptr, opts, a_in, b_in, a_out, b_out, info, "stb_groups_samplejoint");
}
