// groups.hip -- stb_groups_*: the (n,t) pairs and per-restaurant totals of one samplea call resident
// in HBM, and aterms (reference lib/samplea.c:46-83) evaluated on them for one discount or a grid: the set's lifetime, the
// choice of form, the evaluation flow.  The cell lists: lists.hip, lists_sorted.hip; the pairs' way to the device: pairs.hip.

#include <rocprim/device/device_radix_sort.hpp>

#include <atomic>

#include "groups.h"

// The sweep gathers table[row(n) + t]; pairs arrive in restaurant order, i.e. random in (n,t), and a
// random 8-byte gather moves a whole 64-byte sector.  Sorting the pairs once by (n,t) (they are reused
// for every evaluation of a samplea call and for all D tables of a grid) makes neighbouring threads
// read neighbouring addresses.  The sum is order-independent up to rounding and stays deterministic.
__global__ void k_pack_pairs(const uint32_t *n, const uint16_t *t, uint64_t G, uint64_t *key) {
  uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g < G) key[g] = ((uint64_t)n[g] << 16) | t[g];
}
__global__ void k_unpack_pairs(const uint64_t *key, uint64_t G, uint32_t *n, uint16_t *t) {
  uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g < G) {
    n[g] = (uint32_t)(key[g] >> 16);
    t[g] = (uint16_t)(key[g] & 0xffff);
  }
}

static int sort_pairs(uint32_t *d_n, uint16_t *d_t, uint64_t G, hipStream_t st) {
  if (G < 2) return 0;
  uint64_t *k0 = nullptr, *k1 = nullptr;
  void *tmp = nullptr;
  size_t tmp_bytes = 0;
  int rc = 1;
  do {
    if (stb_pool_malloc((void **)&k0, sizeof(uint64_t) * G) != hipSuccess || stb_pool_malloc((void **)&k1, sizeof(uint64_t) * G) != hipSuccess) {
      stb_fail("sort_pairs: out of device memory");
      break;
    }
    const unsigned blocks = (unsigned)((G + 255) / 256);
    hipLaunchKernelGGL(k_pack_pairs, dim3(blocks), dim3(256), 0, st, d_n, d_t, G, k0);
    if (rocprim::radix_sort_keys(nullptr, tmp_bytes, k0, k1, (size_t)G, 0, 48, st) != hipSuccess) {
      stb_fail("sort_pairs: radix_sort_keys (size query) failed");
      break;
    }
    if (stb_pool_malloc(&tmp, tmp_bytes ? tmp_bytes : 1) != hipSuccess) {
      stb_fail("sort_pairs: out of device memory");
      break;
    }
    if (rocprim::radix_sort_keys(tmp, tmp_bytes, k0, k1, (size_t)G, 0, 48, st) != hipSuccess) {
      stb_fail("sort_pairs: radix_sort_keys failed");
      break;
    }
    hipLaunchKernelGGL(k_unpack_pairs, dim3(blocks), dim3(256), 0, st, k1, G, d_n, d_t);
    if (hipStreamSynchronize(st) != hipSuccess) {
      stb_fail("sort_pairs: %s", hipGetErrorString(hipGetLastError()));
      break;
    }
    rc = 0;
  } while (0);
  // (the stream was synchronised above, or nothing was launched on these buffers)
  if (rc != 0) (void)hipStreamSynchronize(st);
  stb_pool_free(k0);
  stb_pool_free(k1);
  stb_pool_free(tmp);
  return rc;
}

extern "C" void stb_groups_free(stb_groups_t *g) {
  STB_ENTRY;
  if (!g) return;
  stb_device_scope dev(g->dev);
  std::vector<void *> ptrs = {g->d_n, g->d_T, g->d_t, g->d_bpar, g->d_tables, g->d_S1, g->d_out, g->d_ws_fill, g->d_ws_sweep, g->d_ws_terms,
                              g->d_cnt, g->d_n2, g->d_t2, g->d_dotp, g->d_slab, g->d_icnt, g->d_ninf, g->d_scan_tmp,
                              g->d_gtab, g->d_dS1g, g->d_gout, g->d_ws_da, g->d_ws_dasweep};
  if (g->st) (void)hipStreamSynchronize(g->st);  // nothing may still be using the buffers
  for (void *p : ptrs) stb_pool_free(p);
  for (stb_cell_list &l : g->lists) stb_list_release(l, true);
  stb_pool_free(g->h_out);
  stb_pool_free(g->h_pn);
  stb_pool_free(g->h_pt);
  stb_pool_free(g->h_T);
  stb_pool_free(g->h_bpar);
  if (g->ev_dep) (void)hipEventDestroy(g->ev_dep);
  if (g->ev_done) (void)hipEventDestroy(g->ev_done);
  for (auto &e : g->ev)
    if (e) (void)hipEventDestroy(e);
  if (g->st) (void)hipStreamDestroy(g->st);
  free(g);
}

#define GCHK(expr)                                                                            \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      stb_fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);        \
      stb_groups_free(g);                                                                     \
      return nullptr;                                                                         \
    }                                                                                         \
  } while (0)

// occurrence count of every table cell among the pairs (same classification as k_sweep_partial)
__global__ void k_count_pairs(const uint32_t *n, const uint16_t *t, uint64_t G, unsigned N, unsigned M,
                              unsigned *cnt) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const unsigned nn = n[g], tt = t[g];
  if (nn <= 1 || nn == tt || tt <= 1 || nn < tt || tt > M || nn > N) return;
  atomicAdd(&cnt[stb_row_offset(nn, M) + (tt - 2)], 1u);
}

// out[d] += sum of the DOT kernel's partial sums of table d, in a fixed order (a table of 10^4 columns has
// 41 000 tiles in the halo-block form: 256 threads, each its stride, then a fixed tree)
__global__ __launch_bounds__(256) void k_dot_reduce(const double *dotp, int parts, double *out) {
  __shared__ dd_t red[4];
  const int d = blockIdx.x;
  dd_t acc{0.0, 0.0};
  for (int i = threadIdx.x; i < parts; i += 256) dd_add(acc, dotp[(size_t)d * parts + i]);
  const dd_t tot = block_reduce_dd(acc, red);
  if (threadIdx.x == 0) out[d] += tot.hi + tot.lo;
}

// Last launch of a fused evaluation in the halo-block or the grid form: per discount the fill's partial sums
// (mode 1: one double per tile; mode 2: per strip an exact exponent sum and a mantissa-log sum) and the restaurant
// terms' partial sums, each in a fixed order, their total written to pinned host memory together with the fill's
// error words -- so that the host waits ONCE and copies nothing.
__global__ __launch_bounds__(256) void k_eval_tail(const double *dotp, int parts, const unsigned *parts_extra, int mode, const dd_t *tpart, int nbt, unsigned long long inf,
                                                   const unsigned long long *inf_dev, const unsigned *hdr, double *out_dev, double *out_host, int Dmax,
                                                   double *out_user, double seq) {
  __shared__ dd_t red[4];
  __shared__ double ks[4];
  const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
  const int d = blockIdx.x;
  dd_t acc{0.0, 0.0};
  double k = 0.0;  // (integers below 2^53: exact in any order)
  if (parts_extra) parts += (int)*parts_extra;  // (the grid form's helper jobs: their number lives with their list, on the device)
  if (mode == 2) {
    for (int i = threadIdx.x; i < parts; i += 256) {
      k += dotp[((size_t)d * parts + i) * 2];
      dd_add(acc, dotp[((size_t)d * parts + i) * 2 + 1]);
    }
  } else {
    for (int i = threadIdx.x; i < parts; i += 256) dd_add(acc, dotp[(size_t)d * parts + i]);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) k += __shfl_down(k, off, 64);
  if ((threadIdx.x & 63) == 0) ks[threadIdx.x >> 6] = k;
  dd_t tot = block_reduce_dd(acc, red);
  dd_t tv{0.0, 0.0};
  for (int b = threadIdx.x; b < nbt; b += 256) dd_merge(tv, tpart[(size_t)d * nbt + b]);
  tv = block_reduce_dd(tv, red);
  if (threadIdx.x == 0) {
    if (mode == 2) {
      k = (ks[0] + ks[1]) + (ks[2] + ks[3]);
      // k ln2 in two pieces: k < 2^38 and LN2_HI has 32 trailing zero bits, so the first product rounds at 2^-53 relative
      dd_add(tot, k * LN2_LO);
      dd_add(tot, k * LN2_HI);
    }
    if (inf_dev) inf += *inf_dev;  // (lists built from the count slab: counted on the device)
    const double dots = inf ? -HUGE_VAL : tot.hi + tot.lo;
    const double terms = tv.hi + tv.lo;
    out_dev[d] = dots;
    out_dev[Dmax + d] = terms;
    out_host[d] = terms + dots;
    if (out_user) out_user[d] = terms + dots;  // (stb_groups_aterms_device: the caller's device buffer)
    if (d == 0) {
      out_host[2 * Dmax] = (double)hdr[1];
      out_host[2 * Dmax + 1] = (double)hdr[2];
      // (what the walk took, first workgroup's start to here, in 100 MHz ticks: the host compares it with what the
      // geometry should take -- a GPU shared with other processes shows there and nowhere else)
      const unsigned long long t0 = *reinterpret_cast<const unsigned long long *>(hdr + STB_HDR_T0);
      out_host[2 * Dmax + 3] = t0 ? (double)((unsigned long long)wall_clock64() - t0) : 0.0;
      // (one discount: everything the host waits for is written -- it spins on this word instead of waiting for the
      // launch's completion signal, which reaches it microseconds later; seq = 0: nobody spins)
      if (seq != 0.0 && gridDim.x == 1) {
        __threadfence_system();
        __hip_atomic_store(out_host + 2 * Dmax + 2, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

int stb_restaurant_partials(const double *x_host, int D, const uint32_t *d_T, const double *d_bpar, uint64_t I, void *d_ws,
                            size_t ws_bytes, double *a_out, const dd_t **partial_out, int *nb_out, hipStream_t st);  // sweep_terms.hip

// What depends on the table bounds.  A Gibbs sampler's largest count moves from call to call, and with it the bounds
// of the table samplea builds (lib/samplea.c:186-208): everything below is given back to the buffer cache and asked
// for again in the new sizes (the cache hands a buffer of up to 5/4 the size out again).
int stb_groups_set_bounds(stb_groups_t *g, unsigned N, unsigned M) {
  if (g->have_bounds && g->N == N && g->M == M) return 0;
  if (N < 1 || M < 1) return stb_fail("stb_groups: table bounds N=%u M=%u", N, M);
  HIPCHK(hipStreamSynchronize(g->st));
  g->have_bounds = 0;  // (until everything below has its new size: a failed allocation must not leave a set that looks ready)
  stb_lists_drop(g, false);
  void **ptrs[] = {(void **)&g->d_tables, (void **)&g->d_S1, &g->d_ws_fill};
  for (void **p : ptrs) {
    stb_pool_free(*p);
    *p = nullptr;
  }
  g->N = N;
  g->M = M;
  g->hb_sum_C = stb_hb_sum_C(N, M, g->Dmax);
  g->tstride = (stb_table_elems(N, M) + 31) & ~31ull;
  g->ws_fill = stb_fill_workspace_bytes(N, M, g->Dmax);
  g->ws_zero = 0;
  HIPCHK(stb_pool_malloc((void **)&g->d_ws_fill, g->ws_fill));
  g->fused = stb_env_int("STB_ATERMS_FUSED", 1) && N >= 3 && N < (1u << 27);  // set up on first use
  g->have_bounds = 1;
  return 0;
}

// The tables of the evaluations that store them (one discount on a set without lists, the fallback of a fused
// evaluation that gave up, stb_groups_aterms_tables) are asked for when the first of those comes: a grid of 64
// discounts at N = M = 10^4 is 27 GB of tables that the fused evaluation never touches.
static int ensure_tables(stb_groups_t *g) {
  if (g->d_tables && g->d_S1 && g->d_ws_sweep) return 0;
  if (!g->d_tables && stb_pool_malloc((void **)&g->d_tables, sizeof(double) * g->tstride * g->Dmax) != hipSuccess)
    return stb_fail("stb_groups_aterms: out of device memory for %d tables of %u x %u", g->Dmax, g->N, g->M);
  if (!g->d_S1 && stb_pool_malloc((void **)&g->d_S1, sizeof(double) * (size_t)g->N * g->Dmax) != hipSuccess) return stb_fail("stb_groups_aterms: out of device memory");
  if (!g->d_ws_sweep) {
    g->ws_sweep = stb_sweep_workspace_bytes(g->G, g->Dmax);
    if (stb_pool_malloc((void **)&g->d_ws_sweep, g->ws_sweep) != hipSuccess) return stb_fail("stb_groups_aterms: out of device memory");
  }
  return 0;
}

static stb_groups_t *groups_create_here(int I, const int *K, const uint32_t *T, const uint32_t *nflat,
                                        const uint16_t *tflat, const double *bpar, unsigned N, unsigned M, int Dmax) {
  if (stb_device_count() < 1) {
    stb_no_device("stb_groups_create");
    return nullptr;
  }
  if (Dmax < 1 || Dmax > STB_TERMS_DMAX) {
    stb_fail("stb_groups_create: Dmax=%d (1..%d)", Dmax, STB_TERMS_DMAX);
    return nullptr;
  }
  stb_groups_t *g = (stb_groups_t *)calloc(1, sizeof(*g));
  if (!g) {
    stb_fail("stb_groups_create: out of host memory");
    return nullptr;
  }
  uint64_t G = 0;
  for (int i = 0; i < I; i++) G += (uint64_t)(K[i] > 0 ? K[i] : 0);
  if (hipGetDevice(&g->dev) != hipSuccess) {
    stb_fail("stb_groups_create: %s", hipGetErrorString(hipGetLastError()));
    free(g);
    return nullptr;
  }
  g->I = I;
  g->G = G;
  g->Dmax = Dmax;
  GCHK(hipStreamCreate(&g->st));
  for (auto &e : g->ev) GCHK(hipEventCreate(&e));
  // (the runtime brings a file's kernels to the device on first use: k_eval_tail closes the span an evaluation measures from
  // its walk's start, so it is there before a walk is queued -- not loaded, for milliseconds, between the two launches)
  hipFuncAttributes tail_attr;
  GCHK(hipFuncGetAttributes(&tail_attr, reinterpret_cast<const void *>(k_eval_tail)));
  GCHK(stb_pool_malloc((void **)&g->d_n, sizeof(uint32_t) * (G ? G : 1)));
  GCHK(stb_pool_malloc((void **)&g->d_t, sizeof(uint16_t) * (G ? G : 1)));
  GCHK(stb_pool_malloc((void **)&g->d_T, sizeof(uint32_t) * (I > 0 ? I : 1)));
  GCHK(stb_pool_malloc((void **)&g->d_bpar, sizeof(double) * (I > 0 ? I : 1)));
  GCHK(stb_pool_malloc((void **)&g->h_T, sizeof(uint32_t) * (I > 0 ? I : 1), 1));
  GCHK(stb_pool_malloc((void **)&g->h_bpar, sizeof(double) * (I > 0 ? I : 1), 1));
  for (int i = 0; i < (I > 0 ? I : 1); i++) g->h_bpar[i] = NAN;  // (no concentrations yet: the joint step refuses such a set)
  GCHK(stb_pool_malloc((void **)&g->d_out, sizeof(double) * 2 * Dmax));
  GCHK(stb_pool_malloc((void **)&g->h_out, sizeof(double) * (2 * Dmax + 4), 1));
  GCHK(hipHostGetDevicePointer((void **)&g->h_out_dev, g->h_out, 0));
  GCHK(hipEventCreateWithFlags(&g->ev_dep, hipEventDisableTiming));
  GCHK(hipEventCreateWithFlags(&g->ev_done, hipEventDisableTiming));
  g->ws_terms = stb_terms_workspace_bytes((uint64_t)I, Dmax);
  GCHK(stb_pool_malloc((void **)&g->d_ws_terms, g->ws_terms));
  if (N && M && stb_groups_set_bounds(g, N, M)) {
    stb_groups_free(g);
    return nullptr;
  }
  // (a set may be made empty -- no pairs, or no bounds either -- and filled with stb_groups_pairs_begin / _put / _commit)
  if (nflat && tflat) {
    if (!g->have_bounds) {
      stb_fail("stb_groups_create: pairs without table bounds");
      stb_groups_free(g);
      return nullptr;
    }
    int bad = stb_groups_pairs_begin(g);
    for (uint64_t o = 0; !bad && o < G; o += (1u << 18)) bad = stb_groups_pairs_put(g, nflat + o, tflat + o, G - o < (1u << 18) ? G - o : (1u << 18), nullptr, nullptr);
    if (!bad) bad = stb_groups_pairs_commit(g, T, bpar, N, M);
    if (bad) {
      stb_groups_free(g);
      return nullptr;
    }
  } else if (T && bpar && I > 0 && stb_groups_update_restaurants(g, T, bpar)) {
    stb_groups_free(g);
    return nullptr;
  }
  if (T && bpar) g->reused = 0;  // (what stb_groups_update_restaurants marks is a set that serves call after call)
  return g;
}

// the pairs in (n, t) order, for the gather over stored tables (on first need: see pairs.hip)
int stb_groups_sort_pairs(stb_groups_t *g) {
  if (g->sorted || !stb_env_int("STB_SORT_PAIRS", 1)) return 0;
  if (sort_pairs(g->d_n, g->d_t, g->G, g->st)) return 1;
  g->sorted = 1;
  return 0;
}

// The set lives on the device stb_get_device() names (stb_set_device / STB_DEVICE / the runtime's
// current device); the caller's current device is put back before returning.
extern "C" stb_groups_t *stb_groups_create(int I, const int *K, const uint32_t *T, const uint32_t *nflat,
                                           const uint16_t *tflat, const double *bpar, unsigned N, unsigned M, int Dmax) {
  STB_ENTRY;
  stb_device_scope dev(stb_get_device());
  return groups_create_here(I, K, T, nflat, tflat, bpar, N, M, Dmax);
}

// partial sums of the fused forms: (column blocks of 64) x 16 waves per table for the chain form, one per tile for the
// halo-block form, two per strip and per helper job for the grid form
int stb_groups_alloc_dotp(stb_groups_t *g) {
  const unsigned N = g->N, M = g->M;
  g->dotp_elems = (size_t)g->Dmax * ((size_t)(M + 63) / 64 + 1) * 16;
  const size_t ckp = stb_launch_ck ? (size_t)g->Dmax * stb_ck_dot_parts(N, M, g->Dmax) : 0;
  if (ckp > g->dotp_elems) g->dotp_elems = ckp;
  hb_dot_info H2;
  if (stb_hb_dot_info(N, M, g->Dmax, &H2, g->hb_sum_C) == 0 && (size_t)g->Dmax * H2.n_tiles > g->dotp_elems) g->dotp_elems = (size_t)g->Dmax * H2.n_tiles;
  // (the self-summing form: two sums per strip, strips of 80 columns at the narrowest)
  size_t hb2 = (size_t)g->Dmax * ((size_t)M / 64 + 8) * 2;
  {
    // (... and two per tile left to helper waves: at most grid_geom::job_cap of them)
    grid_geom gj;
    for (int dd : {1, g->Dmax})
      if (stb_grid_geometry(N, M, dd, &gj) == 0 && (size_t)g->Dmax * ((size_t)gj.JW + gj.job_cap) * 2 > hb2)
        hb2 = (size_t)g->Dmax * ((size_t)gj.JW + gj.job_cap) * 2;
  }
  if (hb2 > g->dotp_elems) g->dotp_elems = hb2;
  if (stb_pool_malloc((void **)&g->d_dotp, sizeof(double) * g->dotp_elems) != hipSuccess) return stb_fail("stb_groups_aterms: out of device memory");
  return 0;
}

// Lazy set-up of the fused evaluation (first call with more than one discount): occurrence count
// per table cell, and the pairs that address no cell.  The pairs come back from the device in their
// sorted order, so the result does not depend on the order the caller supplied them in.
static int groups_fused_setup(stb_groups_t *g) {
  const unsigned N = g->N, M = g->M;
  const uint64_t G = g->G;
  const uint64_t elems = stb_table_elems(N, M);
  HIPCHK(stb_pool_malloc((void **)&g->d_cnt, sizeof(unsigned) * (elems ? elems : 1)));
  HIPCHK(hipMemsetAsync(g->d_cnt, 0, sizeof(unsigned) * (elems ? elems : 1), g->st));
  if (G)
    hipLaunchKernelGGL(k_count_pairs, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, g->st, g->d_n, g->d_t, G, N,
                       M, g->d_cnt);
  uint32_t *hn = (uint32_t *)malloc(sizeof(uint32_t) * (G ? G : 1));
  uint16_t *ht = (uint16_t *)malloc(sizeof(uint16_t) * (G ? G : 1));
  if (!hn || !ht) {
    free(hn);
    free(ht);
    return stb_fail("stb_groups_aterms: out of host memory");
  }
  hipError_t e1 = hipSuccess, e2 = hipSuccess;
  if (G) {
    e1 = hipMemcpyAsync(hn, g->d_n, sizeof(uint32_t) * G, hipMemcpyDeviceToHost, g->st);
    e2 = hipMemcpyAsync(ht, g->d_t, sizeof(uint16_t) * G, hipMemcpyDeviceToHost, g->st);
  }
  if (e1 == hipSuccess && e2 == hipSuccess) e1 = hipStreamSynchronize(g->st);
  uint64_t G2 = 0;
  if (e1 == hipSuccess && e2 == hipSuccess) {
    for (uint64_t q = 0; q < G; q++) {  // compact in place: the pairs outside the table
      const unsigned nn = hn[q], tt = ht[q];
      if (nn > 1 && (nn == tt || tt <= 1 || nn < tt || tt > M || nn > N)) {
        hn[G2] = nn;
        ht[G2] = (uint16_t)tt;
        G2++;
      }
    }
    g->G2 = G2;
    e1 = stb_pool_malloc((void **)&g->d_n2, sizeof(uint32_t) * (G2 ? G2 : 1));
    if (e1 == hipSuccess) e2 = stb_pool_malloc((void **)&g->d_t2, sizeof(uint16_t) * (G2 ? G2 : 1));
    if (e1 == hipSuccess && e2 == hipSuccess && G2) {
      e1 = hipMemcpy(g->d_n2, hn, sizeof(uint32_t) * G2, hipMemcpyHostToDevice);
      e2 = hipMemcpy(g->d_t2, ht, sizeof(uint16_t) * G2, hipMemcpyHostToDevice);
    }
  }
  free(hn);
  free(ht);
  if (e1 != hipSuccess || e2 != hipSuccess) return stb_fail("stb_groups_aterms: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
  // partial sums: at most (column blocks of 64) x 16 waves per table
  g->dotp_elems = (size_t)g->Dmax * ((size_t)(M + 63) / 64 + 1) * 16;
  HIPCHK(stb_pool_malloc((void **)&g->d_dotp, sizeof(double) * g->dotp_elems));
  HIPCHK(hipGetLastError());
  g->fused_ready = 1;
  return 0;
}

// one evaluation in two halves: queue everything on the set's stream, the sums ending in pinned host
// memory; then wait, check the fill and hand the values over.  aterms_finish returns 0, 1 (error) or 2
// (the fused chain fill gave up waiting: the caller repeats the evaluation through stored tables).
// The lean flow of a fused evaluation in the halo-block (tile workers sum) or the grid form (walking waves sum):
//   launch 1  restaurant partial sums; the abscissae go to the device as kernel arguments
//   launch 2  the table walk (its workspace is zero already: the previous evaluation left it so)
//   launch 3  k_eval_tail: every reduction, the total and the walk's error words to pinned host memory
//   then, behind what the host waits for, the workspace is zeroed for the next evaluation.
// ONE wait (an event after launch 3), no copy in either direction, no S1 vector, no gather pass.
// fused evaluations that gave up waiting and were repeated through stored tables (process-wide; stb_groups_fallbacks)
static std::atomic<unsigned> g_fused_giveups{0};
extern "C" unsigned stb_groups_fallbacks(void) { return g_fused_giveups.load(); }

static int aterms_issue_lean(stb_groups_t *g, const double *x_host, int D, double *out_host, int which, bool timed, bool ssum) {
  g->pending = 0;
  char *ws0 = (char *)g->d_ws_fill;
  double *a_dev = (double *)ws0;
  char *ws = ws0 + STB_WS_FORM;
  const size_t ws_left = g->ws_fill - STB_WS_FORM;
  if (timed) HIPCHK(hipEventRecord(g->ev[0], g->st));
  const dd_t *tpart = nullptr;
  int nbt = 0;
  // (the pair sum alone: the same launch over no restaurants -- one empty partial per abscissa, and 0 + dots is dots;
  // the abscissae still travel with it)
  g->pend_ssum = ssum ? 1 : 0;
  if (stb_restaurant_partials(x_host, D, g->d_T, g->d_bpar, g->pend_ssum ? 0 : (uint64_t)g->I, g->d_ws_terms, g->ws_terms, a_dev, &tpart, &nbt, g->st))
    return 1;
  dot_request req;
  stb_list_request(g, which, &req);
  req.dotp = g->d_dotp;
  req.dotp_cap = g->dotp_elems;
  req.ws_zero = g->ws_zero;
  req.no_s1 = 1;
  fill_args A;
  memset(&A, 0, sizeof(A));
  A.a = a_dev;
  A.N = g->N;
  A.M = g->M;
  A.tables = g->d_tables;
  A.tstride = g->tstride;
  A.S1 = g->d_S1;
  A.s1stride = g->N;
  if (stb_logtab(&A.lt)) return 1;
  unsigned *hdr = nullptr;
  g->ws_zero = 0;  // (whatever happens below, the workspace is no longer known to be zero)
  g->pend_seq = 0.0;
  if (D == 1 && !timed && stb_env_int("STB_SPIN_WAIT", 1)) {
    g->seq += 1.0;
    g->pend_seq = g->seq;
    ((volatile double *)g->h_out)[2 * g->Dmax + 2] = 0.0;
  }
  if (which >= 3 ? stb_launch_grid(A, D, ws, ws_left, &req, nullptr, &hdr, g->st) : stb_launch_hb(A, D, ws, ws_left, &req, nullptr, &hdr, g->st)) return 1;
  // (the partial sums' room was checked inside the launch functions, before anything was queued: dot_request::dotp_cap)
  if (timed) HIPCHK(hipEventRecord(g->ev[1], g->st));
  if (timed) HIPCHK(hipEventRecord(g->ev[2], g->st));
  hipLaunchKernelGGL(k_eval_tail, dim3(D), dim3(256), 0, g->st, g->d_dotp, req.parts_per_table, req.parts_extra_dev, which >= 3 ? 2 : 1, tpart, nbt,
                     (unsigned long long)g->n_inf, stb_list_from_slab(g->lists[which]) ? g->d_ninf : nullptr, hdr, g->d_out, g->h_out_dev, g->Dmax, g->pend_user,
                     g->pend_seq);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(g->ev[3], g->st));
  // zero for the next evaluation, behind the event the host waits for
  if (req.zero_bytes) {
    HIPCHK(hipMemsetAsync(ws, 0, req.zero_bytes, g->st));
    g->ws_zero = req.zero_bytes;
  }
  g->pending = 1;
  g->pend_lean = 1;
  g->pend_D = D;
  g->pend_fuse = 1;
  g->pend_v = STB_FILL_HB;
  g->pend_out = out_host;
  memcpy(g->pend_x, x_host, sizeof(double) * D);
  return 0;
}

static int aterms_issue(stb_groups_t *g, const double *x_host, int D, double *out_host, bool fuse, int v, bool timed, bool ssum) {
  if (fuse && v == STB_FILL_HB && g->sparse && g->sel_which >= 2)
    return aterms_issue_lean(g, x_host, D, out_host, g->sel_which, timed, ssum);
  g->pend_lean = 0;
  g->pend_ssum = ssum ? 1 : 0;
  g->ws_zero = 0;  // (this flow's fills zero and use the workspace themselves)
  if (ensure_tables(g)) return 1;
  if (!fuse && stb_groups_sort_pairs(g)) return 1;  // (the gather's sum is then independent of the caller's order)
  // (what is left for this flow: the chain form, v = STB_FILL_CK with fuse: the summing checkpointed form and its cell
  // lists, and every evaluation through stored tables)
  const int which = (fuse && v == STB_FILL_CK) ? 1 : 0;
  g->pending = 0;
  HIPCHK(hipEventRecord(g->ev[0], g->st));
  if (fuse) {
    // the chain form as a DOT kernel: sum over table cells of count * log S, no table in memory;
    // then the few pairs that address no cell (t = 1 -> S1, t = n -> 0, out of bounds -> -inf)
    dot_request req;
    if (g->sparse) stb_list_request(g, which, &req);
    else req.cnt = g->d_cnt;
    req.dotp = g->d_dotp;
    req.dotp_cap = g->dotp_elems;
    const fill_request q = {g->N, g->M, D, which ? STB_FILL_CK : STB_FILL_CHAIN, 0, false, &req};
    if (stb_fill(q, x_host, g->d_tables, g->tstride, g->d_S1, g->N, g->d_ws_fill, g->ws_fill, g->st)) return 1;
    stb_fill_last(&g->pend_fill);
    if ((size_t)D * req.parts_per_table > g->dotp_elems) return stb_fail("stb_groups_aterms: partial-sum buffer too small");
    HIPCHK(hipEventRecord(g->ev[1], g->st));
    if (stb_sweep_S(g->d_tables, g->tstride, g->d_S1, g->N, D, g->N, g->M, g->d_n2, g->d_t2, g->G2,
                    g->d_out, g->d_ws_sweep, g->ws_sweep, g->st))
      return 1;
    hipLaunchKernelGGL(k_dot_reduce, dim3(D), dim3(256), 0, g->st, g->d_dotp, req.parts_per_table, g->d_out);
  } else {
    if (stb_fill_S(x_host, D, g->N, g->M, g->d_tables, g->tstride, g->d_S1, g->N, g->d_ws_fill,
                   g->ws_fill, v, g->st))
      return 1;
    stb_fill_last(&g->pend_fill);
    HIPCHK(hipEventRecord(g->ev[1], g->st));
    if (stb_sweep_S(g->d_tables, g->tstride, g->d_S1, g->N, D, g->N, g->M, g->d_n, g->d_t, g->G,
                    g->d_out, g->d_ws_sweep, g->ws_sweep, g->st))
      return 1;
  }
  HIPCHK(hipEventRecord(g->ev[2], g->st));
  if (!g->pend_ssum && stb_restaurant_terms(x_host, D, g->d_T, g->d_bpar, (uint64_t)g->I, g->d_out + g->Dmax,
                                            g->d_ws_terms, g->ws_terms, g->st))
    return 1;
  HIPCHK(hipEventRecord(g->ev[3], g->st));
  HIPCHK(hipMemcpyAsync(g->h_out, g->d_out, sizeof(double) * 2 * g->Dmax, hipMemcpyDeviceToHost, g->st));
  g->pending = 1;
  g->pend_D = D;
  g->pend_fuse = fuse ? 1 : 0;
  g->pend_v = v;
  g->pend_out = out_host;
  memcpy(g->pend_x, x_host, sizeof(double) * D);
  return 0;
}

static int aterms_finish(stb_groups_t *g, float *ms_fill, float *ms_sweep, float *ms_terms) {
  if (!g->pending) return stb_fail("stb_groups_wait: nothing queued");
  g->pending = 0;
  const int D = g->pend_D;
  if (g->pend_lean) {
    bool there = false;
    if (g->pend_seq != 0.0 && !ms_fill && !ms_sweep && !ms_terms) {
      volatile double *flag = g->h_out + 2 * g->Dmax + 2;
      for (unsigned n = 0; n < 4000000u && *flag != g->pend_seq; n++) __builtin_ia32_pause();  // (bounded: the event below otherwise)
      there = *flag == g->pend_seq;
    }
    if (!there) HIPCHK(hipEventSynchronize(g->ev[3]));
    const unsigned code = (unsigned)g->h_out[2 * g->Dmax], detail = (unsigned)g->h_out[2 * g->Dmax + 1];
    if (code != 0) {
      stb_fail("stb_groups_aterms: the fused evaluation gave up waiting for a neighbour block (code 0x%x, block %u of table %u)", code,
               detail & 0xffffu, detail >> 16);
      g_fused_giveups.fetch_add(1u);
      return 2;  // (the caller repeats the evaluation through stored tables)
    }
    for (int d = 0; d < D; d++) g->pend_out[d] = g->h_out[d];
    // (the walk's own span against what D chains of N rows should take: stb_note_span, abi.hip)
    stb_note_span(g->h_out[2 * g->Dmax + 3] * 1e-5, 1e-3 * (100.0 + 0.05 * (double)g->N * (1.0 + (double)D / 16.0)), "a fused evaluation (stb_groups_aterms)");
    if (ms_fill) HIPCHK(hipEventElapsedTime(ms_fill, g->ev[0], g->ev[1]));
    if (ms_sweep) HIPCHK(hipEventElapsedTime(ms_sweep, g->ev[1], g->ev[2]));
    if (ms_terms) HIPCHK(hipEventElapsedTime(ms_terms, g->ev[2], g->ev[3]));
    return 0;
  }
  HIPCHK(hipStreamSynchronize(g->st));
  if (stb_fill_status_of(&g->pend_fill)) {
    if (g->pend_fuse) g_fused_giveups.fetch_add(1u);
    return g->pend_fuse ? 2 : 1;
  }
  // (whether THIS fill was repeated in the producer/consumer form -- not a counter of the calling thread, which other
  // sets' fills move too and which the waiting thread need not share with the issuing one; a fused evaluation stores no
  // table to sweep again)
  if (g->pend_fill.fell_back && !g->pend_fuse) {
    // the one-launch fill gave up and was repeated with the producer/consumer form: the sum above
    // read unfinished tables, take it again
    if (stb_sweep_S(g->d_tables, g->tstride, g->d_S1, g->N, D, g->N, g->M, g->d_n, g->d_t, g->G,
                    g->d_out, g->d_ws_sweep, g->ws_sweep, g->st))
      return 1;
    HIPCHK(hipMemcpyAsync(g->h_out, g->d_out, sizeof(double) * g->Dmax, hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipStreamSynchronize(g->st));
  }
  for (int d = 0; d < D; d++) g->pend_out[d] = g->pend_ssum ? g->h_out[d] : g->h_out[g->Dmax + d] + g->h_out[d];
  if (ms_fill) HIPCHK(hipEventElapsedTime(ms_fill, g->ev[0], g->ev[1]));
  if (ms_sweep) HIPCHK(hipEventElapsedTime(ms_sweep, g->ev[1], g->ev[2]));
  if (ms_terms) HIPCHK(hipEventElapsedTime(ms_terms, g->ev[2], g->ev[3]));
  return 0;
}

static int aterms_once(stb_groups_t *g, const double *x_host, int D, double *out_host, bool fuse, int v,
                       float *ms_fill, float *ms_sweep, float *ms_terms, bool ssum = false) {
  if (aterms_issue(g, x_host, D, out_host, fuse, v, ms_fill || ms_sweep || ms_terms, ssum)) return 1;
  return aterms_finish(g, ms_fill, ms_sweep, ms_terms);
}

// The summing halo-block form (tile workers sum) holds while its spine workgroups leave the workers a quarter of the
// chip: 25/32 of the compute units (200 of an MI355X's 256: 28 discounts of 10^4 columns at 7 strips a workgroup;
// measured 28 discounts 0.99 ms against the grid form's 1.21, 30: 1.55, 32: 2.03 against 1.23).  STB_ATERMS_HB_MAX_SPINE overrides.
static unsigned hb_max_spine() { return stb_spine_room("STB_ATERMS_HB_MAX_SPINE"); }

// which form an evaluation of D discounts takes, with the one-off set-up of the fused form done
static int aterms_prepare(stb_groups_t *g, int D, bool allow_fuse, bool *fuse_out, int *v_out) {
  if (!g) return stb_fail("stb_groups_aterms: null group set");
  if (!g->have_bounds || (g->G && !g->have_pairs)) return stb_fail("stb_groups_aterms: the set has no pairs yet (stb_groups_pairs_begin / _put / _commit)");
  if (g->putting) return stb_fail("stb_groups_aterms: stb_groups_pairs_commit has not been called");
  if (D < 1 || D > g->Dmax) return stb_fail("stb_groups_aterms: D=%d outside 1..%d", D, g->Dmax);
  if (g->pending == 1) return stb_fail("stb_groups_aterms: an evaluation queued with stb_groups_aterms_async has not been waited for");
  const int v = stb_default_variant();
  // one discount: the gather over a stored table needs no set-up; a grid: fused -- and so is a single discount once
  // the set is known to be used again and again (stb_groups_update_restaurants has been called on it: samplea's kept
  // set), where the one-off set-up is paid back: an evaluation is then three launches and one wait whatever D is
  // (round 5: the lists of the halo-block and grid forms come from a count slab in four launches -- lists.hip -- so a
  // single discount on a fresh set is fused too wherever those forms apply; STB_ATERMS_FUSE1=0 restores the old rule)
  bool fuse1 = g->reused;
  if (!fuse1 && D == 1 && stb_env_int("STB_ATERMS_FUSE1", 1) && stb_env_int("STB_LISTS_SLAB", 1) && g->G * 3 <= stb_table_cells(g->N, g->M)) {
    hb_dot_info H1;
    fuse1 = stb_env_int("STB_ATERMS_HB", 1) && stb_hb_dot_info(g->N, g->M, 1, &H1, g->hb_sum_C) == 0;
  }
  // (a GPU shared with other processes: stored tables and the gather, no waits between workgroups -- abi.hip)
  const bool fuse = allow_fuse && !stb_shared_gpu() && g->fused && (D >= 2 || fuse1) &&
                    (v == STB_FILL_SCALED || v == STB_FILL_CHAIN || v == STB_FILL_CK || v == STB_FILL_HB);
  // The summing fill also exists in the checkpointed form (recurrence-only spine + tile workers that walk
  // a tile again and sum its listed cells; STB_ATERMS_CK=1, or variant STB_FILL_CK), usable while its spine
  // workgroups all fit on the chip.  It is not the default: MI355X, 10^6 pairs, N = M = 10^4, its 0.66 ms
  // at 2-4 discounts and 0.85-0.96 at 8 against the chain form's 0.73-0.77 and 0.87-0.97 (tools/ablation/time_grid.py)
  // -- the tiles' requests for edges, checkpoints and cell lists stretch the spine's hand-offs between
  // workgroups from 2 to ~17 us, which eats what the lighter spine gains.
  int which = 0;
  if (fuse && stb_launch_ck && (stb_env_int("STB_ATERMS_CK", 0) || v == STB_FILL_CK) && v != STB_FILL_CHAIN && stb_ck_eligible(g->N, g->M, D) &&
      stb_ck_dot_spine(g->N, g->M, D) <= (unsigned)stb_env_int("STB_ATERMS_CK_MAX_SPINE", 208))
    which = 1;
  // ... and in the halo-block form (a spine that walks blocks of rows alone + tile workers that sum their
  // tiles' listed cells): the default for a grid while the chip holds its spine -- 49 strips per table of 10^4
  // columns, four to a workgroup up to 17 discounts, seven beyond: up to 24 discounts (1200 strips in all); STB_ATERMS_HB=0 switches
  // it off.  (MI355X, tools/ablation/time_grid.py, 10^6 pairs, N = M = 10^4, kernel / wall ms: 2 discounts 0.36 / 0.45
  // against 0.76 / 0.83 chain, 4: 0.36 / 0.45 against 0.78 / 0.86, 8: 0.44 / 0.53 against 0.89 / 0.97, 16: 0.76 /
  // 0.86 against 0.98 / 1.07, 24: 1.07 / 1.15 against 1.25 / 1.34, 28: 1.22 against 1.32, 30: 1.55 against 1.37,
  // 64: 2.7 against 2.4.)
  // ... and with the walking waves themselves summing their strips' listed cells, no tile workers at all (grid_hb.hip):
  // what a grid beyond the halo-block form's range takes instead of the chain form while the pairs are sparse in the
  // table (its look-ups take one listed cell per lane and group of rows: 10^6 pairs over a 10^4 x 10^4 table, 2 % of
  // the cells, fill them; 12 % -- the same pairs with n < 4000 -- overflow every group).  STB_ATERMS_GRID=1 / 0 forces
  // it on (wherever its geometry exists) / off.  (MI355X, tools/ab_grid.py, 10^6 pairs, N = M = 10^4, kernel ms: 32
  // discounts 1.44 = chain, 48: 1.56 against 1.88, 64: 1.62 against 2.39; N = M = 4000, 64 discounts: 1.35 against 0.57.)
  if (fuse && which == 0 && (v == STB_FILL_HB || v == STB_FILL_SCALED)) {
    const int force = stb_env_int("STB_ATERMS_GRID", -1);
    grid_geom gg;
    if (force != 0 && stb_grid_geometry(g->N, g->M, D, &gg) == 0) {
      hb_dot_info H;
      const bool hb_range = stb_hb_dot_info(g->N, g->M, D, &H, g->hb_sum_C) == 0 && H.n_spine <= hb_max_spine();
      const bool sparse_pairs = (double)g->G <= 0.04 * (double)stb_table_cells(g->N, g->M);
      if (force > 0 || (!hb_range && sparse_pairs && stb_env_int("STB_ATERMS_HB", 1))) which = stb_grid_which(gg.C);
    }
  }
  if (fuse && which == 0 && (v == STB_FILL_HB || (v == STB_FILL_SCALED && stb_env_int("STB_ATERMS_HB", 1)))) {
    hb_dot_info H;
    if (stb_hb_dot_info(g->N, g->M, D, &H, g->hb_sum_C) == 0 && H.n_spine <= hb_max_spine()) which = 2;
  }
  if (fuse && stb_env_int("STB_ATERMS_SPARSE", 1) && (!g->fused_ready || g->sparse) && stb_lists_build(g, which, D)) return 1;
  if (fuse && !g->fused_ready && groups_fused_setup(g)) return 1;
  if (fuse && !g->sparse) which = 0;  // (dense pair sets: the count slab, chain form only)
  bool fuse2 = fuse;
  if (fuse && g->sparse && !g->lists[which].ready) fuse2 = false;  // (no list in this layout: stored tables + gather)
  g->sel_which = which;
  // (diagnostics, stb_groups_last_form: the strip shape the lists of this layout were built for)
  g->last_fused = fuse2 ? 1 : 0;
  g->last_C = !fuse2 || which < 2 ? 0 : (which == 2 ? g->hb_sum_C : stb_which_C(which));
  g->last_R = !fuse2 || which < 2 ? 0 : g->lists[which].R;
  *fuse_out = fuse2;
  *v_out = !fuse2 ? v : (which >= 2 ? STB_FILL_HB : (which ? STB_FILL_CK : STB_FILL_CHAIN));
  return 0;
}

static int groups_aterms(stb_groups_t *g, const double *x_host, int D, double *out_host, bool allow_fuse, float *ms_fill,
                         float *ms_sweep, float *ms_terms, bool ssum = false) {
  if (!g) return stb_fail("stb_groups_aterms: null group set");
  stb_device_scope dev(g->dev);
  bool fuse = false;
  int v = 0;
  int rc = aterms_prepare(g, D, allow_fuse, &fuse, &v);
  if (!rc) rc = aterms_once(g, x_host, D, out_host, fuse, v, ms_fill, ms_sweep, ms_terms, ssum);
  if (rc == 2)  // no waits between workgroups in this form
    rc = aterms_once(g, x_host, D, out_host, false, STB_FILL_PC, ms_fill, ms_sweep, ms_terms, ssum) ? 1 : 0;
  return rc;
}

// The same evaluation in two calls, so that one host thread can keep several GPUs (or several group
// sets) busy: _async queues it on the set's own stream -- behind whatever `stream` holds at this moment,
// when `stream` is not NULL -- and returns; stb_groups_wait blocks until it is through and only then
// writes out_host[0..D-1].  x_host may be reused at once; out_host must stay valid until the wait.
// One evaluation per set at a time.
extern "C" int stb_groups_aterms_async(stb_groups_t *g, const double *x_host, int D, double *out_host, void *stream) {
  STB_ENTRY;
  if (!g) return stb_fail("stb_groups_aterms_async: null group set");
  stb_device_scope dev(g->dev);
  bool fuse = false;
  int v = 0;
  if (aterms_prepare(g, D, true, &fuse, &v)) return 1;
  if (stream && (hipEventRecord(g->ev_dep, (hipStream_t)stream) != hipSuccess || hipStreamWaitEvent(g->st, g->ev_dep, 0) != hipSuccess))
    return stb_fail("stb_groups_aterms_async: %s", hipGetErrorString(hipGetLastError()));
  return aterms_issue(g, x_host, D, out_host, fuse, v, false, false);
}

extern "C" int stb_groups_wait(stb_groups_t *g) {
  STB_ENTRY;
  if (!g) return stb_fail("stb_groups_wait: null group set");
  if (g->pending == 2) {  // (stb_groups_aterms_device in a flow that finished inside the call)
    g->pending = 0;
    return 0;
  }
  stb_device_scope dev(g->dev);
  double *out = g->pend_out;
  const int D = g->pend_D;
  double x[STB_TERMS_DMAX];
  memcpy(x, g->pend_x, sizeof(x));
  double *user = g->pend_user;
  const bool lean = g->pend_lean != 0;
  g->pend_user = nullptr;
  int rc = aterms_finish(g, nullptr, nullptr, nullptr);
  const bool redo = rc == 2;
  const bool ssum = g->pend_ssum != 0;  // (the repeat is the same kind of evaluation)
  if (rc == 2) rc = aterms_once(g, x, D, out, false, STB_FILL_PC, nullptr, nullptr, nullptr, ssum) ? 1 : 0;
  // (stb_groups_aterms_device: only the lean flow's last launch writes the caller's device buffer itself)
  if (!rc && user && (redo || !lean)) {
    if (hipMemcpyAsync(user, out, sizeof(double) * D, hipMemcpyHostToDevice, g->st) != hipSuccess || hipStreamSynchronize(g->st) != hipSuccess)
      rc = stb_fail("stb_groups_wait: %s", hipGetErrorString(hipGetLastError()));
  }
  return rc;
}

// The same evaluation with the D log-posteriors left on the DEVICE, in d_out[0..D): what a caller that hands them to a
// collective wants (the discount axis sharded over GPUs: every rank all-gathers its share) -- no copy to
// the host and back.  Queued on the set's stream behind what `stream` holds now; `stream` in turn waits (on the device)
// for the values, so work queued on it afterwards sees them.  stb_groups_wait(g) must still be called -- before the
// values are trusted: it reports a walk that gave up waiting, and then re-evaluates through stored tables and rewrites
// d_out.
static int groups_eval_device(stb_groups_t *g, const double *x_host, int D, double *d_out, void *stream, bool ssum, const char *who) {
  if (!g || !d_out) return stb_fail("%s: null argument", who);
  stb_device_scope dev(g->dev);
  bool fuse = false;
  int v = 0;
  int rc = aterms_prepare(g, D, true, &fuse, &v);
  if (!rc && stream) {
    if (hipEventRecord(g->ev_dep, (hipStream_t)stream) != hipSuccess || hipStreamWaitEvent(g->st, g->ev_dep, 0) != hipSuccess)
      rc = stb_fail("%s: %s", who, hipGetErrorString(hipGetLastError()));
  }
  if (!rc) {
    g->pend_user = d_out;
    rc = aterms_issue(g, x_host, D, g->pend_host, fuse, v, false, ssum);
    if (rc) g->pend_user = nullptr;
  }
  if (!rc && !g->pend_lean) {
    // (only the lean flow's last launch writes a device buffer: the other flows are finished here and the totals
    // copied, on the set's stream; the wait that must follow has nothing left to do)
    g->pend_user = nullptr;
    rc = aterms_finish(g, nullptr, nullptr, nullptr);
    if (rc == 2) rc = aterms_once(g, x_host, D, g->pend_host, false, STB_FILL_PC, nullptr, nullptr, nullptr, ssum) ? 1 : 0;
    if (!rc && hipMemcpyAsync(d_out, g->pend_host, sizeof(double) * D, hipMemcpyHostToDevice, g->st) != hipSuccess)
      rc = stb_fail("%s: %s", who, hipGetErrorString(hipGetLastError()));
    if (!rc) g->pending = 2;
  }
  if (!rc && (hipEventRecord(g->ev_done, g->st) != hipSuccess || hipStreamWaitEvent((hipStream_t)stream, g->ev_done, 0) != hipSuccess))
    rc = stb_fail("%s: %s", who, hipGetErrorString(hipGetLastError()));
  return rc;
}

extern "C" int stb_groups_aterms_device(stb_groups_t *g, const double *x_host, int D, double *d_out, void *stream) {
  STB_ENTRY;
  return groups_eval_device(g, x_host, D, d_out, stream, false, "stb_groups_aterms_device");
}

// The pair sum alone, W(x_d) = sum over pairs with n > 1 of S_S_{x_d}(n, t): the evaluation above without its restaurant
// terms -- same choice of form, same lists, same fallbacks (what the joint step of hyperj.hip adds its own R(a, b) to).
extern "C" int stb_groups_ssum_device(stb_groups_t *g, const double *x_host, int D, double *d_out, void *stream) {
  STB_ENTRY;
  return groups_eval_device(g, x_host, D, d_out, stream, true, "stb_groups_ssum_device");
}

extern "C" int stb_groups_ssum(stb_groups_t *g, const double *x_host, int D, double *out_host) {
  STB_ENTRY;
  if (!g) return stb_fail("stb_groups_ssum: null group set");
  return groups_aterms(g, x_host, D, out_host, true, nullptr, nullptr, nullptr, true);
}

extern "C" int stb_groups_aterms_timed(stb_groups_t *g, const double *x_host, int D, double *out_host, float *ms_fill,
                                       float *ms_sweep, float *ms_terms) {
  STB_ENTRY;
  return groups_aterms(g, x_host, D, out_host, true, ms_fill, ms_sweep, ms_terms);
}

extern "C" int stb_groups_aterms(stb_groups_t *g, const double *x_host, int D, double *out_host) {
  STB_ENTRY;
  return groups_aterms(g, x_host, D, out_host, true, nullptr, nullptr, nullptr);
}

// the same values through stored tables and the sorted gather whatever D is: no set-up, which is
// what a handful of abscissae evaluated once (ARMS' three starting points) want
// ---- the node from ONE host thread (SURVEY 8e for a C caller; the reference's callers are C: lib/samplea.c:155,
// test/demo.c:478-480).  k group sets -- normally one per device, each made after stb_set_device(dev) from the same pairs
// (stb_groups_create_node does that) -- take contiguous blocks of the D abscissae, sizes differing by at most one, all are
// queued before any is waited for, and out_host[0..D) comes back in the grid's order.  No collective: a C caller's
// "gather" is D doubles arriving in pinned host memory, 8 bytes a discount; RCCL is the transport of the one-process-per-GPU
// layout (libstb_amd/shard.py, bench.py), where the values stay on the devices.
extern "C" int stb_groups_aterms_multi(stb_groups_t *const *sets, int k, const double *x_host, int D, double *out_host) {
  STB_ENTRY;
  if (!sets || k < 1 || !x_host || !out_host || D < 1) return stb_fail("stb_groups_aterms_multi: bad argument (k=%d D=%d)", k, D);
  if (k > D) k = D;  // (a set without a discount sits the call out)
  for (int s = 0; s < k; s++)
    if (!sets[s]) return stb_fail("stb_groups_aterms_multi: set %d is null", s);
  int rc = 0, queued = 0;
  char first_err[512] = "";
  for (int s = 0; s < k && !rc; s++) {
    const int lo = (int)((long long)D * s / k), hi = (int)((long long)D * (s + 1) / k);
    rc = stb_groups_aterms_async(sets[s], x_host + lo, hi - lo, out_host + lo, nullptr);
    if (!rc) queued++;
  }
  if (rc) snprintf(first_err, sizeof(first_err), "%s", stb_last_error());
  for (int s = 0; s < queued; s++)  // (whatever was queued is waited for, error or not)
    if (stb_groups_wait(sets[s]) && !rc) {
      rc = 1;
      snprintf(first_err, sizeof(first_err), "%s", stb_last_error());
    }
  return rc ? stb_fail("stb_groups_aterms_multi: %s", first_err) : 0;
}

// one set per device for the call above: min(ndev, stb_device_count()) sets of the same pairs on devices 0, 1, ..., each able to
// take Dmax discounts (so that any split of a grid of k * Dmax fits); returns how many were made (0: failure, nothing is left)
extern "C" int stb_groups_create_node(int ndev, int I, const int *K, const uint32_t *T, const uint32_t *nflat, const uint16_t *tflat,
                                      const double *bpar, unsigned N, unsigned M, int Dmax, stb_groups_t **sets_out) {
  STB_ENTRY;
  const int have = stb_device_count();
  if (!sets_out || ndev < 1 || have < 1) {
    stb_fail("stb_groups_create_node: %s", have < 1 ? "no HIP device" : "bad argument");
    return 0;
  }
  const int k = ndev < have ? ndev : have;
  for (int s = 0; s < k; s++) {
    {
      stb_device_scope dev(s);
      sets_out[s] = groups_create_here(I, K, T, nflat, tflat, bpar, N, M, Dmax);
    }
    if (!sets_out[s]) {
      char msg[512];
      snprintf(msg, sizeof(msg), "%s", stb_last_error());
      for (int q = 0; q < s; q++) stb_groups_free(sets_out[q]);
      stb_fail("stb_groups_create_node: device %d: %s", s, msg);
      return 0;
    }
  }
  return k;
}

extern "C" int stb_groups_aterms_tables(stb_groups_t *g, const double *x_host, int D, double *out_host) {
  STB_ENTRY;
  return groups_aterms(g, x_host, D, out_host, false, nullptr, nullptr, nullptr);
}

// new per-restaurant totals and concentrations for the same (n,t) pairs (they change with every
// sweep of a Gibbs sampler while the pairs -- sorted once -- may not)
extern "C" int stb_groups_update_restaurants(stb_groups_t *g, const uint32_t *T, const double *bpar) {
  STB_ENTRY;
  if (!g) return stb_fail("stb_groups_update_restaurants: null group set");
  if (g->pending == 1) return stb_fail("stb_groups_update_restaurants: an evaluation queued with stb_groups_aterms_async has not been waited for");
  stb_device_scope dev(g->dev);
  g->reused = 1;
  if (g->I <= 0) return 0;
  // through pinned memory: the caller's arrays are free again on return, and nothing waits for the copy but the
  // evaluation queued behind it (the wait at the START is for an earlier copy out of the same staging area)
  if (hipStreamSynchronize(g->st) != hipSuccess) return stb_fail("stb_groups_update_restaurants: %s", hipGetErrorString(hipGetLastError()));
  memcpy(g->h_T, T, sizeof(uint32_t) * (size_t)g->I);
  memcpy(g->h_bpar, bpar, sizeof(double) * (size_t)g->I);
  if (hipMemcpyAsync(g->d_T, g->h_T, sizeof(uint32_t) * g->I, hipMemcpyHostToDevice, g->st) != hipSuccess ||
      hipMemcpyAsync(g->d_bpar, g->h_bpar, sizeof(double) * g->I, hipMemcpyHostToDevice, g->st) != hipSuccess)
    return stb_fail("stb_groups_update_restaurants: %s", hipGetErrorString(hipGetLastError()));
  return 0;
}

// the hand-over of a resident-count object's pairs, T and (on request) concentrations: groups.h
int stb_groups_take_counts(stb_groups_t *g, const stb_counts_view &v, const double *bpar, const char *who) {
  if (g->I != v.I || g->G != v.G)
    return stb_fail("%s: the group set has I=%d, G=%llu; the %s I=%d, G=%llu", who, g->I, (unsigned long long)g->G, v.noun, v.I,
                    (unsigned long long)v.G);
  if (g->dev != v.dev) return stb_fail("%s: the group set is on device %d, the %s on %d", who, g->dev, v.noun, v.dev);
  if (g->pending == 1) return stb_fail("%s: an evaluation queued with stb_groups_aterms_async has not been waited for", who);
  if (g->putting) return stb_fail("%s: the group set is between stb_groups_pairs_begin and _commit", who);
  if (bpar == STB_BPAR_RESIDENT && !v.resident) return stb_fail("%s: STB_BPAR_RESIDENT, but the object holds no concentrations yet", who);
  // the bounds the new pairs can need, known without looking at them: n up to max n, t up to min(max n, M)
  unsigned N = g->have_bounds ? g->N : 0, M = g->have_bounds ? g->M : 0;
  if (N < v.maxn) N = v.maxn;
  const unsigned tcap = v.maxn < v.Mdraw ? v.maxn : v.Mdraw;
  if (M < tcap) M = tcap;
  if (N < 1) N = 1;
  if (M < 1) M = 1;
  if (hipStreamSynchronize(g->st) != hipSuccess) return STB_STREAM_FAIL(who);
  if (stb_groups_set_bounds(g, N, M)) return 1;  // (re-sizes what depends on the bounds when they grow)
  stb_event_owner ev;
  if (hipEventCreateWithFlags(&ev.ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(ev.ev, v.st) != hipSuccess ||
      hipStreamWaitEvent(g->st, ev.ev, 0) != hipSuccess)
    return STB_STREAM_FAIL(who);
  if ((v.G && (hipMemcpyAsync(g->d_n, v.d_n, sizeof(uint32_t) * v.G, hipMemcpyDeviceToDevice, g->st) != hipSuccess ||
               hipMemcpyAsync(g->d_t, v.d_t, sizeof(uint16_t) * v.G, hipMemcpyDeviceToDevice, g->st) != hipSuccess)) ||
      hipMemcpyAsync(g->d_T, v.d_T, sizeof(uint32_t) * v.I, hipMemcpyDeviceToDevice, g->st) != hipSuccess)
    return STB_STREAM_FAIL(who);
  if (bpar == STB_BPAR_RESIDENT) {  // (g->st waits for the object's stream above)
    for (int i = 0; i < g->I; i++) g->h_bpar[i] = NAN;  // (the host's copy no longer says what the set holds)
    if (hipMemcpyAsync(g->d_bpar, v.d_bpar, sizeof(double) * g->I, hipMemcpyDeviceToDevice, g->st) != hipSuccess) return STB_STREAM_FAIL(who);
  } else if (bpar) {
    memcpy(g->h_bpar, bpar, sizeof(double) * (size_t)g->I);  // (g->st was idle above: its staging area is free)
    if (hipMemcpyAsync(g->d_bpar, g->h_bpar, sizeof(double) * g->I, hipMemcpyHostToDevice, g->st) != hipSuccess) return STB_STREAM_FAIL(who);
  }
  // the object's later work must not overwrite the pairs before the set has its copy
  if (hipEventRecord(ev.ev, g->st) != hipSuccess || hipStreamWaitEvent(v.st, ev.ev, 0) != hipSuccess) return STB_STREAM_FAIL(who);
  stb_groups_new_pairs(g, 1);  // (reused, as stb_groups_update_restaurants marks: a set that serves sweep after sweep)
  return 0;
}

extern "C" int stb_groups_last_form(const stb_groups_t *g, int *fused, int *which, int *sparse, int *C_out, int *R_out) {
  if (!g) return 1;
  if (fused) *fused = g->last_fused;
  if (which) *which = g->sel_which;
  if (sparse) *sparse = g->sparse;
  if (C_out) *C_out = g->last_C;
  if (R_out) *R_out = g->last_R;
  return 0;
}

extern "C" int stb_groups_shape(const stb_groups_t *g, int *I, uint64_t *G, unsigned *N, unsigned *M, int *Dmax) {
  if (!g) return 1;
  if (I) *I = g->I;
  if (G) *G = g->G;
  if (N) *N = g->N;
  if (M) *M = g->M;
  if (Dmax) *Dmax = g->Dmax;
  return 0;
}
