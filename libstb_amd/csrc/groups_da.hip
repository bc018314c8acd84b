// groups_da.hip -- the gradient of aterms in the discount on a group set, and the mode it leads to.
//
// stb_groups_aterms_grad: the value is stb_groups_aterms's own (that call is made: the same bits); the gradient is
//     sum_i d/dx restaurant terms (stb_restaurant_terms_da)  +  sum over pairs with n > 1 of g_x(n, t) (stb_sweep_dS)
// from tables of g = d log S / da that belong to the set (stb_fill_dS), asked for when the first gradient comes and sized
// by the set's bounds.  The reference has neither (lib/samplea.c evaluates aterms only; its samplers are derivative-free).
// stb_groups_modea: the maximum of aterms on [a_lo, a_hi] by sectioning a bracket with a batch of gradients a round;
// plain host C around stb_groups_aterms_grad, no random numbers.

#include "groups.h"

static int da_ensure(stb_groups_t *g) {
  // (bounds below 2 hold no table cell: the slab is then never read, and a smallest one keeps the fill's arguments legal)
  const unsigned N = g->N < 2 ? 2 : g->N, M = g->M < 2 ? 2 : g->M;
  if (!g->d_gout && stb_pool_malloc((void **)&g->d_gout, sizeof(double) * 2 * g->Dmax) != hipSuccess)
    return stb_fail("stb_groups_aterms_grad: out of device memory");
  if (!g->d_gtab || g->da_N != N || g->da_M != M) {
    HIPCHK(hipStreamSynchronize(g->st));
    void **ptrs[] = {(void **)&g->d_gtab, (void **)&g->d_dS1g, &g->d_ws_da};
    for (void **p : ptrs) {
      stb_pool_free(*p);
      *p = nullptr;
    }
    g->da_stride = (stb_table_elems(N, M) + 31) & ~31ull;
    g->ws_da = stb_fill_dS_workspace_bytes(N, M, g->Dmax);
    if (stb_pool_malloc((void **)&g->d_gtab, sizeof(double) * g->da_stride * g->Dmax) != hipSuccess ||
        stb_pool_malloc((void **)&g->d_dS1g, sizeof(double) * (size_t)N * g->Dmax) != hipSuccess ||
        stb_pool_malloc(&g->d_ws_da, g->ws_da) != hipSuccess) {
      for (void **p : ptrs) {
        stb_pool_free(*p);
        *p = nullptr;
      }
      return stb_fail("stb_groups_aterms_grad: out of device memory for %d tables of %u x %u", g->Dmax, N, M);
    }
    g->da_N = N;
    g->da_M = M;
  }
  if (!g->d_ws_dasweep || g->da_G != g->G) {
    HIPCHK(hipStreamSynchronize(g->st));
    stb_pool_free(g->d_ws_dasweep);
    g->d_ws_dasweep = nullptr;
    g->ws_dasweep = stb_sweep_workspace_bytes(g->G, g->Dmax);
    if (stb_pool_malloc(&g->d_ws_dasweep, g->ws_dasweep) != hipSuccess) return stb_fail("stb_groups_aterms_grad: out of device memory");
    g->da_G = g->G;
  }
  return 0;
}

static int grad_here(stb_groups_t *g, const double *x_host, int D, double *val, double *grad) {
  if (da_ensure(g)) return 1;
  // (the pairs in (n, t) order, as the gather over stored tables has them: the sum's order is then the same call after call)
  if (stb_groups_sort_pairs(g)) return 1;
  if (stb_fill_dS(x_host, D, g->da_N, g->da_M, g->d_gtab, g->da_stride, g->d_dS1g, g->da_N, nullptr, 0, nullptr, 0, g->d_ws_da, g->ws_da, g->st))
    return 1;
  if (stb_sweep_dS(g->d_gtab, g->da_stride, g->d_dS1g, g->da_N, D, g->N, g->M, g->d_n, g->d_t, g->G, g->d_gout, g->d_ws_dasweep, g->ws_dasweep,
                   g->st))
    return 1;
  if (stb_restaurant_terms_da(x_host, D, g->d_T, g->d_bpar, (uint64_t)g->I, g->d_gout + g->Dmax, g->d_ws_terms, g->ws_terms, g->st)) return 1;
  double h[2 * STB_TERMS_DMAX];
  HIPCHK(hipMemcpyAsync(h, g->d_gout, sizeof(double) * 2 * g->Dmax, hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipStreamSynchronize(g->st));
  for (int d = 0; d < D; d++) grad[d] = h[g->Dmax + d] + h[d];  // restaurant terms + pair sum, one rounding
  (void)val;
  return 0;
}

extern "C" int stb_groups_aterms_grad(stb_groups_t *g, const double *x_host, int D, double *val_out, double *grad_out) {
  STB_ENTRY;
  if (!g) return stb_fail("stb_groups_aterms_grad: null group set");
  if (!x_host || !val_out || !grad_out) return stb_fail("stb_groups_aterms_grad: null pointer");
  if (D < 1 || D > g->Dmax) return stb_fail("stb_groups_aterms_grad: D=%d outside 1..%d", D, g->Dmax);
  if (!g->have_bounds || !g->have_pairs || g->G == 0)
    return stb_fail("stb_groups_aterms_grad: the set has no pairs yet (stb_groups_pairs_begin / _put / _commit)");
  for (int d = 0; d < D; d++)
    if (!(x_host[d] > 0.0 && x_host[d] < 1.0)) return stb_fail("stb_groups_aterms_grad: discount %g outside (0,1)", x_host[d]);
  double val[STB_TERMS_DMAX], grad[STB_TERMS_DMAX];
  if (stb_groups_aterms(g, x_host, D, val)) return 1;
  {
    stb_device_scope dev(g->dev);
    if (grad_here(g, x_host, D, val, grad)) return 1;
  }
  memcpy(val_out, val, sizeof(double) * D);
  memcpy(grad_out, grad, sizeof(double) * D);
  return 0;
}

// The mode of aterms on [a_lo, a_hi].  k = min(Dmax, 8).
//   round 1     k points lo + i (hi - lo) / (k - 1), i = 0 .. k-1: both bounds are among them.  grad(a_lo) <= 0: the mode is
//               a_lo (at_bound -1); else grad(a_hi) >= 0: a_hi (at_bound +1).
//   round r > 1 k interior points lo + (i + 1) (hi - lo) / (k + 1) of the bracket, whose ends' gradients are known.
//   every round the bracket becomes the leftmost pair of neighbouring points with gradients (> 0, <= 0); rounds end at
//               width <= tol, at rounds_max, or when a round no longer narrows the bracket (its points coincide with its ends).
//   the mode    one secant step inside the last bracket, lo - g_lo (hi - lo) / (g_hi - g_lo), kept inside it.
//   last call   a_hat - delta, a_hat, a_hat + delta with delta = the last bracket's width (tol at a bound), cut to half the
//               distance from a_hat to 0 and to 1: curv = (g(a_hat + delta) - g(a_hat - delta)) / (2 delta), info->grad = g(a_hat).
// A gradient that is not a number (a log-0 pair) fails the call.
extern "C" int stb_groups_modea(stb_groups_t *g, double a_lo, double a_hi, double tol, int rounds_max, double *a_hat, double *curv,
                                stb_modea_info_t *info) {
#pragma clang fp contract(off)
  STB_ENTRY;
  const char *who = "stb_groups_modea";
  if (!g) return stb_fail("%s: null group set", who);
  if (!a_hat) return stb_fail("%s: null pointer", who);
  if (!(a_lo > 0.0 && a_lo < a_hi && a_hi < 1.0)) return stb_fail("%s: interval [%g, %g] (0 < a_lo < a_hi < 1)", who, a_lo, a_hi);
  if (!(tol > 0.0) || rounds_max < 1) return stb_fail("%s: tol=%g rounds_max=%d", who, tol, rounds_max);
  if (g->Dmax < 3) return stb_fail("%s: the set needs Dmax >= 3 (has %d)", who, g->Dmax);
  const int k = g->Dmax < 8 ? g->Dmax : 8;
  double x[10], gr[10], val[8];
  double lo = a_lo, hi = a_hi, glo = 0.0, ghi = 0.0;
  int rounds = 0, evals = 0, at_bound = 0;
  for (;;) {
    const bool first = rounds == 0;
    double px[8];
    for (int i = 0; i < k; i++) px[i] = first ? lo + (double)i * (hi - lo) / (double)(k - 1) : lo + (double)(i + 1) * (hi - lo) / (double)(k + 1);
    if (first) px[k - 1] = hi;
    if (stb_groups_aterms_grad(g, px, k, val, gr + 1)) return 1;
    rounds++;
    evals += k;
    for (int i = 0; i < k; i++)
      if (gr[1 + i] != gr[1 + i]) return stb_fail("%s: the gradient at %.17g is not a number (a pair whose S is 0)", who, px[i]);
    int np;  // points x[0 .. np), gradients gr[0 .. np)
    if (first) {
      for (int i = 0; i < k; i++) {
        x[i] = px[i];
        gr[i] = gr[1 + i];
      }
      np = k;
      if (gr[0] <= 0.0) {
        at_bound = -1;
        hi = lo;
        glo = ghi = gr[0];
        break;
      }
      if (gr[k - 1] >= 0.0) {
        at_bound = 1;
        lo = hi;
        glo = ghi = gr[k - 1];
        break;
      }
    } else {
      x[0] = lo;
      gr[0] = glo;
      for (int i = 0; i < k; i++) x[1 + i] = px[i];
      x[k + 1] = hi;
      gr[k + 1] = ghi;
      np = k + 2;
    }
    int i = 0;
    while (i + 2 < np && !(gr[i] > 0.0 && gr[i + 1] <= 0.0)) i++;  // (the ends are (+, -): one such pair exists)
    const bool narrowed = (x[i + 1] - x[i]) < (hi - lo);
    lo = x[i];
    hi = x[i + 1];
    glo = gr[i];
    ghi = gr[i + 1];
    if (hi - lo <= tol || rounds >= rounds_max || !narrowed) break;
  }
  double ah = lo;
  if (!at_bound) {
    ah = lo - glo * (hi - lo) / (ghi - glo);
    if (!(ah >= lo)) ah = lo;
    if (ah > hi) ah = hi;
  }
  double delta = at_bound ? tol : hi - lo;
  if (delta > 0.5 * ah) delta = 0.5 * ah;
  if (delta > 0.5 * (1.0 - ah)) delta = 0.5 * (1.0 - ah);
  double px[3] = {ah - delta, ah, ah + delta}, g3[3];
  if (stb_groups_aterms_grad(g, px, 3, val, g3)) return 1;
  evals += 3;
  *a_hat = ah;
  if (curv) *curv = (g3[2] - g3[0]) / (2.0 * delta);
  if (info) {
    info->rounds = rounds;
    info->evals = evals;
    info->at_bound = at_bound;
    info->lo = lo;
    info->hi = hi;
    info->g_lo = glo;
    info->g_hi = ghi;
    info->grad = g3[1];
    info->delta = delta;
  }
  return 0;
}
