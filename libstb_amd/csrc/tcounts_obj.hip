// tcounts_obj.hip -- the table-count object (stb_tcounts_t) and every stb_tcounts_* entry point: the pairs, totals and weights
// of a set of restaurants on one device, with an S table for the current discount and a stream of its own.  The host side
// only: the sweep kernels are tcounts.hip's and tcwin.hip's, the other steps' kernels live in the files the comments name.

#include <initializer_list>
#include <vector>

#include "stb_common.h"
#include "pool_scratch.h"
#include "groups.h"
#include "tcounts.h"
#include "hyperq.h"
#include "hyperb.h"
#include "hyperj.h"
#include "logjoint.h"

struct stb_tcounts {
  int dev;
  int I;
  uint64_t G;
  unsigned N, M;        // table bounds: N = the largest n (at least 3), M = the column bound the draws are truncated at
  unsigned maxn;
  uint64_t sumn;        // sum of n over the pairs (the partition's histogram bins are uint32)
  bool need_table;      // some pair can have 2 or more tables (min(max n, M) >= 2); otherwise every draw is t = 1
  uint64_t *d_koff;
  uint32_t *d_n, *d_T;
  uint32_t *d_N;        // customers per restaurant (the sum of n over its pairs), built once at create: sampleb's N
  uint16_t *d_t;
  double *d_h;          // null: every h is 1
  double *d_bpar;
  stb_hb_obj hb;        // d_bpar's staging and what it holds; the per-group concentration step's ranges, L, Y (hyperb.hip)
  double *d_table, *d_S1;
  uint64_t tstride;
  void *d_ws;
  size_t ws_bytes;
  double a_filled;      // the discount the table holds (NaN: none yet)
  hipStream_t st;
};

// ---- the steps the entry points share

static int tc_check_h(const double *h, uint64_t G, const char *who) {
  for (uint64_t g = 0; g < G; g++)
    if (!(h[g] > 0.0) || !std::isfinite(h[g])) return stb_fail("%s: h[%llu]=%g (must be > 0 and finite)", who, (unsigned long long)g, h[g]);
  return 0;
}

// the object's state as the launches take it (views.h)
static stb_table_view tc_table(const stb_tcounts_t *s) { return {s->d_table, s->N, s->M, s->d_S1}; }
static stb_rest_view tc_rest(const stb_tcounts_t *s, double a) { return {a, s->d_bpar, s->I, s->d_koff, s->d_h}; }
static stb_cnts_tT tc_counts(const stb_tcounts_t *s) { return {s->d_n, s->d_t, s->d_T}; }

// what every sweep of the object checks before anything changes: a failure leaves the state as it was
static int tc_check_sweep(stb_tcounts_t *s, double a, const double *bpar, int nsweeps, const char *who) {
  if (!s) return stb_fail("%s: null object", who);
  if (!(a >= 0.0 && a < 1.0)) return stb_fail("%s: discount a=%g outside [0, 1)", who, a);
  if (!bpar) return stb_fail("%s: bpar is required", who);
  if (nsweeps < 0) return stb_fail("%s: nsweeps=%d", who, nsweeps);
  if (bpar == STB_BPAR_RESIDENT) return stb_hb_obj_resident(&s->hb, a, who);  // (what the object holds, by its lower bound)
  for (int i = 0; i < s->I; i++)
    if (!(bpar[i] > -a) || !std::isfinite(bpar[i])) return stb_fail("%s: bpar[%d]=%g (must be > -a = %g)", who, i, bpar[i], -a);
  return 0;
}

// what every sweep of the object needs queued before its kernel (on the object's device): the table for `a` and the
// concentrations bpar on the device
static int tc_stage(stb_tcounts_t *s, double a, const double *bpar, const char *who) {
  if (s->need_table && !(a == s->a_filled)) {  // (refilled only when the discount changes; the refill is checked: a wait)
    s->a_filled = NAN;
    if (stb_fill_S(&a, 1, s->N, s->M, s->d_table, s->tstride, s->d_S1, s->N, s->d_ws, s->ws_bytes, stb_default_variant(), s->st) ||
        stb_fill_status())
      return 1;
    s->a_filled = a;
  }
  return stb_hb_obj_stage(&s->hb, s->I, s->d_bpar, bpar, s->st, who);
}

namespace {
struct tc_copy {  // a device array on its way to the host (tc_fetch)
  void *dst;
  const void *src;
  size_t bytes;
};
}  // namespace

// device arrays to the host on the object's stream, then a wait (a null destination or an empty array is left out)
static int tc_fetch(stb_tcounts_t *s, std::initializer_list<tc_copy> copies, const char *who) {
  for (const tc_copy &c : copies)
    if (c.dst && c.bytes && hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  if (hipStreamSynchronize(s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// create and free

static void tc_release(stb_tcounts_t *s) {
  stb_hb_obj_release(&s->hb);
  void *dev[] = {s->d_koff, s->d_n, s->d_T, s->d_N, s->d_t, s->d_h, s->d_bpar, s->d_table, s->d_S1, s->d_ws};
  for (void *p : dev)
    if (p) (void)hipFree(p);
  if (s->st) (void)hipStreamDestroy(s->st);
  delete s;
}

static stb_tcounts_t *tc_create_here(int I, const int *K, const uint32_t *nflat, const uint16_t *tflat, const double *hflat,
                                     unsigned M) {
  const char *who = "stb_tcounts_create";
  if (stb_device_count() < 1) {
    stb_no_device("stb_tcounts_create");
    return nullptr;
  }
  if (I < 1 || !K || !nflat || !tflat) {
    stb_fail("stb_tcounts_create: I=%d and K, n, t are required", I);
    return nullptr;
  }
  std::vector<uint64_t> koff((size_t)I + 1, 0);
  for (int i = 0; i < I; i++) {
    if (K[i] < 0) {
      stb_fail("stb_tcounts_create: K[%d]=%d", i, K[i]);
      return nullptr;
    }
    koff[i + 1] = koff[i] + (uint64_t)K[i];
  }
  const uint64_t G = koff[I];
  unsigned maxn = 0;
  for (uint64_t g = 0; g < G; g++) maxn = nflat[g] > maxn ? nflat[g] : maxn;
  if (M == 0 && maxn > 65535u) {
    stb_fail("stb_tcounts_create: the largest n is %u; t is a uint16, so pass M <= 65535 (the draws are then from the "
             "conditional truncated at M)", maxn);
    return nullptr;
  }
  if (M == 0) M = maxn > 0 ? maxn : 1;
  if (M > 65535u) {
    stb_fail("stb_tcounts_create: M=%u (t is a uint16: at most 65535)", M);
    return nullptr;
  }
  std::vector<uint32_t> T(I, 0);
  for (int i = 0; i < I; i++)
    for (uint64_t g = koff[i]; g < koff[i + 1]; g++) {
      const unsigned n = nflat[g], t = tflat[g], tm = n < M ? n : M;
      if (n == 0 ? t != 0 : (t < 1 || t > tm)) {
        stb_fail("stb_tcounts_create: pair %llu has n=%u t=%u (t = 0 exactly when n = 0, else 1 <= t <= min(n, M=%u))",
                 (unsigned long long)g, n, t, M);
        return nullptr;
      }
      T[i] += t;
    }
  if (hflat && tc_check_h(hflat, G, who)) return nullptr;
  uint64_t sumn = 0;
  for (int i = 0; i < I; i++) {  // (N_i is a uint32, as sampleb's N[])
    uint64_t ni = 0;
    for (uint64_t g = koff[i]; g < koff[i + 1]; g++) ni += nflat[g];
    if (ni >= (1ull << 32)) {
      stb_fail("stb_tcounts_create: restaurant %d holds %llu customers (fewer than 2^32)", i, (unsigned long long)ni);
      return nullptr;
    }
    sumn += ni;
  }
  stb_tcounts_t *s = new stb_tcounts_t();
  s->I = I;
  s->G = G;
  s->maxn = maxn;
  s->sumn = sumn;
  s->N = maxn < 3 ? 3 : maxn;
  s->M = M;
  s->a_filled = NAN;
  s->need_table = (maxn < M ? maxn : M) >= 2;
  const size_t Gs = G ? G : 1;
  int rc = 0;
  if (hipGetDevice(&s->dev) != hipSuccess || hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc((void **)&s->d_koff, sizeof(uint64_t) * (I + 1)) != hipSuccess ||
      hipMalloc((void **)&s->d_n, sizeof(uint32_t) * Gs) != hipSuccess || hipMalloc((void **)&s->d_t, sizeof(uint16_t) * Gs) != hipSuccess ||
      hipMalloc((void **)&s->d_T, sizeof(uint32_t) * I) != hipSuccess || hipMalloc((void **)&s->d_bpar, sizeof(double) * I) != hipSuccess ||
      hipMalloc((void **)&s->d_N, sizeof(uint32_t) * I) != hipSuccess ||
      (hflat && hipMalloc((void **)&s->d_h, sizeof(double) * Gs) != hipSuccess))
    rc = STB_STREAM_FAIL(who);
  if (!rc) rc = stb_hb_obj_init(&s->hb, I, who);
  // (no table where no draw reads one: every pair has n <= 1, or M = 1)
  s->tstride = s->need_table ? (stb_table_elems(s->N, s->M) + 31) & ~31ull : 0;
  s->ws_bytes = s->need_table ? stb_fill_workspace_bytes(s->N, s->M, 1) : 0;
  if (!rc && s->need_table && (hipMalloc((void **)&s->d_table, sizeof(double) * s->tstride) != hipSuccess ||
              hipMalloc((void **)&s->d_S1, sizeof(double) * s->N) != hipSuccess || hipMalloc(&s->d_ws, s->ws_bytes ? s->ws_bytes : 1) != hipSuccess))
    rc = stb_fail("stb_tcounts_create: out of device memory for a %u x %u table", s->N, s->M);
  if (!rc && (hipMemcpy(s->d_koff, koff.data(), sizeof(uint64_t) * (I + 1), hipMemcpyHostToDevice) != hipSuccess ||
              (G && hipMemcpy(s->d_n, nflat, sizeof(uint32_t) * G, hipMemcpyHostToDevice) != hipSuccess) ||
              (G && hipMemcpy(s->d_t, tflat, sizeof(uint16_t) * G, hipMemcpyHostToDevice) != hipSuccess) ||
              hipMemcpy(s->d_T, T.data(), sizeof(uint32_t) * I, hipMemcpyHostToDevice) != hipSuccess ||
              (hflat && G && hipMemcpy(s->d_h, hflat, sizeof(double) * G, hipMemcpyHostToDevice) != hipSuccess)))
    rc = STB_STREAM_FAIL(who);
  // customers per restaurant: a segmented sum of n over the pair offsets, once (the b step reads it: stb_tcounts_sampleb)
  if (!rc) rc = stb_hq_segsum(s->d_koff, s->d_n, I, s->d_N, s->st);
  if (!rc && hipStreamSynchronize(s->st) != hipSuccess) rc = STB_STREAM_FAIL(who);
  if (rc) {
    tc_release(s);
    return nullptr;
  }
  return s;
}

// The object lives on the device stb_get_device() names, like a group set; every later call switches to it.
extern "C" stb_tcounts_t *stb_tcounts_create(int I, const int *K, const uint32_t *nflat, const uint16_t *tflat,
                                             const double *hflat, unsigned M) {
  STB_ENTRY;
  stb_device_scope dev(stb_get_device());
  return tc_create_here(I, K, nflat, tflat, hflat, M);
}

extern "C" void stb_tcounts_free(stb_tcounts_t *s) {
  STB_ENTRY;
  if (!s) return;
  stb_device_scope dev(s->dev);
  (void)hipStreamSynchronize(s->st);
  tc_release(s);
}

// ------------------------------------------------------------------------------------------------
// setters and getters

extern "C" int stb_tcounts_set_h(stb_tcounts_t *s, const double *hflat) {
  STB_ENTRY;
  const char *who = "stb_tcounts_set_h";
  if (!s) return stb_fail("%s: null object", who);
  if (hflat && tc_check_h(hflat, s->G, who)) return 1;
  stb_device_scope dev(s->dev);
  if (hipStreamSynchronize(s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  if (!hflat && s->d_h) {
    (void)hipFree(s->d_h);
    s->d_h = nullptr;
  } else if (hflat && s->G) {
    if (!s->d_h && hipMalloc((void **)&s->d_h, sizeof(double) * s->G) != hipSuccess) return stb_fail("%s: out of device memory", who);
    if (hipMemcpy(s->d_h, hflat, sizeof(double) * s->G, hipMemcpyHostToDevice) != hipSuccess) return STB_STREAM_FAIL(who);
  }
  return 0;
}

extern "C" int stb_tcounts_set_bpar(stb_tcounts_t *s, const double *bpar) {
  STB_ENTRY;
  const char *who = "stb_tcounts_set_bpar";
  if (!s) return stb_fail("%s: null object", who);
  if (!bpar || bpar == STB_BPAR_RESIDENT) return stb_fail("%s: bpar (host, I values) is required", who);
  for (int i = 0; i < s->I; i++)
    if (!std::isfinite(bpar[i])) return stb_fail("%s: bpar[%d]=%g (must be finite)", who, i, bpar[i]);
  stb_device_scope dev(s->dev);
  return stb_hb_obj_stage(&s->hb, s->I, s->d_bpar, bpar, s->st, who);
}

extern "C" int stb_tcounts_get_bpar(stb_tcounts_t *s, double *bpar_out) {
  STB_ENTRY;
  const char *who = "stb_tcounts_get_bpar";
  if (!s || !bpar_out) return stb_fail("%s: null %s", who, s ? "output" : "object");
  if (!s->hb.resident) return stb_fail("%s: the object holds no concentrations yet", who);
  stb_device_scope dev(s->dev);
  return tc_fetch(s, {{bpar_out, s->d_bpar, sizeof(double) * s->I}}, who);
}

extern "C" int stb_tcounts_get(stb_tcounts_t *s, uint16_t *t_out, uint32_t *T_out) {
  STB_ENTRY;
  if (!s) return stb_fail("stb_tcounts_get: null object");
  stb_device_scope dev(s->dev);
  return tc_fetch(s, {{t_out, s->d_t, sizeof(uint16_t) * s->G}, {T_out, s->d_T, sizeof(uint32_t) * s->I}}, "stb_tcounts_get");
}

// the pairs and T to a group set of the same shape, device to device (stb_groups_take_counts, groups.hip)
extern "C" int stb_tcounts_to_groups(stb_tcounts_t *s, stb_groups_t *g, const double *bpar) {
  STB_ENTRY;
  if (!s || !g) return stb_fail("stb_tcounts_to_groups: null object");
  const stb_counts_view v = {s->dev, s->I, s->G, s->maxn, s->M, s->d_n, s->d_T, s->d_t, s->d_bpar, s->hb.resident, s->st, "counts"};
  stb_device_scope dev(s->dev);
  return stb_groups_take_counts(g, v, bpar, "stb_tcounts_to_groups");
}

// ------------------------------------------------------------------------------------------------
// the sweeps, and the steps for a and b on the object's counts (hyperb.hip, hyperq.hip, hyperj.hip)

extern "C" int stb_tcounts_sweep(stb_tcounts_t *s, double a, const double *bpar, uint64_t seed, uint64_t sweep, int nsweeps) {
  STB_ENTRY;
  const char *who = "stb_tcounts_sweep";
  if (tc_check_sweep(s, a, bpar, nsweeps, who)) return 1;
  if (nsweeps == 0) return 0;
  stb_device_scope dev(s->dev);
  if (tc_stage(s, a, bpar, who)) return 1;
  return stb_tc_launch(tc_table(s), tc_rest(s, a), tc_counts(s), {seed, sweep}, nsweeps, s->maxn < s->M ? s->maxn : s->M, s->st);
}

// the windowed sweep (tcwin.hip) on the same object: the same table, concentrations, stream and checks
extern "C" int stb_tcounts_sweep_window(stb_tcounts_t *s, double a, const double *bpar, unsigned W, unsigned flags,
                                        uint64_t seed, uint64_t sweep, int nsweeps) {
  STB_ENTRY;
  const char *who = "stb_tcounts_sweep_window";
  if (W == 0) return stb_fail("%s: window W=0 (must be >= 1)", who);
  if (flags & ~STB_TC_REF_WINDOW_FLAG) return stb_fail("%s: unknown flags 0x%x", who, flags);
  if (tc_check_sweep(s, a, bpar, nsweeps, who)) return 1;
  if (nsweeps == 0) return 0;
  stb_device_scope dev(s->dev);
  if (tc_stage(s, a, bpar, who)) return 1;
  return stb_tcw_launch(tc_table(s), tc_rest(s, a), tc_counts(s), W, flags, {seed, sweep}, nsweeps, s->st);
}

extern "C" int stb_tcounts_set_bgroups(stb_tcounts_t *s, int G, const uint64_t *goff_host) {
  STB_ENTRY;
  if (!s) return stb_fail("stb_tcounts_set_bgroups: null object");
  stb_device_scope dev(s->dev);
  return stb_hb_obj_set_groups(&s->hb, s->I, G, goff_host, s->st, "stb_tcounts_set_bgroups");
}

// the per-group concentration step (hyperb.hip) on the object's T, N and concentrations, queued behind its sweeps
extern "C" int stb_tcounts_sampleb_groups(stb_tcounts_t *s, double a, double shape, double scale, uint64_t seed, uint64_t sweep,
                                          double *bgrp_host, stb_bgroups_info_t *info) {
  STB_ENTRY;
  if (!s) return stb_fail("stb_tcounts_sampleb_groups: null object");
  stb_device_scope dev(s->dev);
  return stb_hb_obj_step(&s->hb, a, shape, scale, s->I, s->d_N, nullptr, s->d_T, s->d_bpar, seed, sweep, s->st, bgrp_host, info,
                         "stb_tcounts_sampleb_groups");
}

// the concentration step on the object's counts (hyperq.hip, sampleb.c): Q from N on the device, T read in place, queued
// behind the object's sweeps; the call waits for Q and for the sampler's evaluations only.  t and T are not written.
extern "C" double stb_tcounts_sampleb(stb_tcounts_t *s, double b_in, double shape, double scale, double a, void *rng, int loops,
                                      int verbose, uint64_t seed, uint64_t sweep) {
  // (no rand() guard across the call: ARMS draws from the caller's rand() stream, as in sampleb)
  if (!s) {
    stb_fail("stb_tcounts_sampleb: null object");
    return NAN;
  }
  stb_device_scope dev(s->dev);
  return stb_sampleb_device_ex(b_in, s->I, shape, scale, s->d_N, nullptr, s->d_T, a, rng, loops, verbose, seed, sweep, s->st,
                               "stb_tcounts_sampleb");
}

// the joint step for a and b on the object's counts (hyperj.hip): the pairs and T to the set, device to device, then the
// step with the object's N, queued behind its sweeps.  Nothing per restaurant crosses to the host; t and T are not written.
extern "C" int stb_tcounts_samplejoint(stb_tcounts_t *s, stb_groups_t *g, const stb_joint_opts_t *opts, double a_in, double b_in,
                                   double *a_out, double *b_out, stb_joint_info_t *info) {
  if (!s || !g) return stb_fail("stb_tcounts_samplejoint: null object");
  if (stb_tcounts_to_groups(s, g, nullptr)) return 1;
  return stb_hj_samplejoint(g, s->d_N, nullptr, opts, a_in, b_in, a_out, b_out, info, "stb_tcounts_samplejoint");
}

// ------------------------------------------------------------------------------------------------
// the S-free discount step's first stage and the log joint, on the object's pairs

// stage 1 of the S-free discount step (partition.hip) on the object's pairs: the table-size histogram into h, T and bpar
// to h, all on the device, queued behind the object's earlier work; h's later work waits for it
extern "C" int stb_tcounts_partition(stb_tcounts_t *s, double a, stb_hist_t *h, const double *bpar, uint64_t seed,
                                     uint64_t sweep) {
  STB_ENTRY;
  const char *who = "stb_tcounts_partition";
  if (tc_check_sweep(s, a, bpar, 0, who)) return 1;
  stb_hist_view v;
  if (!h || stb_hist_view_of(h, &v)) return stb_fail("%s: null histogram", who);
  if (v.dev != s->dev) return stb_fail("%s: the histogram is on device %d, the counts on %d", who, v.dev, s->dev);
  if (v.I != s->I) return stb_fail("%s: the histogram has I=%d, the counts I=%d", who, v.I, s->I);
  if (v.S <= s->maxn) return stb_fail("%s: histogram length S=%u (must exceed the largest n, %u)", who, v.S, s->maxn);
  if (s->sumn >= (1ull << 32))
    return stb_fail("%s: the pairs hold %llu customers (the bins are uint32: fewer than 2^32)", who,
                    (unsigned long long)s->sumn);
  if (stb_pt_check(a, s->N, s->M, s->G, v.S, 0u, who)) return 1;
  stb_device_scope dev(s->dev);
  if (tc_stage(s, a, bpar, who)) return 1;
  stb_event_owner ev;
  if (hipEventCreateWithFlags(&ev.ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(ev.ev, v.st) != hipSuccess ||
      hipStreamWaitEvent(s->st, ev.ev, 0) != hipSuccess)
    return STB_STREAM_FAIL(who);
  if (stb_pt_launch(tc_table(s), a, s->G, tc_counts(s), v.d_cnt, v.S, 0u, {seed, sweep}, s->st)) return 1;
  if (hipMemcpyAsync(v.d_T, s->d_T, sizeof(uint32_t) * s->I, hipMemcpyDeviceToDevice, s->st) != hipSuccess ||
      hipMemcpyAsync(v.d_bpar, s->d_bpar, sizeof(double) * s->I, hipMemcpyDeviceToDevice, s->st) != hipSuccess ||
      hipEventRecord(ev.ev, s->st) != hipSuccess || hipStreamWaitEvent(v.st, ev.ev, 0) != hipSuccess)
    return STB_STREAM_FAIL(who);
  return 0;
}

// the log joint of the object's state (logjoint.hip) from its own S table, queued behind its sweeps; t and T are not
// written.  Objects without a table read none: S^n_1 (M = 1) is evaluated in place, as the fill would.
extern "C" int stb_tcounts_logjoint(stb_tcounts_t *s, double a, const double *bpar, unsigned flags, double *total,
                                    double *Li_host, stb_logjoint_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_tcounts_logjoint";
  if (!s) return stb_fail("%s: null object", who);
  if (stb_lj_check(a, flags, s->I, who)) return 1;
  if (!total) return stb_fail("%s: total is required", who);
  if (tc_check_sweep(s, a, bpar, 0, who)) return 1;
  stb_device_scope dev(s->dev);
  if (tc_stage(s, a, bpar, who)) return 1;
  stb_pool_scratch sc(s->st);
  double *d_Li = nullptr;
  if (Li_host && sc.take(&d_Li, sizeof(double) * (size_t)s->I) != hipSuccess)
    return stb_fail("%s: out of device memory for %d values", who, s->I);
  // (a run that succeeded has waited for its own answer: the buffer goes back without a second wait)
  return sc.last(stb_lj_run(tc_table(s), tc_rest(s, a), tc_counts(s), flags, d_Li, Li_host, total, info, s->st, who));
}
