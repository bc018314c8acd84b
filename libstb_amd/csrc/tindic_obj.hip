// tindic_obj.hip -- the table-indicator object (stb_tindic_t) and every stb_tindic_* entry point: the pairs, totals, weights
// and customer order of a set of restaurants on one device, with a V table for the current discount and a stream of its
// own.  The host side only: the sweep kernels are tindic.hip's and tdish.hip's, the other steps' kernels live in the files
// the sections below name.

#include <algorithm>
#include <initializer_list>
#include <vector>

#include "stb_common.h"
#include "pool_scratch.h"
#include "groups.h"
#include "hyperq.h"
#include "hyperb.h"
#include "hyperj.h"
#include "logjoint.h"
#include "tindic.h"
#include "tlik.h"
#include "predict.h"
#include "seat.h"
#include "seat_pf.h"
#include "seat_ais.h"
#include "hgroups.h"
#include "htree.h"
#include "dirmult.h"
#include "dirconc.h"
#include "classgen.h"
#include "gauss.h"

// ------------------------------------------------------------------------------------------------
// the object: pairs, totals, weights, customer order, its own V table for the current discount, its own stream

struct stb_tindic {
  int dev;
  int I;
  uint64_t G, C;        // pairs, customers
  unsigned N, M;        // table bounds: N = the largest n (at least 3), M = min(the column bound, N)
  unsigned Mdraw;       // the column bound the draws are truncated at (what create was given, or the largest n)
  unsigned maxn, maxK;
  unsigned flags;
  // the dish sweep (tdish.hip)
  unsigned Mgiven;      // the column bound create was given (0: the largest n)
  uint64_t maxNi;       // the largest restaurant's customers: what one pair's n can reach
  bool dish_ready;      // pair order materialised, bounds grown to maxNi
  uint32_t *d_cls;      // [C] likelihood classes (null: none set)
  unsigned cls_rows;
  double *d_lik;        // [lik_rows x lik_stride] (null: every L is 1)
  unsigned lik_rows, lik_stride;
  bool lik_bad, h_bad;  // a draw of stb_tindic_sample_lik / _sample_gauss / _sample_h failed: the matrix / h is undefined, dish sweeps are refused
  // Gaussian observations (gauss.hip).  d_x set: observation mode -- the classes are the identity, the matrix has a row per
  // customer and is written by the object from (mu, tau)
  double *d_x;          // [C x obs_D] (null: none)
  unsigned obs_D;
  double *d_gpar;       // mu, tau [maxK x obs_D each], then the statistics' mean and Q [maxK x obs_D each]
  uint32_t *d_gn;       // [maxK] the statistics' counts
  bool g_have;          // mu and tau hold values (stb_tindic_set_gauss, or a stb_tindic_sample_gauss that succeeded)
  // the observation held-out set (stb_tindic_set_heldout_obs): storage of its own, apart from d_hoff / d_hcls / d_pacc
  uint64_t *d_ghoff;    // [I + 1] (null: no set)
  double *d_gy;         // [gHc x obs_D]
  double *d_gacc;       // M [gHc], then A [gHc]: the log-domain accumulator pairs
  uint64_t gHc;
  unsigned gsamples;    // states accumulated
  unsigned long long *d_info, *h_info;  // {skipped, stuck} on the device, and pinned
  void *d_cgs;          // the class draw's scratch (classgen.hip), from the buffer cache: kept while the matrix keeps its shape
  size_t cgs_bytes;
  uint64_t *d_cginfo;   // {skipped, stuck, drawn} of the class draw, and the seating's three words behind them
  bool need_table;      // some visit can read a V cell (max n >= 2 and M >= 2); otherwise no indicator is ever added
  uint64_t *d_koff, *d_coff;
  uint32_t *d_n, *d_T;
  uint32_t *d_cust;     // null: pair order
  uint16_t *d_t;
  double *d_h;          // null: every h is 1
  double *d_bpar;
  stb_hb_obj hb;        // d_bpar's staging and what it holds; the per-group concentration step's ranges, L, Y (hyperb.hip)
  // the per-group base weights (hgroups.hip): the ranges, the root and the concentration live with the object
  int hg_G;             // ranges (0: every restaurant its own group)
  uint64_t *d_hgoff;    // [hg_G + 1], or null
  double *d_hroot;      // [maxK] (null: 1/maxK each)
  double hg_alpha;      // what the last successful step left (NaN: none yet)
  // the tree of nested groups (htree.hip): its ranges, every level's rows and the concentrations live with the object
  int ht_L;                        // levels (0: no tree)
  int ht_G[STB_HT_MAXL];           // nodes of every level
  uint64_t *d_htoff[STB_HT_MAXL];  // [ht_G[l] + 1]
  double *d_htnode[STB_HT_MAXL];   // [ht_G[l] x maxK]; level 1's are what the last step drew
  double ht_alpha[STB_HT_MAXL];    // what the last successful step left
  bool ht_have_alpha, ht_have_rows1;
  double *d_vt;
  uint64_t vstride;
  void *d_ws;
  size_t ws_bytes;
  double a_filled;      // the discount the table holds (NaN: none yet)
  // the S slab of stb_tindic_logjoint (bounds N, M as the V table's): from the buffer cache on first use
  double *d_stab, *d_sS1;
  uint64_t sstride;
  void *d_sws;
  size_t sws_bytes;
  double a_sfilled;     // the discount the S slab holds (NaN: none yet)
  // held-out customers (predict.hip): CSR over the restaurants, their classes, and the accumulator of p over states
  uint64_t *d_hoff;     // [I + 1] (null: no held-out set)
  uint32_t *d_hcls;     // [Hc]
  double *d_pacc;       // [Hc] sum over the accumulated states of p_c
  uint64_t Hc;
  unsigned hcls_max;    // the largest held-out class (0 when Hc = 0)
  unsigned hsamples;    // states accumulated
  uint64_t hmaxNi;      // the largest held-out N_i
  // the V table of stb_tindic_heldout_ais (seat_ais.hip): bounds from the held-out customers, not from the object's own
  double *d_avt;
  void *d_aws;
  uint64_t avstride;
  size_t aws_bytes;
  unsigned aN, aM;
  double a_afilled;     // the discount it holds (NaN: none yet)
  hipStream_t st;
};

// ---- the steps the entry points share

static int ti_check_h(const double *h, uint64_t G, const char *who) {
  for (uint64_t g = 0; g < G; g++)
    if (!(h[g] > 0.0) || !std::isfinite(h[g])) return stb_fail("%s: h[%llu]=%g (must be > 0 and finite)", who, (unsigned long long)g, h[g]);
  return 0;
}

// concentrations for discount a: the object's own (STB_BPAR_RESIDENT, by their lower bound) or I host values, each > -a
static int ti_check_bpar(stb_tindic_t *s, double a, const double *bpar, const char *who) {
  if (bpar == STB_BPAR_RESIDENT) return stb_hb_obj_resident(&s->hb, a, who);
  for (int i = 0; i < s->I; i++)
    if (!(bpar[i] > -a) || !std::isfinite(bpar[i])) return stb_fail("%s: bpar[%d]=%g (must be > -a = %g)", who, i, bpar[i], -a);
  return 0;
}

// the refusal of a call that reads the matrix's rows as classes, or depends on a row's scale, in observation mode
static int ti_not_obs(const stb_tindic_t *s, const char *who) {
  if (!s->d_x) return 0;
  return stb_fail("%s: the object holds Gaussian observations (stb_tindic_set_obs): its matrix has one row per customer, each "
                  "scaled by its own maximum, and its classes are the customers' indices", who);
}

// the observation held-out set, freed (the caller has waited for whatever reads it)
static void ti_drop_gh(stb_tindic_t *s) {
  void *dev[] = {s->d_ghoff, s->d_gy, s->d_gacc};
  for (void *p : dev)
    if (p) (void)hipFree(p);
  s->d_ghoff = nullptr;
  s->d_gy = s->d_gacc = nullptr;
  s->gHc = 0;
  s->gsamples = 0;
}

// the observations and what goes with them, freed (the caller has waited for whatever reads them)
static void ti_drop_obs(stb_tindic_t *s) {
  ti_drop_gh(s);
  void *dev[] = {s->d_x, s->d_gpar, s->d_gn};
  for (void *p : dev)
    if (p) (void)hipFree(p);
  s->d_x = s->d_gpar = nullptr;
  s->d_gn = nullptr;
  s->obs_D = 0;
  s->g_have = false;
}

namespace {  // (the helper types are this file's own: no symbols of theirs leave it)

struct ti_bounds {  // what ti_table_bounds returns: the object's fields of these names
  unsigned N, Mdraw;
  bool need_table;
  unsigned M;
};

// a device array on its way to the host (ti_fetch)
struct ti_copy {
  void *dst;
  const void *src;
  size_t bytes;
};

}  // namespace

// table bounds from the largest n a pair can reach and the column bound create was given (0: the largest n)
static ti_bounds ti_table_bounds(unsigned maxn, unsigned Mgiven) {
  ti_bounds b;
  b.N = maxn < 3 ? 3 : maxn;
  b.Mdraw = Mgiven ? Mgiven : (maxn > 0 ? maxn : 1);
  b.need_table = maxn >= 2 && b.Mdraw >= 2;
  // (the draws never address m > max n: a table of min(M, N) columns is the same table)
  b.M = b.need_table ? (b.Mdraw < b.N ? b.Mdraw : b.N) : b.Mdraw;
  return b;
}

// ---- the object's state as the launches take it (views.h).  Customers: the object's own (lik false: without their classes,
// for a launch under no matrix), the held-out ones.  Tables: the sweeps' V, the log joint's S, the anneal ladder's V
static stb_rest_view ti_rest(const stb_tindic_t *s, double a, bool with_h = true) {
  return {a, s->d_bpar, s->I, s->d_koff, with_h ? s->d_h : nullptr, s->maxK, s->G};
}
static stb_cnts_rw ti_counts(const stb_tindic_t *s) { return {s->d_n, s->d_t, s->d_T}; }
static stb_lik_view ti_matrix(const stb_tindic_t *s) { return {s->d_lik, s->lik_rows, s->lik_stride}; }
static stb_cust_rw ti_customers(const stb_tindic_t *s, bool lik = true) { return {s->d_coff, lik ? s->d_cls : nullptr, s->d_cust, s->C}; }
static stb_cust_rw ti_heldout(const stb_tindic_t *s) { return {s->d_hoff, s->d_hcls, nullptr, s->Hc}; }
static stb_table_view ti_vtable(const stb_tindic_t *s) { return {s->d_vt, s->N, s->need_table ? s->M : s->Mdraw}; }
static stb_table_view ti_stable(const stb_tindic_t *s) { return {s->d_stab, s->N, s->need_table ? s->M : s->Mdraw, s->d_sS1}; }
static stb_table_view ti_atable(const stb_tindic_t *s, const ti_bounds &tb) { return {tb.need_table ? s->d_avt : nullptr, tb.N, tb.M}; }

// the S slab back to the buffer cache (the caller has waited for whatever reads it)
static void ti_drop_sslab(stb_tindic_t *s) {
  void *pooled[] = {s->d_stab, s->d_sS1, s->d_sws};
  for (void *p : pooled)
    if (p) stb_pool_free(p);
  s->d_stab = s->d_sS1 = nullptr;
  s->d_sws = nullptr;
  s->a_sfilled = NAN;
}

// device arrays to the host on the object's stream, then a wait (a null destination or an empty array is left out)
static int ti_fetch(stb_tindic_t *s, std::initializer_list<ti_copy> copies, const char *who) {
  for (const ti_copy &c : copies)
    if (c.dst && c.bytes && hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  if (hipStreamSynchronize(s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// create and free

// the class draw's scratch back to the buffer cache (the caller has waited for whatever uses it)
static void ti_drop_cgs(stb_tindic_t *s) {
  if (s->d_cgs) stb_pool_free(s->d_cgs);
  s->d_cgs = nullptr;
  s->cgs_bytes = 0;
}

static void ti_release(stb_tindic_t *s) {
  stb_hb_obj_release(&s->hb);
  ti_drop_sslab(s);
  ti_drop_cgs(s);
  ti_drop_obs(s);
  void *dev[] = {s->d_koff, s->d_coff, s->d_n, s->d_T, s->d_cust, s->d_t, s->d_h, s->d_bpar, s->d_vt, s->d_ws,
                 s->d_cls, s->d_lik, s->d_info, s->d_hoff, s->d_hcls, s->d_pacc, s->d_hgoff, s->d_hroot, s->d_cginfo,
                 s->d_avt, s->d_aws};
  for (void *p : dev)
    if (p) (void)hipFree(p);
  for (int l = 0; l < STB_HT_MAXL; l++) {
    if (s->d_htoff[l]) (void)hipFree(s->d_htoff[l]);
    if (s->d_htnode[l]) (void)hipFree(s->d_htnode[l]);
  }
  if (s->h_info) (void)hipHostFree(s->h_info);
  if (s->st) (void)hipStreamDestroy(s->st);
  delete s;
}

static stb_tindic_t *ti_create_here(int I, const int *K, const uint32_t *nflat, const uint16_t *tflat, const double *hflat,
                                    const uint32_t *cust, unsigned Mgiven, unsigned flags) {
  if (stb_device_count() < 1) {
    stb_no_device("stb_tindic_create");
    return nullptr;
  }
  if (I < 1 || !K || !nflat || !tflat) {
    stb_fail("stb_tindic_create: I=%d and K, n, t are required", I);
    return nullptr;
  }
  if (flags & ~STB_TI_REF_ODDS_FLAG) {
    stb_fail("stb_tindic_create: unknown flags 0x%x", flags);
    return nullptr;
  }
  std::vector<uint64_t> koff((size_t)I + 1, 0), coff((size_t)I + 1, 0);
  unsigned maxK = 0;
  for (int i = 0; i < I; i++) {
    if (K[i] < 0) {
      stb_fail("stb_tindic_create: K[%d]=%d", i, K[i]);
      return nullptr;
    }
    koff[i + 1] = koff[i] + (uint64_t)K[i];
    maxK = (unsigned)K[i] > maxK ? (unsigned)K[i] : maxK;
  }
  const uint64_t G = koff[I];
  unsigned maxn = 0;
  for (uint64_t g = 0; g < G; g++) maxn = nflat[g] > maxn ? nflat[g] : maxn;
  if (Mgiven == 0 && maxn > 65535u) {
    stb_fail("stb_tindic_create: the largest n is %u; t is a uint16, so pass M <= 65535 (the draws are then truncated "
             "at M)", maxn);
    return nullptr;
  }
  const ti_bounds tb = ti_table_bounds(maxn, Mgiven);
  const unsigned M = tb.Mdraw;
  if (M > 65535u) {
    stb_fail("stb_tindic_create: M=%u (t is a uint16: at most 65535)", M);
    return nullptr;
  }
  uint64_t maxNi = 0;
  std::vector<uint32_t> T(I, 0);
  for (int i = 0; i < I; i++) {
    uint64_t ci = 0;
    for (uint64_t g = koff[i]; g < koff[i + 1]; g++) {
      const unsigned n = nflat[g], t = tflat[g], tm = n < M ? n : M;
      if (n == 0 ? t != 0 : (t < 1 || t > tm)) {
        stb_fail("stb_tindic_create: pair %llu has n=%u t=%u (t = 0 exactly when n = 0, else 1 <= t <= min(n, M=%u))",
                 (unsigned long long)g, n, t, M);
        return nullptr;
      }
      T[i] += t;
      ci += n;
    }
    coff[i + 1] = coff[i] + ci;
    maxNi = ci > maxNi ? ci : maxNi;
  }
  const uint64_t C = coff[I];
  if (hflat && ti_check_h(hflat, G, "stb_tindic_create")) return nullptr;
  if (cust) {  // every restaurant's sequence visits pair k exactly n_k times
    std::vector<uint64_t> seen(maxK ? maxK : 1);
    for (int i = 0; i < I; i++) {
      const unsigned Ki = (unsigned)K[i];
      std::fill(seen.begin(), seen.begin() + Ki, 0);
      for (uint64_t c = coff[i]; c < coff[i + 1]; c++) {
        if (cust[c] >= Ki) {
          stb_fail("stb_tindic_create: cust[%llu]=%u is not a pair of restaurant %d (K=%u)", (unsigned long long)c, cust[c], i, Ki);
          return nullptr;
        }
        seen[cust[c]]++;
      }
      for (unsigned k = 0; k < Ki; k++)
        if (seen[k] != nflat[koff[i] + k]) {
          stb_fail("stb_tindic_create: restaurant %d visits pair %u %llu times; its n is %u", i, k,
                   (unsigned long long)seen[k], nflat[koff[i] + k]);
          return nullptr;
        }
    }
  }
  stb_tindic_t *s = new stb_tindic_t();
  s->I = I;
  s->G = G;
  s->C = C;
  s->maxn = maxn;
  s->maxK = maxK;
  s->flags = flags;
  s->Mgiven = Mgiven;
  s->maxNi = maxNi;
  s->N = tb.N;
  s->Mdraw = tb.Mdraw;
  s->need_table = tb.need_table;
  s->M = tb.M;
  s->a_filled = NAN;
  s->a_sfilled = NAN;
  s->a_afilled = NAN;
  s->hg_alpha = NAN;
  const size_t Gs = G ? G : 1;
  int rc = 0;
  if (hipGetDevice(&s->dev) != hipSuccess || hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc((void **)&s->d_koff, sizeof(uint64_t) * (I + 1)) != hipSuccess ||
      hipMalloc((void **)&s->d_coff, sizeof(uint64_t) * (I + 1)) != hipSuccess ||
      hipMalloc((void **)&s->d_n, sizeof(uint32_t) * Gs) != hipSuccess || hipMalloc((void **)&s->d_t, sizeof(uint16_t) * Gs) != hipSuccess ||
      hipMalloc((void **)&s->d_T, sizeof(uint32_t) * I) != hipSuccess || hipMalloc((void **)&s->d_bpar, sizeof(double) * I) != hipSuccess ||
      (hflat && hipMalloc((void **)&s->d_h, sizeof(double) * Gs) != hipSuccess) ||
      (cust && hipMalloc((void **)&s->d_cust, sizeof(uint32_t) * (C ? C : 1)) != hipSuccess))
    rc = STB_STREAM_FAIL("stb_tindic_create");
  if (!rc) rc = stb_hb_obj_init(&s->hb, I, "stb_tindic_create");
  // (no table where no visit reads one: every pair has n <= 1, or M = 1)
  s->vstride = s->need_table ? (stb_vtable_elems(s->N, s->M) + 31) & ~31ull : 0;
  s->ws_bytes = s->need_table ? stb_fill_workspace_bytes(s->N, s->M, 1) : 0;
  if (!rc && s->need_table && (hipMalloc((void **)&s->d_vt, sizeof(double) * s->vstride) != hipSuccess ||
                               hipMalloc(&s->d_ws, s->ws_bytes ? s->ws_bytes : 1) != hipSuccess))
    rc = stb_fail("stb_tindic_create: out of device memory for a %u x %u V table", s->N, s->M);
  if (!rc && (hipMemcpy(s->d_koff, koff.data(), sizeof(uint64_t) * (I + 1), hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(s->d_coff, coff.data(), sizeof(uint64_t) * (I + 1), hipMemcpyHostToDevice) != hipSuccess ||
              (G && hipMemcpy(s->d_n, nflat, sizeof(uint32_t) * G, hipMemcpyHostToDevice) != hipSuccess) ||
              (G && hipMemcpy(s->d_t, tflat, sizeof(uint16_t) * G, hipMemcpyHostToDevice) != hipSuccess) ||
              hipMemcpy(s->d_T, T.data(), sizeof(uint32_t) * I, hipMemcpyHostToDevice) != hipSuccess ||
              (hflat && G && hipMemcpy(s->d_h, hflat, sizeof(double) * G, hipMemcpyHostToDevice) != hipSuccess) ||
              (cust && C && hipMemcpy(s->d_cust, cust, sizeof(uint32_t) * C, hipMemcpyHostToDevice) != hipSuccess)))
    rc = STB_STREAM_FAIL("stb_tindic_create");
  if (rc) {
    ti_release(s);
    return nullptr;
  }
  return s;
}

// The object lives on the device stb_get_device() names, like a group set; every later call switches to it.
extern "C" stb_tindic_t *stb_tindic_create(int I, const int *K, const uint32_t *nflat, const uint16_t *tflat, const double *hflat,
                                           const uint32_t *cust, unsigned M, unsigned flags) {
  STB_ENTRY;
  stb_device_scope dev(stb_get_device());
  return ti_create_here(I, K, nflat, tflat, hflat, cust, M, flags);
}

extern "C" void stb_tindic_free(stb_tindic_t *s) {
  STB_ENTRY;
  if (!s) return;
  stb_device_scope dev(s->dev);
  (void)hipStreamSynchronize(s->st);
  ti_release(s);
}

// ------------------------------------------------------------------------------------------------
// setters and getters

extern "C" int stb_tindic_set_h(stb_tindic_t *s, const double *hflat) {
  STB_ENTRY;
  const char *who = "stb_tindic_set_h";
  if (!s) return stb_fail("%s: null object", who);
  if (hflat && ti_check_h(hflat, s->G, who)) return 1;
  stb_device_scope dev(s->dev);
  if (hipStreamSynchronize(s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  if (!hflat && s->d_h) {
    (void)hipFree(s->d_h);
    s->d_h = nullptr;
  } else if (hflat && s->G) {
    if (!s->d_h && hipMalloc((void **)&s->d_h, sizeof(double) * s->G) != hipSuccess) return stb_fail("%s: out of device memory", who);
    if (hipMemcpy(s->d_h, hflat, sizeof(double) * s->G, hipMemcpyHostToDevice) != hipSuccess) return STB_STREAM_FAIL(who);
  }
  s->h_bad = false;
  return 0;
}

extern "C" int stb_tindic_get_h(stb_tindic_t *s, double *h_out) {
  STB_ENTRY;
  const char *who = "stb_tindic_get_h";
  if (!s || !h_out) return stb_fail("%s: null %s", who, s ? "h_out" : "object");
  if (!s->d_h) {
    for (uint64_t g = 0; g < s->G; g++) h_out[g] = 1.0;
    return 0;
  }
  stb_device_scope dev(s->dev);
  return ti_fetch(s, {{h_out, s->d_h, sizeof(double) * s->G}}, who);
}

extern "C" int stb_tindic_set_bpar(stb_tindic_t *s, const double *bpar) {
  STB_ENTRY;
  const char *who = "stb_tindic_set_bpar";
  if (!s) return stb_fail("%s: null object", who);
  if (!bpar || bpar == STB_BPAR_RESIDENT) return stb_fail("%s: bpar (host, I values) is required", who);
  for (int i = 0; i < s->I; i++)
    if (!std::isfinite(bpar[i])) return stb_fail("%s: bpar[%d]=%g (must be finite)", who, i, bpar[i]);
  stb_device_scope dev(s->dev);
  return stb_hb_obj_stage(&s->hb, s->I, s->d_bpar, bpar, s->st, who);
}

extern "C" int stb_tindic_get_bpar(stb_tindic_t *s, double *bpar_out) {
  STB_ENTRY;
  const char *who = "stb_tindic_get_bpar";
  if (!s || !bpar_out) return stb_fail("%s: null %s", who, s ? "output" : "object");
  if (!s->hb.resident) return stb_fail("%s: the object holds no concentrations yet", who);
  stb_device_scope dev(s->dev);
  return ti_fetch(s, {{bpar_out, s->d_bpar, sizeof(double) * s->I}}, who);
}

extern "C" int stb_tindic_get(stb_tindic_t *s, uint16_t *t_out, uint32_t *T_out) {
  STB_ENTRY;
  if (!s) return stb_fail("stb_tindic_get: null object");
  stb_device_scope dev(s->dev);
  return ti_fetch(s, {{t_out, s->d_t, sizeof(uint16_t) * s->G}, {T_out, s->d_T, sizeof(uint32_t) * s->I}}, "stb_tindic_get");
}

// the pairs and T to a group set of the same shape, device to device (stb_groups_take_counts, groups.hip)
extern "C" int stb_tindic_to_groups(stb_tindic_t *s, stb_groups_t *g, const double *bpar) {
  STB_ENTRY;
  if (!s || !g) return stb_fail("stb_tindic_to_groups: null object");
  const stb_counts_view v = {s->dev, s->I, s->G, s->maxn, s->Mdraw, s->d_n, s->d_T, s->d_t, s->d_bpar, s->hb.resident, s->st, "indicators"};
  stb_device_scope dev(s->dev);
  return stb_groups_take_counts(g, v, bpar, "stb_tindic_to_groups");
}

// ------------------------------------------------------------------------------------------------
// the indicator sweep, and the steps for a and b on the object's counts (hyperb.hip, hyperq.hip, hyperj.hip)

// the V table for discount a (refilled only when the discount changes; the refill is checked: a wait)
static int ti_ensure_V(stb_tindic_t *s, double a) {
  if (!s->need_table || a == s->a_filled) return 0;
  s->a_filled = NAN;
  if (stb_fill_V(&a, 1, s->N, s->M, s->d_vt, s->vstride, s->d_ws, s->ws_bytes, s->st) || stb_fill_status()) return 1;
  s->a_filled = a;
  return 0;
}

extern "C" int stb_tindic_sweep(stb_tindic_t *s, double a, const double *bpar, uint64_t seed, uint64_t sweep, int nsweeps) {
  STB_ENTRY;
  const char *who = "stb_tindic_sweep";
  if (!s) return stb_fail("%s: null object", who);
  if (!(a >= 0.0 && a < 1.0)) return stb_fail("%s: discount a=%g outside [0, 1)", who, a);
  if (!bpar) return stb_fail("%s: bpar is required", who);
  if (nsweeps < 0) return stb_fail("%s: nsweeps=%d", who, nsweeps);
  if (ti_check_bpar(s, a, bpar, who)) return 1;
  if (nsweeps == 0) return 0;
  stb_device_scope dev(s->dev);
  if (ti_ensure_V(s, a) || stb_hb_obj_stage(&s->hb, s->I, s->d_bpar, bpar, s->st, who)) return 1;
  return stb_ti_launch(ti_vtable(s), ti_rest(s, a), ti_counts(s), ti_customers(s), s->flags, {seed, sweep}, nsweeps, s->st);
}

extern "C" int stb_tindic_set_bgroups(stb_tindic_t *s, int G, const uint64_t *goff_host) {
  STB_ENTRY;
  if (!s) return stb_fail("stb_tindic_set_bgroups: null object");
  stb_device_scope dev(s->dev);
  return stb_hb_obj_set_groups(&s->hb, s->I, G, goff_host, s->st, "stb_tindic_set_bgroups");
}

// the per-group concentration step (hyperb.hip) on the object's T, customer offsets and concentrations, queued behind its
// sweeps
extern "C" int stb_tindic_sampleb_groups(stb_tindic_t *s, double a, double shape, double scale, uint64_t seed, uint64_t sweep,
                                         double *bgrp_host, stb_bgroups_info_t *info) {
  STB_ENTRY;
  if (!s) return stb_fail("stb_tindic_sampleb_groups: null object");
  stb_device_scope dev(s->dev);
  return stb_hb_obj_step(&s->hb, a, shape, scale, s->I, nullptr, s->d_coff, s->d_T, s->d_bpar, seed, sweep, s->st, bgrp_host, info,
                         "stb_tindic_sampleb_groups");
}

// the concentration step on the object's counts, as stb_tcounts_sampleb: N_i is the customer offsets' difference
extern "C" double stb_tindic_sampleb(stb_tindic_t *s, double b_in, double shape, double scale, double a, void *rng, int loops,
                                     int verbose, uint64_t seed, uint64_t sweep) {
  // (no rand() guard across the call: ARMS draws from the caller's rand() stream, as in sampleb)
  if (!s) {
    stb_fail("stb_tindic_sampleb: null object");
    return NAN;
  }
  stb_device_scope dev(s->dev);
  return stb_sampleb_device_ex(b_in, s->I, shape, scale, nullptr, s->d_coff, s->d_T, a, rng, loops, verbose, seed, sweep, s->st,
                               "stb_tindic_sampleb");
}

// the joint step for a and b on the object's counts (hyperj.hip): the pairs and T to the set, device to device, then the
// step with the object's N, queued behind its sweeps.  Nothing per restaurant crosses to the host; t and T are not written.
extern "C" int stb_tindic_samplejoint(stb_tindic_t *s, stb_groups_t *g, const stb_joint_opts_t *opts, double a_in, double b_in,
                                   double *a_out, double *b_out, stb_joint_info_t *info) {
  if (!s || !g) return stb_fail("stb_tindic_samplejoint: null object");
  if (stb_tindic_to_groups(s, g, nullptr)) return 1;
  return stb_hj_samplejoint(g, nullptr, s->d_coff, opts, a_in, b_in, a_out, b_out, info, "stb_tindic_samplejoint");
}

// ------------------------------------------------------------------------------------------------
// dishes on the object (the kernel is tdish.hip's)

// pair order written out: the dish sweep writes a customer's dish, so it needs the sequence
static int ti_materialise_cust(stb_tindic_t *s, const char *who) {
  if (s->d_cust) return 0;
  std::vector<uint32_t> n(s->G ? s->G : 1), cust(s->C ? s->C : 1);
  std::vector<uint64_t> koff((size_t)s->I + 1);
  if (hipStreamSynchronize(s->st) != hipSuccess ||
      (s->G && hipMemcpy(n.data(), s->d_n, sizeof(uint32_t) * s->G, hipMemcpyDeviceToHost) != hipSuccess) ||
      hipMemcpy(koff.data(), s->d_koff, sizeof(uint64_t) * (s->I + 1), hipMemcpyDeviceToHost) != hipSuccess)
    return STB_STREAM_FAIL(who);
  uint64_t c = 0;
  for (int i = 0; i < s->I; i++)
    for (uint64_t g = koff[i]; g < koff[i + 1]; g++)
      for (uint32_t r = 0; r < n[g]; r++) cust[c++] = (uint32_t)(g - koff[i]);
  uint32_t *d = nullptr;
  if (hipMalloc((void **)&d, sizeof(uint32_t) * (s->C ? s->C : 1)) != hipSuccess)
    return stb_fail("%s: out of device memory for %llu customers", who, (unsigned long long)s->C);
  if (s->C && hipMemcpy(d, cust.data(), sizeof(uint32_t) * s->C, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    return STB_STREAM_FAIL(who);
  }
  s->d_cust = d;
  return 0;
}

// first dish sweep: the customer sequence, the counters, and bounds that hold whatever moving customers can reach
static int ti_dish_prepare(stb_tindic_t *s, const char *who) {
  if (s->dish_ready) return 0;
  if (s->Mgiven == 0 && s->maxNi > 65535u)
    return stb_fail("%s: a restaurant has %llu customers and the object was created with M = 0; t is a uint16, so create "
                    "it with M <= 65535", who, (unsigned long long)s->maxNi);
  if (s->maxNi > 0x7fffffffull) return stb_fail("%s: a restaurant has %llu customers", who, (unsigned long long)s->maxNi);
  if (ti_materialise_cust(s, who)) return 1;
  if (!s->d_info && hipMalloc((void **)&s->d_info, 2 * sizeof(unsigned long long)) != hipSuccess) return STB_STREAM_FAIL(who);
  if (!s->h_info && hipHostMalloc((void **)&s->h_info, 2 * sizeof(unsigned long long)) != hipSuccess) return STB_STREAM_FAIL(who);
  const unsigned maxn = (unsigned)s->maxNi;
  const ti_bounds tb = ti_table_bounds(maxn, s->Mgiven);
  if (tb.need_table && (!s->d_vt || tb.N != s->N || tb.M != s->M)) {
    const uint64_t vstride = (stb_vtable_elems(tb.N, tb.M) + 31) & ~31ull;
    const size_t ws_bytes = stb_fill_workspace_bytes(tb.N, tb.M, 1);
    double *vt = nullptr;
    void *ws = nullptr;
    if (hipMalloc((void **)&vt, sizeof(double) * vstride) != hipSuccess || hipMalloc(&ws, ws_bytes ? ws_bytes : 1) != hipSuccess) {
      if (vt) (void)hipFree(vt);
      return stb_fail("%s: out of device memory for a %u x %u V table", who, tb.N, tb.M);
    }
    if (hipStreamSynchronize(s->st) != hipSuccess) {  // (queued sweeps read the table that goes)
      (void)hipFree(vt);
      (void)hipFree(ws);
      return STB_STREAM_FAIL(who);
    }
    if (s->d_vt) (void)hipFree(s->d_vt);
    if (s->d_ws) (void)hipFree(s->d_ws);
    s->d_vt = vt;
    s->d_ws = ws;
    s->vstride = vstride;
    s->ws_bytes = ws_bytes;
    s->a_filled = NAN;
  }
  if (tb.N != s->N || tb.M != s->M || tb.need_table != s->need_table) {  // the S slab follows on the log joint's next use
    (void)hipStreamSynchronize(s->st);
    ti_drop_sslab(s);
  }
  s->N = tb.N;
  s->M = tb.M;
  s->Mdraw = tb.Mdraw;
  s->need_table = tb.need_table;
  s->maxn = maxn;
  s->dish_ready = true;
  return 0;
}

extern "C" int stb_tindic_set_classes(stb_tindic_t *s, const uint32_t *cls_host, unsigned rows) {
  STB_ENTRY;
  const char *who = "stb_tindic_set_classes";
  if (!s) return stb_fail("%s: null object", who);
  if (cls_host) {
    if (rows < 1) return stb_fail("%s: rows=%u", who, rows);
    for (uint64_t c = 0; c < s->C; c++)
      if (cls_host[c] >= rows) return stb_fail("%s: cls[%llu]=%u (must be < rows = %u)", who, (unsigned long long)c, cls_host[c], rows);
  }
  stb_device_scope dev(s->dev);
  if (hipStreamSynchronize(s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  if (!cls_host) {
    ti_drop_obs(s);  // (nothing below can fail: the observation mode ends with its classes)
    if (s->d_cls) (void)hipFree(s->d_cls);
    s->d_cls = nullptr;
    s->cls_rows = 0;
    return 0;
  }
  if (!s->d_cls && hipMalloc((void **)&s->d_cls, sizeof(uint32_t) * (s->C ? s->C : 1)) != hipSuccess)
    return stb_fail("%s: out of device memory", who);
  if (s->C && hipMemcpy(s->d_cls, cls_host, sizeof(uint32_t) * s->C, hipMemcpyHostToDevice) != hipSuccess) return STB_STREAM_FAIL(who);
  ti_drop_obs(s);  // (the caller's classes are in place: they end the observation mode)
  s->cls_rows = rows;
  return 0;
}

extern "C" int stb_tindic_set_lik(stb_tindic_t *s, const double *lik_host, unsigned rows, unsigned stride) {
  STB_ENTRY;
  const char *who = "stb_tindic_set_lik";
  if (!s) return stb_fail("%s: null object", who);
  const bool drop = !lik_host && rows == 0;
  if (!drop) {
    if (rows < 1) return stb_fail("%s: rows=%u", who, rows);
    if (stride < s->maxK || stride < 1)
      return stb_fail("%s: stride=%u; the largest restaurant has K=%u dishes", who, stride, s->maxK);
    if (lik_host)
      for (uint64_t j = 0; j < (uint64_t)rows * stride; j++)
        if (!(lik_host[j] >= 0.0) || !std::isfinite(lik_host[j]))
          return stb_fail("%s: lik[%llu]=%g (must be finite and >= 0)", who, (unsigned long long)j, lik_host[j]);
  }
  stb_device_scope dev(s->dev);
  if (hipStreamSynchronize(s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  double *d = nullptr;
  if (!drop) {
    const size_t cells = (size_t)rows * stride;
    std::vector<double> ones;
    if (!lik_host) ones.assign(cells, 1.0);
    if (hipMalloc((void **)&d, sizeof(double) * cells) != hipSuccess) return stb_fail("%s: out of device memory", who);
    if (hipMemcpy(d, lik_host ? lik_host : ones.data(), sizeof(double) * cells, hipMemcpyHostToDevice) != hipSuccess) {
      const int rc = STB_STREAM_FAIL(who);
      (void)hipFree(d);
      return rc;
    }
  }
  if (s->d_lik) (void)hipFree(s->d_lik);
  ti_drop_obs(s);  // (the caller's matrix ends the observation mode)
  if (drop || rows != s->lik_rows || stride != s->lik_stride) ti_drop_cgs(s);
  s->d_lik = d;
  s->lik_rows = drop ? 0 : rows;
  s->lik_stride = drop ? 0 : stride;
  s->lik_bad = false;
  return 0;
}

extern "C" double *stb_tindic_lik_device(stb_tindic_t *s, unsigned *rows, unsigned *stride, void **stream) {
  if (!s) {
    stb_fail("stb_tindic_lik_device: null object");
    return nullptr;
  }
  if (rows) *rows = s->lik_rows;
  if (stride) *stride = s->lik_stride;
  if (stream) *stream = (void *)s->st;
  return s->d_lik;
}

extern "C" int stb_tindic_sweep_dishes(stb_tindic_t *s, double a, const double *bpar, uint64_t seed, uint64_t sweep, int nsweeps,
                                       stb_tdish_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_tindic_sweep_dishes";
  if (!s) return stb_fail("%s: null object", who);
  if (s->flags & STB_TI_REF_ODDS_FLAG)
    return stb_fail("%s: the object was created with STB_TI_REF_ODDS; the dish sweep has the exact ratio only", who);
  if (!(a >= 0.0 && a < 1.0)) return stb_fail("%s: discount a=%g outside [0, 1)", who, a);
  if (!bpar) return stb_fail("%s: bpar is required", who);
  if (nsweeps < 0) return stb_fail("%s: nsweeps=%d", who, nsweeps);
  if (ti_check_bpar(s, a, bpar, who)) return 1;
  if (s->maxK > STB_TD_MAXK)
    return stb_fail("%s: a restaurant has K=%u dishes; the sweep holds at most STB_TD_MAXK = %d", who, s->maxK, STB_TD_MAXK);
  if (s->d_lik && (!s->d_cls || s->cls_rows > s->lik_rows))
    return stb_fail("%s: the likelihood has %u rows; classes %s", who, s->lik_rows,
                    s->d_cls ? "were set with more" : "are not set (stb_tindic_set_classes)");
  if ((s->d_lik && s->lik_bad) || s->h_bad)
    return stb_fail("%s: the last stb_tindic_sample_%s failed and left %s undefined; draw again or set it", who,
                    s->h_bad ? "h" : s->d_x ? "gauss" : "lik", s->h_bad ? "h" : "the likelihood");
  if (info) info->skipped = info->stuck = 0;
  if (nsweeps == 0) return 0;
  stb_device_scope dev(s->dev);
  if (ti_dish_prepare(s, who) || ti_ensure_V(s, a) || stb_hb_obj_stage(&s->hb, s->I, s->d_bpar, bpar, s->st, who)) return 1;
  if (hipMemsetAsync(s->d_info, 0, 2 * sizeof(unsigned long long), s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  if (stb_td_launch(ti_vtable(s), ti_rest(s, a), ti_counts(s), ti_customers(s), ti_matrix(s), {seed, sweep}, nsweeps, s->d_info, s->st))
    return 1;
  if (!info) return 0;
  if (ti_fetch(s, {{s->h_info, s->d_info, 2 * sizeof(unsigned long long)}}, who)) return 1;
  info->skipped = s->h_info[0];
  info->stuck = s->h_info[1];
  return 0;
}

extern "C" int stb_tindic_get_state(stb_tindic_t *s, uint32_t *n_out, uint32_t *cust_out) {
  STB_ENTRY;
  const char *who = "stb_tindic_get_state";
  if (!s) return stb_fail("%s: null object", who);
  stb_device_scope dev(s->dev);
  if (cust_out && ti_materialise_cust(s, who)) return 1;
  return ti_fetch(s, {{n_out, s->d_n, sizeof(uint32_t) * s->G}, {cust_out, s->d_cust, sizeof(uint32_t) * s->C}}, who);
}

extern "C" int stb_tindic_class_counts(stb_tindic_t *s, uint32_t *cnt_out) {
  STB_ENTRY;
  const char *who = "stb_tindic_class_counts";
  if (!s || !cnt_out) return stb_fail("%s: null %s", who, s ? "cnt_out" : "object");
  if (ti_not_obs(s, who)) return 1;
  if (!s->d_cls) return stb_fail("%s: classes are not set (stb_tindic_set_classes)", who);
  const unsigned rows = s->cls_rows, stride = s->d_lik ? s->lik_stride : (s->maxK ? s->maxK : 1);
  const size_t bytes = sizeof(uint32_t) * (size_t)rows * stride;
  stb_device_scope dev(s->dev);
  if (ti_materialise_cust(s, who)) return 1;
  stb_pool_scratch sc(s->st);
  uint32_t *d_cnt = nullptr;
  if (sc.take(&d_cnt, bytes) != hipSuccess) return stb_fail("%s: out of device memory", who);
  if (hipMemsetAsync(d_cnt, 0, bytes, s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  if (stb_td_class_counts(ti_customers(s), rows, stride, d_cnt, s->st)) return 1;
  if (hipMemcpyAsync(cnt_out, d_cnt, bytes, hipMemcpyDeviceToHost, s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  return sc.give_back(true, who);
}

// ------------------------------------------------------------------------------------------------
// the likelihood and the base weights drawn on the device, and the data term (the kernels are tlik.hip's)

// what _sample_lik and _loglik ask of the object before anything is queued
static int ti_lik_ready(stb_tindic_t *s, const char *who) {
  if (!s->d_cls) return stb_fail("%s: classes are not set (stb_tindic_set_classes)", who);
  if (!s->d_lik) return stb_fail("%s: no likelihood matrix is set (stb_tindic_set_lik; a NULL matrix with a shape makes one)", who);
  if (s->cls_rows > s->lik_rows)
    return stb_fail("%s: the likelihood has %u rows; classes were set with %u", who, s->lik_rows, s->cls_rows);
  return 0;
}

// customers per (class, dish) over the matrix's shape, into a buffer of the call's scratch, queued on the object's stream
static int ti_count_classes(stb_tindic_t *s, stb_pool_scratch &sc, uint32_t **d_cnt, const char *who) {
  const size_t bytes = sizeof(uint32_t) * (size_t)s->lik_rows * s->lik_stride;
  if (ti_materialise_cust(s, who)) return 1;
  if (sc.take(d_cnt, bytes) != hipSuccess) return stb_fail("%s: out of device memory for the counts", who);
  if (hipMemsetAsync(*d_cnt, 0, bytes, s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  return stb_td_class_counts(ti_customers(s), s->lik_rows, s->lik_stride, *d_cnt, s->st);
}

extern "C" int stb_tindic_sample_lik(stb_tindic_t *s, const double *beta_host, double beta0, uint64_t seed, uint64_t sweep) {
  STB_ENTRY;
  const char *who = "stb_tindic_sample_lik";
  if (!s) return stb_fail("%s: null object", who);
  if (ti_not_obs(s, who)) return 1;
  if (ti_lik_ready(s, who)) return 1;
  if (stb_tl_check_prior(beta_host, s->lik_rows, beta0, "beta", who)) return 1;
  stb_device_scope dev(s->dev);
  stb_pool_scratch sc(s->st);
  uint32_t *d_cnt = nullptr;
  if (ti_count_classes(s, sc, &d_cnt, who)) return 1;
  bool touched = false;
  const int rc = stb_tl_sample_lik(d_cnt, s->lik_rows, s->lik_stride, beta_host, beta0, s->d_lik, seed, sweep, s->st, who, &touched);
  if (touched) s->lik_bad = rc != 0;  // (a call that failed before its first launch left the matrix as it was)
  return sc.last(rc);
}

extern "C" int stb_tindic_loglik(stb_tindic_t *s, double *total, uint64_t *impossible) {
  STB_ENTRY;
  const char *who = "stb_tindic_loglik";
  if (!s) return stb_fail("%s: null object", who);
  if (!total) return stb_fail("%s: total is required", who);
  if (ti_not_obs(s, who)) return 1;
  if (ti_lik_ready(s, who)) return 1;
  if (s->lik_bad) return stb_fail("%s: the last stb_tindic_sample_lik failed and left the likelihood undefined", who);
  stb_device_scope dev(s->dev);
  stb_pool_scratch sc(s->st);
  uint32_t *d_cnt = nullptr;
  if (ti_count_classes(s, sc, &d_cnt, who)) return 1;
  return sc.last(stb_tl_loglik(d_cnt, s->d_lik, s->lik_rows, s->lik_stride, total, impossible, s->st, who));
}

// the h buffer a draw writes: the object's, or a fresh one (d null: out of device memory) that the object adopts only if
// the draw was queued
namespace {
struct ti_fresh_h {
  stb_tindic_t *s;
  double *d;
  explicit ti_fresh_h(stb_tindic_t *s_) : s(s_), d(s_->d_h) {
    if (!d && hipMalloc((void **)&d, sizeof(double) * (s->G ? s->G : 1)) != hipSuccess) d = nullptr;
  }
  void settle(bool touched, int rc) {
    if (touched) {
      s->d_h = d;
      s->h_bad = rc != 0;
    } else if (d != s->d_h) {
      (void)hipFree(d);  // (nothing was queued: the object keeps the h it had)
    }
  }
};
}  // namespace

extern "C" int stb_tindic_sample_h(stb_tindic_t *s, const double *gamma_host, double gamma0, uint64_t seed, uint64_t sweep) {
  STB_ENTRY;
  const char *who = "stb_tindic_sample_h";
  if (!s) return stb_fail("%s: null object", who);
  if (s->flags & STB_TI_REF_ODDS_FLAG)
    return stb_fail("%s: the object was created with STB_TI_REF_ODDS; its sweeps do not leave the law h is drawn under", who);
  if (s->maxK < 1 || s->maxK > STB_TD_MAXK)
    return stb_fail("%s: the largest restaurant has K=%u dishes (1 to STB_TD_MAXK = %d)", who, s->maxK, STB_TD_MAXK);
  if (stb_tl_check_prior(gamma_host, s->maxK, gamma0, "gamma", who)) return 1;
  stb_device_scope dev(s->dev);
  ti_fresh_h h(s);
  if (!h.d) return stb_fail("%s: out of device memory", who);
  bool touched = false;
  const int rc = stb_tl_sample_h(s->I, s->d_koff, s->d_t, s->maxK, gamma_host, gamma0, h.d, seed, sweep, s->st, who, &touched);
  h.settle(touched, rc);
  return rc;
}

// ------------------------------------------------------------------------------------------------
// base weights per group under a shared root (hgroups.hip)

extern "C" int stb_tindic_set_hgroups(stb_tindic_t *s, int G, const uint64_t *goff_host) {
  STB_ENTRY;
  const char *who = "stb_tindic_set_hgroups";
  if (!s) return stb_fail("%s: null object", who);
  if (goff_host) {
    if (G < 1) return stb_fail("%s: G=%d", who, G);
    if (goff_host[0] != 0 || goff_host[G] != (uint64_t)s->I)
      return stb_fail("%s: the ranges run from %llu to %llu; the object has I=%d restaurants", who,
                      (unsigned long long)goff_host[0], (unsigned long long)goff_host[G], s->I);
    for (int g = 0; g < G; g++)
      if (goff_host[g] > goff_host[g + 1]) return stb_fail("%s: goff[%d] > goff[%d]", who, g, g + 1);
  }
  stb_device_scope dev(s->dev);
  int rc = 0;
  uint64_t *d_new = nullptr;  // the new ranges first: a call that fails leaves the object with the ranges it had
  if (goff_host && hipMalloc((void **)&d_new, sizeof(uint64_t) * ((size_t)G + 1)) != hipSuccess)
    rc = stb_fail("%s: out of device memory for %d ranges", who, G);
  if (!rc && goff_host && hipMemcpy(d_new, goff_host, sizeof(uint64_t) * ((size_t)G + 1), hipMemcpyHostToDevice) != hipSuccess)
    rc = STB_STREAM_FAIL(who);
  if (!rc && hipStreamSynchronize(s->st) != hipSuccess) rc = STB_STREAM_FAIL(who);
  if (rc) {
    if (d_new) (void)hipFree(d_new);
  } else {
    if (s->d_hgoff) (void)hipFree(s->d_hgoff);
    s->d_hgoff = d_new;
    s->hg_G = goff_host ? G : 0;
  }
  return rc;
}

// the object's root on the device, made (1/maxK each) when it has none
static int ti_hroot(stb_tindic_t *s, const double *root_host, const char *who) {
  const unsigned K = s->maxK;
  std::vector<double> flat;
  if (!root_host) {
    flat.assign(K, 1.0 / (double)K);
    root_host = flat.data();
  }
  double *d_new = s->d_hroot;
  if (!d_new && hipMalloc((void **)&d_new, sizeof(double) * K) != hipSuccess) return stb_fail("%s: out of device memory", who);
  if (hipStreamSynchronize(s->st) != hipSuccess || hipMemcpy(d_new, root_host, sizeof(double) * K, hipMemcpyHostToDevice) != hipSuccess) {
    if (d_new != s->d_hroot) (void)hipFree(d_new);
    return STB_STREAM_FAIL(who);
  }
  s->d_hroot = d_new;
  return 0;
}

static int ti_hg_maxk(const stb_tindic_t *s, const char *who) {
  if (s->maxK < 1 || s->maxK > STB_TD_MAXK)
    return stb_fail("%s: the largest restaurant has K=%u dishes (1 to STB_TD_MAXK = %d)", who, s->maxK, STB_TD_MAXK);
  return 0;
}

extern "C" int stb_tindic_set_hroot(stb_tindic_t *s, const double *root_host) {
  STB_ENTRY;
  const char *who = "stb_tindic_set_hroot";
  if (!s) return stb_fail("%s: null object", who);
  if (ti_hg_maxk(s, who)) return 1;
  if (root_host && stb_tl_check_prior(root_host, s->maxK, 0.0, "root", who)) return 1;
  stb_device_scope dev(s->dev);
  return ti_hroot(s, root_host, who);
}

extern "C" int stb_tindic_get_hroot(stb_tindic_t *s, double *root_out) {
  STB_ENTRY;
  const char *who = "stb_tindic_get_hroot";
  if (!s || !root_out) return stb_fail("%s: null %s", who, s ? "root_out" : "object");
  if (ti_hg_maxk(s, who)) return 1;
  if (!s->d_hroot) {
    for (unsigned k = 0; k < s->maxK; k++) root_out[k] = 1.0 / (double)s->maxK;
    return 0;
  }
  stb_device_scope dev(s->dev);
  return ti_fetch(s, {{root_out, s->d_hroot, sizeof(double) * s->maxK}}, who);
}

extern "C" int stb_tindic_sample_hgroups(stb_tindic_t *s, const stb_hgroups_opts_t *opts, uint64_t seed, uint64_t sweep,
                                         stb_hgroups_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_tindic_sample_hgroups";
  stb_hg_clear(info);
  if (!s) return stb_fail("%s: null object", who);
  if (!opts) return stb_fail("%s: opts is required", who);
  if (s->flags & STB_TI_REF_ODDS_FLAG)
    return stb_fail("%s: the object was created with STB_TI_REF_ODDS; its sweeps do not leave the law h is drawn under", who);
  if (ti_hg_maxk(s, who)) return 1;
  stb_hgroups_opts_t o = *opts;
  if (o.alpha == 0.0) {
    if (!(s->hg_alpha == s->hg_alpha)) return stb_fail("%s: alpha=0 asks for the object's concentration, and it has none yet", who);
    o.alpha = s->hg_alpha;
  }
  if (stb_hg_check_opts(&o, s->maxK, who)) return 1;
  stb_device_scope dev(s->dev);
  if (!s->d_hroot && ti_hroot(s, nullptr, who)) return 1;
  ti_fresh_h h(s);
  if (!h.d) return stb_fail("%s: out of device memory", who);
  bool touched = false;
  stb_hgroups_info_t mine;
  if (!info) info = &mine;
  const int rc = stb_hg_sample(s->I, s->d_koff, s->d_t, s->maxK, s->d_hgoff ? s->hg_G : s->I, s->d_hgoff, &o, s->d_hroot, h.d, nullptr,
                               nullptr, nullptr, seed, sweep, s->st, info, who, &touched);
  h.settle(touched, rc);
  if (touched && !rc) s->hg_alpha = info->alpha;
  return rc;
}

// ------------------------------------------------------------------------------------------------
// base weights on a tree of nested groups (htree.hip)

extern "C" int stb_tindic_set_htree(stb_tindic_t *s, int levels, const int *G_host, const uint64_t *const *off_host) {
  STB_ENTRY;
  const char *who = "stb_tindic_set_htree";
  if (!s) return stb_fail("%s: null object", who);
  if (levels < 0 || levels > STB_HT_MAXL) return stb_fail("%s: levels=%d (0 to STB_HT_MAXL = %d)", who, levels, STB_HT_MAXL);
  if (levels && (!G_host || !off_host)) return stb_fail("%s: G_host and off_host are required", who);
  if (levels && ti_hg_maxk(s, who)) return 1;
  for (int l = 0; l < levels; l++) {
    if (G_host[l] < 1) return stb_fail("%s: G[%d]=%d (must be >= 1)", who, l, G_host[l]);
    if (!off_host[l]) return stb_fail("%s: off_host[%d] is required", who, l);
    if (stb_ht_check_ranges(l, G_host[l], off_host[l], l == 0 ? (uint64_t)s->I : (uint64_t)G_host[l - 1], who)) return 1;
  }
  stb_device_scope dev(s->dev);
  const unsigned K = s->maxK;
  // the new tree first: a call that fails leaves the object with the tree it had
  uint64_t *d_off[STB_HT_MAXL] = {};
  double *d_node[STB_HT_MAXL] = {};
  int rc = 0;
  std::vector<double> root(K, K ? 1.0 / (double)K : 0.0), rows;
  if (levels && s->d_hroot && ti_fetch(s, {{root.data(), s->d_hroot, sizeof(double) * K}}, who)) return 1;
  if (hipStreamSynchronize(s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  for (int l = 0; l < levels && !rc; l++) {
    const size_t G = (size_t)G_host[l];
    if (hipMalloc((void **)&d_off[l], sizeof(uint64_t) * (G + 1)) != hipSuccess ||
        hipMalloc((void **)&d_node[l], sizeof(double) * G * K) != hipSuccess) {
      rc = stb_fail("%s: out of device memory for level %d's %zu nodes", who, l + 1, G);
      break;
    }
    if (hipMemcpy(d_off[l], off_host[l], sizeof(uint64_t) * (G + 1), hipMemcpyHostToDevice) != hipSuccess) rc = STB_STREAM_FAIL(who);
    if (!rc && l >= 1) {
      rows.resize(G * K);
      for (size_t v = 0; v < G; v++) std::copy(root.begin(), root.end(), rows.begin() + v * K);
      if (hipMemcpy(d_node[l], rows.data(), sizeof(double) * G * K, hipMemcpyHostToDevice) != hipSuccess) rc = STB_STREAM_FAIL(who);
    }
  }
  for (int l = 0; l < STB_HT_MAXL; l++) {
    uint64_t *&off = rc ? d_off[l] : s->d_htoff[l];
    double *&node = rc ? d_node[l] : s->d_htnode[l];
    if (off) (void)hipFree(off);
    if (node) (void)hipFree(node);
    off = nullptr;
    node = nullptr;
  }
  if (rc) return rc;
  s->ht_L = levels;
  for (int l = 0; l < STB_HT_MAXL; l++) {
    s->ht_G[l] = l < levels ? G_host[l] : 0;
    s->d_htoff[l] = d_off[l];
    s->d_htnode[l] = d_node[l];
  }
  s->ht_have_alpha = s->ht_have_rows1 = false;
  return 0;
}

static int ti_ht_level(const stb_tindic_t *s, int level, int lowest, const char *who) {
  if (s->ht_L < 1) return stb_fail("%s: the object has no tree (stb_tindic_set_htree)", who);
  if (level < lowest || level > s->ht_L) return stb_fail("%s: level=%d (%d to the tree's %d)", who, level, lowest, s->ht_L);
  return 0;
}

extern "C" int stb_tindic_set_htree_level(stb_tindic_t *s, int level, const double *rows) {
  STB_ENTRY;
  const char *who = "stb_tindic_set_htree_level";
  if (!s || !rows) return stb_fail("%s: null %s", who, s ? "rows" : "object");
  if (ti_ht_level(s, level, 2, who)) return 1;
  const size_t cells = (size_t)s->ht_G[level - 1] * s->maxK;
  for (size_t e = 0; e < cells; e++)
    if (!(rows[e] > 0.0) || !std::isfinite(rows[e])) return stb_fail("%s: rows[%zu]=%g (must be > 0 and finite)", who, e, rows[e]);
  stb_device_scope dev(s->dev);
  if (hipStreamSynchronize(s->st) != hipSuccess ||
      hipMemcpy(s->d_htnode[level - 1], rows, sizeof(double) * cells, hipMemcpyHostToDevice) != hipSuccess)
    return STB_STREAM_FAIL(who);
  return 0;
}

extern "C" int stb_tindic_get_htree_level(stb_tindic_t *s, int level, double *rows) {
  STB_ENTRY;
  const char *who = "stb_tindic_get_htree_level";
  if (!s || !rows) return stb_fail("%s: null %s", who, s ? "rows" : "object");
  if (ti_ht_level(s, level, 1, who)) return 1;
  if (level == 1 && !s->ht_have_rows1) return stb_fail("%s: level 1's rows are what a step draws, and none has succeeded yet", who);
  stb_device_scope dev(s->dev);
  return ti_fetch(s, {{rows, s->d_htnode[level - 1], sizeof(double) * (size_t)s->ht_G[level - 1] * s->maxK}}, who);
}

extern "C" int stb_tindic_sample_htree(stb_tindic_t *s, const stb_htree_opts_t *opts, uint64_t seed, uint64_t sweep,
                                       stb_htree_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_tindic_sample_htree";
  stb_ht_clear(info);
  if (!s) return stb_fail("%s: null object", who);
  if (!opts) return stb_fail("%s: opts is required", who);
  if (s->flags & STB_TI_REF_ODDS_FLAG)
    return stb_fail("%s: the object was created with STB_TI_REF_ODDS; its sweeps do not leave the law h is drawn under", who);
  if (ti_hg_maxk(s, who)) return 1;
  if (s->ht_L < 1) return stb_fail("%s: the object has no tree (stb_tindic_set_htree)", who);
  if (opts->levels != s->ht_L) return stb_fail("%s: levels=%d; the object's tree has %d", who, opts->levels, s->ht_L);
  const double *alpha = opts->alpha;
  if (!alpha) {
    if (!s->ht_have_alpha) return stb_fail("%s: alpha=NULL asks for the object's concentrations, and it has none yet", who);
    alpha = s->ht_alpha;
  }
  if (stb_ht_check_opts(opts, alpha, s->maxK, who)) return 1;
  stb_device_scope dev(s->dev);
  if (!s->d_hroot && ti_hroot(s, nullptr, who)) return 1;
  ti_fresh_h h(s);
  if (!h.d) return stb_fail("%s: out of device memory", who);
  bool touched = false;
  stb_htree_info_t mine;
  if (!info) info = &mine;
  const int rc = stb_ht_sample(s->I, s->d_koff, s->d_t, s->maxK, s->ht_G, s->d_htoff, opts, alpha, s->d_hroot, s->d_htnode, h.d, nullptr,
                               nullptr, seed, sweep, s->st, info, stb_hg_geom_env("STB_HTREE_WAVES", "STB_HTREE_FORM"), who, &touched);
  h.settle(touched, rc);
  if (touched) s->ht_have_rows1 = !rc;
  if (touched && !rc) {
    for (int l = 0; l < s->ht_L; l++) s->ht_alpha[l] = info->alpha[l];
    s->ht_have_alpha = true;
  }
  return rc;
}

// ------------------------------------------------------------------------------------------------
// the log joint of the object's state (logjoint.hip), and the collapsed one (dirmult.hip)

// the S slab for discount a, with the V table's bounds: taken from the buffer cache on first use, refilled only when the
// discount changes (the refill is checked: a wait)
static int ti_ensure_S(stb_tindic_t *s, double a, const char *who) {
  if (!s->need_table) return 0;
  if (!s->d_stab) {
    s->sstride = (stb_table_elems(s->N, s->M) + 31) & ~31ull;
    s->sws_bytes = stb_fill_workspace_bytes(s->N, s->M, 1);
    if (stb_pool_malloc((void **)&s->d_stab, sizeof(double) * s->sstride) != hipSuccess ||
        stb_pool_malloc((void **)&s->d_sS1, sizeof(double) * s->N) != hipSuccess ||
        stb_pool_malloc(&s->d_sws, s->sws_bytes ? s->sws_bytes : 1) != hipSuccess) {
      ti_drop_sslab(s);
      return stb_fail("%s: out of device memory for a %u x %u S table", who, s->N, s->M);
    }
    s->a_sfilled = NAN;
  }
  if (a == s->a_sfilled) return 0;
  s->a_sfilled = NAN;
  if (stb_fill_S(&a, 1, s->N, s->M, s->d_stab, s->sstride, s->d_sS1, s->N, s->d_sws, s->sws_bytes, stb_default_variant(), s->st) ||
      stb_fill_status())
    return 1;
  s->a_sfilled = a;
  return 0;
}

// the log joint, queued behind the object's sweeps; t and T are not written.  The S cells come from a slab of the object's
// own, given back by stb_tindic_free.
// (with_h false: h is left out -- the collapsed joint's base, stb_tindic_logjoint_collapsed)
static int ti_logjoint(stb_tindic_t *s, double a, const double *bpar, unsigned flags, bool with_h, double *total, double *Li_host,
                       stb_logjoint_info_t *info, const char *who) {
  if (stb_lj_check(a, flags, s->I, who)) return 1;
  if (!bpar) return stb_fail("%s: bpar is required", who);
  if (!total) return stb_fail("%s: total is required", who);
  if (ti_check_bpar(s, a, bpar, who)) return 1;
  stb_device_scope dev(s->dev);
  if (ti_ensure_S(s, a, who) || stb_hb_obj_stage(&s->hb, s->I, s->d_bpar, bpar, s->st, who)) return 1;
  stb_pool_scratch sc(s->st);
  double *d_Li = nullptr;
  if (Li_host && sc.take(&d_Li, sizeof(double) * (size_t)s->I) != hipSuccess)
    return stb_fail("%s: out of device memory for %d values", who, s->I);
  return sc.last(stb_lj_run(ti_stable(s), ti_rest(s, a, with_h), ti_counts(s), flags, d_Li, Li_host, total, info, s->st, who));
}

extern "C" int stb_tindic_logjoint(stb_tindic_t *s, double a, const double *bpar, unsigned flags, double *total, double *Li_host,
                                   stb_logjoint_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_tindic_logjoint";
  if (!s) return stb_fail("%s: null object", who);
  return ti_logjoint(s, a, bpar, flags, true, total, Li_host, info, who);
}

// ---- the collapsed log joint: base weights and class distributions summed out (dirmult.hip)

extern "C" int stb_tindic_logjoint_collapsed(stb_tindic_t *s, double a, const double *bpar, unsigned flags,
                                             const stb_cj_opts_t *opts, double *total, stb_cj_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_tindic_logjoint_collapsed";
  if (!s) return stb_fail("%s: null object", who);
  if (!opts) return stb_fail("%s: opts is required", who);
  if (!total) return stb_fail("%s: total is required", who);
  if (flags & ~(STB_CJ_INDICATORS | STB_CJ_FLAT | STB_CJ_DATA | STB_CJ_ROOT)) return stb_fail("%s: unknown flags 0x%x", who, flags);
  const bool flat = (flags & STB_CJ_FLAT) != 0, want_data = (flags & STB_CJ_DATA) != 0, want_root = (flags & STB_CJ_ROOT) != 0;
  if (flat && want_root) return stb_fail("%s: STB_CJ_ROOT with STB_CJ_FLAT (the flat model has no root)", who);
  if (s->flags & STB_TI_REF_ODDS_FLAG)
    return stb_fail("%s: the object was created with STB_TI_REF_ODDS; its sweeps do not leave the law this is the joint of", who);
  if (ti_hg_maxk(s, who)) return 1;
  if (s->ht_L >= 2)
    return stb_fail("%s: the object has a tree of %d levels (stb_tindic_set_htree); the collapsed joint's grouped formula is "
                    "not that model's", who, s->ht_L);
  double alpha = 1.0;
  if (!flat) {
    alpha = opts->alpha;
    if (alpha == 0.0) {
      if (!(s->hg_alpha == s->hg_alpha)) return stb_fail("%s: alpha=0 asks for the object's concentration, and it has none yet", who);
      alpha = s->hg_alpha;
    }
    if (!(alpha > 0.0) || !std::isfinite(alpha)) return stb_fail("%s: alpha=%g (must be > 0 and finite)", who, alpha);
  }
  const bool read_gamma = flat || want_root;
  if (read_gamma && stb_tl_check_prior(opts->gamma_host, s->maxK, opts->gamma0, "gamma", who)) return 1;
  if (want_data) {
    if (ti_not_obs(s, who)) return 1;
    if (ti_lik_ready(s, who)) return 1;
    if (stb_tl_check_prior(opts->beta_host, s->lik_rows, opts->beta0, "beta", who)) return 1;
  }
  const unsigned Kmax = s->maxK;
  const bool gvec = read_gamma && opts->gamma_host, bvec = want_data && opts->beta_host;
  // the base: a and bpar are checked there, before anything is queued and before *info is written
  double base = 0.0;
  stb_logjoint_info_t lj;
  if (ti_logjoint(s, a, bpar, (flags & STB_CJ_INDICATORS) ? STB_LJ_INDICATORS : 0u, false, &base, nullptr, &lj, who)) return 1;
  stb_cj_info_t mine;
  if (!info) info = &mine;
  memset(info, 0, sizeof(*info));
  info->lj = lj;
  info->pairs = info->lj.pairs;
  info->restaurants = info->lj.restaurants;
  info->binom = info->lj.binom;
  stb_device_scope dev(s->dev);
  const int G = flat ? 1 : (s->d_hgoff ? s->hg_G : s->I);
  const size_t Gs = (size_t)G, cells = Gs * Kmax;
  // scratch.  Zeroed: c[G Kmax], Cg[G].  Then the flat model's one range, gamma[Kmax], beta[rows], the root's two words
  const size_t up = 255, o_Cg = (4 * cells + up) & ~up, o_go = o_Cg + ((8 * Gs + up) & ~up), o_gam = o_go + 256,
               o_beta = o_gam + (gvec ? (8 * (size_t)Kmax + up) & ~up : 0),
               o_root = o_beta + (bvec ? (8 * (size_t)s->lik_rows + up) & ~up : 0), bytes = o_root + 256;
  const size_t stage_bytes = 16 + (gvec ? 8 * (size_t)Kmax : 0) + (bvec ? 8 * (size_t)s->lik_rows : 0);
  stb_pool_scratch sc(s->st);
  char *d = nullptr, *h = nullptr, *stg = nullptr;
  void *h_dev = nullptr;
  if (sc.take(&d, bytes) != hipSuccess || sc.take(&h, 256, 1) != hipSuccess || hipHostGetDevicePointer(&h_dev, h, 0) != hipSuccess ||
      sc.take(&stg, stage_bytes, 1) != hipSuccess)
    return stb_fail("%s: out of memory for %zu bytes of scratch", who, bytes);
  uint32_t *c = (uint32_t *)d;
  unsigned long long *Cg = (unsigned long long *)(d + o_Cg);
  uint64_t *goff1 = (uint64_t *)(d + o_go);
  double *d_gam = gvec ? (double *)(d + o_gam) : nullptr, *d_beta = bvec ? (double *)(d + o_beta) : nullptr;
  // the host's vectors and the flat range, through one pinned block
  ((uint64_t *)stg)[0] = 0;
  ((uint64_t *)stg)[1] = (uint64_t)s->I;
  if (gvec) memcpy(stg + 16, opts->gamma_host, 8 * (size_t)Kmax);
  if (bvec) memcpy(stg + 16 + (gvec ? 8 * (size_t)Kmax : 0), opts->beta_host, 8 * (size_t)s->lik_rows);
  if (hipMemsetAsync(d, 0, o_go, s->st) != hipSuccess || hipMemcpyAsync(goff1, stg, 16, hipMemcpyHostToDevice, s->st) != hipSuccess ||
      (gvec && hipMemcpyAsync(d_gam, stg + 16, 8 * (size_t)Kmax, hipMemcpyHostToDevice, s->st) != hipSuccess) ||
      (bvec && hipMemcpyAsync(d_beta, stg + 16 + (gvec ? 8 * (size_t)Kmax : 0), 8 * (size_t)s->lik_rows, hipMemcpyHostToDevice,
                              s->st) != hipSuccess))
    return STB_STREAM_FAIL(who);
  if (want_root && stb_dm_root_queue(Kmax, s->d_hroot, d_gam, opts->gamma0, (double *)h_dev, s->st)) return 1;
  if (stb_hg_count_queue(s->I, s->d_koff, s->d_t, Kmax, G, flat ? goff1 : s->d_hgoff, c, Cg,
                         stb_hg_geom_env("STB_HGROUPS_WAVES", "STB_HGROUPS_FORM").nw, s->st))
    return 1;
  // flat: w = gamma, scale 1; grouped: w = the root (none: 1 / Kmax each), scale alpha
  if (stb_dm_run(c, (uint64_t)G, Kmax, Kmax, STB_DM_ROWS, flat ? d_gam : s->d_hroot, flat ? opts->gamma0 : 1.0 / (double)Kmax, alpha,
                 nullptr, nullptr, &info->tables, &info->dm_tables, s->st, who))
    return 1;
  if (want_root) {  // (the wait above covered the root's launch)
    info->root = ((volatile double *)h)[0];
    info->root_left_out = ((volatile unsigned long long *)h)[1];
  }
  if (want_data) {
    uint32_t *d_cls_cnt = nullptr;
    if (ti_count_classes(s, sc, &d_cls_cnt, who) ||
        stb_dm_run(d_cls_cnt, (uint64_t)s->lik_rows, s->lik_stride, s->lik_stride, STB_DM_COLUMNS, d_beta, opts->beta0, 1.0, nullptr,
                   nullptr, &info->data, &info->dm_data, s->st, who))
      return 1;
  }
  *total = ((base + info->tables) + info->data) + info->root;
  return 0;
}

// ------------------------------------------------------------------------------------------------
// the Dirichlet concentrations beta and gamma drawn on the device (dirconc.hip)

// the checks both draws make of their own arguments, after the object's
static int ti_dc_args(const double *base_host, uint64_t len, double s_in, double shape, double scale, const stb_dirconc_info_t *info,
                      const char *who) {
  if (!info) return stb_fail("%s: info is required", who);
  if (stb_tl_check_prior(base_host, len, 1.0, "base", who)) return 1;
  if (!(s_in > 0.0) || !std::isfinite(s_in)) return stb_fail("%s: s_in=%g (must be > 0 and finite)", who, s_in);
  if (!(shape > 0.0) || !std::isfinite(shape)) return stb_fail("%s: shape=%g (must be > 0 and finite)", who, shape);
  if (!(scale > 0.0) || !std::isfinite(scale)) return stb_fail("%s: scale=%g (must be > 0 and finite)", who, scale);
  return 0;
}

// head bytes of device scratch (*d) and, behind them, base_host[len] on the device (*d_base; null without a base), staged
// through a pinned block that holds `head_host` (head bytes, may be null) in front of it
static int ti_dc_stage(stb_pool_scratch &sc, size_t head, const void *head_host, const double *base_host, size_t len, char **d,
                       double **d_base, const char *who) {
  const size_t vec = base_host ? 8 * len : 0;
  char *stage = nullptr;
  if (sc.take(d, head + vec + 256) != hipSuccess || sc.take(&stage, head + vec + 256, 1) != hipSuccess)
    return stb_fail("%s: out of memory for %zu bytes of scratch", who, head + vec + 256);
  *d_base = base_host ? (double *)(*d + head) : nullptr;
  if (head_host) memcpy(stage, head_host, head);
  if (base_host) memcpy(stage + head, base_host, vec);
  if ((head_host && hipMemcpyAsync(*d, stage, head, hipMemcpyHostToDevice, sc.st) != hipSuccess) ||
      (base_host && hipMemcpyAsync(*d_base, stage + head, vec, hipMemcpyHostToDevice, sc.st) != hipSuccess))
    return STB_STREAM_FAIL(who);
  return 0;
}

extern "C" int stb_tindic_sample_beta(stb_tindic_t *s, const double *base_host, double s_in, double shape, double scale,
                                      uint64_t seed, uint64_t sweep, stb_dirconc_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_tindic_sample_beta";
  if (!s) return stb_fail("%s: null object", who);
  if (ti_not_obs(s, who)) return 1;
  if (ti_lik_ready(s, who)) return 1;
  if (ti_dc_args(base_host, s->lik_rows, s_in, shape, scale, info, who)) return 1;
  stb_device_scope dev(s->dev);
  stb_pool_scratch sc(s->st);
  char *d = nullptr;
  double *d_base = nullptr;
  uint32_t *d_cls_cnt = nullptr;
  if (ti_dc_stage(sc, 0, nullptr, base_host, s->lik_rows, &d, &d_base, who)) return 1;
  if (ti_count_classes(s, sc, &d_cls_cnt, who)) return 1;
  return stb_dc_run(d_cls_cnt, s->lik_rows, s->lik_stride, s->lik_stride, STB_DM_COLUMNS, d_base, 1.0, s_in, shape, scale, nullptr,
                    nullptr, seed, sweep, s->st, info, who);
}

extern "C" int stb_tindic_sample_gamma(stb_tindic_t *s, const double *base_host, double s_in, double shape, double scale,
                                       uint64_t seed, uint64_t sweep, stb_dirconc_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_tindic_sample_gamma";
  if (!s) return stb_fail("%s: null object", who);
  if (s->flags & STB_TI_REF_ODDS_FLAG)
    return stb_fail("%s: the object was created with STB_TI_REF_ODDS; its sweeps do not leave the law gamma is drawn under", who);
  if (ti_hg_maxk(s, who)) return 1;
  if (ti_dc_args(base_host, s->maxK, s_in, shape, scale, info, who)) return 1;
  const unsigned Kmax = s->maxK;
  stb_device_scope dev(s->dev);
  // device scratch: the one range {0, I} (256 bytes), c[Kmax], C (256 bytes), then the base
  const size_t o_c = 256, o_C = o_c + ((4 * (size_t)Kmax + 255) & ~(size_t)255), head = o_C + 256;
  stb_pool_scratch sc(s->st);
  char *d = nullptr;
  double *d_base = nullptr;
  const uint64_t range[2] = {0, (uint64_t)s->I};
  std::vector<char> head_host(head, 0);  // (the counts start at zero)
  memcpy(head_host.data(), range, sizeof(range));
  if (ti_dc_stage(sc, head, head_host.data(), base_host, Kmax, &d, &d_base, who)) return 1;
  if (stb_hg_count_queue(s->I, s->d_koff, s->d_t, Kmax, 1, (const uint64_t *)d, (uint32_t *)(d + o_c), (unsigned long long *)(d + o_C),
                         stb_hg_geom_env("STB_HGROUPS_WAVES", "STB_HGROUPS_FORM").nw, s->st))
    return 1;
  return stb_dc_run((const uint32_t *)(d + o_c), 1, Kmax, Kmax, STB_DM_ROWS, d_base, 1.0, s_in, shape, scale, nullptr, nullptr, seed,
                    sweep, s->st, info, who);
}

// ------------------------------------------------------------------------------------------------
// what the state predicts: dish proportions and held-out customers (the kernels are predict.hip's)

extern "C" int stb_tindic_set_heldout(stb_tindic_t *s, const uint64_t *hoff_host, const uint32_t *hcls_host) {
  STB_ENTRY;
  const char *who = "stb_tindic_set_heldout";
  if (!s) return stb_fail("%s: null object", who);
  uint64_t Hc = 0, hmax = 0;
  unsigned cmax = 0;
  if (hoff_host) {
    if (hoff_host[0] != 0) return stb_fail("%s: hoff[0]=%llu (must be 0)", who, (unsigned long long)hoff_host[0]);
    for (int i = 0; i < s->I; i++)
      if (hoff_host[i + 1] < hoff_host[i]) return stb_fail("%s: hoff[%d] < hoff[%d]", who, i + 1, i);
    for (int i = 0; i < s->I; i++) hmax = std::max(hmax, hoff_host[i + 1] - hoff_host[i]);
    Hc = hoff_host[s->I];
    if (Hc && !hcls_host) return stb_fail("%s: the held-out classes are required", who);
    for (uint64_t c = 0; c < Hc; c++) {
      if (s->d_lik && hcls_host[c] >= s->lik_rows)
        return stb_fail("%s: hcls[%llu]=%u (the likelihood has %u rows)", who, (unsigned long long)c, hcls_host[c], s->lik_rows);
      cmax = hcls_host[c] > cmax ? hcls_host[c] : cmax;
    }
  }
  stb_device_scope dev(s->dev);
  int rc = 0;
  uint64_t *d_hoff = nullptr;
  uint32_t *d_hcls = nullptr;
  double *d_pacc = nullptr;
  if (hipStreamSynchronize(s->st) != hipSuccess) rc = STB_STREAM_FAIL(who);
  if (!rc && hoff_host) {
    const size_t Hs = Hc ? Hc : 1;
    if (hipMalloc((void **)&d_hoff, sizeof(uint64_t) * ((size_t)s->I + 1)) != hipSuccess ||
        hipMalloc((void **)&d_hcls, sizeof(uint32_t) * Hs) != hipSuccess || hipMalloc((void **)&d_pacc, sizeof(double) * Hs) != hipSuccess)
      rc = stb_fail("%s: out of device memory for %llu held-out customers", who, (unsigned long long)Hc);
    if (!rc && (hipMemcpy(d_hoff, hoff_host, sizeof(uint64_t) * ((size_t)s->I + 1), hipMemcpyHostToDevice) != hipSuccess ||
                (Hc && hipMemcpy(d_hcls, hcls_host, sizeof(uint32_t) * Hc, hipMemcpyHostToDevice) != hipSuccess) ||
                hipMemset(d_pacc, 0, sizeof(double) * Hs) != hipSuccess))
      rc = STB_STREAM_FAIL(who);
  }
  if (rc) {  // the set the object had stays
    void *fresh[] = {d_hoff, d_hcls, d_pacc};
    for (void *p : fresh)
      if (p) (void)hipFree(p);
  } else {
    void *old[] = {s->d_hoff, s->d_hcls, s->d_pacc};
    for (void *p : old)
      if (p) (void)hipFree(p);
    s->d_hoff = d_hoff;
    s->d_hcls = d_hcls;
    s->d_pacc = d_pacc;
    s->Hc = Hc;
    s->hcls_max = cmax;
    s->hsamples = 0;
    s->hmaxNi = hmax;
  }
  return rc;
}

// what _predict and _heldout ask of the object and of (a, bpar) before anything is queued
static int ti_pr_ready(stb_tindic_t *s, double a, const double *bpar, unsigned flags, bool heldout, const char *who) {
  if (stb_pr_check(a, flags, s->I, who)) return 1;
  if (!bpar) return stb_fail("%s: bpar is required", who);
  if (ti_check_bpar(s, a, bpar, who)) return 1;
  if (s->maxK > STB_TD_MAXK)
    return stb_fail("%s: a restaurant has K=%u dishes; the kernel holds at most STB_TD_MAXK = %d", who, s->maxK, STB_TD_MAXK);
  if (s->h_bad) return stb_fail("%s: the last stb_tindic_sample_h failed and left h undefined; draw again or set it", who);
  if (heldout) {
    if (!s->d_hoff) return stb_fail("%s: no held-out customers are set (stb_tindic_set_heldout)", who);
    if (s->d_lik && s->lik_bad)
      return stb_fail("%s: the last stb_tindic_sample_lik failed and left the likelihood undefined; draw again or set it", who);
    if (s->d_lik && s->Hc && s->hcls_max >= s->lik_rows)
      return stb_fail("%s: a held-out customer has class %u; the likelihood has %u rows", who, s->hcls_max, s->lik_rows);
  }
  return 0;
}

// how the four held-out estimators open: an object, somewhere for the total, and ti_pr_ready's refusals, in that order
static int ti_heldout_ready(stb_tindic_t *s, double a, const double *bpar, unsigned flags, const double *total, const char *who) {
  if (!s) return stb_fail("%s: null object", who);
  if (!total) return stb_fail("%s: total is required", who);
  if (ti_not_obs(s, who)) return 1;
  return ti_pr_ready(s, a, bpar, flags, true, who);
}

extern "C" int stb_tindic_predict(stb_tindic_t *s, double a, const double *bpar, double *theta_host, unsigned tstride) {
  STB_ENTRY;
  const char *who = "stb_tindic_predict";
  if (!s) return stb_fail("%s: null object", who);
  if (!theta_host) return stb_fail("%s: theta_host is required", who);
  if (ti_pr_ready(s, a, bpar, 0, false, who)) return 1;
  if (tstride < s->maxK || tstride < 1) return stb_fail("%s: tstride=%u; the largest restaurant has K=%u dishes", who, tstride, s->maxK);
  stb_device_scope dev(s->dev);
  const size_t bytes = sizeof(double) * (size_t)s->I * tstride;
  if (stb_hb_obj_stage(&s->hb, s->I, s->d_bpar, bpar, s->st, who)) return 1;
  stb_pool_scratch sc(s->st);
  double *d_theta = nullptr;
  if (sc.take(&d_theta, bytes) != hipSuccess) return stb_fail("%s: out of device memory for %d x %u values", who, s->I, tstride);
  if (stb_pr_predict(ti_rest(s, a), ti_counts(s), stb_cust_ro{}, stb_lik_view{}, {d_theta, tstride}, 0, s->st, who)) return 1;
  if (hipMemcpyAsync(theta_host, d_theta, bytes, hipMemcpyDeviceToHost, s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  return sc.give_back(true, who);
}

extern "C" int stb_tindic_heldout(stb_tindic_t *s, double a, const double *bpar, unsigned flags, double *total, double *Hi_host,
                                  stb_predict_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_tindic_heldout";
  if (ti_heldout_ready(s, a, bpar, flags, total, who)) return 1;
  const bool accumulate = (flags & STB_PR_ACCUMULATE) != 0;
  if (accumulate && s->hsamples == 0xffffffffu) return stb_fail("%s: the sample count is full (stb_tindic_heldout_reset)", who);
  stb_device_scope dev(s->dev);
  if (stb_hb_obj_stage(&s->hb, s->I, s->d_bpar, bpar, s->st, who)) return 1;
  stb_pool_scratch sc(s->st);
  stb_pr_out out;  // p: the accumulator, or a buffer of the call's
  double *d_Hi = nullptr;
  if (accumulate) out.p = s->d_pacc;
  if ((!accumulate && sc.take(&out.p, sizeof(double) * (s->Hc ? s->Hc : 1)) != hipSuccess) ||
      (Hi_host && sc.take(&d_Hi, sizeof(double) * (size_t)s->I) != hipSuccess) || sc.take(&out.skipped, sizeof(uint64_t)) != hipSuccess)
    return stb_fail("%s: out of device memory for %llu held-out customers", who, (unsigned long long)s->Hc);
  if (hipMemsetAsync(out.skipped, 0, sizeof(uint64_t), s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  if (stb_pr_predict(ti_rest(s, a), ti_counts(s), ti_heldout(s), ti_matrix(s), out, flags, s->st, who)) return 1;
  const unsigned samples = accumulate ? ++s->hsamples : 1u;
  return sc.last(stb_pr_heldout(out.p, s->d_hoff, s->I, samples, d_Hi, Hi_host, total, info, out.skipped, s->st, who));
}

// ------------------------------------------------------------------------------------------------
// the seating run forwards: a start state for the object, and its held-out customers seated one by one (seat.hip)

// what a seating of all the object's customers asks before anything is queued; prior: no matrix whatever the object holds
static int ti_seat_ready(stb_tindic_t *s, double a, const double *bpar, bool prior, const char *who) {
  const bool lik = s->d_lik && !prior;
  if (s->flags & STB_TI_REF_ODDS_FLAG)
    return stb_fail("%s: the object was created with STB_TI_REF_ODDS; the seating has the exact weights only", who);
  if (stb_seat_check(a, s->Mgiven, 1, STB_SEAT_COMMIT, s->I, who)) return 1;
  if (!bpar) return stb_fail("%s: bpar is required", who);
  if (ti_check_bpar(s, a, bpar, who)) return 1;
  if (s->maxK > STB_TD_MAXK)
    return stb_fail("%s: a restaurant has K=%u dishes; the seating holds at most STB_TD_MAXK = %d", who, s->maxK, STB_TD_MAXK);
  if (lik && (!s->d_cls || s->cls_rows > s->lik_rows))
    return stb_fail("%s: the likelihood has %u rows; classes %s", who, s->lik_rows,
                    s->d_cls ? "were set with more" : "are not set (stb_tindic_set_classes)");
  if ((lik && s->lik_bad) || s->h_bad)
    return stb_fail("%s: the last stb_tindic_sample_%s failed and left %s undefined; draw again or set it", who,
                    s->h_bad ? "h" : s->d_x ? "gauss" : "lik", s->h_bad ? "h" : "the likelihood");
  return 0;
}

// the seating from empty restaurants on the object's stream, no wait (stb_tindic_seat and stb_tindic_generate: one launch
// site, so the two stay bit-equal).  d_lw: I doubles; d_cnt: k_seat's three words, zeroed here
static int ti_seat_queue(stb_tindic_t *s, double a, const double *bpar, bool prior, uint64_t seed, uint64_t sweep, double *d_lw,
                         uint64_t *d_cnt, const char *who) {
  if (ti_dish_prepare(s, who) || stb_hb_obj_stage(&s->hb, s->I, s->d_bpar, bpar, s->st, who)) return 1;
  // (no restaurant of an object is skipped -- K_i <= STB_TD_MAXK, the matrix covers the largest K_i, customers come from
  // pairs -- so every pair is written again: the seating the object had goes here)
  if (hipMemsetAsync(d_cnt, 0, 3 * sizeof(uint64_t), s->st) != hipSuccess ||
      (s->G && (hipMemsetAsync(s->d_n, 0, sizeof(uint32_t) * s->G, s->st) != hipSuccess ||
                hipMemsetAsync(s->d_t, 0, sizeof(uint16_t) * s->G, s->st) != hipSuccess)))
    return STB_STREAM_FAIL(who);
  const bool lik = s->d_lik && !prior;
  return stb_seat_launch(ti_rest(s, a), ti_counts(s), s->Mgiven, ti_customers(s, lik), lik ? ti_matrix(s) : stb_lik_view{}, 1,
                         STB_SEAT_COMMIT, {seed, sweep}, {d_lw, nullptr, d_cnt}, s->st, who);
}

extern "C" int stb_tindic_seat(stb_tindic_t *s, double a, const double *bpar, uint64_t seed, uint64_t sweep, double *total,
                               stb_seat_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_tindic_seat";
  if (!s) return stb_fail("%s: null object", who);
  if (ti_seat_ready(s, a, bpar, false, who)) return 1;
  if (info) memset(info, 0, sizeof(*info));
  stb_device_scope dev(s->dev);
  stb_pool_scratch sc(s->st);
  double *d_lw = nullptr;
  uint64_t *d_cnt = nullptr;
  if (sc.take(&d_lw, sizeof(double) * (size_t)s->I) != hipSuccess || sc.take(&d_cnt, 3 * sizeof(uint64_t)) != hipSuccess)
    return stb_fail("%s: out of device memory for %d values", who, s->I);
  if (ti_seat_queue(s, a, bpar, false, seed, sweep, d_lw, d_cnt, who)) return 1;
  if (!total && !info) return sc.give_back(true, who);
  if (info) info->customers = s->C;
  return sc.last(stb_seat_sum(d_lw, s->I, 1, nullptr, nullptr, total, info, d_cnt, s->st, who));
}

extern "C" int stb_tindic_heldout_seq(stb_tindic_t *s, double a, const double *bpar, unsigned particles, uint64_t seed,
                                      uint64_t sweep, double *total, double *Hi_host, stb_seat_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_tindic_heldout_seq";
  if (ti_heldout_ready(s, a, bpar, 0, total, who)) return 1;
  if (stb_seat_check(a, s->Mgiven, particles, 0, s->I, who)) return 1;
  if (info) memset(info, 0, sizeof(*info));
  stb_device_scope dev(s->dev);
  if (stb_hb_obj_stage(&s->hb, s->I, s->d_bpar, bpar, s->st, who)) return 1;
  stb_pool_scratch sc(s->st);
  double *d_lw = nullptr, *d_Hi = nullptr;
  uint64_t *d_cnt = nullptr;
  if (sc.take(&d_lw, sizeof(double) * (size_t)s->I * particles) != hipSuccess ||
      (Hi_host && sc.take(&d_Hi, sizeof(double) * (size_t)s->I) != hipSuccess) || sc.take(&d_cnt, 3 * sizeof(uint64_t)) != hipSuccess)
    return stb_fail("%s: out of device memory for %d x %u log weights", who, s->I, particles);
  if (hipMemsetAsync(d_cnt, 0, 3 * sizeof(uint64_t), s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  if (stb_seat_launch(ti_rest(s, a), ti_counts(s), s->Mgiven, ti_heldout(s), ti_matrix(s), particles, 0, {seed, sweep},
                      {d_lw, nullptr, d_cnt}, s->st, who))
    return 1;
  if (info) info->customers = s->Hc;
  return sc.last(stb_seat_sum(d_lw, s->I, particles, d_Hi, Hi_host, total, info, d_cnt, s->st, who));
}

extern "C" int stb_tindic_heldout_pf(stb_tindic_t *s, double a, const double *bpar, unsigned particles, double tau, uint64_t seed,
                                     uint64_t sweep, double *total, double *Hi_host, stb_pf_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_tindic_heldout_pf";
  if (ti_heldout_ready(s, a, bpar, 0, total, who)) return 1;
  if (stb_seat_pf_check(a, s->Mgiven, particles, tau, s->I, who)) return 1;
  if (info) memset(info, 0, sizeof(*info));
  stb_device_scope dev(s->dev);
  if (stb_hb_obj_stage(&s->hb, s->I, s->d_bpar, bpar, s->st, who)) return 1;
  stb_pool_scratch sc(s->st);
  double *d_Hi = nullptr;
  uint64_t *d_cnt = nullptr;
  if (sc.take(&d_Hi, sizeof(double) * (size_t)(s->I ? s->I : 1)) != hipSuccess || sc.take(&d_cnt, 5 * sizeof(uint64_t)) != hipSuccess)
    return stb_fail("%s: out of device memory for %d values", who, s->I);
  if (hipMemsetAsync(d_cnt, 0, 5 * sizeof(uint64_t), s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  if (stb_seat_pf_launch(ti_rest(s, a), ti_counts(s), s->Mgiven, ti_heldout(s), ti_matrix(s), particles, tau, {seed, sweep},
                         {d_Hi, d_cnt}, s->st, who))
    return 1;
  // the total: k_seat_sum over one "particle" a restaurant, H = m + log(1 / 1) = m exactly (d_Hi is written with what was
  // read); its three words are the seating's first three, the filter's own two are fetched behind it
  stb_seat_info_t si;
  uint64_t two[2] = {0, 0};
  if (stb_seat_sum(d_Hi, s->I, 1, d_Hi, Hi_host, total, &si, d_cnt, s->st, who)) return sc.last(1);
  if (s->I > 0 && info) {
    if (hipMemcpyAsync(two, d_cnt + 3, sizeof(two), hipMemcpyDeviceToHost, s->st) != hipSuccess ||
        hipStreamSynchronize(s->st) != hipSuccess)
      return sc.last(STB_STREAM_FAIL(who));
  }
  if (info) {
    info->skipped = si.skipped;
    info->impossible = si.impossible;
    info->stuck = si.stuck;
    info->dead = two[0];
    info->resamplings = two[1];
    info->customers = s->Hc;
  }
  return sc.last(0);
}

// the V table the ladder's dish sweeps read: for discount a at the bounds the held-out customers can reach.  Kept with
// the object; allocated again when the bounds change, refilled (checked: a wait) when they or the discount do
static int ti_ais_table(stb_tindic_t *s, double a, const ti_bounds &tb, const char *who) {
  if (!tb.need_table) return 0;
  if (!s->d_avt || tb.N != s->aN || tb.M != s->aM) {
    const uint64_t vstride = (stb_vtable_elems(tb.N, tb.M) + 31) & ~31ull;
    const size_t ws_bytes = stb_fill_workspace_bytes(tb.N, tb.M, 1);
    double *vt = nullptr;
    void *ws = nullptr;
    if (hipMalloc((void **)&vt, sizeof(double) * vstride) != hipSuccess || hipMalloc(&ws, ws_bytes ? ws_bytes : 1) != hipSuccess) {
      if (vt) (void)hipFree(vt);
      return stb_fail("%s: out of device memory for a %u x %u V table", who, tb.N, tb.M);
    }
    if (hipStreamSynchronize(s->st) != hipSuccess) {  // (a queued ladder reads the table that goes)
      (void)hipFree(vt);
      (void)hipFree(ws);
      return STB_STREAM_FAIL(who);
    }
    if (s->d_avt) (void)hipFree(s->d_avt);
    if (s->d_aws) (void)hipFree(s->d_aws);
    s->d_avt = vt;
    s->d_aws = ws;
    s->avstride = vstride;
    s->aws_bytes = ws_bytes;
    s->aN = tb.N;
    s->aM = tb.M;
    s->a_afilled = NAN;
  }
  if (a == s->a_afilled) return 0;
  s->a_afilled = NAN;
  if (stb_fill_V(&a, 1, s->aN, s->aM, s->d_avt, s->avstride, s->d_aws, s->aws_bytes, s->st) || stb_fill_status()) return 1;
  s->a_afilled = a;
  return 0;
}

extern "C" int stb_tindic_heldout_ais(stb_tindic_t *s, double a, const double *bpar, unsigned particles, unsigned S,
                                      const double *betas, unsigned passes, uint64_t seed, uint64_t sweep, double *total,
                                      double *Hi_host, stb_ais_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_tindic_heldout_ais";
  if (ti_heldout_ready(s, a, bpar, 0, total, who)) return 1;
  if (s->flags & STB_TI_REF_ODDS_FLAG)
    return stb_fail("%s: the object was created with STB_TI_REF_ODDS; the dish sweep has the exact weights only", who);
  if (s->C != 0)
    return stb_fail("%s: the object holds %llu customers of its own; the ladder's sweeps would move the held-out customers of a "
                    "restaurant as if its own were exchangeable with them, which is not the conditional given their seating "
                    "(only empty objects: unseen documents)", who, (unsigned long long)s->C);
  if (!s->d_lik) return stb_fail("%s: the object has no likelihood (stb_tindic_set_lik): the prior alone has nothing to anneal to", who);
  if (s->Mgiven == 0 && s->hmaxNi > 65535u)
    return stb_fail("%s: a restaurant has %llu held-out customers and the object was created with M = 0; t is a uint16, so "
                    "create it with M <= 65535", who, (unsigned long long)s->hmaxNi);
  if (s->hmaxNi > 0x7fffffffull) return stb_fail("%s: a restaurant has %llu held-out customers", who, (unsigned long long)s->hmaxNi);
  const ti_bounds tb = ti_table_bounds((unsigned)s->hmaxNi, s->Mgiven);
  if (stb_seat_anneal_check(a, tb.N, tb.M, particles, S, betas, passes, s->I, who)) return 1;
  if (info) memset(info, 0, sizeof(*info));
  stb_device_scope dev(s->dev);
  if (ti_ais_table(s, a, tb, who) || stb_hb_obj_stage(&s->hb, s->I, s->d_bpar, bpar, s->st, who)) return 1;
  const size_t ws_bytes = stb_seat_anneal_workspace_bytes(s->I, s->G, s->Hc, particles, s->lik_rows, s->lik_stride);
  stb_pool_scratch sc(s->st);
  double *d_lw = nullptr, *d_Hi = nullptr;
  uint64_t *d_cnt = nullptr;
  void *d_ws = nullptr;
  if (sc.take(&d_lw, sizeof(double) * (size_t)s->I * particles) != hipSuccess ||
      (Hi_host && sc.take(&d_Hi, sizeof(double) * (size_t)s->I) != hipSuccess) || sc.take(&d_cnt, 3 * sizeof(uint64_t)) != hipSuccess ||
      sc.take(&d_ws, ws_bytes) != hipSuccess)
    return stb_fail("%s: out of device memory for %d x %u replicas (%zu bytes of workspace: split the restaurants)", who, s->I,
                    particles, ws_bytes);
  if (hipMemsetAsync(d_cnt, 0, 3 * sizeof(uint64_t), s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  if (stb_seat_anneal_launch(ti_atable(s, tb), ti_rest(s, a), ti_heldout(s), ti_matrix(s), particles, {S, betas, passes},
                             {seed, sweep}, {d_lw, d_cnt}, d_ws, ws_bytes, s->st, who))
    return 1;
  // k_seat_sum hands the three words on as they are: skipped, dead (in `impossible`'s place), stuck
  stb_seat_info_t si;
  if (stb_seat_sum(d_lw, s->I, particles, d_Hi, Hi_host, total, &si, d_cnt, s->st, who)) return sc.last(1);
  if (info) {
    info->skipped = si.skipped;
    info->dead = si.impossible;
    info->stuck = si.stuck;
    info->customers = s->Hc;
  }
  return sc.last(0);
}

extern "C" int stb_tindic_heldout_reset(stb_tindic_t *s) {
  STB_ENTRY;
  const char *who = "stb_tindic_heldout_reset";
  if (!s) return stb_fail("%s: null object", who);
  if (!s->d_hoff) return stb_fail("%s: no held-out customers are set (stb_tindic_set_heldout)", who);
  stb_device_scope dev(s->dev);
  if (hipMemsetAsync(s->d_pacc, 0, sizeof(double) * (s->Hc ? s->Hc : 1), s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  s->hsamples = 0;
  return 0;
}

extern "C" int stb_tindic_heldout_get(stb_tindic_t *s, double *p_out, unsigned *samples) {
  STB_ENTRY;
  const char *who = "stb_tindic_heldout_get";
  if (!s) return stb_fail("%s: null object", who);
  if (!s->d_hoff) return stb_fail("%s: no held-out customers are set (stb_tindic_set_heldout)", who);
  stb_device_scope dev(s->dev);
  if (ti_fetch(s, {{p_out, s->d_pacc, sizeof(double) * s->Hc}}, who)) return 1;
  if (samples) *samples = s->hsamples;
  return 0;
}

// ------------------------------------------------------------------------------------------------
// customers' classes drawn from the matrix given their dishes, and the model's own data (the kernels are classgen.hip's)

// what a class draw asks of the object before anything is queued
static int ti_cls_ready(stb_tindic_t *s, bool masked, const char *who) {
  if (!s->d_lik) return stb_fail("%s: no likelihood matrix is set (stb_tindic_set_lik)", who);
  if (s->lik_bad) return stb_fail("%s: the last stb_tindic_sample_lik failed and left the likelihood undefined; draw again or set it", who);
  if (masked && !s->d_cls) return stb_fail("%s: a mask keeps classes, and none are set (stb_tindic_set_classes)", who);
  // (also where every customer is visited: one that is masked out, stuck or skipped keeps its class, and afterwards the
  // classes' rows are the matrix's)
  if (s->d_cls && s->cls_rows > s->lik_rows)
    return stb_fail("%s: the likelihood has %u rows; classes were set with %u", who, s->lik_rows, s->cls_rows);
  return 0;
}

namespace {
// what a class draw needs beyond the object's arrays, taken before anything is queued: the customer sequence, the scratch,
// the counters, and a class array where the object has none (zeroed: a customer whose column is stuck keeps class 0).  A
// fresh array that the object did not adopt goes when the call ends, behind a wait for what was queued on it
struct ti_cls_room {
  hipStream_t st;
  uint32_t *d_cls = nullptr;
  bool fresh = false;
  explicit ti_cls_room(hipStream_t st_) : st(st_) {}
  ti_cls_room(const ti_cls_room &) = delete;
  ti_cls_room &operator=(const ti_cls_room &) = delete;
  ~ti_cls_room() {
    if (!fresh) return;
    (void)hipStreamSynchronize(st);
    (void)hipFree(d_cls);
  }
};
}  // namespace

static int ti_cls_take(stb_tindic_t *s, ti_cls_room &room, const char *who) {
  if (ti_materialise_cust(s, who)) return 1;
  const size_t need = stb_cg_scratch_bytes(s->lik_rows, s->lik_stride);
  if (!s->d_cgs || s->cgs_bytes != need) {
    void *d = nullptr;
    if (stb_pool_malloc(&d, need) != hipSuccess)
      return stb_fail("%s: out of device memory for a %u x %u scratch", who, s->lik_rows, s->lik_stride);
    if (s->d_cgs && hipStreamSynchronize(s->st) != hipSuccess) {
      stb_pool_free(d);
      return STB_STREAM_FAIL(who);
    }
    ti_drop_cgs(s);
    s->d_cgs = d;
    s->cgs_bytes = need;
  }
  if (!s->d_cginfo && hipMalloc((void **)&s->d_cginfo, 6 * sizeof(uint64_t)) != hipSuccess) return STB_STREAM_FAIL(who);
  room.d_cls = s->d_cls;
  if (!room.d_cls) {
    const size_t bytes = sizeof(uint32_t) * (s->C ? s->C : 1);
    if (hipMalloc((void **)&room.d_cls, bytes) != hipSuccess) return stb_fail("%s: out of device memory for %llu classes", who, (unsigned long long)s->C);
    room.fresh = true;
    if (hipMemsetAsync(room.d_cls, 0, bytes, s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  }
  return 0;
}

// the draw on the object's stream, no wait; the object adopts a fresh class array once the draw is queued
static int ti_cls_draw(stb_tindic_t *s, ti_cls_room &room, const uint8_t *d_mask, uint64_t seed, uint64_t sweep, const char *who) {
  if (hipMemsetAsync(s->d_cginfo, 0, 3 * sizeof(uint64_t), s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  if (stb_cg_launch(ti_matrix(s), s->d_cust, d_mask, s->C, {seed, sweep}, room.d_cls, s->d_cginfo, s->d_cgs, s->st, who)) return 1;
  room.fresh = false;
  s->d_cls = room.d_cls;
  s->cls_rows = s->lik_rows;
  return 0;
}

static int ti_cls_info(stb_tindic_t *s, stb_classes_info_t *info, const char *who) {
  uint64_t w[3] = {0, 0, 0};
  if (ti_fetch(s, {{w, s->d_cginfo, sizeof(w)}}, who)) return 1;
  info->skipped = w[0];
  info->stuck = w[1];
  info->drawn = w[2];
  return 0;
}

extern "C" int stb_tindic_sample_classes(stb_tindic_t *s, const uint8_t *mask_host, uint64_t seed, uint64_t sweep,
                                         stb_classes_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_tindic_sample_classes";
  if (!s) return stb_fail("%s: null object", who);
  if (ti_not_obs(s, who)) return 1;
  if (ti_cls_ready(s, mask_host != nullptr, who)) return 1;
  if (info) info->skipped = info->stuck = info->drawn = 0;
  stb_device_scope dev(s->dev);
  stb_pool_scratch sc(s->st);
  uint8_t *d_mask = nullptr;
  if (mask_host && s->C) {
    if (sc.take(&d_mask, s->C) != hipSuccess) return stb_fail("%s: out of device memory for the mask", who);
    if (hipMemcpyAsync(d_mask, mask_host, s->C, hipMemcpyHostToDevice, s->st) != hipSuccess) return STB_STREAM_FAIL(who);
  }
  ti_cls_room room(s->st);
  if (ti_cls_take(s, room, who) || ti_cls_draw(s, room, d_mask, seed, sweep, who)) return 1;
  if (info) return sc.last(ti_cls_info(s, info, who));
  return sc.give_back(true, who);  // (nothing taken, no mask: no wait)
}

extern "C" int stb_tindic_generate(stb_tindic_t *s, double a, const double *bpar, uint64_t seed, uint64_t sweep,
                                   stb_seat_info_t *seat_info, stb_classes_info_t *cls_info) {
  STB_ENTRY;
  const char *who = "stb_tindic_generate";
  if (!s) return stb_fail("%s: null object", who);
  if (ti_not_obs(s, who)) return 1;
  if (ti_seat_ready(s, a, bpar, true, who) || ti_cls_ready(s, false, who)) return 1;
  if (seat_info) memset(seat_info, 0, sizeof(*seat_info));
  if (cls_info) cls_info->skipped = cls_info->stuck = cls_info->drawn = 0;
  stb_device_scope dev(s->dev);
  stb_pool_scratch sc(s->st);
  double *d_lw = nullptr;
  if (sc.take(&d_lw, sizeof(double) * (size_t)s->I) != hipSuccess) return stb_fail("%s: out of device memory for %d values", who, s->I);
  ti_cls_room room(s->st);
  if (ti_cls_take(s, room, who)) return 1;
  // the seating under the prior (its three words live behind the class draw's), then every class
  uint64_t *d_cnt = s->d_cginfo + 3;
  if (ti_seat_queue(s, a, bpar, true, seed, sweep, d_lw, d_cnt, who) || ti_cls_draw(s, room, nullptr, seed, sweep, who)) return 1;
  if (seat_info) {
    seat_info->customers = s->C;
    if (stb_seat_sum(d_lw, s->I, 1, nullptr, nullptr, nullptr, seat_info, d_cnt, s->st, who)) return 1;
  }
  if (cls_info) return sc.last(ti_cls_info(s, cls_info, who));
  return sc.give_back(true, who);
}

extern "C" int stb_tindic_get_classes(stb_tindic_t *s, uint32_t *cls_out, unsigned *rows_out) {
  STB_ENTRY;
  const char *who = "stb_tindic_get_classes";
  if (!s) return stb_fail("%s: null object", who);
  if (!s->d_cls) return stb_fail("%s: classes are not set (stb_tindic_set_classes, stb_tindic_sample_classes)", who);
  if (rows_out) *rows_out = s->cls_rows;
  stb_device_scope dev(s->dev);
  return ti_fetch(s, {{cls_out, s->d_cls, sizeof(uint32_t) * s->C}}, who);
}

// ------------------------------------------------------------------------------------------------
// Gaussian observations: the object in observation mode (the kernels are gauss.hip's)

static double *ti_gmu(const stb_tindic_t *s) { return s->d_gpar; }
static double *ti_gtau(const stb_tindic_t *s) { return s->d_gpar + (size_t)s->maxK * s->obs_D; }
static double *ti_gmean(const stb_tindic_t *s) { return s->d_gpar + 2 * (size_t)s->maxK * s->obs_D; }
static double *ti_gQ(const stb_tindic_t *s) { return s->d_gpar + 3 * (size_t)s->maxK * s->obs_D; }

// what the calls of this section ask of the object before anything is queued; params: mu and tau must be defined
static int ti_obs_ready(stb_tindic_t *s, bool params, const char *who) {
  if (!s) return stb_fail("%s: null object", who);
  if (!s->d_x) return stb_fail("%s: the object holds no observations (stb_tindic_set_obs)", who);
  if (params && s->lik_bad)
    return stb_fail("%s: the last stb_tindic_sample_gauss failed and left the parameters undefined; draw again or set them", who);
  if (params && !s->g_have) return stb_fail("%s: no parameters yet (stb_tindic_set_gauss, stb_tindic_sample_gauss)", who);
  return 0;
}

extern "C" int stb_tindic_set_obs(stb_tindic_t *s, const double *x_host, unsigned D) {
  STB_ENTRY;
  const char *who = "stb_tindic_set_obs";
  if (!s) return stb_fail("%s: null object", who);
  stb_device_scope dev(s->dev);
  if (!x_host) {
    if (D != 0) return stb_fail("%s: D=%u without observations", who, D);
    if (hipStreamSynchronize(s->st) != hipSuccess) return STB_STREAM_FAIL(who);
    ti_drop_obs(s);
    ti_drop_cgs(s);
    if (s->d_cls) (void)hipFree(s->d_cls);
    if (s->d_lik) (void)hipFree(s->d_lik);
    s->d_cls = nullptr;
    s->d_lik = nullptr;
    s->cls_rows = s->lik_rows = s->lik_stride = 0;
    s->lik_bad = false;
    return 0;
  }
  if (stb_gs_check_shape(s->maxK, D, who)) return 1;
  if (s->C < 1 || s->C > 0xffffffffull) return stb_fail("%s: %llu customers (the matrix has a row per customer: 1 .. 2^32 - 1)", who, (unsigned long long)s->C);
  for (uint64_t j = 0; j < s->C * D; j++)
    if (!std::isfinite(x_host[j])) return stb_fail("%s: x[%llu]=%g (must be finite)", who, (unsigned long long)j, x_host[j]);
  std::vector<uint64_t> koff((size_t)s->I + 1);
  if (hipStreamSynchronize(s->st) != hipSuccess ||
      hipMemcpy(koff.data(), s->d_koff, sizeof(uint64_t) * (s->I + 1), hipMemcpyDeviceToHost) != hipSuccess)
    return STB_STREAM_FAIL(who);
  for (int i = 0; i < s->I; i++)
    if (koff[i + 1] - koff[i] != s->maxK)
      return stb_fail("%s: restaurant %d has K=%llu dishes and another %u; observation mode needs every K_i equal", who, i,
                      (unsigned long long)(koff[i + 1] - koff[i]), s->maxK);
  if (ti_materialise_cust(s, who)) return 1;
  const size_t KD = (size_t)s->maxK * D, cells = (size_t)s->C * s->maxK;
  double *dx = nullptr, *gpar = nullptr, *lik = nullptr;
  uint32_t *gn = nullptr, *cls = nullptr;
  int rc = 0;
  if (hipMalloc((void **)&dx, sizeof(double) * s->C * D) != hipSuccess || hipMalloc((void **)&gpar, sizeof(double) * 4 * KD) != hipSuccess ||
      hipMalloc((void **)&gn, sizeof(uint32_t) * s->maxK) != hipSuccess || hipMalloc((void **)&cls, sizeof(uint32_t) * s->C) != hipSuccess ||
      hipMalloc((void **)&lik, sizeof(double) * cells) != hipSuccess)
    rc = stb_fail("%s: out of device memory for %llu x %u observations and a %llu x %u matrix", who, (unsigned long long)s->C, D,
                  (unsigned long long)s->C, s->maxK);
  if (!rc && hipMemcpy(dx, x_host, sizeof(double) * s->C * D, hipMemcpyHostToDevice) != hipSuccess) rc = STB_STREAM_FAIL(who);
  if (!rc) rc = stb_gs_init(cls, s->C, lik, s->maxK, s->st);
  if (!rc && hipStreamSynchronize(s->st) != hipSuccess) rc = STB_STREAM_FAIL(who);
  if (rc) {
    void *fresh[] = {dx, gpar, gn, cls, lik};
    for (void *p : fresh)
      if (p) (void)hipFree(p);
    return 1;
  }
  // (new observations of the same D keep the observation held-out set and its accumulator; another D drops them)
  const bool keep_gh = s->d_ghoff && s->obs_D == D;
  uint64_t *ghoff = s->d_ghoff;
  double *gy = s->d_gy, *gacc = s->d_gacc;
  const uint64_t gHc = s->gHc;
  const unsigned gsamples = s->gsamples;
  if (keep_gh) {
    s->d_ghoff = nullptr;
    s->d_gy = s->d_gacc = nullptr;
  }
  ti_drop_obs(s);
  if (keep_gh) {
    s->d_ghoff = ghoff;
    s->d_gy = gy;
    s->d_gacc = gacc;
    s->gHc = gHc;
    s->gsamples = gsamples;
  }
  ti_drop_cgs(s);
  if (s->d_cls) (void)hipFree(s->d_cls);
  if (s->d_lik) (void)hipFree(s->d_lik);
  s->d_x = dx;
  s->obs_D = D;
  s->d_gpar = gpar;
  s->d_gn = gn;
  s->g_have = false;
  s->d_cls = cls;
  s->cls_rows = (unsigned)s->C;
  s->d_lik = lik;
  s->lik_rows = (unsigned)s->C;
  s->lik_stride = s->maxK;
  s->lik_bad = false;
  return 0;
}

extern "C" int stb_tindic_set_gauss(stb_tindic_t *s, const double *mu, const double *tau) {
  STB_ENTRY;
  const char *who = "stb_tindic_set_gauss";
  if (ti_obs_ready(s, false, who)) return 1;
  if (!mu || !tau) return stb_fail("%s: mu and tau are required", who);
  const size_t KD = (size_t)s->maxK * s->obs_D;
  for (size_t e = 0; e < KD; e++) {
    if (!std::isfinite(mu[e])) return stb_fail("%s: mu[%zu]=%g (must be finite)", who, e, mu[e]);
    if (!(tau[e] > 0.0) || !std::isfinite(tau[e])) return stb_fail("%s: tau[%zu]=%g (must be > 0 and finite)", who, e, tau[e]);
  }
  stb_device_scope dev(s->dev);
  if (hipStreamSynchronize(s->st) != hipSuccess || hipMemcpy(ti_gmu(s), mu, sizeof(double) * KD, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(ti_gtau(s), tau, sizeof(double) * KD, hipMemcpyHostToDevice) != hipSuccess)
    return STB_STREAM_FAIL(who);
  const int rc = stb_gs_lik(s->d_x, s->obs_D, s->C, ti_gmu(s), ti_gtau(s), s->maxK, s->d_lik, s->lik_stride, nullptr, s->st, who);
  s->g_have = rc == 0;
  s->lik_bad = rc != 0;
  return rc;
}

extern "C" int stb_tindic_get_gauss(stb_tindic_t *s, double *mu_out, double *tau_out) {
  STB_ENTRY;
  const char *who = "stb_tindic_get_gauss";
  if (ti_obs_ready(s, true, who)) return 1;
  const size_t KD = (size_t)s->maxK * s->obs_D;
  stb_device_scope dev(s->dev);
  return ti_fetch(s, {{mu_out, ti_gmu(s), sizeof(double) * KD}, {tau_out, ti_gtau(s), sizeof(double) * KD}}, who);
}

extern "C" int stb_tindic_sample_gauss(stb_tindic_t *s, const stb_gauss_prior_t *prior, uint64_t seed, uint64_t sweep,
                                       stb_gauss_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_tindic_sample_gauss";
  if (ti_obs_ready(s, false, who)) return 1;
  if (stb_gs_check_prior(prior, s->obs_D, who)) return 1;
  stb_device_scope dev(s->dev);
  bool touched = false;
  const int rc = stb_gs_step(s->d_x, s->obs_D, s->d_cust, s->C, s->maxK, prior, seed, sweep, s->d_gn, ti_gmean(s), ti_gQ(s), ti_gmu(s),
                             ti_gtau(s), s->d_lik, s->lik_stride, info, s->st, who, &touched);
  if (touched) {  // (a call that failed before its first launch left the parameters and the matrix as they were)
    s->lik_bad = rc != 0;
    s->g_have = rc == 0;
  }
  return rc;
}

extern "C" int stb_tindic_gauss_loglik(stb_tindic_t *s, double *total) {
  STB_ENTRY;
  const char *who = "stb_tindic_gauss_loglik";
  if (ti_obs_ready(s, true, who)) return 1;
  if (!total) return stb_fail("%s: total is required", who);
  stb_device_scope dev(s->dev);
  return stb_gs_loglik(s->d_x, s->obs_D, s->d_cust, s->C, ti_gmu(s), ti_gtau(s), s->maxK, total, nullptr, s->st, who);
}

extern "C" int stb_tindic_gauss_logml(stb_tindic_t *s, const stb_gauss_prior_t *prior, double *total) {
  STB_ENTRY;
  const char *who = "stb_tindic_gauss_logml";
  if (ti_obs_ready(s, false, who)) return 1;
  if (!total) return stb_fail("%s: total is required", who);
  if (stb_gs_check_prior(prior, s->obs_D, who)) return 1;
  stb_device_scope dev(s->dev);
  if (stb_gs_stats(s->d_x, s->obs_D, s->d_cust, s->C, s->maxK, s->d_gn, ti_gmean(s), ti_gQ(s), nullptr, s->st, who)) return 1;
  return stb_gs_logml(s->d_gn, ti_gmean(s), ti_gQ(s), s->maxK, s->obs_D, prior, total, s->st, who);
}

// ------------------------------------------------------------------------------------------------
// held-out points under Gaussian observations (the kernels are gauss.hip's and predict.hip's k_gh_sum)

extern "C" int stb_tindic_set_heldout_obs(stb_tindic_t *s, const uint64_t *hoff_host, const double *y_host) {
  STB_ENTRY;
  const char *who = "stb_tindic_set_heldout_obs";
  if (ti_obs_ready(s, false, who)) return 1;
  uint64_t Hc = 0;
  if (hoff_host) {
    if (hoff_host[0] != 0) return stb_fail("%s: hoff[0]=%llu (must be 0)", who, (unsigned long long)hoff_host[0]);
    for (int i = 0; i < s->I; i++)
      if (hoff_host[i + 1] < hoff_host[i]) return stb_fail("%s: hoff[%d] < hoff[%d]", who, i + 1, i);
    Hc = hoff_host[s->I];
    if (Hc && !y_host) return stb_fail("%s: the held-out points are required", who);
    for (uint64_t j = 0; j < Hc * s->obs_D; j++)
      if (!std::isfinite(y_host[j])) return stb_fail("%s: y[%llu]=%g (must be finite)", who, (unsigned long long)j, y_host[j]);
  }
  stb_device_scope dev(s->dev);
  int rc = 0;
  uint64_t *d_hoff = nullptr;
  double *d_y = nullptr, *d_acc = nullptr;
  if (hipStreamSynchronize(s->st) != hipSuccess) rc = STB_STREAM_FAIL(who);
  if (!rc && hoff_host) {
    const size_t Hs = Hc ? Hc : 1;
    if (hipMalloc((void **)&d_hoff, sizeof(uint64_t) * ((size_t)s->I + 1)) != hipSuccess ||
        hipMalloc((void **)&d_y, sizeof(double) * Hs * s->obs_D) != hipSuccess || hipMalloc((void **)&d_acc, sizeof(double) * 2 * Hs) != hipSuccess)
      rc = stb_fail("%s: out of device memory for %llu held-out points", who, (unsigned long long)Hc);
    if (!rc && (hipMemcpy(d_hoff, hoff_host, sizeof(uint64_t) * ((size_t)s->I + 1), hipMemcpyHostToDevice) != hipSuccess ||
                (Hc && hipMemcpy(d_y, y_host, sizeof(double) * Hc * s->obs_D, hipMemcpyHostToDevice) != hipSuccess)))
      rc = STB_STREAM_FAIL(who);
    if (!rc) rc = stb_gs_heldout_reset(d_acc, d_acc + Hs, Hs, s->st);
    if (!rc && hipStreamSynchronize(s->st) != hipSuccess) rc = STB_STREAM_FAIL(who);
  }
  if (rc) {  // the set the object had stays
    void *fresh[] = {d_hoff, d_y, d_acc};
    for (void *p : fresh)
      if (p) (void)hipFree(p);
    return rc;
  }
  ti_drop_gh(s);
  s->d_ghoff = d_hoff;
  s->d_gy = d_y;
  s->d_gacc = d_acc;
  s->gHc = Hc;
  s->gsamples = 0;
  return 0;
}

// the accumulator's halves: M, then A (a set without points holds one pair)
static double *ti_gaccM(const stb_tindic_t *s) { return s->d_gacc; }
static double *ti_gaccA(const stb_tindic_t *s) { return s->d_gacc + (s->gHc ? s->gHc : 1); }

static int ti_gh_ready(stb_tindic_t *s, const char *who) {
  if (ti_obs_ready(s, false, who)) return 1;
  if (!s->d_ghoff) return stb_fail("%s: no held-out points are set (stb_tindic_set_heldout_obs)", who);
  return 0;
}

extern "C" int stb_tindic_gauss_heldout(stb_tindic_t *s, double a, const double *bpar, unsigned flags, double *total,
                                        double *Hi_host, double *resp_host, stb_predict_info_t *info) {
  STB_ENTRY;
  const char *who = "stb_tindic_gauss_heldout";
  if (ti_obs_ready(s, true, who)) return 1;
  if (!total) return stb_fail("%s: total is required", who);
  if (!s->d_ghoff) return stb_fail("%s: no held-out points are set (stb_tindic_set_heldout_obs)", who);
  if (flags & ~STB_GH_ACCUMULATE) return stb_fail("%s: unknown flags 0x%x", who, flags);
  if (ti_pr_ready(s, a, bpar, 0, false, who)) return 1;
  const bool accumulate = (flags & STB_GH_ACCUMULATE) != 0;
  if (accumulate && s->gsamples == 0xffffffffu) return stb_fail("%s: the sample count is full (stb_tindic_gauss_heldout_reset)", who);
  stb_device_scope dev(s->dev);
  if (stb_hb_obj_stage(&s->hb, s->I, s->d_bpar, bpar, s->st, who)) return 1;
  const unsigned K = s->maxK;
  const size_t Hs = s->gHc ? s->gHc : 1;
  stb_pool_scratch sc(s->st);
  double *d_theta = nullptr, *d_ell = nullptr, *d_Hi = nullptr, *d_resp = nullptr;
  if (sc.take(&d_theta, sizeof(double) * (size_t)(s->I ? s->I : 1) * K) != hipSuccess ||
      (!accumulate && sc.take(&d_ell, sizeof(double) * Hs) != hipSuccess) ||
      (Hi_host && sc.take(&d_Hi, sizeof(double) * (size_t)(s->I ? s->I : 1)) != hipSuccess) ||
      (resp_host && sc.take(&d_resp, sizeof(double) * Hs * K) != hipSuccess))
    return stb_fail("%s: out of device memory for %llu held-out points", who, (unsigned long long)s->gHc);
  if (stb_pr_predict(ti_rest(s, a), ti_counts(s), stb_cust_ro{}, stb_lik_view{}, {d_theta, K}, 0, s->st, who)) return 1;
  if (stb_gs_heldout(d_theta, K, s->I, s->d_ghoff, s->d_gy, s->obs_D, ti_gmu(s), ti_gtau(s), K, d_ell, d_resp, d_resp ? K : 0,
                     accumulate ? ti_gaccM(s) : nullptr, accumulate ? ti_gaccA(s) : nullptr, s->st, who))
    return 1;
  if (d_resp && s->gHc &&
      hipMemcpyAsync(resp_host, d_resp, sizeof(double) * s->gHc * K, hipMemcpyDeviceToHost, s->st) != hipSuccess)
    return STB_STREAM_FAIL(who);
  const unsigned samples = accumulate ? ++s->gsamples : 1u;
  return sc.last(stb_pr_heldout_log(accumulate ? ti_gaccM(s) : d_ell, accumulate ? ti_gaccA(s) : nullptr, samples, s->d_ghoff, s->I,
                                    d_Hi, Hi_host, total, info, s->st, who));
}

extern "C" int stb_tindic_gauss_heldout_reset(stb_tindic_t *s) {
  STB_ENTRY;
  const char *who = "stb_tindic_gauss_heldout_reset";
  if (ti_gh_ready(s, who)) return 1;
  stb_device_scope dev(s->dev);
  if (stb_gs_heldout_reset(ti_gaccM(s), ti_gaccA(s), s->gHc ? s->gHc : 1, s->st)) return 1;
  s->gsamples = 0;
  return 0;
}

extern "C" int stb_tindic_gauss_heldout_get(stb_tindic_t *s, double *M_out, double *A_out, unsigned *samples) {
  STB_ENTRY;
  const char *who = "stb_tindic_gauss_heldout_get";
  if (ti_gh_ready(s, who)) return 1;
  stb_device_scope dev(s->dev);
  if (ti_fetch(s, {{M_out, ti_gaccM(s), sizeof(double) * s->gHc}, {A_out, ti_gaccA(s), sizeof(double) * s->gHc}}, who)) return 1;
  if (samples) *samples = s->gsamples;
  return 0;
}
