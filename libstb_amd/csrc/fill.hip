// fill.hip -- stb_fill_S / stb_fill_V: the device form of S_make / S_remake's table fill
// (reference lib/stable.c:321-388 for S, :451-482 for V).  Makes the plan of a fill (plan_fill: the form and its
// geometry, chosen once), lays out the workspace, launches, keeps the status of the last fill and the optional
// per-launch timing.
//
// Forms (fill_form below; kernels in their own translation units):
//   hb        k_fill_hb                    one launch: a spine that walks blocks of rows alone behind a halo + tile
//                                          workers (default wherever the row chain decides: tables of >= 512 rows
//                                          while the spine fits, e.g. 1-24 tables of 10^4 columns; floats and V ratios;
//                                          the fused aterms of 2-24 discounts)
//   grid      k_grid_hb                    the fused aterms whose walking waves sum their own strips (a dot request
//                                          with lists for strips, col0 = 4)
//   chain     k_fill_chain                 one launch per fill (small tables, many short ones, the fused aterms of
//                                          more than 24 discounts)
//   v-chain   k_fillv_chain                the V table on the reference's own recurrence, one launch
//   ck        k_fill_ck                    (ablation build only) one launch: recurrence-only spine + tile workers
//   pc        k_fill_pc                    launched per 128 rows (many tables; fallback of the one-launch forms)
//   rows-log  k_fill_rows                  the reference's own operation order (STB_FILL_LOGDOMAIN; 2^27 rows and more)
//   rows-V    k_fill_rows                  the V table per row block (STB_FILLV_CHAIN=0, a shared GPU)
//   ablation  the superseded forms of tools/ablation/ablation.hip in the library `make -C tools/ablation` builds
//   none      no kernel stores this kind at these bounds: the fill is refused with the plan's message

#include "stb_common.h"

static unsigned frontier_pitch(unsigned M) { return (unsigned)stb_align_up((size_t)M + 2, 64); }

// A cell grows per row by U^n_m = n - m a + S^n_{m-1}/S^n_m, and the last term reaches n(n-1)/2
// next to the diagonal, so the bound is N^2 per row, not N.  Significands start a period at 2^-700
// and may use 1450 bits.
int stb_period_rows(unsigned N) {
  int bits = 1;
  while ((1ull << bits) < (unsigned long long)N) bits++;
  const int p = 1450 / (2 * bits + 1);
  return p < 1 ? 1 : p;
}

// ------------------------------------------------------------------------------------------------
// per-launch timing: when armed, every fill kernel is launched with a begin/end event pair
// (hipExtLaunchKernelGGL stamps them with the dispatch's own start/stop, i.e. what a kernel trace
// reports), so a caller can obtain the kernel-only time of a fill without a profiler attached.
struct fill_prof {
  bool armed = false;
  int used = 0;
  hipEvent_t ev[2 * 4096];
  int made = 0;
  double span_ms = 0.0;
};
static thread_local fill_prof g_prof;

void stb_prof_events(hipEvent_t *e0, hipEvent_t *e1) {
  *e0 = *e1 = nullptr;
  if (!g_prof.armed || g_prof.used + 2 > 2 * 4096) return;
  while (g_prof.made < g_prof.used + 2) {
    if (hipEventCreate(&g_prof.ev[g_prof.made]) != hipSuccess) return;
    g_prof.made++;
  }
  *e0 = g_prof.ev[g_prof.used];
  *e1 = g_prof.ev[g_prof.used + 1];
  g_prof.used += 2;
}

extern "C" void stb_fill_profile_begin(void) {
  g_prof.armed = true;
  g_prof.used = 0;
}

extern "C" int stb_fill_profile_end(double *kernel_ms_total, int *launches) {
  STB_ENTRY;
  // caller must have synchronised the stream(s) the fills ran on
  g_prof.armed = false;
  double tot = 0.0;
  const int n = g_prof.used / 2;
  for (int i = 0; i < n; i++) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]));
    tot += ms;
  }
  // device time from the first launch's start to the last end: what the launches took together when
  // some of them ran side by side on forked streams (the sum above counts such time twice)
  double span = 0.0;
  for (int i = 0; i < n; i++) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_prof.ev[0], g_prof.ev[2 * i + 1]) == hipSuccess && ms > span) span = ms;
  }
  g_prof.span_ms = span;
  if (kernel_ms_total) *kernel_ms_total = tot;
  if (launches) *launches = n;
  g_prof.used = 0;
  return 0;
}

extern "C" double stb_fill_profile_span(void) { return g_prof.span_ms; }

// ------------------------------------------------------------------------------------------------
// workspace

static size_t ws_head(unsigned M, int D) {  // discounts + frontier
  const size_t W = frontier_pitch(M);
  return stb_align_up((size_t)D * sizeof(double), 256) + stb_align_up((size_t)D * 2 * W * (sizeof(double) + sizeof(int)), 256);
}

static size_t fill_workspace_need(unsigned N, unsigned M, int D) {
  size_t form = stb_chain_workspace(N, M, D);
  const size_t ck = stb_launch_ck ? stb_ck_workspace(N, M, D) : 0;
  if (ck > form) form = ck;
  const size_t hb = stb_hb_workspace(N, M, D);
  if (hb > form) form = hb;
  const size_t gr = stb_grid_workspace(N, M, D);
  if (gr > form) form = gr;
  if (stb_ablation_workspace) {
    const size_t ab = stb_ablation_workspace(N, M, D);
    if (ab > form) form = ab;
  }
  return ws_head(M, D) + form + 512;
}

// enough for D tables and for any smaller batch run in the same workspace
extern "C" size_t stb_fill_workspace_bytes(unsigned N, unsigned M, int D) {
  size_t need = fill_workspace_need(N, M, D);
  for (int d2 = 1; d2 < D && d2 <= 4096; d2++) {  // (the block shape, hence the edge streams, depends on the batch)
    const size_t n2 = fill_workspace_need(N, M, d2);
    if (n2 > need) need = n2;
  }
  return need;
}

// ------------------------------------------------------------------------------------------------
// the plan of a fill: which form runs, with what geometry, and what may be done about it afterwards.  plan_fill makes it
// from the request, once; the fill launches it, stb_fill_tuning and stb_fill_takes_kind report it, and the fallback of
// stb_fill_status_of asks it for the producer/consumer form's geometry -- so that no two of them can disagree.

extern "C" int stb_default_variant(void) {
  const int v = stb_env_int("STB_FILL_VARIANT", STB_FILL_SCALED);
  return (v == STB_FILL_LOGDOMAIN || v == STB_FILL_SCALED_STEP || v == STB_FILL_SPLIT || v == STB_FILL_FUSED ||
          v == STB_FILL_PC || v == STB_FILL_CHAIN || v == STB_FILL_CHAINX || v == STB_FILL_CK || v == STB_FILL_HB)
             ? v
             : STB_FILL_SCALED;
}

extern "C" int stb_has_ablation(void) { return stb_ablation_fill != nullptr; }

enum fill_form { FORM_NONE, FORM_ROWS_LOG, FORM_ROWS_V, FORM_PC, FORM_CHAIN, FORM_VCHAIN, FORM_CK, FORM_HB, FORM_GRID, FORM_ABLATION };

struct fill_plan {
  fill_form form = FORM_NONE;
  char why[200] = "";          // FORM_NONE: the refusal
  int C = 0, R = 0, H = 0, Wv = 0;  // pc and rows: columns per lane, rows per launch, halo columns, own columns of a strip
  // what stb_fill_tuning reports: 2 producer/consumer, 3 chain, 4 checkpointed, 6 halo blocks, 5 another form; the pc
  // form's report is its geometry, the row and ablation forms' is the nominal STB_FILL_C / STB_FILL_R it has always been
  int code = 5, rep_C = 0, rep_R = 0, launches = 1;
  bool hb_range = false;       // the halo-block form's range test said yes for this kind (stb_fill_takes_kind)
  bool s_table = true, can_fall_back = false, stamped = false;  // for last_fill
};

// The ONLY place of this file that reads the route environment (STB_HB*, STB_CK*, STB_CHAIN_MAX_COLS, STB_FILLV_*,
// STB_PC_CONSUMERS, STB_FILL_C, STB_FILL_R) and the shared-GPU mode -- on every call: tests and tools change them
// between calls.  report: also the strip and block shape of a one-launch form, which only stb_fill_tuning asks for (a
// geometry evaluation the fill itself has no use for).
static fill_plan plan_fill(const fill_request &q, bool report = false) {
  const unsigned N = q.N, M = q.M;
  const int D = q.D;
  const bool vtable = (q.kind & 2) != 0;
  const char *who = vtable ? "stb_fill_V" : "stb_fill_S";
  fill_plan P;
  P.s_table = !vtable;
  const bool big = N >= (1u << 27);  // the block-floating forms bound the scale between lanes for N < 2^27 (see k_fill_pc)
  // (a GPU shared with other processes: the forms without waits between workgroups, see abi.hip)
  const bool shared = stb_shared_gpu();

  // The halo-block form (a spine that walks blocks of rows alone behind a halo + tile workers) is the fast one
  // wherever the ROW CHAIN, not the chip's throughput, decides.  Chosen for tables of >= 512 rows while the batch's
  // spine workgroups leave the tile workers room (stb_spine_room: 24 tables of 10^4 columns, 64 of 4000) and the batch
  // stays below 1.25 x 10^9 cells.  (MI355X, tools/ab_ck.py, ms: N = M = 10^4: 1 table 0.32-0.33 against 0.70 chain /
  // 0.71 checkpointed, 2 tables 0.365 against 0.72, 4 tables 0.48-0.50 against 0.76, 8 tables 0.73-0.75 against
  // 0.90-0.93, 16 tables 1.34-1.50 against 1.51-1.65, 24 tables 2.13 against 2.37 pc, 32 tables 4.3 against 2.9 pc;
  // N = M = 4000: 1 table 0.15-0.16 against 0.28 chain, 3 tables 0.158 against 0.289, 8 tables 0.20 against 0.34,
  // 64 tables 0.99 against 1.02 pc; N = M = 2000: 1 / 3 tables 0.095 / 0.10 against 0.15, 64 tables 0.32 against
  // 0.37 chain, 128 tables 0.61 against 0.55 pc; N = M = 1000: 1 / 8 / 16 / 32 / 64 tables 0.06 / 0.067 / 0.075 /
  // 0.087 / 0.122 against 0.08 / 0.086 / 0.089 / 0.090 / 0.118; N = M = 512: 0.05 = chain; N = M = 300: 0.05
  // against 0.04; N = 3000, M = 200, 100 tables 0.23 against 0.25; N = 50000, M = 100, 4 tables 1.18 against 2.32;
  // N = M = 20000: 1 table 0.75 against 1.44.)
  // It is also the only form that stores floats (S_FLOAT) and V ratios: its tile workers narrow or divide what they hold
  // in double before the store.  One range test for all four kinds, with these differences:
  //   STB_HB=0 and the shared mode switch every kind off;
  //   STB_HB=1 forces kind 0 only, wherever the geometry exists (kinds 1-3 keep the thresholds);
  //   a pending dot request keeps the automatic choice away from this form (the evaluation names its form itself).
  auto hb_range = [&]() -> bool {
    const int force = stb_env_int("STB_HB", -1);
    if (force == 0 || shared || q.dot) return false;
    if (force > 0 && q.kind == 0) return stb_hb_eligible(N, M, D);
    const uint64_t cells = (uint64_t)D * stb_table_cells(N, M);
    if (N < (unsigned)stb_env_int("STB_HB_MIN_N", 512) || cells > (uint64_t)stb_env_int("STB_HB_MAX_MCELLS", 1250) * 1000000ull) return false;
    if (q.kind && !stb_hb_eligible_out(N, M, D, q.kind)) return false;
    // (bounds the form does not take at all have a spine of 2^32 - 1 workgroups)
    return stb_hb_spine(N, M, D) <= stb_spine_room("STB_HB_MAX_SPINE");
  };
  // the chain form where the choice is not free: a variant that asks for it, or for a form that does not take these bounds
  auto chain_or_next = [&]() { return (N >= 3 && !big) ? FORM_CHAIN : (N < 3 ? FORM_PC : FORM_ROWS_LOG); };
  auto refuse = [&](const char *fmt, auto... args) {
    P.form = FORM_NONE;
    snprintf(P.why, sizeof P.why, fmt, args...);
  };
  auto nominal_report = [&]() {  // (the row and ablation forms: see fill_plan)
    P.rep_C = stb_env_int("STB_FILL_C", 2);
    P.rep_R = std::max(1, stb_env_int("STB_FILL_R", 64));
  };
  auto rows_halo = [&]() {  // the row kernels' strips: halo columns in whole lanes
    P.H = (P.R + P.C - 1) / P.C * P.C;
    P.Wv = 64 * P.C - P.H;
  };

  if (q.kind != 0) {
    // floats, and the V table from the S recurrence's own cells (one division per cell, off the serial path: 1e-10 of
    // the reference; STB_FILLV_EXACT=1 / stb_fill_V_exact keep the V table on the reference's own recurrence, bit for bit)
    P.hb_range = hb_range();
    if (P.hb_range && !(q.kind == 2 && (q.v_exact || stb_env_int("STB_FILLV_EXACT", 0)))) P.form = FORM_HB;
    else if (q.kind != 2)
      refuse("%s: no kernel stores %s for N=%u M=%u D=%d (the caller narrows a double table instead)", who,
             q.kind == 1 ? "floats" : "float V ratios", N, M, D);
    else P.form = (stb_env_int("STB_FILLV_CHAIN", 1) && !shared) ? FORM_VCHAIN : FORM_ROWS_V;
  } else {
    switch (q.variant) {
      case STB_FILL_LOGDOMAIN: P.form = FORM_ROWS_LOG; break;
      case STB_FILL_PC: P.form = big ? FORM_ROWS_LOG : FORM_PC; break;
      case STB_FILL_CHAIN: P.form = chain_or_next(); break;
      case STB_FILL_CK: P.form = (stb_launch_ck && stb_ck_eligible(N, M, D)) ? FORM_CK : chain_or_next(); break;
      case STB_FILL_HB: P.form = stb_hb_eligible(N, M, D) ? FORM_HB : chain_or_next(); break;
      case STB_FILL_CHAINX:  // (its converter blocks need a compute unit per 64-column chunk)
        P.form = (D <= 2 && N >= 3 && !big) ? FORM_ABLATION : chain_or_next();
        break;
      case STB_FILL_SCALED_STEP:
      case STB_FILL_SPLIT:
      case STB_FILL_FUSED: P.form = FORM_ABLATION; break;
      default: {
        // STB_FILL_SCALED picks the form itself.  Outside the halo-block form's range, by how many table columns are
        // in flight: the chain form (one launch, no halo) up to STB_CHAIN_MAX_COLS columns over all tables, the
        // producer/consumer form beyond.  (MI355X, tools/ab_chain.py: 16 tables of 10^4 columns 2.01 ms pc against
        // 2.11 chain, 12 tables 1.78 against 1.68; 32 tables of 4000 columns 0.78 against 0.70.)
        // The checkpointed form (spine + tile workers) is chosen on request only since the halo-block form took over
        // the batches it was made for: STB_CK=1 wherever it is eligible, STB_CK=-1 between STB_CK_MIN_MCELLS and
        // STB_CK_MAX_MCELLS million cells; what the halo-block form leaves -- very many mid-sized tables -- is the
        // producer/consumer form's: 64 tables of 4000 columns 1.04 against 1.17 ms, 128 of 2000 0.56 against 0.68.
        auto ck_asked = [&]() -> bool {
          const int ck = stb_env_int("STB_CK", 0);
          if (ck == 0 || q.dot || !stb_launch_ck || !stb_ck_eligible(N, M, D)) return false;
          const uint64_t cells = (uint64_t)D * stb_table_cells(N, M);
          return ck > 0 || (cells >= (uint64_t)stb_env_int("STB_CK_MIN_MCELLS", 40) * 1000000ull &&
                            cells <= (uint64_t)stb_env_int("STB_CK_MAX_MCELLS", 1000) * 1000000ull);
        };
        if (big) P.form = FORM_ROWS_LOG;
        else if (shared && !q.dot) P.form = FORM_PC;
        else if ((P.hb_range = hb_range())) P.form = FORM_HB;
        else if (ck_asked()) P.form = FORM_CK;
        else
          P.form = ((uint64_t)D * M <= (uint64_t)stb_env_int("STB_CHAIN_MAX_COLS", 150000) && N >= 3) ? FORM_CHAIN : FORM_PC;
      }
    }
    // (the walking waves sum their strips' listed cells themselves: grid_hb.hip)
    if (P.form == FORM_HB && q.dot && q.dot->col0 == 4) P.form = FORM_GRID;
    if (q.dot && P.form != FORM_CHAIN && P.form != FORM_CK && P.form != FORM_HB && P.form != FORM_GRID)
      refuse("%s: the fused evaluation needs the chain or the checkpointed form", who);
    if (P.form == FORM_ABLATION) {
      nominal_report();
      if (!stb_ablation_fill) refuse("%s: fill variant %d is one of the superseded forms, which this build does not carry "
                                     "(make -C tools/ablation builds a library that does)", who, q.variant);
    }
  }

  switch (P.form) {
    case FORM_HB:
    case FORM_GRID:
      P.code = 6;
      P.stamped = P.form == FORM_HB;
      // (k_fill_pc stores log S in double only, and no table at all for an evaluation: those callers repeat in another way)
      P.can_fall_back = q.kind == 0 && !q.dot;
      if (report) stb_hb_tuning(N, M, D, &P.rep_C, &P.rep_R);  // own columns of a strip, rows of a block
      break;
    case FORM_CHAIN:
      P.code = 3;
      P.can_fall_back = !q.dot;
      P.rep_R = (int)N;
      if (report) stb_chain_tuning(N, M, D, &P.rep_C);  // columns per strip
      break;
    case FORM_VCHAIN:
      P.code = 3;
      P.rep_R = (int)N;
      break;
    case FORM_CK:
      P.code = 4;
      P.can_fall_back = !q.dot;
      if (report) stb_ck_tuning(N, M, D, &P.rep_C, &P.rep_R);  // columns of a wave strip, rows of a tile
      break;
    case FORM_PC:  // rows 2..N in launches of R rows; H = 256 - 64 * consumer waves; R <= H
      P.code = 2;
      P.C = 4;
      P.H = 256 - 64 * (stb_env_int("STB_PC_CONSUMERS", 2) == 3 ? 3 : 2);
      P.R = std::max(1, std::min(P.H, stb_env_int("STB_FILL_R", P.H)));
      P.Wv = 256 - P.H;
      P.rep_C = P.C;
      P.rep_R = P.R;
      break;
    case FORM_ROWS_V:
      P.C = 2;
      P.R = std::max(1, std::min(126, stb_env_int("STB_FILL_R", 48)));
      rows_halo();
      P.rep_C = P.C;
      P.rep_R = P.R;
      break;
    case FORM_ROWS_LOG: {
      nominal_report();
      const bool few = (uint64_t)D * M < 40000;
      P.C = stb_env_int("STB_FILL_C", few ? 1 : 2);
      P.R = std::max(1, stb_env_int("STB_FILL_R", few ? 48 : 64));
      if (P.C != 1 && P.C != 2 && P.C != 4) {
        refuse("%s", "STB_FILL_C must be 1, 2 or 4");
        break;
      }
      rows_halo();
      if (P.H > 64 * P.C - P.C) refuse("STB_FILL_R=%d too large for C=%d", P.R, P.C);
      break;
    }
    default: break;  // (the ablation forms' report is made above, a refusal has none)
  }
  if ((P.code == 2 || P.code == 5) && P.rep_R > 0) P.launches = ((int)N - 1 + P.rep_R - 1) / P.rep_R;
  return P;
}

extern "C" int stb_fill_tuning(unsigned N, unsigned M, int D, int *C_out, int *R_out, int *launches) {
  const fill_plan P = plan_fill({N, M, D, stb_default_variant(), 0, false, nullptr}, true);
  if (C_out) *C_out = P.rep_C;
  if (R_out) *R_out = P.rep_R;
  if (launches) *launches = P.launches;
  return P.code;
}

// The halo-block form also stores floats (S_FLOAT) and V ratios -- the only form that does: whether a fill of this
// kind is in its range (what stb_fill_Sf / _Vf need, and what sends stb_fill_V to it)
extern "C" int stb_fill_takes_kind(unsigned N, unsigned M, int D, int kind) {
  return plan_fill({N, M, D, STB_FILL_SCALED, kind, false, nullptr}).hb_range ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// the fill

// what the last fill of this thread was, so that stb_fill_status can wait for it, report a chain
// form that gave up, and repeat the fill with the producer/consumer form (struct in stb_common.h: an
// object that queues a fill and checks it later, possibly after other fills, keeps a copy).  These are results
// a later call of the API reads back, not arguments: what a fill is asked travels in its fill_request.
static thread_local last_fill g_last;
static thread_local unsigned g_fallbacks = 0;

extern "C" unsigned stb_fill_fallbacks(void) { return g_fallbacks; }

void stb_fill_last(last_fill *out) { *out = g_last; }

// Waits for the fill on ITS stream (a copy on the null stream does not wait for a non-blocking stream,
// and torch's side streams are non-blocking), reads the header, and on a give-up repeats the fill with
// the form that has no waits between workgroups.
int stb_fill_status_of(last_fill *lf) {
  if (!lf->hdr) return 0;
  unsigned h[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(h, lf->hdr, lf->stamped ? sizeof(h) : 4 * sizeof(unsigned), hipMemcpyDeviceToHost, lf->st));
  HIPCHK(hipStreamSynchronize(lf->st));
  if (lf->stamped) {
    // (the halo-block form stamps its first workgroup's start and its spine waves' ends, 100 MHz ticks)
    const unsigned long long t0 = (unsigned long long)h[STB_HDR_T0] | ((unsigned long long)h[STB_HDR_T0 + 1] << 32);
    const unsigned long long t1 = (unsigned long long)h[STB_HDR_T1] | ((unsigned long long)h[STB_HDR_T1 + 1] << 32);
    if (t0 && t1 > t0)
      stb_note_span((double)(t1 - t0) * 1e-5, 1e-3 * (100.0 + 0.05 * (double)lf->A.N * (1.0 + (double)lf->D / 8.0)), "a table fill (stb_fill_S)");
  }
  if (h[1] == 0) return 0;
  stb_fail("%s: the fill gave up waiting for a neighbour block (code 0x%x, block %u of table %u)",
           lf->s_table ? "stb_fill_S" : "stb_fill_V", h[1], h[2] & 0xffffu, h[2] >> 16);
  if (!lf->can_fall_back || stb_env_int("STB_CHAIN_NO_FALLBACK", 0)) {
    lf->hdr = nullptr;
    return 1;
  }
  lf->hdr = nullptr;
  lf->fell_back = true;
  g_fallbacks++;
  fill_args A = lf->A;
  const fill_plan P = plan_fill({A.N, A.M, lf->D, STB_FILL_PC, 0, false, nullptr});
  A.R = P.R;
  A.H = P.H;
  A.Wv = P.Wv;
  if (stb_launch_pc(A, lf->D, lf->st)) return 1;
  HIPCHK(hipStreamSynchronize(lf->st));
  return 0;
}

extern "C" int stb_fill_status(void) {
  STB_ENTRY;
  return stb_fill_status_of(&g_last);
}

__global__ void k_set_a(stb_a64 av, double *a, int D) {
  if ((int)threadIdx.x < D) a[threadIdx.x] = av.v[threadIdx.x];
}
int stb_a_flush(const fill_args &A, a_pending *pend, hipStream_t st) {
  if (!pend || pend->n <= 0) return 0;
  hipLaunchKernelGGL(k_set_a, dim3(1), dim3(64), 0, st, pend->av, const_cast<double *>(A.a), pend->n);
  pend->n = 0;
  HIPCHK(hipGetLastError());
  return 0;
}

int stb_fill(const fill_request &q, const double *a_host, double *d_tables, uint64_t table_stride, double *d_S1, uint64_t s1_stride,
             void *d_ws, size_t ws_bytes, hipStream_t st) {
  const unsigned N = q.N, M = q.M;
  const int D = q.D;
  const bool vtable = (q.kind & 2) != 0;
  const char *who = vtable ? "stb_fill_V" : "stb_fill_S";
  g_last = last_fill();  // whatever this thread filled before is no longer "the last fill"
  if (D < 1) return stb_fail("%s: D=%d", who, D);
  if (N < 2 || M < 2) return stb_fail("%s: bounds N=%u M=%u too small", who, N, M);
  if (!a_host || !d_tables || !d_ws || (!vtable && !d_S1)) return stb_fail("%s: null pointer", who);
  if (ws_bytes < fill_workspace_need(N, M, D))
    return stb_fail("%s: workspace %zu < %zu", who, ws_bytes, fill_workspace_need(N, M, D));
  // (for every D: with one table the stride is the caller's slab size, and nothing else stops a fill past its end)
  const uint64_t need = vtable ? stb_vtable_elems(N, M) : stb_table_elems(N, M);
  if (table_stride < need || (!vtable && s1_stride < N)) return stb_fail("%s: strides too small", who);
  if (D > 1 && (table_stride & 1)) return stb_fail("%s: table stride must be even", who);
  for (int d = 0; d < D; d++)
    if (!(a_host[d] >= 0.0 && a_host[d] < 1.0)) return stb_fail("%s: discount %g outside [0,1)", who, a_host[d]);

  fill_args A;
  memset(&A, 0, sizeof(A));
  char *ws = (char *)d_ws;
  A.a = (const double *)ws;
  ws += stb_align_up((size_t)D * sizeof(double), 256);
  A.W = frontier_pitch(M);
  A.fm = (double *)ws;
  A.fe = (int *)(ws + (size_t)D * 2 * A.W * sizeof(double));
  ws = (char *)d_ws + ws_head(M, D);
  const size_t ws_left = ws_bytes - ws_head(M, D);
  A.tables = d_tables;
  A.tstride = table_stride;
  A.S1 = d_S1;
  A.s1stride = s1_stride;
  A.N = N;
  A.M = M;
  if (stb_logtab(&A.lt)) return 1;

  const fill_plan P = plan_fill(q);
  if (P.form == FORM_NONE) return stb_fail("%s", P.why);
  A.R = P.R;
  A.H = P.H;
  A.Wv = P.Wv;

  a_pending pend;  // (the launcher's first kernel writes them, or stb_a_flush below)
  if (D <= 64 && stb_env_int("STB_A_BY_VALUE", 1)) {
    for (int d = 0; d < D; d++) pend.av.v[d] = a_host[d];
    pend.n = D;
  } else {
    HIPCHK(hipMemcpyAsync((void *)A.a, a_host, (size_t)D * sizeof(double), hipMemcpyHostToDevice, st));
  }
  // (stb_launch_hb hands them to its k_prep, stb_launch_grid flushes them itself; the ablation library's launchers
  // know nothing of them)
  if (P.form != FORM_HB && P.form != FORM_GRID && stb_a_flush(A, &pend, st)) return 1;

  unsigned *hdr = nullptr;  // (stays null for the forms that cannot give up)
  int rc = 1;
  switch (P.form) {
    case FORM_HB: rc = stb_launch_hb(A, D, ws, ws_left, q.dot, &pend, &hdr, st, q.kind); break;
    case FORM_GRID: rc = stb_launch_grid(A, D, ws, ws_left, q.dot, &pend, &hdr, st); break;
    case FORM_CHAIN: rc = stb_launch_chain(A, D, ws, ws_left, q.dot, &hdr, st); break;
    case FORM_CK: rc = stb_launch_ck(A, D, ws, ws_left, q.dot, &hdr, st); break;
    case FORM_VCHAIN: rc = stb_launch_vchain(A, D, ws, ws_left, &hdr, st); break;
    case FORM_PC: rc = stb_launch_pc(A, D, st); break;
    case FORM_ROWS_LOG: rc = stb_launch_rows(A, D, P.C, STB_ROWS_LOGDOM, st); break;
    case FORM_ROWS_V: rc = stb_launch_rows(A, D, P.C, STB_ROWS_VRATIO, st); break;
    case FORM_ABLATION: rc = stb_ablation_fill(A, D, q.variant, ws, ws_left, &hdr, st); break;
    case FORM_NONE: break;
  }
  if (rc) return 1;
  g_last.hdr = hdr;
  g_last.A = A;
  g_last.D = D;
  g_last.st = st;
  g_last.s_table = P.s_table;
  g_last.can_fall_back = P.can_fall_back;
  g_last.stamped = P.stamped;
  return 0;
}

extern "C" int stb_fill_S(const double *a_host, int D, unsigned N, unsigned M, double *d_tables, uint64_t table_stride,
                          double *d_S1, uint64_t s1_stride, void *d_ws, size_t ws_bytes, int variant, void *stream) {
  STB_ENTRY;
  return stb_fill({N, M, D, variant, 0, false, nullptr}, a_host, d_tables, table_stride, d_S1, s1_stride, d_ws, ws_bytes, (hipStream_t)stream);
}

// S_FLOAT storage written once, as floats (lib/stable.c:389-449: the recurrence in double, the stored value a float):
// D float slabs with the double slab's element offsets.  Fails (and says so) where only the double forms apply:
// stb_fill_takes_kind(N, M, D, 1) tells beforehand.
extern "C" int stb_fill_Sf(const double *a_host, int D, unsigned N, unsigned M, float *d_tables, uint64_t table_stride,
                           double *d_S1, uint64_t s1_stride, void *d_ws, size_t ws_bytes, void *stream) {
  STB_ENTRY;
  return stb_fill({N, M, D, STB_FILL_SCALED, 1, false, nullptr}, a_host, reinterpret_cast<double *>(d_tables), table_stride, d_S1, s1_stride,
                  d_ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int stb_fill_Vf(const double *a_host, int D, unsigned N, unsigned M, float *d_vtables, uint64_t vtable_stride,
                           void *d_ws, size_t ws_bytes, void *stream) {
  STB_ENTRY;
  return stb_fill({N, M, D, STB_FILL_SCALED, 3, false, nullptr}, a_host, reinterpret_cast<double *>(d_vtables), vtable_stride, nullptr, 0,
                  d_ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int stb_fill_V(const double *a_host, int D, unsigned N, unsigned M, double *d_vtables, uint64_t vtable_stride,
                          void *d_ws, size_t ws_bytes, void *stream) {
  STB_ENTRY;
  return stb_fill({N, M, D, STB_FILL_SCALED, 2, false, nullptr}, a_host, d_vtables, vtable_stride, nullptr, 0, d_ws, ws_bytes, (hipStream_t)stream);
}

// the V table on the reference's own recurrence (k_fillv_chain: two dependent divisions a row, bit for bit the
// reference's table), whatever the size: what stb_fill_V does by itself below 512 rows and under STB_FILLV_EXACT=1
extern "C" int stb_fill_V_exact(const double *a_host, int D, unsigned N, unsigned M, double *d_vtables, uint64_t vtable_stride,
                                void *d_ws, size_t ws_bytes, void *stream) {
  STB_ENTRY;
  return stb_fill({N, M, D, STB_FILL_SCALED, 2, true, nullptr}, a_host, d_vtables, vtable_stride, nullptr, 0, d_ws, ws_bytes, (hipStream_t)stream);
}
