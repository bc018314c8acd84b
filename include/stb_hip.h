/*
 * stb_hip.h -- additive C ABI of libstb_amd for device-resident / batched use of the hot path.
 *
 * The reference (wbuntine/libstb) has no such interface: its only API is the scalar host one in
 * stable.h / psample.h, which this library also exports unchanged (see those headers).  The entry
 * points below expose the same arithmetic -- the table fill of S_remake_part
 * (reference lib/stable.c:321-388), the S_S gather-sum and restaurant terms of aterms
 * (lib/samplea.c:46-83) and the lgamma sum of bterms (lib/sampleb.c:33-41) -- for callers that keep
 * tables and (n,t) groups resident in HBM and evaluate many discounts at once (SURVEY 8b "new,
 * additive C ABI").  Plain pointers and sizes only; every device pointer is a hipMalloc'd (or
 * torch-allocated) address on the current device; `stream` is a hipStream_t passed as void*
 * (NULL = default stream).  All functions return 0 on success, non-zero on failure with the
 * message available from stb_last_error(); nothing here falls back to the CPU.
 */
#ifndef STB_HIP_H
#define STB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- diagnostics ---- */
const char *stb_last_error(void);
int stb_device_count(void);                 /* 0 when no usable GPU */
int stb_device_name(char *buf, int len);    /* name + gcnArch of the current device */

/* ---- which GPU.  The reference is a host library and has no such notion; SURVEY 5 asks for a
 * device-id knob.  A thread picks the GPU for the objects it creates (S_make, stb_groups_create) with
 * stb_set_device(k); without it STB_DEVICE=k in the environment decides; without either the HIP
 * runtime's current device is used.  Tables and group sets remember their device: every later call
 * on them (S_remake, growth inside S_S / S_V, S_free, stb_groups_aterms ...) switches to it and puts
 * the caller's current device back.  stb_device_enter / stb_device_leave are that switch, for
 * callers of the raw-pointer entry points below (which run on the current device). ---- */
int stb_set_device(int dev);                /* non-zero if dev is not a usable device */
int stb_get_device(void);                   /* the device the next S_make / stb_groups_create will use */
int stb_device_enter(int dev);              /* make dev current; returns what to pass to stb_device_leave */
void stb_device_leave(int prev);

/* ---- memory and stream helpers, so that C / FFI callers need no HIP headers ---- */
void *stb_device_malloc(size_t bytes);                 /* hipMalloc; NULL on failure */
void stb_device_free(void *p);
void *stb_host_malloc(size_t bytes);                   /* pinned (hipHostMalloc); NULL on failure */
void stb_host_free(void *p);
void *stb_host_malloc_huge(size_t bytes);              /* pinned AND on 2 MB pages (aligned_alloc + madvise + hipHostRegister); NULL on failure */
void stb_host_free_huge(void *p);
int stb_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes, void *stream);
int stb_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes, void *stream);
int stb_stream_sync(void *stream);
void *stb_stream_create(void);                         /* a stream that does not synchronise with the null stream; NULL on failure */
void stb_stream_destroy(void *stream);
void *stb_event_create(void);
void stb_event_destroy(void *ev);
int stb_event_record(void *ev, void *stream);
int stb_event_wait(void *ev);                          /* blocks the calling thread */
int stb_event_done(void *ev);                          /* 1 done, 0 not yet, -1 error */

/* ---- layout of one table slab (see libstb_amd/csrc/stb_layout.h) ---- */
uint64_t stb_cells(unsigned N, unsigned M);        /* stored values: sum_{n=3..N} min(n-2,M-1) */
uint64_t stb_elems(unsigned N, unsigned M);        /* doubles to allocate (rows start 16B aligned) */
uint64_t stb_rowoff(unsigned n, unsigned M);       /* element offset of row n; value (n,m) at +m-2 */
uint64_t stb_vcells(unsigned N, unsigned M);       /* same three for the V (ratio) table */
uint64_t stb_velems(unsigned N, unsigned M);
uint64_t stb_vrowoff(unsigned n, unsigned M);

/* growth policy of the table object (reference lib/stable.c:564-630, S_extend): given current and
 * maximum bounds and the (n+1, m+1) an accessor asks for, the bounds the table grows to.  Pure
 * integer function; S_S / S_V use it internally, exported so callers can pre-size. */
void stb_extend_policy(unsigned usedN, unsigned usedM, unsigned maxN, unsigned maxM, int N, int M,
                       unsigned *newN, unsigned *newM);

/* ---- K1/K2: fill D log-Stirling tables (D=1: S_remake; D>1: the batched-discount mode) ----
 * a_host[D]            discounts (host memory), 0 <= a < 1 (a = 0: the unsigned Stirling numbers of the first kind)
 * d_tables             D slabs of stb_elems(N,M) doubles, slab d at d_tables + d*table_stride
 * d_S1                 D vectors of N doubles (S1[n-1] = log S^n_{1,a}), vector d at + d*s1_stride
 * d_ws / ws_bytes      scratch of at least stb_fill_workspace_bytes(N,M,D)
 * variant              STB_FILL_SCALED (default), STB_FILL_LOGDOMAIN or STB_FILL_SCALED_STEP
 */
#define STB_FILL_SCALED 0      /* linear-domain recurrence, block-floating cells, table log; picks HB, CHAIN or PC by size */
#define STB_FILL_LOGDOMAIN 1   /* logadd(log(.)+., .) per cell, operation order of lib/stable.c:380-388 */
#define STB_FILL_SCALED_STEP 2 /* (ablation build) linear-domain, renormalised every row, libm-grade log */
#define STB_FILL_SPLIT 3       /* (ablation build) recurrence kernel + in-place log conversion on auxiliary streams */
#define STB_FILL_FUSED 4       /* (ablation build) recurrence and log in one kernel, launched per row block */
#define STB_FILL_PC 5          /* one producer wave (recurrence) + consumer waves (logs) per column block, via LDS */
#define STB_FILL_CHAIN 6       /* one launch: column blocks keep their columns for all rows, edges handed on in HBM */
#define STB_FILL_CHAINX 7      /* (ablation build) the chain alone in its blocks; logs by converter blocks (D <= 2) */
#define STB_FILL_CK 8          /* one launch: a recurrence-only spine publishes edges and checkpoints, tile workers convert and store */
#define STB_FILL_HB 9          /* one launch: a spine that walks blocks of rows behind a halo, alone; tile workers convert and store */
size_t stb_fill_workspace_bytes(unsigned N, unsigned M, int D);
int stb_default_variant(void); /* STB_FILL_SCALED unless the environment says STB_FILL_VARIANT=1 */
/* table_stride: elements from one table's slab to the next, which is also the room each slab has: at least
 * stb_elems(N, M) (stb_velems(N, M) for V tables) whatever D, and an even number when D > 1; s1_stride at least N.
 * Less is refused before anything is queued ("strides too small"), in every fill below. */
int stb_fill_S(const double *a_host, int D, unsigned N, unsigned M, double *d_tables,
               uint64_t table_stride, double *d_S1, uint64_t s1_stride, void *d_ws, size_t ws_bytes,
               int variant, void *stream);
/* what stb_fill_S will use for these sizes: columns per lane, rows per launch, kernel launches;
 * returns the form: 2 producer/consumer, 3 chain, 4 checkpointed (spine + tile workers), 5 another,
 * 6 halo blocks (spine that walks blocks of rows alone + tile workers) */
int stb_fill_tuning(unsigned N, unsigned M, int D, int *C_out, int *R_out, int *launches);
/* Completion status of the last one-launch fill (halo-block, chain, checkpointed) issued by THIS thread (waits
 * for it): 0, or non-zero with stb_last_error() set when a workgroup gave up waiting for its neighbour (the
 * fill's polls are bounded; STB_CHAIN_TIMEOUT_MS, default 2000).  The other forms cannot fail on the device. */
int stb_fill_status(void);
/* A one-launch stb_fill_S whose wait expired is repeated by stb_fill_status with the
 * producer/consumer form (no waits between workgroups) before it returns 0; this counts how often
 * that happened on this thread.  STB_CHAIN_NO_FALLBACK=1 turns the repeat off (status then fails). */
unsigned stb_fill_fallbacks(void);
/* A GPU shared with other processes.  The one-launch forms have workgroups that wait for each other; when other
 * processes hold the compute units those waits burn scheduler quanta (a 1.4 ms evaluation was measured at 725 ms with
 * four processes on one GPU).  Every such launch is timed on the device; stb_slow_launches() counts those that took more
 * than 20 x what their geometry should (the first one is reported through yaps_message).  After two of them -- or from
 * the start with STB_SHARED_GPU=1 in the environment / stb_set_shared_gpu(1) -- fills take the producer/consumer form and
 * evaluations go through stored tables: no waits between workgroups, results within 1e-10 as ever.  STB_SHARED_GPU=0 /
 * stb_set_shared_gpu(0) never switches; stb_set_shared_gpu(-1) is the automatic rule again. */
unsigned stb_slow_launches(void);
int stb_shared_gpu_mode(void);           /* 1: the forms without waits are being taken */
void stb_set_shared_gpu(int mode);
void stb_note_launch_span(double span_ms, double expect_ms);   /* (what the launches report; for tests of the rule) */
/* 1 when the library carries the superseded fill forms (STB_FILL_SCALED_STEP / _SPLIT / _FUSED /
 * _CHAINX; tools/ablation); the default build refuses those variants with a message */
int stb_has_ablation(void);
/* release the device buffers the library keeps for reuse between stb_groups_create / samplea calls
 * (capped at STB_POOL_MB, default 4096) */
void stb_pool_trim(void);
/* kernel-only timing of the fills issued by THIS thread between begin and end (the stream must be
 * synchronised before _end): sum of the per-launch device durations in ms and their count */
void stb_fill_profile_begin(void);
int stb_fill_profile_end(double *kernel_ms_total, int *launches);
/* device time in ms from the first of those launches' start to the last one's end (large batches of
 * the producer/consumer form run two sub-batches side by side, so the sum counts that time twice) */
double stb_fill_profile_span(void);
/* V tables (next row 8f-1): V^n_m = S^n_m / S^n_{m-1} for 2<=n<=N, 2<=m<=min(n,M); lib/stable.c:451-482.  Tables of 512 rows
 * or more are taken from the S recurrence's block-floating cells (one division per cell off the serial path; within
 * 1e-10 of the reference); smaller ones, and every table under STB_FILLV_EXACT=1, walk the reference's own V
 * recurrence, bit for bit. */
int stb_fill_V(const double *a_host, int D, unsigned N, unsigned M, double *d_vtables,
               uint64_t vtable_stride, void *d_ws, size_t ws_bytes, void *stream);
int stb_fill_V_exact(const double *a_host, int D, unsigned N, unsigned M, double *d_vtables,
                     uint64_t vtable_stride, void *d_ws, size_t ws_bytes, void *stream);

/* the same tables written once as floats (S_FLOAT, reference lib/stable.c:389-449 and :483-537: all arithmetic in
 * double, only the stored value is a float): D float slabs with the double slabs' element offsets, no double slab
 * anywhere.  Only the halo-block form narrows before the store: stb_fill_takes_kind(N, M, D, kind) says whether a fill
 * of kind 1 (log S as float), 2 (V as double, taken from the S recurrence's cells) or 3 (V as float) applies to these
 * sizes; where it does not, stb_fill_Sf / stb_fill_Vf fail and the caller narrows a double table (stb_table_to_float). */
int stb_fill_takes_kind(unsigned N, unsigned M, int D, int kind);
int stb_fill_Sf(const double *a_host, int D, unsigned N, unsigned M, float *d_tables, uint64_t table_stride,
                double *d_S1, uint64_t s1_stride, void *d_ws, size_t ws_bytes, void *stream);
int stb_fill_Vf(const double *a_host, int D, unsigned N, unsigned M, float *d_vtables, uint64_t vtable_stride,
                void *d_ws, size_t ws_bytes, void *stream);

/* narrow a table slab to float, element for element (S_FLOAT storage, reference lib/stable.h:31-33:
 * "keep final table values in float, but all intermediate calcs done in double") */
int stb_table_to_float(const double *d_src, float *d_dst, uint64_t elems, void *stream);

/* ---- lookups with S_S semantics (lib/stable.c:941-974, no growth): out[g] = S_S(n[g], t[g]) ---- */
int stb_lookup_S(const double *d_table, const double *d_S1, unsigned N, unsigned M,
                 const uint32_t *d_n, const uint32_t *d_m, uint64_t G, double *d_out, void *stream);

/* ... and of the ratio table (a slab filled by stb_fill_V): out[g] = S_V / S_U / S_UV (n[g], m[g]) with the reference's
 * identities and bounds (lib/stable.c:875-939; no growth, no asymptotic branch: outside the slab's bounds S_V is 0 as in
 * :922).  What the table-indicator sampling step either side of the path reads (test/demo.c:405-445). */
int stb_lookup_V(const double *d_vtable, unsigned N, unsigned M, const uint32_t *d_n, const uint32_t *d_m, uint64_t G,
                 double *d_out, void *stream);
int stb_lookup_U(const double *d_vtable, unsigned N, unsigned M, double a, const uint32_t *d_n, const uint32_t *d_m,
                 uint64_t G, double *d_out, void *stream);
int stb_lookup_UV(const double *d_vtable, unsigned N, unsigned M, double a, const uint32_t *d_n, const uint32_t *d_m,
                  uint64_t G, double *d_out, void *stream);

/* ---- K3: sweep.  out[d] = sum over pairs g with n[g]>1 of S_S_d(n[g], t[g])  (samplea.c:68-80) ---- */
size_t stb_sweep_workspace_bytes(uint64_t G, int D);
int stb_sweep_S(const double *d_tables, uint64_t table_stride, const double *d_S1,
                uint64_t s1_stride, int D, unsigned N, unsigned M, const uint32_t *d_n,
                const uint16_t *d_t, uint64_t G, double *d_out, void *d_ws, size_t ws_bytes,
                void *stream);

/* ---- the slope of log S in the discount (fill_da.hip; additive: the reference's only derivative, S_approx_da of
 * lib/sapprox.c:76-114, covers m <= 4 and is wrong at m = 4 -- DESIGN.md section 6) ----
 * g(n, m) = d log S^n_{m,a} / da = -E / S with E^n_m = (n-1-m a) E^{n-1}_m + m S^{n-1}_m + E^{n-1}_{m-1}, E^1_1 = 0, walked
 * next to S by the producer/consumer form (no waits between workgroups); one FP64 division a cell.
 * stb_fill_dS: D slabs of g in exactly the S table's layout (stb_elems / stb_rowoff) and D vectors
 * dS1[n-1] = d log S^n_1 / da = -sum_{k=1}^{n-1} 1 / (k - a) (a fixed summation order).  d_tables / d_S1: both NULL, or D
 * slabs and vectors that receive log S as well, the bits of stb_fill_S(..., STB_FILL_PC).  Strides, bounds and discounts
 * as for stb_fill_S (a = 0 allowed), refused the same way before anything is queued; D <= 64, N < 2^27.  The bits do not
 * depend on D (they do on STB_FILL_P / STB_FILL_R, which move where a coefficient is formed anew, as in stb_fill_S).
 * stb_lookup_dS: S_S's cases -- n == m: 0; m == 1: dS1; inside the bounds: the slab; where S_S is log 0 (m == 0, n < m,
 * beyond the bounds): NaN, the slope of -inf.
 * stb_sweep_dS: out[d] = sum over pairs with n > 1 of g_d(n, t), stb_sweep_S's gather and order on the g slabs (its
 * workspace: stb_sweep_workspace_bytes); a set with a log-0 pair gives NaN for that discount.
 * stb_restaurant_terms_da: out[d] = sum_i [T_i / x_d - (b_i / x_d^2) (psi(T_i + b_i/x_d) - psi(b_i/x_d))], the derivative
 * of stb_restaurant_terms in x (workspace: stb_terms_workspace_bytes). */
size_t stb_fill_dS_workspace_bytes(unsigned N, unsigned M, int D);
int stb_fill_dS(const double *a_host, int D, unsigned N, unsigned M, double *d_gtables, uint64_t gtable_stride,
                double *d_dS1, uint64_t ds1_stride, double *d_tables /* or NULL */, uint64_t table_stride,
                double *d_S1 /* or NULL */, uint64_t s1_stride, void *d_ws, size_t ws_bytes, void *stream);
/* the fill's constants, for tests that sit on its boundaries (any pointer may be NULL): rows per launch, owned and halo
 * columns of a column block, rows between two barriers, rows of a renormalisation period at N rows */
void stb_fill_dS_geometry(unsigned N, int *rows_per_launch, int *owned_cols, int *halo_cols, int *trip_rows, int *period_rows);
int stb_lookup_dS(const double *d_gtable, const double *d_dS1, unsigned N, unsigned M, const uint32_t *d_n,
                  const uint32_t *d_m, uint64_t G, double *d_out, void *stream);
int stb_sweep_dS(const double *d_gtables, uint64_t gtable_stride, const double *d_dS1, uint64_t ds1_stride, int D,
                 unsigned N, unsigned M, const uint32_t *d_n, const uint16_t *d_t, uint64_t G, double *d_out, void *d_ws,
                 size_t ws_bytes, void *stream);
int stb_restaurant_terms_da(const double *x_host, int D, const uint32_t *d_T, const double *d_bpar, uint64_t I,
                            double *d_out, void *d_ws, size_t ws_bytes, void *stream);

/* ---- K4: per-restaurant terms.
 * restaurant: out[d] = sum_i T_i*log(x_d) + lgamma(T_i + b_i/x_d) - lgamma(b_i/x_d)  (samplea.c:65-67)
 * bterms:     out[j] = -Q*x_j + (shape-1)*log(x_j) + sum_i (lgamma(T_i + x_j/apar) - lgamma(x_j/apar))
 *                                                                            (sampleb.c:33-41)
 * x_host[D] are host doubles; d_T (uint32) and d_bpar (double) device arrays of I entries. */
size_t stb_terms_workspace_bytes(uint64_t I, int D);
int stb_restaurant_terms(const double *x_host, int D, const uint32_t *d_T, const double *d_bpar,
                         uint64_t I, double *d_out, void *d_ws, size_t ws_bytes, void *stream);
int stb_bterms(const double *x_host, int J, double Q, double shape, double apar,
               const uint32_t *d_T, uint64_t I, double *d_out, void *d_ws, size_t ws_bytes,
               void *stream);
/* the same for a host sampler that evaluates bterms many times over one T[] (sampleb's ARMS / slice callback,
 * lib/sampleb.c:33-41): T resident, an evaluation of J <= 64 abscissae is two kernel launches and ONE wait, the
 * values arriving in pinned host memory without a copy call */
typedef struct stb_bctx stb_bctx_t;
stb_bctx_t *stb_bterms_create(const uint32_t *T, int I);
int stb_bterms_update(stb_bctx_t *c, const uint32_t *T, int I); /* new totals, I <= the I it was created with; else non-zero */
int stb_bterms_eval(stb_bctx_t *c, const double *x_host, int J, double Q, double shape, double apar, double *out_host);
void stb_bterms_free(stb_bctx_t *c);
/* borrowed-T mode: a context over totals that already live on the device.  Evaluations read d_T in place (nothing is
 * copied) and are queued on `stream` (a hipStream_t, or NULL) behind whatever it holds.  c = NULL makes a context; a
 * context made here before is pointed at the new array and keeps its buffers when they fit.  NULL on failure (c is then
 * freed).  stb_bterms_update refuses such a context; stb_bterms_free leaves d_T alone. */
stb_bctx_t *stb_bterms_borrow(stb_bctx_t *c, const uint32_t *d_T, int I, void *stream);

/* ---- the concentration step from device-resident counts (hyperq.hip; reference lib/sampleb.c:79-159) ----
 * stb_sample_logq: for every restaurant with N_i > 0 customers an auxiliary q_i ~ Beta(b, N_i) is drawn on the device
 * and L_i = -log q_i formed in the log domain (q itself is never formed, so it cannot underflow at b = B_MIN, where the
 * reference exits with "Illegal q"); *Q_host = 1/scale + sum_i L_i, the Q of lib/sampleb.c:90-99.  d_N[I] customers
 * per restaurant; d_L (NULL, or I doubles) receives L_i (0 where N_i = 0).  One launch and one wait.  b > 0, scale > 0.
 * Uniforms: key = mix(seed + (sweep+1) gamma); restaurant i owns key_i = mix(key + (i+1) gamma); its k-th uniform is the
 * top 53 bits m of mix(key_i + k gamma) as m / 2^53, with 2^-54 in place of m = 0 (the open interval).  The Gamma
 * variates are Marsaglia-Tsang's with Box-Muller's cosine member, in the order hyperq.hip's header writes out
 * (tests/hq_oracle.py replays it); the draws depend on (seed, sweep, i) alone and Q's bits do not depend on launch
 * geometry (STB_HYPERQ_WAVES = 1, 2, 4 or 8 waves a workgroup).  The rejection loop is bounded (64 attempts a variate,
 * acceptance above 0.95 each): running out fails the call with a message.
 * stb_sampleb_device: sampleb with that Q and with bterms evaluated over d_T where it lives.  a = 0: the Gamma (or, above
 * 400, Gaussian) draw of lib/sampleb.c:101-118 with the caller's rng, sum T from a device reduction.  Otherwise ARMS
 * (libc rand()) or the slice sampler per STB_SAMPLER, with sampleb's bracket, B_MIN / B_MAX clamps and trace
 * (stb_sampler_trace_*).  Work is queued on `stream`; the call waits for Q and for each evaluation.
 * stb_tcounts_sampleb / stb_tindic_sampleb: the same on an object's counts, queued behind its sweeps on its stream;
 * nothing is read back but Q and the evaluations, and t and T are not written.
 * Failures -- a null object, a outside [0, 1), b_in <= -a or not finite (and b_in <= 0: no Beta draw exists), scale <= 0,
 * a rejection loop that ran out -- return NaN with stb_last_error() set; unlike the drop-in sampleb they never exit. */
int stb_sample_logq(double b, double scale, int I, const uint32_t *d_N, double *d_L, double *Q_host,
                    uint64_t seed, uint64_t sweep, void *stream);
double stb_sampleb_device(double b_in, int I, double shape, double scale, const uint32_t *d_N, const uint32_t *d_T,
                          double a, void *rng, int loops, int verbose, uint64_t seed, uint64_t sweep, void *stream);
double stb_sampleb_last_Q(void);          /* the Q of this thread's last device b step, for tests */

/* ---- one concentration per group of restaurants, drawn on the device (hyperb.hip; an additive algorithm, Teh's
 * auxiliary-variable scheme: DESIGN.md section 6) ----
 * The restaurants 0 .. I-1 are partitioned into G contiguous ranges d_goff[G+1] (uint64, 0 = goff[0] <= ... <= goff[G]
 * = I, empty ranges allowed; NULL: every restaurant its own group, G = I).  Group g shares one concentration b > 0 with
 * the prior Gamma(shape, scale); d_bpar[I] holds it once per restaurant (every layer's bpar).  With the discount a in
 * [0, 1), T_i tables and N_i customers (d_N[I] uint32, or d_coff[I+1] uint64 prefix sums; exactly one of the two):
 *     q_i | b ~ Beta(b, N_i) for N_i > 0, L_i = -log q_i;   y_ik | b ~ Bernoulli(b / (b + k a)), k = 1 .. T_i - 1,
 *     Y_i = [T_i >= 1] + sum_k y_ik;   b_g | q, y ~ Gamma(shape + sum_{i in g} Y_i, rate = 1/scale + sum_{i in g} L_i).
 * These are the exact conditionals of an augmented joint whose marginal is p(b | .) ~ b^(shape-1) e^(-b/scale) prod_i
 * (b|a)_{T_i} Gamma(b) / Gamma(b + N_i): the step leaves it invariant, with no ARMS, no lgamma and no host in the loop.
 * a = 0: every y is 1 and the step is the Gamma draw of lib/sampleb.c:101-118.  A restaurant without customers adds
 * nothing; a group without customers draws from the prior.
 * d_bpar is read (b_i, from the restaurant's own entry) and, on success, overwritten with b_g for i in g; d_bgrp (G, or
 * NULL) receives b_g; d_L (I doubles) receives L_i (0 where N_i = 0), d_Y (I uint32, or NULL) Y_i.
 * Streams: key = mix(seed + (sweep+1) gamma); restaurant i owns key_i = mix(key + (i+1) gamma).  L_i is stb_sample_logq's
 * draw on key_i with b_i: with every b_i equal, d_L is that call's, to the bit.  The y take the substream mix(key_i ^
 * 0x59B1D5A7C3E9F24D): y_ik = [u_k (b + k a) < b] in doubles as written (no contraction), u_k its element k (the open
 * interval), so they do not depend on how many uniforms the Beta draw took.  Group g's variate is the log-Gamma variate
 * of stb_sample_logq with shape + sum Y on the substream mix(key' + (g+1) gamma), key' = mix(key ^ 0x6A09E667F3BCC909),
 * and b_g = exp(log G - log rate).
 * Associations: sum Y is a sum of integers.  sum L is taken relative to the group's first restaurant: blocks of 256
 * restaurants, inside a block stb_sample_logq's tree (four quarters per lane, then the shuffle tree of a 64-lane wave),
 * the block sums lane-strided in double-double, merged by the same tree, 1/scale added last -- one group of equal b has
 * stb_sample_logq's Q as its rate.  No bit depends on STB_HYPERB_WAVES (1, 2, 4 or 8 waves a workgroup), on
 * STB_HYPERB_FORM (lane | wave: how a restaurant's y are spread over lanes; by default a wave takes the restaurants with
 * more than 257 tables) or on whether ranges of one restaurant each or NULL are passed.
 * Three kernels queued on `stream`, one wait; the counts and, for G = 1, b come back in pinned words (info).
 * Refusals return non-zero with stb_last_error() set and nothing written to d_bpar or d_bgrp: a outside [0, 1), shape
 * <= 0, scale <= 0, both or neither of d_N and d_coff, and a raised error word (info->error_word: 1 a rejection loop
 * ran out, 2 a b_i is not a positive finite double, 4 a b_i differs from its group's first restaurant's, 8 bad ranges;
 * info->bad_restaurants counts the restaurants of 1, 2 and 4).  A group whose draw is not a positive finite double
 * keeps its b and is counted in info->kept_groups; the call succeeds. */
struct stb_tcounts;
struct stb_tindic;
typedef struct stb_bgroups_info {
  uint64_t bad_restaurants, kept_groups;
  unsigned error_word, reserved;
  double b;                 /* G = 1: the new b; otherwise NaN */
} stb_bgroups_info_t;
int stb_sample_bgroups(double a, double shape, double scale, int I, const uint32_t *d_N, const uint64_t *d_coff,
                       const uint32_t *d_T, int G, const uint64_t *d_goff /* NULL: every restaurant its own group, G = I */,
                       double *d_bpar /* in: current, out: new */, double *d_bgrp /* G, or NULL */, double *d_L,
                       uint32_t *d_Y /* or NULL */, uint64_t seed, uint64_t sweep, void *stream, stb_bgroups_info_t *info);
/* On the objects (their declarations follow below): stb_*_set_bpar uploads I concentrations, stb_*_get_bpar reads back what
 * the object holds (after the queued work), stb_*_set_bgroups sets the ranges (goff_host[G+1], kept on the device with
 * the object; NULL: every restaurant its own group -- the state of a new object).  stb_*_sampleb_groups runs the step
 * behind the object's queued sweeps on its own T, customers and concentrations; bgrp_host (G, or NULL) receives b_g.
 * STB_BPAR_RESIDENT in place of a host bpar[I] means "what the object holds": no upload, and in place of the host-side
 * range check the object's lower bound of what it holds (the smallest value of the last upload; positive after a step,
 * which only ever writes positive finite values) must exceed -a; it fails while the object holds none.  Every object
 * entry point that takes bpar accepts it; stb_*_to_groups with it copies device to device into the set. */
#define STB_BPAR_RESIDENT ((const double *)(uintptr_t)8)
int stb_tcounts_set_bpar(struct stb_tcounts *s, const double *bpar /* host [I] */);
int stb_tcounts_get_bpar(struct stb_tcounts *s, double *bpar_out /* host [I] */);
int stb_tcounts_set_bgroups(struct stb_tcounts *s, int G, const uint64_t *goff_host /* G+1, or NULL: per restaurant */);
int stb_tcounts_sampleb_groups(struct stb_tcounts *s, double a, double shape, double scale, uint64_t seed, uint64_t sweep,
                               double *bgrp_host /* G, or NULL */, stb_bgroups_info_t *info);
int stb_tindic_set_bpar(struct stb_tindic *s, const double *bpar /* host [I] */);
int stb_tindic_get_bpar(struct stb_tindic *s, double *bpar_out /* host [I] */);
int stb_tindic_set_bgroups(struct stb_tindic *s, int G, const uint64_t *goff_host /* G+1, or NULL: per restaurant */);
int stb_tindic_sampleb_groups(struct stb_tindic *s, double a, double shape, double scale, uint64_t seed, uint64_t sweep,
                              double *bgrp_host /* G, or NULL */, stb_bgroups_info_t *info);

/* ---- the joint step for discount and concentration from device-resident counts (hyperj.hip; an additive algorithm,
 * not the reference's: DESIGN.md section 6, deviation 14) ----
 * All restaurants share one discount a and one concentration b (test/demo.c's model).  With beta = log b the target is
 *     L(a, beta) = W(a) + R(a, b) + (shape - 1) beta - b / scale + beta           on [a_lo, a_hi] x [b_lo, b_hi]
 *     W(a)    = sum over pairs with n > 1 of S_S_a(n, t)                          (stb_groups_ssum)
 *     R(a, b) = sum_i [ T_i log a + lgamma(T_i + b/a) - lgamma(b/a) - lgamma(b + N_i) + lgamma(b) ]   (0 where N_i = 0)
 * -- a flat prior on a, sampleb's Gamma(shape, scale) on b, the Jacobian of b -> beta.
 * stb_joint_terms: d_out[d J + j] = R(a_d, b_j) for a grid of D x J (1 <= D, J <= 64) from d_T[I], d_N[I] (uint32, device),
 * queued on `stream`; one launch, FP64.  The bits do not depend on launch geometry (STB_HYPERJ_WAVES = 1, 2, 4 or 8 waves
 * a workgroup); the association is written out in hyperj.hip's header.  One stream at a time per calling thread.
 * stb_groups_samplejoint: one independence Metropolis-Hastings step that leaves exp(L) on the rectangle invariant.  Up to
 * five nested stages; stage s lays D x J cells (uniform in a and in beta) over its rectangle, evaluates L at the cell
 * midpoints (one batched stb_groups_ssum of D + 1 discounts -- the current a rides along -- and one stb_joint_terms launch),
 * weights w = exp(max(L - max, -60)), and takes as its box the bounding box of the cells with L >= max - 40, padded by one
 * cell and clipped; while the box spans at most half of the cells on either axis (and s < 5) the next stage repeats on the
 * box.  The proposal is q = sum_s eps_s q_s (eps_s = 1/64 for every stage but the last, which takes the rest), q_s
 * piecewise constant over stage s's cells: the stage from u5, the cell by inverse CDF of the weights in d-major order from
 * u1, the point uniform in the cell from u2, u3; accepted iff log u4 < [L(x') - L(x)] + [log q(x) - log q(x')], with L
 * evaluated at the two points themselves.  u_k = element k of the stream of key = mix(seed + (sweep+1) gamma)
 * (libstb_amd/synth.py's unit(., key)).  The rectangle must not depend on the state.  S + 1 waits for S stages.
 * The set needs Dmax >= D + 1 and holds the pairs and T (stb_tcounts_to_groups ...).  Its bpar are NOT read -- b is the
 * argument, and after an accepted move the set's copy is stale until the caller sets it again; they are only a consistency
 * token for the model of one shared b: a set whose bpar were last set to unequal values is refused, one whose bpar were
 * never set is accepted.  Failures -- a null set, a bad rectangle (A_MIN <= a_lo < a_hi <= A_MAX,
 * B_MIN <= b_lo < b_hi <= B_MAX of include/psample.h), a state outside it, Dmax too small, unequal bpar, a non-finite L at
 * the current state or a NaN / +inf on a grid -- return non-zero with stb_last_error() set and leave *a_out, *b_out alone.
 * stb_tcounts_samplejoint / stb_tindic_samplejoint: the same on an object's counts: stb_*_to_groups(s, g, NULL) first, then
 * the step with the object's N, queued behind its sweeps; nothing per restaurant crosses to the host, t and T are not
 * written. */
#define STB_JOINT_KEEP_L 1u   /* info->L receives every stage's D J values of L (for tests) */
typedef struct stb_joint_opts {
  double a_lo, a_hi, b_lo, b_hi;   /* the rectangle, in a and b */
  int D, J;                        /* cells per stage; 0: 24.  D <= 63, J <= 64 */
  double shape, scale;             /* the Gamma prior of b, as sampleb's */
  uint64_t seed, sweep;
  unsigned flags;
} stb_joint_opts_t;
typedef struct stb_joint_info {
  int stages, accepted, evals;     /* stages taken, 1 if x' was accepted, batched pair-sum evaluations (stages + 1) */
  int stage_pick;                  /* the stage x' was drawn from, 1-based */
  double log_alpha;
  double rect[4];                  /* the last stage's rectangle: a_lo, a_hi, beta_lo, beta_hi */
  double a_prop, b_prop, L_cur, L_prop;
  int cell[5];                     /* per stage the cell u1 picks, d J + j */
  int box[5][4];                   /* per stage its box: d lo, d hi, j lo, j hi (cells, inclusive) */
  const double *L;                 /* STB_JOINT_KEEP_L: [stages][D J], valid until this thread's next step */
} stb_joint_info_t;
struct stb_groups;
struct stb_tcounts;
struct stb_tindic;
int stb_joint_terms(const double *a_host, int D, const double *b_host, int J, const uint32_t *d_T, const uint32_t *d_N,
                    uint64_t I, double *d_out, void *stream);
int stb_groups_samplejoint(struct stb_groups *g, const uint32_t *d_N, const stb_joint_opts_t *opts, double a_in, double b_in,
                           double *a_out, double *b_out, stb_joint_info_t *info);
int stb_tcounts_samplejoint(struct stb_tcounts *s, struct stb_groups *g, const stb_joint_opts_t *opts, double a_in, double b_in,
                            double *a_out, double *b_out, stb_joint_info_t *info);
int stb_tindic_samplejoint(struct stb_tindic *s, struct stb_groups *g, const stb_joint_opts_t *opts, double a_in, double b_in,
                           double *a_out, double *b_out, stb_joint_info_t *info);

/* ---- device-resident group set + grid evaluation (host-friendly wrappers over the above) ----
 * stb_groups_t owns device copies of the flat (n,t) pairs and the per-restaurant T, bpar, plus
 * the scratch needed to evaluate aterms on up to Dmax discounts with table bounds (N,M). */
typedef struct stb_groups stb_groups_t;
stb_groups_t *stb_groups_create(int I, const int *K, const uint32_t *T, const uint32_t *nflat,
                                const uint16_t *tflat, const double *bpar, unsigned N, unsigned M,
                                int Dmax);
void stb_groups_free(stb_groups_t *g);
/* out_host[D] = aterms(x_d) for every d: table build + sweep + restaurant terms.  D <= Dmax. */
int stb_groups_aterms(stb_groups_t *g, const double *x_host, int D, double *out_host);
/* The same evaluation in two calls, so that ONE host thread can keep several GPUs (or several group sets)
 * busy: _async queues it on the set's own stream -- behind whatever `stream` (a hipStream_t, or NULL)
 * holds at this moment -- and returns without waiting; stb_groups_wait blocks until it is through and
 * only then writes out_host[0..D-1].  x_host may be reused at once, out_host must stay valid until the
 * wait; one evaluation per set at a time.  (All entry points of this library may be called from several
 * host threads at once -- one per GPU, or several on one GPU; see INTEGRATION.md.) */
int stb_groups_aterms_async(stb_groups_t *g, const double *x_host, int D, double *out_host, void *stream);
int stb_groups_wait(stb_groups_t *g);
/* The node from ONE host thread, for a C caller (the reference's callers are C: lib/samplea.c:155, test/demo.c:478-480).
 * `sets` are k group sets made from the same pairs -- one per GPU: stb_groups_create_node makes min(ndev,
 * stb_device_count()) of them on devices 0, 1, ... and returns how many (0 on failure); or the caller's own, e.g. several
 * on one GPU -- and the D abscissae are sharded over them in contiguous blocks whose sizes differ by at most one (each
 * must fit its set's Dmax): all are queued before any is waited for, and out_host[0..D) comes back in the grid's order,
 * 8 bytes a discount through pinned host memory.  This is the discount-axis sharding of SURVEY 8e without a collective;
 * the one-process-per-GPU layout (libstb_amd/shard.py, bench.py --gpus N) keeps the values on the devices and gathers
 * them over RCCL instead. */
int stb_groups_aterms_multi(stb_groups_t *const *sets, int k, const double *x_host, int D, double *out_host);
int stb_groups_create_node(int ndev, int I, const int *K, const uint32_t *T, const uint32_t *nflat, const uint16_t *tflat,
                           const double *bpar, unsigned N, unsigned M, int Dmax, stb_groups_t **sets_out);
/* ... with the D log-posteriors left on the DEVICE, in d_out[0..D) (a device address), for a caller that hands them to a
 * collective: the discount axis sharded over the GPUs of a node, every rank all-gathers its share.  Queued
 * like _async; `stream` then waits on the device for the values, so work queued on it afterwards sees them.
 * stb_groups_wait(g) must still follow, before the values are trusted: it reports a table walk that gave up waiting
 * for a neighbour, in which case it re-evaluates through stored tables and rewrites d_out. */
int stb_groups_aterms_device(stb_groups_t *g, const double *x_host, int D, double *d_out, void *stream);
/* the pair sum alone: out[d] = W(x_d) = sum over pairs with n > 1 of S_S_{x_d}(n, t), without the restaurant terms.  It
 * goes through exactly the forms stb_groups_aterms_device takes (same lists, same fallbacks); _device queues like
 * stb_groups_aterms_device and stb_groups_wait(g) must follow; stb_groups_ssum blocks and writes out_host[0..D). */
int stb_groups_ssum_device(stb_groups_t *g, const double *x_host, int D, double *d_out, void *stream);
int stb_groups_ssum(stb_groups_t *g, const double *x_host, int D, double *out_host);
/* the same values through stored tables and the sorted gather whatever D is (stb_groups_aterms sums
 * inside the fill when D >= 2, which needs a set-up pass over the pairs on first use) */
int stb_groups_aterms_tables(stb_groups_t *g, const double *x_host, int D, double *out_host);
/* samplea's draw on a set that already holds the pairs, T and bpar (stb_groups_create, stb_groups_pairs_*,
 * stb_tcounts_to_groups, stb_tindic_to_groups): the bracket of lib/samplea.c:161-177 around a, the three abscissae ARMS
 * asks for first in one batched evaluation, ARMS (libc rand()) or the slice sampler (the caller's rng) per STB_SAMPLER,
 * and the trace; the drop-in samplea() runs this same code on its kept set.  The set needs Dmax >= 3.  Returns the new
 * discount, or NaN with stb_last_error() set (a null set, a outside (0, 1), a failed evaluation): it never exits. */
double stb_groups_samplea(stb_groups_t *g, double a, void *rng, int loops, int verbose);
/* ---- gradient and mode of aterms in the discount (groups_da.hip) ----
 * stb_groups_aterms_grad: val_out[d] = what stb_groups_aterms returns for the same call, bit for bit; grad_out[d] =
 * d aterms / dx at x_d = stb_restaurant_terms_da + stb_sweep_dS over the set's pairs, from g tables private to the set
 * (asked for on first need, sized by the set's bounds).  0 < x_d < 1, D <= Dmax; a set without pairs is refused; a log-0
 * pair makes the gradient NaN (the value is -inf).  Non-zero return: stb_last_error() is set and nothing is written.
 * stb_groups_modea: the maximum of aterms on [a_lo, a_hi] -- under samplea's flat prior the posterior mode of the
 * discount.  k = min(Dmax, 8) gradients a round in ONE stb_groups_aterms_grad call: round 1 at k equally spaced points
 * that include both bounds (gradient at a_lo <= 0: a_hat = a_lo, at_bound -1; at a_hi >= 0: a_hat = a_hi, at_bound +1),
 * later rounds at k equally spaced interior points of the bracket; the bracket becomes the leftmost pair of neighbours
 * with gradients (> 0, <= 0); rounds end at width <= tol, at rounds_max, or when the bracket no longer narrows.  a_hat is
 * one secant step inside the last bracket.  A last call evaluates a_hat - delta, a_hat, a_hat + delta (delta: the last
 * bracket's width -- tol at a bound -- cut to half the distance from a_hat to 0 and to 1): *curv = (g(a_hat + delta) -
 * g(a_hat - delta)) / (2 delta) (may be NULL).  Host C, deterministic, no random numbers.  Needs Dmax >= 3,
 * 0 < a_lo < a_hi < 1, tol > 0, rounds_max >= 1; refusals and failures (a NaN gradient) leave the outputs untouched. */
typedef struct stb_modea_info {
  int rounds, evals, at_bound;     /* bracketing rounds, gradient evaluations in all (the last three included), -1 / 0 / +1 */
  double lo, hi, g_lo, g_hi;       /* the last bracket and the gradients at its ends (lo == hi at a bound) */
  double grad, delta;              /* the gradient at a_hat, the step of the curvature's difference */
} stb_modea_info_t;
int stb_groups_aterms_grad(stb_groups_t *g, const double *x_host, int D, double *val_out, double *grad_out);
int stb_groups_modea(stb_groups_t *g, double a_lo, double a_hi, double tol, int rounds_max, double *a_hat, double *curv,
                     stb_modea_info_t *info);
/* new per-restaurant totals T[I] and concentrations bpar[I] for the same pairs */
int stb_groups_update_restaurants(stb_groups_t *g, const uint32_t *T, const double *bpar);
/* NEW PAIRS for a set of the same shape (I restaurants, G = sum K pairs): what a caller whose counts change between
 * calls does instead of stb_groups_free + stb_groups_create -- the reference's own Gibbs loop rewrites t[j][i] and T[j]
 * in every iteration (test/demo.c:405-445) and then resamples a (:478-480).  No allocation, no sort: the pairs are
 * copied once into pinned memory, piece by piece, each piece on its way to the device while the caller hands over the
 * next; the cell lists of the fused evaluation are rebuilt on the device when the next evaluation is queued.
 *   stb_groups_pairs_begin(g)                       waits for whatever still uses the old pairs
 *   stb_groups_pairs_put(g, n, t, count, &mn, &mt)  the next `count` pairs, in order (e.g. restaurant after restaurant:
 *                                                   n[i], t[i], K[i]); mn / mt (may be NULL) receive the largest n and t
 *                                                   so far -- what samplea derives its table bounds from
 *   stb_groups_pairs_commit(g, T, bpar, N, M)       all G pairs are in; T, bpar (both or neither NULL) new restaurant
 *                                                   totals; N, M the table bounds (0, 0: unchanged).  New bounds
 *                                                   re-size what depends on them (buffers come from the library's cache)
 * stb_groups_update_pairs = begin + put + commit(NULL, NULL, 0, 0) from flat arrays.  A set may be created EMPTY
 * (stb_groups_create with nflat = tflat = NULL, and N = M = 0 when the bounds are not known yet) and filled this way.
 * Results are the same bits as those of a set created from the same pairs, in whatever order they are handed over. */
int stb_groups_pairs_begin(stb_groups_t *g);
int stb_groups_pairs_put(stb_groups_t *g, const uint32_t *n, const uint16_t *t, uint64_t count, unsigned *maxn, unsigned *maxt);
/* all G pairs at once from samplea's ragged arrays (restaurant i: n[i][0..K[i]), t[i][0..K[i])), between begin and
 * commit instead of the puts: a few host threads of the library's own copy (STB_PUT_THREADS, default 4; 0: the caller's
 * thread alone) while the calling thread hands what is copied to the device */
int stb_groups_pairs_put_ragged(stb_groups_t *g, int I, const int *K, uint32_t *const *n, uint16_t *const *t, unsigned *maxn, unsigned *maxt);
int stb_groups_pairs_commit(stb_groups_t *g, const uint32_t *T, const double *bpar, unsigned N, unsigned M);
int stb_groups_update_pairs(stb_groups_t *g, const uint32_t *nflat, const uint16_t *tflat);
/* how often, in this process, a fused evaluation (halo-block, grid or chain form) gave up waiting for a neighbour and
 * was repeated through stored tables (stb_fill_fallbacks counts the repeated FILLS of the calling thread) */
unsigned stb_groups_fallbacks(void);
/* the strip shape the grid form (k_grid_hb) takes for D discounts of an N x M table: columns per lane, rows per group,
 * every K-th row staged (any pointer may be NULL); non-zero where that form does not apply.  Diagnostics. */
int stb_grid_shape(unsigned N, unsigned M, int D, int *C_out, int *G_out, int *K_out);
/* what the set was created with (any pointer may be NULL) */
int stb_groups_shape(const stb_groups_t *g, int *I, uint64_t *G, unsigned *N, unsigned *M, int *Dmax);
/* which form the set's most recent evaluation was prepared in (any pointer may be NULL): fused 1 when the sums are taken
 * inside the fill, 0 for stored tables and the gather; which the list layout -- 0 chain, 1 checkpointed, 2 halo-block, 3 / 4 / 5
 * the grid form with 2 / 4 / 8 columns a lane; sparse 1 for cell lists, 0 for the count slab (chain form only); C, R the
 * columns per lane and rows per block the lists taken were built for (0, 0 for the forms without strips).  It reads the set
 * and changes nothing; an evaluation that gave up on a wait and was redone through stored tables still reports the form
 * it was prepared in, and stb_groups_fallbacks counts it.  Diagnostics. */
int stb_groups_last_form(const stb_groups_t *g, int *fused, int *which, int *sparse, int *C, int *R);
/* pieces of the same evaluation, for timing: ms of device time per stage (may be NULL) */
int stb_groups_aterms_timed(stb_groups_t *g, const double *x_host, int D, double *out_host,
                            float *ms_fill, float *ms_sweep, float *ms_terms);

/* ---- table counts: a collapsed Gibbs sweep over t (the step a Pitman-Yor sampler alternates with sampleb / samplea;
 * reference test/check.c:868-935, SampleCT without its early stop).  Restaurant i owns pairs k = 0 .. K_i-1 in CSR order
 * (n uint32, t uint16, base-measure weight h > 0, NULL: all 1), a total T_i = sum_k t_ik and a concentration b_i > -a;
 * one discount 0 <= a < 1.  A sweep visits each restaurant's pairs in order and draws t_ik from its conditional given the
 * rest, with T_ = T_i - t_ik:
 *     log w(tau) = S_S(n, tau) + (tau-1) log h + sum_{s=T_+1}^{T_+tau-1} log(b_i + s a),   tau = 1 .. min(n, M)
 * (S_S with stb_lookup_S's semantics), the smallest tau whose cumulative weight exceeds u W (weights scaled by
 * exp(-max log w), W their sum); T_i is updated before the next pair.  n = 0 keeps t = 0, n = 1 gets t = 1.  With M < n
 * the draw is from the conditional TRUNCATED at M: exact only when M >= the largest n.  The uniform of pair g (flat
 * index) in sweep s is splitmix64's (libstb_amd/synth.py): key = mix(seed + (s+1) gamma), u = top 53 bits of
 * mix(key + (g+1) gamma) / 2^53 -- the draws depend on (seed, sweep, g) alone.
 * Raw layer: d_table / d_S1 one slab of stb_fill_S for `a` with bounds (N, M) (never read, and may be NULL, when no pair
 * has min(n, M) >= 2); a pair with n > N lies outside the table and keeps its t, whatever M; d_koff[I+1] the CSR
 * offsets; d_t and d_T are updated in place.  One sweep. */
int stb_sample_tcounts(const double *d_table, const double *d_S1, unsigned N, unsigned M, double a,
                       const double *d_bpar, int I, const uint64_t *d_koff /* I+1 */, const uint32_t *d_n,
                       uint16_t *d_t, uint32_t *d_T, const double *d_h /* NULL: 1 */,
                       uint64_t seed, uint64_t sweep, void *stream);
/* Object layer: owns the pairs, T, h, its own stream and its own S table (bounds: the largest n, M), filled by
 * stb_fill_S for the current a and refilled only when a changes.  Inputs are checked (sum K = G; t = 0 exactly when
 * n = 0, else 1 <= t <= min(n, M); h > 0 and finite; 0 <= a < 1; b_i > -a; M = 0 with a largest n above 65535 is
 * refused, t being a uint16): a failure returns non-zero (NULL from create) with stb_last_error() set and leaves the
 * state as it was.  Objects whose pairs all have n <= 1, or with M = 1, hold no table: every draw is t = 1.  Device
 * rules as for group sets (stb_set_device).
 *   stb_tcounts_sweep      sweeps sweep .. sweep+nsweeps-1, queued on the object's stream (bpar: host [I], copied
 *                          before the call returns).  The call waits only when `a` differs from the last call's: the
 *                          table is refilled and its fill checked (stb_fill_status) behind the sweeps already queued
 *   stb_tcounts_get        waits, then t (G) and / or T (I) to the host (either may be NULL)
 *   stb_tcounts_to_groups  pairs and T to a group set of the same shape on the same device, device to device: what
 *                          stb_groups_update_pairs + stb_groups_update_restaurants do from the host.  Only I and
 *                          G = sum K are checked (a set does not keep K; its evaluation reads flat pairs and per-
 *                          restaurant T, as with stb_groups_update_pairs).  The set re-sorts its copy and rebuilds its
 *                          cell lists on first need; its table bounds grow to at least (max n, min(max n, M)) -- what
 *                          any t can need, so no count is read back; bpar (host [I]) replaces its concentrations, NULL
 *                          keeps them.  Work queued on the set afterwards sees the new pairs; later sweeps wait for the
 *                          copy.  Nothing waits on the host but for the set's own earlier work. */
typedef struct stb_tcounts stb_tcounts_t;
stb_tcounts_t *stb_tcounts_create(int I, const int *K, const uint32_t *nflat, const uint16_t *tflat,
                                  const double *hflat, unsigned M /* 0: max n */);
int stb_tcounts_set_h(stb_tcounts_t *s, const double *hflat);   /* NULL: all 1 */
int stb_tcounts_sweep(stb_tcounts_t *s, double a, const double *bpar /* host [I] */,
                      uint64_t seed, uint64_t sweep, int nsweeps);
int stb_tcounts_get(stb_tcounts_t *s, uint16_t *t_out, uint32_t *T_out);
int stb_tcounts_to_groups(stb_tcounts_t *s, stb_groups_t *g, const double *bpar /* NULL: keep */);
/* the concentration step on the object's counts (see stb_sampleb_device): N_i is built once at create */
double stb_tcounts_sampleb(stb_tcounts_t *s, double b_in, double shape, double scale, double a, void *rng,
                           int loops, int verbose, uint64_t seed, uint64_t sweep);
void stb_tcounts_free(stb_tcounts_t *s);

/* ---- windowed table counts: t drawn from a window around itself, O(W) a pair instead of O(min(n, M)) (reference
 * test/check.c:905-935, SampleCTW, made exact).  Pairs, h, T_i, b_i, a and the weights w(tau) exactly as for
 * stb_tcounts above (T_ = T_i - t).  With Mt = min(n, M), lo(x) = max(1, x - W), hi(x) = min(Mt, x + W),
 * win(x) = [lo(x), hi(x)] and Z(x) = sum over win(x) of w, a sweep visits each restaurant's pairs in order:
 *   1. n = 0 keeps t = 0.  n = 1, or Mt = 1, gives t = 1.  n > N (outside the table) keeps t.  (A raw-layer t outside
 *      [1, Mt] is first clamped into it; T_ still uses the stored t.)
 *   2. proposal: tau' = the smallest tau in win(t) whose cumulative weight (ascending tau, weights of win(t) scaled by
 *      exp(-max log w over win(t))) exceeds u1 Z(t).
 *   3. acceptance (the default, exact mode): if tau' != t, t = tau' iff u2 Z(tau') < Z(t), both sums scaled by
 *      exp(-max log w over [lo(min(t, tau')), hi(max(t, tau'))]).  STB_TC_REF_WINDOW accepts every proposal: the
 *      reference's chain in law.  Its normaliser Z(t) depends on the state, so that chain does not leave the PYP joint
 *      invariant (deviation 11); with the test, pi(t) q(t -> tau') alpha = pi(t) pi(tau')
 *      min(1/Z(t), 1/Z(tau')) is symmetric (|t - tau'| <= W either way) and the exact conditional is invariant.
 *   4. T_i is updated before the next pair.
 * log w is evaluated up to a constant per visit (the log terms summed outward from t on spans of up to 64 tau, from the
 * span's start on longer ones): the draws agree with a replay in another summation order up to rounding.  W >= 1 is any
 * unsigned value; windows are clipped to [1, Mt].  When W >= Mt - 1 for every pair the proposal is the full conditional
 * and every proposal is accepted: the law of stb_tcounts_sweep, not its bits.  Uniforms of sweep s: key = mix(seed +
 * (s+1) gamma); u1 = top 53 bits of mix(key + (2g+1) gamma) / 2^53, u2 the same at 2g+2 (g the flat pair index) --
 * stb_tindic's convention on pairs, the same stream as stb_tcounts' and stb_tindic's for the same seed and sweep (a caller
 * that alternates samplers gives them different seeds).  The draws depend on (seed, sweep, g) alone, not on launch
 * geometry (STB_TCWIN_WAVES = 1, 2, 4 or 8 waves a workgroup, one restaurant a wave).
 * Raw layer: the arguments of stb_sample_tcounts plus W and flags; M <= 65535.  W = 0 and unknown flag bits are refused.
 * One sweep.  Object layer: stb_tcounts_sweep_window runs on an stb_tcounts_t with stb_tcounts_sweep's table (refilled
 * only when a changes), staging, stream and input checks; full and windowed sweeps mix freely on one object, and
 * _get / _to_groups see either.  A failure returns non-zero with stb_last_error() set and leaves the state as it was. */
#define STB_TC_REF_WINDOW 1u
int stb_sample_tcounts_window(const double *d_table, const double *d_S1, unsigned N, unsigned M, double a,
                              const double *d_bpar, int I, const uint64_t *d_koff /* I+1 */, const uint32_t *d_n,
                              uint16_t *d_t, uint32_t *d_T, const double *d_h /* NULL: 1 */, unsigned W, unsigned flags,
                              uint64_t seed, uint64_t sweep, void *stream);
int stb_tcounts_sweep_window(stb_tcounts_t *s, double a, const double *bpar /* host [I] */, unsigned W, unsigned flags,
                             uint64_t seed, uint64_t sweep, int nsweeps);

/* ---- table indicators: the other t-sampler, one Gibbs step per customer (reference test/demo.c:405-436, SampleTI of
 * test/check.c:843-866), with the exact prior ratio.  Pairs, h, T_i, b_i and a as for stb_tcounts above.  The customers of
 * restaurant i are a sequence of its pair indices, cust[coff[i] .. coff[i+1]) (uint32, local k): pair k appears exactly
 * n_ik times; cust == NULL is PAIR ORDER (pair 0 n_0 times, then pair 1, ...).  c = 0 .. C-1 is the flat customer index
 * over all restaurants in CSR order.  A sweep visits each restaurant's customers in sequence; a visit to a customer of
 * pair (n, t, h):
 *   1. n <= 1, or n > N (outside the table, as in stb_sample_tcounts): nothing.
 *   2. remove: if t > 1 and (double)(n-1) * u1 < (double)(t-1): t -= 1, T_i -= 1.  (Now t < n.)
 *   3. odds = h * (b + (double)T_i * a) * (double)t / (double)(n - t) * V, evaluated left to right without contraction,
 *      V = what stb_lookup_V returns for (n, t+1): 0 when t+1 > M, the draw truncated at M as in stb_tcounts.
 *      With STB_TI_REF_ODDS the divisor is (double)(n - t + 1), the reference's factor (its chain
 *      does not leave the PYP joint invariant; t / (n-t) is C(n-1, t-1) / C(n-1, t), the exact ratio).
 *   4. add: p = odds / (odds + 1.0) (1 when odds is +inf); if u2 < p: t += 1, T_i += 1.
 * Uniforms of sweep s: key = mix(seed + (s+1) gamma); u1 = top 53 bits of mix(key + (2c+1) gamma) / 2^53, u2 the same
 * at 2c+2 (elements 2c and 2c+1 of libstb_amd/synth.py's unit(2C, key)).  The draws depend on (seed, sweep, c) alone,
 * not on launch geometry or on the kernel form.  This stream coincides with stb_tcounts' for the same seed and sweep: a
 * caller that alternates the two samplers gives them different seeds.
 * Two kernels with the same arithmetic: one lane per restaurant (many short restaurants) and one wave per restaurant
 * (few long ones); the form follows the number of restaurants, STB_TINDIC_FORM=lane|wave forces one.
 * Raw layer: d_vtable a slab of stb_fill_V for `a` with bounds (N, M) (never read, and may be NULL, when M = 1 or no
 * pair has 2 <= n <= N); d_koff[I+1] the pair offsets, d_coff[I+1] (uint64) the customer offsets -- the prefix sums of
 * each restaurant's sum of n; d_cust NULL or every entry a pair of its restaurant; t and T updated in place.  One
 * sweep. */
#define STB_TI_REF_ODDS 1
int stb_sample_tindic(const double *d_vtable, unsigned N, unsigned M, double a, const double *d_bpar, int I,
                      const uint64_t *d_koff /* I+1 */, const uint32_t *d_n, uint16_t *d_t, uint32_t *d_T,
                      const double *d_h /* NULL: 1 */, const uint64_t *d_coff /* I+1 */, const uint32_t *d_cust /* NULL: pair order */,
                      unsigned flags, uint64_t seed, uint64_t sweep, void *stream);
/* Object layer, as stb_tcounts_*: owns the pairs, T, h, the customer order, its own stream and its own V table (bounds:
 * the largest n, M), filled by stb_fill_V for the current a and refilled only when a changes.  Inputs are checked (t = 0
 * exactly when n = 0, else 1 <= t <= min(n, M); h > 0 and finite; every cust entry < K_i and pair k visited exactly n_k
 * times; known flag bits; 0 <= a < 1; b_i > -a; M = 0 with a largest n above 65535 is refused): a failure returns
 * non-zero (NULL from create) with stb_last_error() set and leaves the state as it was.  Objects whose pairs all have
 * n <= 1, or with M = 1, hold no table (no indicator is ever added).  _sweep, _get and _to_groups behave as
 * stb_tcounts_sweep, _get and _to_groups. */
typedef struct stb_tindic stb_tindic_t;
stb_tindic_t *stb_tindic_create(int I, const int *K, const uint32_t *nflat, const uint16_t *tflat, const double *hflat,
                                const uint32_t *cust /* NULL: pair order */, unsigned M /* 0: max n */, unsigned flags);
int stb_tindic_set_h(stb_tindic_t *s, const double *hflat);   /* NULL: all 1 */
int stb_tindic_sweep(stb_tindic_t *s, double a, const double *bpar /* host [I] */, uint64_t seed, uint64_t sweep,
                     int nsweeps);
int stb_tindic_get(stb_tindic_t *s, uint16_t *t_out, uint32_t *T_out);
int stb_tindic_to_groups(stb_tindic_t *s, stb_groups_t *g, const double *bpar /* NULL: keep */);
double stb_tindic_sampleb(stb_tindic_t *s, double b_in, double shape, double scale, double a, void *rng,
                          int loops, int verbose, uint64_t seed, uint64_t sweep);
void stb_tindic_free(stb_tindic_t *s);

/* ---- dishes: the step that moves data.  Every customer leaves its dish and is seated again, at any dish of its
 * restaurant, under a likelihood that is a fixed table during the sweep; restaurants stay independent and the sweep is
 * exact.  The reference has no such step (test/demo.c:405-434 re-seats a customer in its own dish):
 * like stb_tcounts_partition this is additive.  Pairs, h, T_i, b_i, a, cust / coff and the V slab as for stb_sample_tindic;
 * cust is required and is written.  cls[c] (uint32, flat customer index c) is the customer's likelihood class, lik a device
 * matrix of rows x stride doubles, row-major, finite and >= 0: L_k = lik[cls[c] * stride + k] for local pair k.  lik == NULL:
 * every L is 1 and cls is not read.  A visit to customer c, now at pair k0 = cust[c]:
 *   1. remove.  (n, t) of k0: n >= 2: if t > 1 and (double)(n-1) * u1 < (double)(t-1): t -= 1, T_i -= 1 (the indicator
 *      sweep's removal); then n -= 1.  n == 1: (n, t) = (0, 0), T_i -= 1.
 *   2. weights.  g = b + (double)T_i * a.  Every pair k with (n, t, h): z_k = L_k * (A_k + g * B_k), where
 *        n = 0:   A = 0, B = h
 *        n >= 1:  U = t == 1 ? n - a : (n - t * a) + 1 / V^n_t                  (S^{n+1}_t / S^n_t)
 *                 A = U * (n - t + 1) / n
 *                 R = t + 1 > M ? 0 : (t == n ? 1 : (n - (t+1) * a) * V^n_{t+1} + 1)     (S^{n+1}_{t+1} / S^n_t)
 *                 B = h * t * R / n
 *      n, t, n - t + 1 and t + 1 converted to double first; FP64, evaluated left to right as written (g * B is one product,
 *      then the sum, then the product with L), no contraction.  t/n and (n-t+1)/n are the binomial ratios of the
 *      held-first indicator representation (C(n-1, t-1) against C(n, t) and C(n, t-1)); z_k is the total weight of seating
 *      c at k, at a new table or an old one.  A_k and B_k depend on the pair's own (n, t, h) alone.
 *   3. choose.  Cumulative sums of z in this association: dishes in blocks of 64 (dish k in block k / 64, lane k % 64,
 *      lanes past K_i holding 0); inside a block the inclusive Kogge-Stone scan x_l <- x_l + x_{l-d} (l >= d, all lanes at
 *      once) for d = 1, 2, 4, 8, 16, 32; cum_k = base_j + scan_k with base_0 = 0 and base_{j+1} = cum of block j's lane
 *      63.  Z = the last base.  If Z is not positive and finite the customer goes back to k0 with the (n, t, T_i) it had
 *      and counts as stuck.  Otherwise thr = u3 * Z and k* is the smallest k with z_k > 0 and cum_k > thr, or, if there is
 *      none, the largest k with z_k > 0.
 *   4. seat.  n_{k*} = 0: (n, t) = (1, 1), T_i += 1.  Otherwise n += 1 and the indicator sweep's step 3-4 on (n, t), with
 *      V^n_{t+1} and u2 and the exact ratio, decides t += 1, T_i += 1.  cust[c] = k*.
 * u1 and u2 are stb_sample_tindic's (elements 2c+1, 2c+2 of the sweep's stream), u3 is element 2C+1+c, C = coff[I] the
 * number of customers: the draws depend on (seed, sweep, c, C) alone, not on launch geometry or kernel form.  A visit
 * where only k0 has positive weight (K_i = 1, a one-hot likelihood row) equals stb_sample_tindic's bit for bit.
 * One wave per restaurant, lanes over dishes; K_i <= 64 everywhere: n, t, h, A, B in registers, else in LDS.
 * Raw layer: n, t, T and cust updated in place; d_info NULL or two uint64 the call ADDS to: skipped, stuck.  A restaurant
 * with N_i = coff[i+1] - coff[i] > N, K_i > STB_TD_MAXK, or (with a likelihood) K_i > stride is left untouched and counts
 * in skipped (K_i lives on the device: the call cannot refuse it); a class >= rows makes every L 0.  Refused before
 * anything is queued: a outside [0, 1), bounds as stb_sample_tindic, a null d_cust or other required array, a likelihood
 * without d_cls or with rows or stride 0.  One sweep. */
#define STB_TD_MAXK 1024
typedef struct stb_tdish_info {
  uint64_t skipped, stuck; /* restaurants left untouched; visits that found no dish of positive finite weight */
} stb_tdish_info_t;
int stb_sample_tdishes(const double *d_vtable, unsigned N, unsigned M, double a, const double *d_bpar, int I,
                       const uint64_t *d_koff /* I+1 */, uint32_t *d_n, uint16_t *d_t, uint32_t *d_T,
                       const double *d_h /* NULL: 1 */, const uint64_t *d_coff /* I+1 */, uint32_t *d_cust,
                       const uint32_t *d_cls, const double *d_lik /* NULL: 1 */, unsigned rows, unsigned stride,
                       uint64_t seed, uint64_t sweep, uint64_t *d_info /* NULL, or {skipped, stuck} */, void *stream);
/* Object layer, on an stb_tindic_t; dish sweeps, indicator sweeps, _sampleb, _samplejoint, _logjoint and _to_groups mix
 * freely on one object.
 *   stb_tindic_set_classes  cls[C] from the host, every entry < rows (NULL: none)
 *   stb_tindic_set_lik      rows x stride doubles from the host, finite and >= 0, stride >= the largest K_i; a NULL
 *                           matrix with rows = 0 removes the likelihood, with rows > 0 holds all ones (for device writers)
 *   stb_tindic_lik_device   the device matrix, its shape and the object's stream (hipStream_t as void*): work that writes
 *                           it is queued there, or ordered before the next dish sweep by the caller; NULL when none is set
 *   stb_tindic_sweep_dishes sweeps sweep .. sweep+nsweeps-1, queued in one launch; *info (may be NULL: then no wait)
 *                           receives the call's counts.  With a likelihood, classes must be set, with rows <= the matrix's.
 *   stb_tindic_get_state    n[G] and cust[C] to the host (either may be NULL), after the queued sweeps
 *   stb_tindic_class_counts customers per (class, dish): cnt[rows x stride] uint32, rows as given to _set_classes, stride
 *                           the matrix's, or the largest K_i when none is set
 * The first dish sweep materialises pair order if the object was created without cust, and grows the object's bounds to
 * what moving customers can reach: N = max(3, max_i N_i), the truncation M as given at create (0: max_i N_i).  The V table
 * is reallocated and refilled (checked with stb_fill_status as in _sweep), the log joint's S slab is given back and taken
 * again at the new bounds on its next use, and the largest n the object vouches for becomes max_i N_i, so _to_groups
 * still needs no read-back.  Refused, the state left as it was: objects created with STB_TI_REF_ODDS; some K_i >
 * STB_TD_MAXK; M = 0 at create with some N_i > 65535; a, bpar as for _sweep; the checks above. */
int stb_tindic_set_classes(stb_tindic_t *s, const uint32_t *cls_host, unsigned rows);
int stb_tindic_set_lik(stb_tindic_t *s, const double *lik_host, unsigned rows, unsigned stride);
double *stb_tindic_lik_device(stb_tindic_t *s, unsigned *rows, unsigned *stride, void **stream);
int stb_tindic_sweep_dishes(stb_tindic_t *s, double a, const double *bpar /* host [I] */, uint64_t seed, uint64_t sweep,
                            int nsweeps, stb_tdish_info_t *info /* or NULL */);
int stb_tindic_get_state(stb_tindic_t *s, uint32_t *n_out, uint32_t *cust_out);
int stb_tindic_class_counts(stb_tindic_t *s, uint32_t *cnt_out);

/* ---- the likelihood and the base weights, drawn on the device (tlik.hip; additive: the reference has no such step) ----
 * The dish sweep is exact because the likelihood is a fixed table while it runs.  The step that completes the chain is the
 * uncollapsed one: with a Dirichlet(beta) prior on every dish's distribution over classes, the distribution of dish k given
 * the customers is Dirichlet(beta_w + cnt_wk), cnt_wk the customers of class w at dish k, independently over dishes; drawing
 * it and sweeping the dishes under it is a Gibbs sampler on (likelihood, seating).  The same holds for
 * the base weights: every table draws its dish from h, so h enters the joint as prod_k h_k^{c_k}, c_k the tables serving
 * dish k -- the H term of stb_logjoint -- and with a Dirichlet(gamma) prior h | t is Dirichlet(gamma_k + c_k).
 * stb_sample_lik: d_cnt and d_lik are rows x stride, row-major (class w, dish k at w * stride + k; uint32 and double).  For
 * every cell lg_wk = log G, G ~ Gamma(beta_w + cnt_wk) (beta_w = beta_host[w], or beta0 when beta_host is NULL), by
 * stb_sample_logq's recipe unchanged: Marsaglia-Tsang with Box-Muller's cosine member, the log-domain boost for a shape
 * below 1, at most 64 attempts a variate (libstb_amd/csrc/gamma_dev.h writes it out; tests/tl_oracle.py replays it).
 * Uniforms: key = mix(seed + (sweep+1) gamma); cell e = w * stride + k owns key_e = mix(key + (e+1) gamma) and takes its
 * elements 1, 2, ... (m / 2^53 of the top 53 bits, 2^-54 in place of 0) in the recipe's order: the draws depend on
 * (seed, sweep, e) alone.  Every column is then normalised in the log domain in this association, FP64, no contraction:
 *     M_k = max over all w of lg_wk;  e_wk = exp(lg_wk - M_k);
 *     rows in chunks of 256 (chunk j = rows 256 j .. 256 j + 255); a chunk's sum adds its e_wk one after another in row
 *     order, starting from the chunk's first; Z_k adds the chunk sums one after another in chunk order;
 *     lik[w * stride + k] = e_wk / Z_k.
 * A column sums to 1 within 2 u rows (u = 2^-53); rows = 1 gives exactly 1.0.  A cell whose e_wk underflows is 0 (a dish
 * sweep gives such a class no weight at that dish; it happens for beta far below 1 only).  The bits do not depend on launch
 * geometry (STB_TLIK_WAVES = 1, 2, 4 or 8 waves a workgroup).  Five launches and one wait, for the error word; d_lik is
 * scratch between them.  Refused before anything is queued, with stb_last_error() set: a null array, rows or stride 0, a
 * beta that is not positive and finite.  A rejection loop that runs out, or a column whose Z_k is not positive and finite
 * (every lg_wk -inf: beta below 1e-300), fails the call after the wait; d_lik is then undefined.
 * stb_lik_loglik: the data term log p(classes | dishes, lik) = sum_wk cnt_wk log lik_wk.  x_wk = (double)cnt * log(lik)
 * where cnt > 0 and 0 where cnt = 0; a column's sum by the chunk association above (a chunk's x in row order, then the
 * chunks in order), then the columns one after another in k order.  A cell with cnt > 0 and lik = 0 counts in
 * *impossible_host (may be NULL) and makes the total -inf; a finite matrix >= 0 never gives a NaN.  Two launches; the
 * answer arrives through pinned memory: one wait.
 * Object layer, queued on the object's stream behind its sweeps; t, T, n and cust are not written and nothing per class,
 * dish or restaurant crosses to the host.
 *   stb_tindic_sample_lik  counts (class, dish) on the device over the matrix's shape and draws all of its rows x stride
 *                          cells into it (beta_host: the matrix's rows values, or NULL).  Classes and a matrix must be set,
 *                          the classes' rows <= the matrix's (stb_tindic_set_lik(s, NULL, rows, stride) makes one); rows
 *                          past the classes' and columns past the largest K_i have zero counts: drawn from the prior.
 *   stb_tindic_sample_h    dish k is local pair k of every restaurant, the dish sweep's convention.  c_k = sum of t_ik over
 *                          the restaurants with K_i > k; for k < Kmax = max_i K_i (1 <= Kmax <= STB_TD_MAXK) lg_k = log of a
 *                          Gamma(gamma_k + c_k) variate as above with e = k (gamma_host: Kmax values, or NULL for gamma0);
 *                          M = max lg_k, e_k = exp(lg_k - M), Z = the e_k added one after another in k order, h_k = e_k / Z,
 *                          written to every pair (i, k): it replaces the object's h, later sweeps and log joints see it.
 *                          The weights are one distribution over Kmax dishes; a restaurant with K_i < Kmax sees its first
 *                          K_i.  Equal seeds give _sample_lik and _sample_h one stream: give them different seeds.
 *   stb_tindic_loglik      the data term of the current state under the object's matrix; with stb_tindic_logjoint's total
 *                          it is the complete-data log joint log p(classes, n, t | a, b, h, lik)
 *   stb_tindic_get_h       the object's h[G] to the host (1 everywhere when none is set), after the queued work
 * Refused before anything is queued, the state as it was: a null object (or total / h_out); no classes or no matrix, or
 * classes with more rows than the matrix; a beta or gamma that is not positive and finite; for _sample_h an object created
 * with STB_TI_REF_ODDS, or Kmax outside 1 .. STB_TD_MAXK.  A draw that fails after its wait (above) leaves the matrix, or
 * h, undefined: stb_tindic_sweep_dishes (and, for the matrix, _loglik) is then refused until a _sample_lik / _sample_h
 * that succeeds, or a stb_tindic_set_lik / _set_h. */
int stb_sample_lik(const uint32_t *d_cnt, unsigned rows, unsigned stride, const double *beta_host /* rows, or NULL */,
                   double beta0, double *d_lik, uint64_t seed, uint64_t sweep, void *stream);
int stb_lik_loglik(const uint32_t *d_cnt, const double *d_lik, unsigned rows, unsigned stride, double *total_host,
                   uint64_t *impossible_host /* or NULL */, void *stream);
int stb_tindic_sample_lik(stb_tindic_t *s, const double *beta_host, double beta0, uint64_t seed, uint64_t sweep);
int stb_tindic_sample_h(stb_tindic_t *s, const double *gamma_host /* Kmax, or NULL */, double gamma0, uint64_t seed,
                        uint64_t sweep);
int stb_tindic_loglik(stb_tindic_t *s, double *total, uint64_t *impossible /* or NULL */);
int stb_tindic_get_h(stb_tindic_t *s, double *h_out);

/* ---- base weights per group of restaurants under a shared root (hgroups.hip; additive: the reference has no such step) ----
 * stb_tindic_sample_h draws one h for every restaurant.  Here restaurants 0 .. I-1 are cut into G contiguous ranges
 * goff[G+1] (stb_sample_bgroups' convention: 0 = goff[0] <= ... <= goff[G] = I, empty ranges allowed; d_goff NULL: every
 * restaurant its own group, G = I), each range with weights of its own that share strength through a root (the HDP / HPYP
 * structure):
 *     r ~ Dirichlet(gamma_1 .. gamma_Kmax);   h_g | r ~ Dirichlet(alpha r_1, .., alpha r_Kmax), alpha > 0;
 *     every table of a restaurant of group g draws its dish from h_g.
 * Dish k is local pair k of every restaurant and Kmax = max_i K_i <= STB_TD_MAXK, as for _sample_h.  c_gk = sum of t_ik over
 * the restaurants i of group g with K_i > k.  One call is one exact Gibbs step, in this order -- r and alpha are updated with
 * h integrated out, then h is drawn from its full conditional:
 *   1. c_gk (integers), C_g = sum_k c_gk.
 *   2. auxiliary tables from the Antoniak law: w = alpha * r_k (one FP64 product), then
 *        m_gk = [c_gk >= 1] + sum_{j=1}^{c_gk - 1} [u_j * (w + (double)j) < w]      (doubles as written, no contraction)
 *      M_g = sum_k m_gk, s_k = sum_g m_gk.
 *   3. r' ~ Dirichlet(gamma_k + s_k) (gamma_host: Kmax values, or NULL for gamma0), written over d_root.  Skipped with
 *      STB_HG_KEEP_ROOT (gamma is then not read).
 *   4. with STB_HG_SAMPLE_ALPHA: q_g ~ Beta(alpha, C_g) (C_g > 0), alpha' ~ Gamma(shape + sum_g M_g, rate = 1/scale + sum_g
 *      -log q_g): exactly stb_sample_bgroups with a = 0, I = G "restaurants" of N = C_g customers and T = M_g tables, one
 *      group {0, G}, every b = alpha, and seed ^ 0xA54FF53A5F1D36F1 (same sweep).  alpha' stays in a device word and feeds
 *      step 5 without passing through the host.  Without the flag alpha' = alpha and shape, scale are not read.
 *   5. h_g ~ Dirichlet(alpha' r'_k + c_gk) for every group (empty ranges too: a draw from the prior), written to every pair
 *      (i, k) with i in g and k < K_i, to d_hgrp[g * Kmax + k] when given; d_c and d_m receive c_gk and m_gk when given.
 * Uniforms: key = mix(seed + (sweep+1) gamma), the constant and mix of stb_sample_lik.  Cell e = g * Kmax + k (uint64) owns
 * key_e = mix(key + (e+1) gamma); its group variate takes key_e's elements 1, 2, ... by the log-Gamma recipe above, exactly
 * as _sample_h does with e = k; its u_j are element j of the substream mix(key_e ^ 0x59B1D5A7C3E9F24D) (stb_sample_bgroups'
 * y substream and open-interval unit).  Root cell k owns mix(key_R + (k+1) gamma), key_R = mix(key ^ 0x6A09E667F3BCC909).
 * Every draw depends on (seed, sweep, e) alone.  Each Dirichlet (the root, every group row) is normalised as _sample_h's:
 * shape_k = alpha' * r'_k + (double)c_gk (the root: gamma_k + (double)s_k), lg_k the log-Gamma variate, M = max lg_k,
 * e_k = exp(lg_k - M), Z the e_k added one after another in k order, h_k = e_k / Z; a row sums to 1 within 2 u Kmax.  So
 * with STB_HG_KEEP_ROOT, G = 1, alpha = 1 and d_root = gamma the call gives _sample_h(gamma)'s bits.  No bit depends on the
 * launch geometry (STB_HGROUPS_WAVES = 1, 2, 4 or 8 waves a workgroup) or on who takes a cell's Bernoulli draws
 * (STB_HGROUPS_FORM = lane | wave; default: a wave takes the cells with c_gk > 257).  tests/hh_oracle.py replays the step.
 * d_root (Kmax doubles, in: r, out: r') need only be positive and finite; it need not sum to 1.  All launches are queued
 * back to back on the stream; one wait, for the error and info words (with d_goff given, the raw call first reads the G + 1
 * offsets back to check them).  info (may be NULL): alpha' (alpha without the flag), tables = sum_g C_g, aux_tables =
 * sum_g M_g, the error word.
 * Refused before anything is queued, with stb_last_error() set and nothing written: a null d_koff, d_t, d_root, d_h or opts;
 * I < 1; Kmax outside 1 .. STB_TD_MAXK; G < 1, G != I without ranges, ranges that are not 0 = goff[0] <= ... <= goff[G] = I;
 * unknown flags; alpha, gamma (unless STB_HG_KEEP_ROOT) or shape, scale (with STB_HG_SAMPLE_ALPHA) not positive and finite.
 * Fails after the wait, error word: 1 a rejection loop ran out, 2 a Z is not positive and finite, 4 a shape
 * alpha r_k + c_gk is negative, infinite or NaN, 8 a group's C_g is above 2^32 - 1; or the concentration's draw was not a
 * positive finite double.  The outputs are then undefined.  A shape of exactly 0 is no failure: it is a base weight that
 * underflowed to 0 (a Dirichlet coordinate of a shape far below 1 is often smaller than the smallest double) under c_gk = 0,
 * its coordinate is 0 -- the limit of the draw -- and it takes no uniform.  (On the tree below, where a drawn row is the
 * base of the rows under it, that is a common event with many dishes and few tables, not a rare one.)
 * Object layer, queued on the object's stream behind its sweeps; ranges, root and alpha live with the object:
 *   stb_tindic_set_hgroups     the ranges (goff_host[G+1], checked as above; NULL: every restaurant its own group, the
 *                              state of a new object)
 *   stb_tindic_set_hroot       the root, Kmax positive finite values (NULL: 1/Kmax each, the state of a new object)
 *   stb_tindic_get_hroot       the root to the host, after the queued work
 *   stb_tindic_sample_hgroups  the step on the object's t.  opts->alpha > 0: the concentration of this step; opts->alpha = 0:
 *                              the one the last successful step left (info->alpha), refused when there is none.  It
 *                              replaces the object's h (one is made when it had none) and root; stb_tindic_set_h,
 *                              _sample_h, the sweeps, _logjoint, _predict and _heldout simply see the per-group h.
 * Refused, the object's h, root, ranges and alpha as they were: the refusals above, a null object, an object created with
 * STB_TI_REF_ODDS, the largest K_i outside 1 .. STB_TD_MAXK.  A step that fails after its wait leaves h and the root
 * undefined: stb_tindic_sweep_dishes is then refused until a _sample_hgroups / _sample_h that succeeds or a _set_h, as
 * after a failed _sample_h; give the root again with _set_hroot. */
#define STB_HG_KEEP_ROOT 1u
#define STB_HG_SAMPLE_ALPHA 2u
typedef struct stb_hgroups_opts {
  double alpha, gamma0, shape, scale;
  const double *gamma_host; /* Kmax, or NULL for gamma0 */
  unsigned flags, reserved;
} stb_hgroups_opts_t;
typedef struct stb_hgroups_info {
  double alpha;
  uint64_t tables, aux_tables;
  unsigned error_word, reserved;
} stb_hgroups_info_t;
int stb_sample_hgroups(int I, const uint64_t *d_koff, const uint16_t *d_t, unsigned Kmax, int G, const uint64_t *d_goff,
                       const stb_hgroups_opts_t *opts, double *d_root /* Kmax: in r, out r' */, double *d_h /* pairs, out */,
                       double *d_hgrp /* G x Kmax or NULL */, uint32_t *d_c /* G x Kmax or NULL */,
                       uint32_t *d_m /* G x Kmax or NULL */, uint64_t seed, uint64_t sweep, void *stream,
                       stb_hgroups_info_t *info);
int stb_tindic_set_hgroups(stb_tindic_t *s, int G, const uint64_t *goff_host /* G + 1, or NULL */);
int stb_tindic_set_hroot(stb_tindic_t *s, const double *root_host /* Kmax, or NULL */);
int stb_tindic_get_hroot(stb_tindic_t *s, double *root_out /* Kmax */);
int stb_tindic_sample_hgroups(stb_tindic_t *s, const stb_hgroups_opts_t *opts, uint64_t seed, uint64_t sweep,
                              stb_hgroups_info_t *info);

/* ---- base weights on a tree of nested groups (htree.hip; additive: the reference has no such step) ----
 * stb_sample_hgroups has two layers, groups under one root.  Here the tree has levels 1 .. L, 1 <= L <= STB_HT_MAXL (corpus ->
 * year -> author -> document):
 *   level 1 cuts the restaurants 0 .. I-1 into G_1 contiguous ranges off[0][G_1 + 1] (stb_sample_bgroups' convention:
 *   0 = off[0] <= ... <= off[G_1] = I, empty ranges allowed); level l + 1 cuts the G_l nodes of level l into G_(l+1) contiguous
 *   ranges off[l][G_(l+1) + 1] that end at G_l (childless nodes allowed); above level L sits the root.
 *     r ~ Dirichlet(gamma_1 .. gamma_Kmax);   h_v | h_par(v) ~ Dirichlet(alpha_l h_par(v)) for a node v of level l (the root
 *     its parent at level L);   every table of a restaurant of the level-1 node g draws its dish from h_g.
 * Dish k is local pair k of every restaurant and Kmax <= STB_TD_MAXK, as for _sample_h and _sample_hgroups.  Arrays over
 * levels (G_host, d_off, d_hnode, d_c, d_m, alpha, info's) are indexed l - 1: level 1 first.  One call is one exact Gibbs
 * step, in this order:
 *   1. level 1's counts c_gk (integers) and C_g, as stb_sample_hgroups' step 1.
 *   2. upwards, l = 1 .. L: for every node v and dish k, w = alpha_l * h_par(v),k (one FP64 product; h_par(v) the row that
 *      d_hnode holds for level l + 1 on entry, d_root at l = L), m_vk by stb_sample_hgroups' step 2 exactly as written there,
 *      M_v = sum_k m_vk; the next level's counts are the integer sums c_(par(v)),k = sum over the children of m_vk, C_par their
 *      sum over k (64-bit); at l = L the sums are s_k.  Only the auxiliary tables are handed up, never all tables.
 *   3. r' ~ Dirichlet(gamma_k + s_k), written over d_root.  Skipped with STB_HT_KEEP_ROOT (gamma is then not read).
 *   4. with STB_HT_SAMPLE_ALPHA: one stb_sample_bgroups step with a = 0 over all nodes of all levels concatenated (level 1's
 *      first) as "restaurants" of N = C_v customers and T = M_v tables, L ranges, one a level, b = alpha_l on level l's nodes,
 *      one shape and scale for every level, seed ^ 0xA54FF53A5F1D36F1 (same sweep).  alpha'_l stays in device words and feeds
 *      step 5.  With L = 1 this is stb_sample_hgroups' step 4.  Without the flag alpha'_l = alpha_l.
 *   5. downwards, l = L .. 1: h'_v ~ Dirichlet(alpha'_l * h'_par(v),k + c_vk) for every node (childless and empty ones too: a
 *      draw from the prior given the new parent); levels >= 2 are written over d_hnode[l - 1], level 1 to every pair (i, k)
 *      with k < K_i and to d_hnode[0] when given.  d_c[l - 1] and d_m[l - 1] receive c and m of level l when given.
 * Uniforms: key = mix(seed + (sweep+1) gamma); key_1 = key and key_l = mix(key ^ (0x3C6EF372FE94F82B + l)) for l >= 2.  Cell
 * e = v * Kmax + k (uint64) of level l owns key_e = mix(key_l + (e+1) gamma): its variate takes key_e's elements 1, 2, ..., its
 * u_j are element j of mix(key_e ^ 0x59B1D5A7C3E9F24D).  Root cell k owns mix(key_R + (k+1) gamma), key_R = mix(key ^
 * 0x6A09E667F3BCC909).  Every draw depends on (seed, sweep, level, cell) alone; with L = 1 every stream, every operation and
 * every output bit is stb_sample_hgroups'.  Each Dirichlet is normalised as stb_sample_hgroups': shape_k = alpha'_l *
 * h'_par,k + (double)c_vk.  No bit depends on the launch geometry (STB_HTREE_WAVES = 1, 2, 4 or 8 waves a workgroup) or on who
 * takes a cell's Bernoulli draws (STB_HTREE_FORM = lane | wave; default: a wave takes the cells with c_vk > 257, and where a
 * level has few rows several waves a slice of the draws each).  tests/ht_oracle.py replays the step.
 * The step is exact: going up, level l's h is integrated out when m of level l is drawn given the level above, so m is an
 * exact conditional of the model with the levels <= l summed out (dropping the stale row of level l + 1 before m of level
 * l + 1 is drawn marginalises a variable of a stationary sample); alpha_l | (C, M) of level l and r | s are exact conditionals
 * of that collapsed model; the downward draws restore the rows from their full conditionals, top first.
 * All launches are queued back to back on the stream; one wait (the raw call first reads every level's offsets back to check
 * them).  info (may be NULL): per level alpha', tables = sum_v C_v, aux_tables = sum_v M_v (entries past `levels`: NaN, 0).
 * Refused before anything is queued, with stb_last_error() set and nothing written: a null d_koff, d_t, G_host, d_off, a
 * d_off[l], d_root, d_hnode, a d_hnode[l] with l >= 1, d_h, opts or opts->alpha; I < 1; levels outside 1 .. STB_HT_MAXL; Kmax
 * outside 1 .. STB_TD_MAXK; a G_l < 1; ranges of a level that are not monotone from 0 to the size of the level below; unknown
 * flags; an alpha_l, gamma (unless STB_HT_KEEP_ROOT) or shape, scale (with STB_HT_SAMPLE_ALPHA) not positive and finite.
 * Fails after the wait with stb_sample_hgroups' error words (8: a node's C_v is above 2^32 - 1), or when a concentration's
 * draw was not a positive finite double.  The outputs are then undefined.
 * Object layer, queued on the object's stream behind its sweeps; the tree's ranges (independent of _set_hgroups'), the rows
 * and the concentrations live with the object, the root is _set_hroot's:
 *   stb_tindic_set_htree        levels, G_host[levels] and off_host[levels] (checked as above); the rows of the levels >= 2
 *                               are made and set to the object's root (1/Kmax each on a new object); the concentrations are
 *                               forgotten.  levels = 0 removes the tree
 *   stb_tindic_set_htree_level  the G_l x Kmax rows of a level l >= 2 (1-based), positive and finite
 *   stb_tindic_get_htree_level  a level's rows to the host, after the queued work; level 1: what the last step drew (refused
 *                               before the first)
 *   stb_tindic_sample_htree     the step on the object's t; opts->levels must be the tree's.  opts->alpha NULL: the
 *                               concentrations the last successful step left, refused when there are none.  It replaces the
 *                               object's h, root and stored rows; the sweeps, _logjoint, _loglik, _predict, the held-out calls
 *                               and _generate see the new h through the pairs.
 * Refusals and the rule that a step which fails after its wait blocks stb_tindic_sweep_dishes are stb_tindic_sample_hgroups'.
 * stb_tindic_logjoint_collapsed is refused on an object whose tree has two or more levels: its grouped formula is not this
 * model's. */
#define STB_HT_MAXL 8
#define STB_HT_KEEP_ROOT 1u
#define STB_HT_SAMPLE_ALPHA 2u
typedef struct stb_htree_opts {
  int levels;
  const double *alpha; /* [levels], level 1 first */
  double gamma0, shape, scale;
  const double *gamma_host; /* Kmax, or NULL for gamma0 */
  unsigned flags, reserved;
} stb_htree_opts_t;
typedef struct stb_htree_info {
  double alpha[STB_HT_MAXL];
  uint64_t tables[STB_HT_MAXL], aux_tables[STB_HT_MAXL];
  unsigned error_word, reserved;
} stb_htree_info_t;
int stb_sample_htree(int I, const uint64_t *d_koff, const uint16_t *d_t, unsigned Kmax, const int *G_host /* [levels] */,
                     const uint64_t *const *d_off /* [levels] */, const stb_htree_opts_t *opts, double *d_root /* Kmax: in r, out r' */,
                     double *const *d_hnode /* [levels]: level >= 2 in and out (G x Kmax); level 1 out or NULL */,
                     double *d_h /* pairs, out */, uint32_t *const *d_c, uint32_t *const *d_m /* [levels] or NULL, entries may be NULL */,
                     uint64_t seed, uint64_t sweep, void *stream, stb_htree_info_t *info);
int stb_tindic_set_htree(stb_tindic_t *s, int levels, const int *G_host /* [levels] */, const uint64_t *const *off_host /* [levels] */);
int stb_tindic_set_htree_level(stb_tindic_t *s, int level /* 2 .. levels */, const double *rows /* G x Kmax */);
int stb_tindic_get_htree_level(stb_tindic_t *s, int level /* 1 .. levels */, double *rows /* G x Kmax */);
int stb_tindic_sample_htree(stb_tindic_t *s, const stb_htree_opts_t *opts, uint64_t seed, uint64_t sweep, stb_htree_info_t *info);

/* ---- the log joint probability of a sampler state (logjoint.hip): what a Gibbs chain is watched by, what runs are
 * compared on, what annealed and bridge estimates of the evidence feed on.  Pairs, h, b_i and a as for stb_tcounts above;
 * T_i = sum_k t_ik, N_i = sum_k n_ik:
 *     log p(n, t | a, b, h) = sum_i L_i,     L_i = P_i + H_i + R_i
 *     P_i = sum_k S_S_a(n_ik, t_ik)            pairs with n >= 1 (stb_lookup_S's semantics; n = 0, t = 0 contributes 0)
 *     H_i = sum_k t_ik log h_ik                0 when h is NULL
 *     R_i = log (b_i|a)_{T_i} - log (b_i)_{N_i}
 *         = T_i log a + [lgamma(T_i + b_i/a) - lgamma(b_i/a)] - [lgamma(b_i + N_i) - lgamma(b_i)]      a > 0
 *         = T_i log b_i - [lgamma(b_i + N_i) - lgamma(b_i)]                                             a = 0
 *         = 0                                                                                           N_i = 0
 * This is the table-count representation, the law stb_sample_tcounts draws from: changing one pair's t from tau to tau'
 * changes the sum by log w(tau') - log w(tau), w as written there.  With STB_LJ_INDICATORS every pair with n >= 1 also
 * contributes -log C(n - 1, t - 1): the table-indicator representation, one indicator of a pair held at 1 and the other
 * n - 1 uniform given t, whose Gibbs step is stb_sample_tindic with the exact ratio t / (n - t) = C(n-1, t-1) / C(n-1, t)
 * (with C(n, t) the ratio would be (t + 1) / (n - t), which is not that step's).  lgamma is log |Gamma|: for -a < b_i < 0 (allowed when a > 0) Gamma(b_i/a) and Gamma(b_i) are both
 * negative, Gamma(T_i + b_i/a) and Gamma(b_i + N_i) both positive (b_i + N_i and b_i lie on opposite sides of zero exactly
 * when T_i + b_i/a and b_i/a do, and for b_i > -a > -1, N_i >= 1 no second sign change can happen), so the signs cancel and
 * the difference of the log |Gamma| values is the logarithm of a positive quotient.  b_i = 0 (a > 0) takes the limit.
 * One pass over the pairs, one table gather a pair; every sum in a fixed association (logjoint.hip's header; DESIGN.md
 * section 6), so the bits of every output depend on neither grid nor workgroup size (STB_LOGJOINT_WAVES = 1, 2, 4 or 8).
 *   impossible  pairs whose S_S is log 0 (t = 0 with n > 0, or t > n) or whose h is not positive and finite: the
 *               restaurant's L_i, the component (pairs, or base for h) and the total are -inf.  No NaN is ever produced
 *               (for b_i > -a, which the raw layer trusts as the sweeps do).
 *   outside     pairs the table cannot answer (n > N, or 1 < t < n with t > M or with no table): left out of the sums, as
 *               stb_sample_partition's cnt[0].  They still count in T_i and N_i.
 *   t_mismatch  restaurants with d_T[i] != sum_k t_ik (d_T given): a free check of the sweeps' invariant.  The kernel's
 *               own integer sum is the one used.
 * Raw layer: d_table / d_S1 one slab of stb_fill_S for `a` with bounds (N, M); either may be NULL when no pair has
 * min(n, M) >= 2 (stb_sample_tcounts' rule), and S^n_1 is then evaluated as the fill does, lgamma(n - a) - lgamma(1 - a).
 * d_Li: NULL, or I doubles on the device.  One launch, one wait; *total_host and *info (may be NULL) arrive through
 * pinned memory, as stb_sample_logq's Q.  I = 0 gives 0.  Refused before anything is queued, with stb_last_error() set: a
 * outside [0, 1), unknown flag bits, a null koff, n or t, I < 0.
 * Object layer: queued behind the object's sweeps on its stream; bpar (host [I]) is checked as by _sweep; neither t nor
 * T is written and a failure leaves the state as it was; Li_host (may be NULL) receives the I values L_i.
 * stb_tcounts_logjoint reads the object's S table, refilled when `a` differs from the table's, as in _sweep.
 * stb_tindic_logjoint needs an S slab of its own, the object holding only a V table: same bounds as the V table, taken
 * from the library's buffer cache on first use, filled by stb_fill_S and checked (stb_fill_status), refilled only when `a`
 * changes, given back when the object is freed.  It costs what the V table costs once more -- 8 stb_elems(N, M) bytes
 * plus 8 N for S^n_1 and the fill's workspace (stb_fill_workspace_bytes(N, M, 1)): 0.7 MB at max n = 200, M = 200.
 * Objects without a table (all n <= 1, or M = 1) work and read none. */
#define STB_LJ_INDICATORS 1u
typedef struct stb_logjoint_info {
  double pairs, base, restaurants, binom;      /* sum P_i, sum H_i, sum R_i, -sum log C(n-1, t-1) (0 without the flag); total = their sum */
  uint64_t outside, impossible, t_mismatch;
} stb_logjoint_info_t;
int stb_logjoint(const double *d_table, const double *d_S1, unsigned N, unsigned M, double a,
                 const double *d_bpar, int I, const uint64_t *d_koff, const uint32_t *d_n,
                 const uint16_t *d_t, const uint32_t *d_T /* or NULL */, const double *d_h /* or NULL */,
                 unsigned flags, double *d_Li /* NULL, or I doubles */, double *total_host,
                 stb_logjoint_info_t *info /* or NULL */, void *stream);
int stb_tcounts_logjoint(stb_tcounts_t *s, double a, const double *bpar, unsigned flags, double *total, double *Li_host,
                         stb_logjoint_info_t *info);
int stb_tindic_logjoint(stb_tindic_t *s, double a, const double *bpar, unsigned flags, double *total, double *Li_host,
                        stb_logjoint_info_t *info);

/* ---- the log marginal of multinomials under a Dirichlet prior, from a count matrix on the device (dirmult.hip) ----
 * For a multinomial with counts c_j, weights w_j, W = sum_j w_j and C = sum_j c_j:
 *     log ml = [lgamma(W) - lgamma(W + C)] + sum_j [lgamma(w_j + c_j) - lgamma(w_j)]
 * d_cnt is rows x stride uint32, its first cols columns the matrix.  STB_DM_ROWS: every row is a multinomial over its cols
 * cells, d_w holds cols weights; STB_DM_COLUMNS: every column is a multinomial over its rows cells, d_w holds rows weights.
 * Operation by operation (FP64, no contraction; dirmult.hip's header has the associations, DESIGN.md section 6 the bar):
 *     s = d_scale ? *d_scale (a device word) : scale;  w_j = s * d_w[j], one product (s = 1.0 changes no bit); d_w NULL:
 *     every w is s * w0
 *     rise(x, m) = log(x + 0.0) + log(x + 1.0) + ... + log(x + (double)(m - 1)), added in that order
 *     cell term   c = 0: exactly 0.0, nothing evaluated; 1 <= c <= 8: rise(w, c); c > 8: lgamma(w + (double)c) - lgamma(w)
 *     W           d_w NULL: (double)ncat * (s * w0); else the categories in chunks of 256, a chunk by a fixed tree, the
 *                 chunk sums in order in double-double
 *     normaliser  C = 0: 0.0; 1 <= C <= 8: -rise(W, C); else lgamma(W) - lgamma(W + (double)C).  C is a uint64
 *     a multinomial's value = its cells' sum + its normaliser (d_each: NULL, or one double a multinomial on the device)
 * Every sum has a fixed association, so no bit depends on the launch geometry (STB_DIRMULT_WAVES = 1, 2, 4 or 8 waves a
 * workgroup).  info (may be NULL): cells and norms are the two sums over all multinomials, the total their merged sum.
 *   zero_weight  cells with w = 0 and c = 0: they contribute 0 (an underflowed root coordinate)
 *   impossible   cells with w = 0 and c > 0: that multinomial's value, `cells` and the total are -inf
 *   error_word   1: a weight or the device's scale is negative, NaN or infinite; 2: W is not positive and finite.  The call
 *                then fails after its wait with the outputs undefined.  No input >= 0 and finite ever gives a NaN.
 * Two launches (the weights; the matrix, whose last workgroup to take a ticket adds the parts: nobody waits), one wait;
 * *total_host and *info arrive through pinned words.  rows = 0 gives 0.  Refused before anything is queued, with
 * stb_last_error() set and the outputs untouched: a null d_cnt or total_host; cols = 0 or cols > stride; neither or both
 * orientation flags, or unknown flags; w0 (d_w NULL) or scale (d_scale NULL) not positive and finite. */
#define STB_DM_ROWS    1u
#define STB_DM_COLUMNS 2u
typedef struct stb_dirmult_info {
  double cells, norms;              /* sum of the cell terms, sum of the normalisers; total = their sum */
  uint64_t nonzero, count;          /* cells with c > 0; sum of all c */
  uint64_t zero_weight, impossible; /* cells with w = 0 and c = 0 (contribute 0); cells with w = 0 and c > 0 */
  unsigned error_word, reserved;
} stb_dirmult_info_t;
int stb_dirmult_logml(const uint32_t *d_cnt, uint64_t rows, unsigned cols, unsigned stride, unsigned flags,
                      const double *d_w /* or NULL: every weight w0 */, double w0, double scale,
                      const double *d_scale /* or NULL; a device word that replaces `scale` */,
                      double *d_each /* NULL, or one double per multinomial */, double *total_host,
                      stb_dirmult_info_t *info /* or NULL */, void *stream);

/* ---- the collapsed log joint of a table-indicator object: base weights and class distributions summed out ----
 *     total = pairs + restaurants + binom     stb_tindic_logjoint's components with h absent, bit for bit
 *           + tables = sum_g log ml(c_g. ; alpha r)   STB_DM_ROWS on c_gk, the tables of group g that serve dish k, counted
 *                                                     by stb_sample_hgroups' own kernel over the object's ranges (none:
 *                                                     every restaurant its own group); weights the object's root (none:
 *                                                     1 / Kmax each) scaled by alpha.  STB_CJ_FLAT: one group over all
 *                                                     restaurants, weights gamma, scale 1 -- the model of _sample_h
 *           + data   = sum_k log ml(cnt_.k ; beta)    STB_CJ_DATA: STB_DM_COLUMNS on the (class, dish) counts over the
 *                                                     matrix's shape, the counts _sample_lik takes
 *           + root   = lgamma(sum gamma) - sum lgamma(gamma_k) + sum (gamma_k - 1) log(r_k / R)      STB_CJ_ROOT; R = sum r_k
 *                                                     in k order; cells with r_k = 0 are left out of the last sum and
 *                                                     counted in root_left_out (one workgroup; dirmult.hip, k_dm_root)
 * added in that order in plain doubles: -inf when any component is impossible, never NaN.  h and the matrix's values are
 * not read: the quantity is finite wherever the state is possible, however small alpha r_k or beta are.  The Gamma
 * hyper-priors of alpha and b are closed-form scalars the caller adds.  opts: alpha > 0, or 0 for the one the last
 * successful _sample_hgroups left (not read with STB_CJ_FLAT); gamma (read with STB_CJ_FLAT or STB_CJ_ROOT) and beta
 * (read with STB_CJ_DATA) as a host vector or, when that is NULL, one value for every cell.  Everything is queued on the
 * object's stream behind its sweeps; nothing per restaurant, group, dish or class crosses to the host; t, T, n, cust, h,
 * the root and the matrix are not written.  The count matrices come from the buffer cache and go back: G Kmax uint32 --
 * what _sample_hgroups takes for its c -- and the matrix's shape in uint32.
 * Refused, with the state, *total and *info as they were: a null object, opts or total; unknown flags; STB_CJ_ROOT with STB_CJ_FLAT; alpha = 0
 * while the object holds none, alpha not positive and finite; gamma or beta (when read) not positive and finite;
 * STB_CJ_DATA without classes or a matrix shape, or with more class rows than the matrix has; an object created with
 * STB_TI_REF_ODDS; the largest K_i outside 1 .. STB_TD_MAXK; a and bpar as _logjoint checks them (STB_BPAR_RESIDENT is
 * accepted). */
#define STB_CJ_INDICATORS 1u   /* as STB_LJ_INDICATORS */
#define STB_CJ_FLAT       2u   /* the model of _sample_h: one multinomial over all restaurants, w = gamma */
#define STB_CJ_DATA       4u   /* add the classes' term (classes and a matrix shape must be set) */
#define STB_CJ_ROOT       8u   /* add log p(r | gamma) (not with STB_CJ_FLAT) */
typedef struct stb_cj_opts {
  double alpha;                       /* > 0, or 0: the one the last successful _sample_hgroups left */
  double gamma0, beta0;
  const double *gamma_host /* Kmax or NULL */, *beta_host /* the matrix's rows or NULL */;
} stb_cj_opts_t;
typedef struct stb_cj_info {
  double pairs, restaurants, binom;   /* stb_tindic_logjoint's, with h absent */
  double tables, data, root;          /* the two integrated terms; log p(r | gamma) */
  stb_logjoint_info_t lj;
  stb_dirmult_info_t dm_tables, dm_data;
  uint64_t root_left_out;
} stb_cj_info_t;
int stb_tindic_logjoint_collapsed(stb_tindic_t *s, double a, const double *bpar, unsigned flags,
                                  const stb_cj_opts_t *opts, double *total, stb_cj_info_t *info /* or NULL */);

/* ---- the scale of Dirichlet weights shared by many multinomials, drawn on the device (dirconc.hip) ----
 * The two Dirichlet hyper-parameters the calls above take from the host -- beta of every dish's class distribution
 * (stb_sample_lik, STB_CJ_DATA) and gamma of the flat base weights (_sample_h, STB_CJ_FLAT) -- and the alpha of base
 * weights under a root are all the scale s of weights w_j = s * v_j that many multinomials share.  With the prior
 * s ~ Gamma(shape, scale) (stb_sample_bgroups' convention: mean shape * scale), V = sum_j v_j, counts c_mu,j and
 * n_mu = sum_j c_mu,j:
 *     p(s | c) ~ p(s) prod_mu Gamma(sV) / Gamma(sV + n_mu) prod_j Gamma(s v_j + c_mu,j) / Gamma(s v_j)
 * d_cnt, rows, cols, stride, flags, d_w and w0 are stb_dirmult_logml's: STB_DM_ROWS a multinomial a row over cols
 * categories (d_w: cols values), STB_DM_COLUMNS a multinomial a column over rows categories (d_w: rows values); d_w NULL:
 * every v is w0.  One call is one exact Gibbs step (FP64, no contraction; DESIGN.md section 6 derives it):
 *   1. n_mu (uint64).  V: stb_dirmult_logml's W with scale 1 -- d_w NULL: (double)ncat * w0; else chunks of 256 by the fixed
 *      tree, the chunk sums in order in double-double.  A total n_mu above 2^32 - 1 sets error bit 8, and step 2 then
 *      makes no draw at all: the call fails within milliseconds.
 *   2. auxiliary tables: w = s * v_j (one product), m_mu,j = [c >= 1] + sum_{i=1}^{c-1} [u_i * (w + (double)i) < w]
 *      (stb_sample_hgroups' step 2 unchanged); M_mu = sum_j m_mu,j.  Integers: no bit depends on the launch geometry.
 *   3. B = s * V, scale_B = scale * V (one product each; s ~ Gamma(shape, scale) <=> sV ~ Gamma(shape, scale V)); then
 *      exactly stb_sample_bgroups with a = 0, a "restaurant" per multinomial (N = n_mu, T = M_mu), one group {0,
 *      #multinomials}, every b = B, 1/scale = 1.0 / scale_B and seed ^ 0xA54FF53A5F1D36F1 (same sweep), as
 *      stb_sample_hgroups' step 4; s' = B' / V, one division.
 * Uniforms: key = mix(seed + (sweep+1) gamma).  Cell e = mu * cols + j for rows (stb_sample_hgroups' g * Kmax + k), j * stride
 * + mu for columns (stb_sample_lik's w * stride + k); u_i is element i of mix(mix(key + (e+1) gamma) ^ 0x59B1D5A7C3E9F24D).
 * So STB_DM_ROWS on stb_sample_hgroups' c_gk with v = r, s = alpha gives that call's m and, when r sums to exactly 1.0, its
 * alpha' to the bit.  No bit of any output depends on STB_DIRCONC_WAVES = 1, 2, 4 or 8 waves a workgroup or on who takes a
 * cell's draws (STB_DIRCONC_FORM = lane | wave; default: its wave takes a cell with c > 257).  tests/dc_oracle.py replays it.
 * info (required): s = s'; count = sum n; aux_tables = sum M; nonempty = multinomials with n > 0; zero_weight = cells with
 * v = 0 and c = 0, which contribute nothing; the error word.  d_m (NULL, or rows x stride uint32: m at the matrix's own
 * index, 0 in the padding) and d_M (NULL, or one uint32 a multinomial).  All launches are queued back to back on the
 * stream; one wait, for the pinned words.  A multinomial without counts contributes nothing.
 * Refused before anything is queued, with stb_last_error() set and the outputs untouched: a null d_cnt or info; cols = 0 or
 * cols > stride; neither or both orientation flags, or unknown flags; w0 (d_w NULL), s, shape or scale not positive and
 * finite; rows = 0; more multinomials than an int holds.
 * Fails after the wait, error word: 1 a v is negative, NaN or infinite; 2 V is not positive and finite; 4 a cell with
 * v = 0 holds a count; 8 a total above 2^32 - 1; or stb_sample_bgroups' own failures, or an s' that is not a positive
 * finite double.  info->s is then NaN and d_m, d_M undefined.
 * Object layer, queued on the object's stream behind its sweeps; t, T, n, cust, h, the root and the matrix are not written:
 *   stb_tindic_sample_beta   STB_DM_COLUMNS on the (class, dish) counts over the matrix's shape (what _sample_lik takes):
 *                            beta_w = s * base_w, base_host the matrix's rows values or NULL for 1 each.  A dish without
 *                            customers contributes nothing.  Refused as _sample_lik refuses (a null object, no classes, no
 *                            matrix, more class rows than the matrix has, base not positive and finite), and as above
 *   stb_tindic_sample_gamma  the flat model of _sample_h: STB_DM_ROWS on the one row c_k = sum_i t_ik (stb_sample_hgroups'
 *                            counting kernel over one range), gamma_k = s * base_k, base_host Kmax values or NULL for 1
 *                            each.  Refused as _sample_h refuses (STB_TI_REF_ODDS, Kmax outside 1 .. STB_TD_MAXK), and as above
 * The caller passes s' (times its base) on to _sample_lik, _sample_h and stb_cj_opts_t. */
typedef struct stb_dirconc_info {
  double s;                      /* s' (NaN after a failure) */
  uint64_t count, aux_tables;    /* sum n_mu, sum M_mu */
  uint64_t nonempty;             /* multinomials with n_mu > 0 */
  uint64_t zero_weight;          /* cells with v = 0 and c = 0 */
  unsigned error_word, reserved;
} stb_dirconc_info_t;
int stb_sample_dirconc(const uint32_t *d_cnt, uint64_t rows, unsigned cols, unsigned stride, unsigned flags,
                       const double *d_w /* or NULL: every v is w0 */, double w0, double s, double shape, double scale,
                       uint32_t *d_m /* rows x stride or NULL */, uint32_t *d_M /* one a multinomial or NULL */, uint64_t seed,
                       uint64_t sweep, void *stream, stb_dirconc_info_t *info);
int stb_tindic_sample_beta(stb_tindic_t *s, const double *base_host /* the matrix's rows, or NULL: 1 each */, double s_in,
                           double shape, double scale, uint64_t seed, uint64_t sweep, stb_dirconc_info_t *info);
int stb_tindic_sample_gamma(stb_tindic_t *s, const double *base_host /* Kmax, or NULL: 1 each */, double s_in, double shape,
                            double scale, uint64_t seed, uint64_t sweep, stb_dirconc_info_t *info);

/* ---- the launch geometry of the ticket reductions (for tests) ----
 * stb_sample_logq (k_logq), stb_joint_terms (k_joint_terms) and stb_logjoint (k_logjoint) share one design: workgroups take
 * steps of `chunks` blocks of 256 restaurants grid-stride in x -- step blockIdx.x, then + grid_x, ... -- (k_joint_terms
 * also the b_j grid-stride in y), write block sums to a per-thread buffer, and the last workgroup to take a ticket adds the
 * blocks in order.  stb_reduce_geometry says what a call on I >= 1 restaurants (and, for STB_GEOM_JOINT_TERMS, a D x J
 * grid) launches on the current device: it is computed by the function the three launch sites compute their launch
 * from, so it cannot drift from them.  waves = 1, 2, 4 or 8 waves a workgroup; 0: what the call itself would take now
 * (STB_HYPERQ_WAVES / STB_HYPERJ_WAVES / STB_LOGJOINT_WAVES, else the default).  need / cap0: what the call needs of the
 * buffer of block sums and what the buffer holds when first allocated -- in block sums, and for STB_GEOM_JOINT_TERMS in
 * doubles (a block sum is D J of them); a call with need > cap0 replaces the buffer.  No device work.  Returns 0, or
 * non-zero with stb_last_error() set for an unknown `which`, waves, I = 0 or a grid outside 1..64. */
#define STB_GEOM_LOGQ 0
#define STB_GEOM_JOINT_TERMS 1
#define STB_GEOM_LOGJOINT 2
typedef struct stb_reduce_geom {
  unsigned grid_x, grid_y;   /* workgroups */
  unsigned steps, chunks;    /* steps in all, blocks of 256 restaurants a step */
  unsigned blocks, waves;    /* blocks of 256 restaurants in all, waves a workgroup */
  uint64_t need, cap0;
} stb_reduce_geom_t;
int stb_reduce_geometry(int which, uint64_t I, int D, int J, int waves, stb_reduce_geom_t *out);

/* ---- what a state predicts: dish proportions and held-out customers (predict.hip) ----
 * Pairs (n_k, t_k, h_k), k < K_i, b_i and a as for stb_sample_tdish; T_i = sum_k t_k, N_i = sum_k n_k.  Given the seating,
 * the next customer of restaurant i sits at an existing table of dish k with weight n_k - t_k a and opens a new table
 * serving k with weight (b_i + T_i a) h_k; the sizes of the tables do not enter.  So
 *     theta_ik = ((n_k - t_k a) + g_i h_k) / (b_i + N_i),     g_i = b_i + T_i a
 *     p_c      = sum_k theta_ik lik[cls_c stride + k]         a held-out customer c of restaurant i
 * the state's exact one-step predictive: with S^{n+1}_{t'} = (n - t' a) S^n_{t'} + S^n_{t'-1},
 * p(n + e_k, t) + p(n + e_k, t + e_k) = p(n, t) theta_k(t) term by term, and summing over t gives
 * E_{t|n}[theta_k] = p(n + e_k) / p(n).  No Stirling table is read.  sum_k theta_ik = 1 exactly when the restaurant's
 * h sums to 1 -- after stb_tindic_sample_h that is every restaurant with K_i = Kmax; otherwise theta is the
 * sub-probability on the listed dishes, and p_c the probability that the customer is of class cls_c AND eats a listed dish.
 * The estimate of a held-out set's log likelihood over S states of a chain is sum_c log((1/S) sum_s p_c^(s)), not the
 * mean of the states' logs: STB_PR_ACCUMULATE adds a state's p_c into the caller's p, stb_heldout_loglik divides by S.
 *
 * stb_predict_dishes (k_predict), one wave a restaurant.  The arithmetic is part of the contract (FP64, no contraction;
 * tests/pr_oracle.py replays it):
 *   T_i and N_i are the kernel's own uint64 sums over the restaurant's pairs (no d_T is read).
 *   T = (double)T_i, N = (double)N_i, n = (double)n_k, t = (double)t_k, b = d_bpar[i], h = d_h[pair] (1.0 without d_h):
 *       g = b + T * a        den = b + N        x = n - t * a        theta = (x + g * h) / den
 *   each one product, then one sum, left to right as written, then the one division.  N_i = 0: theta = h, no division.
 *   L_k = d_lik[cls * stride + k]; 0.0 when cls >= rows; 1.0 without d_lik.  q_k = theta_k * L_k.
 *   Dishes are taken in blocks of 64, lane l the dish 64 j + l of block j (+0.0 past K_i); a block is summed by the
 *   64-lane shuffle tree of stb_logjoint, v += shfl_down(v, o), o = 32, 16, .. 1, lane 0 taken: s_j.  p_c = s_0, then
 *   p_c = p_c + s_j for j = 1, 2, .. in plain doubles.
 *   theta: d_theta NULL, or I rows of tstride doubles; columns K_i .. tstride-1 are written 0.
 *   p: d_p[c], c the flat held-out index -- CSR over d_hoff[I + 1], classes d_hcls[d_hoff[I]]; d_hoff NULL: no held-out
 *   customers.  With STB_PR_ACCUMULATE d_p[c] = d_p[c] + p_c (one lane owns a customer: S calls give the bits of the S
 *   values added in call order), else d_p[c] = p_c.
 *   skipped  a restaurant with K_i > STB_TD_MAXK, K_i > stride (with a matrix) or K_i > tstride (with d_theta): its
 *            theta row is 0, its customers' p is 0 when overwriting and left alone when accumulating; *d_skipped (NULL,
 *            or one uint64 on the device) is increased by their number.
 * The bits depend on neither grid nor workgroup size (STB_PREDICT_WAVES = 1, 2, 4 or 8 waves a workgroup; default 4),
 * nor on which restaurants share a call: K_i <= 64 keeps theta in registers and K_i > 64 in LDS, chosen per restaurant,
 * the arithmetic the same.  No wait: the call returns when the launch is queued.
 *
 * stb_heldout_loglik (k_heldout_sum): x_c = log(d_p[c] / (double)samples).  A customer whose d_p[c] / samples is not a
 * positive finite number (0, negative, inf, NaN, or a quotient that underflows to 0) is impossible: it adds +0.0 to the
 * sums and is counted; its restaurant's H_i and the total are -inf.  No NaN is ever produced.  Per restaurant the x_c are
 * taken in chunks of 64 in CSR order through the same tree (+0.0 past the end), the chunk sums added in order in
 * double-double, H_i = hi + lo (d_Hi: NULL, or I doubles on the device).  Over restaurants: stb_logjoint's association,
 * geometry and ticket (blocks of 256 in the one fixed tree, block sums added in block order in double-double by the last
 * workgroup; stb_reduce_geometry(STB_GEOM_LOGJOINT, I, 0, 0, waves) is the launch, waves STB_PREDICT_WAVES where it is
 * set, else stb_logjoint's choice).  One launch, one wait; *total_host and *info arrive through pinned memory.  info:
 * impossible customers, customers = d_hoff[I] - d_hoff[0], skipped = 0 (the object layer puts k_predict's count there).
 * I = 0 or no customers gives 0.
 * Both calls refuse before anything is queued, with stb_last_error() set: a outside [0, 1), a null required array (koff,
 * n, t, bpar; p, hoff and total_host for the sum), d_hoff without d_hcls and d_p, a matrix with rows or stride 0, d_theta
 * with tstride 0, samples 0, unknown flag bits, I < 0.
 *
 * Object layer, on an stb_tindic_t: queued on the object's stream behind its sweeps; none of it writes n, t, T, cust, h
 * or the matrix; a and bpar are arguments, as for _sweep and _logjoint.
 *   stb_tindic_set_heldout    hoff[I + 1] (hoff[0] = 0, non-decreasing) and the classes hcls[hoff[I]] from the host,
 *                             every class < the matrix's rows when a matrix is set (checked again at use).  Allocates
 *                             the accumulator p[hoff[I]], zeroes it and sets the sample count to 0.  hoff NULL removes
 *                             the held-out customers.
 *   stb_tindic_predict        theta to the host, I x tstride, tstride >= the largest K_i
 *   stb_tindic_heldout        without flags: the current state's sum_c log p_c through a scratch p; the accumulator is
 *                             left alone.  With STB_PR_ACCUMULATE: adds the state's p_c into the accumulator, counts the
 *                             sample (S), and returns the running estimate sum_c log(acc_c / S).  Hi_host (or NULL)
 *                             receives the I values H_i.
 *   stb_tindic_heldout_reset  zeroes the accumulator and S
 *   stb_tindic_heldout_get    the accumulator (p_out: hoff[I] doubles, or NULL) and S (or NULL) to the host
 * Refused, the state and the accumulator as they were: no held-out set (_heldout, _heldout_reset, _heldout_get); a, bpar
 * as _sweep refuses them; h left undefined by a failed stb_tindic_sample_h, or (_heldout) the matrix by a failed
 * _sample_lik; a held-out class >= the matrix's rows; some K_i > STB_TD_MAXK; tstride below the largest K_i. */
#define STB_PR_ACCUMULATE 1u
typedef struct stb_predict_info { uint64_t skipped, impossible, customers; } stb_predict_info_t;
int stb_predict_dishes(double a, const double *d_bpar, int I, const uint64_t *d_koff, const uint32_t *d_n,
                       const uint16_t *d_t, const double *d_h /* NULL: 1 */,
                       double *d_theta /* NULL, or I x tstride */, unsigned tstride,
                       const uint64_t *d_hoff /* I+1, or NULL: no held-out customers */, const uint32_t *d_hcls,
                       const double *d_lik /* NULL: 1 */, unsigned rows, unsigned stride,
                       double *d_p, unsigned flags, uint64_t *d_skipped /* NULL, or one uint64 the call adds to */,
                       void *stream);
int stb_heldout_loglik(const double *d_p, const uint64_t *d_hoff, int I, unsigned samples,
                       double *d_Hi /* NULL, or I */, double *total_host, stb_predict_info_t *info /* or NULL */,
                       void *stream);
int stb_tindic_set_heldout(stb_tindic_t *s, const uint64_t *hoff_host /* I+1, or NULL */, const uint32_t *hcls_host);
int stb_tindic_predict(stb_tindic_t *s, double a, const double *bpar, double *theta_host, unsigned tstride);
int stb_tindic_heldout(stb_tindic_t *s, double a, const double *bpar, unsigned flags, double *total,
                       double *Hi_host /* or NULL */, stb_predict_info_t *info /* or NULL */);
int stb_tindic_heldout_reset(stb_tindic_t *s);
int stb_tindic_heldout_get(stb_tindic_t *s, double *p_out /* or NULL */, unsigned *samples /* or NULL */);

/* ---- seating customers one by one: start states and the likelihood of unseen documents (seat.hip) ----
 * The Chinese-restaurant seating run forwards.  Restaurant i has pairs (n_k, t_k, h_k), T = sum t, N = sum n, b_i and a.
 * The next customer, of class w, sits in dish k at an old table with weight L_k (n_k - t_k a) and at a new one with
 * weight L_k (b + T a) h_k, both over b + N, L_k = lik[w stride + k]: the theta of stb_predict_dishes.  Seat a sequence
 * of customers this way, each (dish, old or new) drawn from those weights, and let W = prod_c p_c, p_c = sum_k theta_k
 * L_k on the state before c.  Then for every final state (z, t)
 *     sum over the paths that reach (z, t) of P(path) W(path)
 *         = (b|a)_T / (b)_N  prod_k S^{n_k}_{t_k} h_k^{t_k}  prod_c L[cls_c][z_c],
 * the unnormalised joint of the dish sweep.  So E[W] = p(w_1 .. w_N | L, h, a, b), the marginal
 * likelihood of the sequence with the seating summed out: log((1/R) sum_r W_r) over R independent particles estimates
 * its log (sequential importance sampling, the particle form of the left-to-right evaluation); and with L = 1 the
 * final state is an exact draw from the prior.  With a truncation M (no new table in a dish that has t = M) the same
 * holds over the states with t <= M.  No Stirling table is read.
 *
 * stb_seat_customers (k_seat): one wave per (restaurant, particle), lanes over dishes; K_i <= 64 keeps the state in
 * registers, larger K_i in LDS, chosen per restaurant.  n and t on entry are the start state (all zero: an empty
 * restaurant); T_i and N_i are the kernel's own integer sums over the pairs.  The customers to seat are CSR over
 * d_coff[I + 1] with classes d_cls (read only with a matrix).  The arithmetic is part of the contract (FP64, no
 * contraction, left to right as written, conversions to double first; tests/st_oracle.py replays it).  The stream of
 * particle r is that of sweep `sweep + r`: key = mix(seed + (sweep + r + 1) gamma), element j = stb_unit(key, j); C =
 * d_coff[I], c the flat customer index.  A visit to customer c of class w, on the particle's private (n_k, t_k, T, N):
 *   1. g = b + T * a;  den = b + N;  x_k = n_k - t_k * a;  y_k = (n_k >= 1 && t_k + 1 > M) ? 0 : g * h_k;
 *      theta_k = N == 0 ? h_k : (x_k + y_k) / den;  L_k as stb_predict_dishes (0 when w >= rows, 1 without a matrix);
 *      q_k = theta_k * L_k.  (h = 1.0 without d_h.)
 *   2. the cumulative sums of q in the dish sweep's association: blocks of 64 dishes (+0.0 past K_i), a Kogge-Stone
 *      inclusive scan inside a block, the block bases added in sequence; Z = the last base, p_c = Z.  thr = u3 * Z, u3 =
 *      element 2C + 1 + c; k* = the smallest k with q_k > 0 and cum_k > thr, else the largest k with q_k > 0.
 *   3. impossible -- Z not positive and finite: p_c = 0, the particle's log weight is -inf, the visit is counted; so
 *      that a committed state stays valid the customer is seated by the same rule on q_k = theta_k, with the same u3; if
 *      that sum is not positive and finite either (h <= 0) it is seated at k = 0 and the visit is counted as stuck.
 *   4. new = n_k* == 0 || u2 * (x + y) < y, with k*'s x and y and u2 = element 2c + 2.  n_k* += 1, N += 1; if new:
 *      t_k* += 1, T += 1.  M = 0 means 65535 (t is a uint16).
 *   5. lw += log(p_c) in seating order, in double-double; at the end lw = hi + lo.  d_lw[i particles + r] = lw.
 * The bits of n, t, T, cust and every p_c depend on (seed, sweep, r, c, C) and the start state alone: not on the waves
 * of a workgroup (STB_SEAT_WAVES = 1, 2, 4 or 8; default 4), the register or LDS form, or which restaurants share the
 * call.  Without STB_SEAT_COMMIT nothing but d_lw is written.  With it particles must be 1, and n, t, d_T[i] = T,
 * d_cust[c] = k* and (d_p non-null) d_p[c] = p_c are written.  A restaurant with K_i > STB_TD_MAXK, K_i > stride (with a
 * matrix), or K_i = 0 with customers is left untouched, its lw is 0 and it is counted in skipped.  d_info: NULL, or
 * three uint64 on the device the call adds to: skipped restaurants, impossible visits, stuck visits (visits counted
 * per particle).  No wait: the call returns when the launch is queued.
 *
 * stb_seat_loglik (k_seat_sum): per restaurant m = max_r lw_r, s = sum_r exp(lw_r - m) in particle order in plain
 * doubles, H_i = m + log(s / (double)R).  Every lw_r -inf: H_i = -inf, no NaN, the restaurant is counted
 * (info->impossible; the other counters of info are 0) and the total is -inf.  Over restaurants: stb_logjoint's
 * association, geometry and ticket, as stb_heldout_loglik (waves STB_SEAT_WAVES where it is set).  One launch, one wait;
 * *total_host arrives through pinned memory.
 * Refused before anything is queued, with stb_last_error() set: what stb_predict_dishes refuses (a outside [0, 1), a
 * null koff, n, t, coff or bpar, a matrix without classes or with rows or stride 0, I < 0), M > 65535, particles = 0 or
 * > 4096, STB_SEAT_COMMIT with particles != 1 or without d_T and d_cust, unknown flags, a null d_lw or total_host.
 *
 * Object layer, on an stb_tindic_t, queued on the object's stream:
 *   stb_tindic_seat         forgets the object's seating and seats all its C customers in CSR order from empty
 *                           restaurants, under the object's classes and matrix (the prior when none is set): writes n,
 *                           t, T and cust.  It does to the bounds what the first dish sweep does (the customer sequence
 *                           exists, N = max(3, max_i N_i), M as given at create, the largest n vouched for is max_i N_i),
 *                           so every later call works on the result with no read-back.  *total = sum_i lw_i.  info:
 *                           skipped, impossible, stuck as above, customers = C.  Refused as stb_tindic_sweep_dishes
 *                           refuses, the state as it was.
 *   stb_tindic_heldout_seq  the held-out customers of stb_tindic_set_heldout seated in their order on a private copy of
 *                           every restaurant's current state, `particles` times: *total = sum_i H_i, Hi_host (or NULL)
 *                           the I values.  An all-empty object with a trained matrix and h scores unseen documents.
 *                           Writes nothing of the object, not the state, not the accumulator.  info: the seating's
 *                           counters over all particles, customers = hoff[I].  Refused as stb_tindic_heldout refuses. */
#define STB_SEAT_COMMIT 1u
typedef struct stb_seat_info { uint64_t skipped, impossible, stuck, customers; } stb_seat_info_t;
int stb_seat_customers(double a, const double *d_bpar, int I, const uint64_t *d_koff, uint32_t *d_n, uint16_t *d_t,
                       uint32_t *d_T /* NULL unless COMMIT */, const double *d_h /* NULL: 1 */, unsigned M,
                       const uint64_t *d_coff /* I+1: the customers to seat */, const uint32_t *d_cls, uint32_t *d_cust,
                       const double *d_lik /* NULL: 1 */, unsigned rows, unsigned stride, unsigned particles,
                       unsigned flags, uint64_t seed, uint64_t sweep, double *d_lw /* I x particles */,
                       double *d_p /* C, or NULL */, uint64_t *d_info /* NULL or 3 uint64 added to */, void *stream);
int stb_seat_loglik(const double *d_lw, int I, unsigned particles, double *d_Hi /* NULL, or I */, double *total_host,
                    stb_seat_info_t *info /* or NULL */, void *stream);
int stb_tindic_seat(stb_tindic_t *s, double a, const double *bpar, uint64_t seed, uint64_t sweep,
                    double *total /* or NULL */, stb_seat_info_t *info /* or NULL */);
int stb_tindic_heldout_seq(stb_tindic_t *s, double a, const double *bpar, unsigned particles, uint64_t seed,
                           uint64_t sweep, double *total, double *Hi_host /* or NULL */, stb_seat_info_t *info /* or NULL */);

/* ---- the seating as a particle filter: resampling between customers (seat_pf.hip) ----
 * stb_seat_customers' R particles never meet: W_r is a product of N predictives, for a document of a few hundred
 * customers all but one of the R weights are negligible, and log((1/R) sum W_r) is in effect one particle's.  Here the R
 * particles ("slots") of a restaurant seat each customer side by side, and after a customer the light ones may be
 * replaced by copies of the heavy ones.  The estimate Zhat (H_i = log Zhat) stays unbiased for p(w_1 .. w_N | L, h, a, b):
 * a step without resampling preserves E[Zm (1/R) sum_r w_r p(future | state_r)] as E[p_c p(future | next)] = p(future |
 * state); systematic resampling gives slot r an expected R w_r / S1 offspring; and the decision is a function of the
 * present system with both branches preserving the expectation (tests/test_pf_host.py enumerates it).
 *
 * stb_seat_filter (k_seat_pf): one workgroup per restaurant.  A visit of slot r to customer c is stb_seat_customers'
 * visit, word for word (steps 1 to 4 above: theta, q, the cumulative sums, k*, the impossible and stuck rules, new or old
 * from u2), with u2 and u3 from the stream of sweep `sweep + r`: a run that never resamples seats slot r exactly as
 * k_seat seats particle r.  Per restaurant: weights w_r (doubles, 1.0 at the start), a running factor Zm (1.0) and an
 * exponent E (int64, 0).  After all R slots have seated customer c, with p_c(r) the visit's p:
 *   1. w_r = w_r * p_c(r) (an impossible visit has p = 0: the particle is dead, and still seated by the fallback rule).
 *   2. e = the largest ilogb(w_r) over the w_r > 0.  None: the restaurant is dead, H_i = -inf, it is counted; the other
 *      customers are still seated with no more weight work.  Else w_r = +0.0 where ilogb(w_r) < e - 1000, ldexp(w_r, -e)
 *      elsewhere, and E += e.  (No subnormal arises.)
 *   3. cum = the cumulative sums of w in the dish sweep's association (one block: slot r in lane r, +0.0 past R: so R <=
 *      STB_PF_MAXR = 64); S1 = the last; S2 = the last of the same scan over w_r * w_r.
 *   4. resample iff c is not the restaurant's last customer and S1 * S1 < (tau * (double)R) * S2.  (tau = 0: never.)
 *   5. Zm = Zm * (S1 / (double)R); ez = ilogb(Zm), Zm = ldexp(Zm, -ez), E += ez.  u4 = element 2c + 1 of slot 0's stream
 *      (the dish sweep's u1: seating never draws it).  thr_j = (((double)j + u4) / (double)R) * S1; the ancestor A_j = the
 *      smallest r with w_r > 0 and cum_r > thr_j, else the largest r with w_r > 0.  Slot j becomes a copy of slot A_j's
 *      (n, t, T, N) -- it keeps its own stream -- and w_j = 1.0.  The restaurant's resampling count goes up by one.
 *   6. after the last customer v = Zm * (S1 / (double)R), H_i = log(v) + (double)E * ln 2 (v = 0: -inf, never NaN).  No
 *      customers: H_i = 0.
 * Only + - x /, comparisons, conversions, ilogb and ldexp by integers decide the path: every slot's final (n, t), every
 * w_r, E and the resampling count are bit-equal to tests/pf_oracle.py's replay whatever the waves of a workgroup
 * (STB_SEAT_WAVES = 1, 2, 4 or 8), the register or LDS form, or whoever shares the launch; H_i holds one logarithm.
 * The start state (d_n, d_t) is read and never written.  Outputs: d_Hi[I]; optional d_w[I x R] and d_E[I] (after the
 * last customer's step 2), d_res[I], and the final states d_pn, d_pt: slot r of restaurant i at koff[i] R + r K_i + k, the
 * weighted sample of the document's seating (weights w_r).  d_info: NULL, or five uint64 added to: skipped restaurants,
 * impossible visits, stuck visits, dead restaurants, resamplings.  sum_i H_i is stb_seat_loglik(d_Hi, I, 1, ...) as it
 * stands (one particle: H = m exactly).  No wait: the call returns when the launch is queued.
 * The slots' states live in LDS twice over (a resampling copies from one buffer to the other): stb_seat_filter_budget(K)
 * is the largest R the kernel takes for a restaurant of K dishes, min(64, 61440 / (12 K')) with K' = K rounded up to
 * even -- 64 for K <= 80, 39 for K = 130, 5 for K = 1024 (a workgroup takes 64 KB at most).  A restaurant whose (K_i, R) is
 * over it, or K_i > STB_TD_MAXK, K_i > stride (with a matrix), or K_i = 0 with customers, is left out: H_i = 0, counted in
 * skipped, nothing else of it written.  Refused before anything is queued, with stb_last_error() set: what
 * stb_seat_customers refuses of these arguments, particles = 0 or > 64, tau outside [0, 1] or NaN, a null d_Hi.
 *
 * stb_tindic_heldout_pf is stb_tindic_heldout_seq's twin: the held-out customers seated on a private copy of every
 * restaurant's current state by the filter; writes nothing of the object; refused as _heldout_seq is. */
#define STB_PF_MAXR 64
typedef struct stb_pf_info { uint64_t skipped, impossible, stuck, dead, resamplings, customers; } stb_pf_info_t;
int stb_seat_filter(double a, const double *d_bpar, int I, const uint64_t *d_koff, const uint32_t *d_n, const uint16_t *d_t,
                    const double *d_h /* NULL: 1 */, unsigned M, const uint64_t *d_coff, const uint32_t *d_cls,
                    const double *d_lik /* NULL: 1 */, unsigned rows, unsigned stride, unsigned particles, double tau,
                    uint64_t seed, uint64_t sweep, double *d_Hi /* I */, double *d_w /* NULL, or I x particles */,
                    int64_t *d_E /* NULL, or I */, uint32_t *d_res /* NULL, or I */, uint32_t *d_pn, uint16_t *d_pt /* NULL, or
                    koff[I] x particles each */, uint64_t *d_info /* NULL or 5 uint64 added to */, void *stream);
unsigned stb_seat_filter_budget(unsigned K);
int stb_tindic_heldout_pf(stb_tindic_t *s, double a, const double *bpar, unsigned particles, double tau, uint64_t seed,
                          uint64_t sweep, double *total, double *Hi_host /* or NULL */, stb_pf_info_t *info /* or NULL */);

/* ---- annealed importance sampling for unseen documents (seat_ais.hip) ----
 * Both estimators above buy accuracy with particles.  This one buys it with temperatures: a particle starts as a draw
 * from the prior and is moved, by dish sweeps, through laws that lean on the likelihood more and more.  Restaurant i
 * starts EMPTY; its N_i customers have classes cls_c; the ladder is 0 = beta_0 < beta_1 < ... < beta_S = 1 and
 *     f_s(z, t) = P(z, t | a, b, h, M) prod_c L[cls_c][z_c]^beta_s,
 * so f_0 is the prior (Z_0 = 1: stb_seat_customers' statement with L = 1, with or without a truncation M) and
 * Z_S = p(w_1 .. w_N | L, h, a, b).  Per particle:
 *   1. x_0 ~ prior: stb_seat_customers without a matrix, one committed particle; lw starts at that seating's own log
 *      weight.  Without a truncation that is 0 up to rounding (every sum of theta is 1).  With a truncation M the sums
 *      fall short of 1 and the seating is a WEIGHTED draw from the prior over the states with t <= M -- its statement
 *      above -- and the weight is what makes Z_S the truncated p(w), the quantity _heldout_seq estimates.
 *   2. for s = 1 .. S:  lw += (beta_s - beta_{s-1}) * D(x_{s-1}),  D(x) = sum_c log L[cls_c][z_c];
 *   3. if s < S, AFTER the increment:  x_s = `passes` dish sweeps (stb_sample_tdishes) of x_{s-1} under the matrix L^beta_s.
 * The dish sweep leaves prior x prod_c L'[cls_c][z_c] invariant for any matrix L' >= 0, L^beta_s included, so
 * E[exp lw] = Z_S for every S, every ladder and every number of passes, and H_i = log((1/R) sum_r exp lw_r) is
 * stb_seat_loglik's, unchanged.  The order is part of the law: the increment is taken on the state BEFORE the sweep, and
 * the sweep runs under the NEW temperature (DESIGN.md section 6 has the two wrong orders' numbers).  S = 1 has no sweep:
 * importance sampling from the prior.  Only empty starts: the dish sweep's removal treats every customer of a pair as
 * exchangeable, so moving only the held-out customers of a restaurant that holds training customers too could take t
 * below the training seating's -- not the conditional given that seating.
 *
 * stb_seat_anneal queues, on one stream and with no wait, the existing kernels on a replicated problem of I R restaurants
 * and R C customers: replica j = i R + r has its pairs at koff'[j] = koff[i] R + r K_i (stb_seat_filter's d_pn layout), its
 * customers at coff'[j] = coff[i] R + r N_i, the classes, h and b of restaurant i, and n' = t' = 0 (k_ais_expand; all
 * offsets uint64).  Then stb_seat_customers(particles = 1, STB_SEAT_COMMIT, no matrix, sweep number `sweep`) on the
 * replicas, and per temperature s: the matrix lik^beta_s if s < S (k_ais_temper), the increment (k_ais_weight), and if
 * s < S `passes` dish sweeps numbered sweep + 1 + (s-1) passes .. under that matrix.  Every uniform is therefore the one
 * the two contracts above name, on the replicated problem: C' = R C, c the replica's flat customer index.  One M, the
 * V table's, goes to the seating and to the sweeps.
 *   stb_lik_temper (k_ais_temper): out = 0 where lik = 0, elsewhere exp(beta * log(lik)) -- a log, one product, an exp, in
 *     FP64 with no contraction, a cell a thread.  Public so that a replay can fetch exactly the matrix the sweeps read:
 *     a matrix per temperature is materialised (one streaming pass) so that no bit of the path depends on an exp the
 *     host cannot reproduce.
 *   D (k_ais_weight): a wave a replica.  Customer q of the replica (q = 0 .. N_i - 1) belongs to lane q mod 64; a lane
 *     adds its x_q = log(lik[cls'_q stride + cust'_q]) in increasing q in double-double (dd_add: t = hi + x; if t is
 *     finite, bb = t - hi and lo += (hi - (t - bb)) + (x - bb); hi = t -- k_seat's lw); the lanes 0 .. min(64, N_i) - 1
 *     are then added in lane order into one double-double (the lane's hi by dd_add, its lo added to lo), and
 *     D = hi + lo.  log 0 = -inf; a class >= rows counts as L = 0, as the dish sweep reads it.  Then
 *     lw = lw + dbeta * D (one product, one sum), dbeta = beta_s - beta_{s-1} taken once on the host in FP64.  beta
 *     strictly increasing keeps 0 * inf out; a particle at -inf stays there and counts as dead.  The bits of lw depend on
 *     the replica's customers alone: not on the waves of a workgroup (STB_AIS_WAVES = 1, 2, 4 or 8; default 4), the grid,
 *     or who shares the launch.
 * Arguments: the V slab and its bounds (N, M) for discount a; a, d_bpar, I, d_koff, d_h (or NULL: 1), d_coff, d_cls,
 * d_lik, rows, stride; G = koff[I] and C = coff[I] as the caller states them (the workspace is sized from them: they are
 * checked on the device, and a disagreement leaves every restaurant out and counts all I as skipped); particles (1 ..
 * 4096); S >= 1; betas_host (S values) or NULL for beta_s = (double)s / (double)S, beta_S = 1.0; passes >= 1; seed, sweep.
 * Outputs: d_lw[I x particles], to be finished by stb_seat_loglik; optional final states d_pn, d_pt (G x particles) and
 * d_pcust (C x particles) in the replicated layout, the weighted posterior sample; d_info: NULL, or three uint64 added
 * to: skipped restaurants, dead particles (lw = -inf at the end), stuck visits of the seating and the sweeps.  A restaurant
 * that one of the kernels would skip -- K_i > STB_TD_MAXK, K_i > stride, K_i = 0 with customers, N_i > the table's N -- is
 * left out whole: lw = 0 for every r, H_i = 0, counted once in skipped; its replicas keep their places in the layout (so
 * the others' streams do not move) and their final states mean nothing.  d_ws: stb_seat_anneal_workspace_bytes(I, G, C,
 * particles, rows, stride) bytes of device memory, the call's own until the stream has run it.  No chunking inside the
 * call -- the streams depend on C' -- so a caller short of memory splits its restaurants.  Refused before anything is
 * queued, with stb_last_error() set: what stb_sample_tdishes and stb_seat_customers refuse of these arguments; S = 0 or
 * passes = 0; betas not strictly increasing inside (0, 1] or not ending at exactly 1.0; a null matrix or null classes; a
 * workspace that is null or too small; I x particles beyond an int.
 *
 * stb_tindic_heldout_ais is the twin of _heldout_seq and _heldout_pf over the customers of stb_tindic_set_heldout, for an
 * object that holds NO customers of its own (otherwise refused, for the reason above) and has a matrix.  It keeps a V
 * table of its own for this call, at N = max(3, max_i held-out N_i) and M as given at create, refilled only when a or the
 * bounds change and checked with stb_fill_status as _sweep does.  It writes nothing of the object's state or
 * accumulator.  info: skipped, dead, stuck as above, customers = hoff[I]. */
typedef struct stb_ais_info { uint64_t skipped, dead, stuck, customers; } stb_ais_info_t;
size_t stb_seat_anneal_workspace_bytes(int I, uint64_t G, uint64_t C, unsigned particles, unsigned rows, unsigned stride);
int stb_lik_temper(const double *d_lik, unsigned rows, unsigned stride, double beta, double *d_out, void *stream);
int stb_seat_anneal(const double *d_vtable, unsigned N, unsigned M, double a, const double *d_bpar, int I,
                    const uint64_t *d_koff /* I+1 */, const double *d_h /* NULL: 1 */, const uint64_t *d_coff /* I+1 */,
                    const uint32_t *d_cls, const double *d_lik, unsigned rows, unsigned stride, uint64_t G, uint64_t C,
                    unsigned particles, unsigned S, const double *betas_host /* S, or NULL */, unsigned passes, uint64_t seed,
                    uint64_t sweep, double *d_lw /* I x particles */, uint32_t *d_pn, uint16_t *d_pt /* NULL, or G x
                    particles each */, uint32_t *d_pcust /* NULL, or C x particles */, uint64_t *d_info /* NULL or 3 uint64
                    added to */, void *d_ws, size_t ws_bytes, void *stream);
int stb_tindic_heldout_ais(stb_tindic_t *s, double a, const double *bpar, unsigned particles, unsigned S,
                           const double *betas /* S, or NULL */, unsigned passes, uint64_t seed, uint64_t sweep,
                           double *total, double *Hi_host /* or NULL */, stb_ais_info_t *info /* or NULL */);

/* ---- customers' classes drawn on the device: generated and missing data (classgen.hip; additive) ----
 * The one variable of DESIGN.md section 6's joint that the steps above take from the caller: customer c's class given
 * its dish, cls_c ~ lik[.][z_c] / Z_{z_c}.  With it the object generates from its own model (stb_tindic_generate), and
 * missing classes are part of the chain: alternated with the dish sweep, the draw is Gibbs sampling on the joint with
 * the missing classes included.
 *
 * lik is rows x stride doubles, row-major, finite and >= 0; dish k is local pair k (the dish sweep's and
 * stb_sample_lik's convention), so column k is dish k's class weights; k = cust[c] is customer c's dish.
 *
 * Cumulative sums of column k, in stb_sample_lik's chunk association (FP64, no contraction): rows in chunks of 256
 * (chunk j = rows 256 j .. 256 j + 255); pre_w the running sum inside a chunk in row order, starting from the chunk's
 * first row; S_j = pre at the chunk's last row; base_0 = 0, base_1 = S_0, base_{j+1} = base_j + S_j; cum_w = pre_w in
 * chunk 0, else base_j + pre_w; Z_k = the last base, bit for bit the Z_k of stb_sample_lik on the same cells.  cum is
 * non-decreasing, and cum_w > cum_{w-1} implies lik_wk > 0.
 *
 * The draw: u = element 3C + 1 + c of the stream of (seed, sweep), key = mix(seed + (sweep+1) gamma) as the sweeps'; C
 * the call's number of customers, c the flat customer index.  (Elements 2c+1, 2c+2 and 2C+1+c are u1, u2/u4 and u3 of the
 * sweeps and the seating: this one is free, so one (seed, sweep) serves a seating and a class draw together.)
 * thr = u * Z_k; w* = the smallest w with cum_w > thr; if there is none, the smallest w with cum_w >= Z_k (the last row
 * at which the sum grew).  For u < 1, fl(u Z) < Z holds for every Z > 2^-1022, so the second form is reachable only for
 * columns whose total is at most 2^-1022 (there u Z can round to Z itself: DESIGN.md section 6); it keeps the rule total
 * there, as the dish choice's is.  cls[c] = w*: never a class of zero weight.  The rule is a binary search over the chunk
 * bases, then inside the chunk.
 *
 * Left alone, and counted (d_info: NULL, or three uint64 added to -- skipped, stuck, drawn):
 *   cust[c] >= stride             the class stays; skipped
 *   Z_k not positive and finite   the class stays; stuck
 *   mask[c] == 0 (uint8 per customer; NULL: all are drawn)    the class stays; nothing is counted
 *   otherwise                     drawn
 * A class depends on (seed, sweep, c, C), the customer's dish and the matrix alone: not on launch geometry, on the waves
 * of a workgroup (STB_CLS_WAVES = 1, 2, 4 or 8), or on who shares the call.
 *
 * stb_sample_classes      the raw call on device arrays.  It takes a rows x stride scratch (pre) from the buffer cache
 *                         and fails before anything is written if there is none; it waits once, to give the scratch back.
 *                         Refused before anything is queued: a null d_lik, a null d_cust or d_cls with C > 0, rows or
 *                         stride 0.
 * stb_tindic_sample_classes   the object's classes drawn from its matrix (which must not be one a failed
 *                         stb_tindic_sample_lik left), queued on the object's stream behind its sweeps.  mask_host: C
 *                         bytes or NULL.  The customer sequence is written out if the object still has pair order.  An
 *                         object without classes gets them (mask must then be NULL: refused otherwise).  Afterwards the
 *                         classes' rows are the matrix's, so _class_counts, _sample_lik and _loglik work on the result.
 *                         Writes only the classes: not n, t, T, cust, h, the matrix or the held-out accumulator.  info
 *                         NULL and no mask: no wait (a mask travels through the buffer cache, which is given back behind
 *                         a wait).  The object keeps the scratch until its matrix changes shape or it is freed.
 * stb_tindic_generate     a draw of (z, t, cls) from the model given (lik, h, a, b): all C customers seated from empty
 *                         restaurants under the prior (stb_tindic_seat's launch with no matrix, whatever the object
 *                         holds), then every class drawn.  Bit-equal to: remove the matrix, stb_tindic_seat, put the
 *                         matrix back, stb_tindic_sample_classes with the same (seed, sweep).  Refuses what
 *                         stb_tindic_seat refuses, an object with no matrix, and what _sample_classes refuses.
 *                         seat_info: stb_tindic_seat's counters (customers = C); no total is computed.  Waits.
 * stb_tindic_get_classes  the classes (C values) and their rows, after the queued work.
 * Every refusal leaves the state as it was, with stb_last_error() set. */
typedef struct stb_classes_info { uint64_t skipped, stuck, drawn; } stb_classes_info_t;
int stb_sample_classes(const double *d_lik, unsigned rows, unsigned stride, const uint32_t *d_cust,
                       const uint8_t *d_mask /* or NULL */, uint64_t C, uint64_t seed, uint64_t sweep,
                       uint32_t *d_cls, uint64_t *d_info /* NULL or 3 uint64 added to */, void *stream);
int stb_tindic_sample_classes(stb_tindic_t *s, const uint8_t *mask_host /* C, or NULL */, uint64_t seed,
                              uint64_t sweep, stb_classes_info_t *info /* or NULL: no wait */);
int stb_tindic_generate(stb_tindic_t *s, double a, const double *bpar, uint64_t seed, uint64_t sweep,
                        stb_seat_info_t *seat_info /* or NULL */, stb_classes_info_t *cls_info /* or NULL */);
int stb_tindic_get_classes(stb_tindic_t *s, uint32_t *cls_out /* C */, unsigned *rows_out /* or NULL */);

/* ---- Gaussian observations: a PYP mixture of Gaussians on the device (gauss.hip; additive) ----
 * Every likelihood step above takes a customer's observation to be a class index.  Here customer c (flat index, as for
 * cls) carries x_c in R^D, 1 <= D <= STB_GS_MAXD, and dish k (local pair k of every restaurant, stb_tindic_sample_h's
 * convention; k < K <= STB_TD_MAXK) has a mean mu_k in R^D and a diagonal precision tau_k in R^D_+:
 *     x_cd | z_c = k ~ N(mu_kd, 1 / tau_kd), independent over d;
 *     tau_kd ~ Gamma(alpha0, rate beta0_d),  mu_kd | tau_kd ~ N(m0_d, 1 / (kappa0 tau_kd)), independent over (k, d).
 * Given the n customers of dish k, their mean xbar and centred sum of squares Q, the posterior is Normal-Gamma with
 *     kappa_n = kappa0 + n,  m_n = (kappa0 m0 + n xbar) / kappa_n,  alpha_n = alpha0 + n / 2,
 *     beta_n = beta0 + Q / 2 + kappa0 n (xbar - m0)^2 / (2 kappa_n).
 * The dish sweep needs no change: k_tdish reads L_k = lik[cls[c] * stride + k], it is exact because the matrix is a fixed
 * table while it runs, and multiplying a row by a positive constant changes no choice.  With one row per customer
 * (cls[c] = c, rows = C) a matrix of Gaussian densities makes the dish sweep the assignment step of the mixture, and
 * alternating it with the redraw of (mu, tau) is Gibbs sampling on (seating, mu, tau).  The matrix
 * takes 8 C stride bytes.
 *
 * Everything is FP64 without contraction; x is C x D, mu, tau, mean and Q are K x D, all row-major; no bit depends on
 * launch geometry (STB_GAUSS_WAVES = 1, 2, 4 or 8 waves a workgroup).  tests/gs_oracle.py replays every operation below.
 *
 * Sums over the customers of a dish (S and Q, nothing else): customers in chunks of 256 by flat index (chunk j =
 * customers 256 j .. 256 j + 255); inside a chunk the members of dish k are added one after another in customer order,
 * starting from the chunk's first member; non-members add nothing and a chunk without members is skipped; the chunk
 * partials are combined in chunk order in double-double (TwoSum on the high word, the error into the low: dd_add,
 * libstb_amd/csrc/stb_common.h, as stb_dirmult_logml's chunk sums) starting from (0, 0); the result is hi + lo.
 * stb_gauss_stats, two passes: A -- n_k as an integer count, S_kd = sum x_cd, mean_kd = S_kd / (double)n_k; B --
 * Q_kd = sum (x_cd - mean_kd) * (x_cd - mean_kd).  n_k = 0: mean and Q are +0.0.  A customer with cust[c] >= K counts in
 * info.skipped and belongs to no dish.  (The one-pass form sum x^2 - n xbar^2 cancels: tests/test_gauss_host.py shows it
 * many bars out where the two passes are inside theirs.)  The outputs need no initialisation.  Scratch from the buffer
 * cache: 8 D K + 4 K bytes per chunk.  Four launches, one wait.
 * stb_sample_gauss: key = mix(seed + (sweep+1) gamma), the constant and mix of stb_sample_lik; cell e = k * D + d owns
 * key_e = mix(key + (e+1) gamma).  With n = (double)n_k, dm = mean - m0_d (m0 NULL: 0.0; beta0 NULL: beta00 for every d):
 *     kappa_n = kappa0 + n;  m_n = (kappa0 * m0_d + n * mean) / kappa_n;  alpha_n = alpha0 + 0.5 * n;
 *     beta_n = (beta0_d + 0.5 * Q) + 0.5 * (((kappa0 * n) / kappa_n) * (dm * dm));
 * n_k = 0: the prior's values, nothing evaluated.  lg = log of a Gamma(alpha_n) variate from key_e by stb_sample_lik's
 * recipe unchanged (gamma_dev.h); lt = lg - log(beta_n); tau = exp(lt); the next two uniforms of the same substream are
 * u1, u2; z = sqrt(-2 log u1) * cos(6.283185307179586 * u2); mu = m_n + z / sqrt(kappa_n * tau).  A rejection loop that
 * runs out, or a tau that is not positive and finite, fails the call after its wait; mu and tau are then undefined.
 * One launch, one wait.
 * stb_gauss_lik: H_k = sum_d 0.5 * log(tau_kd) and q_ck = sum_d ((x_cd - mu_kd) * (x_cd - mu_kd)) * tau_kd, both added one
 * after another in d order starting from the d = 0 term; l_ck = H_k - 0.5 * q_ck; m_c = max over k < K of l_ck;
 * lik[c * stride + k] = exp(l_ck - m_c) for k < K and 0.0 for K <= k < stride (stride >= K): every row holds an exact
 * 1.0.  A row whose m_c is not finite is written as zeros and counted in info.dead; the dish sweep reports its customer as
 * stuck.  Two launches, one wait.
 * stb_gauss_loglik: the data term log p(x | z, mu, tau).  v_c = l_{c, cust[c]}, recomputed as above; a customer with
 * cust[c] >= K adds 0.0 and counts in info.skipped.  Customers 256 b .. 256 b + 255 (0.0 beyond C) are block b, summed by
 * stb_logjoint's block tree: (v[l] + v[l + 64]) + (v[l + 128] + v[l + 192]) per lane l, then v += shfl_down(v, o),
 * o = 32, 16, .. 1; the block sums are added in order in double-double, and the total is
 * (hi + lo) + (double)(C * D) * (-0.9189385332046727).  C = 0 gives that constant's 0.  -inf or finite, never a NaN, for
 * finite x, mu and positive finite tau.  The answer arrives through pinned memory: two launches, one wait.
 * stb_gauss_logml: the collapsed evidence log p(x | z), mu and tau summed out.  Cell e = k * D + d with n_k > 0 is
 *     lgamma(alpha_n) - lgamma(alpha0) + alpha0 * log(beta0_d) - alpha_n * log(beta_n)
 *         + 0.5 * (log(kappa0) - log(kappa_n)) - (0.5 * n) * 1.8378770664093453
 * evaluated left to right (the posterior's values as in the draw); a cell with n_k = 0 is exactly 0.0.  The K * D cells
 * are summed in blocks of 256 by the same tree and the block sums in order in double-double: hi + lo.  One launch, one
 * wait.
 * Refused before anything is queued, with stb_last_error() set: a null array that would be read or written, D outside
 * 1 .. STB_GS_MAXD, K outside 1 .. STB_TD_MAXK, stride < K, for stb_gauss_stats C above 2^32 - 1 (n_k is a uint32); a prior whose kappa0, alpha0 or a beta0 is not positive and
 * finite, or with an m0 that is not finite.  info may be NULL; the member a call does not count is 0. */
#define STB_GS_MAXD 64
typedef struct stb_gauss_prior {
  double kappa0, alpha0, beta00;
  const double *m0;    /* host, D, NULL: 0 */
  const double *beta0; /* host, D, NULL: beta00 */
} stb_gauss_prior_t;
typedef struct stb_gauss_info { uint64_t skipped, dead; } stb_gauss_info_t;
int stb_gauss_stats(const double *d_x, unsigned D, const uint32_t *d_cust, uint64_t C, unsigned K, uint32_t *d_n,
                    double *d_mean, double *d_Q, stb_gauss_info_t *info /* or NULL */, void *stream);
int stb_sample_gauss(const uint32_t *d_n, const double *d_mean, const double *d_Q, unsigned K, unsigned D,
                     const stb_gauss_prior_t *prior, uint64_t seed, uint64_t sweep, double *d_mu, double *d_tau, void *stream);
int stb_gauss_lik(const double *d_x, unsigned D, uint64_t C, const double *d_mu, const double *d_tau, unsigned K,
                  double *d_lik, unsigned stride, stb_gauss_info_t *info /* or NULL */, void *stream);
int stb_gauss_loglik(const double *d_x, unsigned D, const uint32_t *d_cust, uint64_t C, const double *d_mu,
                     const double *d_tau, unsigned K, double *total_host, stb_gauss_info_t *info /* or NULL */, void *stream);
int stb_gauss_logml(const uint32_t *d_n, const double *d_mean, const double *d_Q, unsigned K, unsigned D,
                    const stb_gauss_prior_t *prior, double *total_host, void *stream);
/* Object layer: an stb_tindic_t in observation mode.  K = the largest K_i, which every restaurant must have; the calls queue
 * on the object's stream behind its sweeps.
 *   stb_tindic_set_obs      x_host is C x D.  Refused: a non-finite x, D outside 1 .. STB_GS_MAXD, K outside 1 .. STB_TD_MAXK,
 *                           restaurants whose K_i are not all equal, no customers.  Puts x on the device, sets the classes to
 *                           the identity with rows = C, makes a C x K matrix of ones (8 C K bytes) and materialises cust as
 *                           the first dish sweep does.  The object is then in observation mode, without parameters.
 *                           stb_tindic_set_obs(s, NULL, 0) removes the observations and leaves the object with neither
 *                           classes nor a matrix.  A later stb_tindic_set_classes or _set_lik by the caller ends the mode too
 *                           (and keeps what the other of the two holds).
 *   stb_tindic_set_gauss    mu and tau from host K x D arrays (mu finite, tau positive and finite), and the matrix rewritten
 *                           from them (stb_gauss_lik).  stb_tindic_get_gauss returns them.
 *   stb_tindic_sample_gauss stb_gauss_stats on (x, cust), stb_sample_gauss, stb_gauss_lik into the object's matrix: the raw
 *                           calls' launches in their order, bit for bit, with one wait; nothing per customer or dish crosses
 *                           to the host, and n, t, T, cust and h are not written.  A draw that fails after its wait leaves
 *                           the parameters and the matrix undefined: dish sweeps (and _get_gauss, _gauss_loglik) are refused
 *                           until a _sample_gauss or _set_gauss that succeeds.
 *   stb_tindic_gauss_loglik the data term under the object's parameters; with stb_tindic_logjoint's total it is the
 *                           complete-data log joint.  stb_tindic_gauss_logml: statistics, then the evidence: the figure to
 *                           watch a chain by (it needs no parameters).
 * In observation mode these work as they stand: stb_tindic_sweep_dishes, _sweep and _seat (they read the matrix row
 * cls[c] = c, and a row's scale changes no choice -- but stb_tindic_seat's total, a log weight, carries every row's own
 * scale and means nothing there: pass NULL); every h, b, a and joint step; stb_tindic_logjoint, _predict (it reads no
 * matrix), _logjoint_collapsed without STB_CJ_DATA; the get_* calls, stb_tindic_lik_device, _set_heldout, _heldout_reset and
 * _heldout_get.  These are refused, the state untouched and stb_last_error() set, because they read rows as classes or
 * depend on a row's scale: stb_tindic_sample_lik, _loglik, _class_counts, _sample_beta, _logjoint_collapsed with
 * STB_CJ_DATA, _sample_classes, _generate, _heldout, _heldout_seq, _heldout_pf, _heldout_ais.  Outside observation mode no
 * call changes in any way. */
int stb_tindic_set_obs(stb_tindic_t *s, const double *x_host /* C x D, or NULL */, unsigned D);
int stb_tindic_set_gauss(stb_tindic_t *s, const double *mu, const double *tau);
int stb_tindic_get_gauss(stb_tindic_t *s, double *mu_out, double *tau_out);
int stb_tindic_sample_gauss(stb_tindic_t *s, const stb_gauss_prior_t *prior, uint64_t seed, uint64_t sweep,
                            stb_gauss_info_t *info /* or NULL */);
int stb_tindic_gauss_loglik(stb_tindic_t *s, double *total);
int stb_tindic_gauss_logml(stb_tindic_t *s, const stb_gauss_prior_t *prior, double *total);

/* ---- Held-out points under Gaussian observations (gauss.hip, predict.hip; additive) ----
 * The Gaussian twin of stb_predict_dishes / stb_heldout_loglik.  Held-out point j (flat index, CSR over hoff[I + 1] as the
 * held-out customers above; y is C_h x D row-major, C_h = hoff[I]) of restaurant i has, under one state,
 *     log p(y_j | state) = log sum_k theta_ik N(y_j | mu_k, 1 / tau_k),
 * computed from x-space quantities with the true normalisation: the row-scaled matrix never enters.  Densities in up to
 * 64 dimensions leave the range of a double, so everything per point is kept as a logarithm, the accumulator over
 * states included.  FP64, no contraction; K is the common K_i; tests/gh_oracle.py replays every operation.
 *   theta_ik   stb_predict_dishes' theta, bit for bit: call it with d_theta, no held-out customers and no matrix.
 *   l_jk       = H_k - 0.5 * q_jk, stb_gauss_lik's values with y_j for x_c (H_k, q_jk added in d order from the d = 0 term).
 *   m_j        = max of l_jk over the k < K with theta_ik > 0 (a NaN is never greater).  m_j not finite: the point is
 *              impossible -- ell_j = -inf, its responsibilities are 0, its accumulator is left alone, and the sum counts
 *              it.  The restriction to theta_ik > 0 guarantees s_j >= theta_ik* > 0 for a possible point: under the plain
 *              maximum a dish with theta = 0 that lies nearest the point can underflow every term.
 *   w_jk       = theta_ik * exp(l_jk - m_j); +0.0 where theta_ik is not > 0 or k >= K.
 *   s_j        the w_jk in blocks of 64 dishes, lane l taking dish 64 b + l, a block by the shuffle tree
 *              v += shfl_down(v, o), o = 32 .. 1, the block sums added in block order: stb_predict_dishes' p_c.
 *   ell_j      = (m_j + log(s_j)) + (double)D * (-0.9189385332046727).
 *   r_jk       = w_jk / s_j into d_resp[j * rstride + k], 0.0 for K <= k < rstride.
 *   (M_j, A_j) with STB_GH_ACCUMULATE, standing for A_j e^{M_j} = sum over the accumulated states of p_j; empty: (-inf, 0.0).
 *              ell_j = -inf leaves the pair alone; ell_j > M_j: A_j = A_j * exp(M_j - ell_j) + 1.0 (1.0 from the empty pair),
 *              then M_j = ell_j; otherwise A_j = A_j + exp(ell_j - M_j).  One lane owns a point: S calls give the bits of
 *              the S updates in call order.
 * stb_gauss_heldout (k_gs_prep, then k_gh_point_reg for K <= 64 and D <= 16, else k_gh_point: a wave a point, lanes along
 * k) queues its two launches and returns; the transposed parameters live in a buffer of the calling thread, so calls of
 * one thread on different streams must not be in flight together.  No bit depends on STB_GAUSS_WAVES or on the grid.
 * stb_gauss_heldout_loglik (k_gh_sum, which shares k_heldout_sum's body): x_j = ell_j (d_accM and d_accA NULL; a value
 * that is not finite is impossible), or x_j = M_j + log(A_j / (double)samples), impossible when A_j / samples is not a
 * positive finite number.  An impossible point adds +0.0, counts in info.impossible and makes H_i and the total -inf.
 * The x_j are summed exactly as stb_heldout_loglik sums its x_c: chunks of 64 in CSR order through the tree, the chunk
 * sums in order in double-double, H_i = hi + lo; over restaurants stb_logjoint's association, geometry and ticket.  One
 * launch, one wait.  No NaN is produced for finite y, finite mu and positive finite tau.
 * Refused before anything is queued, with stb_last_error() set: a null required array, D outside 1 .. STB_GS_MAXD, K
 * outside 1 .. STB_TD_MAXK, tstride < K, rstride < K with d_resp, STB_GH_ACCUMULATE without both accumulator arrays,
 * samples = 0 with accumulators, unknown flag bits, I < 0. */
#define STB_GH_ACCUMULATE 1u
int stb_gauss_heldout(const double *d_theta, unsigned tstride, int I, const uint64_t *d_hoff, const double *d_y, unsigned D,
                      const double *d_mu, const double *d_tau, unsigned K, double *d_ell /* NULL, or C_h */,
                      double *d_resp /* NULL, or C_h x rstride */, unsigned rstride, double *d_accM,
                      double *d_accA /* both with STB_GH_ACCUMULATE, else ignored */, unsigned flags, void *stream);
int stb_gauss_heldout_loglik(const double *d_ell, const double *d_accM, const double *d_accA, unsigned samples,
                             const uint64_t *d_hoff, int I, double *d_Hi /* NULL, or I */, double *total_host,
                             stb_predict_info_t *info /* or NULL */, void *stream);
/* Object layer, in observation mode only.  The observation held-out set is storage of its own: stb_tindic_set_heldout, its
 * classes and its accumulator are untouched, and _heldout, _heldout_seq, _heldout_pf, _heldout_ais stay refused.
 *   stb_tindic_set_heldout_obs     hoff_host[I + 1] and y_host (hoff[I] x D, D as set_obs gave it); NULL offsets remove the
 *                                  set.  An empty accumulator, no samples.  Refused: outside observation mode, hoff[0] != 0
 *                                  or decreasing offsets, a y that is not finite.  Leaving the mode (set_obs(NULL, 0), a
 *                                  caller's set_classes / set_lik) drops the set, and so does a set_obs with another D.
 *   stb_tindic_gauss_heldout       stb_predict_dishes into scratch theta (tstride = K), stb_gauss_heldout (rstride = K),
 *                                  stb_gauss_heldout_loglik: the raw composition bit for bit, queued behind the object's
 *                                  sweeps with one wait; n, t, T, cust, h, mu, tau and the matrix are not written.  Without
 *                                  flags it scores the current state through a scratch ell and leaves the accumulator
 *                                  alone; with STB_GH_ACCUMULATE it updates the accumulator, counts the sample and returns
 *                                  the running estimate sum_j log((1/S) sum_s p_j).  STB_BPAR_RESIDENT, per-group and tree
 *                                  h work as for stb_tindic_predict.  Refused, state and accumulator as they were: no
 *                                  observations, no held-out set, parameters undefined (none yet, or a failed
 *                                  _sample_gauss), h undefined after a failed _sample_h, a / bpar as the sweeps refuse them.
 *   stb_tindic_gauss_heldout_reset an empty accumulator and no samples; _gauss_heldout_get returns the pairs and the count. */
int stb_tindic_set_heldout_obs(stb_tindic_t *s, const uint64_t *hoff_host /* I+1, or NULL */, const double *y_host /* hoff[I] x D */);
int stb_tindic_gauss_heldout(stb_tindic_t *s, double a, const double *bpar, unsigned flags, double *total,
                             double *Hi_host /* or NULL */, double *resp_host /* NULL, or hoff[I] x K */,
                             stb_predict_info_t *info /* or NULL */);
int stb_tindic_gauss_heldout_reset(stb_tindic_t *s);
int stb_tindic_gauss_heldout_get(stb_tindic_t *s, double *M_out, double *A_out, unsigned *samples); /* each or NULL */

/* ---- aterms2, the S-free discount posterior of samplea2 (lib/samplea.c:85-150) ----
 * For a sampled partition of the customers into tables the posterior needs only how many tables have
 * each size: cnt[s] = number of tables with s customers (s = 2 .. S-1; entries 0 and 1 are ignored),
 * plus the per-restaurant T[I], bpar[I] of aterms.  out[d] = sum_i restaurant terms(x_d)
 * + sum_s cnt[s] * log((1-x_d)(2-x_d)...(s-1-x_d)), evaluated as lib/lgamma.c:36-52 does. */
typedef struct stb_hist stb_hist_t;
stb_hist_t *stb_hist_create(const uint32_t *cnt, unsigned S, int I, const uint32_t *T, const double *bpar);
int stb_hist_aterms2(stb_hist_t *h, const double *x_host, int D, double *out_host);
void stb_hist_free(stb_hist_t *h);
/* A histogram the device fills (stb_sample_partition, stb_tcounts_partition):
 *   stb_hist_create_empty   S sizes, I restaurants on the current device; counts 0, T 0, bpar 1
 *   stb_hist_restaurants    T[I], bpar[I] from the host, after the histogram's queued work
 *   stb_hist_counts_device  its device counts cnt[S] and its stream (hipStream_t as void*): work that writes the counts
 *                           is queued there (or ordered before the histogram's next call by the caller)
 *   stb_hist_get            waits for its stream, then cnt[S] to the host
 * stb_hist_aterms2 on a histogram the device filled returns what stb_hist_create returns on the same counts, T and bpar
 * uploaded from the host: the same buffers, the same kernels. */
stb_hist_t *stb_hist_create_empty(unsigned S, int I);
int stb_hist_restaurants(stb_hist_t *h, const uint32_t *T, const double *bpar);
uint32_t *stb_hist_counts_device(stb_hist_t *h, unsigned *S, void **stream);
int stb_hist_get(stb_hist_t *h, uint32_t *cnt_out);

/* ---- table-size partitions: stage 1 of the S-free discount step, on the device (partition.hip) ----
 * For every pair (n, t), how the n customers split over the t tables, drawn exactly: in rounds r = 0 .. t-2, with M = t-1-r
 * tables to open after this one and N customers unplaced, the next table's size l = 1 .. N-M with probability
 *     C(N-1, l-1) (1-a)_{l-1} S^{N-l}_M / S^N_{M+1}
 * (S with stb_lookup_S's semantics); the last table takes the N left.  Each round draws the smallest l whose cumulative
 * weight exceeds u W (W the round's total, the arithmetic written out in partition.hip's header) with a fresh uniform:
 * key = mix(seed + (sweep+1) gamma), u = element g 65536 + r + 1 of that stream (splitmix64, libstb_amd/synth.py) --
 * the draws depend on (seed, sweep, g, r) alone.  STB_PT_REF_WALK draws with lib/samplea.c:295-320's walk instead (the
 * drop-in samplea2's, one uniform a pair, r = 0's; it does not sample this law: DESIGN.md section 6, deviation 12).
 * The counts: cnt[s], s = 2 .. S-1, tables of s customers (stb_hist's layout); cnt[1] singleton tables (aterms2 ignores
 * them); cnt[0] pairs left out.  n = 0 and t = n count nothing; t = 1 counts one table of n (reading no table); left out:
 * t = 0, t > n, n >= S, and 1 < t < n with n > N or t > M.  cnt is zeroed and filled on `stream`.  d_sizes / d_soff
 * (both or neither; d_soff G+1 offsets): pair g's t sizes in draw order at d_sizes + d_soff[g], the remainder last
 * (t = 1: n; t = n: n ones), when its slot holds at least t entries; pairs left out get none.
 * Raw layer: d_table / d_S1 one slab of stb_fill_S for `a` with bounds (N, M) (not read, and may be NULL, when no pair
 * has 1 < t < n).  Object layer: stb_tcounts_partition on the object's pairs, table (refilled when a changes) and
 * stream, queued behind its sweeps; fills h's counts, copies T (device to device) and bpar (host [I]) to h; nothing comes
 * back to the host, and h's later calls wait for it.  Refused, with the state as it was: a outside [0, 1), bad bpar (as
 * stb_tcounts_sweep), a histogram on another device, with another I, or with S <= the largest n, and pairs holding 2^32
 * or more customers. */
#define STB_PT_REF_WALK 1u
int stb_sample_partition(const double *d_table, const double *d_S1, unsigned N, unsigned M, double a, uint64_t G,
                         const uint32_t *d_n, const uint16_t *d_t, uint32_t *d_cnt, unsigned S,
                         uint16_t *d_sizes, const uint64_t *d_soff /* both NULL: histogram only */, unsigned flags,
                         uint64_t seed, uint64_t sweep, void *stream);
int stb_tcounts_partition(stb_tcounts_t *s, double a, stb_hist_t *h, const double *bpar /* host [I] */, uint64_t seed,
                          uint64_t sweep);
/* stage 2 on a histogram: samplea2's bracket around a and its ARMS or slice draw (STB_SAMPLER as for samplea2) from
 * aterms2 on h, with the caller's rng (an rngp_t, include/srng.h); the drop-in samplea2 runs this same code.  h must
 * hold the partition drawn at `a`, and its T and bpar. */
double stb_samplea2_hist(double a, stb_hist_t *h, void *rng, int loops, int verbose);
/* the table sizes the most recent samplea2() sampled, in the reference's layout (ALData.m,
 * lib/samplea.c:283-320): returns the number of entries and, through m, the array (uint16) */
size_t stb_samplea2_partition(const uint16_t **m);

/* ---- diagnostics of the host samplers (include/psample.h) ----
 * the log-posterior evaluations of the most recent samplea()/sampleb() call on this process:
 * how many, ARMS' return code (ignored by the samplers themselves, as in the reference), and the
 * i-th (abscissa, value) pair */
/* samplea() keeps, per calling thread, ONE group set as a container (device buffers, pinned staging, stream, count
 * slab) and hands every call's pairs over into it (stb_groups_pairs_*): a call of the same shape allocates nothing.
 * The pairs themselves are NOT assumed to be the last call's: that reuse is opt-in (STB_SAMPLEA_CACHE=1 skips the
 * hand-over when a 128-bit fingerprint of K, n, t and the shapes equals the last call's; INTEGRATION.md section 7 has the
 * failure mode).  This call frees the calling thread's kept set and its device memory. */
void stb_sampler_cache_clear(void);
int stb_sampler_trace_count(void);
int stb_sampler_trace_code(void);
int stb_sampler_trace_get(int i, double *x, double *y);
/* entry i of the ziggurat tables the Gaussian generator rebuilt (which: 0 heights, 1 widths,
 * 2 integer thresholds); for tests */
double stb_zig_table(int which, int i);

#ifdef __cplusplus
}
#endif
#endif
