/*
 * sampleb.c -- one MCMC step for the Pitman-Yor concentration b (include/psample.h).
 *
 * Host control flow as the reference's lib/sampleb.c:79-159: auxiliary q_i ~ Beta(b, N_i) give
 * Q = 1/scale - sum log q_i; for a == 0 the conditional is a Gamma (drawn directly, or through its
 * Gaussian limit above 400); otherwise b is drawn with ARMS (or the slice sampler) from the
 * log-posterior `bterms` (lib/sampleb.c:33-41).  The Beta/Gamma/Gaussian draws stay on the host:
 * they consume glibc's global rand48 stream one after another.
 *
 * Every evaluation of bterms -- the sum over restaurants of lgamma(T_i + x/a) - lgamma(x/a) --
 * runs on the GPU over a device-resident copy of T[] (stb_bterms); there is no host evaluation.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/psample.h"
#include "../../include/stb_hip.h"
#include "sampler_trace.h"
#include "hyperq.h"
#include "hyperb.h"
#include "hyperj.h"
#include "logjoint.h"
#include "predict.h"
#include "seat.h"

#define NPRE 3 /* abscissae ARMS is known to ask for first (lib/arms.c:117-119) */

typedef struct {
  double shape, Q, apar;
  stb_bctx_t *dev; /* T[] resident in HBM; an evaluation is two launches and one wait */
  /* values evaluated ahead of time, served when ARMS asks for exactly these abscissae */
  int npre;
  double xpre[NPRE], ypre[NPRE];
  /* the device b step (stb_sampleb_device) never exits: a failed evaluation is remembered and the call returns NaN */
  int noexit, failed;
} b_posterior;

static double bterms(double x, void *vp) {
  b_posterior *bp = vp;
  double val;
  int i;
  for (i = 0; i < bp->npre; i++)
    if (x == bp->xpre[i]) {
      stb_trace_add(x, bp->ypre[i]);
      return bp->ypre[i];
    }
  if (bp->failed) return 0.0;
  if (stb_bterms_eval(bp->dev, &x, 1, bp->Q, bp->shape, bp->apar, &val)) {
    if (bp->noexit) {
      bp->failed = 1;
      return 0.0;
    }
    fprintf(stderr, "bterms(): device evaluation failed: %s\n", stb_last_error());
    exit(1);
  }
  stb_trace_add(x, val);
  return val;
}

static _Thread_local stb_bctx_t *kept_b; /* one per calling thread, like samplea's kept pairs */

static _Thread_local stb_bctx_t *kept_bdev; /* ... and the one that borrows a device-resident T (stb_sampleb_device) */
static _Thread_local double last_Q;

void stb_sampleb_cache_clear(void) {
  if (kept_b) stb_bterms_free(kept_b);
  kept_b = NULL;
  if (kept_bdev) stb_bterms_free(kept_bdev);
  kept_bdev = NULL;
  stb_hq_release();
  stb_hb_release();
  stb_hj_release();
  stb_lj_release();
  stb_pr_release();
  stb_gh_release();
  stb_seat_release();
}

static int use_slice(void) {
  const char *s = getenv("STB_SAMPLER");
#ifdef PSAMPLE_ARS
  return s && strcmp(s, "slice") == 0;
#else
  return !(s && strcmp(s, "ars") == 0);
#endif
}

/* lib/sampleb.c:51-68: a few fixed-point steps towards the mode, used only to start the slice
 * sampler.  The reference needs digammaInv() for it, which its default build compiles out
 * (lib/digamma.h:25); here the start point is simply the current value. */

/* lib/sampleb.c:101-118: b | q ~ Gamma(shape + sum T, 1/Q), Tsum = shape + sum T */
static double draw_b_gamma(double Tsum, double Q, rngp_t rng, int verbose) {
  double myb;
  if (Tsum > 400) {
    do {
      myb = Tsum + rng_gaussian(rng, 1) * sqrt(Tsum);
    } while (myb <= 0);
  } else
    myb = rng_gamma(rng, Tsum);
  myb /= Q;
  if (myb < B_MIN) myb = B_MIN;
  if (myb > B_MAX) myb = B_MAX;
  if (verbose > 1) fprintf(stderr, "Sample b ~ gamma(%lg,%lg) = %lf\n", Tsum, Q, myb);
  return myb;
}

/* lib/sampleb.c:120-157: ARMS or the slice sampler on bterms, given Q, shape, apar and the device context in bp.  With
 * bp->noexit a failure returns NaN with stb_last_error() set; otherwise it ends the process, as the reference does. */
static double draw_b_posterior(double b_in, b_posterior *bp, rngp_t rng, int loops, int verbose) {
  double initb[3] = {B_MIN, 1, B_MAX};
  double myb;
  int i;
  bp->npre = 0;
  stb_trace_reset();
  if (!use_slice()) {
    int code;
    /* lib/sampleb.c:127-139 */
    initb[1] = b_in;
    if (fabs(initb[1] - B_MAX) / B_MAX < 0.00001) initb[1] = B_MAX * 0.999 + B_MIN * 0.001;
    if (fabs(initb[1] - B_MIN) / B_MIN < 0.00001) initb[1] = B_MIN * 0.999 + B_MAX * 0.001;
    {
      /* ARMS starts from three abscissae it fixes before any evaluation (lib/arms.c:117-119, the same
       * expression here, so the same bits): evaluate them in ONE device call */
      double x3[NPRE], y3[NPRE];
      for (i = 0; i < NPRE; i++) x3[i] = initb[0] + (i + 1.0) * (initb[2] - initb[0]) / (NPRE + 1.0);
      if (stb_bterms_eval(bp->dev, x3, NPRE, bp->Q, bp->shape, bp->apar, y3)) {
        if (bp->noexit) return NAN;
        fprintf(stderr, "bterms(): device evaluation failed: %s\n", stb_last_error());
        exit(1);
      }
      for (i = 0; i < NPRE; i++) {
        bp->xpre[i] = x3[i];
        bp->ypre[i] = y3[i];
      }
      bp->npre = NPRE;
    }
    code = arms_simple(3, initb, initb + 2, bterms, bp, 0, initb + 1, &myb);
    stb_trace_code(code);
    if (bp->failed) return NAN;
    if (myb < B_MIN || myb > B_MAX) {
      if (bp->noexit) {
        stb_fail_msg("stb_sampleb_device: arms_simple returned a value out of bounds");
        return NAN;
      }
      fprintf(stderr, "Arms_simple(bpar) returned value out of bounds\n");
      exit(1);
    }
  } else {
    /* lib/sampleb.c:141-153 */
    myb = b_in;
    if (verbose > 1) fprintf(stderr, "Max b (%lg,%lg) -> %lg\n", b_in, bp->Q, myb);
    initb[1] = B_MAX;
    if (SliceSimple(&myb, bterms, initb, rng, loops, bp)) {
      if (bp->noexit) {
        if (!bp->failed) stb_fail_msg("stb_sampleb_device: SliceSimple error");
        return NAN;
      }
      fprintf(stderr, "SliceSimple error\n");
      exit(1);
    }
    if (bp->failed) return NAN;
  }
  if (verbose > 1) fprintf(stderr, "Sample b ~ G(%lg) = %lf\n", bp->Q, myb);
  return myb;
}

double sampleb(double b_in, int I, double shape, double scale, scnt_int *N, scnt_int *T, double apar,
               rngp_t rng, int loops, int verbose) {
  double Q, q;
  int i;
  if (scale <= 0) {
    fprintf(stderr, "Illegal scale in sampleb()\n"); /* lib/sampleb.c:86-89 */
    exit(1);
  }
  Q = 1.0 / scale;
  for (i = 0; i < I; i++) {
    if (N[i] <= 0) continue;
    q = rng_beta(rng, b_in, (int)N[i]); /* lib/sampleb.c:94 */
    if (q <= 0) {
      fprintf(stderr, "Illegal q in sampleb(b=%lf)\n", b_in);
      exit(1);
    }
    Q -= log(q);
  }
  if (apar == 0) {
    double Tsum = shape;
    for (i = 0; i < I; i++) Tsum += T[i];
    return draw_b_gamma(Tsum, Q, rng, verbose);
  }
  {
    b_posterior bp;
    memset(&bp, 0, sizeof(bp));
    bp.Q = Q;
    bp.apar = apar;
    bp.shape = shape;
    /* the device context of the previous call on this thread, when it is large enough: T[] is copied anew (it changes
     * from call to call), the stream, the pinned result buffer and the device memory are kept */
    if (kept_b && stb_bterms_update(kept_b, T, I) == 0)
      bp.dev = kept_b;
    else {
      if (kept_b) stb_bterms_free(kept_b);
      kept_b = bp.dev = stb_bterms_create(T, I);
    }
    if (!bp.dev) {
      fprintf(stderr, "sampleb(): no device memory for T[] (%s)\n", stb_last_error());
      exit(1);
    }
    /* (bp.dev stays: kept_b; stb_sampler_cache_clear drops it) */
    return draw_b_posterior(b_in, &bp, rng, loops, verbose);
  }
}

/* ---- the same step for a caller whose counts live on the device (include/stb_hip.h): Q from k_logq (hyperq.hip), T read
 * where it lives; lib/sampleb.c:101-157 from there on.  Never exits: NaN with stb_last_error() set. ---- */
double stb_sampleb_last_Q(void) { return last_Q; }

double stb_sampleb_device_ex(double b_in, int I, double shape, double scale, const uint32_t *d_N, const uint64_t *d_coff,
                             const uint32_t *d_T, double apar, void *rng, int loops, int verbose, uint64_t seed,
                             uint64_t sweep, void *stream, const char *who) {
  char msg[200];
  double Q;
  const char *bad = NULL;
  if (!(apar >= 0.0 && apar < 1.0)) bad = "discount a outside [0, 1)";
  else if (!isfinite(b_in) || !(b_in > -apar)) bad = "b_in must be finite and > -a";
  else if (!(scale > 0) || !isfinite(scale)) bad = "scale must be > 0";
  else if (I < 1 || !d_T || (!d_N && !d_coff)) bad = "I >= 1, the customers per restaurant and T are required";
  if (bad) {
    snprintf(msg, sizeof(msg), "%s: %s (a=%g, b_in=%g, scale=%g, I=%d)", who, bad, apar, b_in, scale, I);
    stb_fail_msg(msg);
    return NAN;
  }
  if (stb_hq_logq(b_in, scale, I, d_N, d_coff, NULL, &Q, seed, sweep, stream)) return NAN;
  last_Q = Q;
  if (apar == 0) {
    uint64_t Tsum;
    if (stb_hq_sum_u32(d_T, I, &Tsum, stream)) return NAN;
    return draw_b_gamma(shape + (double)Tsum, Q, rng, verbose);
  }
  {
    b_posterior bp;
    memset(&bp, 0, sizeof(bp));
    bp.Q = Q;
    bp.apar = apar;
    bp.shape = shape;
    bp.noexit = 1;
    kept_bdev = bp.dev = stb_bterms_borrow(kept_bdev, d_T, I, stream);
    if (!bp.dev) return NAN;
    return draw_b_posterior(b_in, &bp, rng, loops, verbose);
  }
}

double stb_sampleb_device(double b_in, int I, double shape, double scale, const uint32_t *d_N, const uint32_t *d_T,
                          double a, void *rng, int loops, int verbose, uint64_t seed, uint64_t sweep, void *stream) {
  if (I >= 1 && !d_N) {
    stb_fail_msg("stb_sampleb_device: d_N is required");
    return NAN;
  }
  return stb_sampleb_device_ex(b_in, I, shape, scale, d_N, NULL, d_T, a, rng, loops, verbose, seed, sweep, stream,
                               "stb_sampleb_device");
}
