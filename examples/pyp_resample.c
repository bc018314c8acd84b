/*
 * pyp_resample.c -- this repo's own end-to-end driver for the path libstb_amd accelerates
 * (the reference's counterpart is the hand-run test/demo.c).
 *
 *   1. synthesise seating data from a hierarchical Chinese-restaurant process: J restaurants share a
 *      base distribution over DISHES dishes; restaurant j seats NCUST customers under PYP(a0, b0);
 *   2. run the table-indicator Gibbs sampler on the table counts t[j][i] given the customer counts
 *      n[j][i], reading V^n_m = S^n_m / S^n_{m-1} from the library's ratio table (S_V);
 *   3. every few sweeps resample the concentration b (sampleb) and the discount a (samplea) and
 *      rebuild the table for the new discount (S_remake);
 *   4. optionally (-g D) also evaluate the discount's log-posterior on a D-point grid in one batched
 *      device call (stb_groups_aterms) and report its mode next to the sampled value;
 *   5. with -G k as well: the same grid sharded over k group sets, set s on GPU s % (number of GPUs), driven by
 *      THIS one host thread (stb_set_device + stb_groups_aterms_async on every set, then stb_groups_wait on
 *      every set: INTEGRATION.md section 5, pattern (a)) -- the discount axis of SURVEY 8e without MPI.
 *   6. with -d steps 2 and 3 run on the device from resident counts: stb_tindic_sweep -> stb_tindic_sampleb ->
 *      stb_tindic_to_groups + stb_groups_samplea; no pair and no per-restaurant array crosses to the host inside the loop
 *      (the indicator step then uses the exact prior ratio t/(n-t), see stb_hip.h, and counter-based uniforms).
 *   7. with -j the device loop draws a and b JOINTLY instead: stb_tindic_sweep -> stb_tindic_samplejoint, an exact
 *      independence Metropolis-Hastings step from nested grids on [0.02, 0.97] x [0.05, 500] (stb_hip.h).
 *   8. with -L the device loop (-d or -j) prints the log joint probability of the state after every iteration
 *      (stb_tindic_logjoint, the table-indicator representation): one launch on the resident counts, 64 bytes back.
 *   9. with -z the device loop also moves the data: before each indicator sweep every customer leaves its dish and is
 *      seated again at any dish of its restaurant (stb_tindic_sweep_dishes), under a likelihood with two synthetic
 *      classes (even customers favour even dishes, odd customers odd ones); n changes on the device and comes back once.
 *  10. with -w (needs -d -z) the likelihood and the base weights are parameters of the chain too: after each dish sweep every
 *      dish's class distribution is drawn from its Dirichlet(0.5) posterior given the (class, dish) counts and h from its
 *      Dirichlet(1) posterior given the table counts (stb_tindic_sample_lik, stb_tindic_sample_h), on the device; with -L
 *      the line gains the data term (stb_tindic_loglik) and the complete-data log joint.
 *  11. with -P (needs -d -z) every restaurant gets NCUST / 5 held-out customers of the same two synthetic classes; each
 *      iteration's line carries their log likelihood under the state's predictive dish proportions and the running
 *      estimate sum_c log((1/S) sum_s p_c) over the iterations so far (stb_tindic_heldout), and the per-customer
 *      perplexity is printed at the end.
 *  12. with -B (needs -d) every restaurant has a concentration of its own: after each sweep all of them are redrawn on the
 *      device in one exact step (stb_tindic_sampleb_groups, Teh's auxiliary variables), every later call reads them where
 *      they live (STB_BPAR_RESIDENT), and the discount step runs on them: stb_tindic_to_groups(..., STB_BPAR_RESIDENT) +
 *      stb_groups_samplea.  Each iteration's line ends with min, median and max of b_i from one read-back.  -B with -j is
 *      refused: the joint step models one shared b.
 *  13. with -H G (needs -d -z -w) the base weights are hierarchical: the restaurants are cut into G equal contiguous ranges,
 *      each with weights of its own under a shared root, and stb_tindic_sample_hgroups takes stb_tindic_sample_h's place
 *      (auxiliary tables, the root, the concentration alpha from a Gamma(1.1, 20) prior, then every group's h, one call);
 *      each iteration prints alpha and the largest |sum_k h_gk - 1| over the restaurants from one read-back of h.
 *  14. with -C (needs -d -z -w) every iteration also prints the collapsed log joint (stb_tindic_logjoint_collapsed): the base
 *      weights and every dish's class distribution summed out, so the figure is finite however small the drawn weights
 *      are and comparable between runs.  With -H it is the grouped model's, with log p(root | gamma = 1) and the
 *      concentration the step left; without, the flat model's with gamma = 1.  beta = 0.5 as the draws'.
 *  15. with -K (needs -d -z -w) the two Dirichlet concentrations are no longer constants: after every dish sweep beta, the
 *      prior of every dish's class distribution, is drawn from its conditional given the (class, dish) counts under a
 *      Gamma(1.1, 1) prior (stb_tindic_sample_beta) and feeds that iteration's stb_tindic_sample_lik and -C; without -H
 *      gamma, the prior of the flat base weights, is drawn too, under Gamma(1.1, 10) (stb_tindic_sample_gamma), and feeds
 *      stb_tindic_sample_h and -C.  Each iteration prints the drawn values.  (Under -H the root's gamma stays 1.)
 *  16. with -S (needs -d) the device loop does not start from the seating built in step 1: the object forgets it and seats
 *      its customers one by one on the device, from empty restaurants, under the start values of a and b and (with -z) the
 *      likelihood (stb_tindic_seat); the line printed is the log weight of that seating.
 *  17. with -Q R (needs -P) each iteration's held-out figures gain the sequential estimate: every restaurant's held-out
 *      customers seated one after another on a private copy of its state, R particles averaged inside the logarithm
 *      (stb_tindic_heldout_seq) -- the likelihood of the held-out customers as a whole, where -P scores each one alone.
 *  18. with -F tau (needs -Q R, R <= 64) the particle filter's figure stands next to it: the same R particles, resampled
 *      between customers when their effective number falls below tau R (stb_tindic_heldout_pf), and the resamplings.
 *  19. with -A S (needs -Q R) annealed importance sampling stands next to them: the same held-out customers scored as
 *      UNSEEN documents -- restaurants that start empty, with the chain's current h and likelihood -- by R particles that
 *      climb S temperatures, one dish sweep at each (stb_tindic_heldout_ais, on an empty twin of the object: the ladder's
 *      sweeps are exact only where every customer of a restaurant is the document's own).
 *  20. with -V rows (needs -d -z) the corpus is the model's own: every dish's distribution over `rows` classes is a draw
 *      from its Dirichlet(0.5) prior (stb_sample_lik on zero counts, into the object's matrix), and the seating and every
 *      customer's class are drawn on the device given that matrix (stb_tindic_generate).  The chain then starts from a
 *      fresh stb_tindic_seat under the generated classes, as with -S, and every iteration prints the data term
 *      (stb_tindic_loglik) and the collapsed log joint of the flat model.
 *  21. with -T a:b[:c...] (needs -d -z -w; not with -H or -C) the base weights sit on a tree of nested groups: a nodes of
 *      level 1 cut the restaurants into equal contiguous ranges as -H does, b nodes of level 2 cut those, and so on up to
 *      the root; stb_tindic_sample_htree takes stb_tindic_sample_h's place (auxiliary tables upwards, the root, every
 *      level's concentration from a Gamma(1.1, 20) prior, then the rows downwards, one call); each iteration prints the
 *      concentrations, level 1's first.
 *  22. with -X D the observations are real-valued: a PYP mixture of Gaussians with diagonal precisions in R^D
 *      (stb_tindic_set_obs).  Data from a few well-separated centres, a random start, then dish sweep ->
 *      stb_tindic_sample_gauss -> stb_tindic_sample_h -> stb_tindic_sampleb; every iteration prints the collapsed evidence
 *      log p(x | z) (stb_tindic_gauss_logml), which rises from the random start.  The other flags but -J -n -c -s -P are
 *      ignored.  With -P every restaurant gets NCUST / 5 further points from the same clusters, held out
 *      (stb_tindic_set_heldout_obs); each iteration prints their log predictive density under the state (`heldout`) and under
 *      the average over the iterations so far (`avg`, stb_tindic_gauss_heldout with STB_GH_ACCUMULATE), and the run ends
 *      with the share of held-out points whose largest responsibility names the dish that most training points of their
 *      generating cluster sit at.
 *
 * All table builds and every log-posterior evaluation run on the GPU through libstb_amd.so; this file
 * only uses the public headers.  Usage: pyp_resample [-J 3] [-n 2000] [-a 0.5] [-b 10] [-c 60]
 *                                                    [-g 64] [-G 2] [-s seed] [-d] [-j] [-L] [-z] [-w] [-P] [-B] [-H 4] [-C] [-K] [-S] [-Q 16] [-F 0.5] [-A 8] [-V 1000] [-T 8:2] [-X 2]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "psample.h"
#include "stable.h"
#include "stb_hip.h"
#include "yaps.h"

#define DISHES 50

static int cmp_double(const void *x, const void *y) {
  const double a = *(const double *)x, b = *(const double *)y;
  return a < b ? -1 : a > b;
}

/* -X D: a PYP mixture of Gaussians.  J restaurants x ncust customers; customer c carries x_c in R^D, drawn around one of
 * XTRUE well-separated centres (its restaurant prefers some of them); the model has XDISHES dishes, every customer starts
 * at a random one, and each iteration is dish sweep -> stb_tindic_sample_gauss -> stb_tindic_sample_h -> sampleb.  Prints
 * the collapsed evidence log p(x | z) (stb_tindic_gauss_logml) every iteration; returns 1 if it did not rise. */
#define XTRUE 4
#define XDISHES 8
static int gauss_mixture(int J, int ncust, int D, int cycles, long seed, int predict) {
  const size_t C = (size_t)J * ncust, G = (size_t)J * XDISHES;
  const double a = 0.1;
  double b = 1.0, centre[XTRUE][STB_GS_MAXD], first = 0.0, last = 0.0;
  double *x = malloc(sizeof(double) * C * D), *hf = malloc(sizeof(double) * G), *bvec = malloc(sizeof(double) * J);
  scnt_int *nf = calloc(G, sizeof(*nf)), *cust = malloc(sizeof(*cust) * C);
  stcnt_int *tf = calloc(G, sizeof(*tf));
  int *K = malloc(sizeof(int) * J), j, d, it;
  size_t c, g;
  /* -P: NCUST / 5 further points a restaurant from the same clusters, held out; ztrue / zheld: the generating clusters */
  const size_t nheld = predict ? (size_t)(ncust / 5 > 0 ? ncust / 5 : 1) : 0, Ch = (size_t)J * nheld;
  int *ztrue = malloc(sizeof(int) * C), *zheld = malloc(sizeof(int) * (Ch ? Ch : 1));
  double *y = malloc(sizeof(double) * (Ch ? Ch : 1) * D), *resp = malloc(sizeof(double) * (Ch ? Ch : 1) * XDISHES);
  uint64_t *hoff = malloc(sizeof(uint64_t) * (J + 1));
  for (j = 0; j < XTRUE; j++)
    for (d = 0; d < D; d++) centre[j][d] = 8.0 * ((j >> (d & 1)) & 1 ? 1.0 : -1.0) + (d > 1 ? 2.0 * j : 0.0);
  for (c = 0; c < C; c++) {
    const int rest = (int)(c / ncust), z = drand48() < 0.7 ? rest % XTRUE : (int)(drand48() * XTRUE) % XTRUE;
    ztrue[c] = z;
    for (d = 0; d < D; d++) /* Box-Muller's cosine member */
      x[c * D + d] = centre[z][d] + sqrt(-2.0 * log(1.0 - drand48())) * cos(6.283185307179586 * drand48());
    cust[c] = (scnt_int)((int)(drand48() * XDISHES) % XDISHES); /* the random start */
    nf[(size_t)rest * XDISHES + cust[c]]++;
  }
  for (c = 0; c < Ch; c++) { /* (after the training points: without -P the data are what they were) */
    const int rest = (int)(c / nheld), z = drand48() < 0.7 ? rest % XTRUE : (int)(drand48() * XTRUE) % XTRUE;
    zheld[c] = z;
    for (d = 0; d < D; d++)
      y[c * D + d] = centre[z][d] + sqrt(-2.0 * log(1.0 - drand48())) * cos(6.283185307179586 * drand48());
  }
  for (j = 0; j <= J; j++) hoff[j] = (uint64_t)j * nheld;
  for (g = 0; g < G; g++) {
    tf[g] = nf[g] ? 1 : 0;
    hf[g] = 1.0 / XDISHES;
  }
  for (j = 0; j < J; j++) K[j] = XDISHES, bvec[j] = b;
  const stb_gauss_prior_t prior = {0.01, 1.0, 1.0, NULL, NULL};
  stb_gauss_info_t gi;
  stb_tindic_t *ti = stb_tindic_create(J, K, nf, tf, hf, cust, ncust > 65535 ? 65535 : 0, 0);
  if (!ti || stb_tindic_set_obs(ti, x, (unsigned)D)) yaps_quit("the observations: %s\n", stb_last_error());
  if (predict && stb_tindic_set_heldout_obs(ti, hoff, y)) yaps_quit("the held-out points: %s\n", stb_last_error());
  if (stb_tindic_sample_gauss(ti, &prior, (uint64_t)seed + 2, 0, &gi) || stb_tindic_gauss_logml(ti, &prior, &first))
    yaps_quit("the first draw: %s\n", stb_last_error());
  printf("Gaussian mixture: %d restaurants x %d customers in R^%d, %d centres, %d dishes; start: log p(x | z) = %.6f\n", J, ncust, D,
         XTRUE, XDISHES, first);
  for (it = 1; it <= cycles; it++) {
    stb_tdish_info_t di;
    double data = 0.0;
    if (stb_tindic_sweep_dishes(ti, a, bvec, (uint64_t)seed, (uint64_t)it, 1, &di) ||
        stb_tindic_sample_gauss(ti, &prior, (uint64_t)seed + 2, (uint64_t)it, &gi) ||
        stb_tindic_sample_h(ti, NULL, 1.0, (uint64_t)seed + 3, (uint64_t)it))
      yaps_quit("iteration %d: %s\n", it, stb_last_error());
    b = stb_tindic_sampleb(ti, b, 1.1, 20.0, a, 0, 1, 0, (uint64_t)seed + 1, (uint64_t)it);
    if (b != b) yaps_quit("stb_tindic_sampleb: %s\n", stb_last_error());
    for (j = 0; j < J; j++) bvec[j] = b;
    if (stb_tindic_gauss_logml(ti, &prior, &last) || stb_tindic_gauss_loglik(ti, &data))
      yaps_quit("the evidence: %s\n", stb_last_error());
    printf("iter %3d  b=%.4f  log p(x | z) = %.6f  log p(x | z, mu, tau) = %.6f  stuck %llu dead rows %llu", it, b, last, data,
           (unsigned long long)di.stuck, (unsigned long long)gi.dead);
    if (predict) { /* this state's log predictive density of the held-out points, and the average over the states so far */
      double ho = 0.0, ho_avg = 0.0;
      if (stb_tindic_gauss_heldout(ti, a, bvec, 0, &ho, NULL, NULL, NULL) ||
          stb_tindic_gauss_heldout(ti, a, bvec, STB_GH_ACCUMULATE, &ho_avg, NULL, it == cycles ? resp : NULL, NULL))
        yaps_quit("stb_tindic_gauss_heldout: %s\n", stb_last_error());
      printf("  heldout = %.6f  avg = %.6f", ho, ho_avg);
    }
    printf("\n");
  }
  if (predict && cycles > 0) {
    /* a cluster's dish: where most of its training points sit now; a held-out point is classified by its largest
     * responsibility under the last state */
    unsigned long votes[XTRUE][XDISHES] = {{0}}, hit = 0;
    uint32_t *now = malloc(sizeof(uint32_t) * C);
    int major[XTRUE], k;
    if (stb_tindic_get_state(ti, NULL, now)) yaps_quit("stb_tindic_get_state: %s\n", stb_last_error());
    for (c = 0; c < C; c++) votes[ztrue[c]][now[c] % XDISHES]++;
    for (j = 0; j < XTRUE; j++)
      for (major[j] = 0, k = 1; k < XDISHES; k++)
        if (votes[j][k] > votes[j][major[j]]) major[j] = k;
    for (c = 0; c < Ch; c++) {
      int best = 0;
      for (k = 1; k < XDISHES; k++)
        if (resp[c * XDISHES + k] > resp[c * XDISHES + best]) best = k;
      hit += best == major[zheld[c]];
    }
    printf("held-out points classified to their cluster's dish: %lu of %lu (%.1f %%)\n", hit, (unsigned long)Ch, 100.0 * hit / Ch);
    free(now);
  }
  printf("evidence: %.6f -> %.6f (%s)\n", first, last, last > first ? "rose" : "DID NOT RISE");
  stb_tindic_free(ti);
  free(x), free(hf), free(bvec), free(nf), free(cust), free(tf), free(K);
  free(ztrue), free(zheld), free(y), free(resp), free(hoff);
  return last > first ? 0 : 1;
}

int main(int argc, char **argv) {
  int xdim = 0;
  int J = 3, ncust = 2000, cycles = 60, grid = 0, nsets = 0, ondev = 0, joint = 0, showlj = 0, dishes = 0, redraw = 0, predict = 0, explicit_d = 0, pergroup = 0, hgroups = 0, collapsed = 0, drawconc = 0, seatdev = 0, seqpart = 0, filter = 0, vrows = 0, anneal = 0, tlevels = 0, tnodes[STB_HT_MAXL], c, j, i, it;
  double ftau = 0.0;
  double a0 = 0.5, b0 = 10.0, beta = 0.5, gam = 1.0;
  long seed = 12345;
  while ((c = getopt(argc, argv, "J:n:a:b:c:g:G:s:djLzwPBH:CKSQ:F:V:A:T:X:")) >= 0) {
    if (c == 'J') J = atoi(optarg);
    else if (c == 'n') ncust = atoi(optarg);
    else if (c == 'a') a0 = atof(optarg);
    else if (c == 'b') b0 = atof(optarg);
    else if (c == 'c') cycles = atoi(optarg);
    else if (c == 'g') grid = atoi(optarg);
    else if (c == 'G') nsets = atoi(optarg);
    else if (c == 's') seed = atol(optarg);
    else if (c == 'd') ondev = explicit_d = 1;
    else if (c == 'j') ondev = joint = 1;
    else if (c == 'L') showlj = 1;
    else if (c == 'z') ondev = dishes = 1;
    else if (c == 'w') redraw = 1;
    else if (c == 'P') predict = 1;
    else if (c == 'B') pergroup = 1;
    else if (c == 'H') hgroups = atoi(optarg);
    else if (c == 'C') collapsed = 1;
    else if (c == 'K') drawconc = 1;
    else if (c == 'S') seatdev = 1;
    else if (c == 'Q') seqpart = atoi(optarg) >= 1 ? atoi(optarg) : -1;
    else if (c == 'F') filter = 1, ftau = atof(optarg);
    else if (c == 'A') anneal = atoi(optarg) >= 1 ? atoi(optarg) : -1;
    else if (c == 'T') { /* the nodes of every level, level 1 first */
      const char *p = optarg;
      tlevels = 0;
      while (*p) {
        char *end;
        const long v = strtol(p, &end, 10);
        if (end == p || v < 1 || v > 1000000 || tlevels == STB_HT_MAXL || (*end && (*end != ':' || !end[1]))) {
          tlevels = -1;
          break;
        }
        tnodes[tlevels++] = (int)v;
        p = *end ? end + 1 : end;
      }
      if (tlevels == 0) tlevels = -1;
    }
    else if (c == 'V') vrows = atoi(optarg) >= 2 ? atoi(optarg) : -1;
    else if (c == 'X') xdim = atoi(optarg) >= 1 && atoi(optarg) <= STB_GS_MAXD ? atoi(optarg) : -1;
    else return 2;
  }
  if (collapsed && !(explicit_d && dishes && redraw)) {
    fprintf(stderr, "pyp_resample: -C needs -d -z -w\n");
    return 2;
  }
  if (drawconc && !(explicit_d && dishes && redraw)) {
    fprintf(stderr, "pyp_resample: -K needs -d -z -w\n");
    return 2;
  }
  if (redraw && !(explicit_d && dishes)) {
    fprintf(stderr, "pyp_resample: -w needs -d -z\n");
    return 2;
  }
  if (hgroups < 0 || (hgroups && !(explicit_d && dishes && redraw))) {
    fprintf(stderr, "pyp_resample: -H G needs G >= 1 and -d -z -w\n");
    return 2;
  }
  if (tlevels < 0 || (tlevels && (!(explicit_d && dishes && redraw) || hgroups || collapsed))) {
    fprintf(stderr, "pyp_resample: -T a:b[:c] needs 1 to %d levels of >= 1 nodes and -d -z -w, without -H and -C\n", STB_HT_MAXL);
    return 2;
  }
  if (predict && !xdim && !(explicit_d && dishes)) {
    fprintf(stderr, "pyp_resample: -P needs -d -z\n");
    return 2;
  }
  if (seatdev && !explicit_d) {
    fprintf(stderr, "pyp_resample: -S needs -d\n");
    return 2;
  }
  if (seqpart < 0 || seqpart > 4096 || (seqpart && !predict)) {
    fprintf(stderr, "pyp_resample: -Q R needs 1 <= R <= 4096 and -P\n");
    return 2;
  }
  if (filter && (!seqpart || seqpart > STB_PF_MAXR || !(ftau >= 0.0 && ftau <= 1.0))) {
    fprintf(stderr, "pyp_resample: -F tau needs 0 <= tau <= 1 and -Q R with R <= %d\n", STB_PF_MAXR);
    return 2;
  }
  if (anneal < 0 || (anneal && !seqpart)) {
    fprintf(stderr, "pyp_resample: -A S needs S >= 1 and -Q R\n");
    return 2;
  }
  if (vrows < 0 || (vrows && !(explicit_d && dishes))) {
    fprintf(stderr, "pyp_resample: -V rows needs rows >= 2 and -d -z\n");
    return 2;
  }
  if (pergroup && (!explicit_d || joint)) {
    fprintf(stderr, joint ? "pyp_resample: -B with -j is refused: the joint step models one shared b\n" : "pyp_resample: -B needs -d\n");
    return 2;
  }
  if (xdim < 0) {
    fprintf(stderr, "pyp_resample: -X D needs 1 <= D <= %d\n", STB_GS_MAXD);
    return 2;
  }
  srand48(seed);
  srand((unsigned)seed);
  if (xdim) return gauss_mixture(J, ncust, xdim, cycles, seed, predict); /* 22.: a mixture of Gaussians, nothing else of this file */

  /* ---- 1. data: seat customers, remember per (restaurant, dish) customers n and tables t ---- */
  scnt_int **n = malloc(sizeof(*n) * J), *N = calloc(J, sizeof(*N)), *T = calloc(J, sizeof(*T));
  stcnt_int **t = malloc(sizeof(*t) * J);
  int *K = malloc(sizeof(int) * J);
  int *dish_of = malloc(sizeof(int) * (size_t)J * ncust); /* customer -> dish, for the Gibbs sweep */
  unsigned maxn = 1;
  for (j = 0; j < J; j++) {
    /* tables of this restaurant: size and dish */
    int *tsize = calloc(ncust, sizeof(int)), *tdish = calloc(ncust, sizeof(int)), ntab = 0, cst;
    n[j] = calloc(DISHES, sizeof(scnt_int));
    t[j] = calloc(DISHES, sizeof(stcnt_int));
    K[j] = DISHES;
    for (cst = 0; cst < ncust; cst++) {
      double pnew = (b0 + a0 * ntab) / (b0 + cst);
      int tab;
      if (ntab == 0 || rng_unit(0) < pnew) {
        tab = ntab++;
        tdish[tab] = (int)(rng_unit(0) * DISHES) % DISHES; /* uniform base distribution */
        t[j][tdish[tab]]++;
      } else {
        /* existing table k with probability proportional to (size_k - a0) */
        double u = rng_unit(0) * (cst - a0 * ntab);
        for (tab = 0; tab < ntab - 1; tab++) {
          u -= tsize[tab] - a0;
          if (u < 0) break;
        }
      }
      tsize[tab]++;
      n[j][tdish[tab]]++;
      dish_of[(size_t)j * ncust + cst] = tdish[tab];
    }
    N[j] = ncust;
    T[j] = ntab;
    for (i = 0; i < DISHES; i++)
      if (n[j][i] >= maxn) maxn = n[j][i] + 1;
    free(tsize);
    free(tdish);
  }
  printf("data: %d restaurants x %d customers, true a=%.3f b=%.2f, tables:", J, ncust, a0, b0);
  for (j = 0; j < J; j++) printf(" %u", T[j]);
  printf("\n");

  /* ---- 2./3. Gibbs on table counts with periodic hyper-parameter resampling ---- */
  double a = 0.3, b = 5.0, asum = 0, bsum = 0;
  int kept = 0;
  unsigned maxt = maxn < 400 ? maxn : 400;
  stable_t *S = ondev ? NULL : S_make(maxn, maxt, maxn, maxn, a, S_STABLE | S_UVTABLE);
  if (!S && !ondev) yaps_quit("S_make failed: %s\n", stb_last_error());
  double *bvec = malloc(sizeof(double) * J);
  if (ondev) {
    /* ---- 6. the same loop from device-resident counts: the pairs go to the device once, t and T come back once ---- */
    size_t G = (size_t)J * DISHES, g = 0, cc;
    scnt_int *nf = malloc(sizeof(*nf) * G), *cust = malloc(sizeof(*cust) * (size_t)J * ncust);
    stcnt_int *tf = malloc(sizeof(*tf) * G);
    double *hf = malloc(sizeof(double) * G);
    for (j = 0; j < J; j++)
      for (i = 0; i < DISHES; i++, g++) {
        nf[g] = n[j][i];
        tf[g] = t[j][i];
        hf[g] = 1.0 / DISHES;
      }
    for (cc = 0; cc < (size_t)J * ncust; cc++) cust[cc] = (scnt_int)dish_of[cc]; /* (K = DISHES: the dish is the local pair) */
    stb_tindic_t *ti = stb_tindic_create(J, K, nf, tf, hf, cust, maxn > 65535 || ((dishes || seatdev) && ncust > 65535) ? 65535 : 0, 0);
    stb_groups_t *gs = stb_groups_create(J, K, NULL, NULL, NULL, NULL, 0, 0, joint ? 25 : 3);
    int accepted = 0, steps = 0;
    if (!ti || !gs) yaps_quit("device loop: %s\n", stb_last_error());
    for (j = 0; j < J; j++) bvec[j] = b;
    /* -B: the concentrations live on the device from here on; every call below reads them there */
    const double *bp = pergroup ? STB_BPAR_RESIDENT : bvec;
    double *bsort = malloc(sizeof(double) * J);
    if (pergroup && stb_tindic_set_bpar(ti, bvec)) yaps_quit("stb_tindic_set_bpar: %s\n", stb_last_error());
    unsigned long long stuck = 0;
    if (vrows) { /* the model's own corpus: the matrix from its prior, then seating and classes drawn given it */
      unsigned lr, ls;
      void *lst;
      const size_t cells = (size_t)vrows * DISHES;
      scnt_int *zero = calloc(cells, sizeof(*zero));
      void *d_zero = stb_device_malloc(sizeof(*zero) * cells);
      stb_seat_info_t si;
      stb_classes_info_t ci;
      if (stb_tindic_set_lik(ti, NULL, (unsigned)vrows, DISHES)) yaps_quit("stb_tindic_set_lik: %s\n", stb_last_error());
      double *d_lik = stb_tindic_lik_device(ti, &lr, &ls, &lst);
      if (!d_zero || !d_lik || stb_memcpy_h2d(d_zero, zero, sizeof(*zero) * cells, lst) ||
          stb_sample_lik(d_zero, lr, ls, NULL, beta, d_lik, (uint64_t)seed + 9, 0, lst))
        yaps_quit("the matrix from its prior: %s\n", stb_last_error());
      double *btrue = malloc(sizeof(double) * J); /* the corpus comes from the true a and b, the chain starts elsewhere */
      for (j = 0; j < J; j++) btrue[j] = b0;
      if (stb_tindic_generate(ti, a0, btrue, (uint64_t)seed + 10, 0, &si, &ci)) yaps_quit("stb_tindic_generate: %s\n", stb_last_error());
      if (pergroup && stb_tindic_set_bpar(ti, bvec)) yaps_quit("stb_tindic_set_bpar: %s\n", stb_last_error());
      free(btrue);
      printf("corpus generated on the device: %llu customers, %llu classes drawn over %d rows, %llu left alone\n",
             (unsigned long long)si.customers, (unsigned long long)ci.drawn, vrows, (unsigned long long)(ci.stuck + ci.skipped));
      stb_device_free(d_zero);
      free(zero);
      seatdev = 1;
    } else if (dishes) { /* two classes by the customer's parity; a class likes the dishes of its parity twice as much */
      scnt_int *cls = malloc(sizeof(*cls) * (size_t)J * ncust);
      double lik[2 * DISHES];
      for (cc = 0; cc < (size_t)J * ncust; cc++) cls[cc] = (scnt_int)(cc & 1);
      for (i = 0; i < 2 * DISHES; i++) lik[i] = ((i % DISHES) & 1) == i / DISHES ? 1.0 : 0.5;
      if (stb_tindic_set_classes(ti, cls, 2) || stb_tindic_set_lik(ti, lik, 2, DISHES)) yaps_quit("dishes: %s\n", stb_last_error());
      free(cls);
    }
    double ho_avg = 0.0;
    uint64_t ho_n = 0;
    if (predict) { /* ncust / 5 held-out customers a restaurant, the classes by parity as above */
      const uint64_t per = (uint64_t)ncust / 5;
      uint64_t *hoff = malloc(sizeof(*hoff) * ((size_t)J + 1));
      scnt_int *hcls = malloc(sizeof(*hcls) * ((size_t)J * per + 1));
      ho_n = (uint64_t)J * per;
      for (j = 0; j <= J; j++) hoff[j] = (uint64_t)j * per;
      for (cc = 0; cc < ho_n; cc++) hcls[cc] = (scnt_int)(cc & 1);
      if (stb_tindic_set_heldout(ti, hoff, hcls)) yaps_quit("held-out customers: %s\n", stb_last_error());
      free(hoff);
      free(hcls);
    }
    /* -A: an empty twin of the object -- the same dishes, no customers -- that scores the held-out customers as unseen
     * documents; it is given the chain's h and matrix before every use */
    stb_tindic_t *tu = NULL;
    double *ulik = NULL, *uh = NULL;
    if (anneal) {
      int *Ku = malloc(sizeof(*Ku) * (size_t)J);
      scnt_int *nu = calloc((size_t)J * DISHES, sizeof(*nu));
      stcnt_int *tz = calloc((size_t)J * DISHES, sizeof(*tz));
      const uint64_t per = (uint64_t)ncust / 5;
      uint64_t *hoff = malloc(sizeof(*hoff) * ((size_t)J + 1));
      scnt_int *hcls = malloc(sizeof(*hcls) * ((size_t)J * per + 1));
      for (j = 0; j < J; j++) Ku[j] = DISHES;
      for (j = 0; j <= J; j++) hoff[j] = (uint64_t)j * per;
      for (cc = 0; cc < (size_t)J * per; cc++) hcls[cc] = (scnt_int)(cc & 1);
      tu = stb_tindic_create(J, Ku, nu, tz, NULL, NULL, 0, 0);
      if (!tu || stb_tindic_set_lik(tu, NULL, 2, DISHES) || stb_tindic_set_heldout(tu, hoff, hcls))
        yaps_quit("the empty twin: %s\n", stb_last_error());
      uh = malloc(sizeof(double) * (size_t)J * DISHES);
      free(Ku), free(nu), free(tz), free(hoff), free(hcls);
    }
    double *hflat = NULL;
    if (hgroups) { /* hgroups equal contiguous ranges of restaurants, each with base weights of its own */
      uint64_t *hgoff = malloc(sizeof(*hgoff) * ((size_t)hgroups + 1));
      for (j = 0; j <= hgroups; j++) hgoff[j] = (uint64_t)j * (uint64_t)J / (uint64_t)hgroups;
      if (stb_tindic_set_hgroups(ti, hgroups, hgoff)) yaps_quit("stb_tindic_set_hgroups: %s\n", stb_last_error());
      free(hgoff);
      hflat = malloc(sizeof(double) * (size_t)J * DISHES);
    }
    if (tlevels) { /* every level cuts the one below into equal contiguous ranges */
      uint64_t *toff[STB_HT_MAXL];
      int below = J;
      for (i = 0; i < tlevels; i++) {
        toff[i] = malloc(sizeof(uint64_t) * ((size_t)tnodes[i] + 1));
        for (j = 0; j <= tnodes[i]; j++) toff[i][j] = (uint64_t)j * (uint64_t)below / (uint64_t)tnodes[i];
        below = tnodes[i];
      }
      if (stb_tindic_set_htree(ti, tlevels, tnodes, (const uint64_t *const *)toff)) yaps_quit("stb_tindic_set_htree: %s\n", stb_last_error());
      for (i = 0; i < tlevels; i++) free(toff[i]);
      hflat = malloc(sizeof(double) * (size_t)J * DISHES);
    }
    if (seatdev) { /* the start state from the model, on the device: a seed of its own */
      double lw;
      stb_seat_info_t si;
      if (stb_tindic_seat(ti, a, bp, (uint64_t)seed + 7, 0, &lw, &si)) yaps_quit("stb_tindic_seat: %s\n", stb_last_error());
      printf("start state seated on the device: %llu customers, log weight %.6f, %llu impossible visits\n",
             (unsigned long long)si.customers, lw, (unsigned long long)si.impossible);
    }
    for (it = 0; it < cycles; it++) {
      if (dishes) {
        stb_tdish_info_t di;
        if (stb_tindic_sweep_dishes(ti, a, bp, (uint64_t)seed + 2, (uint64_t)it, 1, &di)) yaps_quit("stb_tindic_sweep_dishes: %s\n", stb_last_error());
        stuck += di.stuck + di.skipped;
        if (drawconc) { /* the concentrations first, given the counts the sweep left: seeds of their own again */
          stb_dirconc_info_t ki;
          if (stb_tindic_sample_beta(ti, NULL, beta, 1.1, 1.0, (uint64_t)seed + 5, (uint64_t)it, &ki))
            yaps_quit("stb_tindic_sample_beta: %s\n", stb_last_error());
          beta = ki.s;
          printf("iteration %d: beta %.6f from %llu customers, %llu auxiliary\n", it, beta, (unsigned long long)ki.count,
                 (unsigned long long)ki.aux_tables);
          if (!hgroups && !tlevels) {
            if (stb_tindic_sample_gamma(ti, NULL, gam, 1.1, 10.0, (uint64_t)seed + 6, (uint64_t)it, &ki))
              yaps_quit("stb_tindic_sample_gamma: %s\n", stb_last_error());
            gam = ki.s;
            printf("iteration %d: gamma %.6f from %llu tables, %llu auxiliary\n", it, gam, (unsigned long long)ki.count,
                   (unsigned long long)ki.aux_tables);
          }
        }
        /* the uncollapsed step: seeds of their own, so neither shares a stream with a sweep or with the other */
        if (redraw && hgroups) { /* alpha: 5 to start with, then what the step before left on the device */
          stb_hgroups_opts_t ho = {it == 0 ? 5.0 : 0.0, 1.0, 1.1, 20.0, NULL, STB_HG_SAMPLE_ALPHA, 0};
          stb_hgroups_info_t hi;
          double worst = 0.0;
          if (stb_tindic_sample_lik(ti, NULL, beta, (uint64_t)seed + 3, (uint64_t)it) ||
              stb_tindic_sample_hgroups(ti, &ho, (uint64_t)seed + 4, (uint64_t)it, &hi) || stb_tindic_get_h(ti, hflat))
            yaps_quit("stb_tindic_sample_lik / _sample_hgroups: %s\n", stb_last_error());
          for (j = 0; j < J; j++) {
            double sum = 0.0;
            for (i = 0; i < DISHES; i++) sum += hflat[(size_t)j * DISHES + i];
            if (fabs(sum - 1.0) > worst) worst = fabs(sum - 1.0);
          }
          printf("iteration %d: base weights in %d groups, alpha %.6f, %llu tables, %llu auxiliary, largest |sum h - 1| %.3g\n", it,
                 hgroups, hi.alpha, (unsigned long long)hi.tables, (unsigned long long)hi.aux_tables, worst);
        } else if (redraw && tlevels) { /* every alpha: 5 to start with, then what the step before left on the device */
          const double start[STB_HT_MAXL] = {5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0};
          stb_htree_opts_t to = {tlevels, it == 0 ? start : NULL, 1.0, 1.1, 20.0, NULL, STB_HT_SAMPLE_ALPHA, 0};
          stb_htree_info_t hi;
          double worst = 0.0;
          if (stb_tindic_sample_lik(ti, NULL, beta, (uint64_t)seed + 3, (uint64_t)it) ||
              stb_tindic_sample_htree(ti, &to, (uint64_t)seed + 4, (uint64_t)it, &hi) || stb_tindic_get_h(ti, hflat))
            yaps_quit("stb_tindic_sample_lik / _sample_htree: %s\n", stb_last_error());
          for (j = 0; j < J; j++) {
            double sum = 0.0;
            for (i = 0; i < DISHES; i++) sum += hflat[(size_t)j * DISHES + i];
            if (fabs(sum - 1.0) > worst) worst = fabs(sum - 1.0);
          }
          printf("iteration %d: base weights on a tree of %d levels, alpha", it, tlevels);
          for (i = 0; i < tlevels; i++) printf(" %.6f", hi.alpha[i]);
          printf(", %llu tables, %llu auxiliary at level 1, largest |sum h - 1| %.3g\n", (unsigned long long)hi.tables[0],
                 (unsigned long long)hi.aux_tables[0], worst);
        } else if (redraw && (stb_tindic_sample_lik(ti, NULL, beta, (uint64_t)seed + 3, (uint64_t)it) ||
                              stb_tindic_sample_h(ti, NULL, gam, (uint64_t)seed + 4, (uint64_t)it)))
          yaps_quit("stb_tindic_sample_lik / _sample_h: %s\n", stb_last_error());
      }
      if (stb_tindic_sweep(ti, a, bp, (uint64_t)seed, (uint64_t)it, 1)) yaps_quit("stb_tindic_sweep: %s\n", stb_last_error());
      if (pergroup) {
        stb_bgroups_info_t bi;
        if (stb_tindic_sampleb_groups(ti, a, 1.1, 20.0, (uint64_t)seed + 1, (uint64_t)it, NULL, &bi))
          yaps_quit("stb_tindic_sampleb_groups: %s\n", stb_last_error());
        if (it % 3 == 2) {
          if (stb_tindic_to_groups(ti, gs, STB_BPAR_RESIDENT)) yaps_quit("stb_tindic_to_groups: %s\n", stb_last_error());
          a = stb_groups_samplea(gs, a, 0, 1, 0);
          if (a != a) yaps_quit("stb_groups_samplea: %s\n", stb_last_error());
        }
      } else if (it % 3 == 2 && joint) {
        stb_joint_opts_t jo = {0.02, 0.97, 0.05, 500.0, 24, 24, 1.1, 20.0, (uint64_t)seed + 1, (uint64_t)it, 0};
        stb_joint_info_t ji;
        if (stb_tindic_samplejoint(ti, gs, &jo, a, b, &a, &b, &ji)) yaps_quit("stb_tindic_samplejoint: %s\n", stb_last_error());
        accepted += ji.accepted;
        steps++;
        for (j = 0; j < J; j++) bvec[j] = b;
        if (it >= cycles / 2) {
          asum += a;
          bsum += b;
          kept++;
        }
      } else if (it % 3 == 2) {
        b = stb_tindic_sampleb(ti, b, 1.1, 20.0, a, 0, 1, 0, (uint64_t)seed + 1, (uint64_t)it);
        if (b != b) yaps_quit("stb_tindic_sampleb: %s\n", stb_last_error());
        for (j = 0; j < J; j++) bvec[j] = b;
        if (stb_tindic_to_groups(ti, gs, bvec)) yaps_quit("stb_tindic_to_groups: %s\n", stb_last_error());
        a = stb_groups_samplea(gs, a, 0, 1, 0);
        if (a != a) yaps_quit("stb_groups_samplea: %s\n", stb_last_error());
        if (it >= cycles / 2) {
          asum += a;
          bsum += b;
          kept++;
        }
      }
      if (showlj) {
        double lj;
        stb_logjoint_info_t li;
        if (stb_tindic_logjoint(ti, a, bp, STB_LJ_INDICATORS, &lj, NULL, &li)) yaps_quit("stb_tindic_logjoint: %s\n", stb_last_error());
        if (redraw) {
          double dt;
          if (stb_tindic_loglik(ti, &dt, NULL)) yaps_quit("stb_tindic_loglik: %s\n", stb_last_error());
          printf("iteration %d: log joint %.6f (pairs %.6f, base %.6f, restaurants %.6f, indicators %.6f) data %.6f complete %.6f "
                 "a=%.4f b=%.3f%s", it, lj, li.pairs, li.base, li.restaurants, li.binom, dt, lj + dt, a, b, predict ? "" : "\n");
        } else
          printf("iteration %d: log joint %.6f (pairs %.6f, base %.6f, restaurants %.6f, indicators %.6f) a=%.4f b=%.3f%s", it, lj,
                 li.pairs, li.base, li.restaurants, li.binom, a, b, predict ? "" : "\n");
      }
      if (predict) {
        double ho;
        if (stb_tindic_heldout(ti, a, bp, 0, &ho, NULL, NULL) || stb_tindic_heldout(ti, a, bp, STB_PR_ACCUMULATE, &ho_avg, NULL, NULL))
          yaps_quit("stb_tindic_heldout: %s\n", stb_last_error());
        if (showlj) printf(" heldout %.6f avg %.6f", ho, ho_avg);
        else printf("iteration %d: heldout %.6f avg %.6f", it, ho, ho_avg);
        if (seqpart) { /* the held-out customers of a restaurant as a whole: seated one by one, a seed of its own */
          double hs;
          if (stb_tindic_heldout_seq(ti, a, bp, (unsigned)seqpart, (uint64_t)seed + 8, (uint64_t)it * 4096u, &hs, NULL, NULL))
            yaps_quit("stb_tindic_heldout_seq: %s\n", stb_last_error());
          printf(" seq %.6f", hs);
          if (filter) { /* the same particles, resampled between customers */
            stb_pf_info_t fi;
            if (stb_tindic_heldout_pf(ti, a, bp, (unsigned)seqpart, ftau, (uint64_t)seed + 8, (uint64_t)it * 4096u, &hs, NULL, &fi))
              yaps_quit("stb_tindic_heldout_pf: %s\n", stb_last_error());
            printf(" pf %.6f (%llu resamplings)", hs, (unsigned long long)fi.resamplings);
          }
          if (anneal) { /* the same customers as unseen documents: the chain's h and matrix on the empty twin */
            unsigned lr, ls;
            void *lst;
            stb_ais_info_t ai;
            const double *d_lik = stb_tindic_lik_device(ti, &lr, &ls, &lst);
            if (d_lik && !ulik) ulik = malloc(sizeof(double) * (size_t)lr * ls);
            if (!d_lik || stb_memcpy_d2h(ulik, d_lik, sizeof(double) * (size_t)lr * ls, lst) || stb_tindic_get_h(ti, uh) ||
                stb_tindic_set_lik(tu, ulik, lr, ls) || stb_tindic_set_h(tu, uh) || (pergroup && stb_tindic_get_bpar(ti, bvec)))
              yaps_quit("the empty twin's h and matrix: %s\n", stb_last_error());
            if (stb_tindic_heldout_ais(tu, a, pergroup ? bvec : bp, (unsigned)seqpart, (unsigned)anneal, NULL, 1, (uint64_t)seed + 8,
                                       (uint64_t)it * 4096u, &hs, NULL, &ai))
              yaps_quit("stb_tindic_heldout_ais: %s\n", stb_last_error());
            printf(" ais %.6f (unseen, %d temperatures, %llu dead)", hs, anneal, (unsigned long long)ai.dead);
          }
        }
        printf("\n");
      }
      if (collapsed) { /* h and the likelihood summed out: alpha 0 is the concentration the -H step left on the object */
        stb_cj_opts_t co = {0.0, hgroups ? 1.0 : gam, beta, NULL, NULL};
        stb_cj_info_t ci;
        double cj;
        if (stb_tindic_logjoint_collapsed(ti, a, bp, STB_CJ_INDICATORS | STB_CJ_DATA | (hgroups ? STB_CJ_ROOT : STB_CJ_FLAT), &co,
                                          &cj, &ci))
          yaps_quit("stb_tindic_logjoint_collapsed: %s\n", stb_last_error());
        printf("iteration %d: collapsed log joint %.6f (pairs %.6f, restaurants %.6f, indicators %.6f, tables %.6f, data %.6f, "
               "root %.6f)\n", it, cj, ci.pairs, ci.restaurants, ci.binom, ci.tables, ci.data, ci.root);
      }
      if (vrows) { /* the generated corpus: the data term under the matrix, and the flat model's collapsed log joint */
        stb_cj_opts_t co = {0.0, gam, beta, NULL, NULL};
        double dt, cj;
        if (stb_tindic_loglik(ti, &dt, NULL) ||
            stb_tindic_logjoint_collapsed(ti, a, bp, STB_CJ_INDICATORS | STB_CJ_DATA | STB_CJ_FLAT, &co, &cj, NULL))
          yaps_quit("stb_tindic_loglik / _logjoint_collapsed: %s\n", stb_last_error());
        printf("iteration %d: generated corpus data %.6f collapsed %.6f\n", it, dt, cj);
      }
      if (pergroup) { /* the iteration's one read-back: the J concentrations */
        if (stb_tindic_get_bpar(ti, bvec)) yaps_quit("stb_tindic_get_bpar: %s\n", stb_last_error());
        memcpy(bsort, bvec, sizeof(double) * J);
        qsort(bsort, J, sizeof(double), cmp_double);
        b = bsort[J / 2];
        printf("iteration %d: a=%.4f b_i min %.6g median %.6g max %.6g\n", it, a, bsort[0], b, bsort[J - 1]);
        if (it % 3 == 2 && it >= cycles / 2) {
          asum += a;
          bsum += b;
          kept++;
        }
      }
    }
    if (stb_tindic_get(ti, tf, T)) yaps_quit("stb_tindic_get: %s\n", stb_last_error());
    if (predict && ho_n && cycles > 0)
      printf("held-out: %llu customers, log likelihood %.6f averaged over %d states, perplexity %.6f\n", (unsigned long long)ho_n,
             ho_avg, cycles, exp(-ho_avg / (double)ho_n));
    if (joint) printf("joint steps: %d of %d proposals accepted, last a=%.4f b=%.3f\n", accepted, steps, a, b);
    for (j = 0, g = 0; j < J; j++)
      for (i = 0; i < DISHES; i++, g++) t[j][i] = tf[g];
    if (dishes || seatdev) { /* the customers moved: n comes back too */
      unsigned long long moved = 0;
      if (stb_tindic_get_state(ti, nf, cust)) yaps_quit("stb_tindic_get_state: %s\n", stb_last_error());
      for (j = 0, g = 0; j < J; j++)
        for (i = 0; i < DISHES; i++, g++) {
          n[j][i] = nf[g];
          if (nf[g] >= maxn) maxn = nf[g] + 1;
        }
      for (cc = 0; cc < (size_t)J * ncust; cc++) moved += cust[cc] != (scnt_int)dish_of[cc];
      if (dishes)
        printf("dish sweeps: %llu of %llu customers ended at another dish, %llu visits found none\n", moved,
               (unsigned long long)J * ncust, stuck);
    }
    stb_groups_free(gs);
    stb_tindic_free(ti);
    if (tu) stb_tindic_free(tu);
    free(ulik), free(uh);
    free(hflat);
    free(nf);
    free(tf);
    free(hf);
    free(cust);
    free(bsort);
  }
  for (it = 0; it < cycles && !ondev; it++) {
    for (j = 0; j < J; j++) {
      int cst;
      for (cst = 0; cst < ncust; cst++) {
        i = dish_of[(size_t)j * ncust + cst];
        unsigned nn = n[j][i];
        if (nn == 1) continue; /* a single customer always opens the table */
        /* remove this customer's indicator: it heads a table with probability (t-1)/(n-1) */
        if (t[j][i] > 1 && (nn - 1) * rng_unit(0) < (double)(t[j][i] - 1)) {
          t[j][i]--;
          T[j]--;
        }
        /* odds of opening a table: H (b + a T) t/(n-t+1) V^n_{t+1}, V from the ratio table */
        double odds = (1.0 / DISHES) * (b + T[j] * a) * t[j][i] / (nn - t[j][i] + 1.0) * S_V(S, nn, t[j][i] + 1);
        if (rng_unit(0) < odds / (odds + 1.0)) {
          t[j][i]++;
          T[j]++;
        }
      }
    }
    if (it % 3 == 2) {
      b = sampleb(b, J, 1.1, 20.0, N, T, a, 0, 1, 0);
      for (j = 0; j < J; j++) bvec[j] = b;
      a = samplea(a, J, K, T, n, t, NULL, bvec, 0, 1, 0);
      if (S_remake(S, a)) yaps_quit("S_remake failed\n");
      if (it >= cycles / 2) {
        asum += a;
        bsum += b;
        kept++;
      }
    }
  }
  printf("posterior means after %d sweeps: a=%.3f b=%.2f; tables:", cycles, kept ? asum / kept : a, kept ? bsum / kept : b);
  for (j = 0; j < J; j++) printf(" %u", T[j]);
  printf("\n");

  /* ---- 4. batched grid evaluation of the discount posterior ---- */
  if (grid > 1 && grid <= 64) {
    size_t G = (size_t)J * DISHES, g = 0;
    scnt_int *nf = malloc(sizeof(*nf) * G);
    stcnt_int *tf = malloc(sizeof(*tf) * G);
    unsigned mt = 1;
    double x[64], lp[64];
    int d, best = 0;
    for (j = 0; j < J; j++)
      for (i = 0; i < DISHES; i++, g++) {
        nf[g] = n[j][i];
        tf[g] = t[j][i];
        if (tf[g] >= mt) mt = tf[g] + 1;
      }
    unsigned M = mt < 10 ? 10 : mt, Nb = maxn < M ? M : maxn;
    stb_groups_t *gs = stb_groups_create(J, K, T, nf, tf, bvec, Nb, M, grid);
    if (!gs) yaps_quit("stb_groups_create: %s\n", stb_last_error());
    for (d = 0; d < grid; d++) x[d] = 0.02 + 0.95 * (d + 0.5) / grid;
    if (stb_groups_aterms(gs, x, grid, lp)) yaps_quit("grid evaluation: %s\n", stb_last_error());
    for (d = 1; d < grid; d++)
      if (lp[d] > lp[best]) best = d;
    printf("grid of %d discounts in one batched call: posterior mode at a=%.3f (log-posterior %.3f)\n", grid,
           x[best], lp[best]);
    stb_groups_free(gs);
    /* ---- 5. the same grid, a contiguous block of it per group set, the sets spread over the GPUs ---- */
    if (nsets >= 1 && nsets <= 8 && nsets <= grid) {
      const int ndev = stb_device_count(), home = stb_get_device();
      stb_groups_t *set[8];
      double lp2[64];
      int lo[9], s, worst = 0;
      for (s = 0; s <= nsets; s++) lo[s] = (int)((long)grid * s / nsets);
      for (s = 0; s < nsets; s++) {
        if (stb_set_device(s % (ndev > 0 ? ndev : 1))) yaps_quit("stb_set_device: %s\n", stb_last_error());
        set[s] = stb_groups_create(J, K, T, nf, tf, bvec, Nb, M, lo[s + 1] - lo[s]); /* (lives on that GPU from now on) */
        if (!set[s]) yaps_quit("stb_groups_create: %s\n", stb_last_error());
      }
      stb_set_device(home);
      /* one call: contiguous blocks of the grid queued on every set, then all waited for -- the GPUs (or the sets of one
         GPU) work side by side (what it does inside: stb_groups_aterms_async on each, then stb_groups_wait on each) */
      if (stb_groups_aterms_multi(set, nsets, x, grid, lp2)) yaps_quit("grid evaluation: %s\n", stb_last_error());
      for (d = 0; d < grid; d++) {
        const double err = fabs(lp2[d] - lp[d]) / (fabs(lp[d]) > 1 ? fabs(lp[d]) : 1);
        if (err > 1e-12) worst++;
      }
      best = 0;
      for (d = 1; d < grid; d++)
        if (lp2[d] > lp2[best]) best = d;
      printf("the same grid over %d group sets on %d GPU(s), one host thread: posterior mode at a=%.3f (log-posterior %.3f), %d of %d values differ from the single call by more than 1e-12\n",
             nsets, ndev < nsets ? ndev : nsets, x[best], lp2[best], worst, grid);
      for (s = 0; s < nsets; s++) stb_groups_free(set[s]);
    }
    free(nf);
    free(tf);
  }
  if (S) S_free(S);
  return 0;
}
