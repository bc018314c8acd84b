/* tcounts_host.c -- a single-core C restatement of one table-count sweep (include/stb_hip.h, stb_sample_tcounts),
 * timed by tools/time_tcounts.py as the host baseline: the same conditional, the same uniforms, glibc's log / exp.
 * The table is the device slab's packed layout (rows n = 3.., m = 2 .. min(n-1, M); tests/orc.py row_offset). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <time.h>

static uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static uint64_t rowoff(unsigned n, unsigned M) {
  if (n <= 3) return 0;
  if (n <= M + 1) {
    const uint64_t k = n - 3;
    return k * (k + 1) / 2;
  }
  return (uint64_t)(M - 1) * M / 2 + (uint64_t)(n - M - 2) * (M - 1);
}

/* sweeps restaurants i0 .. i1-1 once; returns the seconds it took (CLOCK_MONOTONIC) */
double tc_host_sweep(const double *S1, const double *tab, unsigned M, double a, const double *bpar, int i0, int i1,
                     const uint64_t *koff, const uint32_t *nv, uint16_t *tv, uint32_t *Tv, uint64_t seed, uint64_t sweep) {
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  const uint64_t key = mix64(seed + (sweep + 1) * 0x9E3779B97F4A7C15ull);
  double *lw = malloc(sizeof(double) * (M + 1));
  for (int i = i0; i < i1; i++) {
    uint32_t T = Tv[i];
    const double b = bpar[i];
    for (uint64_t g = koff[i]; g < koff[i + 1]; g++) {
      const unsigned n = nv[g], told = tv[g];
      if (n == 0) continue;
      const unsigned tmax = n < M ? n : M;
      unsigned tnew = 1;
      if (tmax >= 2) {
        const double Tm = (double)(T - told);
        const double *row = tab + rowoff(n, M);
        double L = 0.0, mx = -HUGE_VAL;
        for (unsigned tau = 1; tau <= tmax; tau++) {
          if (tau >= 2) L += log(b + (Tm + (double)(tau - 1)) * a);
          const double S = tau == n ? 0.0 : (tau == 1 ? S1[n - 1] : row[tau - 2]);
          lw[tau] = S + L;
          if (lw[tau] > mx) mx = lw[tau];
        }
        double W = 0.0;
        for (unsigned tau = 1; tau <= tmax; tau++) W += (lw[tau] = exp(lw[tau] - mx));
        const double u = (double)(mix64(key + (g + 1) * 0x9E3779B97F4A7C15ull) >> 11) * (1.0 / 9007199254740992.0);
        const double target = u * W;
        double C = 0.0;
        for (tnew = 1; tnew < tmax; tnew++)
          if ((C += lw[tnew]) > target) break;
      }
      T = T - told + tnew;
      tv[g] = (uint16_t)tnew;
    }
    Tv[i] = T;
  }
  free(lw);
  clock_gettime(CLOCK_MONOTONIC, &t1);
  return (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
}
