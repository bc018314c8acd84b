/* partition_host.c -- a single-core C restatement of the exact table-size partition draw (include/stb_hip.h,
 * stb_sample_partition), timed by tools/time_partition.py as the host baseline: the same law, the same uniforms, glibc's
 * log / exp, the cumulative weights summed in l order (not the kernel's wave scan: draws can differ at near-ties only).
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

static double S_at(const double *S1, const double *tab, unsigned M, unsigned n, unsigned m) {
  if (m == n) return 0.0;
  if (m == 1) return S1[n - 1];
  return tab[rowoff(n, M) + m - 2];
}

/* pairs g0 .. g1-1 (all with 1 <= t <= min(n, M), n <= N), sizes in draw order at sizes[soff[g]], the histogram into
 * cnt; returns the seconds it took (CLOCK_MONOTONIC) */
double pt_host(const double *S1, const double *tab, unsigned M, double a, uint64_t g0, uint64_t g1, const uint32_t *nv,
               const uint16_t *tv, const uint64_t *soff, uint16_t *sizes, uint32_t *cnt, uint64_t seed, uint64_t sweep) {
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  const uint64_t key = mix64(seed + (sweep + 1) * 0x9E3779B97F4A7C15ull);
  double *C = NULL;
  size_t cap = 0;
  for (uint64_t g = g0; g < g1; g++) {
    const unsigned n = nv[g], t = tv[g];
    uint16_t *out = sizes + soff[g];
    if (n == 0 || t == n) continue;
    unsigned Nr = n;
    for (unsigned r = 0; r + 1 < t; r++) {
      const unsigned Mc = t - 1 - r, L = Nr - Mc;
      unsigned l = 1;
      if (L > 1) {
        if (L > cap) {
          cap = 2 * L;
          C = realloc(C, sizeof(double) * cap);
        }
        const double ptot = S_at(S1, tab, M, Nr, Mc + 1);
        const double u = (double)(mix64(key + (g * 65536 + r + 1) * 0x9E3779B97F4A7C15ull) >> 11) * (1.0 / 9007199254740992.0);
        double F = 0.0, W = 0.0;
        for (unsigned k = 1; k <= L; k++) {
          if (k >= 2) F += log((((double)(k - 1) - a) * (double)(Nr - k + 1)) / (double)(k - 1));
          W += exp((F + S_at(S1, tab, M, Nr - k, Mc)) - ptot);
          C[k - 1] = W;
        }
        const double target = u * W;
        for (l = 1; l < L && !(C[l - 1] > target); l++) {
        }
      }
      out[r] = (uint16_t)l;
      cnt[l]++;
      Nr -= l;
    }
    out[t - 1] = (uint16_t)Nr;
    cnt[Nr]++;
  }
  free(C);
  clock_gettime(CLOCK_MONOTONIC, &t1);
  return (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
}
