/* tindic_host.c -- a single-core C restatement of one table-indicator sweep (include/stb_hip.h, stb_sample_tindic),
 * timed by tools/time_tindic.py as the host baseline: the same visit, the same uniforms, the same V cells.
 * The V table is the device slab's packed layout (rows n = 2 .. N, m = 2 .. min(n, M); tests/ti_oracle.py VTab). */
#include <math.h>
#include <stdint.h>
#include <time.h>

static uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static double unit(uint64_t key, uint64_t j) {
  return (double)(mix64(key + j * 0x9E3779B97F4A7C15ull) >> 11) * (1.0 / 9007199254740992.0);
}

/* first cell of row n: sum_{r=2}^{n-1} min(r-1, M-1) */
static uint64_t vrowoff(unsigned n, unsigned M) {
  if (n - 1 <= M) return (uint64_t)(n - 2) * (n - 1) / 2;
  return (uint64_t)(M - 1) * M / 2 + (uint64_t)(n - 1 - M) * (M - 1);
}

/* sweeps restaurants i0 .. i1-1 once (cust: local pair indices, coff: customer offsets); returns the seconds it took */
double ti_host_sweep(const double *vpk, unsigned N, unsigned M, double a, const double *bpar, int i0, int i1,
                     const uint64_t *koff, const uint64_t *coff, const uint32_t *cust, const uint32_t *nv, uint16_t *tv,
                     uint32_t *Tv, const double *hv, unsigned flags, uint64_t seed, uint64_t sweep) {
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  const uint64_t key = mix64(seed + (sweep + 1) * 0x9E3779B97F4A7C15ull);
  for (int i = i0; i < i1; i++) {
    uint32_t T = Tv[i];
    const double b = bpar[i];
    for (uint64_t c = coff[i]; c < coff[i + 1]; c++) {
      const uint64_t g = koff[i] + cust[c];
      const unsigned n = nv[g];
      if (n <= 1 || n > N) continue;
      unsigned t = tv[g];
      if (t > 1 && (double)(n - 1) * unit(key, 2 * c + 1) < (double)(t - 1)) t--, T--;
      const unsigned m = t + 1;
      const double V = m > M ? 0.0 : vpk[vrowoff(n, M) + m - 2];
      const double h = hv ? hv[g] : 1.0;
      const double odds = h * (b + (double)T * a) * (double)t / (double)((flags & 1) ? n - t + 1 : n - t) * V;
      const double p = isinf(odds) ? 1.0 : odds / (odds + 1.0);
      if (unit(key, 2 * c + 2) < p) t++, T++;
      tv[g] = (uint16_t)t;
    }
    Tv[i] = T;
  }
  clock_gettime(CLOCK_MONOTONIC, &t1);
  return (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
}
