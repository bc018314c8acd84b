/* tcwin_host.c -- a single-core C restatement of one exact windowed table-count sweep (include/stb_hip.h,
 * stb_sample_tcounts_window), timed by tools/time_tcwin.py as the host baseline: the same weights on the same span, the
 * same uniforms, glibc's log / exp.  The table is the device slab's packed layout (tools/tcounts_host.c). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <time.h>

static uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static double unit(uint64_t key, uint64_t j) {
  return (double)(mix64(key + j * 0x9E3779B97F4A7C15ull) >> 11) * (1.0 / 9007199254740992.0);
}

static uint64_t rowoff(unsigned n, unsigned M) {
  if (n <= 3) return 0;
  if (n <= M + 1) {
    const uint64_t k = n - 3;
    return k * (k + 1) / 2;
  }
  return (uint64_t)(M - 1) * M / 2 + (uint64_t)(n - M - 2) * (M - 1);
}

static unsigned lo_of(unsigned x, unsigned W) { return x > W ? x - W : 1u; }
static unsigned hi_of(unsigned x, unsigned W, unsigned Mt) { return (uint64_t)x + W < Mt ? x + W : Mt; }

/* sweeps restaurants i0 .. i1-1 once (h = 1); moves[0] += proposals tau' != t, moves[1] += those accepted;
 * returns the seconds it took (CLOCK_MONOTONIC) */
double tcw_host_sweep(const double *S1, const double *tab, unsigned M, double a, const double *bpar, int i0, int i1,
                      const uint64_t *koff, const uint32_t *nv, uint16_t *tv, uint32_t *Tv, unsigned W, unsigned flags,
                      uint64_t seed, uint64_t sweep, uint64_t *moves) {
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  const uint64_t key = mix64(seed + (sweep + 1) * 0x9E3779B97F4A7C15ull);
  double *lw = malloc(sizeof(double) * (M + 2));
  for (int i = i0; i < i1; i++) {
    uint32_t T = Tv[i];
    const double b = bpar[i];
    for (uint64_t g = koff[i]; g < koff[i + 1]; g++) {
      const unsigned n = nv[g], told = tv[g];
      if (n == 0) continue;
      const unsigned Mt = n < M ? n : M;
      unsigned tnew = 1;
      if (Mt >= 2) {
        const unsigned t = told < 1 ? 1 : (told > Mt ? Mt : told);
        const unsigned slo = lo_of(lo_of(t, W), W), shi = hi_of(hi_of(t, W, Mt), W, Mt);
        const double Tm = (double)(T - told);
        const double *row = tab + rowoff(n, M);
        double L = 0.0;
        for (unsigned tau = slo; tau <= shi; tau++) {  /* log w up to a constant: the log terms summed from slo */
          if (tau > slo) L += log(b + (Tm + (double)(tau - 1)) * a);
          lw[tau] = (tau == n ? 0.0 : (tau == 1 ? S1[n - 1] : row[tau - 2])) + L;
        }
        const unsigned lo1 = lo_of(t, W), hi1 = hi_of(t, W, Mt);
        double m1 = -HUGE_VAL, Z = 0.0, C = 0.0;
        for (unsigned tau = lo1; tau <= hi1; tau++) m1 = lw[tau] > m1 ? lw[tau] : m1;
        for (unsigned tau = lo1; tau <= hi1; tau++) Z += exp(lw[tau] - m1);
        const double target = unit(key, 2 * g + 1) * Z;
        unsigned tp = hi1;
        for (unsigned tau = lo1; tau <= hi1; tau++)
          if ((C += exp(lw[tau] - m1)) > target) {
            tp = tau;
            break;
          }
        tnew = tp;
        if (tp != t && !(flags & 1)) {
          const unsigned lo2 = lo_of(t < tp ? t : tp, W), hi2 = hi_of(t < tp ? tp : t, W, Mt);
          const unsigned lop = lo_of(tp, W), hip = hi_of(tp, W, Mt);
          double m2 = -HUGE_VAL, Zt = 0.0, Zp = 0.0;
          for (unsigned tau = lo2; tau <= hi2; tau++) m2 = lw[tau] > m2 ? lw[tau] : m2;
          for (unsigned tau = lo1; tau <= hi1; tau++) Zt += exp(lw[tau] - m2);
          for (unsigned tau = lop; tau <= hip; tau++) Zp += exp(lw[tau] - m2);
          if (!(unit(key, 2 * g + 2) * Zp < Zt)) tnew = t;
        }
        if (tp != t) {
          moves[0]++;
          moves[1] += tnew == tp;
        }
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
