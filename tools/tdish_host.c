/* tdish_host.c -- a single-core C restatement of one dish sweep (include/stb_hip.h, stb_sample_tdishes), timed by
 * tools/time_tdish.py as the host baseline: the same visit, the same uniforms, the same V cells, the same association
 * of the cumulative sums, so its draws can be compared with the device's.  A and B are kept per pair and evaluated
 * again for the dish left and the dish entered only, as the kernel does; the weights and their sums are formed anew for
 * every visit (T_i changes them all).
 * The V table is the device slab's packed layout (rows n = 2 .. N, m = 2 .. min(n, M); tests/ti_oracle.py VTab). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <time.h>

#define MAXK 1024

static uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static double unit(uint64_t key, uint64_t j) {
  return (double)(mix64(key + j * 0x9E3779B97F4A7C15ull) >> 11) * (1.0 / 9007199254740992.0);
}

static uint64_t vrowoff(unsigned n, unsigned M) {
  if (n - 1 <= M) return (uint64_t)(n - 2) * (n - 1) / 2;
  return (uint64_t)(M - 1) * M / 2 + (uint64_t)(n - 1 - M) * (M - 1);
}

static double V(const double *vpk, unsigned N, unsigned M, unsigned n, unsigned m) {
  if (n > N || m < 2 || m > M || m > n) return 0.0;
  return vpk[vrowoff(n, M) + m - 2];
}

static void AB(const double *vpk, unsigned N, unsigned M, unsigned n, unsigned t, double h, double a, double *A, double *B) {
  if (n == 0) {
    *A = 0.0;
    *B = h;
    return;
  }
  const double dn = (double)n;
  const double U = t == 1 ? dn - a : (dn - (double)t * a) + 1.0 / V(vpk, N, M, n, t);
  *A = U * (double)(n - t + 1) / dn;
  const double R = t + 1 > M ? 0.0 : (t == n ? 1.0 : (dn - (double)(t + 1) * a) * V(vpk, N, M, n, t + 1) + 1.0);
  *B = h * (double)t * R / dn;
}

/* cumulative sums in the header's association: Kogge-Stone inside blocks of 64, bases in sequence; returns Z */
static double cumsum64(const double *z, unsigned K, double *cum) {
  double base = 0.0;
  for (unsigned k0 = 0; k0 < K; k0 += 64) {
    double x[64], y[64];
    for (unsigned l = 0; l < 64; l++) x[l] = k0 + l < K ? z[k0 + l] : 0.0;
    for (unsigned d = 1; d < 64; d <<= 1) {
      for (unsigned l = 0; l < 64; l++) y[l] = l >= d ? x[l] + x[l - d] : x[l];
      for (unsigned l = 0; l < 64; l++) x[l] = y[l];
    }
    for (unsigned l = 0; l < 64; l++) {
      x[l] = base + x[l];
      if (k0 + l < K) cum[k0 + l] = x[l];
    }
    base = x[63];
  }
  return base;
}

/* sweeps restaurants i0 .. i1-1 once; C = all customers of the state (u3's offset); returns the seconds it took.
 * stuck[0] receives the visits that found no dish. */
double td_host_sweep(const double *vpk, unsigned N, unsigned M, double a, const double *bpar, int i0, int i1,
                     const uint64_t *koff, const uint64_t *coff, uint32_t *cust, const uint32_t *cls, const double *lik,
                     unsigned stride, uint32_t *nv, uint16_t *tv, uint32_t *Tv, const double *hv, uint64_t C, uint64_t seed,
                     uint64_t sweep, uint64_t *stuck) {
  struct timespec t0, t1;
  static double A[MAXK], B[MAXK], z[MAXK], cum[MAXK];
  clock_gettime(CLOCK_MONOTONIC, &t0);
  const uint64_t key = mix64(seed + (sweep + 1) * 0x9E3779B97F4A7C15ull);
  uint64_t nstuck = 0;
  for (int i = i0; i < i1; i++) {
    const unsigned K = (unsigned)(koff[i + 1] - koff[i]);
    if (K > MAXK || coff[i + 1] - coff[i] > N) continue;
    uint32_t *n = nv + koff[i], T = Tv[i];
    uint16_t *t = tv + koff[i];
    const double *h = hv ? hv + koff[i] : 0;
    const double b = bpar[i];
    for (unsigned k = 0; k < K; k++) AB(vpk, N, M, n[k], t[k], h ? h[k] : 1.0, a, &A[k], &B[k]);
    for (uint64_t c = coff[i]; c < coff[i + 1]; c++) {
      const unsigned k0 = cust[c], n0 = n[k0], t0 = t[k0];
      const double A0 = A[k0], B0 = B[k0];
      const uint32_t T0 = T;
      unsigned nn = n0, tt = t0;
      if (nn >= 2) {
        if (tt > 1 && (double)(nn - 1) * unit(key, 2 * c + 1) < (double)(tt - 1)) tt--, T--;
        nn--;
      } else {
        nn = 0, tt = 0, T--;
      }
      n[k0] = nn, t[k0] = (uint16_t)tt;
      AB(vpk, N, M, nn, tt, h ? h[k0] : 1.0, a, &A[k0], &B[k0]);
      const double g = b + (double)T * a;
      const double *Lr = lik ? lik + (uint64_t)cls[c] * stride : 0;
      for (unsigned k = 0; k < K; k++) {
        const double gB = g * B[k];
        z[k] = (Lr ? Lr[k] : 1.0) * (A[k] + gB);
      }
      const double Z = cumsum64(z, K, cum);
      if (!(Z > 0.0 && isfinite(Z))) {
        n[k0] = n0, t[k0] = (uint16_t)t0, A[k0] = A0, B[k0] = B0, T = T0;
        nstuck++;
        continue;
      }
      const double thr = unit(key, 2 * C + 1 + c) * Z;
      unsigned ks = K, last = 0;
      for (unsigned k = 0; k < K; k++)
        if (z[k] > 0.0) {
          last = k;
          if (cum[k] > thr) {
            ks = k;
            break;
          }
        }
      if (ks == K) ks = last;
      nn = n[ks], tt = t[ks];
      const double hs = h ? h[ks] : 1.0;
      if (nn == 0) {
        nn = 1, tt = 1, T++;
      } else {
        nn++;
        const double odds = hs * (b + (double)T * a) * (double)tt / (double)(nn - tt) * V(vpk, N, M, nn, tt + 1);
        const double p = isinf(odds) ? 1.0 : odds / (odds + 1.0);
        if (unit(key, 2 * c + 2) < p) tt++, T++;
      }
      n[ks] = nn, t[ks] = (uint16_t)tt;
      AB(vpk, N, M, nn, tt, hs, a, &A[ks], &B[ks]);
      cust[c] = ks;
    }
    Tv[i] = T;
  }
  if (stuck) *stuck = nstuck;
  clock_gettime(CLOCK_MONOTONIC, &t1);
  return (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
}
