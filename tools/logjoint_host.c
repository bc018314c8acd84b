/* logjoint_host.c -- the log joint of a sampler state summed on one host core from counts read back from the device:
 * the route a caller had before stb_logjoint (tools/time_logjoint.py times it).  The table is the device's slab copied
 * to the host once (stb_layout.h's offsets); h = NULL or per pair; one concentration per restaurant. */
#include <math.h>
#include <stdint.h>
#include <time.h>

#include "../libstb_amd/csrc/stb_layout.h"

double lj_host_sum(const double *S1, const double *slab, unsigned N, unsigned M, double a, const double *bpar, int I,
                   const uint64_t *koff, const uint32_t *n, const uint16_t *t, const double *h, double *seconds) {
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  double total = 0.0;
  const double la = a > 0.0 ? log(a) : 0.0;
  for (int i = 0; i < I; i++) {
    double P = 0.0, H = 0.0;
    uint64_t Ti = 0, Ni = 0;
    for (uint64_t g = koff[i]; g < koff[i + 1]; g++) {
      const unsigned nn = n[g], tt = t[g];
      Ti += tt;
      Ni += nn;
      if (nn == 0 || nn > N || tt == 0 || tt > nn) continue;
      if (tt == nn) P += 0.0;
      else if (tt == 1) P += S1[nn - 1];
      else if (tt <= M) P += slab[stb_row_offset(nn, M) + tt - 2];
      if (h) H += (double)tt * log(h[g]);
    }
    double R = 0.0;
    if (Ni > 0) {
      const double b = bpar[i], T = (double)Ti, Nd = (double)Ni;
      R = a > 0.0 ? (T * la + (lgamma(T + b / a) - lgamma(b / a))) - (lgamma(b + Nd) - lgamma(b))
                  : T * log(b) - (lgamma(b + Nd) - lgamma(b));
    }
    total += (P + H) + R;
  }
  clock_gettime(CLOCK_MONOTONIC, &t1);
  *seconds = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
  return total;
}
