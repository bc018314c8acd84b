// views.h -- private: the inputs the device launches share, as small records.  A launch (stb_*_launch, stb_lj_run,
// stb_pr_predict) takes these in place of loose pointers and sizes; a raw entry point builds them once from its flat
// arguments, an object from its fields (the ti_* and tc_* makers of tindic_obj.hip and tcounts_obj.hip).  Plain structs:
// a slot with an initialiser may be left out, and a record that may be written converts to the ones that may not.
#ifndef STB_VIEWS_H
#define STB_VIEWS_H
#include <stdint.h>

// the restaurants' shape and parameters (no launch writes these): koff [I + 1]; h null: every h is 1; maxK: the largest
// K_i, a sweep's cap, where the caller knows it, else 0; G: pairs in all (koff[I]), for the launch that asks for it
struct stb_rest_view {
  double a;
  const double *bpar;
  int I;
  const uint64_t *koff;
  const double *h = nullptr;
  unsigned maxK = 0;
  uint64_t G = 0;
};

// the counts n, t per pair and T per restaurant: read only, t and T written under a fixed n, all three written
struct stb_cnts_ro { const uint32_t *n; const uint16_t *t; const uint32_t *T = nullptr; };
struct stb_cnts_tT {
  const uint32_t *n; uint16_t *t; uint32_t *T;
  operator stb_cnts_ro() const { return {n, t, T}; }
};
struct stb_cnts_rw {
  uint32_t *n; uint16_t *t; uint32_t *T;
  operator stb_cnts_tT() const { return {n, t, T}; }
  operator stb_cnts_ro() const { return {n, t, T}; }
};

// a customer list in CSR order over the restaurants: offsets [I + 1] (null: no list), classes, dishes; C: customers in
// all (off[I]), for the launch that asks for it
struct stb_cust_ro { const uint64_t *off = nullptr; const uint32_t *cls = nullptr, *cust = nullptr; uint64_t C = 0; };
struct stb_cust_rw {
  const uint64_t *off; const uint32_t *cls; uint32_t *cust; uint64_t C = 0;
  operator stb_cust_ro() const { return {off, cls, cust, C}; }
};

// a likelihood matrix, rows x stride; stb_lik_view{} is none: every L is 1
struct stb_lik_view { const double *lik = nullptr; unsigned rows = 0, stride = 0; };

// a stored table for one discount: a V slab, or an S slab with its S1 vector
struct stb_table_view { const double *tab; unsigned N, M; const double *S1 = nullptr; };

// what a draw's uniforms are keyed by
struct stb_draw_key { uint64_t seed, sweep; };

#endif
