/*
 * stable_host.c -- host side of the Stirling-table object behind include/stable.h.
 *
 * Mirrors the reference's lib/stable.c interface (S_make :110, S_remake :549, S_extend :564,
 * S_S1 :822, S_U :875, S_UV :885, S_V :900, S_S :941, S_free :980, S_report :1025,
 * S_asympt :1057) but not its construction: tables are filled on the GPU (stb_fill_S / stb_fill_V
 * in fill.hip) into one slab per table; a pinned host mirror with the same layout is copied from it
 * on demand, 128 rows at a time, and the row pointers S[n-3], V[n-2] of the public struct point into
 * that mirror, so an accessor is a flag test and the reference's two loads.  Growth recomputes the whole table for the new bounds (the
 * result equals the reference's incremental extension) under the reference's integer
 * growth policy.  There is no CPU fill anywhere in this file.
 *
 * Deliberate deviations from reference behaviour (each is a reference defect):
 *  - S_S1 beyond usedN returns the value for the n that was asked for (lib/stable.c:845-871
 *    overwrites n with the grown size first) and never returns holding the mutex (:842-844).
 *  - usedN1 is kept >= usedN after growth (lib/stable.c:809 passes the stale value, after which
 *    :856-857 would zero valid S1 entries).
 *  - S_make with neither table flag frees the struct it allocated (:131-132 leaks it).
 *  - m < 2 in S_V returns 0 instead of indexing before the row.
 *  - when one growth step is capped short of the requested column (new usedM <= old usedN,
 *    lib/stable.c:626-628) the reference reads past the end of the row; here growth repeats until
 *    the request is covered, so usedM can end up larger than the reference's in that case only.
 *  - S_FLOAT: the SfrontN/SfrontM/VfrontN/VfrontM double frontiers stay NULL; they exist in the
 *    reference only so that incremental extension loses no precision (lib/stable.c:389-449), and
 *    growth here recomputes from scratch in double.
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define H_THREADS /* as the reference's lib/Makefile:7: the library always carries the mutex */
#include "../../include/stable.h"
#include "../../include/stb_hip.h"
#include "../../include/yaps.h"
#include "stb_layout.h"

/*
 * Host mirror.  The device slab is the table; the host mirror is filled LAZILY, in blocks of
 * STB_MIRROR_ROWS table rows, the first time an accessor touches a row of the block (one D2H copy
 * of the block's contiguous slab range).  S_make / S_remake / growth therefore cost the device
 * fill only -- a caller that reads a few rows of a 10^4 x 10^4 table does not pay for 400 MB over
 * PCIe -- and the reference's own accessors S_S / S_V / S_U / S_UV see exactly the values a full
 * copy would give them.  STB_MIRROR=eager (environment) copies everything at build time, which is
 * what a caller that reads sp->S[n][m] directly (no in-tree caller does) needs; stb_table_sync()
 * does the same on demand.
 *
 * One generation of mirror (slabs, row-pointer vectors, valid flags) is one object, published by a
 * single pointer store AFTER it is complete and BEFORE the bounds that admit readers to it
 * (lib/stable.c:539-545 publishes bounds last for the same reason).  Under S_THREADS growth makes a
 * new generation and parks the old one (a reader may still hold its pointer: lib/stable.c:56-81
 * allocate-copy-swap); the last two are kept, older ones are freed.
 */
#define STB_MIRROR_ROWS 128u
/*
 * Look-ahead (round 6).  A caller that goes through the table -- the reference's Gibbs sweep reads S_V for every customer
 * after every S_remake (test/demo.c:405-445, :487) -- used to stop at every block for a synchronous copy: 78 stops and
 * 400 MB for a table of 10^4 x 10^4.  Now a miss copies its own block and, behind it on a stream of the table's own, a RUN
 * of the blocks that follow (at least STB_MIRROR_AHEAD_MB, default 16 MB; two runs under way at most); the accessor waits
 * for the block it touched only, and finds the following ones there -- or waits for their run's event, which is under way
 * already -- while the caller computes.  A caller that reads a few rows pays for one run per touched region at most, none
 * of it waited for.  Runs are drained before the device slabs are written again (S_remake, growth) or freed.
 */
#define STB_MIRROR_RUNS 3

typedef struct mirror {
  void *slabS, *slabV;               /* pinned (or malloc'd) host slabs, device layout */
  int pinS, pinV;
  void **rowsS, **rowsV;             /* row-pointer vectors: what sp->S / sp->V (or Sf / Vf) point to */
  volatile unsigned char *validS, *validV; /* one flag per block of STB_MIRROR_ROWS rows */
  unsigned N, M;                     /* bounds this generation describes */
  unsigned nvalidS, nvalidV;         /* blocks that are there (counted under the table's lock) */
  uint64_t elemsS, elemsV, bytes;
  struct mirror *next;               /* retired list */
} mirror;

typedef struct s1_gen {
  double *p;
  struct s1_gen *next;
} s1_gen;

typedef struct stb_impl {
  /* device */
  int dev; /* the GPU the table lives on (stb_get_device() at S_make time) */
  double *d_S, *d_V, *d_S1;
  float *d_Sf, *d_Vf; /* S_FLOAT: narrowed copies of the double slabs, same element offsets */
  void *d_ws;
  size_t ws_bytes;
  uint64_t d_S_elems, d_V_elems, d_S1_elems, d_Sf_elems, d_Vf_elems;
  struct s1_gen *retired_s1; /* S1 vectors replaced by growth while readers may hold them (S_THREADS) */
  mirror *cur;      /* current generation (readers load it once per access) */
  mirror *retired;  /* older generations a reader may still hold, newest first */
  int eager;        /* STB_MIRROR=eager */
  /* look-ahead copies (round 6): blocks behind the one an accessor missed, under way on a stream of the table's own */
  void *cp_stream;
  struct cp_run {
    int live, which;      /* which: 0 the S slab, 1 the V slab */
    unsigned b0, b1;      /* blocks b0 .. b1 of the current generation */
    void *ev;
  } runs[STB_MIRROR_RUNS];
  uint64_t ahead_bytes;   /* how far ahead a run reaches at least (STB_MIRROR_AHEAD_MB, default 16; 0: no look-ahead) */
  /* every block of the current generation's S / V mirror is there: the accessors' short way (two loads, as the
   * reference's; tables without S_THREADS and S_FLOAT) */
  volatile int fullS, fullV;
  uint64_t bytes_host, bytes_dev;
} stb_impl;

static void account(stable_t *sp) {
  stb_impl *im = sp->impl;
  uint64_t tot = im->bytes_host + im->bytes_dev;
  mirror *g;
  if (im->cur) tot += im->cur->bytes;
  for (g = im->retired; g; g = g->next) tot += g->bytes;
  sp->memalloced = tot > 0xffffffffull ? 0xffffffffu : (uint32_t)tot;
}

void stb_table_bytes(stable_t *sp, unsigned long long *device_bytes, unsigned long long *host_bytes) {
  unsigned long long dv = 0, hs = 0;
  if (sp && sp->impl) {
    const stb_impl *im = sp->impl;
    const mirror *g;
    dv = im->bytes_dev;
    hs = im->bytes_host;
    if (im->cur) hs += im->cur->bytes;
    for (g = im->retired; g; g = g->next) hs += g->bytes;
  }
  if (device_bytes) *device_bytes = dv;
  if (host_bytes) *host_bytes = hs;
}

static void lock(stable_t *sp) {
  if (sp->flags & S_THREADS) pthread_mutex_lock(&sp->mutex);
}
static void unlock(stable_t *sp) {
  if (sp->flags & S_THREADS) pthread_mutex_unlock(&sp->mutex);
}

/* the mirror's memory: pinned and on 2 MB pages (2: aligned_alloc + madvise + hipHostRegister; from 8 MB on), pinned (1:
 * hipHostMalloc; STB_MIRROR_PAGES=small asks for it), or plain (0: copies are then staged by the runtime).  A caller's
 * look-ups are random reads over the whole slab: 10^6 of them over 400 MB take 14.3 ms on 2 MB pages on every box measured;
 * on hipHostMalloc's memory 14.3 on one box and 20-22 on another (whether the runtime's allocation happens to sit on huge
 * pages is the box's state, not ours). */
static void *host_slab(size_t bytes, int *pinned) {
  const char *pg = getenv("STB_MIRROR_PAGES");
  void *p = NULL;
  if (bytes >= ((size_t)8 << 20) && !(pg && strcmp(pg, "small") == 0)) {
    p = stb_host_malloc_huge(bytes);
    *pinned = 2;
  }
  if (!p) {
    p = stb_host_malloc(bytes);
    *pinned = p != NULL;
  }
  if (!p) p = malloc(bytes ? bytes : 1);
  return p;
}
static void host_slab_free(void *p, int pinned) {
  if (!p) return;
  if (pinned == 2)
    stb_host_free_huge(p);
  else if (pinned)
    stb_host_free(p);
  else
    free(p);
}

/* an S1 vector that growth replaced: freed at once, or parked while concurrent readers may hold it */
static void retire_s1(stable_t *sp, double *old) {
  stb_impl *im = sp->impl;
  if (sp->flags & S_THREADS) {
    s1_gen *g = malloc(sizeof(*g));
    if (g) {
      g->p = old;
      g->next = im->retired_s1;
      im->retired_s1 = g;
      return;
    }
  }
  free(old);
}

/* bytes per stored table value: the reference's S_FLOAT keeps tables as float (lib/stable.h:31-33) */
static size_t esz(const stable_t *sp) { return (sp->flags & S_FLOAT) ? sizeof(float) : sizeof(double); }

static void mirror_free(mirror *m) {
  if (!m) return;
  host_slab_free(m->slabS, m->pinS);
  host_slab_free(m->slabV, m->pinV);
  free(m->rowsS);
  free(m->rowsV);
  free((void *)m->validS);
  free((void *)m->validV);
  free(m);
}

/* a complete, all-invalid generation for bounds (N,M); NULL when out of memory */
static mirror *mirror_new(const stable_t *sp, unsigned N, unsigned M) {
  mirror *m = calloc(1, sizeof(*m));
  unsigned n;
  if (!m) return NULL;
  m->N = N;
  m->M = M;
  if (sp->flags & S_STABLE) {
    uint64_t el = stb_table_elems(N, M);
    const unsigned nb = (N >= 3 ? N - 3 : 0) / STB_MIRROR_ROWS + 1;
    if (el < 2) el = 2;
    m->elemsS = el;
    m->slabS = host_slab(esz(sp) * el, &m->pinS);
    m->rowsS = malloc(sizeof(void *) * (N > 3 ? N : 3));
    m->validS = calloc(nb, 1);
    if (!m->slabS || !m->rowsS || !m->validS) goto fail;
    for (n = 3; n <= N; n++) m->rowsS[n - 3] = (char *)m->slabS + esz(sp) * stb_row_offset(n, M);
    m->bytes += esz(sp) * el + sizeof(void *) * N + nb;
  }
  if (sp->flags & S_UVTABLE) {
    uint64_t el = stb_vtable_elems(N, M);
    const unsigned nb = (N >= 2 ? N - 2 : 0) / STB_MIRROR_ROWS + 1;
    if (el < 2) el = 2;
    m->elemsV = el;
    m->slabV = host_slab(esz(sp) * el, &m->pinV);
    m->rowsV = malloc(sizeof(void *) * (N > 2 ? N : 2));
    m->validV = calloc(nb, 1);
    if (!m->slabV || !m->rowsV || !m->validV) goto fail;
    for (n = 2; n <= N; n++) m->rowsV[n - 2] = (char *)m->slabV + esz(sp) * stb_vrow_offset(n, M);
    m->bytes += esz(sp) * el + sizeof(void *) * N + nb;
  }
  return m;
fail:
  mirror_free(m);
  return NULL;
}

static void mirror_invalidate(const stable_t *sp, mirror *m) {
  stb_impl *im = sp->impl;
  __atomic_store_n(&im->fullS, 0, __ATOMIC_RELEASE);
  __atomic_store_n(&im->fullV, 0, __ATOMIC_RELEASE);
  m->nvalidS = m->nvalidV = 0;
  if (m->validS) memset((void *)m->validS, 0, (m->N >= 3 ? m->N - 3 : 0) / STB_MIRROR_ROWS + 1);
  if (m->validV) memset((void *)m->validV, 0, (m->N >= 2 ? m->N - 2 : 0) / STB_MIRROR_ROWS + 1);
}

/* byte range of blocks b0 .. b1 of the S (which = 0) or V (which = 1) slab of generation m */
static void block_range(const stable_t *sp, const mirror *m, int which, unsigned b0, unsigned b1, uint64_t *o0, uint64_t *o1) {
  const unsigned first = (which ? 2u : 3u) + b0 * STB_MIRROR_ROWS;
  unsigned last = (which ? 2u : 3u) + b1 * STB_MIRROR_ROWS + STB_MIRROR_ROWS - 1;
  if (last > m->N) last = m->N;
  if (which) {
    *o0 = esz(sp) * stb_vrow_offset(first, m->M);
    *o1 = esz(sp) * stb_vrow_offset(last + 1, m->M);
  } else {
    *o0 = esz(sp) * stb_row_offset(first, m->M);
    *o1 = esz(sp) * stb_row_offset(last + 1, m->M);
  }
}
static unsigned n_blocks(const mirror *m, int which) { return (m->N >= (which ? 2u : 3u) ? m->N - (which ? 2u : 3u) : 0) / STB_MIRROR_ROWS + 1; }

/* queue the copy of blocks b0 .. b1 on `stream` (NULL: the null stream) */
static int copy_blocks(stable_t *sp, mirror *m, int which, unsigned b0, unsigned b1, void *stream) {
  stb_impl *im = sp->impl;
  uint64_t o0, o1;
  const char *src = which ? ((sp->flags & S_FLOAT) ? (const char *)im->d_Vf : (const char *)im->d_V)
                          : ((sp->flags & S_FLOAT) ? (const char *)im->d_Sf : (const char *)im->d_S);
  char *dst = which ? m->slabV : m->slabS;
  block_range(sp, m, which, b0, b1, &o0, &o1);
  return stb_memcpy_d2h(dst + o0, src + o0, o1 - o0, stream);
}
static void mark_valid(stb_impl *im, mirror *m, int which, unsigned b0, unsigned b1) {
  unsigned b;
  for (b = b0; b <= b1; b++) {
    volatile unsigned char *v = which ? &m->validV[b] : &m->validS[b];
    if (!*v) {
      __atomic_store_n(v, 1, __ATOMIC_RELEASE);
      if (which) m->nvalidV++; else m->nvalidS++;
    }
  }
  if (m == im->cur) {
    if (which ? m->nvalidV == n_blocks(m, 1) : m->nvalidS == n_blocks(m, 0))
      __atomic_store_n(which ? &im->fullV : &im->fullS, 1, __ATOMIC_RELEASE);
  }
}

/* copy block b of the S (which = 0) or V (which = 1) table of generation m from the device, now;
 * the caller holds the table's lock (when it has one) and has made the table's device current */
static int mirror_fetch_locked(stable_t *sp, mirror *m, int which, unsigned b) {
  if (copy_blocks(sp, m, which, b, b, NULL)) return 1;
  if (stb_stream_sync(NULL)) return 1;
  mark_valid(sp->impl, m, which, b, b);
  return 0;
}

/* every look-ahead copy under way is waited for (their blocks are NOT marked: the caller is about to write the device slabs
 * again, or to free them); the table's device is current */
static void drain_runs(stb_impl *im) {
  int r;
  for (r = 0; r < STB_MIRROR_RUNS; r++)
    if (im->runs[r].live) {
      (void)stb_event_wait(im->runs[r].ev);
      im->runs[r].live = 0;
    }
}

/* runs that have arrived: their blocks are there */
static void retire_runs(stb_impl *im, mirror *m) {
  int r;
  for (r = 0; r < STB_MIRROR_RUNS; r++)
    if (im->runs[r].live && stb_event_done(im->runs[r].ev) != 0) {
      mark_valid(im, m, im->runs[r].which, im->runs[r].b0, im->runs[r].b1);
      im->runs[r].live = 0;
    }
}

/* Queue a run on the copy stream: the blocks from `from` on that are neither there nor under way -- `one`: that block
 * alone; otherwise at least ahead_bytes of them.  Returns the slot (-1: nothing was queued: no free slot, nothing to copy,
 * an error) and, through `behind`, the block after the run's last. */
static int queue_run(stable_t *sp, mirror *m, int which, unsigned from, int one, unsigned *behind) {
  stb_impl *im = sp->impl;
  const unsigned nb = n_blocks(m, which);
  volatile unsigned char *valid = which ? m->validV : m->validS;
  int r, slot = -1;
  unsigned b1;
  uint64_t o0, o1;
  if (behind) *behind = from;
  if (from >= nb || valid[from]) return -1;
  for (r = 0; r < STB_MIRROR_RUNS; r++) {
    if (!im->runs[r].live) {
      if (slot < 0) slot = r;
    } else if (im->runs[r].which == which && from >= im->runs[r].b0 && from <= im->runs[r].b1) {
      return -1; /* under way already */
    }
  }
  if (slot < 0) return -1;
  if (!im->cp_stream && !(im->cp_stream = stb_stream_create())) return -1;
  if (!im->runs[slot].ev && !(im->runs[slot].ev = stb_event_create())) return -1;
  for (b1 = from; !one; b1++) {
    int stop = b1 + 1 >= nb || valid[b1 + 1] || b1 - from >= 63;
    for (r = 0; r < STB_MIRROR_RUNS && !stop; r++)
      if (im->runs[r].live && im->runs[r].which == which && b1 + 1 >= im->runs[r].b0 && b1 + 1 <= im->runs[r].b1) stop = 1;
    block_range(sp, m, which, from, b1, &o0, &o1);
    if (stop || o1 - o0 >= im->ahead_bytes) break;
  }
  if (copy_blocks(sp, m, which, from, b1, im->cp_stream) || stb_event_record(im->runs[slot].ev, im->cp_stream)) return -1;
  im->runs[slot].live = 1;
  im->runs[slot].which = which;
  im->runs[slot].b0 = from;
  im->runs[slot].b1 = b1;
  if (behind) *behind = b1 + 1;
  return slot;
}

/* block b of generation m is wanted and not there (the lock is held, the table's device current) */
static int mirror_miss_locked(stable_t *sp, mirror *m, int which, unsigned b) {
  stb_impl *im = sp->impl;
  volatile unsigned char *valid = which ? m->validV : m->validS;
  int r, mine = -1, live = 0;
  unsigned far = b + 1;
  if (!im->ahead_bytes || (which ? !m->pinV : !m->pinS)) return mirror_fetch_locked(sp, m, which, b); /* (pageable mirror: nothing to overlap) */
  retire_runs(im, m);
  if (valid[b]) return 0;
  for (r = 0; r < STB_MIRROR_RUNS; r++)
    if (im->runs[r].live && im->runs[r].which == which && b >= im->runs[r].b0 && b <= im->runs[r].b1) mine = r; /* on its way */
  if (mine < 0) {
    /* nobody has asked for it: the block alone first -- what the caller waits for -- and the runs behind it */
    mine = queue_run(sp, m, which, b, 1, NULL);
    if (mine < 0) return mirror_fetch_locked(sp, m, which, b);
  }
  /* two runs under way behind the block the caller is at, queued BEFORE the wait: they travel while the caller works */
  for (r = 0; r < STB_MIRROR_RUNS; r++)
    if (r != mine && im->runs[r].live && im->runs[r].which == which) {
      live++;
      if (im->runs[r].b1 + 1 > far) far = im->runs[r].b1 + 1;
    }
  if (im->runs[mine].b1 + 1 > far) far = im->runs[mine].b1 + 1;
  while (live < 2) {
    unsigned behind = far;
    if (queue_run(sp, m, which, far, 0, &behind) < 0) break;
    far = behind;
    live++;
  }
  if (stb_event_wait(im->runs[mine].ev)) return 1;
  mark_valid(im, m, im->runs[mine].which, im->runs[mine].b0, im->runs[mine].b1);
  im->runs[mine].live = 0;
  return 0;
}

/* make sure row n of the S / V table is in the host mirror; returns the generation to read from,
 * NULL on a device error */
static mirror *mirror_row(stable_t *sp, int which, unsigned n) {
  stb_impl *im = sp->impl;
  mirror *m = __atomic_load_n(&im->cur, __ATOMIC_ACQUIRE);
  const unsigned b = (n - (which ? 2u : 3u)) / STB_MIRROR_ROWS;
  volatile unsigned char *valid = which ? m->validV : m->validS;
  if (__atomic_load_n(&valid[b], __ATOMIC_ACQUIRE)) return m;
  {
    int rc = 0, prev_dev;
    lock(sp);
    m = im->cur; /* growth may have swapped generations while we waited */
    valid = which ? m->validV : m->validS;
    if (!valid[b]) {
      prev_dev = stb_device_enter(im->dev);
      rc = mirror_miss_locked(sp, m, which, b);
      stb_device_leave(prev_dev);
    }
    unlock(sp);
    if (rc) {
      yaps_message("libstb_amd: copying table rows from the device failed: %s\n", stb_last_error());
      return NULL;
    }
  }
  return m;
}

/* the whole mirror, now (STB_MIRROR=eager, stb_table_sync) */
static int mirror_all_locked(stable_t *sp, mirror *m) {
  unsigned b;
  if (sp->flags & S_STABLE)
    for (b = 0; b <= (m->N >= 3 ? m->N - 3 : 0) / STB_MIRROR_ROWS; b++)
      if (!m->validS[b] && 3 + b * STB_MIRROR_ROWS <= m->N && mirror_fetch_locked(sp, m, 0, b)) return 1;
  if (sp->flags & S_UVTABLE)
    for (b = 0; b <= (m->N >= 2 ? m->N - 2 : 0) / STB_MIRROR_ROWS; b++)
      if (!m->validV[b] && 2 + b * STB_MIRROR_ROWS <= m->N && mirror_fetch_locked(sp, m, 1, b)) return 1;
  return 0;
}

int stb_table_sync(stable_t *sp) {
  stb_impl *im;
  int rc, prev_dev;
  if (!sp || !sp->impl) return 1;
  im = sp->impl;
  lock(sp);
  prev_dev = stb_device_enter(im->dev);
  rc = mirror_all_locked(sp, im->cur);
  stb_device_leave(prev_dev);
  unlock(sp);
  return rc;
}

/* out[g] = S_S (which = 0) or S_V (which = 1) of (n[g], m[g]), g = 0 .. G-1: the accessors in a loop, for callers (and
 * benchmarks) that come through a foreign-function interface one call at a time otherwise */
void stb_table_probe(stable_t *sp, int which, const unsigned *n, const unsigned *m, size_t G, double *out) {
  size_t g;
  if (which)
    for (g = 0; g < G; g++) out[g] = S_V(sp, n[g], m[g]);
  else
    for (g = 0; g < G; g++) out[g] = S_S(sp, n[g], m[g]);
}

void stb_table_mirrored(stable_t *sp, unsigned *s_blocks, unsigned *v_blocks) {
  unsigned b, ns = 0, nv = 0;
  if (sp && sp->impl) {
    const mirror *m = ((stb_impl *)sp->impl)->cur;
    if (m->validS)
      for (b = 0; b <= (m->N >= 3 ? m->N - 3 : 0) / STB_MIRROR_ROWS; b++) ns += m->validS[b];
    if (m->validV)
      for (b = 0; b <= (m->N >= 2 ? m->N - 2 : 0) / STB_MIRROR_ROWS; b++) nv += m->validV[b];
  }
  if (s_blocks) *s_blocks = ns;
  if (v_blocks) *v_blocks = nv;
}

static int devf_grow(stb_impl *im, float **slot, uint64_t *have, uint64_t want) {
  if (want <= *have) return 0;
  stb_device_free(*slot);
  im->bytes_dev -= *have * sizeof(float);
  *have = 0;
  *slot = stb_device_malloc(sizeof(float) * want);
  if (!*slot) return 1;
  *have = want;
  im->bytes_dev += want * sizeof(float);
  return 0;
}

static int dev_grow(stb_impl *im, double **slot, uint64_t *have, uint64_t want) {
  if (want <= *have) return 0;
  stb_device_free(*slot);
  im->bytes_dev -= *have * sizeof(double);
  *have = 0;
  *slot = stb_device_malloc(sizeof(double) * want);
  if (!*slot) return 1;
  *have = want;
  im->bytes_dev += want * sizeof(double);
  return 0;
}

/* S_FLOAT tables are written once, as floats, wherever the fill that narrows before the store applies (the
 * halo-block form: stb_fill_takes_kind); the double slab then does not exist at all -- half the device memory of a
 * double table, as the reference's S_FLOAT has half the host memory (lib/stable.h:80-90).  STB_FLOAT_NARROW=1 keeps the
 * old way: a double slab, narrowed by a second pass. */
static int float_direct(const stable_t *sp, unsigned N, unsigned M, int vtable) {
  const char *e = getenv("STB_FLOAT_NARROW");
  if (!(sp->flags & S_FLOAT) || (e && *e && strcmp(e, "0") != 0)) return 0;
  return stb_fill_takes_kind(N, M, 1, vtable ? 3 : 1);
}

/* size the device slabs and scratch for bounds (N,M) */
static int provision(stable_t *sp, unsigned N, unsigned M) {
  stb_impl *im = sp->impl;
  size_t ws = stb_fill_workspace_bytes(N, M, 1);
  if (ws > im->ws_bytes) {
    stb_device_free(im->d_ws);
    im->bytes_dev -= im->ws_bytes;
    im->ws_bytes = 0;
    im->d_ws = stb_device_malloc(ws);
    if (!im->d_ws) return 1;
    im->ws_bytes = ws;
    im->bytes_dev += ws;
  }
  if (dev_grow(im, &im->d_S1, &im->d_S1_elems, N)) return 1;
  if (sp->flags & S_STABLE) {
    uint64_t el = stb_table_elems(N, M);
    if (el < 2) el = 2;
    if (!float_direct(sp, N, M, 0) && dev_grow(im, &im->d_S, &im->d_S_elems, el)) return 1;
    if ((sp->flags & S_FLOAT) && devf_grow(im, &im->d_Sf, &im->d_Sf_elems, el)) return 1;
  }
  if (sp->flags & S_UVTABLE) {
    uint64_t el = stb_vtable_elems(N, M);
    if (el < 2) el = 2;
    if (!(sp->flags & S_STABLE) && dev_grow(im, &im->d_S, &im->d_S_elems, stb_table_elems(N, 2) + 2))
      return 1; /* scratch for the S1-only fill */
    if (!float_direct(sp, N, M, 1) && dev_grow(im, &im->d_V, &im->d_V_elems, el)) return 1;
    if ((sp->flags & S_FLOAT) && devf_grow(im, &im->d_Vf, &im->d_Vf_elems, el)) return 1;
  }
  return 0;
}

/* device fill for discount a at bounds (N,M); S1[0..N) refreshed on the host; nothing else is copied */
static int build(stable_t *sp, double a, unsigned N, unsigned M) {
  stb_impl *im = sp->impl;
  if (sp->flags & S_STABLE) {
    int done = 0;
    if (float_direct(sp, N, M, 0))
      /* all arithmetic in double (as lib/stable.c:389-449 does through its frontier vectors), the stored value
       * narrowed by the kernel that computed it: one pass, no double slab.  A fill that gave up waiting cannot be
       * repeated in this form: the old way below takes over (and only then gets its double slab). */
      done = !stb_fill_Sf(&a, 1, N, M, im->d_Sf, im->d_Sf_elems, im->d_S1, N, im->d_ws, im->ws_bytes, NULL) && !stb_fill_status();
    if (!done) {
      /* the double slab as these bounds need it: provision() sized it for the route of its own time, and the route
       * changes under a table -- the shared-GPU mode turns the direct one off, and growth past STB_HB_MIN_N turns it
       * on without a double slab for the new bounds (nothing when the slab is large enough already) */
      uint64_t el = stb_table_elems(N, M);
      if (dev_grow(im, &im->d_S, &im->d_S_elems, el < 2 ? 2 : el)) return 1;
      if (stb_fill_S(&a, 1, N, M, im->d_S, im->d_S_elems, im->d_S1, N, im->d_ws, im->ws_bytes,
                     stb_default_variant(), NULL))
        return 1;
      /* waits for the fill and, if a one-launch form gave up, repeats it in the other form: only then
       * may anything read the table (the narrowing below included) */
      if (stb_fill_status()) return 1;
      if ((sp->flags & S_FLOAT) && stb_table_to_float(im->d_S, im->d_Sf, stb_table_elems(N, M), NULL)) return 1;
    }
    if (stb_memcpy_d2h(sp->S1, im->d_S1, sizeof(double) * N, NULL)) return 1;
  }
  if (sp->flags & S_UVTABLE) {
    int done = 0;
    if (float_direct(sp, N, M, 1))
      done = !stb_fill_Vf(&a, 1, N, M, im->d_Vf, im->d_Vf_elems, im->d_ws, im->ws_bytes, NULL) && !stb_fill_status();
    if (!done) {
      uint64_t el = stb_vtable_elems(N, M); /* (sized here, as the S slab above) */
      int rc;
      if (dev_grow(im, &im->d_V, &im->d_V_elems, el < 2 ? 2 : el)) return 1;
      rc = stb_fill_V(&a, 1, N, M, im->d_V, im->d_V_elems, im->d_ws, im->ws_bytes, NULL);
      if (!rc) rc = stb_fill_status(); /* before anything reads it or a later fill reuses the workspace and its header */
      if (rc) {
        /* (the V table from the S recurrence's cells gave up waiting: the reference's own recurrence, which cannot) */
        rc = stb_fill_V_exact(&a, 1, N, M, im->d_V, im->d_V_elems, im->d_ws, im->ws_bytes, NULL);
        if (rc || stb_fill_status()) return 1;
      }
      if ((sp->flags & S_FLOAT) && stb_table_to_float(im->d_V, im->d_Vf, stb_vtable_elems(N, M), NULL)) return 1;
    }
  }
  if (!(sp->flags & S_STABLE)) {
    /* U/V-only tables still keep S1 (lib/stable.c:155, :337-348): take it from a width-2 S fill
     * on the device (N-2 cells) so that no table arithmetic runs on the host */
    if (stb_fill_S(&a, 1, N, 2, im->d_S, im->d_S_elems, im->d_S1, N, im->d_ws, im->ws_bytes,
                   stb_default_variant(), NULL))
      return 1;
    if (stb_memcpy_d2h(sp->S1, im->d_S1, sizeof(double) * N, NULL)) return 1;
    if (stb_fill_status()) return 1;
  }
  if (stb_stream_sync(NULL)) return 1;
  return 0;
}

/* make a complete generation visible: the public row-pointer vectors and the generation pointer
 * first, bounds last (lib/stable.c:539-545) */
static void publish(stable_t *sp, mirror *m) {
  stb_impl *im = sp->impl;
  mirror *old = im->cur;
  __atomic_store_n(&im->fullS, 0, __ATOMIC_RELEASE); /* (until the new generation's blocks are counted, below) */
  __atomic_store_n(&im->fullV, 0, __ATOMIC_RELEASE);
  if (sp->flags & S_FLOAT) {
    sp->Sf = (float **)m->rowsS;
    sp->Vf = (float **)m->rowsV;
  } else {
    sp->S = (double **)m->rowsS;
    sp->V = (double **)m->rowsV;
  }
  __atomic_store_n(&im->cur, m, __ATOMIC_RELEASE);
  __atomic_store_n(&sp->usedN, m->N, __ATOMIC_RELEASE);
  __atomic_store_n(&sp->usedM, m->M, __ATOMIC_RELEASE);
  if ((sp->flags & S_STABLE) && m->nvalidS == n_blocks(m, 0)) __atomic_store_n(&im->fullS, 1, __ATOMIC_RELEASE); /* (STB_MIRROR=eager) */
  if ((sp->flags & S_UVTABLE) && m->nvalidV == n_blocks(m, 1)) __atomic_store_n(&im->fullV, 1, __ATOMIC_RELEASE);
  if (old) {
    if (sp->flags & S_THREADS) {
      /* a reader may still be inside the old generation: park it; keep the last two */
      mirror *g;
      int kept = 1;
      old->next = im->retired;
      im->retired = old;
      for (g = old; g->next; g = g->next)
        if (++kept > 2) {
          mirror *dead = g->next;
          g->next = NULL;
          while (dead) {
            mirror *nx = dead->next;
            mirror_free(dead);
            dead = nx;
          }
          break;
        }
    } else {
      mirror_free(old);
    }
  }
  account(sp);
}

stable_t *S_make(unsigned initN, unsigned initM, unsigned maxN, unsigned maxM, double a,
                 uint32_t flags) {
  stable_t *sp;
  stb_impl *im;
  /* lib/stable.c:118-129, including the :126-127 assignment of maxM */
  if (maxM < 10) maxM = 10;
  if (maxN < maxM) maxN = maxM;
  if (initM < 10) initM = 10;
  if (initN < initM) initN = initM;
  if (initN > maxN) initN = maxM;
  if (initN > maxN) initN = maxN;
  if (initN < initM) initM = initN; /* the quirk above can leave initN<initM: unusable, clamp */

  if ((flags & S_STABLE) == 0 && (flags & S_UVTABLE) == 0) return NULL; /* lib/stable.c:131-132 */
  if (!(a >= 0.0 && a < 1.0)) {
    yaps_message("S_make: discount %lf outside [0,1)\n", a);
    return NULL;
  }
  if (stb_device_count() < 1) {
    yaps_message("S_make: no HIP device available; libstb_amd has no CPU table fill\n");
    return NULL;
  }
  sp = calloc(1, sizeof(*sp));
  im = calloc(1, sizeof(*im));
  if (!sp || !im) {
    free(sp);
    free(im);
    return NULL;
  }
  sp->impl = im;
  im->dev = stb_get_device();
  if (im->dev < 0 || im->dev >= stb_device_count()) {
    yaps_message("S_make: device %d does not exist (stb_set_device / STB_DEVICE)\n", im->dev);
    free(sp);
    free(im);
    return NULL;
  }
  sp->flags = flags;
  sp->maxN = maxN;
  sp->maxM = maxM;
  sp->usedN = initN;
  sp->usedM = initM;
  sp->usedN1 = initN;
  sp->startM = initM;
  if (flags & S_THREADS) pthread_mutex_init(&sp->mutex, NULL);
  sp->S1 = malloc(sizeof(double) * initN);
  if (!sp->S1) {
    S_free(sp);
    return NULL;
  }
  im->bytes_host = sizeof(*sp) + sizeof(double) * initN;
  sp->a = a;
  sp->lga = lgamma(1.0 - a); /* lib/stable.c:329 */
  {
    const char *mm = getenv("STB_MIRROR");
    mirror *m;
    const int prev_dev = stb_device_enter(im->dev);
    im->eager = mm && strcmp(mm, "eager") == 0;
    {
      /* STB_MIRROR=lazy: every miss a synchronous copy of its own block and nothing else (rounds 1-5) */
      const char *ah = getenv("STB_MIRROR_AHEAD_MB");
      const long mb = ah ? atol(ah) : 16;
      im->ahead_bytes = (mm && strcmp(mm, "lazy") == 0) || mb <= 0 ? 0 : (uint64_t)mb << 20;
    }
    m = mirror_new(sp, initN, initM);
    if (!m || provision(sp, initN, initM) || build(sp, a, initN, initM) || (im->eager && mirror_all_locked(sp, m))) {
      yaps_message("S_make: %s\n", m ? stb_last_error() : "out of host memory");
      mirror_free(m);
      stb_device_leave(prev_dev);
      S_free(sp);
      return NULL;
    }
    publish(sp, m);
    stb_device_leave(prev_dev);
  }
  if (flags & S_VERBOSE) S_report(sp, stderr);
  return sp;
}

void S_tag(stable_t *sp, char *tag) {
  /* lib/stable.c:105-108 */
  sp->tag = malloc(strlen(tag) + 1);
  if (sp->tag) strcpy(sp->tag, tag);
}

int S_remake(stable_t *sp, double a) {
  unsigned n;
  if (!sp || !sp->impl) return 1;
  if (!(a >= 0.0 && a < 1.0)) return 1;
  {
    /* same bounds, new discount: the mirror keeps its storage and is refilled on demand (nobody may
     * be reading during S_remake, as in the reference) */
    stb_impl *im = sp->impl;
    const int prev_dev = stb_device_enter(im->dev);
    int rc;
    drain_runs(im); /* (copies still under way read the slabs this fill writes) */
    mirror_invalidate(sp, im->cur);
    rc = build(sp, a, sp->usedN, sp->usedM) || (im->eager && mirror_all_locked(sp, im->cur));
    stb_device_leave(prev_dev);
    if (rc) {
      /* the table keeps its old discount; its contents are undefined until a remake succeeds */
      yaps_message("S_remake: %s\n", stb_last_error());
      return 1;
    }
  }
  sp->a = a;
  sp->lga = lgamma(1.0 - a); /* lib/stable.c:328-329 */
  /* the discount changed, so lazily cached S1 entries past usedN are void (lib/stable.c:350-353) */
  for (n = sp->usedN; n < sp->usedN1; n++) sp->S1[n] = 0;
  if (sp->flags & S_VERBOSE) S_report(sp, stderr);
  return 0;
}

/* lib/stable.c:564-630: the growth policy, integers only (kept separate so it can be unit-tested
 * without a device; exported for that purpose) */
void stb_extend_policy(unsigned usedN, unsigned usedM, unsigned maxN, unsigned maxM, int N, int M,
                       unsigned *newN, unsigned *newM) {
  unsigned n, m;
  N++;
  M++;
  if ((unsigned)N < usedN && (unsigned)M < usedM) {
    *newN = usedN;
    *newM = usedM;
    return;
  }
  n = (unsigned)N;
  if (n < usedN) n = usedN;
  if (n > maxN) n = maxN;
  if (n > usedN) {
    /* at least 10 % and at least 50 more rows; the 1.1 product truncates like the reference's
     * int = double assignment */
    if ((double)n < usedN * 1.1) n = (unsigned)(usedN * 1.1);
    if (n < usedN + 50) n = usedN + 50;
    if (n > maxN) n = maxN;
  }
  m = (unsigned)M;
  if (m < usedM) m = usedM;
  if (n < m) m = n;
  if (m > maxM) m = maxM;
  if (m > usedM) {
    if ((double)m < usedM * 1.1) m = (unsigned)(usedM * 1.1);
    if (m < usedM + 50) m = usedM + 50;
    if (m > maxM) m = maxM;
    if (m > usedN) m = usedN;
  }
  *newN = n;
  *newM = m;
}

/* grow to cover (N,M) as requested by an accessor; non-zero on allocation/device failure */
static int extend(stable_t *sp, int N, int M) {
  unsigned newN, newM;
  int rc = 0;
  lock(sp);
  stb_extend_policy(sp->usedN, sp->usedM, sp->maxN, sp->maxM, N, M, &newN, &newM);
  if (newN != sp->usedN || newM != sp->usedM) {
    stb_impl *im = sp->impl;
    if (newN > sp->usedN1) {
      /* allocate-copy-swap so a concurrent S_S1 reader never sees freed memory */
      double *s1 = malloc(sizeof(double) * newN);
      if (!s1) {
        unlock(sp);
        return 1;
      }
      memcpy(s1, sp->S1, sizeof(double) * sp->usedN1);
      memset(s1 + sp->usedN1, 0, sizeof(double) * (newN - sp->usedN1));
      retire_s1(sp, sp->S1);
      sp->S1 = s1;
      im->bytes_host += sizeof(double) * (newN - sp->usedN1);
      sp->usedN1 = newN;
    }
    {
      mirror *m = mirror_new(sp, newN, newM);
      const int prev_dev = stb_device_enter(im->dev);
      drain_runs(im); /* (copies under way read device slabs that provision() may replace and build() writes) */
      rc = !m || provision(sp, newN, newM) || build(sp, sp->a, newN, newM) || (im->eager && mirror_all_locked(sp, m));
      if (!rc)
        publish(sp, m);
      else
        mirror_free(m);
      stb_device_leave(prev_dev);
    }
  }
  unlock(sp);
  return rc;
}

double S_S1(stable_t *sp, unsigned n) {
  double v;
  if (n == 0) return -HUGE_VAL;
  if (!sp->S1) return -HUGE_VAL;
  if (n <= sp->usedN) return sp->S1[n - 1];
  if (n > sp->maxN) {
    /* lib/stable.c:842-844: log(0) unless the asymptote flag is set; with it, Gamma(n-a)/Gamma(1-a)
     * is available in closed form, so answer exactly */
    if (!(sp->flags & S_ASYMPT)) return -HUGE_VAL;
    return lgamma(n - sp->a) - sp->lga;
  }
  lock(sp);
  if (n > sp->usedN1) {
    /* lib/stable.c:845-857: grow the cache by at least 10 % / 50 entries, capped at maxN */
    unsigned g = n;
    double *s1;
    if ((double)g < sp->usedN1 * 1.1) g = (unsigned)(sp->usedN1 * 1.1);
    if (g < sp->usedN1 + 50) g = sp->usedN1 + 50;
    if (g > sp->maxN) g = sp->maxN;
    s1 = malloc(sizeof(double) * g);
    if (!s1) {
      unlock(sp);
      return -HUGE_VAL;
    }
    memcpy(s1, sp->S1, sizeof(double) * sp->usedN1);
    memset(s1 + sp->usedN1, 0, sizeof(double) * (g - sp->usedN1));
    retire_s1(sp, sp->S1);
    sp->S1 = s1;
    ((stb_impl *)sp->impl)->bytes_host += sizeof(double) * (g - sp->usedN1);
    sp->usedN1 = g;
    account(sp);
  }
  if (sp->S1[n - 1] == 0) {
    /* lib/stable.c:859-864 */
    if (sp->S1[n - 2] == 0)
      sp->S1[n - 1] = lgamma(n - sp->a) - sp->lga;
    else
      sp->S1[n - 1] = sp->S1[n - 2] + log(n - 1 - sp->a);
  }
  v = sp->S1[n - 1];
  unlock(sp);
  return v;
}

double S_U(stable_t *sp, unsigned n, unsigned m) {
  /* lib/stable.c:875-883 */
  if (m == 1) return n - sp->a;
  if (m <= 1) yaps_quit("Bad constraints in S_U(%s,%u,%u)\n", sp->tag, n, m);
  return n - m * sp->a + 1 / S_V(sp, n, m);
}

double S_UV(stable_t *sp, unsigned n, unsigned m) {
  /* lib/stable.c:885-897 */
  double SV;
  if (m == 1) return -HUGE_VAL;
  if (m == n + 1) return 1; /* S^n_n == 1 */
  if (m == n) return (n + 1.0) / (n - 1.0);
  SV = S_V(sp, n, m);
  return (n - m * sp->a) * SV + 1.0;
}

static double S_V_long(stable_t *sp, unsigned n, unsigned m);
double S_V(stable_t *sp, unsigned n, unsigned m) {
  /* the short way (see S_S): inside the part of the table that lib/stable.c:903 does not grow for */
  if ((sp->flags & (S_UVTABLE | S_FLOAT | S_THREADS)) == S_UVTABLE && m >= 2 && n >= m && m + 1 < sp->usedM && n + 1 < sp->usedN &&
      ((const stb_impl *)sp->impl)->fullV)
    return sp->V[n - 2][m - 2];
  return S_V_long(sp, n, m);
}
static double __attribute__((noinline)) S_V_long(stable_t *sp, unsigned n, unsigned m) {
  if ((sp->flags & S_UVTABLE) == 0) return 0;
  if (m >= sp->usedM - 1 || n >= sp->usedN - 1) {
    /* lib/stable.c:903-925 */
    if (n > sp->maxN || m > sp->maxM) {
      if (n > sp->maxN && (sp->flags & S_ASYMPT)) {
        if (sp->a > 0) return (1.0 - pow(n, -sp->a)) / sp->a / (m - 1);
        {
          double ln = log(n);
          return ln / (m - 1) * exp(lgamma(1 + (m - 2) / ln) - lgamma(1 + (m - 1) / ln));
        }
      }
      if (sp->flags & S_QUITONBOUND) {
        if (sp->tag)
          yaps_quit("S_V(%u,%u,%lf) tagged '%s' hit bounds (%u,%u)\n", n, m, sp->a, sp->tag,
                    sp->maxN, sp->maxM);
        else
          yaps_quit("S_V(%u,%u,%lf) hit bounds\n", n, m, sp->a);
      }
      return 0;
    }
    {
      /* one step as the reference does (lib/stable.c:924); more only while the request is still
       * outside the table (see S_S) */
      int tries;
      if (extend(sp, n + 1, m + 1)) yaps_quit("S_extend() out of memory\n");
      for (tries = 0; tries < 3 && (m > sp->usedM || n > sp->usedN); tries++)
        if (extend(sp, n + 1, m + 1)) yaps_quit("S_extend() out of memory\n");
    }
  }
  if (m < 2) return 0;
  if (n < m) return 0;
  if (n > sp->usedN || m > sp->usedM) return 0; /* growth was capped by the max bounds */
  {
    mirror *mr = mirror_row(sp, 1, n);
    if (!mr) return 0;
    if (sp->flags & S_FLOAT) return ((float **)mr->rowsV)[n - 2][m - 2];
    return ((double **)mr->rowsV)[n - 2][m - 2];
  }
}

static double S_S_long(stable_t *sp, unsigned N, unsigned T);
double S_S(stable_t *sp, unsigned N, unsigned T) {
  /* The short way: a stored cell of a table whose mirror is complete -- the reference's two loads behind the same tests
   * (lib/stable.c:941-974 reach sp->S[N-3][T-2] for exactly these N, T).  10^6 random look-ups on a 400 MB table: 15 ms
   * as the reference's, where the long way's call, flag and generation loads made it 27. */
  if ((sp->flags & (S_STABLE | S_FLOAT | S_THREADS)) == S_STABLE && T >= 2 && N > T && T <= sp->usedM && N <= sp->usedN &&
      ((const stb_impl *)sp->impl)->fullS)
    return sp->S[N - 3][T - 2];
  return S_S_long(sp, N, T);
}
static double __attribute__((noinline)) S_S_long(stable_t *sp, unsigned N, unsigned T) {
  /* test order of lib/stable.c:941-974 */
  if ((sp->flags & S_STABLE) == 0) return -HUGE_VAL;
  if (N == T) return 0;
  if (T == 1) return S_S1(sp, N);
  if (N < T || T == 0) return -HUGE_VAL;
  if (T > sp->usedM || N > sp->usedN) {
    if (N > sp->maxN || T > sp->maxM) {
      if (N > sp->maxN && (sp->flags & S_ASYMPT)) return S_asympt(sp, N, T);
      if (sp->flags & S_QUITONBOUND) {
        if (sp->tag)
          yaps_quit("S_S(%u,%u,%lf) tagged '%s' hit bounds\n", N, T, sp->a, sp->tag);
        else
          yaps_quit("S_S(%u,%u,%lf) hit bounds\n", N, T, sp->a);
      }
      return -HUGE_VAL;
    }
    {
      /* one growth step can stop short of T: the policy caps the new usedM at the OLD usedN
       * (lib/stable.c:626-628), after which the reference indexes past the end of the row.  Here
       * growth is repeated until the request is covered (the second step always suffices). */
      int tries;
      for (tries = 0; tries < 4 && (T > sp->usedM || N > sp->usedN); tries++)
        if (extend(sp, N + 1, T + 1)) yaps_quit("S_extend() out of memory\n");
      if (T > sp->usedM || N > sp->usedN) return -HUGE_VAL;
    }
  }
  {
    mirror *mr = mirror_row(sp, 0, N);
    if (!mr) return -HUGE_VAL;
    if (sp->flags & S_FLOAT) return ((float **)mr->rowsS)[N - 3][T - 2];
    return ((double **)mr->rowsS)[N - 3][T - 2];
  }
}

void S_free(stable_t *sp) {
  stb_impl *im;
  if (!sp) return;
  im = sp->impl;
  free(sp->tag);
  free(sp->S1);
  if (im) {
    const int prev_dev = stb_device_enter(im->dev);
    mirror *g = im->retired;
    s1_gen *s = im->retired_s1;
    while (g) {
      mirror *nx = g->next;
      mirror_free(g);
      g = nx;
    }
    while (s) {
      s1_gen *nx = s->next;
      free(s->p);
      free(s);
      s = nx;
    }
    drain_runs(im);
    {
      int r;
      for (r = 0; r < STB_MIRROR_RUNS; r++) stb_event_destroy(im->runs[r].ev);
      stb_stream_destroy(im->cp_stream);
    }
    mirror_free(im->cur); /* (owns the row-pointer vectors sp->S / sp->V point to) */
    stb_device_free(im->d_S);
    stb_device_free(im->d_V);
    stb_device_free(im->d_Sf);
    stb_device_free(im->d_Vf);
    stb_device_free(im->d_S1);
    stb_device_free(im->d_ws);
    stb_device_leave(prev_dev);
    free(im);
  }
  if (sp->flags & S_THREADS) pthread_mutex_destroy(&sp->mutex);
  free(sp);
}

void S_report(stable_t *sp, FILE *fp) {
  /* text format of lib/stable.c:1025-1055, byte for byte (including the doubled newline of the
   * FILE variant) */
  const char *s = (sp->flags & S_STABLE) ? "+S" : "";
  const char *uv = (sp->flags & S_UVTABLE) ? "+U/V" : "";
  const char *ty = (sp->flags & S_FLOAT) ? "float" : "double";
  if (fp) {
    if (sp->tag)
      fprintf(fp, "S-table '%s': ", sp->tag);
    else
      fprintf(fp, "S-table: ");
    fprintf(fp, "a=%lf, N=%u/%u, M=%u/%u, %s%s %s", sp->a, sp->usedN, sp->maxN, sp->usedM,
            sp->maxM, s, uv, ty);
    fprintf(fp, " mem=%uk\n", sp->memalloced / 1024);
    fprintf(fp, "\n");
  } else {
    if (sp->tag)
      yaps_message("S-table '%s': ", sp->tag);
    else
      yaps_message("S-table: ");
    yaps_message("a=%lf, N=%u/%u, M=%u/%u, %s%s %s", sp->a, sp->usedN, sp->maxN, sp->usedM,
                 sp->maxM, s, uv, ty);
    yaps_message(" mem=%uk", sp->memalloced / 1024);
    yaps_message("\n");
  }
}

double S_asympt(stable_t *sp, unsigned n, unsigned m) {
  if (sp->a == 0) {
    /* lib/stable.c:1058-1065: Hwang's expansion for Stirling numbers of the first kind */
    double ln = log(n);
    return lgamma(n) + (m - 1) * log(ln) - lgamma(m) - lgamma(1 + (m - 1) / ln);
  } else {
    /* lib/stable.c:1066-1082: Gamma(n) / (Gamma(1-a) Gamma(m) a^{m-1} n^a) (1-n^{-a})^{m-1} */
    double acc = 0;
    double la1 = lgamma(1.0 - sp->a);
    double aln = sp->a * log((double)n);
    double np = pow(n, -sp->a);
    acc += lgamma((double)n) - la1 - lgamma((double)m) - (m - 1.0) * log(sp->a) - aln;
    if (np < 1e-5)
      acc -= (m - 1) * np * (1 + np * (0.5 + np / 3.0));
    else
      acc += (m - 1) * log(1.0 - np);
    return acc;
  }
}
