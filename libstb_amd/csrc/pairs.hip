// pairs.hip -- the pairs' way to the device: what a group set needs when its (n,t) pairs are NEW (why: lists.hip; rounds
// 2-4 copied the ragged arrays twice, flat, then to the device through the runtime's own staging).  Here:
//   * stb_groups_pairs_begin / _put / _put_ragged / _commit: the caller's arrays are copied ONCE, into pinned memory (the
//     maxima of n and t -- the table bounds of lib/samplea.c:186-208 -- fall out of the same pass); a whole set at once is
//     copied by a few host threads of the library's own while the calling thread hands the finished pieces to the DMA
//     engine (one core of the GPU box's host moves the 6 MB of 10^6 pairs in 0.41 ms, four in 0.18).
//   * pairs are no longer sorted by (n,t) when a set is made: the fused evaluation does not read them, and the gather
//     over a stored table of 4000 x 4000 (64 MB: it lives in the Infinity Cache) is as fast on unsorted pairs
//     (0.035 ms either way, profiles/r05_fresh_before.txt).  The sort is made on first need by the evaluations through
//     stored tables, whose sum then does not depend on the caller's order, as before.
#include <algorithm>
#include <vector>

#include <pthread.h>
#include <sched.h>

#include "groups.h"

// The set's d_n / d_t hold new pairs (stb_groups_pairs_commit, stb_groups_take_counts): the cell lists are rebuilt and the
// pairs sorted again on first need.  reused: the caller is one that serves sweep after sweep (stb_groups_update_restaurants)
void stb_groups_new_pairs(stb_groups_t *g, int reused) {
  stb_lists_drop(g, true);
  g->sorted = 0;
  g->have_pairs = 1;
  g->reused = reused;
}


// ------------------------------------------------------------------------------------------------
// the pairs' way to the device

#define STB_PUT_CHUNK (256u * 1024u)  // pairs per piece handed to the stream (1.5 MB)

extern "C" int stb_groups_pairs_begin(stb_groups_t *g) {
  STB_ENTRY;
  if (!g) return stb_fail("stb_groups_pairs_begin: null group set");
  if (g->pending == 1) return stb_fail("stb_groups_pairs_begin: an evaluation queued with stb_groups_aterms_async has not been waited for");
  stb_device_scope dev(g->dev);
  g->put_n = g->flushed_n = 0;
  g->put_maxn = g->put_maxt = 0;
  g->putting = 0;
  // (whatever still reads the device copy of the old pairs, or copies out of the staging area, must be through)
  if (hipStreamSynchronize(g->st) != hipSuccess) return stb_fail("stb_groups_pairs_begin: %s", hipGetErrorString(hipGetLastError()));
  // (each staging area for itself: one may be there from a call that failed on the other)
  if (g->G && ((!g->h_pn && stb_pool_malloc((void **)&g->h_pn, 4 * (size_t)g->G, 1) != hipSuccess) ||
               (!g->h_pt && stb_pool_malloc((void **)&g->h_pt, 2 * (size_t)g->G, 1) != hipSuccess)))
    return stb_fail("stb_groups_pairs_begin: out of pinned host memory");
  g->putting = 1;
  return 0;
}

// copy and maxima in one pass (the compiler turns both loops into vector code)
static unsigned copy_max_u32(uint32_t *__restrict d, const uint32_t *__restrict s, size_t n, unsigned m) {
  for (size_t i = 0; i < n; i++) {
    const uint32_t v = s[i];
    d[i] = v;
    m = v > m ? v : m;
  }
  return m;
}
static unsigned copy_max_u16(uint16_t *__restrict d, const uint16_t *__restrict s, size_t n, unsigned m) {
  uint16_t mm = 0;
  for (size_t i = 0; i < n; i++) {
    const uint16_t v = s[i];
    d[i] = v;
    mm = v > mm ? v : mm;
  }
  return mm > m ? mm : m;
}

static int put_flush(stb_groups_t *g, bool all) {
  while (g->put_n - g->flushed_n >= (all ? 1u : STB_PUT_CHUNK)) {
    const uint64_t c = all ? g->put_n - g->flushed_n : STB_PUT_CHUNK;
    const uint64_t o = g->flushed_n;
    HIPCHK(hipMemcpyAsync(g->d_n + o, g->h_pn + o, 4 * c, hipMemcpyHostToDevice, g->st));
    HIPCHK(hipMemcpyAsync(g->d_t + o, g->h_pt + o, 2 * c, hipMemcpyHostToDevice, g->st));
    g->flushed_n += c;
  }
  return 0;
}

extern "C" int stb_groups_pairs_put(stb_groups_t *g, const uint32_t *n, const uint16_t *t, uint64_t count, unsigned *maxn, unsigned *maxt) {
  // (no STB_ENTRY: called a thousand times per set, and nothing below can reach the runtime's initialisation -- the
  // set exists, so the runtime is up)
  if (!g || !g->putting) return stb_fail("stb_groups_pairs_put: stb_groups_pairs_begin comes first");
  if (g->put_n + count > g->G) return stb_fail("stb_groups_pairs_put: %llu pairs for a set of %llu", (unsigned long long)(g->put_n + count), (unsigned long long)g->G);
  if (count) {
    g->put_maxn = copy_max_u32(g->h_pn + g->put_n, n, count, g->put_maxn);
    g->put_maxt = copy_max_u16(g->h_pt + g->put_n, t, count, g->put_maxt);
    g->put_n += count;
  }
  if (maxn) *maxn = g->put_maxn;
  if (maxt) *maxt = g->put_maxt;
  if (g->put_n - g->flushed_n < STB_PUT_CHUNK) return 0;
  stb_device_scope dev(g->dev);
  return put_flush(g, false);
}

extern "C" int stb_groups_pairs_commit(stb_groups_t *g, const uint32_t *T, const double *bpar, unsigned N, unsigned M) {
  STB_ENTRY;
  if (!g || !g->putting) return stb_fail("stb_groups_pairs_commit: stb_groups_pairs_begin comes first");
  if (g->put_n != g->G) return stb_fail("stb_groups_pairs_commit: %llu of the set's %llu pairs supplied", (unsigned long long)g->put_n, (unsigned long long)g->G);
  stb_device_scope dev(g->dev);
  g->putting = 0;
  if (put_flush(g, true)) return 1;
  if (N == 0 || M == 0) {
    if (!g->have_bounds) return stb_fail("stb_groups_pairs_commit: the set has no table bounds yet");
    N = g->N;
    M = g->M;
  }
  if (stb_groups_set_bounds(g, N, M)) return 1;  // (drops what depends on the bounds when they change)
  stb_groups_new_pairs(g, 0);
  if (T && bpar && g->I > 0) {
    memcpy(g->h_T, T, sizeof(uint32_t) * (size_t)g->I);
    memcpy(g->h_bpar, bpar, sizeof(double) * (size_t)g->I);
    if (hipMemcpyAsync(g->d_T, g->h_T, sizeof(uint32_t) * (size_t)g->I, hipMemcpyHostToDevice, g->st) != hipSuccess ||
        hipMemcpyAsync(g->d_bpar, g->h_bpar, sizeof(double) * (size_t)g->I, hipMemcpyHostToDevice, g->st) != hipSuccess)
      return stb_fail("stb_groups_pairs_commit: %s", hipGetErrorString(hipGetLastError()));
  }
  return 0;
}

// ---- a whole set at once, copied by several host threads while the calling thread hands the finished pieces to the
// stream.  One core copies 6 MB into pinned memory in 0.41 ms (14.6 GB/s: what a core of the GPU box's host moves),
// which was the largest single piece of a samplea call on new pairs; four copy 1.5 MB each while the DMA engine takes
// what is done.  The workers are the library's own (started on first use, STB_PUT_THREADS of them, default 4; 0: the
// calling thread copies); they touch host memory only.
#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>

namespace {
struct put_slice {
  // restaurants [i0, i1) of a ragged set, or one flat range when K is null; the slice's pairs start at `off`
  int i0, i1;
  uint64_t off, count;
  std::atomic<uint64_t> done;  // pairs of the slice copied so far
  unsigned maxn, maxt;
};
struct put_job {
  const int *K;
  uint32_t *const *n;
  uint16_t *const *t;
  const uint32_t *nflat;
  const uint16_t *tflat;
  uint32_t *dn;
  uint16_t *dt;
  put_slice *slices;
  int nslices;
  std::atomic<int> next;  // the next slice nobody has taken
};
struct put_pool {
  std::mutex use;  // one hand-over at a time has the workers; another thread's meanwhile is copied by that thread itself
  std::mutex mu;
  std::condition_variable cv;
  std::vector<std::thread> th;
  put_job *job = nullptr;
  unsigned long long gen = 0;
  int busy = 0;
};
put_pool *g_put_pool = nullptr;  // (never destroyed: its threads sleep until the process ends)
std::once_flag g_put_once;

// one slice, if any is left: copied by whoever calls (a worker of the pool, or the calling thread while it waits for them)
bool put_step(put_job *J) {
  {
    const int k = J->next.fetch_add(1);
    if (k >= J->nslices) return false;
    put_slice &S = J->slices[k];
    unsigned mn = 0, mt = 0;
    uint64_t o = S.off, since = 0;
    if (J->K) {
      for (int i = S.i0; i < S.i1; i++) {
        const uint64_t c = (uint64_t)(J->K[i] > 0 ? J->K[i] : 0);
        mn = copy_max_u32(J->dn + o, J->n[i], c, mn);
        mt = copy_max_u16(J->dt + o, J->t[i], c, mt);
        o += c;
        since += c;
        if (since >= 32768) {  // (publish: the calling thread hands finished pieces to the stream)
          S.done.store(o - S.off, std::memory_order_release);
          since = 0;
        }
      }
    } else {
      for (uint64_t c0 = 0; c0 < S.count; c0 += 32768) {
        const uint64_t c = S.count - c0 < 32768 ? S.count - c0 : 32768;
        mn = copy_max_u32(J->dn + o, J->nflat + o, c, mn);
        mt = copy_max_u16(J->dt + o, J->tflat + o, c, mt);
        o += c;
        S.done.store(o - S.off, std::memory_order_release);
      }
    }
    S.maxn = mn;
    S.maxt = mt;
    S.done.store(S.count, std::memory_order_release);
  }
  return true;
}
void put_run(put_job *J) {
  while (put_step(J)) {
  }
}

// (a fork()ed child has the pool's pointer but none of its threads: it copies on its own thread)
void put_atfork_child() { g_put_pool = nullptr; }

void put_worker(put_pool *P) {
  unsigned long long seen = 0;
  for (;;) {
    put_job *J;
    {
      std::unique_lock<std::mutex> lk(P->mu);
      P->cv.wait(lk, [&] { return P->gen != seen; });
      seen = P->gen;
      J = P->job;
      if (!J) continue;
      P->busy++;
    }
    put_run(J);
    {
      std::lock_guard<std::mutex> lk(P->mu);
      P->busy--;
    }
    P->cv.notify_all();
  }
}
}  // namespace

// all G pairs of the set, ragged (K, n[i], t[i]) or flat (K null: nflat, tflat), between begin and commit
static int put_all(stb_groups_t *g, int I, const int *K, uint32_t *const *n, uint16_t *const *t, const uint32_t *nflat, const uint16_t *tflat,
                   unsigned *maxn, unsigned *maxt) {
  if (!g || !g->putting || g->put_n != 0) return stb_fail("stb_groups_pairs_put_ragged: between stb_groups_pairs_begin and the first put only");
  uint64_t G = 0;
  if (K) {
    for (int i = 0; i < I; i++) G += (uint64_t)(K[i] > 0 ? K[i] : 0);
    if (G != g->G) return stb_fail("stb_groups_pairs_put_ragged: %llu pairs for a set of %llu", (unsigned long long)G, (unsigned long long)g->G);
  } else {
    G = g->G;
  }
  int W = stb_env_int("STB_PUT_THREADS", 4);
  // (the cores this process may run on, not those of the machine: under taskset to one core the calling thread copies alone)
  unsigned hw = std::thread::hardware_concurrency();
  {
    cpu_set_t cs;
    CPU_ZERO(&cs);
    if (sched_getaffinity(0, sizeof(cs), &cs) == 0 && CPU_COUNT(&cs) > 0) hw = (unsigned)CPU_COUNT(&cs);
  }
  if (hw && W > (int)hw - 1) W = (int)hw - 1;
  if (W > 16) W = 16;
  if (G < 131072) W = 0;  // (small sets: the calling thread is through before a worker is awake)
  // slices of about 64 K pairs, taken in order by whoever is free
  const uint64_t per = 65536;
  const size_t cap = (size_t)(G / per + 2);  // (every slice but the last holds at least `per` pairs)
  std::unique_ptr<put_slice[]> slices(new put_slice[cap]);
  int ns = 0;
  auto add = [&](int i0, int i1, uint64_t off, uint64_t cnt) {
    put_slice &S = slices[(size_t)ns++];
    S.i0 = i0;
    S.i1 = i1;
    S.off = off;
    S.count = cnt;
    S.done.store(0);
    S.maxn = S.maxt = 0;
  };
  if (K) {
    int i0 = 0;
    uint64_t off = 0, cnt = 0;
    for (int i = 0; i < I; i++) {
      cnt += (uint64_t)(K[i] > 0 ? K[i] : 0);
      if (cnt >= per || i == I - 1) {
        add(i0, i + 1, off, cnt);
        off += cnt;
        cnt = 0;
        i0 = i + 1;
      }
    }
  } else {
    for (uint64_t off = 0; off < G; off += per) add(0, 0, off, G - off < per ? G - off : per);
  }
  put_job J;
  J.K = K;
  J.n = n;
  J.t = t;
  J.nflat = nflat;
  J.tflat = tflat;
  J.dn = g->h_pn;
  J.dt = g->h_pt;
  J.slices = slices.get();
  J.nslices = ns;
  J.next.store(0);
  put_pool *P = nullptr;
  std::unique_lock<std::mutex> use_lk;
  if (W > 0 && J.nslices > 1) {
    std::call_once(g_put_once, [W] {
      put_pool *np = new put_pool;
      try {
        for (int w = 0; w < W; w++) np->th.emplace_back(put_worker, np);
      } catch (...) {  // (no more threads to be had: those that started serve; none: the callers copy themselves)
      }
      for (auto &th : np->th) th.detach();
      g_put_pool = np;
      (void)pthread_atfork(nullptr, nullptr, put_atfork_child);
    });
    P = (g_put_pool && !g_put_pool->th.empty()) ? g_put_pool : nullptr;
    if (P) {
      // (samplers of different host threads share the workers: whoever finds them busy copies on its own thread)
      use_lk = std::unique_lock<std::mutex>(P->use, std::try_to_lock);
      if (!use_lk.owns_lock()) P = nullptr;
    }
  }
  if (P) {
    {
      std::lock_guard<std::mutex> lk(P->mu);
      P->job = &J;
      P->gen++;
    }
    P->cv.notify_all();
  }
  int rc = 0;
  {
    stb_device_scope dev(g->dev);
    if (!P) put_run(&J);  // (the calling thread copies; the pieces go out below)
    // hand finished pieces to the stream, in order, while the workers copy
    uint64_t flushed = 0;
    int k = 0;
    while (k < J.nslices && !rc) {
      put_slice &S = slices[(size_t)k];
      const uint64_t d = S.done.load(std::memory_order_acquire);
      const uint64_t upto = S.off + d;
      if (d == S.count) k++;
      if (upto - flushed >= 131072 || (k == J.nslices && upto > flushed)) {
        if (hipMemcpyAsync(g->d_n + flushed, g->h_pn + flushed, 4 * (upto - flushed), hipMemcpyHostToDevice, g->st) != hipSuccess ||
            hipMemcpyAsync(g->d_t + flushed, g->h_pt + flushed, 2 * (upto - flushed), hipMemcpyHostToDevice, g->st) != hipSuccess)
          rc = stb_fail("stb_groups_pairs_put_ragged: %s", hipGetErrorString(hipGetLastError()));
        flushed = upto;
      } else if (d != S.count) {
        // (nothing to hand over yet: take a slice too -- the workers may be busy, few, or, in a fork()ed child, gone)
        if (!put_step(&J)) __builtin_ia32_pause();
      }
    }
  }
  if (P) {  // (the job lives on this stack: every worker must have let go of it)
    std::unique_lock<std::mutex> lk(P->mu);
    P->job = nullptr;
    P->cv.wait(lk, [&] { return P->busy == 0; });
  }
  if (rc) return rc;
  unsigned mn = 0, mt = 0;
  for (int k = 0; k < ns; k++) {
    mn = slices[(size_t)k].maxn > mn ? slices[(size_t)k].maxn : mn;
    mt = slices[(size_t)k].maxt > mt ? slices[(size_t)k].maxt : mt;
  }
  g->put_n = g->flushed_n = G;
  g->put_maxn = mn;
  g->put_maxt = mt;
  if (maxn) *maxn = mn;
  if (maxt) *maxt = mt;
  return 0;
}

extern "C" int stb_groups_pairs_put_ragged(stb_groups_t *g, int I, const int *K, uint32_t *const *n, uint16_t *const *t, unsigned *maxn, unsigned *maxt) {
  if (!K || !n || !t) return stb_fail("stb_groups_pairs_put_ragged: null argument");
  return put_all(g, I, K, n, t, nullptr, nullptr, maxn, maxt);
}

// new pairs for the same shape and the same table bounds, from flat arrays
extern "C" int stb_groups_update_pairs(stb_groups_t *g, const uint32_t *nflat, const uint16_t *tflat) {
  if (!g) return stb_fail("stb_groups_update_pairs: null group set");
  if (!g->have_bounds) return stb_fail("stb_groups_update_pairs: the set has no table bounds yet (stb_groups_pairs_commit sets them)");
  if (stb_groups_pairs_begin(g)) return 1;
  if (g->G && put_all(g, 0, nullptr, nullptr, nullptr, nflat, tflat, nullptr, nullptr)) return 1;
  return stb_groups_pairs_commit(g, nullptr, nullptr, 0, 0);
}
