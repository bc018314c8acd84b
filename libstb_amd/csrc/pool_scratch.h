// pool_scratch.h -- private: what one call of an object layer (tcounts_obj.hip, tindic_obj.hip) takes from the buffer cache.
#ifndef STB_POOL_SCRATCH_H
#define STB_POOL_SCRATCH_H

#include "stb_common.h"

namespace {  // (each file that includes this has its own: no symbols of it leave the file)

// what one call takes from the buffer cache: given back when the call ends, behind a wait for the object's stream (the cache
// may hand a buffer on at once).  Declared after the call's device scope, so it goes while the object's device is current.
struct stb_pool_scratch {
  hipStream_t st;
  void *p[4] = {nullptr, nullptr, nullptr, nullptr};
  int n = 0;
  explicit stb_pool_scratch(hipStream_t st_) : st(st_) {}
  stb_pool_scratch(const stb_pool_scratch &) = delete;
  stb_pool_scratch &operator=(const stb_pool_scratch &) = delete;
  template <class T>
  hipError_t take(T **out, size_t bytes, int kind = 0) {  // kind as stb_pool_malloc's
    if (n == 4) return hipErrorOutOfMemory;
    const hipError_t e = stb_pool_malloc((void **)out, bytes, kind);
    if (e == hipSuccess) p[n++] = (void *)*out;
    return e;
  }
  // who non-null: a failed wait is the call's failure
  int give_back(bool wait, const char *who) {
    int rc = 0;
    if (n && wait && hipStreamSynchronize(st) != hipSuccess && who) rc = STB_STREAM_FAIL(who);
    for (int k = 0; k < n; k++) stb_pool_free(p[k]);
    n = 0;
    return rc;
  }
  // rc of the call's last step, which has waited for its own answer where it succeeded (or, the draw of
  // stb_tindic_sample_lik, left nothing the host waits for): no second wait then; a failed one waits
  int last(int rc) {
    if (!rc) (void)give_back(false, nullptr);
    return rc;
  }
  ~stb_pool_scratch() { (void)give_back(true, nullptr); }
};

}  // namespace

#endif
