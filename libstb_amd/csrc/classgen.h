// classgen.h -- private: what the object layer (tindic_obj.hip) needs of classgen.hip beyond include/stb_hip.h.
#ifndef STB_CLASSGEN_H
#define STB_CLASSGEN_H

#include "stb_common.h"
#include "views.h"

// bytes of the scratch a class draw under a rows x stride matrix needs: the running sums inside the chunks (as large as
// the matrix) and the chunks' cumulative ends
size_t stb_cg_scratch_bytes(unsigned rows, unsigned stride);
// the cumulative pass, the chunk bases and the draw on st, no wait; the arguments are checked by the caller.  d_scratch:
// stb_cg_scratch_bytes(L.rows, L.stride) bytes that stay the call's until the stream has run it.  d_info: NULL, or three
// uint64 (skipped, stuck, drawn), added to.  Only d_cls, d_scratch and d_info are written
int stb_cg_launch(const stb_lik_view &L, const uint32_t *d_cust, const uint8_t *d_mask, uint64_t C, const stb_draw_key &k,
                  uint32_t *d_cls, uint64_t *d_info, void *d_scratch, hipStream_t st, const char *who);

#endif
