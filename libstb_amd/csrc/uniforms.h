// uniforms.h -- private: the counter-based uniforms every sampler kernel and its host replay share (libstb_amd/synth.py's
// splitmix64).  A sweep s of a call has the key mix(seed + (s+1) gamma); element j of its stream is stb_unit(key, j), so a
// draw depends on (seed, sweep, j) alone, not on launch geometry or timing.
#ifndef STB_UNIFORMS_H
#define STB_UNIFORMS_H

#include "stb_common.h"

static constexpr uint64_t STB_GAMMA = 0x9E3779B97F4A7C15ull;

__host__ __device__ static inline uint64_t stb_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// element j of a stream: top 53 bits of mix(key + j gamma) / 2^53, in [0, 1)
__host__ __device__ __forceinline__ double stb_unit(uint64_t key, uint64_t j) {
  return (double)(stb_mix64(key + j * STB_GAMMA) >> 11) * (1.0 / 9007199254740992.0);
}

#endif
