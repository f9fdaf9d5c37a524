// Threefry-2x32 (20 rounds) and jax 0.4.16's counter layout, shared by the kernels that draw random bits: the fill
// (rc_prng.hip), the training batch that maps such bits to indices itself (rc_batch.hip) and the categorical draw over an
// environment image's texels (rc_relight.hip); and the map from bits to a uniform and a Gumbel value.  Host twin: ../prng.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

__device__ __forceinline__ void threefry2x32(uint32_t k0, uint32_t k1, uint32_t& x0, uint32_t& x1) {
  const uint32_t ks[3] = {k0, k1, k0 ^ k1 ^ 0x1BD11BDAu};
  constexpr int R[2][4] = {{13, 15, 26, 6}, {17, 29, 16, 24}};
  x0 += ks[0];
  x1 += ks[1];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x0 += x1;
      x1 = rotl32(x1, R[i & 1][j]) ^ x0;
    }
    x0 += ks[(i + 1) % 3];
    x1 += ks[(i + 2) % 3] + (uint32_t)(i + 1);
  }
}

// Element e of random_bits(key, (n,)): the counters iota(n) are cut in two halves, block i holds the counters
// (i, i + half) and its words land at i and i + half; an odd n is padded with a zero counter.
__device__ __forceinline__ uint32_t prng_bits_at(uint32_t k0, uint32_t k1, uint32_t e, uint32_t n) {
  const uint32_t half = (n + 1u) >> 1;
  const uint32_t i = e < half ? e : e - half;
  uint32_t x0 = i;
  uint32_t x1 = i + half < n ? i + half : 0u;
  threefry2x32(k0, k1, x0, x1);
  return e < half ? x0 : x1;
}

// jax.random.uniform's float of 32 random bits: the top 23 as the mantissa of a value in [1, 2), minus 1; then
// max(lo, u (hi - lo) + lo)
__device__ __forceinline__ float prng_unit_float(uint32_t bits) { return __uint_as_float((bits >> 9) | 0x3F800000u) - 1.0f; }
__device__ __forceinline__ float prng_uniform(uint32_t bits, float lo, float hi) { return fmaxf(lo, prng_unit_float(bits) * (hi - lo) + lo); }
// jax.random.gumbel: -log(-log(u)) of a uniform in (tiny, 1)
constexpr float kPrngTiny = 1.17549435e-38f;
__device__ __forceinline__ float prng_gumbel_of(float u) { return -logf(-logf(u)); }
__device__ __forceinline__ float prng_gumbel(uint32_t bits) { return prng_gumbel_of(prng_uniform(bits, kPrngTiny, 1.0f)); }
