// Counter-based random fill in HBM with the stream layout of the reference's jax.random (jax 0.4.16: threefry2x32,
// non-partitionable counters) -- SURVEY.md §8(f) rank 3.  Host twin and the conventions: ../prng.py.
//
// Layout (jax/_src/prng.py of the pinned jax, restated): the counters iota(n) are cut in two halves; block i has
// counter words (i, i + half) and its two output words land at out[i] and out[i + half]; an odd n is padded with
// a zero counter whose output is dropped.  One lane per block: 20 rounds of 32-bit add/rotate/xor, two coalesced
// 4-byte stores -- a pure streaming kernel (8 bytes written per block, nothing read).
#include <hip/hip_runtime.h>

#include "rc_internal.h"
#include "rc_dev_prng.h"

namespace {

// XLA's single-precision erfinv (Giles' polynomial), evaluated in the same order as ../prng.py
__device__ __forceinline__ float erfinv32(float x) {
  const float w = -log1pf(-x * x);
  float p, ww;
  if (w < 5.0f) {
    ww = w - 2.5f;
    p = 2.81022636e-08f;
    p = 3.43273939e-07f + p * ww;
    p = -3.5233877e-06f + p * ww;
    p = -4.39150654e-06f + p * ww;
    p = 0.00021858087f + p * ww;
    p = -0.00125372503f + p * ww;
    p = -0.00417768164f + p * ww;
    p = 0.246640727f + p * ww;
    p = 1.50140941f + p * ww;
  } else {
    ww = sqrtf(w) - 3.0f;
    p = -0.000200214257f;
    p = 0.000100950558f + p * ww;
    p = 0.00134934322f + p * ww;
    p = -0.00367342844f + p * ww;
    p = 0.00573950773f + p * ww;
    p = -0.0076224613f + p * ww;
    p = 0.00943887047f + p * ww;
    p = 1.00167406f + p * ww;
    p = 2.83297682f + p * ww;
  }
  return p * x;
}

__device__ __forceinline__ uint32_t shape_value(uint32_t bits, int mode, float lo, float hi) {
  if (mode == RC_PRNG_BITS) return bits;
  const float u = prng_uniform(bits, lo, hi);
  float v = u;
  if (mode == RC_PRNG_NORMAL) v = 1.41421356237309515f * erfinv32(u);
  if (mode == RC_PRNG_GUMBEL) v = prng_gumbel_of(u);
  return __float_as_uint(v);
}

__global__ __launch_bounds__(256) void k_prng_fill(RcPrngArgs a) {
  const int64_t half = (a.n + 1) >> 1;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < half; i += (int64_t)gridDim.x * 256) {
    uint32_t x0 = (uint32_t)i;
    uint32_t x1 = i + half < a.n ? (uint32_t)(i + half) : 0u;     // odd n: zero pad
    threefry2x32(a.key0, a.key1, x0, x1);
    a.out[i] = shape_value(x0, a.mode, a.lo, a.hi);
    if (i + half < a.n) a.out[i + half] = shape_value(x1, a.mode, a.lo, a.hi);
  }
}

// Several fills in one launch: a workgroup finds its row of the table from blockIdx.x alone, so key, mode, range and
// offsets are wave-uniform; the lane's block is the one k_prng_fill computes for the same key and element count, and its
// two words go through the same shape_value.  Two planes: element e lands at plane[e & 1][e >> 1].
__global__ __launch_bounds__(256) void k_prng_fill_segments(RcPrngSegArgs a) {
  const uint32_t wg = blockIdx.x;
  int s = 0;
  while (s < a.n_segs - 1 && wg >= a.wg_end[s]) ++s;
  const RcPrngSegRow& r = a.seg[s];
  const uint32_t n = r.n, half = (n >> 1) + (n & 1u);
  const uint32_t i = (wg - (s ? a.wg_end[s - 1] : 0u)) * 256u + threadIdx.x;
  if (i >= half) return;
  const uint32_t e1 = i + half;                                  // < 2^32 - 1: no wrap
  uint32_t x0 = i;
  uint32_t x1 = e1 < n ? e1 : 0u;                                // odd n: zero pad
  threefry2x32(r.key0, r.key1, x0, x1);
  const uint32_t v0 = shape_value(x0, r.mode, r.lo, r.hi), v1 = shape_value(x1, r.mode, r.lo, r.hi);
  if (r.off2 < 0) {
    a.arena[r.off + i] = v0;
    if (e1 < n) a.arena[r.off + e1] = v1;
  } else {
    a.arena[((i & 1u) ? r.off2 : r.off) + (i >> 1)] = v0;
    if (e1 < n) a.arena[((e1 & 1u) ? r.off2 : r.off) + (e1 >> 1)] = v1;
  }
}

}  // namespace

void rc_launch_prng_fill_segments(const RcPrngSegArgs& a, hipStream_t stream) {
  const uint32_t blocks = a.n_segs > 0 ? a.wg_end[a.n_segs - 1] : 0u;
  if (blocks) hipLaunchKernelGGL(k_prng_fill_segments, dim3(blocks), dim3(256), 0, stream, a);
}

void rc_launch_prng_fill(const RcPrngArgs& a, hipStream_t stream) {
  const int64_t half = (a.n + 1) >> 1;
  int64_t blocks = (half + 255) / 256;
  if (blocks > 256 * 32) blocks = 256 * 32;       // grid-stride beyond 2M blocks of counters
  hipLaunchKernelGGL(k_prng_fill, dim3((unsigned)blocks), dim3(256), 0, stream, a);
}
