// Order-fixed sums in double for the evaluation kernels (rc_metrics.hip, rc_albedo.hip): a workgroup of kReduceThreads
// threads adds its values wave by wave and writes them to its own slot, and one workgroup adds the slots.  No atomics, so
// two runs on the same inputs are bitwise equal.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

constexpr int kReduceThreads = 256;

__device__ __forceinline__ double wave_sum_d(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;                                 // lane 0 holds the sum
}

// The sums of K values over a workgroup of kReduceThreads threads, in a fixed order: wave sums (shuffles), then the four
// waves in order by thread 0, which writes them to dst[0..K).
template <int K>
__device__ __forceinline__ void block_sums(double (&v)[K], double* lds /* [4][K] */, double* dst) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double s = wave_sum_d(v[k]);
    if (lane == 0) lds[wave * K + k] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) dst[k] = ((lds[k] + lds[K + k]) + lds[2 * K + k]) + lds[3 * K + k];
  }
}

// The sum of n doubles at stride `stride`, by one workgroup in a fixed order: a strided partial per thread, a tree through
// LDS (lds: [kReduceThreads]).
__device__ inline double ordered_sum(const double* p, int64_t n, int stride, double* lds) {
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kReduceThreads) s += p[i * stride];
  __syncthreads();                          // the previous sum's lds[0] has been read
  lds[threadIdx.x] = s;
  __syncthreads();
  for (int st = kReduceThreads / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) lds[threadIdx.x] += lds[threadIdx.x + st];
    __syncthreads();
  }
  return lds[0];
}
