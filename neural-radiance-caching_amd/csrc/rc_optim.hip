// The cache stage's optimizer step on the flat parameter / gradient buffers.
//
// What train_step does after value_and_grad and pmean (internal/train_utils.py:3128-3161), element by element:
//   g = nan_to_num(g)                            NaN -> 0, +-inf -> +-FLT_MAX        (:3157)
//   g = clip(g, -grad_max_val, grad_max_val)     when grad_max_val > 0               clip_gradients (:1274-1298)
//   g = mult * g                                 when grad_max_norm > 0, mult = min(1, max_norm / (FLT_EPSILON + norm)),
//                                                norm = sqrt(sum g^2) over the top-level module (the buffers of one call)
// then optax.adam (scale_by_adam, eps_root = 0, then scale_by_learning_rate) and apply_updates, at count t before the step:
//   mu = (1 - b1) g + b1 mu;  nu = (1 - b2) (g g) + b2 nu
//   u  = (mu / bc1) / (sqrt(nu / bc2) + eps),  bc1 = 1 - b1^(t+1), bc2 = 1 - b2^(t+1)
//   p  = p + u * (-lr(t))
// in float32 with every operation rounded on its own (the library builds with -ffp-contract=off): bitwise what a numpy
// float32 restatement fed the same per-step scalars computes (tests/optimizer_ref.py).  The update is dense: every
// element moves every step.  Optionally g = 0 is written back, so the next step's backward calls accumulate into it.
//
// Kernels:
//   k_adam         one launch over every buffer of the call: a workgroup owns a tile of kAdamTile consecutive floats of one
//                  buffer, each lane kAdamVec float4 of each of p, g, mu, nu (16-byte loads, all issued before the first
//                  use: 64 KiB in flight per workgroup), the group of an element from the call's runs (a run = consecutive
//                  segments of one group; a tile usually lies in one run).
//   k_adam_sumsq   the same tiles: per tile the sum of the sanitized, value-clipped g^2 in double (fixed order).
//   k_adam_norm    one workgroup: the tile partials added in a fixed order, norm and the clip multiplier, written to the
//                  device (k_adam reads it there: no host sync).
#include <hip/hip_runtime.h>

#include <float.h>

#include "rc_internal.h"

namespace {

constexpr int kAdamThreads = 256;
constexpr int kAdamVec = 4;                                   // float4 per lane per array
constexpr int64_t kAdamTile = (int64_t)kAdamThreads * kAdamVec * 4;

struct Span { int kb; int64_t t0, t1; };

// The buffer and element range [t0, t1) of this workgroup's tile (uniform).
__device__ inline Span tile_of(const RcAdamArgs& a) {
  const int64_t b = blockIdx.x;
  int kb = 0;
  for (int k = 1; k < a.nbuf; ++k)
    if (b >= a.buf[k].block0) kb = k;
  const int64_t t0 = (b - a.buf[kb].block0) * kAdamTile;
  const int64_t t1 = t0 + kAdamTile < a.buf[kb].n ? t0 + kAdamTile : a.buf[kb].n;
  return {kb, t0, t1};
}

// nan_to_num, then the clip by value (max_val > 0)
__device__ inline float sanitize(float g, float max_val) {
  g = g != g ? 0.0f : (g == INFINITY ? FLT_MAX : (g == -INFINITY ? -FLT_MAX : g));
  if (max_val > 0.0f) g = fminf(fmaxf(g, -max_val), max_val);
  return g;
}

__device__ inline float comp(const float4& v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }
__device__ inline void set_comp(float4& v, int c, float x) {
  if (c == 0) v.x = x; else if (c == 1) v.y = x; else if (c == 2) v.z = x; else v.w = x;
}

// 4 elements from element e (16-byte aligned); past n: zeros
__device__ inline float4 load4(const float* __restrict__ p, int64_t e, int64_t n) {
  if (e + 4 <= n) return *reinterpret_cast<const float4*>(p + e);
  float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (int c = 0; c < 4; ++c)
    if (e + c < n) set_comp(v, c, p[e + c]);
  return v;
}
__device__ inline void store4(float* __restrict__ p, int64_t e, int64_t n, const float4& v) {
  if (e + 4 <= n) { *reinterpret_cast<float4*>(p + e) = v; return; }
  for (int c = 0; c < 4; ++c)
    if (e + c < n) p[e + c] = comp(v, c);
}

__global__ void __launch_bounds__(kAdamThreads) k_adam(const RcAdamArgs a) {
  const Span s = tile_of(a);
  const RcAdamBuf& B = a.buf[s.kb];
  float4 p[kAdamVec], g[kAdamVec], m[kAdamVec], v[kAdamVec];
  int64_t e[kAdamVec];
#pragma unroll
  for (int k = 0; k < kAdamVec; ++k) e[k] = s.t0 + 4 * ((int64_t)k * kAdamThreads + threadIdx.x);
#pragma unroll
  for (int k = 0; k < kAdamVec; ++k) {
    if (e[k] >= s.t1) continue;
    g[k] = load4(B.grads, e[k], s.t1);
    p[k] = load4(B.params, e[k], s.t1);
    m[k] = load4(B.mu, e[k], s.t1);
    v[k] = load4(B.nu, e[k], s.t1);
  }
  const float mult = a.mult ? *a.mult : 1.0f;
  // the runs that overlap the tile (uniform loop; one run for all but the tiles across a group boundary)
  for (int r = B.run0; r < B.run0 + B.nruns; ++r) {
    const int64_t r0 = r == B.run0 ? 0 : a.run_end[r - 1], r1 = a.run_end[r];
    if (r1 <= s.t0 || r0 >= s.t1) continue;
    const RcAdamGroup G = a.group[a.run_group[r]];
    const float neg_lr = -G.lr;
#pragma unroll
    for (int k = 0; k < kAdamVec; ++k) {
      if (e[k] >= s.t1) continue;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int64_t i = e[k] + c;
        if (i < r0 || i >= r1) continue;
        float gi = sanitize(comp(g[k], c), a.max_val);
        if (a.mult) gi = mult * gi;
        const float mu = G.omb1 * gi + G.b1 * comp(m[k], c);
        const float nu = G.omb2 * (gi * gi) + G.b2 * comp(v[k], c);
        const float u = (mu / G.bc1) / (sqrtf(nu / G.bc2) + G.eps);
        set_comp(p[k], c, comp(p[k], c) + u * neg_lr);
        set_comp(m[k], c, mu);
        set_comp(v[k], c, nu);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kAdamVec; ++k) {
    if (e[k] >= s.t1) continue;
    store4(B.params, e[k], s.t1, p[k]);
    store4(B.mu, e[k], s.t1, m[k]);
    store4(B.nu, e[k], s.t1, v[k]);
    if (a.zero_grads) store4(B.grads, e[k], s.t1, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
  }
}

__global__ void __launch_bounds__(kAdamThreads) k_adam_sumsq(const RcAdamArgs a, double* __restrict__ part) {
  const Span s = tile_of(a);
  const RcAdamBuf& B = a.buf[s.kb];
  float4 g[kAdamVec];
  int64_t e[kAdamVec];
#pragma unroll
  for (int k = 0; k < kAdamVec; ++k) {
    e[k] = s.t0 + 4 * ((int64_t)k * kAdamThreads + threadIdx.x);
    g[k] = e[k] < s.t1 ? load4(B.grads, e[k], s.t1) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < kAdamVec; ++k)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double x = (double)sanitize(comp(g[k], c), a.max_val);     // zeros past the tile add nothing
      acc += x * x;
    }
  __shared__ double sh[kAdamThreads];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int st = kAdamThreads / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

__global__ void __launch_bounds__(kAdamThreads) k_adam_norm(const double* __restrict__ part, int64_t nparts, float max_norm,
                                                           float* __restrict__ mult, float* __restrict__ norm_out) {
  __shared__ double sh[kAdamThreads];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < nparts; i += kAdamThreads) acc += part[i];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int st = kAdamThreads / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(sh[0]);
    *norm_out = norm;
    *mult = fminf(1.0f, max_norm / (FLT_EPSILON + norm));          // jnp.minimum(1, max_norm / (eps + tree_norm(g)))
  }
}

}  // namespace

int64_t rc_adam_tile() { return kAdamTile; }

void rc_launch_adam(const RcAdamArgs& a, int64_t blocks, hipStream_t st) {
  if (blocks <= 0) return;
  hipLaunchKernelGGL(k_adam, dim3((unsigned)blocks), dim3(kAdamThreads), 0, st, a);
}

void rc_launch_adam_norm(const RcAdamArgs& a, int64_t blocks, float max_norm, double* part, float* mult, float* norm,
                         hipStream_t st) {
  if (blocks > 0) hipLaunchKernelGGL(k_adam_sumsq, dim3((unsigned)blocks), dim3(kAdamThreads), 0, st, a, part);
  hipLaunchKernelGGL(k_adam_norm, dim3(1), dim3(kAdamThreads), 0, st, part, blocks, max_norm, mult, norm);
}
