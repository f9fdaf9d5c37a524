// Evaluation of the albedo on the device (rc_eval_albedo, rc_albedo_ratio): the trainer's
// _compute_and_log_albedo_metrics (engine/trainer.py:1499-1567) and the ratio of _compute_albedo_ratio (:2207-2234).
//
//   k_albedo_count    one thread per pixel: the valid pixels of each workgroup (ballot, popcount)
//   k_albedo_scan     one workgroup: those counts -> the rows before each workgroup, in order; reads and advances the
//                     caller's device row count
//   k_albedo_write    the valid rows (gt'[3], p[3]) in pixel order: row = rows before the workgroup + before the wave +
//                     before the lane; a row at or behind the capacity is dropped
//   k_albedo_begin    ranks, prefixes and the histogram of a select / the row count of the least squares
//   k_albedo_hist     one radix pass of 8 bits: per-workgroup LDS histograms of the ratios' keys that match a selection's
//                     prefix, added into the global histogram (integer atomics)
//   k_albedo_narrow   one workgroup: the digit that holds each selection's rank; after the last pass the medians
//   k_albedo_lstsq, k_albedo_lstsq_finish   the closed form of the reference's block-diagonal least squares, in double
//   k_albedo_score    one thread per pixel: the ratio applied, the gamma, the squared error, the optional images
//   k_albedo_finish   the partial sums in a fixed order, the result array
//
// The only atomics add integers, whose sum does not depend on the order; every floating sum goes over per-workgroup
// partials (doubles) added in a fixed order.  Two calls on the same inputs are therefore bitwise equal.  The element-wise
// arithmetic is fp32 in the order of tests/albedo_metrics_ref.py; each clip hands a NaN on, as np.clip does.
#include <hip/hip_runtime.h>

#include "rc_dev_reduce.h"
#include "rc_internal.h"

namespace {

constexpr int kThreads = kReduceThreads;
constexpr int kPasses = 4, kDigitBits = 8;                // 4 x 8 bits of the 32-bit key
static_assert((1 << kDigitBits) == kRcAlbedoDigits && kRcAlbedoDigits == kThreads, "one thread per digit");

__device__ __forceinline__ float nan_f() { return __uint_as_float(0x7fc00000u); }

// np.clip: a NaN stays a NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float clip(float x, float lo, float hi) { return x != x ? x : fminf(fmaxf(x, lo), hi); }

struct Pixel { bool in, valid; float m; float g[3], p[3]; };

// trainer.py:1515-1525 of pixel i
__device__ __forceinline__ Pixel load_pixel(const RcAlbedoPixelArgs& a, int64_t i) {
  Pixel x;
  x.m = a.mask ? a.mask[i] : 1.0f;
  x.in = x.m > 0.0f;
  const float acc = a.acc[i];
  x.valid = x.in && acc > 0.5f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    x.g[c] = x.in ? a.albedo_gt[3 * i + c] : 1.0f;
    x.p[c] = x.in ? a.albedo[3 * i + c] + (1.0f - acc) : 1.0f;
  }
  return x;
}

__device__ __forceinline__ bool pixel_valid(const RcAlbedoPixelArgs& a, int64_t i) {
  return i < a.n_pix && (a.mask ? a.mask[i] : 1.0f) > 0.0f && a.acc[i] > 0.5f;
}

__global__ void __launch_bounds__(kThreads) k_albedo_count(RcAlbedoPixelArgs a) {
  __shared__ int waves[4];
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const unsigned long long b = __ballot(pixel_valid(a, i) ? 1 : 0);
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) a.wg[blockIdx.x] = (waves[0] + waves[1]) + (waves[2] + waves[3]);
}

// wg[b] = valid pixels of the workgroups before b (fewer than 2^31: n_pix is); the view's total; the caller's count
__global__ void __launch_bounds__(kThreads) k_albedo_scan(RcAlbedoPixelArgs a, int64_t blocks) {
  __shared__ int lds[kThreads];
  const int t = threadIdx.x;
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < blocks; b0 += kThreads) {
    const int64_t b = b0 + t;
    const int v = b < blocks ? a.wg[b] : 0;
    lds[t] = v;
    __syncthreads();
    for (int o = 1; o < kThreads; o <<= 1) {
      const int below = t >= o ? lds[t - o] : 0;
      __syncthreads();
      lds[t] += below;
      __syncthreads();
    }
    if (b < blocks) a.wg[b] = (int)(carry + (lds[t] - v));
    carry += lds[kThreads - 1];
    __syncthreads();
  }
  if (t == 0) {
    const int64_t base = a.count ? *a.count : 0;
    a.state->base = base;
    a.state->total = carry;
    if (a.count) *a.count = base + carry;
  }
}

__device__ __forceinline__ void store_row(float* dst, const Pixel& x) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    dst[c] = x.g[c];
    dst[3 + c] = x.p[c];
  }
}

__global__ void __launch_bounds__(kThreads) k_albedo_write(RcAlbedoPixelArgs a) {
  __shared__ int waves[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool valid = pixel_valid(a, i);
  const unsigned long long b = __ballot(valid ? 1 : 0);
  if (lane == 0) waves[wave] = __popcll(b);
  __syncthreads();
  if (!valid) return;
  int64_t row = a.wg[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) row += waves[w];
  const Pixel x = load_pixel(a, i);
  if (a.own) store_row(a.own + 6 * row, x);               // the workspace's buffer holds n_pix rows
  if (a.pairs) {
    const int64_t at = a.state->base + row;
    if (at >= 0 && at < a.capacity) store_row(a.pairs + 6 * at, x);
  }
}

// ---- the ratio over a pair buffer ---------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads) k_albedo_begin(RcAlbedoRatioArgs a) {
  RcAlbedoState* s = a.state;
  for (int i = threadIdx.x; i < kRcAlbedoSelections * kRcAlbedoDigits; i += kThreads) (&s->hist[0][0])[i] = 0u;
  if (threadIdx.x != 0) return;
  const int64_t m = a.count ? *a.count : s->total;
  const bool overflow = m > a.capacity;
  const int64_t rows = overflow || m < 0 ? 0 : m;           // at most the capacity, which is below 2^31
  s->overflow = overflow;
  s->rows = rows;
  for (int c = 0; c < 3; ++c) {
    s->nan[c] = 0u;
    s->prefix[2 * c] = s->prefix[2 * c + 1] = 0u;
    s->rank[2 * c] = rows ? (uint32_t)((rows - 1) / 2) : 0u;
    s->rank[2 * c + 1] = (uint32_t)(rows / 2);
    s->ratio[c] = nan_f();
    if (a.ratio) a.ratio[c] = nan_f();
  }
}

// unsigned keys in the order of the floats: negative values with every bit flipped, the others with the sign bit set
__device__ __forceinline__ uint32_t float_key(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// Pass `pass` (0: the top 8 bits): of every ratio whose key agrees with a selection's prefix in the bits above, the
// digit.  NaN ratios are counted in pass 0 and take no part: their channel's median is NaN.
__global__ void __launch_bounds__(kThreads) k_albedo_hist(RcAlbedoRatioArgs a, int pass) {
  __shared__ uint32_t h[kRcAlbedoSelections * kRcAlbedoDigits];
  __shared__ uint32_t nans[3];
  for (int i = threadIdx.x; i < kRcAlbedoSelections * kRcAlbedoDigits; i += kThreads) h[i] = 0u;
  if (threadIdx.x < 3) nans[threadIdx.x] = 0u;
  __syncthreads();
  RcAlbedoState* s = a.state;
  const int shift = 32 - kDigitBits * (pass + 1);
  const int64_t rows = s->rows;
  uint32_t prefix[kRcAlbedoSelections];
#pragma unroll
  for (int k = 0; k < kRcAlbedoSelections; ++k) prefix[k] = s->prefix[k];
  for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < rows; r += (int64_t)gridDim.x * kThreads) {
    const float* row = a.pairs + 6 * r;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float ratio = row[c] / clip(row[3 + c], 1e-6f, 1.0f);
      if (ratio != ratio) {
        if (pass == 0) atomicAdd(&nans[c], 1u);
        continue;
      }
      const uint32_t key = float_key(ratio), digit = (key >> shift) & (kRcAlbedoDigits - 1);
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int k = 2 * c + e;
        // bits above this pass's digit: a 64-bit shift, since pass 0 shifts by 32
        if (((uint64_t)(key ^ prefix[k]) >> (shift + kDigitBits)) == 0) atomicAdd(&h[k * kRcAlbedoDigits + digit], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kRcAlbedoSelections * kRcAlbedoDigits; i += kThreads)
    if (h[i]) atomicAdd(&(&s->hist[0][0])[i], h[i]);
  if (threadIdx.x < 3 && nans[threadIdx.x]) atomicAdd(&s->nan[threadIdx.x], nans[threadIdx.x]);
}

// Thread k < 6 walks selection k's histogram to the digit that holds its rank and makes the rank relative to that digit;
// the histogram is zeroed for the next pass.  After the last pass the prefixes are the order statistics' keys.
__global__ void __launch_bounds__(kThreads) k_albedo_narrow(RcAlbedoRatioArgs a, int pass) {
  __shared__ uint32_t key[kRcAlbedoSelections];
  RcAlbedoState* s = a.state;
  const int shift = 32 - kDigitBits * (pass + 1);
  if (threadIdx.x < kRcAlbedoSelections) {
    const int k = threadIdx.x;
    const uint32_t rank = s->rank[k];
    uint32_t before = 0u, d = 0u;
    for (; d < kRcAlbedoDigits - 1; ++d) {                  // without NaNs the rank lies inside the histogram
      const uint32_t n = s->hist[k][d];
      if (before + n > rank) break;
      before += n;
    }
    key[k] = s->prefix[k] | (d << shift);
    s->prefix[k] = key[k];
    s->rank[k] = rank - before;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kRcAlbedoSelections * kRcAlbedoDigits; i += kThreads) (&s->hist[0][0])[i] = 0u;
  if (pass != kPasses - 1 || threadIdx.x >= 3) return;
  const int c = threadIdx.x;
  const float lo = key_float(key[2 * c]), hi = key_float(key[2 * c + 1]);
  float m = (s->rows & 1) ? lo : (lo + hi) / 2.0f;          // np.median of float32: the mean of the middle one or two
  if (s->rows == 0 || s->nan[c] != 0u) m = nan_f();         // an overflow has rows = 0
  s->ratio[c] = m;
  if (a.ratio) a.ratio[c] = m;
}

// trainer.py:2213-2234: the system is block-diagonal, channel c solves min sum (p_c^g x - gt_c^g)^2
__global__ void __launch_bounds__(kThreads) k_albedo_lstsq(RcAlbedoRatioArgs a) {
  __shared__ double lds[4 * 6];
  const int64_t rows = a.state->rows;
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};             // sum p gt per channel, sum p p per channel
  for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < rows; r += (int64_t)gridDim.x * kThreads) {
    const float* row = a.pairs + 6 * r;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double g = (double)row[c], p = (double)row[3 + c];
      if (a.gamma) {
        g = pow(g, 1.0 / 2.2);
        p = pow(p, 1.0 / 2.2);
      }
      v[c] += p * g;
      v[3 + c] += p * p;
    }
  }
  block_sums<6>(v, lds, a.part + (int64_t)blockIdx.x * 6);
}

__global__ void __launch_bounds__(kThreads) k_albedo_lstsq_finish(RcAlbedoRatioArgs a, int blocks) {
  __shared__ double lds[kThreads];
  double v[6];
  for (int k = 0; k < 6; ++k) v[k] = ordered_sum(a.part + k, blocks, 6, lds);
  if (threadIdx.x != 0) return;
  for (int c = 0; c < 3; ++c) {
    double x = v[c] / v[3 + c];
    if (a.gamma) x = pow(x, 2.2);
    const float r = a.state->rows == 0 ? nan_f() : (float)x;
    a.state->ratio[c] = r;
    if (a.ratio) a.ratio[c] = r;
  }
}

// ---- apply and score ----------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads) k_albedo_score(RcAlbedoPixelArgs a) {
  __shared__ double lds[4];
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  double v[1] = {0.0};
  if (i < a.n_pix) {
    const Pixel x = load_pixel(a, i);
    const float inv_gamma = (float)(1.0 / 2.2);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (a.ratio_im) a.ratio_im[3 * i + c] = clip(x.g[c] / x.p[c], 0.0f, 1.0f);
      const float p = x.valid ? clip(x.p[c] * a.ratio[c], 0.0f, a.albedo_clip) : x.p[c];
      const float pa = powf(p, inv_gamma), pg = powf(x.g[c], inv_gamma);
      if (a.post_pred) a.post_pred[3 * i + c] = pa;
      if (a.post_gt) a.post_gt[3 * i + c] = pg;
      const float d = pa * x.m - pg * x.m;
      v[0] += (double)(d * d);
    }
  }
  block_sums<1>(v, lds, a.part + blockIdx.x);
}

__global__ void __launch_bounds__(kThreads) k_albedo_finish(RcAlbedoPixelArgs a, int64_t blocks) {
  __shared__ double lds[kThreads];
  const double se = ordered_sum(a.part, blocks, 1, lds);
  if (threadIdx.x != 0) return;
  const double mse = se / (3.0 * (double)a.n_pix);
  a.out[RC_ALBEDO_MSE] = mse;
  a.out[RC_ALBEDO_PSNR] = -10.0 / log(10.0) * log(mse);
  a.out[RC_ALBEDO_RATIO_R] = (double)a.ratio[0];
  a.out[RC_ALBEDO_RATIO_G] = (double)a.ratio[1];
  a.out[RC_ALBEDO_RATIO_B] = (double)a.ratio[2];
  a.out[RC_ALBEDO_VALID] = (double)a.state->total;
}

}  // namespace

int rc_albedo_pixel_blocks(int64_t n_pix) { return (int)((n_pix + kThreads - 1) / kThreads); }
int rc_albedo_row_blocks(int64_t capacity) {
  const int64_t b = (capacity + kThreads - 1) / kThreads;
  return (int)(b < 1 ? 1 : (b < 2048 ? b : 2048));
}

void rc_launch_albedo_compact(const RcAlbedoPixelArgs& a, hipStream_t stream) {
  const int blocks = rc_albedo_pixel_blocks(a.n_pix);
  hipLaunchKernelGGL(k_albedo_count, dim3(blocks), dim3(kThreads), 0, stream, a);
  hipLaunchKernelGGL(k_albedo_scan, dim3(1), dim3(kThreads), 0, stream, a, (int64_t)blocks);
  hipLaunchKernelGGL(k_albedo_write, dim3(blocks), dim3(kThreads), 0, stream, a);
}
void rc_launch_albedo_score(const RcAlbedoPixelArgs& a, hipStream_t stream) {
  const int blocks = rc_albedo_pixel_blocks(a.n_pix);
  hipLaunchKernelGGL(k_albedo_score, dim3(blocks), dim3(kThreads), 0, stream, a);
  hipLaunchKernelGGL(k_albedo_finish, dim3(1), dim3(kThreads), 0, stream, a, (int64_t)blocks);
}
void rc_launch_albedo_median(const RcAlbedoRatioArgs& a, hipStream_t stream) {
  const int blocks = rc_albedo_row_blocks(a.capacity);
  hipLaunchKernelGGL(k_albedo_begin, dim3(1), dim3(kThreads), 0, stream, a);
  for (int pass = 0; pass < kPasses; ++pass) {
    hipLaunchKernelGGL(k_albedo_hist, dim3(blocks), dim3(kThreads), 0, stream, a, pass);
    hipLaunchKernelGGL(k_albedo_narrow, dim3(1), dim3(kThreads), 0, stream, a, pass);
  }
}
void rc_launch_albedo_lstsq(const RcAlbedoRatioArgs& a, hipStream_t stream) {
  const int blocks = rc_albedo_row_blocks(a.capacity);
  hipLaunchKernelGGL(k_albedo_begin, dim3(1), dim3(kThreads), 0, stream, a);
  hipLaunchKernelGGL(k_albedo_lstsq, dim3(blocks), dim3(kThreads), 0, stream, a);
  hipLaunchKernelGGL(k_albedo_lstsq_finish, dim3(1), dim3(kThreads), 0, stream, a, blocks);
}
