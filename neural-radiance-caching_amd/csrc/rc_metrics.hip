// Evaluation of a rendered view on the device (rc_eval_image): the trainer's postprocess_fn
// (engine/trainer.py:617-637), image.MetricHarness' PSNR and dm_pix.ssim (internal/image_utils.py:411-489), the transient
// IoU (trainer.py:1633-1636), the depth L1 errors (:1766-1779) and the normals' mean angular error (:1810-1855).
//
//   k_eval_bins    [H W][n_bins][3] x 2 -> per pixel and channel the sum over the bins of both arrays, and the partial
//                  sums of min / max over all elements (the IoU): ONE pass over the two histograms, 16-byte loads
//   k_eval_pixels  one thread per pixel: post-process of both images, squared error, depth L1, normal error
//   k_eval_ssim    one workgroup per 32 x 32 tile of the valid window and channel: the five Gaussian moments, the map
//   k_eval_finish  every partial sum added in a fixed order in double, the result array
//
// and the shift-invariant PSNR / SSIM (rc_eval_shift_invariant, §4.16.1; image_utils.py:74-189), per di row of shifts:
//
//   k_si_metric    the metric map of each shift of the row: squared error per pixel, or k_eval_ssim's tile body on the
//                  reflect-padded pair with the prediction read through the shift
//   k_si_select    one workgroup per 32 x 32 tile: box pooling of each map, the >= / <= comparison, the search state
//   k_si_finish    the partial sums of both searches in a fixed order in double, the result array
//
// No float atomics anywhere: a workgroup writes its partial sums (doubles) to its own slots and k_eval_finish adds them in
// a fixed order, so two calls on the same inputs are bitwise equal.  The element-wise arithmetic is fp32 in the order of
// tests/eval_metrics_ref.py (-ffp-contract=off keeps multiply and add apart).
#include <hip/hip_runtime.h>

#include "rc_dev_reduce.h"
#include "rc_internal.h"

namespace {

constexpr int kEvalThreads = kReduceThreads;
constexpr float kF32Eps = 1.1920928955078125e-07f;      // np.finfo(np.float32).eps

__device__ __forceinline__ float wave_sum_f(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// x added to the channel c (0, 1, 2) of s, without a dynamically indexed array
__device__ __forceinline__ void add_channel(float (&s)[3], int c, float x) {
  s[0] += c == 0 ? x : 0.0f;
  s[1] += c == 1 ? x : 0.0f;
  s[2] += c == 2 ? x : 0.0f;
}

// One wave per pixel (grid-stride): the row of 3 n_bins floats of both arrays is read once.  Where both rows reach a
// 16-byte boundary after the same number of floats (vec_ok, the same for every pixel of a call) the body goes through
// float4 loads, and the head before the boundary and the tail behind the last whole float4 through scalar ones; otherwise
// the whole row is "head".  Element e of a row belongs to channel e % 3.
__global__ void __launch_bounds__(kEvalThreads) k_eval_bins(RcEvalBinsArgs a) {
  __shared__ double lds[4 * 2];
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
  const int row = 3 * a.n_bins;
  double acc[2] = {0.0, 0.0};               // sum of min, sum of max: per lane over this wave's pixels
  for (int64_t pix = wave; pix < a.n_pix; pix += nwaves) {
    const float* p = a.pred + pix * row;
    const float* g = a.gt + pix * row;
    int head = row;
    if (a.vec_ok) {
      head = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
      if (head > row) head = row;
    }
    const int nvec = (row - head) >> 2, tail0 = head + 4 * nvec, nscalar = head + (row - tail0);
    float sp[3] = {0.0f, 0.0f, 0.0f}, sg[3] = {0.0f, 0.0f, 0.0f};
    float smin = 0.0f, smax = 0.0f;
    for (int e = lane; e < nscalar; e += 64) {
      const int idx = e < head ? e : tail0 + (e - head);
      const float x = p[idx], y = g[idx];
      add_channel(sp, idx % 3, x);
      add_channel(sg, idx % 3, y);
      smin += fminf(x, y);
      smax += fmaxf(x, y);
    }
    for (int v = lane; v < nvec; v += 64) {
      const int idx = head + 4 * v;
      const float4 x = *reinterpret_cast<const float4*>(p + idx);
      const float4 y = *reinterpret_cast<const float4*>(g + idx);
      const int c0 = idx % 3, c1 = c0 == 2 ? 0 : c0 + 1, c2 = c1 == 2 ? 0 : c1 + 1;   // channels of .x (and .w), .y, .z
      add_channel(sp, c0, x.x + x.w);
      add_channel(sp, c1, x.y);
      add_channel(sp, c2, x.z);
      add_channel(sg, c0, y.x + y.w);
      add_channel(sg, c1, y.y);
      add_channel(sg, c2, y.z);
      smin += (fminf(x.x, y.x) + fminf(x.y, y.y)) + (fminf(x.z, y.z) + fminf(x.w, y.w));
      smax += (fmaxf(x.x, y.x) + fmaxf(x.y, y.y)) + (fmaxf(x.z, y.z) + fmaxf(x.w, y.w));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float tp = wave_sum_f(sp[c]), tg = wave_sum_f(sg[c]);
      if (lane == 0) {
        a.binsum_pred[3 * pix + c] = tp;
        a.binsum_gt[3 * pix + c] = tg;
      }
    }
    acc[0] += (double)smin;
    acc[1] += (double)smax;
  }
  block_sums<2>(acc, lds, a.part + (int64_t)blockIdx.x * 2);
}

// image_utils.linear_to_srgb (internal/image_utils.py:192-198) with eps = float32's
__device__ __forceinline__ float linear_to_srgb(float x) {
  const float srgb0 = (float)(323.0 / 25.0) * x;
  const float srgb1 = ((211.0f * powf(fmaxf(kF32Eps, x), (float)(5.0 / 12.0))) - 11.0f) / 200.0f;
  return x <= 0.0031308f ? srgb0 : srgb1;
}

// postprocess_fn of one value (trainer.py:617-637): bins -> clip(binsum / img_scale, 0, 1); linear_to_srgb(x exposure);
// clip to [0, 1] under clip_eval (a.skip: neither of the two); then the mask
__device__ __forceinline__ float post_process(float x, const RcEvalPixelArgs& a, float m) {
  if (a.bins) x = fminf(fmaxf(x / a.img_scale, 0.0f), 1.0f);
  float y = a.skip ? x : linear_to_srgb(x * a.exposure);
  if (a.clip_eval && !a.skip) y = fminf(fmaxf(y, 0.0f), 1.0f);
  return a.mask ? y * m : y;
}

// n + shift, normalised, or zero where its norm is below 1e-5 (trainer.py:1819-1840)
__device__ __forceinline__ void shifted_unit(const float* n, float shift, float (&u)[3]) {
  const float x = n[0] + shift, y = n[1] + shift, z = n[2] + shift;
  const float norm = sqrtf((x * x + y * y) + z * z);
  const bool zero = norm < 1e-5f;
  u[0] = zero ? 0.0f : x / norm;
  u[1] = zero ? 0.0f : y / norm;
  u[2] = zero ? 0.0f : z / norm;
}

// partial sums of a workgroup of k_eval_pixels
enum { EP_SE, EP_L1_MEAN, EP_L1_MEDIAN, EP_MASK, EP_MAE, EP_COUNT };

__global__ void __launch_bounds__(kEvalThreads) k_eval_pixels(RcEvalPixelArgs a) {
  __shared__ double lds[4 * EP_COUNT];
  const int64_t i = (int64_t)blockIdx.x * kEvalThreads + threadIdx.x;
  double v[EP_COUNT] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (i < a.n_pix) {
    const float m = a.mask ? a.mask[i] : 1.0f;
    float se = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float p = post_process(a.pred[3 * i + c], a, m), g = post_process(a.gt[3 * i + c], a, m);
      a.post_pred[3 * i + c] = p;
      a.post_gt[3 * i + c] = g;
      const float d = p - g;
      se += d * d;
    }
    v[EP_SE] = (double)se;
    v[EP_MASK] = (double)m;
    if (a.depth_gt) {
      const float d = a.depth_gt[i];
      if (a.distance_mean) v[EP_L1_MEAN] = (double)(fabsf(a.distance_mean[i] - d) * m);
      if (a.distance_median) v[EP_L1_MEDIAN] = (double)(fabsf(a.distance_median[i] - d) * m);
    }
    if (a.normals) {
      float ug[3], up[3];
      shifted_unit(a.normals_gt + 3 * i, 1.0f - m, ug);
      shifted_unit(a.normals + 3 * i, 1.0f - a.acc[i], up);
      const float dot = (ug[0] * up[0] + ug[1] * up[1]) + ug[2] * up[2];
      const float deg = acosf(fminf(fmaxf(dot, -1.0f), 1.0f)) * 180.0f / 3.14159265358979323846f;
      v[EP_MAE] = (double)(a.mask ? deg * m : deg);
    }
  }
  block_sums<EP_COUNT>(v, lds, a.part + (int64_t)blockIdx.x * EP_COUNT);
}

// dm_pix.ssim with its defaults on one 32 x 32 tile of the valid window [H - 10][W - 10] of one channel.  The 42 x 42
// patches of both images go to LDS (zeros outside the image: they only reach outputs outside the window, which are
// dropped), the pass along H of the five moments a, b, a^2, b^2, ab to LDS, the pass along W runs in registers.
constexpr int kSsimTile = 32, kSsimTaps = 11, kSsimPatch = kSsimTile + kSsimTaps - 1;

using SsimPatch = float[kSsimPatch][kSsimPatch + 1];
using SsimRows = float[5][kSsimTile][kSsimPatch + 1];

// The moments by index: E[a], E[b], E[a^2], E[b^2], E[ab].  MASK (bit m: moment m) picks those a pass computes: all five
// in k_eval_ssim; in k_si_metric the two of the ground truth once for several shifts, the other three per shift.  Every
// moment is a sum of its own, so a value does not depend on which pass computed its moments.
constexpr int kSsimAll = 31, kSsimOfB = (1 << 1) | (1 << 3), kSsimOfA = kSsimAll & ~kSsimOfB;

// The pass along H of a tile: patches -> rows, the 11 products of a moment added in tap order.
template <int MASK>
__device__ __forceinline__ void ssim_pass_h(const SsimPatch& pa, const SsimPatch& pb, SsimRows& rows, const float (&taps)[kSsimTaps]) {
  for (int t = threadIdx.x; t < kSsimTile * kSsimPatch; t += kEvalThreads) {
    const int r = t / kSsimPatch, q = t - r * kSsimPatch;
    float s[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < kSsimTaps; ++k) {
      const float w = taps[k], v = pb[r + k][q];
      const float u = (MASK & kSsimOfA) ? pa[r + k][q] : 0.0f;
      if (MASK & 1) s[0] += w * u;
      if (MASK & 2) s[1] += w * v;
      if (MASK & 4) s[2] += w * (u * u);
      if (MASK & 8) s[3] += w * (v * v);
      if (MASK & 16) s[4] += w * (u * v);
    }
#pragma unroll
    for (int m = 0; m < 5; ++m)
      if (MASK & (1 << m)) rows[m][r][q] = s[m];
  }
}

// The pass along W at (r, q) of a tile, in registers: the moments of MASK into s, the others are left as they are.
template <int MASK>
__device__ __forceinline__ void ssim_pass_w(const SsimRows& rows, int r, int q, const float (&taps)[kSsimTaps], float (&s)[5]) {
#pragma unroll
  for (int m = 0; m < 5; ++m)
    if (MASK & (1 << m)) s[m] = 0.0f;
#pragma unroll
  for (int k = 0; k < kSsimTaps; ++k) {
    const float w = taps[k];
#pragma unroll
    for (int m = 0; m < 5; ++m)
      if (MASK & (1 << m)) s[m] += w * rows[m][r][q + k];
  }
}

// dm_pix.ssim's value of the five moments
__device__ __forceinline__ float ssim_of_moments(const float (&s)[5], float c1, float c2) {
  const float mu0 = s[0], mu1 = s[1];
  const float mu00 = mu0 * mu0, mu11 = mu1 * mu1, mu01 = mu0 * mu1;
  const float eps2 = kF32Eps * kF32Eps;
  const float s00 = fmaxf(eps2, s[2] - mu00), s11 = fmaxf(eps2, s[3] - mu11);
  float s01 = s[4] - mu01;
  const float sgn = s01 > 0.0f ? 1.0f : (s01 < 0.0f ? -1.0f : 0.0f);
  s01 = sgn * fminf(sqrtf(s00 * s11), fabsf(s01));
  const float numer = (2.0f * mu01 + c1) * (2.0f * s01 + c2);
  const float denom = ((mu00 + mu11) + c1) * ((s00 + s11) + c2);
  return numer / denom;
}

__device__ __forceinline__ float ssim_value(const SsimRows& rows, int r, int q, const float (&taps)[kSsimTaps], float c1, float c2) {
  float s[5];
  ssim_pass_w<kSsimAll>(rows, r, q, taps, s);
  return ssim_of_moments(s, c1, c2);
}

__global__ void __launch_bounds__(kEvalThreads) k_eval_ssim(RcEvalSsimArgs a) {
  __shared__ SsimPatch pa, pb;
  __shared__ SsimRows rows;
  __shared__ double lds[4];
  const int c = blockIdx.z, y0 = blockIdx.y * kSsimTile, x0 = blockIdx.x * kSsimTile;
  const int oh = a.height - (kSsimTaps - 1), ow = a.width - (kSsimTaps - 1);
  for (int t = threadIdx.x; t < kSsimPatch * kSsimPatch; t += kEvalThreads) {
    const int r = t / kSsimPatch, q = t - r * kSsimPatch, y = y0 + r, x = x0 + q;
    const bool in = y < a.height && x < a.width;
    const int64_t at = ((int64_t)y * a.width + x) * 3 + c;
    pa[r][q] = in ? a.a[at] : 0.0f;
    pb[r][q] = in ? a.b[at] : 0.0f;
  }
  __syncthreads();
  ssim_pass_h<kSsimAll>(pa, pb, rows, a.taps);
  __syncthreads();
  double sum = 0.0;
  for (int t = threadIdx.x; t < kSsimTile * kSsimTile; t += kEvalThreads) {
    const int r = t / kSsimTile, q = t - r * kSsimTile, y = y0 + r, x = x0 + q;
    if (y >= oh || x >= ow) continue;
    const float val = ssim_value(rows, r, q, a.taps, a.c1, a.c2);
    if (a.map) a.map[((int64_t)y * ow + x) * 3 + c] = val;
    sum += (double)val;
  }
  double v[1] = {sum};
  block_sums<1>(v, lds, a.part + ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
}

__global__ void __launch_bounds__(kEvalThreads) k_eval_finish(RcEvalFinishArgs a) {
  __shared__ double lds[kEvalThreads];
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double n = (double)a.n_pix;
  double px[EP_COUNT];
  for (int k = 0; k < EP_COUNT; ++k) px[k] = ordered_sum(a.part_pixels + k, a.n_part_pixels, EP_COUNT, lds);
  const double ssim = a.n_part_ssim ? ordered_sum(a.part_ssim, a.n_part_ssim, 1, lds) : 0.0;
  const double imin = a.n_part_bins ? ordered_sum(a.part_bins, a.n_part_bins, 2, lds) : 0.0;
  const double imax = a.n_part_bins ? ordered_sum(a.part_bins + 1, a.n_part_bins, 2, lds) : 0.0;
  if (threadIdx.x != 0) return;
  const double mse = px[EP_SE] / (3.0 * n);
  const double den = a.masked ? px[EP_MASK] : n;          // depth: the mask's sum, or a plain mean
  a.out[RC_EVAL_MSE] = mse;
  a.out[RC_EVAL_PSNR] = -10.0 / log(10.0) * log(mse);
  a.out[RC_EVAL_SSIM] = a.n_part_ssim ? ssim / a.ssim_count : nan;
  a.out[RC_EVAL_TRANSIENT_IOU] = a.n_part_bins ? imin / imax : nan;
  a.out[RC_EVAL_L1_MEAN] = a.have_l1_mean ? px[EP_L1_MEAN] / den : nan;
  a.out[RC_EVAL_L1_MEDIAN] = a.have_l1_median ? px[EP_L1_MEDIAN] / den : nan;
  a.out[RC_EVAL_MAE] = a.have_mae ? px[EP_MAE] / n : nan;   // over ALL pixels, as the reference's np.mean
}

// ---- shift-invariant PSNR / SSIM (rc_eval_shift_invariant) -------------------------------------------

// numpy's "reflect" (no edge repeat) of an index that is at most n - 1 outside [0, n)
__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i > n - 1 ? 2 * (n - 1) - i : i); }

// The metric map of every shift (a.di, dj) of a group, shift s = dj + radius_j into metric[s][H][W].
//   mse:  one thread per pixel and shift (blockIdx.z): ((d_0^2 + d_1^2) + d_2^2) / 3 of d = pred[R(y + di)][R(x + dj)] - gt[y][x]
//   ssim: one workgroup per 32 x 32 tile of the [H][W] map, which is the valid window of the two images reflect-padded by
//         5, and batch of kSiBatch shifts (blockIdx.z): k_eval_ssim's tile body per channel on patches gathered through
//         the index maps -- the ground truth's patch and its two moments once per batch, the prediction's patch and the
//         three moments it enters per shift -- and the channel mean in registers
constexpr int kSiBatch = 3;
template <int KIND>
__global__ void __launch_bounds__(kEvalThreads) k_si_metric(RcSiMetricArgs a) {
  if constexpr (KIND == RC_SI_MSE) {
    const int dj = (int)blockIdx.z - a.radius_j;
    float* out = a.metric + (int64_t)blockIdx.z * a.height * a.width;
    const int64_t i = (int64_t)blockIdx.x * kEvalThreads + threadIdx.x;
    if (i >= (int64_t)a.height * a.width) return;
    const int y = (int)(i / a.width), x = (int)(i - (int64_t)y * a.width);
    const float* p = a.pred + ((int64_t)reflect(y + a.di, a.height) * a.width + reflect(x + dj, a.width)) * 3;
    const float* g = a.gt + i * 3;
    const float d0 = p[0] - g[0], d1 = p[1] - g[1], d2 = p[2] - g[2];
    out[i] = ((d0 * d0 + d1 * d1) + d2 * d2) / 3.0f;
  } else {
    __shared__ SsimPatch pa, pb;
    __shared__ SsimRows rows;
    constexpr int kPer = kSsimTile * kSsimTile / kEvalThreads;
    const int y0 = blockIdx.y * kSsimTile, x0 = blockIdx.x * kSsimTile;
    const int ph = a.height + (kSsimTaps - 1), pw = a.width + (kSsimTaps - 1);      // the padded images
    const int s0 = (int)blockIdx.z * kSiBatch;                                       // this workgroup's shifts: s0 ..
    const int ns = min(kSiBatch, 2 * a.radius_j + 1 - s0);
    float acc[kSiBatch][kPer];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      // the ground truth's patch and its two moments, once for the batch
      for (int t = threadIdx.x; t < kSsimPatch * kSsimPatch; t += kEvalThreads) {
        const int r = t / kSsimPatch, q = t - r * kSsimPatch, y = y0 + r, x = x0 + q;
        float v = 0.0f;                        // beyond the padded image: reaches only outputs outside the map
        if (y < ph && x < pw) {
          const int yg = reflect(y - kSsimTaps / 2, a.height), xg = reflect(x - kSsimTaps / 2, a.width);
          v = a.gt[((int64_t)yg * a.width + xg) * 3 + c];
        }
        pb[r][q] = v;
      }
      __syncthreads();                         // also: the previous channel's last pass along W has read `rows`
      ssim_pass_h<kSsimOfB>(pa, pb, rows, a.taps);
      __syncthreads();
      float mom[kPer][5];
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const int t = threadIdx.x + j * kEvalThreads, r = t / kSsimTile, q = t - r * kSsimTile;
        ssim_pass_w<kSsimOfB>(rows, r, q, a.taps, mom[j]);
      }
#pragma unroll
      for (int b = 0; b < kSiBatch; ++b) {
        if (b >= ns) break;
        const int dj = s0 + b - a.radius_j;
        for (int t = threadIdx.x; t < kSsimPatch * kSsimPatch; t += kEvalThreads) {
          const int r = t / kSsimPatch, q = t - r * kSsimPatch, y = y0 + r, x = x0 + q;
          float u = 0.0f;
          if (y < ph && x < pw) {
            const int yg = reflect(y - kSsimTaps / 2, a.height), xg = reflect(x - kSsimTaps / 2, a.width);
            const int yp = reflect(yg + a.di, a.height), xp = reflect(xg + dj, a.width);
            u = a.pred[((int64_t)yp * a.width + xp) * 3 + c];
          }
          pa[r][q] = u;                        // the previous shift's pass along H is behind a barrier
        }
        __syncthreads();                       // also: the previous shift's pass along W has read `rows`
        ssim_pass_h<kSsimOfA>(pa, pb, rows, a.taps);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
          const int t = threadIdx.x + j * kEvalThreads, r = t / kSsimTile, q = t - r * kSsimTile;
          ssim_pass_w<kSsimOfA>(rows, r, q, a.taps, mom[j]);
          const float val = ssim_of_moments(mom[j], a.c1, a.c2);
          acc[b][j] = c == 0 ? val : acc[b][j] + val;
        }
      }
    }
#pragma unroll
    for (int b = 0; b < kSiBatch; ++b) {
      if (b >= ns) break;
      float* out = a.metric + (int64_t)(s0 + b) * a.height * a.width;
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const int t = threadIdx.x + j * kEvalThreads, r = t / kSsimTile, q = t - r * kSsimTile, y = y0 + r, x = x0 + q;
        if (y < a.height && x < a.width) out[(int64_t)y * a.width + x] = acc[b][j] / 3.0f;
      }
    }
  }
}

// Pooling and selection over the shifts of a group, one workgroup per 32 x 32 tile.  Per shift: the tile plus a halo of hw
// from its metric map to LDS (zeros outside the image), the sums over 2 hw + 1 rows, then over 2 hw + 1 columns, taps in
// increasing order, one division; then the comparison.  Every shift goes through the same additions, zeros included, so
// pooled values that tie exactly in the restatement tie exactly here.  The state lives in registers within a group and in
// the [H][W] arrays between groups.
constexpr int kSiTile = 32, kSiMaxPatch = kSiTile + 2 * RC_EVAL_SI_MAX_HALFWIDTH;

template <int KIND>
__global__ void __launch_bounds__(kEvalThreads) k_si_select(RcSiSelectArgs a) {
  __shared__ float patch[kSiMaxPatch][kSiMaxPatch + 1];
  __shared__ float cols[kSiTile][kSiMaxPatch + 1];
  __shared__ double lds[4];
  constexpr int kPer = kSiTile * kSiTile / kEvalThreads;
  const int hw = a.halfwidth, taps = 2 * hw + 1, side = kSiTile + 2 * hw;
  const int y0 = blockIdx.y * kSiTile, x0 = blockIdx.x * kSiTile;
  const float area = (float)(taps * taps);
  const int64_t n_pix = (int64_t)a.height * a.width;
  float bp[kPer], bm[kPer];
  int bi[kPer], bj[kPer];
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int t = threadIdx.x + j * kEvalThreads, r = t / kSiTile, q = t - r * kSiTile, y = y0 + r, x = x0 + q;
    const bool in = y < a.height && x < a.width && !a.first;
    const int64_t at = (int64_t)y * a.width + x;
    bp[j] = in ? a.best_pooled[at] : 0.0f;
    bm[j] = in ? a.best_metric[at] : 0.0f;
    bi[j] = in ? a.best_di[at] : 0;
    bj[j] = in ? a.best_dj[at] : 0;
  }
  for (int s = 0; s <= 2 * a.radius_j; ++s) {
    const float* m = a.metric + (int64_t)s * n_pix;
    __syncthreads();                          // the previous shift's patch and sums have been read
    for (int t = threadIdx.x; t < side * side; t += kEvalThreads) {
      const int r = t / side, q = t - r * side, y = y0 - hw + r, x = x0 - hw + q;
      patch[r][q] = (y >= 0 && y < a.height && x >= 0 && x < a.width) ? m[(int64_t)y * a.width + x] : 0.0f;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < kSiTile * side; t += kEvalThreads) {
      const int r = t / side, q = t - r * side;
      float sum = 0.0f;
      for (int k = 0; k < taps; ++k) sum += patch[r + k][q];
      cols[r][q] = sum;
    }
    __syncthreads();
    const bool take_all = a.first && s == 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int t = threadIdx.x + j * kEvalThreads, r = t / kSiTile, q = t - r * kSiTile;
      float sum = 0.0f;
      for (int k = 0; k < taps; ++k) sum += cols[r][q + k];
      const float pooled = sum / area;
      const bool take = take_all || (KIND == RC_SI_SSIM ? pooled >= bp[j] : pooled <= bp[j]);
      bp[j] = take ? pooled : bp[j];
      bm[j] = take ? patch[r + hw][q + hw] : bm[j];
      bi[j] = take ? a.di : bi[j];
      bj[j] = take ? s - a.radius_j : bj[j];
    }
  }
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int t = threadIdx.x + j * kEvalThreads, r = t / kSiTile, q = t - r * kSiTile, y = y0 + r, x = x0 + q;
    if (y >= a.height || x >= a.width) continue;
    const int64_t at = (int64_t)y * a.width + x;
    if (!a.last) {
      a.best_pooled[at] = bp[j];
      a.best_metric[at] = bm[j];
      a.best_di[at] = bi[j];
      a.best_dj[at] = bj[j];
      continue;
    }
    if (a.out_map) a.out_map[at] = bm[j];
    if (a.out_di) a.out_di[at] = bi[j];
    if (a.out_dj) a.out_dj[at] = bj[j];
    if (y >= a.crop && y < a.height - a.crop && x >= a.crop && x < a.width - a.crop) sum += (double)bm[j];
  }
  if (a.last) {
    double v[1] = {sum};
    block_sums<1>(v, lds, a.part + (int64_t)blockIdx.y * gridDim.x + blockIdx.x);
  }
}

__global__ void __launch_bounds__(kEvalThreads) k_si_finish(RcSiFinishArgs a) {
  __shared__ double lds[kEvalThreads];
  const double mse_sum = ordered_sum(a.part_mse, a.n_part, 1, lds);
  const double ssim_sum = a.part_ssim ? ordered_sum(a.part_ssim, a.n_part, 1, lds) : 0.0;
  if (threadIdx.x != 0) return;
  const double mse = mse_sum / a.n_mse;
  a.out[RC_EVAL_SI_MSE] = mse;
  a.out[RC_EVAL_SI_PSNR] = -10.0 / log(10.0) * log(mse);
  a.out[RC_EVAL_SI_SSIM] = a.part_ssim ? ssim_sum / a.n_ssim : __longlong_as_double(0x7ff8000000000000LL);
}

}  // namespace

int rc_eval_bins_blocks(int64_t n_pix) {
  const int64_t b = (n_pix + 3) / 4;
  return (int)(b < 2048 ? b : 2048);
}
int rc_eval_pixel_blocks(int64_t n_pix) { return (int)((n_pix + kEvalThreads - 1) / kEvalThreads); }
int rc_eval_pixel_parts() { return EP_COUNT; }
void rc_eval_ssim_tiles(int height, int width, int* ty, int* tx) {
  *ty = (height - (kSsimTaps - 1) + kSsimTile - 1) / kSsimTile;
  *tx = (width - (kSsimTaps - 1) + kSsimTile - 1) / kSsimTile;
}

void rc_launch_eval_bins(const RcEvalBinsArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_eval_bins, dim3(rc_eval_bins_blocks(a.n_pix)), dim3(kEvalThreads), 0, stream, a);
}
void rc_launch_eval_pixels(const RcEvalPixelArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_eval_pixels, dim3(rc_eval_pixel_blocks(a.n_pix)), dim3(kEvalThreads), 0, stream, a);
}
void rc_launch_eval_ssim(const RcEvalSsimArgs& a, hipStream_t stream) {
  int ty, tx;
  rc_eval_ssim_tiles(a.height, a.width, &ty, &tx);
  hipLaunchKernelGGL(k_eval_ssim, dim3(tx, ty, 3), dim3(kEvalThreads), 0, stream, a);
}
void rc_launch_eval_finish(const RcEvalFinishArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_eval_finish, dim3(1), dim3(kEvalThreads), 0, stream, a);
}

static_assert(kSiTile == kSsimTile, "k_si_metric and k_si_select share rc_si_tiles");
void rc_si_tiles(int height, int width, int* ty, int* tx) {
  *ty = (height + kSiTile - 1) / kSiTile;
  *tx = (width + kSiTile - 1) / kSiTile;
}
void rc_launch_si_metric(int kind, const RcSiMetricArgs& a, hipStream_t stream) {
  const int nj = 2 * a.radius_j + 1;
  if (kind == RC_SI_MSE) {
    hipLaunchKernelGGL(k_si_metric<RC_SI_MSE>, dim3(rc_eval_pixel_blocks((int64_t)a.height * a.width), 1, nj), dim3(kEvalThreads), 0, stream, a);
    return;
  }
  int ty, tx;
  rc_si_tiles(a.height, a.width, &ty, &tx);
  hipLaunchKernelGGL(k_si_metric<RC_SI_SSIM>, dim3(tx, ty, (nj + kSiBatch - 1) / kSiBatch), dim3(kEvalThreads), 0, stream, a);
}
void rc_launch_si_select(int kind, const RcSiSelectArgs& a, hipStream_t stream) {
  int ty, tx;
  rc_si_tiles(a.height, a.width, &ty, &tx);
  if (kind == RC_SI_MSE) hipLaunchKernelGGL(k_si_select<RC_SI_MSE>, dim3(tx, ty), dim3(kEvalThreads), 0, stream, a);
  else hipLaunchKernelGGL(k_si_select<RC_SI_SSIM>, dim3(tx, ty), dim3(kEvalThreads), 0, stream, a);
}
void rc_launch_si_finish(const RcSiFinishArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_si_finish, dim3(1), dim3(kEvalThreads), 0, stream, a);
}
