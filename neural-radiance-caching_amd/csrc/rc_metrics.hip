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

__global__ void __launch_bounds__(kEvalThreads) k_eval_ssim(RcEvalSsimArgs a) {
  __shared__ float pa[kSsimPatch][kSsimPatch + 1], pb[kSsimPatch][kSsimPatch + 1];
  __shared__ float rows[5][kSsimTile][kSsimPatch + 1];
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
  for (int t = threadIdx.x; t < kSsimTile * kSsimPatch; t += kEvalThreads) {
    const int r = t / kSsimPatch, q = t - r * kSsimPatch;
    float s[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < kSsimTaps; ++k) {
      const float w = a.taps[k], u = pa[r + k][q], v = pb[r + k][q];
      s[0] += w * u;
      s[1] += w * v;
      s[2] += w * (u * u);
      s[3] += w * (v * v);
      s[4] += w * (u * v);
    }
#pragma unroll
    for (int m = 0; m < 5; ++m) rows[m][r][q] = s[m];
  }
  __syncthreads();
  double sum = 0.0;
  for (int t = threadIdx.x; t < kSsimTile * kSsimTile; t += kEvalThreads) {
    const int r = t / kSsimTile, q = t - r * kSsimTile, y = y0 + r, x = x0 + q;
    if (y >= oh || x >= ow) continue;
    float s[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < kSsimTaps; ++k) {
      const float w = a.taps[k];
#pragma unroll
      for (int m = 0; m < 5; ++m) s[m] += w * rows[m][r][q + k];
    }
    const float mu0 = s[0], mu1 = s[1];
    const float mu00 = mu0 * mu0, mu11 = mu1 * mu1, mu01 = mu0 * mu1;
    const float eps2 = kF32Eps * kF32Eps;
    const float s00 = fmaxf(eps2, s[2] - mu00), s11 = fmaxf(eps2, s[3] - mu11);
    float s01 = s[4] - mu01;
    const float sgn = s01 > 0.0f ? 1.0f : (s01 < 0.0f ? -1.0f : 0.0f);
    s01 = sgn * fminf(sqrtf(s00 * s11), fabsf(s01));
    const float numer = (2.0f * mu01 + a.c1) * (2.0f * s01 + a.c2);
    const float denom = ((mu00 + mu11) + a.c1) * ((s00 + s11) + a.c2);
    const float val = numer / denom;
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
