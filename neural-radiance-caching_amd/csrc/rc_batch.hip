// Rays of a batch that mixes cameras, and the training batch of one step, each in one launch.
//
// k_cast_rays_multi: camera_utils.cast_ray_batch (internal/camera_utils.py:1225-1329) with the per-ray camera lookup
// `pixtocams[cam_idx]`, `camtoworlds[cam_idx]`, `lights[cam_idx]` (:1266-1288) done on the device: one lane per ray reads
// its camera's 24 floats from the tables (consecutive rays of a patch share a camera: the same cache lines) and runs the
// per-pixel body of rc_dev_camera.h, the one k_cast_rays runs.
//
// k_train_batch: Dataset._next_train + _make_ray_batch (internal/datasets.py:948-993, 850-946) for the image-shaped
// data set: per patch three words of random_bits(key, (P, 3)) -> (camera, x, y) by multiply-shift, the p x p block of
// pixel_coordinates(p, p) in row-major order, the ray of each pixel, images[cam, y, x], lossmult[cam].  The words are
// computed in the kernel (one Threefry block each, rc_dev_prng.h): nothing but the key comes from the host.
//
// Both stream: ~100 B read (tables, cached) and 30 floats + 3 ints written per ray; no LDS, no atomics.
#include "rc_internal.h"
#include "rc_dev_camera.h"
#include "rc_dev_prng.h"

namespace {

struct CamRegs { float p2c[9], rot[9], trans[3], light[3]; };

__device__ __forceinline__ CamRegs load_camera(const RcCameraTables& t, int c) {
  CamRegs r;
  const float* p = t.pixtocams + (size_t)c * 9;
  const float* w = t.camtoworlds + (size_t)c * 12;
#pragma unroll
  for (int k = 0; k < 9; ++k) r.p2c[k] = p[k];
#pragma unroll
  for (int row = 0; row < 3; ++row) {
#pragma unroll
    for (int col = 0; col < 3; ++col) r.rot[3 * row + col] = w[4 * row + col];
    r.trans[row] = w[4 * row + 3];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) r.light[k] = t.lights ? t.lights[(size_t)c * 3 + k] : r.trans[k];
  return r;
}

__device__ __forceinline__ int clamp_camera(int c, int count) { return c < 0 ? 0 : (c >= count ? count - 1 : c); }

__global__ __launch_bounds__(256) void k_cast_rays_multi(RcCastMultiArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  // memory safety only: an index outside [0, C) is the caller's error
  const CamRegs cam = load_camera(a.cams, clamp_camera(a.cam_idx[i], a.cams.count));
  const bool jit = a.pix_dx != nullptr;
  const RcCastRow row = cast_pixel(a.s, cam.p2c, cam.rot, cam.trans, a.pix_x[i], a.pix_y[i], jit, jit ? a.pix_dx[i] : 0.0f,
                                   jit ? a.pix_dy[i] : 0.0f);
  store_cast_row(a.out, i, row, cam.rot, cam.light, a.s.near_v, a.s.far_v);
}

// idx = lo + floor(w * range / 2^32): exact in 64-bit integers, no rejection loop, bias <= range / 2^32
__device__ __forceinline__ int pick(uint32_t w, int lo, int range) { return lo + (int)(((uint64_t)w * (uint32_t)range) >> 32); }

__global__ __launch_bounds__(256) void k_train_batch(RcTrainBatchArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const int pp = a.patch * a.patch;
  const uint32_t q = (uint32_t)(i / pp);                      // patch
  const int j = (int)(i - (int64_t)q * pp);                   // pixel of the patch, row-major
  const uint32_t w_cam = prng_bits_at(a.key0, a.key1, a.single_image ? 0u : 3u * q, a.n_words);
  const uint32_t w_x = prng_bits_at(a.key0, a.key1, 3u * q + 1u, a.n_words);
  const uint32_t w_y = prng_bits_at(a.key0, a.key1, 3u * q + 2u, a.n_words);
  const int c = pick(w_cam, 0, a.cams.count);
  const int px = pick(w_x, a.x_lo, a.x_range) + j % a.patch;  // pixel_coordinates(p, p): dx = column, dy = row
  const int py = pick(w_y, a.y_lo, a.y_range) + j / a.patch;
  const CamRegs cam = load_camera(a.cams, c);
  const bool jit = a.pix_dx != nullptr;
  const RcCastRow row = cast_pixel(a.s, cam.p2c, cam.rot, cam.trans, px, py, jit, jit ? a.pix_dx[i] : 0.0f, jit ? a.pix_dy[i] : 0.0f);
  store_cast_row(a.out, i, row, cam.rot, cam.light, a.s.near_v, a.s.far_v);
  if (a.rgb) {
    // the host validated 0 <= x < W, 0 <= y < H for every admissible pick
    const size_t at = (((size_t)c * a.height + py) * a.width + px) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      a.rgb[3 * i + k] = a.image_u8 ? (float)((const uint8_t*)a.images)[at + k] / 255.0f : ((const float*)a.images)[at + k];
  }
  if (a.lossmult) a.lossmult[i] = a.cam_lossmult ? a.cam_lossmult[c] : 1.0f;
  if (a.cam_idx) a.cam_idx[i] = c;
  if (a.pix_x) a.pix_x[i] = px;
  if (a.pix_y) a.pix_y[i] = py;
}

}  // namespace

void rc_launch_cast_rays_multi(const RcCastMultiArgs& a, hipStream_t stream) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_cast_rays_multi, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, stream, a);
}

void rc_launch_train_batch(const RcTrainBatchArgs& a, hipStream_t stream) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_train_batch, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, stream, a);
}
