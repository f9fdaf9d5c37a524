// The explicit environment image of the relighting path: the lookup of one direction, shared by
// k_env_lookup and every kernel that reads the image (rc_relight.hip).  Device code only; include after rc_internal.h.
//
// render_utils.get_environment_color (render_utils.py:1552-1598) + grid_utils.jax_resample_2d (grid_utils.py:245-325,
// CONSTANT_OUTSIDE, padding 0, coordinate_order 'yx'), read literally and in fp32.  The image is the handle's PADDED copy
// [(H + 2)][(W + 2)][4] with a border of zeros (RcEnvImage): the reference pads the array and clamps the corner indices
// into the padded array, so a corner is ONE aligned 16-byte load at the clamped index, no branch on the border.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr float kEnvPi = 3.14159274f;          // float32(jnp.pi)
constexpr float kEnvTwoPi = 6.28318548f;       // float32(2 * jnp.pi)

// jnp.maximum(astype(int32), 0) then jnp.minimum(., hi) with ORDERED compares: a NaN position selects index 0 (the
// padding), never an index outside [0, hi]
__device__ __forceinline__ int env_clamp_index(float p, int hi) {
  if (!(p > 0.0f)) return 0;
  return p < (float)hi ? (int)p : hi;
}

__device__ __forceinline__ void env_lookup(const RcEnvImage& im, float dx, float dy, float dz, float out[3]) {
  // x, y, z = x, z, -y, then the identity rotation written out (R.from_quat([0, 0, 0, 1]).as_matrix(): exact zeros and
  // ones; 0 * inf = NaN makes a non-finite direction a NaN colour)
  const float x0 = dx, y0 = dz, z0 = -dy;
  const float x = 1.0f * x0 + 0.0f * y0 + 0.0f * z0;
  const float y = 0.0f * x0 + 1.0f * y0 + 0.0f * z0;
  const float z = 0.0f * x0 + 0.0f * y0 + 1.0f * z0;
  const float s = sqrtf(x * x + y * y + 1e-8f);
  const float phi = atan2f(y / (s + 1e-8f), x / (s + 1e-8f));
  const float theta = atan2f(s, z);
  // locations (row, col), + 1 for the padding
  const float col = ((-phi + kEnvPi) / kEnvTwoPi) * (float)im.W + 1.0f;
  const float row = (theta / kEnvPi) * (float)im.H + 1.0f;
  const float fr = floorf(row), fc = floorf(col);
  const float cwr = row - fr, cwc = col - fc;            // ceil_w
  const float fwr = 1.0f - cwr, fwc = 1.0f - cwc;        // floor_w
  const int r0 = env_clamp_index(fr, im.H + 1), r1 = env_clamp_index(fr + 1.0f, im.H + 1);
  const int c0 = env_clamp_index(fc, im.W + 1), c1 = env_clamp_index(fc + 1.0f, im.W + 1);
  const int64_t pitch = (int64_t)im.W + 2;
  const float4* px = reinterpret_cast<const float4*>(im.padded);
  const float4 v00 = px[r0 * pitch + c0], v01 = px[r0 * pitch + c1], v10 = px[r1 * pitch + c0], v11 = px[r1 * pitch + c1];
  const float w00 = fwr * fwc, w01 = fwr * cwc, w10 = cwr * fwc, w11 = cwr * cwc;
  // output = zeros; output += gathered * weight, the four corners in the order written there
  out[0] = (((0.0f + v00.x * w00) + v01.x * w01) + v10.x * w10) + v11.x * w11;
  out[1] = (((0.0f + v00.y * w00) + v01.y * w01) + v10.y * w10) + v11.y * w11;
  out[2] = (((0.0f + v00.z * w00) + v01.z * w01) + v10.z * w10) + v11.z * w11;
}

}  // namespace
