// The colour arithmetic of a picture's value, shared by the kernels that write pictures: rc_vis.hip (the visualisation
// suite) and rc_probe.hip (the vMF panorama).  Every caller inlines the same operations, so a value does not depend on
// which kernel drew it.
#pragma once
#include "rc_internal.h"

constexpr float kF32Eps = 1.1920928955078125e-07f;        // np.finfo(np.float32).eps
constexpr float kF32Max = 3.4028234663852886e+38f;

// np.clip / jnp.clip: a NaN stays a NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float clip(float x, float lo, float hi) { return x != x ? x : fminf(fmaxf(x, lo), hi); }

// image.linear_to_srgb (internal/image.py:192-200) with eps = float32's under jnp: jnp.maximum hands a NaN on
__device__ __forceinline__ float linear_to_srgb(float x) {
  if (x != x) return x;
  const float srgb0 = (float)(323.0 / 25.0) * x;
  const float srgb1 = ((211.0f * powf(fmaxf(kF32Eps, x), (float)(5.0 / 12.0))) - 11.0f) / 200.0f;
  return x <= 0.0031308f ? srgb0 : srgb1;
}

__device__ __forceinline__ float nan_to_num(float x) {
  if (x != x) return 0.0f;
  return fminf(fmaxf(x, -kF32Max), kF32Max);
}

// utils.save_img_u8: round(clip(nan_to_num(x), 0, 1) * 255), half to even
__device__ __forceinline__ uint8_t save_u8(float x) { return (uint8_t)rintf(clip(nan_to_num(x), 0.0f, 1.0f) * 255.0f); }
