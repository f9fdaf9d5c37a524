// Device pieces shared by the loss backwards (rc_interlevel.hip, rc_data.hip, rc_geometry.hip, rc_light.hip): the reverse wave scan
// of compute_alpha_weights, ref_utils.l2_normalize's override_gradient, the column order of k_density_mlp's hbuf and a few
// scalar helpers.
#pragma once
#include <hip/hip_runtime.h>

#include "rc_dev_sample.h"

namespace rcdev {

__device__ __forceinline__ float readlane_f(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }
// nan_to_num: NaN -> 0, +-inf -> +-FLT_MAX
__device__ __forceinline__ float fix_nan(float v) { return v != v ? 0.0f : fminf(fmaxf(v, -RC_FMAX), RC_FMAX); }
__device__ __forceinline__ float shfl_f(float v, int src) {
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src << 2, __builtin_bit_cast(int, v)));
}

// compute_alpha_weights backward (render.py:134-169) on one wave, one interval per lane: x = density |delta|,
// T_{k+1} = exp(-cumsum(x)_k), g = d L / d weights_k (0 on inactive lanes), w = weights_k (0 on inactive lanes).
// Returns d L / d x_k = g_k T_{k+1} - sum_{i>k} g_i w_i (the sum: an inclusive scan over the reversed lanes, read back
// one lane further); d L / d density_k = that times |delta_k|.  Every lane of the wave takes part.
__device__ __forceinline__ float alpha_weights_bwd(float g, float gw, float x, int lane) {
  const float tnext = expf(-wave_scan_incl(x, lane));
  const float rev = wave_scan_incl(shfl_f(gw, 63 - lane), lane);
  const float rev_next = shfl_f(rev, (62 - lane) & 63);
  const float after = lane < 63 ? rev_next : 0.0f;
  return g * tnext - after;
}

// ref_utils.l2_normalize's backward (override_gradient): through x / sqrt(max(eps, |x|^2)), zero where |x|^2 < tiny.
// (ux, uy, uz) = d L / d l2_normalize(p) -> d L / d p.
__device__ __forceinline__ void l2_normalize_bwd(float px, float py, float pz, float ux, float uy, float uz, float& dpx,
                                                 float& dpy, float& dpz) {
  const float s = px * px + py * py + pz * pz;
  dpx = 0.0f; dpy = 0.0f; dpz = 0.0f;
  if (!(s < RC_TINY)) {
    const float d = sqrtf(fmaxf(RC_EPS, s));
    dpx = ux / d; dpy = uy / d; dpz = uz / d;
    if (s > RC_EPS) {
      const float k = (ux * px + uy * py + uz * pz) / (d * d * d);
      dpx -= k * px; dpy -= k * py; dpz -= k * pz;
    }
  }
}

// The same backward for any grad_eps (vmf_loss_fn: 1e-5), with jnp.maximum's tie rule: at |p|^2 == grad_eps half the
// gradient reaches the squared norm.
__device__ __forceinline__ void l2_normalize_bwd_eps(float px, float py, float pz, float ux, float uy, float uz, float grad_eps,
                                                     float& dpx, float& dpy, float& dpz) {
  const float s = px * px + py * py + pz * pz;
  dpx = 0.0f; dpy = 0.0f; dpz = 0.0f;
  if (!(s < RC_TINY)) {
    const float d = sqrtf(fmaxf(grad_eps, s));
    dpx = ux / d; dpy = uy / d; dpz = uz / d;
    if (s >= grad_eps) {
      float k = (ux * px + uy * py + uz * pz) / (d * d * d);
      if (s == grad_eps) k = 0.5f * k;
      dpx -= k * px; dpy -= k * py; dpz -= k * pz;
    }
  }
}

// k_density_mlp's hbuf holds the hidden vector of each 32-point tile in MFMA accumulator order: reference column i of
// point g sits at hbuf[(g >> 5) * 2048 + hbuf_offset(i) + (g & 31)], i = 32 t + (r & 3) + 8 (r >> 2) + 4 h.
__device__ __forceinline__ int hbuf_offset(int i) {
  const int t = i >> 5, rem = i & 31, hh = (rem >> 2) & 1, r = (rem & 3) + 4 * (rem >> 3);
  return (t * 16 + r) * 64 + 32 * hh;
}

}  // namespace rcdev
