// Mask loss of the cache stage on the last sampler level's opacity, and the rays of its backward term.
//
// train_utils.compute_mask_loss (internal/train_utils.py:785-836), per ray with acc = sum of the last level's weights
// (render.py:202):
//   loss = mean(lossmult * wt * sqrt((acc - m)^2 + charb_padding^2)),  wt = m > 0.5 ? weight_opaque : weight_empty
// (the decay / ease schedules, train_utils.py:897-932, are folded into the two weights by the caller).  The backward
// term (train_utils.py:2929-2945) is the same loss with m = 0 and weights (0, backward_mask_loss_weight) on the rays of
// _compute_backward_mask_loss (train_utils.py:3348-3401): one ray per batch ray from shadow_near_max in front of the
// camera, its direction drawn uniformly from the hemisphere around -look
// (render_utils.get_secondary_rays :927-1056 with UniformHemisphereSampler :395-403, one sample, no MIS).
//
// Kernels:
//   k_backward_mask_rays  one thread per ray: origin, direction (= viewdir), near, far of the backward ray.
//   k_mask_loss_bwd       one wave per ray, one lane per interval: the last level's weights (written to the workspace:
//                         the training forward stops behind the density MLP), acc by a wave sum, the per-ray term
//                         (loss_ray [n], reduced in a fixed order by k_interlevel_reduce), g = d L / d acc = d L / d
//                         weights_s for every interval, d L / d density by the reverse wave scan (alpha_weights_bwd).
// fp32 throughout; no float atomics, no scratch, no MFMA.
#include <hip/hip_runtime.h>

#include "rc_dev_bwd.h"
#include "rc_internal.h"
#include "rc_dev_material.h"

using namespace rcdev;

namespace {

constexpr float kPi = 3.14159265358979323846f;

__global__ void __launch_bounds__(256) k_backward_mask_rays(RcBackwardMaskRaysArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const V3 o{a.origins[3 * i], a.origins[3 * i + 1], a.origins[3 * i + 2]};
  const V3 look{a.look[3 * i], a.look[3 * i + 1], a.look[3 * i + 2]};
  const V3 nrm{-look.x, -look.y, -look.z};
  // means = origins + look * shadow_near_max (train_utils.py:3367), then + normals * normal_eps (render_utils.py:947)
  const float s = a.shadow_near_max, e = a.normal_eps;
  a.o_origins[3 * i] = (o.x + look.x * s) + nrm.x * e;
  a.o_origins[3 * i + 1] = (o.y + look.y * s) + nrm.y * e;
  a.o_origins[3 * i + 2] = (o.z + look.z * s) + nrm.z * e;
  // UniformHemisphereSampler.sample_directions in the frame of the normal
  const float u1 = a.u1[i], u2 = a.u2[i];
  const float ct = 1.0f - u1;
  const float sn = sqrtf((2.0f - u1) * u1);
  const float phi = u2 * 2.0f * kPi - kPi;
  const V3 wi{sn * cosf(phi), sn * sinf(phi), ct};
  const V3 d = to_global(wi, make_frame(nrm));
  a.o_directions[3 * i] = d.x; a.o_directions[3 * i + 1] = d.y; a.o_directions[3 * i + 2] = d.z;
  a.o_near[i] = s;
  a.o_far[i] = a.far;
}

__global__ void __launch_bounds__(256) k_mask_loss_bwd(RcMaskLossArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= a.n) return;                     // wave-uniform
  const int S = a.S;
  const bool act = lane < S;
  const int64_t p = ray * S + (act ? lane : 0);
  const float lm = a.lossmult ? a.lossmult[ray] : 1.0f;
  const float* td = a.tdist + ray * (S + 1);
  const float t0 = act ? td[lane] : 0.0f, t1 = act ? td[lane + 1] : 0.0f;
  const float dx = a.directions[3 * ray], dy = a.directions[3 * ray + 1], dz = a.directions[3 * ray + 2];
  const float dnorm = sqrtf(dx * dx + dy * dy + dz * dz);
  const float dens = act ? a.density[p] : 0.0f;
  // the last level's weights (compute_alpha_weights, the composite's own arithmetic), kept in the workspace
  const float wt = alpha_weight(dens, t0, t1, dnorm, act, lane);
  if (act) a.weights[p] = wt;
  const float acc = wave_sum(act ? wt : 0.0f);

  const float m = a.zero_masks ? 0.0f : (a.masks ? a.masks[ray] : 1.0f);
  const float wm = m > 0.5f ? a.weight_opaque : a.weight_empty;
  const float d = acc - m;
  const float r = sqrtf(d * d + a.padding * a.padding);
  if (lane == 0) a.loss_ray[ray] = lm * (r * wm);
  // d L / d acc, the same for every interval's weight
  const float g = act ? lm * wm * (d / r) * a.inv_n : 0.0f;
  const float adelta = act ? fabsf((t1 - t0) * dnorm) : 0.0f;
  const float x = act ? dens * adelta : 0.0f;
  const float dx_k = alpha_weights_bwd(g, act ? g * wt : 0.0f, x, lane);
  if (act) a.d_density[p] = dx_k * adelta;
}

}  // namespace

void rc_launch_backward_mask_rays(const RcBackwardMaskRaysArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_backward_mask_rays, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, st, a);
}

void rc_launch_mask_loss_bwd(const RcMaskLossArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_mask_loss_bwd, dim3((unsigned)((a.n + 3) / 4)), dim3(256), 0, st, a);
}
