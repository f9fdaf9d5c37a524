// The time-resolved cache's data loss through the compositing weights of the last sampler level.
//
// rc_transient_data_backward leaves d loss / d weights_s of every shaded sample in "td:d_weights": the weights enter the
// TransientVolumeIntegrator as a leaf.  This file takes that adjoint back through render.compute_alpha_weights
// (internal/render.py:134-169) to d loss / d density_s, which rc_density_backward turns into the gradient of MLP_2 (grid
// tables and density layers).  As in rc_data_backward / rc_mask_backward, sdist / tdist / means carry no gradient
// (sampling.py:354-355).
//
// This is the WEIGHTS path only.  The data loss also reaches MLP_2 through the geometry feature and through the predicted
// and analytic normals that the shader reads (stopgrad_geometry_feature_weight = stopgrad_geometry_normals_weight = 1.0,
// transient_simulation_ngp_yobo.gin:261-262); those paths run through the shader's backward, which does not exist for
// this model, and are NOT part of the gradient this kernel starts.
//
// Kernel:
//   k_transient_weights_bwd   one wave per ray, lane = shaded sample (S <= 32): x = density |delta| with the delta of the
//                             forward's compositing on this handle (k_composite, rc_sample.hip: delta = (t1 - t0) |direction|,
//                             tdist the metric distances of the power-ladder sampler), w = the weights k_composite stored,
//                             d_density = alpha_weights_bwd(g, g w, x) |delta|.  No atomics, no LDS, no scratch.
#include <hip/hip_runtime.h>

#include "rc_dev_bwd.h"
#include "rc_internal.h"

using namespace rcdev;

namespace {

__global__ void __launch_bounds__(256) k_transient_weights_bwd(RcTransWeightsBwdArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= a.n) return;                     // wave-uniform
  const int S = a.S;
  const bool act = lane < S;
  const int64_t p = ray * S + (act ? lane : 0);
  const float* td = a.tdist + ray * (S + 1);
  const float t0 = act ? td[lane] : 0.0f, t1 = act ? td[lane + 1] : 0.0f;
  const float dx = a.directions[3 * ray], dy = a.directions[3 * ray + 1], dz = a.directions[3 * ray + 2];
  const float dnorm = sqrtf(dx * dx + dy * dy + dz * dz);
  const float dens = act ? a.density[p] : 0.0f;
  const float wt = act ? a.weights[p] : 0.0f;
  const float g = act ? a.d_weights[p] : 0.0f;
  const float adelta = act ? fabsf((t1 - t0) * dnorm) : 0.0f;
  const float x = act ? dens * adelta : 0.0f;
  const float dx_k = alpha_weights_bwd(g, act ? g * wt : 0.0f, x, lane);
  if (act) a.d_density[p] = dx_k * adelta;
}

}  // namespace

void rc_launch_transient_weights_bwd(const RcTransWeightsBwdArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_transient_weights_bwd, dim3((unsigned)((a.n + 3) / 4)), dim3(256), 0, st, a);
}
