// The probe of a surface point (rc_probe_rays, rc_vmf_panorama): the `vis_secondary` block of the
// reference's evaluation loop (engine/trainer.py:848-1069) for P selected pixels of a rendered view at once.
//
//   k_probe_rays     one thread per ray of the P latitude-longitude panoramas: the hit point of the pixel
//                    (origin + direction * distance_median + normal_offset * normal, :863-871), the panoramic cast from it
//                    (camera_utils.cast_spherical_rays with the identity rotation, :874-894) for the radii, and the
//                    directions / viewdirs of utils.get_sphere_directions (internal/utils.py:55-83) in their place
//                    (_update_secondary_rays, :934-942); lights, imageplane, look and up are row 0 of the view (:944-1012)
//   k_vmf_panorama   one thread per panorama pixel, blockIdx.y the probe: render_vmf (:1026-1069).  The workgroup builds the
//                    probe's lobe table (unit mean, kappa, 4 pi sinh kappa, weight) in LDS once; the lobe loop reads it at
//                    addresses the whole wave shares (a broadcast read), the pixel's direction stays in registers
//
// The element-wise arithmetic is fp32 in the order of tests/probe_ref.py (-ffp-contract=off keeps multiply and add apart);
// every sum over the lobes runs over j ascending.  No atomics: two calls on the same inputs are bitwise equal.
#include <hip/hip_runtime.h>

#include "rc_dev_camera.h"
#include "rc_dev_vis.h"
#include "rc_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr float kPiF = 3.14159265358979323846f;

// utils.get_sphere_directions(H, W, flip)[row * W + col].  jnp.linspace(a, b, n, endpoint=False)[i] is
// a (1 - s) + b s with s = i / n in fp32 (oracle/JAX_CALLS.md N4, without the appended end point); the half-pixel offsets
// are Python doubles rounded once.  phi runs from pi to -pi along a row, theta from 0 to pi down the rows.
__device__ __forceinline__ void sphere_direction(int row, int col, int H, int W, float phi_offset, float theta_offset, int flip,
                                                 float& x, float& y, float& z) {
  const float sp = (float)col / (float)W, st = (float)row / (float)H;
  const float phi = (kPiF * (1.0f - sp) + (-kPiF) * sp) - phi_offset;
  const float theta = (0.0f * (1.0f - st) + kPiF * st) + theta_offset;
  const float sin_t = sinf(theta), cos_t = cosf(theta), sin_p = sinf(phi), cos_p = cosf(phi);
  if (flip) {
    x = -cos_t; y = sin_t * cos_p; z = sin_t * sin_p;
  } else {
    x = sin_t * cos_p; y = sin_t * sin_p; z = cos_t;
  }
}

__global__ void __launch_bounds__(kThreads) k_probe_rays(RcProbeRaysArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.n) return;
  const int hw = a.height * a.width;
  const int probe = (int)(i / hw), pix = (int)(i - (int64_t)probe * hw);
  const int py = pix / a.width, px = pix - py * a.width;
  int64_t v = a.pixel[0];
#pragma unroll
  for (int k = 1; k < kRcProbeMax; ++k) v = k == probe ? a.pixel[k] : v;
  // positions = origins + directions * distance_median, then + normal_offset * normals (trainer.py:863-871)
  const float dm = a.distance_median[v];
  float pos[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    pos[c] = (a.origins[3 * v + c] + a.directions[3 * v + c] * dm) + a.normal_offset * a.normals[3 * v + c];
  if (a.positions && pix == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a.positions[3 * probe + c] = pos[c];
  }
  // the panoramic cast of this pixel around the hit point: its radius (and its image plane, when the view has none)
  const RcCastRow row = cast_pixel(a.s, a.pixtocam, a.rot, pos, px, py, false, 0.0f, 0.0f);
  float d[3];
  sphere_direction(py, px, a.height, a.width, a.phi_offset, a.theta_offset, a.flip, d[0], d[1], d[2]);
  const RcCastOut& o = a.out;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (o.origins) o.origins[3 * i + c] = row.o[c];
    if (o.directions) o.directions[3 * i + c] = d[c];
    if (o.viewdirs) o.viewdirs[3 * i + c] = d[c];
    if (o.lights) o.lights[3 * i + c] = a.lights ? a.lights[c] : pos[c];
    if (o.look) o.look[3 * i + c] = a.look ? a.look[c] : -a.rot[3 * c + 2];
    if (o.up) o.up[3 * i + c] = a.up ? a.up[c] : a.rot[3 * c + 1];
  }
  if (o.radii) o.radii[i] = row.radius;
  if (o.imageplane) {
    o.imageplane[2 * i] = a.imageplane ? a.imageplane[0] : row.ip[0];
    o.imageplane[2 * i + 1] = a.imageplane ? a.imageplane[1] : row.ip[1];
  }
  if (o.near) o.near[i] = a.s.near_v;
  if (o.far) o.far[i] = a.s.far_v;
}

__global__ void __launch_bounds__(kThreads) k_vmf_panorama(RcVmfPanoramaArgs a) {
  __shared__ float4 s_lobe[kRcProbeMaxLobes];              // unit mean, kappa
  __shared__ float2 s_scale[kRcProbeMaxLobes];             // 4 pi sinh(kappa), weight
  __shared__ float s_exp[kRcProbeMaxLobes];
  const int t = threadIdx.x, probe = blockIdx.y, V = a.V;
  float e = 0.0f;
  if (t < V) {
    const int64_t j = (int64_t)probe * V + t;
    // means / max(|means|, 1e-5) (trainer.py:1042), math.safe_exp of the logit (:1046, the clip at 70)
    const float mx = a.means[3 * j], my = a.means[3 * j + 1], mz = a.means[3 * j + 2], kappa = a.kappas[j];
    const float nrm = fmaxf(sqrtf((mx * mx + my * my) + mz * mz), 1e-5f);
    s_lobe[t] = make_float4(mx / nrm, my / nrm, mz / nrm, kappa);
    e = rc_safe_exp(a.logits[j]);
    s_exp[t] = e;
  }
  __syncthreads();
  if (t < V) {
    float sum = 0.0f;
    for (int j = 0; j < V; ++j) sum = sum + s_exp[j];
    s_scale[t] = make_float2(4.0f * kPiF * sinhf(s_lobe[t].w), e / sum);
  }
  __syncthreads();
  const int hw = a.height * a.width;
  const int pix = blockIdx.x * kThreads + t;
  if (pix >= hw) return;
  const int py = pix / a.width, px = pix - py * a.width;
  float x, y, z;
  sphere_direction(py, px, a.height, a.width, a.phi_offset, a.theta_offset, a.flip, x, y, z);
  // sum_j w_j eval_vmf(xyz, mean_j, kappa_j) (render_utils.py:1335-1346; its safe_exp is inverse_render.math's,
  // exp(min(x, 80)), as in rc_material.hip)
  float L = 0.0f;
  for (int j = 0; j < V; ++j) {
    const float4 m = s_lobe[j];
    const float2 c = s_scale[j];
    const float dot = (x * m.x + y * m.y) + z * m.z;
    const float vmf = m.w <= RC_EPS ? 1.0f / (4.0f * kPiF) : m.w * expf(fminf(m.w * dot, 80.0f)) / c.x;
    L = L + c.y * vmf;
  }
  const int64_t at = (int64_t)probe * hw + pix;
  if (a.out_linear) a.out_linear[at] = L;
  if (a.out_srgb || a.out_u8) {
    const float s = linear_to_srgb(L);
    if (a.out_srgb) { a.out_srgb[3 * at] = s; a.out_srgb[3 * at + 1] = s; a.out_srgb[3 * at + 2] = s; }
    if (a.out_u8) {
      const uint8_t u = save_u8(s);
      a.out_u8[3 * at] = u; a.out_u8[3 * at + 1] = u; a.out_u8[3 * at + 2] = u;
    }
  }
}

}  // namespace

void rc_launch_probe_rays(const RcProbeRaysArgs& a, hipStream_t stream) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_probe_rays, dim3((unsigned)((a.n + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, a);
}

void rc_launch_vmf_panorama(const RcVmfPanoramaArgs& a, int P, hipStream_t stream) {
  const int64_t hw = (int64_t)a.height * a.width;
  if (hw <= 0 || P <= 0) return;
  hipLaunchKernelGGL(k_vmf_panorama, dim3((unsigned)((hw + kThreads - 1) / kThreads), (unsigned)P), dim3(kThreads), 0, stream, a);
}
