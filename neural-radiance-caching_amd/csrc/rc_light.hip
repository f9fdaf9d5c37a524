// The light sampler's own loss, light_sampling: train_utils.light_sampling_loss
// (internal/train_utils.py:1985-2067) -> render_utils.vmf_loss_fn (internal/inverse_render/render_utils.py:1493-1547).
//
// Per shading point r and secondary sample k of suffix s (K_s samples: the Ks GGX rays, then the Kd cosine + vMF rays):
//   like = sum_j safe_exp(logit_j) eval_vmf(d_k, m^_j, kappa_j),  m^_j = l2_normalize(mean_j, grad_eps = 1e-5)
//   l    = srgb(max(like, 1e-5)),  f = srgb(max(|nan_to_num(rgb_k)|, 1e-5))
//   term = (f - l) sg(f - l) w_k (lossmult_r / K_s) / max(pdf_k, 1e-2),  w_k = clip(weight_k, 0, 10) [d_k . n_r > 0]
//   loss = mult / 2 * sum_s mean over the n K_s samples of term
// with get_vmfs (light_sampler.py:135-160): mean = vp[0:3] vmf_scale + noise vmf_scale / 2 - p, kappa = min(softplus(vp[3]
// + 1), 50), logit = max(vp[4] + 1, -50).  JAX rules: jnp.maximum / jnp.minimum give half the gradient on ties;
// safe_exp = exp(min(x, 80)) (no custom JVP); eval_vmf's kappa <= FLT_EPSILON branch is constant; linear_to_srgb's
// branch at 0.0031308; l2_normalize's override gradient.
//
// Kernels:
//   k_light_sampling_loss_bwd  one wave per shading point, lobes j = lane and lane + 64: per sample the mixture likelihood
//                              (a butterfly over the wave, lane 0's sum broadcast), the scalar d loss / d like, and per
//                              lobe the sums it needs for d loss / d (m^, kappa, logit) in registers; then d loss /
//                              d vmf_params [n][640] in the output layer's column order (lobe * 5 + channel) and the
//                              point's loss sum (loss_ray, reduced in a fixed order by k_interlevel_reduce).
// The dense layers' recompute and backward run on rc_data.hip's k_gemm (rc_light_host.inc).
#include <hip/hip_runtime.h>

#include "rc_dev_bwd.h"
#include "rc_internal.h"

using namespace rcdev;

namespace {

constexpr float kPi = 3.14159265358979323846f;

// the wave's sum, lane 0's order, on every lane
__device__ __forceinline__ float wave_total(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return readlane_f(v, 0);
}
// d max(x, c) / d x and d min(x, c) / d x with the balanced tie rule
__device__ __forceinline__ float max_grad(float x, float c) { return x > c ? 1.0f : (x == c ? 0.5f : 0.0f); }
__device__ __forceinline__ float min_grad(float x, float c) { return x < c ? 1.0f : (x == c ? 0.5f : 0.0f); }

// image.linear_to_srgb (internal/image.py:192-200) and its derivative
__device__ __forceinline__ float srgb(float x) {
  return x <= 0.0031308f ? (323.0f / 25.0f) * x : (211.0f * powf(fmaxf(RC_EPS, x), 5.0f / 12.0f) - 11.0f) / 200.0f;
}
__device__ __forceinline__ float srgb_grad(float x) {
  if (x <= 0.0031308f) return 323.0f / 25.0f;
  const float g = (211.0f / 200.0f) * (5.0f / 12.0f) * powf(fmaxf(RC_EPS, x), -7.0f / 12.0f);
  return g * max_grad(x, RC_EPS);
}

__global__ void __launch_bounds__(256) k_light_sampling_loss_bwd(RcLightLossArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.n) return;                       // wave-uniform; no barriers below
  const int Ks = a.Ks, Kd = a.Kd, K = Ks + Kd;
  const float px = a.pts[3 * r], py = a.pts[3 * r + 1], pz = a.pts[3 * r + 2];
  const float nx = a.nrm[3 * r], ny = a.nrm[3 * r + 1], nz = a.nrm[3 * r + 2];
  const float lm = a.lossmult ? a.lossmult[r] : 1.0f;

  // the two lobes of the lane: get_vmfs, then vmf_loss_fn's activations
  float vm[2][3], mh[2][3], kap[2], ex[2], den[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int j = lane + 64 * q;
    const float* v = a.vp + r * 640 + j * 5;
    const float* nzp = a.noise + (r * 128 + j) * 3;
    vm[q][0] = v[0] * a.vmf_scale + 0.0f + nzp[0] * a.vmf_scale / 2.0f - px;
    vm[q][1] = v[1] * a.vmf_scale + 0.0f + nzp[1] * a.vmf_scale / 2.0f - py;
    vm[q][2] = v[2] * a.vmf_scale + 0.0f + nzp[2] * a.vmf_scale / 2.0f - pz;
    const float s = vm[q][0] * vm[q][0] + vm[q][1] * vm[q][1] + vm[q][2] * vm[q][2];
    const float inv = s < RC_TINY ? 0.0f : 1.0f / sqrtf(fmaxf(RC_TINY, s));
    mh[q][0] = vm[q][0] * inv; mh[q][1] = vm[q][1] * inv; mh[q][2] = vm[q][2] * inv;
    kap[q] = fminf(softplus_f(v[3] + 1.0f), 50.0f);
    ex[q] = expf(fminf(fmaxf(v[4] + 1.0f, -50.0f), 80.0f));     // safe_exp(logit)
    den[q] = 4.0f * kPi * sinhf(kap[q]);
  }
  // per lobe: T = sum_k G e v, C = sum_k G e v [a < 80] c, D = sum_k G e v [a < 80] d  (G = d loss / d like)
  float T[2] = {0.0f, 0.0f}, Cs[2] = {0.0f, 0.0f}, D[2][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
  float loss_r = 0.0f;
  for (int s = 0; s < 2; ++s) {
    const int Kx = s == 0 ? Ks : Kd;
    float part = 0.0f;
    for (int k = 0; k < Kx; ++k) {
      const int64_t idx = s == 0 ? r * Ks + k : a.n * Ks + r * Kd + k;
      const float* sm = a.samples + (r * K + (s == 0 ? k : Ks + k)) * RC_SMP_CH;
      const float dx = a.sec_dirs[3 * idx], dy = a.sec_dirs[3 * idx + 1], dz = a.sec_dirs[3 * idx + 2];
      const float pdf = sm[3], wraw = sm[4];
      const float cr = fix_nan(a.sec_rgb[3 * idx]), cg = fix_nan(a.sec_rgb[3 * idx + 1]), cb = fix_nan(a.sec_rgb[3 * idx + 2]);
      float fv = fmaxf(sqrtf(cr * cr + cg * cg + cb * cb), 1e-5f);
      float w = fminf(fmaxf(wraw, 0.0f), 10.0f);
      if (!(dx * nx + dy * ny + dz * nz > 0.0f)) w = 0.0f;
      const float dn = fmaxf(pdf, 1e-2f);
      // the mixture likelihood
      float ev[2], ind[2], cq[2];
      float acc = 0.0f;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        cq[q] = dx * mh[q][0] + dy * mh[q][1] + dz * mh[q][2];
        const float arg = kap[q] * cq[q];
        ind[q] = min_grad(arg, 80.0f);
        const float v = kap[q] <= RC_EPS ? 1.0f / (4.0f * kPi) : kap[q] * expf(fminf(arg, 80.0f)) / den[q];
        ev[q] = ex[q] * v;
        acc = acc + ev[q];
      }
      const float like = wave_total(acc);
      const float lmax = fmaxf(like, 1e-5f);
      float lv = lmax;
      float dl = max_grad(like, 1e-5f);                        // d l / d like
      if (a.srgb) { fv = srgb(fv); lv = srgb(lmax); dl *= srgb_grad(lmax); }
      const float diff = fv - lv;
      const float sc = w * (lm / (float)Kx) / dn;
      part = part + diff * diff * sc;
      const float G = -diff * sc * (s == 0 ? a.coef_spec : a.coef_diff) * dl;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const float t = G * ev[q];
        T[q] += t;
        if (kap[q] > RC_EPS) {
          const float tc = t * ind[q];
          Cs[q] += tc * cq[q];
          D[q][0] += tc * dx; D[q][1] += tc * dy; D[q][2] += tc * dz;
        }
      }
    }
    loss_r = loss_r + part / (float)Kx;
  }
  if (lane == 0) a.loss_ray[r] = loss_r;
  if (!a.dvp) return;
  // through eval_vmf's kappa / mean, safe_exp and get_vmfs' activations to vmf_params
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int j = lane + 64 * q;
    const float* v = a.vp + r * 640 + j * 5;
    float* o = a.dvp + r * 640 + j * 5;
    float gk = 0.0f, gm[3] = {0.0f, 0.0f, 0.0f};
    if (kap[q] > RC_EPS) {
      const float k = kap[q];
      gk = T[q] * (1.0f / k - coshf(k) / sinhf(k)) + Cs[q];    // d v / d kappa = v (1 / kappa + [a < 80] c - coth kappa)
      gm[0] = k * D[q][0]; gm[1] = k * D[q][1]; gm[2] = k * D[q][2];
    }
    float d0, d1, d2;
    l2_normalize_bwd_eps(vm[q][0], vm[q][1], vm[q][2], gm[0], gm[1], gm[2], 1e-5f, d0, d1, d2);
    const float x3 = v[3] + 1.0f, x4 = v[4] + 1.0f;
    const float sp = softplus_f(x3);
    const float lg = fmaxf(x4, -50.0f);
    o[0] = d0 * a.vmf_scale; o[1] = d1 * a.vmf_scale; o[2] = d2 * a.vmf_scale;
    o[3] = gk * min_grad(sp, 50.0f) * sigm(x3);
    o[4] = T[q] * min_grad(lg, 80.0f) * max_grad(x4, -50.0f);
  }
}

}  // namespace

void rc_launch_light_sampling_loss_bwd(const RcLightLossArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_light_sampling_loss_bwd, dim3((unsigned)((a.n + 3) / 4)), dim3(256), 0, st, a);
}
