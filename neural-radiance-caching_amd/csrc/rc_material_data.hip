// The material stage's data loss: the "data" term of the MaterialIntegrator's output "main" in the
// material_light_from_scratch stage, train_utils.compute_data_loss (internal/train_utils.py:402-528) with loss_type
// 'rawnerf_transient_unbiased', loss_weight 0.1 (configs/nerf_ngp_yobo.gin:427-428), is_material (rawnerf exponent 1,
// eps 1e-2, nerf_ngp_yobo.gin:437, 440) and data_loss_mult 1 (ngp_yobo.gin:456).  _select_data_loss_function (:643-684)
// maps that type to compute_unbiased_loss_rawnerf (:173-197), so with rgb_clip from _get_rgb_clip_for_rawnerf (:369-395;
// use_combined_rawnerf = True, internal/configs.py:588; c = the rendering's "cache_rgb", DESIGN Oddities):
//   s       = 1 / (sg(clip(max(clip(c, 0, 1e4), gt), 0, 1e4)) ** exponent + eps)      per ray and channel
//   loss    = weight * data_loss_mult * mean_{n x 3}(lossmult * 2 (rgb - gt) sg(rgb - gt) s)
//   lossmult = 0 where gt > loss_thresh (1e6).
// rgb = w * sh_rgb + max(0, 1 - acc) * bg, sh_rgb = the four integration means of k_material_integrate.  The gradient is
// the exact one of params/MaterialShader through the BRDF evaluation under Trainer.stopgrad = True (path (a), DESIGN
// §4.12): directions, pdf, MIS weight, the secondary radiance, acc, the EnvMap radiance, w and the primary geometry are
// constants.  JAX rules: jnp.clip = minimum(maximum(x, lo), hi), each with ties split (half the gradient at 0 and at
// rgb_max); jnp.maximum ties split (the RC_EPS floors of D and G); nan_to_num passes the gradient through; the factor
// 2 (rgb - gt) sg(rgb - gt) gives d loss / d rgb = 2 sg(rgb - gt) s lossmult (half the derivative of the loss's value).
//
// Kernels:
//   k_material_data_bwd       one wave per shading point, lane = secondary sample, k_material_integrate's arithmetic:
//                             the lobes, the four means and rgb (bitwise rc_render_material's "rgb"), the loss terms of
//                             the point, then d loss / d (albedo rgb, roughness, metalness) per lane, added over the
//                             wave by the same butterfly: per point [5] floats written, nothing per (point, sample).
//   k_material_data_env_bwd   the same body with the other tail: d loss / d (EnvMap radiance) of every
//                             secondary ray, [n Ks | n Kd][3] in the trace's ray order; nothing else written.
//   k_material_data_head_bwd  one workgroup of 128 threads takes chunks of 16 shading points: the material head's
//                             recompute in material_head_block's order, material_head_bwd (rc_dev_material.h), d loss /
//                             d features ([n][32], for rc_hashgrid_backward) and one weight-gradient partial per
//                             workgroup, no atomics; the workgroup's loss sum (its points in order, double).
// The partials and loss sums go through rc_launch_material_partials_reduce (k_material_smoothness_reduce: fixed order).
// Everything runs in fp32 (no MFMA, no scratch).
#include <hip/hip_runtime.h>

#include "rc_internal.h"
#include "rc_dev_material.h"

namespace {

constexpr float kPi = 3.14159265358979323846f;
constexpr float kDenomEps = 1e-5f;         // render_utils.DENOMINATOR_EPS
constexpr int kMdMaxBlocks = 512;          // workgroups (and partials) of the head's backward at most

// as rc_material.hip (the forward's arithmetic, repeated here bit for bit)
__device__ __forceinline__ float wsum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ V3 ir_normalize(V3 v) {
  const float l = sqrtf(1e-10f + dot(v, v));
  return {v.x / l, v.y / l, v.z / l};
}
__device__ __forceinline__ float ggx_d(float c, float a) {
  const float t = c * c * (a * a - 1.0f) + 1.0f;
  return (a * a) / fmaxf(RC_EPS, kPi * (t * t));
}
// d ggx_d(c, a) / d a, through the floor max(RC_EPS, pi t^2) with its tie rule
__device__ __forceinline__ float ggx_d_grad(float c, float a) {
  const float t = c * c * (a * a - 1.0f) + 1.0f;
  const float den = kPi * (t * t), M = fmaxf(RC_EPS, den);
  const float dden = kPi * 2.0f * t * (c * c * 2.0f * a);
  return 2.0f * a / M - (a * a) / (M * M) * max_grad(den, RC_EPS) * dden;
}
// d jnp.clip(x, 0, hi) / d x = d minimum(maximum(x, 0), hi): each tie passes half
__device__ __forceinline__ float clip_grad(float x, float hi) {
  const float y = fmaxf(x, 0.0f);
  return max_grad(x, 0.0f) * (y < hi ? 1.0f : (y == hi ? 0.5f : 0.0f));
}
__device__ __forceinline__ float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// The body of k_material_data_bwd; kEnv: k_material_data_env_bwd's, which leaves the point's outputs alone and writes
// d loss / d (the EnvMap radiance of its secondary rays) instead of d loss / d material.
template <bool kEnv>
__device__ __forceinline__ void material_data_point(const RcMatDataArgs& a, float env_scale, float* d_env) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int64_t r = (int64_t)blockIdx.x * 4 + wave;
  const bool ok = r < a.n;
  if (!ok) r = a.n - 1;
  const int Ks = a.Ks, Kd = a.Kd, K = Ks + Kd;
  const float* m = a.mat + r * RC_MAT_CH;
  const float albedo[3] = {m[0], m[1], m[2]};
  const float rough = m[3], metal = m[4];
  const V3 wo = {a.local_view[3 * r], a.local_view[3 * r + 1], a.local_view[3 * r + 2]};
  const bool act = lane < K;
  const bool spec = lane < Ks;
  // the forward, k_material_integrate's per-lane arithmetic (the irradiance terms left out: they do not reach rgb)
  float ind[3] = {0, 0, 0}, dir[3] = {0, 0, 0};
  float rin[3] = {0, 0, 0}, ein[3] = {0, 0, 0}, lobe[3] = {0, 0, 0};
  float wd = 0.0f, D = 0.0f, G = 0.0f, n_v = 0.0f, n_l = 0.0f, n_h = 0.0f, c5 = 0.0f;
  float dein[3] = {0, 0, 0};               // kEnv: d ein / d (the EnvMap's clipped softplus)
  int64_t sec = 0;
  if (act) {
    const float* sm = a.samples + (r * K + lane) * RC_SMP_CH;
    const V3 wi = {sm[0], sm[1], sm[2]};
    const float pdf = sm[3];
    float weight = fmaxf(sm[4], 0.0f);
    if (!(wi.z > 0.0f)) weight = 0.0f;
    const float denom = fmaxf(pdf, kDenomEps);
    const int64_t idx = spec ? r * Ks + lane : a.n * Ks + r * Kd + (lane - Ks);
    const float acc = a.sec_acc[idx];
    const V3 h = ir_normalize(V3{wi.x + wo.x, wi.y + wo.y, wi.z + wo.z});
    n_v = fmaxf(0.0f, wo.z); n_l = fmaxf(0.0f, wi.z); n_h = fmaxf(0.0f, h.z);
    const float l_h = fmaxf(0.0f, dot(wi, h));
    D = ggx_d(n_h, rough);
    const float k = rough / 2.0f;
    G = (n_v / fmaxf(RC_EPS, n_v * (1.0f - k) + k)) * (n_l / fmaxf(RC_EPS, n_l * (1.0f - k) + k));
    const float c1 = fminf(fmaxf(1.0f - l_h, 0.0f), 1.0f), c2 = c1 * c1, c4 = c2 * c2;
    c5 = c1 * c4;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float F0 = albedo[c] * metal + a.f0 * (1.0f - metal);
      const float F = F0 + (1.0f - F0) * c5;
      const float ggx = D * F * G / fmaxf(RC_EPS, 4.0f * n_v);
      const float lambert = n_l * albedo[c] / kPi;
      lobe[c] = spec ? ggx * 1.0f * 1.0f : lambert * 1.0f * (1.0f - metal);
      float ri = a.sec_rgb[3 * idx + c];
      if (ri != ri) ri = 0.0f;
      ri = fmaxf(fminf(fmaxf(ri, -RC_FMAX), RC_FMAX), 0.0f);
      float ei = fmaxf(a.sec_env[3 * idx + c], 0.0f) * (1.0f - acc);
      if (kEnv) {
        // env_map_fn's jnp.maximum(., 0) (ties split), the product with 1 - acc, nan_to_num (passes where finite)
        const float e0 = a.sec_env[3 * idx + c];
        dein[c] = (ei == ei && fabsf(ei) <= RC_FMAX) ? max_grad(e0, 0.0f) * (1.0f - acc) : 0.0f;
        sec = idx;
      }
      if (ei != ei) ei = 0.0f;
      ei = fminf(fmaxf(ei, -RC_FMAX), RC_FMAX);
      rin[c] = ri; ein[c] = ei;
      ind[c] = fminf(fmaxf(ri * lobe[c], 0.0f), a.rgb_max) * weight / denom;
      dir[c] = fminf(fmaxf(ei * lobe[c], 0.0f), a.rgb_max) * weight / denom;
    }
    wd = weight / denom;
  }
  float o_is[3], o_id[3], o_ds[3], o_dd[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    o_is[c] = wsum(act && spec ? ind[c] : 0.0f) / (float)Ks;
    o_ds[c] = wsum(act && spec ? dir[c] : 0.0f) / (float)Ks;
    o_id[c] = wsum(act && !spec ? ind[c] : 0.0f) / (float)Kd;
    o_dd[c] = wsum(act && !spec ? dir[c] : 0.0f) / (float)Kd;
  }
  const int S = a.S;
  const float acc_p = wsum(lane < S ? a.weights[r * S + lane] : 0.0f);
  const float w = a.filt_weight[r];
  const float bgw = fmaxf(0.0f, 1.0f - acc_p) * a.bg;
  // the loss terms of the point (every lane holds the sums)
  float out[3], cr[3], gt[3];
  const float lm0 = a.lossmult ? a.lossmult[r] : 1.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    out[c] = w * (((o_dd[c] + o_ds[c]) + o_id[c]) + o_is[c]) + bgw;
    gt[c] = a.gt[3 * r + c];
    // _get_rgb_clip_for_rawnerf
    if (a.use_gt) {
      cr[c] = clampf(gt[c], 0.0f, a.clip_val);
    } else {
      cr[c] = clampf(a.cache_rgb[3 * r + c], 0.0f, a.clip_val);
      if (a.use_combined) cr[c] = clampf(fmaxf(cr[c], gt[c]), 0.0f, a.clip_val);
    }
  }
  if (a.use_norm) {
    const float nv = sqrtf(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
    cr[0] = nv; cr[1] = nv; cr[2] = nv;
  }
  float lsum = 0.0f, grgb[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float lm = gt[c] > a.thresh ? 0.0f : lm0;
    const float sc = 1.0f / ((a.exponent == 1.0f ? cr[c] : powf(cr[c], a.exponent)) + a.eps);
    const float d = out[c] - gt[c];
    lsum += lm * (2.0f * d * d * sc);
    grgb[c] = a.coef * lm * 2.0f * d * sc * w;             // d loss / d sh_rgb[c]
  }
  if (kEnv) {
    // d loss / d env = d loss / d sh_rgb * (1 / K_pass) * weight / max(pdf, 1e-5) * clip'(ein lobe) * lobe * d ein / d env
    if (act && ok) {
      const float inv = 1.0f / (float)(spec ? Ks : Kd);
#pragma unroll
      for (int c = 0; c < 3; ++c)
        d_env[3 * sec + c] = env_scale * (grgb[c] * inv * wd * (clip_grad(ein[c] * lobe[c], a.rgb_max) * lobe[c]) * dein[c]);
    }
    return;
  }
  if (lane == 0 && ok) {
    a.rgb[3 * r] = out[0]; a.rgb[3 * r + 1] = out[1]; a.rgb[3 * r + 2] = out[2];
    a.loss_ray[r] = lsum;
  }
  if (!a.dmat) return;
  // d loss / d lobe per channel, then through the lobe to (albedo, roughness, metalness)
  float dm[5] = {0, 0, 0, 0, 0};
  if (act) {
    const float inv = 1.0f / (float)(spec ? Ks : Kd);
    float dl[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      dl[c] = grgb[c] * inv * wd * (rin[c] * clip_grad(rin[c] * lobe[c], a.rgb_max) + ein[c] * clip_grad(ein[c] * lobe[c], a.rgb_max));
    if (spec) {
      const float M4 = fmaxf(RC_EPS, 4.0f * n_v);
      const float k = rough / 2.0f;
      const float Av = n_v * (1.0f - k) + k, Al = n_l * (1.0f - k) + k;
      const float Mv = fmaxf(RC_EPS, Av), Ml = fmaxf(RC_EPS, Al);
      const float G1v = n_v / Mv, G1l = n_l / Ml;
      const float dG1v = -n_v / (Mv * Mv) * max_grad(Av, RC_EPS) * (1.0f - n_v);     // d / d k
      const float dG1l = -n_l / (Ml * Ml) * max_grad(Al, RC_EPS) * (1.0f - n_l);
      const float dG = 0.5f * (dG1v * G1l + G1v * dG1l);                             // d G / d roughness (k = a / 2)
      const float dD = ggx_d_grad(n_h, rough);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float F0 = albedo[c] * metal + a.f0 * (1.0f - metal);
        const float F = F0 + (1.0f - F0) * c5;
        const float gF0 = dl[c] * (D * G / M4) * (1.0f - c5);
        dm[c] += gF0 * metal;
        dm[4] += gF0 * (albedo[c] - a.f0);
        dm[3] += dl[c] * (F / M4) * (dD * G + D * dG);
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        dm[c] += dl[c] * (n_l / kPi) * (1.0f - metal);
        dm[4] -= dl[c] * (n_l * albedo[c] / kPi);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) dm[k] = wsum(dm[k]);
  if (lane == 0 && ok) {
#pragma unroll
    for (int k = 0; k < 5; ++k) a.dmat[r * 5 + k] = dm[k];
  }
}

__global__ __launch_bounds__(256) void k_material_data_bwd(RcMatDataArgs a) { material_data_point<false>(a, 0.0f, nullptr); }

__global__ __launch_bounds__(256) void k_material_data_env_bwd(RcMatDataArgs a, float env_scale, float* d_env) {
  material_data_point<true>(a, env_scale, d_env);
}

__global__ __launch_bounds__(128) void k_material_data_head_bwd(RcMatDataHeadArgs a) {
  const int t = threadIdx.x;
  const int64_t n = a.n;
  const int64_t chunks = (n + kMsE - 1) / kMsE;
  if (!a.part) {                                   // loss only: the workgroup's loss sum, its points in order
    if (t == 0) {
      double acc = 0.0;
      for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x)
        for (int64_t p = ch * kMsE; p < n && p < (ch + 1) * kMsE; ++p) acc += (double)a.loss_ray[p];
      a.loss_part[blockIdx.x] = acc;
    }
    return;
  }
  __shared__ MsShared s;
  const float r0 = a.min_roughness * a.min_roughness;
  float w0r[kMsIn], w1r[5];
#pragma unroll
  for (int i = 0; i < kMsIn; ++i) w0r[i] = a.w0[i * kMsHid + t];
#pragma unroll
  for (int k = 0; k < 5; ++k) w1r[k] = a.w1[t * 10 + kMsCol[k]];
  const float b0 = a.b0[t];
  for (int e = t; e < kMsIn * kMsHid; e += 128) s.w0t[e & (kMsHid - 1)][e >> 7] = a.w0[e];
  for (int e = t; e < kMsHid * 10; e += 128) s.w1[e] = a.w1[e];
  MsAcc acc;
#pragma unroll
  for (int i = 0; i < kMsIn; ++i) acc.dw0[i] = 0.0f;
#pragma unroll
  for (int k = 0; k < 5; ++k) acc.dw1[k] = 0.0f;
  acc.db0 = 0.0f; acc.db1 = 0.0f;
  double loss_acc = 0.0;

  for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const int64_t p0 = ch * kMsE;
    const int np = (int)((n - p0) < kMsE ? (n - p0) : kMsE);
    __syncthreads();                               // the previous chunk's LDS reads are done
    for (int e = t; e < kMsE * kMsIn; e += 128) {
      const int ev = e / kMsIn, i = e - ev * kMsIn;
      s.f[ev][i] = ev < np ? a.feat[(p0 + ev) * kMsIn + i] : 0.0f;
    }
    __syncthreads();
    // bottleneck_layer, material_head_block's order
#pragma unroll 1
    for (int e = 0; e < kMsE; ++e) {
      float h = 0.0f;
#pragma unroll
      for (int i = 0; i < kMsIn; ++i) h = h + s.f[e][i] * w0r[i];
      s.h[e][t] = h + b0;
    }
    __syncthreads();
    if (t < kMsE * 5) {
      const int e = t / 5, k = t - e * 5, c = kMsCol[k];
      float o = 0.0f;
      for (int j = 0; j < kMsHid; ++j) o = o + s.h[e][j] * s.w1[j * 10 + c];
      s.o[e][k] = o + a.b1[c];
    }
    __syncthreads();
    if (t < kMsE) {
      const int e = t;
      const float* so = s.o[e];
      s.mat[e][0] = sigmoidf(so[0] - 1.0f); s.mat[e][1] = sigmoidf(so[1] - 1.0f); s.mat[e][2] = sigmoidf(so[2] - 1.0f);
      s.mat[e][3] = sigmoidf(so[3] - 1.0f) * (1.0f - r0) + r0;
      s.mat[e][4] = sigmoidf(so[4] + 0.0f);
#pragma unroll
      for (int k = 0; k < 5; ++k) s.dm[e][k] = e < np ? a.dmat[(p0 + e) * 5 + k] : 0.0f;
    }
    __syncthreads();
    if (t == 0)
      for (int q = 0; q < np; ++q) loss_acc += (double)a.loss_ray[p0 + q];
    material_head_bwd(s, kMsE, w1r, r0, acc);
    __syncthreads();
    // d loss / d features = dh W0^T: thread (feature i = t & 31, evaluations (t >> 5) + 4 k)
    const int i = t & 31;
#pragma unroll 1
    for (int k = 0; k < kMsE / 4; ++k) {
      const int e = (t >> 5) + 4 * k;
      float d = 0.0f;
      for (int j = 0; j < kMsHid; ++j) d = fmaf(s.w0t[j][i], s.dh[e][j], d);
      if (e < np) a.dfeat[(p0 + e) * kMsIn + i] = d;
    }
  }
  if (t == 0) a.loss_part[blockIdx.x] = loss_acc;
  // the workgroup's partial in the layout's order (as k_material_smoothness_bwd)
  float* part = a.part + (int64_t)blockIdx.x * kRcMatSmoothParts;
#pragma unroll
  for (int i = 0; i < kMsIn; ++i) part[i * kMsHid + t] = acc.dw0[i];
  part[kMsIn * kMsHid + t] = acc.db0;
  float* pw1 = part + kMsIn * kMsHid + kMsHid;
  for (int c = 0; c < 10; ++c) {
    float v = 0.0f;
#pragma unroll
    for (int k = 0; k < 5; ++k) if (kMsCol[k] == c) v = acc.dw1[k];
    pw1[t * 10 + c] = v;
  }
  if (t < 10) pw1[kMsHid * 10 + t] = acc.db1;
}

}  // namespace

int rc_mat_data_blocks(int64_t n) {
  const int64_t chunks = (n + kMsE - 1) / kMsE;
  return (int)(chunks < kMdMaxBlocks ? chunks : kMdMaxBlocks);
}

void rc_launch_material_data_bwd(const RcMatDataArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_material_data_bwd, dim3((unsigned)((a.n + 3) / 4)), dim3(256), 0, st, a);
}

void rc_launch_material_data_env_bwd(const RcMatDataArgs& a, float env_scale, float* d_env, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_material_data_env_bwd, dim3((unsigned)((a.n + 3) / 4)), dim3(256), 0, st, a, env_scale, d_env);
}

void rc_launch_material_data_head_bwd(const RcMatDataHeadArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_material_data_head_bwd, dim3((unsigned)rc_mat_data_blocks(a.n)), dim3(128), 0, st, a);
}
