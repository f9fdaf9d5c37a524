// The material network's smoothness loss, material_smoothness: train_utils.material_smoothness_loss
// (internal/train_utils.py:2505-2700), called from _compute_extra_losses (:3599-3659) with mult 1.0
// (configs/trainer.gin:340-344) and the hotdog Config values (configs/nerf_ngp_yobo.gin:400-408, ngp_yobo.gin:432):
// l1 loss, tensoir albedo, noise 0.01, weight_albedo = weight_other = 1e-4, no irradiance weight, no albedo stopgrad.
//
// Per shading point p (the one sample per ray of the material pass: m_pts, weight w = filt_weight), x' = x + noise nu
// (stop-gradiented, :2568-2572), m = material_mlp at x, m' = nan_to_num(material_mlp at x') (:2592-2595), and
// lambda = lossmult_r sg(w) (:2601-2607; maybe_resample over the one sample leaves w / sg(1 + 1e-8) = w in float32):
//   albedo term     weight_albedo * mean over n x 3 of |(a - a') / max(1e-6, max(a, a'))| lambda   (denominator not stopped)
//   roughness term  weight_other * mean over n of |r - r'| lambda,  metalness term the same with m
//   loss = mult * (sum of the terms)      (F_0 is a constant, diffuseness / mirrorness zeros: they add 0, no gradient)
// with material_mlp (MaterialMLP._predict_material_and_feature, internal/material.py:2073-2123): material grid features
// (32) -> Dense 128 (bottleneck_layer, no activation) -> Dense 10 (pred_brdf_layer) = b, albedo = sigmoid(b[0:3] - 1),
// roughness = sigmoid(b[6] - 1) (1 - r0) + r0 (r0 = min_roughness^2), metalness = sigmoid(b[8]).
// JAX rules: jnp.maximum gives half the gradient to each side on a tie; d|x|/dx = +1 at x = 0 (jax 0.4.16 _abs_jvp_rule:
// select(x >= 0, g, -g)); nan_to_num passes the gradient unchanged where the value is finite; lax.logistic's derivative
// is g ans (1 - ans); d(u / v) / dv = -u / v^2.
//
// Kernels:
//   k_material_smoothness_points  pts [2n][3] = (x, x + noise_scale nu): the lookup points of both evaluations.
//   k_material_smoothness_bwd     one workgroup of 128 threads takes chunks of 8 shading points (16 evaluations); per
//                                 chunk: the bottleneck layer (thread t = hidden column t, its column of W0 in registers;
//                                 material_head_block's summation order, so m(x) is bitwise m_mat), the five used outputs
//                                 of pred_brdf_layer (one thread per (evaluation, output), sequential over the 128 inputs
//                                 as material_head_block), the loss terms and d loss / d (albedo, roughness, metalness) per
//                                 point, then material_head_bwd: the sigmoid heads, both dense layers and d loss /
//                                 d features ([2n][32], for rc_hashgrid_backward).  The weight gradients of the
//                                 workgroup's points stay in registers until its end and are written as one partial per
//                                 workgroup, no atomics, and its loss sum (its points in order, double).
//   k_material_smoothness_reduce  the dense gradients: the partials added in workgroup order into the layout's dense
//                                 segments; the loss: the workgroups' sums in a fixed tree, * mult / n.
// Everything runs in fp32 (no MFMA, no scratch).
#include <hip/hip_runtime.h>

#include "rc_internal.h"
#include "rc_dev_material.h"

namespace {

constexpr int kMsMaxBlocks = 512;          // workgroups (and partials) at most (<= 1024: the loss reduction's block)

__global__ __launch_bounds__(256) void k_material_smoothness_points(const float* __restrict__ pts, const float* __restrict__ noise,
                                                                   float scale, int64_t n, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 3 * n) return;
  const float x = pts[i];
  out[i] = x;
  out[3 * n + i] = x + noise[i] * scale;           // origins + noise * config.material_smoothness_noise
}

__global__ __launch_bounds__(128) void k_material_smoothness_bwd(RcMatSmoothArgs a) {
  __shared__ MsShared s;
  const int t = threadIdx.x;
  const int64_t n = a.n;
  const float r0 = a.min_roughness * a.min_roughness;
  const bool grads = a.part != nullptr;
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
  double loss_acc = 0.0;                           // thread 0: the workgroup's loss sum, its points in order

  const int64_t chunks = (n + kMsPts - 1) / kMsPts;
  for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const int64_t p0 = ch * kMsPts;
    const int np = (int)((n - p0) < kMsPts ? (n - p0) : kMsPts);
    __syncthreads();                               // the previous chunk's LDS reads are done
    for (int e = t; e < kMsE * kMsIn; e += 128) {
      const int ev = e / kMsIn, i = e - ev * kMsIn, q = ev >> 1;
      s.f[ev][i] = q < np ? ((ev & 1) ? a.feat_p : a.feat_x)[(p0 + q) * kMsIn + i] : 0.0f;
    }
    __syncthreads();
    // bottleneck_layer, material_head_block's order: acc = acc + f_i w_i over i, then + b0
#pragma unroll 1
    for (int e = 0; e < kMsE; ++e) {
      float h = 0.0f;
#pragma unroll
      for (int i = 0; i < kMsIn; ++i) h = h + s.f[e][i] * w0r[i];
      s.h[e][t] = h + b0;
    }
    __syncthreads();
    // pred_brdf_layer's five used outputs, sequential over j as material_head_block
    if (t < kMsE * 5) {
      const int e = t / 5, k = t - e * 5, c = kMsCol[k];
      float o = 0.0f;
      for (int j = 0; j < kMsHid; ++j) o = o + s.h[e][j] * s.w1[j * 10 + c];
      s.o[e][k] = o + a.b1[c];
    }
    __syncthreads();
    // the heads, the loss terms and d loss / d material, one thread per shading point
    if (t < kMsPts) {
      const int q = t;
      float mv[2][5];
#pragma unroll
      for (int sx = 0; sx < 2; ++sx) {
        const float* so = s.o[2 * q + sx];
        mv[sx][0] = sigmoidf(so[0] - 1.0f); mv[sx][1] = sigmoidf(so[1] - 1.0f); mv[sx][2] = sigmoidf(so[2] - 1.0f);
        mv[sx][3] = sigmoidf(so[3] - 1.0f) * (1.0f - r0) + r0;
        mv[sx][4] = sigmoidf(so[4] + 0.0f);
#pragma unroll
        for (int k = 0; k < 5; ++k) s.mat[2 * q + sx][k] = mv[sx][k];
      }
      float dmx[5] = {0, 0, 0, 0, 0}, dmp[5] = {0, 0, 0, 0, 0};
      if (q < np) {
        const int64_t p = p0 + q;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          a.mat_x[p * RC_MAT_CH + k] = mv[0][k];
          a.mat_p[p * RC_MAT_CH + k] = mv[1][k];
        }
        const float lam = (a.lossmult ? a.lossmult[p] : 1.0f) * a.filt_weight[p];
        float term = 0.0f, term_o = 0.0f;
        // albedo: |(a - a') / max(1e-6, max(a, a'))| (tensoir_albedo) or |a - a'|
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float u = mv[0][k], v = nan_to_num(mv[1][k]);
          const float d = u - v;
          if (a.tensoir) {
            const float M = fmaxf(u, v), D = fmaxf(1e-6f, M);
            const float qv = d / D;
            term += fabsf(qv);
            const float g = a.ga * lam * abs_grad(qv);
            const float gD = -(d / (D * D)) * max_grad(M, 1e-6f);      // d q / d D, then through max(1e-6, .)
            dmx[k] = g * (1.0f / D + gD * max_grad(u, v));
            dmp[k] = g * (-1.0f / D + gD * max_grad(v, u));
          } else {
            term += fabsf(d);
            const float g = a.ga * lam * abs_grad(d);
            dmx[k] = g; dmp[k] = -g;
          }
        }
#pragma unroll
        for (int k = 3; k < 5; ++k) {
          const float d = mv[0][k] - nan_to_num(mv[1][k]);
          term_o += fabsf(d);
          const float g = a.go * lam * abs_grad(d);
          dmx[k] = g; dmp[k] = -g;
        }
        const float lp = lam * (a.wa * term + a.wo * term_o);
        a.loss_ray[p] = lp;
        s.loss[q] = lp;
      }
#pragma unroll
      for (int k = 0; k < 5; ++k) { s.dm[2 * q][k] = dmx[k]; s.dm[2 * q + 1][k] = dmp[k]; }
    }
    __syncthreads();
    if (t == 0)
      for (int q = 0; q < np; ++q) loss_acc += (double)s.loss[q];
    if (!grads) continue;
    material_head_bwd(s, kMsE, w1r, r0, acc);
    __syncthreads();
    // d loss / d features = dh W0^T: thread (feature i = t & 31, evaluations (t >> 5) + 4 k)
    const int i = t & 31;
#pragma unroll 1
    for (int k = 0; k < kMsE / 4; ++k) {
      const int e = (t >> 5) + 4 * k, q = e >> 1;
      float d = 0.0f;
      for (int j = 0; j < kMsHid; ++j) d = fmaf(s.w0t[j][i], s.dh[e][j], d);
      if (q < np) a.dfeat[((e & 1) * n + p0 + q) * kMsIn + i] = d;
    }
  }
  if (t == 0) a.loss_part[blockIdx.x] = loss_acc;
  if (!grads) return;
  // the workgroup's partial in the layout's order: bottleneck kernel [32][128], bias [128], pred_brdf kernel [128][10],
  // bias [10]
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

// Blocks [0, col_blocks): grads[c] += the workgroups' partials of column c in workgroup order (16 row groups of 64
// columns, each summing every 16th partial, then the 16 sums in order).  Block col_blocks: loss = mult * (the workgroups'
// loss sums added in a fixed tree) / n.  Both bitwise reproducible.
constexpr int kMsRedCols = 64, kMsRedRows = 16;
__global__ __launch_bounds__(1024) void k_material_smoothness_reduce(const float* __restrict__ part, int nparts,
                                                                     const double* __restrict__ loss_part, float* grads,
                                                                     int col_blocks, float mult, double count,
                                                                     float* __restrict__ loss) {
  const int t = threadIdx.x;
  if ((int)blockIdx.x < col_blocks) {
    __shared__ float s_sum[kMsRedRows][kMsRedCols];
    const int c = blockIdx.x * kMsRedCols + (t & (kMsRedCols - 1)), r = t / kMsRedCols;
    float v = 0.0f;
    if (c < kRcMatSmoothParts)
      for (int z = r; z < nparts; z += kMsRedRows) v += part[(int64_t)z * kRcMatSmoothParts + c];
    s_sum[r][t & (kMsRedCols - 1)] = v;
    __syncthreads();
    if (r == 0 && c < kRcMatSmoothParts) {
      float tot = 0.0f;
      for (int k = 0; k < kMsRedRows; ++k) tot += s_sum[k][t];
      grads[c] += tot;
    }
    return;
  }
  __shared__ double s_loss[1024];
  s_loss[t] = t < nparts ? loss_part[t] : 0.0;
  __syncthreads();
  for (int st = 512; st > 0; st >>= 1) {
    if (t < st) s_loss[t] += s_loss[t + st];
    __syncthreads();
  }
  if (t == 0) loss[0] = mult * (float)(s_loss[0] / count);
}

}  // namespace

int rc_mat_smooth_blocks(int64_t n) {
  const int64_t chunks = (n + kMsPts - 1) / kMsPts;
  return (int)(chunks < kMsMaxBlocks ? chunks : kMsMaxBlocks);
}

void rc_launch_material_smoothness_points(const float* pts, const float* noise, float scale, int64_t n, float* out,
                                          hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_material_smoothness_points, dim3((unsigned)((3 * n + 255) / 256)), dim3(256), 0, st, pts, noise, scale,
                     n, out);
}

void rc_launch_material_smoothness_bwd(const RcMatSmoothArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_material_smoothness_bwd, dim3((unsigned)rc_mat_smooth_blocks(a.n)), dim3(128), 0, st, a);
}

void rc_launch_material_partials_reduce(const float* part, int nparts, const double* loss_part, float* grads, float mult,
                                        double count, float* loss, hipStream_t st) {
  if (nparts <= 0) return;
  const int col_blocks = grads ? (kRcMatSmoothParts + kMsRedCols - 1) / kMsRedCols : 0;
  hipLaunchKernelGGL(k_material_smoothness_reduce, dim3((unsigned)(col_blocks + 1)), dim3(1024), 0, st, part, nparts,
                     loss_part, grads, col_blocks, mult, count, loss);
}

void rc_launch_material_smoothness_reduce(const RcMatSmoothArgs& a, float* grads, float mult, float* loss, hipStream_t st) {
  if (a.n <= 0) return;
  rc_launch_material_partials_reduce(a.part, rc_mat_smooth_blocks(a.n), a.loss_part, grads, mult, (double)a.n, loss, st);
}
