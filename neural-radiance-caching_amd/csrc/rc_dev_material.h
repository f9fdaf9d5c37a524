// The material head's backward, shared by the material network's losses: k_material_smoothness_bwd
// (rc_material_bwd.hip) and k_material_data_head_bwd (rc_material_data.hip), and the shading frame
// (render_utils.get_rotation_matrix) of rc_material.hip and rc_mask.hip.  Device code only; include after
// rc_internal.h.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// Shading frames of the material stage (rc_material.hip) and of the backward mask rays (rc_mask.hip).
struct V3 { float x, y, z; };
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// render_utils.get_rotation_matrix (y_up=False): columns (new_x, new_y, normal)
struct Frame { V3 x, y, z; };
__device__ __forceinline__ Frame make_frame(V3 n) {
  const V3 up = fabsf(n.z) < 0.9f ? V3{0.0f, 0.0f, 1.0f} : V3{0.0f, 1.0f, 0.0f};
  V3 nx = cross(up, n);
  float l = sqrtf(dot(nx, nx)) + 1e-10f;
  nx = {nx.x / l, nx.y / l, nx.z / l};
  V3 ny = cross(n, nx);
  l = sqrtf(dot(ny, ny)) + 1e-10f;
  ny = {ny.x / l, ny.y / l, ny.z / l};
  return {nx, ny, n};
}
// global_to_local: d0 * R[0,:] + d1 * R[1,:] + d2 * R[2,:] with R[i,:] = (x_i, y_i, z_i)
__device__ __forceinline__ V3 to_local(V3 d, const Frame& f) {
  return {d.x * f.x.x + d.y * f.x.y + d.z * f.x.z, d.x * f.y.x + d.y * f.y.y + d.z * f.y.z,
          d.x * f.z.x + d.y * f.z.y + d.z * f.z.z};
}
// local_to_global: d0 * R[:,0] + d1 * R[:,1] + d2 * R[:,2]
__device__ __forceinline__ V3 to_global(V3 d, const Frame& f) {
  return {d.x * f.x.x + d.y * f.y.x + d.z * f.z.x, d.x * f.x.y + d.y * f.y.y + d.z * f.z.y,
          d.x * f.x.z + d.y * f.y.z + d.z * f.z.z};
}
constexpr int kMsPts = 8;                  // shading points per chunk
constexpr int kMsE = 2 * kMsPts;           // evaluations per chunk: e = 2 q + s, s = 0 at x, 1 at x'
constexpr int kMsHid = 128;                // bottleneck width
constexpr int kMsIn = 32;                  // material grid features
// the five pred_brdf_layer outputs the loss reads: albedo 0..2, roughness 6, metalness 8
__constant__ int kMsCol[5] = {0, 1, 2, 6, 8};

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }   // as rc_material.hip
__device__ __forceinline__ float nan_to_num(float v) {                                    // jnp.nan_to_num
  if (v != v) return 0.0f;
  if (isinf(v)) return v > 0.0f ? 3.40282347e38f : -3.40282347e38f;
  return v;
}
__device__ __forceinline__ float abs_grad(float v) { return v >= 0.0f ? 1.0f : -1.0f; }  // _abs_jvp_rule
// d jnp.maximum(u, v) / d u with the tie rule
__device__ __forceinline__ float max_grad(float u, float v) { return u > v ? 1.0f : (u == v ? 0.5f : 0.0f); }

struct MsShared {
  float f[kMsE][kMsIn];                    // features of the chunk's evaluations
  float h[kMsE][kMsHid + 1];               // bottleneck outputs (rows padded: the per-output sums read across rows)
  float dh[kMsE][kMsHid + 1];              // d loss / d bottleneck outputs
  float w0t[kMsHid][kMsIn];                // W0 transposed: [hidden][feature]
  float w1[kMsHid * 10];                   // W1 [128][10]
  float o[kMsE][5];                        // the five used outputs of pred_brdf_layer (after the bias)
  float dm[kMsE][5];                       // d loss / d (albedo rgb, roughness, metalness)
  float mat[kMsE][5];                      // the material values (before nan_to_num)
  float loss[kMsPts];                      // the chunk's per-point loss sums
};

// The material head's backward on one chunk of `E` evaluations, given d loss / d (albedo rgb, roughness, metalness) per
// evaluation (s.dm) and the forward's features (s.f), bottleneck outputs (s.h) and materials (s.mat): d loss / d b of the
// sigmoid heads, the weight gradients of both dense layers added to the caller's registers (thread t: column t of W0 and
// b0, row t of W1; threads t < 10: b1[t]), and d loss / d features into s.dh -> dfeat.  Shared by k_material_smoothness_bwd and
// k_material_data_head_bwd (rc_material_data.hip).
struct MsAcc { float dw0[kMsIn]; float db0; float dw1[5]; float db1; };

__device__ __forceinline__ void material_head_bwd(MsShared& s, int E, const float (&w1r)[5], float r0, MsAcc& acc) {
  const int t = threadIdx.x;
  // d loss / d b[c] of the five used outputs (lax.logistic: g ans (1 - ans)); recomputed per thread from s.mat
#pragma unroll 1
  for (int e = 0; e < E; ++e) {
    float db[5];
#pragma unroll
    for (int k = 0; k < 3; ++k) { const float a = s.mat[e][k]; db[k] = s.dm[e][k] * (a * (1.0f - a)); }
    const float s6 = sigmoidf(s.o[e][3] - 1.0f);
    db[3] = s.dm[e][3] * (1.0f - r0) * (s6 * (1.0f - s6));
    const float m = s.mat[e][4];
    db[4] = s.dm[e][4] * (m * (1.0f - m));
    // pred_brdf_layer: dh_t = sum_c W1[t][c] db[c]; dW1[t][c] += h_t db[c]; db1[c] += db[c]
    float dh = 0.0f;
#pragma unroll
    for (int k = 0; k < 5; ++k) dh = fmaf(w1r[k], db[k], dh);
    const float hv = s.h[e][t];
#pragma unroll
    for (int k = 0; k < 5; ++k) acc.dw1[k] = fmaf(hv, db[k], acc.dw1[k]);
    if (t < 10) {
#pragma unroll
      for (int k = 0; k < 5; ++k) if (kMsCol[k] == t) acc.db1 += db[k];
    }
    // bottleneck_layer (no activation): dW0[i][t] += f_i dh_t; db0[t] += dh_t
    acc.db0 += dh;
#pragma unroll
    for (int i = 0; i < kMsIn; ++i) acc.dw0[i] = fmaf(s.f[e][i], dh, acc.dw0[i]);
    s.dh[e][t] = dh;
  }
}

}  // namespace
