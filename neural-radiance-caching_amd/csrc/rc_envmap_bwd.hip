// The model-level EnvMap's gradient of the material stage's data loss: the kernels behind the
// envmap_grads of rc_material_data_backward_env (rc_material_data_host.inc).
//
// Model._handle_env_map (internal/models.py:360-421) queries params/Cache/EnvMap (SurfaceLightFieldMLP as configured by
// NeRFModel.env_map_params, internal/surface_light_field.py:480-499, 1011-1058) at the secondary rays' directions:
//   x = pos_enc(d, 0, 4, append_identity) [27] -> layer_0, layer_1, layer_2 (256, ReLU) -> concat([., x]) [283] ->
//   layer_bottleneck (128, ReLU) -> output_rgba_layer [4];  rgb = clip(softplus(raw[:3] + rgb_bias), 0, inf).
// d is stopped (Trainer.stopgrad = True), so the backward ends at the weights.  k_material_data_env_bwd
// (rc_material_data.hip) gives d loss / d rgb per secondary ray; here, per chunk of rows:
//   k_envmap_stage    the encoded rows, k_envmap's sinf arguments, beside layer_2's output in the [C][288] buffer
//   k_gemm_tile       the dense layers (the thin 128 -> 4 output layer stays on k_gemm): the fp32 recompute (X W + b,
//                     ReLU), dX = dY W^T masked by ReLU', dW = X^T dY and db over fixed K slices (summed by k_sum_parts
//                     in slice order: bitwise reproducible)
//   k_envmap_out_bwd  d loss / d rgb -> d loss / d raw: softplus' = sigmoid, the clip's max with JAX's tie rule (half);
//                     the alpha column gets an exact 0.
//
// k_gemm_tile: RcGemmArgs' contract (arbitrary strides, bias, ReLU, mask, accumulate, K slices) on
// v_mfma_f32_32x32x2_f32 with the operands staged through LDS.  A workgroup of four waves owns a 128 x 128 tile of C; per
// step of 16 k it stages a 128 x 16 panel of A and a 16 x 128 panel of B k-major in LDS (row stride 132 floats: 16-byte
// aligned rows), each wave then runs its 2 x 2 tiles of 32 x 32 over the step: 4 LDS reads feed 4 MFMAs, against k_gemm's 2
// strided global loads per MFMA.  A product with fewer such tiles (times K slices) than the device has CUs takes the
// 64 x 64 instantiation (one MFMA tile per wave): the weight gradients, whose C is a layer's kernel.  Global loads are
// 16 bytes wide along whichever axis of an operand is contiguous (rows of X and of W^T along k, columns of X^T and rows
// of W along i / j) when base and strides are 16-byte aligned, single floats otherwise and at the tile edges; the next
// step's panels are loaded into registers before the current step's MFMAs.  LDS reads are 32 consecutive floats per half wave (no bank conflict); the k-major writes of a k-contiguous
// operand are 2-way conflicted (a quarter of the LDS traffic).  The sum over k runs in k_gemm's order.
#include <hip/hip_runtime.h>

#include "rc_internal.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kTk = 16;                    // k per staged step
// WT: MFMA tiles per wave and dimension; a workgroup's tile of C is 64 WT rows and columns, a panel's LDS row stride
// 64 WT + 4 floats

__device__ __forceinline__ float softplus_e(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }

__global__ __launch_bounds__(256) void k_envmap_stage(const float* __restrict__ dirs, int64_t c0, int64_t C,
                                                      float* __restrict__ xb) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= C) return;
  const float* dp = dirs + 3 * (c0 + p);
  const float d[3] = {dp[0], dp[1], dp[2]};
  float* x = xb + p * kRcEnvLdx + kRcEnvWidth;
  // pos_enc(x, 0, 4, append_identity): [x(3), sin(2^j x)(12), sin(2^j x + pi/2)(12)], as k_envmap's enc()
#pragma unroll
  for (int k = 0; k < 3; ++k) x[k] = d[k];
#pragma unroll
  for (int k = 3; k < kRcEnvIn; ++k) {
    const int q = (k - 3) % 12, second = (k - 3) / 12;
    const float sx = d[q % 3] * (float)(1 << (q / 3));
    x[k] = sinf(second ? sx + 1.5707963267948966f : sx);
  }
#pragma unroll
  for (int k = kRcEnvIn; k < kRcEnvLdx - kRcEnvWidth; ++k) x[k] = 0.0f;
}

__global__ __launch_bounds__(256) void k_envmap_out_bwd(const float* __restrict__ d_env, const float* __restrict__ raw,
                                                        float rgb_bias, int64_t c0, int64_t C, float* __restrict__ d_raw) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= C) return;
  f32x4 o;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float z = raw[4 * p + c] + rgb_bias;
    const float y = softplus_e(z);
    const float tie = y > 0.0f ? 1.0f : (y == 0.0f ? 0.5f : 0.0f);       // jnp.clip(y, 0, inf) at y = 0
    o[c] = d_env[3 * (c0 + p) + c] * tie * (1.0f / (1.0f + expf(-z)));
  }
  o[3] = 0.0f;
  *reinterpret_cast<f32x4*>(d_raw + 4 * p) = o;
}

// One operand's panel of a step: element (mn, k) = p[mn s_mn + k s_k], mn in [mn0, mn0 + 64 WT) below MN, k in [k, k + 16)
// below k1, zeros outside.  mode bit 0: the thread mapping (0: a thread takes 4 consecutive k of one row, 1: 4 consecutive
// mn of one k), bit 1: 16-byte loads allowed along that axis.
template <int WT>
__device__ __forceinline__ void panel_load(const float* __restrict__ p, int64_t s_mn, int64_t s_k, int mn0, int MN, int64_t k,
                                           int64_t k1, int mode, float (&v)[4 * WT]) {
  const int t = threadIdx.x;
  constexpr int TPR = 16 * WT;             // threads per k row of the panel in the mn-major mapping
  if (!(mode & 1)) {
#pragma unroll
    for (int q = 0; q < WT; ++q) {
      const int mn = mn0 + (t >> 2) + 64 * q;
      const int64_t kk = k + (t & 3) * 4;
      const bool ok = mn < MN;
      const float* src = p + (int64_t)(ok ? mn : 0) * s_mn + kk * s_k;
      if ((mode & 2) && ok && kk + 3 < k1) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(src);
        v[4 * q] = x[0]; v[4 * q + 1] = x[1]; v[4 * q + 2] = x[2]; v[4 * q + 3] = x[3];
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[4 * q + u] = (ok && kk + u < k1) ? src[u * s_k] : 0.0f;
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < WT; ++q) {
      const int64_t kk = k + t / TPR + (256 / TPR) * q;
      const int mn = mn0 + (t % TPR) * 4;
      const bool ok = kk < k1;
      const float* src = p + (int64_t)mn * s_mn + (ok ? kk : 0) * s_k;
      if ((mode & 2) && ok && mn + 3 < MN) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(src);
        v[4 * q] = x[0]; v[4 * q + 1] = x[1]; v[4 * q + 2] = x[2]; v[4 * q + 3] = x[3];
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[4 * q + u] = (ok && mn + u < MN) ? src[u * s_mn] : 0.0f;
      }
    }
  }
}

// the panel into LDS, k-major: s[k][mn]
template <int WT>
__device__ __forceinline__ void panel_store(float* __restrict__ s, int mode, const float (&v)[4 * WT]) {
  const int t = threadIdx.x;
  constexpr int kLd = 64 * WT + 4, TPR = 16 * WT;
  if (!(mode & 1)) {
#pragma unroll
    for (int q = 0; q < WT; ++q)
#pragma unroll
      for (int u = 0; u < 4; ++u) s[((t & 3) * 4 + u) * kLd + (t >> 2) + 64 * q] = v[4 * q + u];
  } else {
#pragma unroll
    for (int q = 0; q < WT; ++q) {
      f32x4 x;
      x[0] = v[4 * q]; x[1] = v[4 * q + 1]; x[2] = v[4 * q + 2]; x[3] = v[4 * q + 3];
      *reinterpret_cast<f32x4*>(s + (t / TPR + (256 / TPR) * q) * kLd + (t % TPR) * 4) = x;
    }
  }
}

// blockIdx.x = the workgroup's tile of C (row-major over the tiles), blockIdx.y = the K slice.  Wave w: the quarter
// (w >> 1, w & 1) of the tile as WT x WT MFMA tiles; operand and accumulator lanes as k_gemm.  WT = 2: 128 x 128 per
// workgroup; WT = 1: 64 x 64, for products with too few large tiles to fill the device (the weight gradients).
template <int WT>
__global__ __launch_bounds__(256) void k_gemm_tile(RcGemmArgs a, int amode, int bmode) {
  constexpr int kTile = 64 * WT, kLd = kTile + 4;
  __shared__ __attribute__((aligned(16))) float sa[kTk * kLd];
  __shared__ __attribute__((aligned(16))) float sb[kTk * kLd];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tiles_n = (a.N + kTile - 1) / kTile;
  const int i0 = ((int)blockIdx.x / tiles_n) * kTile, j0 = ((int)blockIdx.x % tiles_n) * kTile;
  const int64_t k0 = (int64_t)blockIdx.y * a.kslice;
  const int64_t k1 = k0 + a.kslice < a.K ? k0 + a.kslice : a.K;
  const int wi = i0 + (wave >> 1) * 32 * WT, wj = j0 + (wave & 1) * 32 * WT;
  // wave-uniform: which of the wave's MFMA tiles reach into C at all
  bool live_i[WT], live_j[WT];
#pragma unroll
  for (int x = 0; x < WT; ++x) { live_i[x] = wi + 32 * x < a.M; live_j[x] = wj + 32 * x < a.N; }
  f32x16 acc[WT][WT];
#pragma unroll
  for (int x = 0; x < WT; ++x)
#pragma unroll
    for (int y = 0; y < WT; ++y)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.0f;
  const float* ra = sa + (lane >> 5) * kLd + (wave >> 1) * 32 * WT + (lane & 31);
  const float* rb = sb + (lane >> 5) * kLd + (wave & 1) * 32 * WT + (lane & 31);
  float va[4 * WT], vb[4 * WT];
  if (k0 < k1) {
    panel_load<WT>(a.a, a.sai, a.sak, i0, a.M, k0, k1, amode, va);
    panel_load<WT>(a.b, a.sbj, a.sbk, j0, a.N, k0, k1, bmode, vb);
  }
  for (int64_t k = k0; k < k1; k += kTk) {
    __syncthreads();                       // the previous step's LDS reads are done
    panel_store<WT>(sa, amode, va);
    panel_store<WT>(sb, bmode, vb);
    __syncthreads();
    if (k + kTk < k1) {
      panel_load<WT>(a.a, a.sai, a.sak, i0, a.M, k + kTk, k1, amode, va);
      panel_load<WT>(a.b, a.sbj, a.sbk, j0, a.N, k + kTk, k1, bmode, vb);
    }
#pragma unroll
    for (int s = 0; s < kTk / 2; ++s) {
      float av[WT], bv[WT];
#pragma unroll
      for (int x = 0; x < WT; ++x) { av[x] = ra[2 * s * kLd + 32 * x]; bv[x] = rb[2 * s * kLd + 32 * x]; }
#pragma unroll
      for (int x = 0; x < WT; ++x)
#pragma unroll
        for (int y = 0; y < WT; ++y)
          if (live_i[x] && live_j[y]) acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[x], bv[y], acc[x][y], 0, 0, 0);
    }
  }
  float* c = a.c + (int64_t)blockIdx.y * a.spart;
#pragma unroll
  for (int x = 0; x < WT; ++x)
#pragma unroll
    for (int y = 0; y < WT; ++y) {
      const int j = wj + 32 * y + (lane & 31);
      if (j >= a.N) continue;
      const float bias = a.bias ? a.bias[j] : 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = wi + 32 * x + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (i >= a.M) continue;
        float v = acc[x][y][r];
        if (a.bias) v += bias;
        float* dst = c + (int64_t)i * a.sci + (int64_t)j * a.scj;
        if (a.accumulate) v = *dst + v;
        if (a.relu) v = fmaxf(v, 0.0f);
        if (a.mask && !(a.mask[(int64_t)i * a.smi + (int64_t)j * a.smj] > 0.0f)) v = 0.0f;
        *dst = v;
      }
    }
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

// mode of panel_load for an operand with strides (s_mn, s_k) whose slices start at multiples of kslice
int panel_mode(const float* p, int64_t s_mn, int64_t s_k, int64_t kslice) {
  const bool aligned = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
  if (s_k == 1) return (aligned && s_mn % 4 == 0 && kslice % 4 == 0) ? 2 : 0;
  if (s_mn == 1) return 1 | ((aligned && s_k % 4 == 0) ? 2 : 0);
  return 0;
}

}  // namespace

void rc_launch_envmap_stage(const float* dirs, int64_t c0, int64_t C, float* xb, hipStream_t st) {
  if (C <= 0) return;
  hipLaunchKernelGGL(k_envmap_stage, dim3(blocks_of(C)), dim3(256), 0, st, dirs, c0, C, xb);
}

void rc_launch_envmap_out_bwd(const float* d_env, const float* raw, float rgb_bias, int64_t c0, int64_t C, float* d_raw,
                              hipStream_t st) {
  if (C <= 0) return;
  hipLaunchKernelGGL(k_envmap_out_bwd, dim3(blocks_of(C)), dim3(256), 0, st, d_env, raw, rgb_bias, c0, C, d_raw);
}

void rc_launch_gemm_tile(const RcGemmArgs& a, int kparts, hipStream_t st) {
  if (a.M <= 0 || a.N <= 0) return;
  const int am = panel_mode(a.a, a.sai, a.sak, a.kslice), bm = panel_mode(a.b, a.sbj, a.sbk, a.kslice);
  const int64_t big = (int64_t)((a.M + 127) / 128) * ((a.N + 127) / 128);
  if (big * kparts >= rc_device_cus()) {
    hipLaunchKernelGGL(k_gemm_tile<2>, dim3((unsigned)big, (unsigned)kparts), dim3(256), 0, st, a, am, bm);
  } else {                               // fewer 128 x 128 tiles than CUs: 64 x 64 tiles
    const int small = ((a.M + 63) / 64) * ((a.N + 63) / 64);
    hipLaunchKernelGGL(k_gemm_tile<1>, dim3((unsigned)small, (unsigned)kparts), dim3(256), 0, st, a, am, bm);
  }
}
