// Data loss of the cache pass and its backward through the compositing, the cache shader and the level-2 heads
// (DESIGN.md §4.7).
//
// Replaces, for the hotdog cache stage (MaterialModel, use_material=False), the part of jax.value_and_grad(loss_fn)
// that train_utils.compute_data_loss (internal/train_utils.py:402-528, loss_type 'charb') contributes:
//   L = mult * mean_{n x 3}(lossmult * sqrt((rgb - gt)^2 + charb_padding^2)),
//   rgb = sum_s w_s rgb_s + max(0, 1 - acc) bg          (render.py:172-247, bg = 1)
// sdist carries no gradient (sampling.py:354-355), so L reaches MLP_2 (grid, layers, pred_normals_layer) and the
// Cache/Shader layers only.  JAX derivative rules restated here:
//   * jnp.maximum / jnp.clip pass HALF of the gradient to each side at a tie (lax.max's balanced-eq JVP);
//   * ref_utils.l2_normalize: forward x / sqrt(max(tiny, |x|^2)), backward through x / sqrt(max(eps, |x|^2)), zero
//     output (and gradient) where |x|^2 < tiny;  ReLU'(0) = 0.
//
// Kernels:
//   k_data_loss_bwd   one wave per ray (S <= 32): charb term, d L / d rgb, d L / d rgb_s = w_s d L / d rgb, d L / d w_s
//                     (background term under the tie rule) and d L / d density_s by the reverse wave scan of
//                     k_interlevel_bwd.  Per-ray sums go to loss_ray (reduced in a fixed order by k_interlevel_reduce).
//   k_gemm            C = op(A) op(B) on v_mfma_f32_32x32x2_f32 with arbitrary strides: every dense layer of the
//                     shader's recompute (X W + b, ReLU), its input gradients (dY W^T, masked by ReLU') and its weight
//                     gradients (X^T dY with the sample axis as K, split into fixed slices).  One wave = one 32 x 32 tile.
//   k_sum_parts       grads += the K-slices of k_gemm in slice order (bitwise reproducible weight gradients).
//   k_stage_feature   feature96 = [hidden vector (hbuf's accumulator order -> reference column order) | appearance].
//   k_shader_glue_fwd n.(-v), reflect, the IDE and the head activations of the recompute.
//   k_shader_out_bwd  the rgb sum, its clamps, tint * ibrdf * SLF ambient -> d L / d (heads, ibrdf logit, ambient logit).
//   k_shader_glue_bwd IDE w.r.t. refdir and roughness, reflect, n.(-v), the l2_normalize override -> d L / d pred_raw,
//                     d L / d bottleneck, d L / d roughness logit.
//   k_split_feature   d L / d feature96 -> d feature64 [n, 64] (rc_density_backward) | d app32 [n, 32] (grid 3 scatter).
#include <hip/hip_runtime.h>

#include "rc_dev_bwd.h"
#include "rc_internal.h"

using namespace rcdev;

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

// d clip(y, lo, hi) / d y under jnp.clip = minimum(maximum(y, lo), hi) with the balanced tie rule
__device__ __forceinline__ float clip_grad(float y, float lo, float hi) {
  const float a = y > lo ? 1.0f : (y == lo ? 0.5f : 0.0f);
  const float m = fmaxf(y, lo);
  return a * (m < hi ? 1.0f : (m == hi ? 0.5f : 0.0f));
}

__global__ void __launch_bounds__(256) k_data_loss_bwd(RcDataLossArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= a.n) return;                     // wave-uniform
  const int S = a.S;
  const bool act = lane < S;
  const int64_t np = a.n * S;
  const int64_t p = ray * S + lane;
  const float lm = a.lossmult ? a.lossmult[ray] : 1.0f;
  float g[3], term = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float d = a.rgb[3 * ray + c] - a.gt[3 * ray + c];
    const float r = sqrtf(d * d + a.padding * a.padding);
    term += lm * r;
    g[c] = lm == 0.0f ? 0.0f : a.coef * lm * (d / r);
  }
  if (lane == 0) a.loss_ray[ray] = term;
  // background: max(0, 1 - acc) * bg, acc = sum of the weights (no resampling: weights_no_filter == weights)
  const float w = act ? a.weights[p] : 0.0f;
  const float acc = wave_sum(w);
  const float omacc = 1.0f - acc;
  const float tie = omacc > 0.0f ? 1.0f : (omacc == 0.0f ? 0.5f : 0.0f);
  const float g_acc = -a.bg * tie * (g[0] + g[1] + g[2]);
  float gw = g_acc;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float rs = act ? a.shade[(int64_t)(RC_SH_RGB + c) * np + p] : 0.0f;
    gw += g[c] * rs;
    if (act) a.d_rgbs[3 * p + c] = w * g[c];
  }
  // compute_alpha_weights backward: x = density |delta|, d L / d x_k = g_k T_{k+1} - sum_{i>k} g_i w_i
  const float dx = a.directions[3 * ray], dy = a.directions[3 * ray + 1], dz = a.directions[3 * ray + 2];
  const float dnorm = sqrtf(dx * dx + dy * dy + dz * dz);
  const float* td = a.tdist + ray * (S + 1);
  const float adelta = act ? fabsf((td[lane + 1] - td[lane]) * dnorm) : 0.0f;
  const float x = act ? a.density[p] * adelta : 0.0f;
  const float dx_k = alpha_weights_bwd(gw, act ? gw * w : 0.0f, x, lane);
  if (act) a.d_density[p] = dx_k * adelta;
}

// One wave per 32 x 32 tile of C; blockIdx.y = K slice.  Lane l: A(i0 + (l & 31), k + (l >> 5)), B(k + (l >> 5), j0 + (l & 31));
// accumulator register r: row i0 + (r & 3) + 8 (r >> 2) + 4 (l >> 5), column j0 + (l & 31).
__global__ void __launch_bounds__(256) k_gemm(RcGemmArgs a) {
  const int lane = threadIdx.x & 63;
  const int tiles_n = (a.N + 31) >> 5;
  const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= ((a.M + 31) >> 5) * tiles_n) return;     // wave-uniform; no barriers below
  const int i0 = (tile / tiles_n) * 32, j0 = (tile % tiles_n) * 32;
  const int64_t k0 = (int64_t)blockIdx.y * a.kslice;
  const int64_t k1 = k0 + a.kslice < a.K ? k0 + a.kslice : a.K;
  const int ia = i0 + (lane & 31), jb = j0 + (lane & 31), kh = lane >> 5;
  const bool iok = ia < a.M, jok = jb < a.N;
  const float* pa = a.a + (iok ? (int64_t)ia * a.sai : 0);
  const float* pb = a.b + (jok ? (int64_t)jb * a.sbj : 0);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  for (int64_t k = k0; k < k1; k += 16) {
    float av[8], bv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t kk = k + 2 * u + kh;
      const bool ok = kk < k1;
      av[u] = (ok && iok) ? pa[kk * a.sak] : 0.0f;
      bv[u] = (ok && jok) ? pb[kk * a.sbk] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
  }
  float* c = a.c + (int64_t)blockIdx.y * a.spart;
  if (!jok) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = i0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
    if (i >= a.M) continue;
    float v = acc[r];
    if (a.bias) v += a.bias[jb];
    float* dst = c + (int64_t)i * a.sci + (int64_t)jb * a.scj;
    if (a.accumulate) v = *dst + v;
    if (a.relu) v = fmaxf(v, 0.0f);
    if (a.mask && !(a.mask[(int64_t)i * a.smi + (int64_t)jb * a.smj] > 0.0f)) v = 0.0f;
    *dst = v;
  }
}

__global__ void __launch_bounds__(256) k_sum_parts(const float* __restrict__ part, int nparts, int64_t count,
                                                   float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  float s = 0.0f;
  for (int z = 0; z < nparts; ++z) s += part[(int64_t)z * count + i];
  out[i] += s;
}

__global__ void __launch_bounds__(256) k_stage_feature(RcShaderBwdArgs a) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.C) return;
  const int64_t g = a.c0 + p;
  const float* hb = a.hbuf + (g >> 5) * (32 * 64) + (g & 31);
  float* f = a.f96 + p * 96;
  for (int i = 0; i < 64; ++i) f[i] = hb[hbuf_offset(i)];
  for (int i = 0; i < 32; ++i) f[64 + i] = a.app[(int64_t)i * a.np + g];
}

struct Geo { float nx, ny, nz, dot, rx, ry, rz, rough; };

__device__ __forceinline__ Geo geometry(const RcShaderBwdArgs& a, int64_t p, int64_t g) {
  Geo o;
  const float px = a.p3[3 * p], py = a.p3[3 * p + 1], pz = a.p3[3 * p + 2];
  const float s = px * px + py * py + pz * pz;
  const float inv = s < RC_TINY ? 0.0f : 1.0f / sqrtf(fmaxf(RC_TINY, s));
  // nan_to_num(-l2_normalize(p)) (geometry.py:467-471)
  auto fix = [](float v) { return v != v ? 0.0f : fminf(fmaxf(v, -RC_FMAX), RC_FMAX); };
  o.nx = fix(-px * inv); o.ny = fix(-py * inv); o.nz = fix(-pz * inv);
  const int64_t ray = g / a.S;
  const float vx = a.viewdirs[3 * ray], vy = a.viewdirs[3 * ray + 1], vz = a.viewdirs[3 * ray + 2];
  o.dot = o.nx * (-vx) + o.ny * (-vy) + o.nz * (-vz);
  o.rx = 2.0f * o.dot * o.nx + vx; o.ry = 2.0f * o.dot * o.ny + vy; o.rz = 2.0f * o.dot * o.nz + vz;
  o.rough = softplus_f(a.heads[p * 10] + a.roughness_bias);
  return o;
}

// IDE term i of (x, y, z) at roughness: Re / Im of (x + i y)^m * P_lm(z) * exp(-sigma_l rough) (ref_utils.py:155-190)
__global__ void __launch_bounds__(256) k_shader_glue_fwd(RcShaderBwdArgs a) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.C) return;
  const Geo o = geometry(a, p, a.c0 + p);
  a.ib_in[p * 129 + 128] = o.dot;
  float* ide = a.x328 + p * 328 + 256;
  float cre = 1.0f, cim = 0.0f;
  int mcur = 0;
  for (int i = 0; i < RC_IDE_TERMS; ++i) {
    const int m = a.ide->m[i];
    if (m < mcur) { cre = 1.0f; cim = 0.0f; mcur = 0; }
    while (mcur < m) { const float nr = cre * o.rx - cim * o.ry; cim = cre * o.ry + cim * o.rx; cre = nr; ++mcur; }
    float poly = 0.0f, zp = 1.0f;
    for (int k = 0; k < RC_IDE_ZPOW; ++k) { poly += kRcIdeCoef[i][k] * zp; zp *= o.rz; }
    const float att = expf(-a.ide->sigma[i] * o.rough);
    ide[i] = cre * poly * att;
    ide[RC_IDE_TERMS + i] = cim * poly * att;
  }
}

// rgb_c = clip(softplus(amb_c + b), 0, M) + clip(softplus(irr_c + b), 0, M) + clip(tint_c ibrdf slf_c, 0, M)
// (ambient_specular is an exact 0 and passes no gradient: it multiplies by 1 - ref_acc = 0)
__global__ void __launch_bounds__(256) k_shader_out_bwd(RcShaderBwdArgs a) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.C) return;
  const float* hd = a.heads + p * 10;        // 0 roughness | 1-3 ambient | 4-6 tint | 7-9 irradiance (pre-activation)
  float* dh = a.dheads + p * 10;
  const float ib = sigm(a.io[p] + 1.0986123f);
  float dib = 0.0f;
  for (int c = 0; c < 3; ++c) {
    const float g = a.d_rgbs[3 * (a.c0 + p) + c];
    const float ya = softplus_f(hd[1 + c] + a.ambient_bias);
    dh[1 + c] = g * clip_grad(ya, 0.0f, a.rgb_max) * sigm(hd[1 + c] + a.ambient_bias);
    const float yi = softplus_f(hd[7 + c] + a.irradiance_bias);
    dh[7 + c] = g * clip_grad(yi, 0.0f, a.rgb_max) * sigm(hd[7 + c] + a.irradiance_bias);
    const float so = a.so[p * 3 + c] + a.slf_ambient_bias;
    const float ys = softplus_f(so);
    const float amb = fmaxf(ys, 0.0f);
    const float tint = sigm(hd[4 + c]);
    const float gis = g * clip_grad(tint * ib * amb, 0.0f, a.rgb_max);
    dh[4 + c] = gis * ib * amb * tint * (1.0f - tint);
    dib += gis * tint * amb;
    a.dso[p * 3 + c] = gis * tint * ib * (ys > 0.0f ? 1.0f : (ys == 0.0f ? 0.5f : 0.0f)) * sigm(so);
  }
  a.dio[p] = dib * ib * (1.0f - ib);
  dh[0] = 0.0f;
}

__global__ void __launch_bounds__(256) k_shader_glue_bwd(RcShaderBwdArgs a) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.C) return;
  const int64_t g = a.c0 + p;
  const Geo o = geometry(a, p, g);
  // d bottleneck: the SLF input and the integrated-BRDF input
  for (int i = 0; i < 128; ++i) a.db128[p * 128 + i] = a.dx328[p * 328 + 128 + i] + a.dib_in[p * 129 + i];
  // IDE backward
  const float* gide = a.dx328 + p * 328 + 256;
  float drx = 0.0f, dry = 0.0f, drz = 0.0f, drough = 0.0f;
  float cre = 1.0f, cim = 0.0f, pre = 1.0f, pim = 0.0f;   // (x + i y)^m and ^(m - 1)
  int mcur = 0;
  for (int i = 0; i < RC_IDE_TERMS; ++i) {
    const int m = a.ide->m[i];
    if (m < mcur) { cre = 1.0f; cim = 0.0f; pre = 1.0f; pim = 0.0f; mcur = 0; }
    while (mcur < m) {
      pre = cre; pim = cim;
      const float nr = cre * o.rx - cim * o.ry; cim = cre * o.ry + cim * o.rx; cre = nr; ++mcur;
    }
    float poly = 0.0f, dpoly = 0.0f, zp = 1.0f;
    for (int k = 0; k < RC_IDE_ZPOW; ++k) {
      poly += a.ide->coef[i][k] * zp;
      if (k + 1 < RC_IDE_ZPOW) dpoly += (float)(k + 1) * a.ide->coef[i][k + 1] * zp;
      zp *= o.rz;
    }
    const float att = expf(-a.ide->sigma[i] * o.rough);
    const float gr = gide[i], gi = gide[RC_IDE_TERMS + i];
    const float gc = gr * cre + gi * cim;            // d L / d (poly att) per unit of the complex factor
    drough += -a.ide->sigma[i] * att * poly * gc;
    drz += gc * att * dpoly;
    if (m > 0) {
      // d c^m = m c^(m-1) dc:  d L / dx = gRe Re(w) + gIm Im(w),  d L / dy = -gRe Im(w) + gIm Re(w),  w = m c^(m-1)
      const float wr = (float)m * pre, wi = (float)m * pim, gR = gr * poly * att, gI = gi * poly * att;
      drx += gR * wr + gI * wi;
      dry += -gR * wi + gI * wr;
    }
  }
  a.dheads[p * 10] = drough * sigm(a.heads[p * 10] + a.roughness_bias);
  // reflect: r = 2 (n.(-v)) n + v;  the integrated-BRDF input n.(-v)
  const int64_t ray = g / a.S;
  const float vx = a.viewdirs[3 * ray], vy = a.viewdirs[3 * ray + 1], vz = a.viewdirs[3 * ray + 2];
  const float ddot = a.dib_in[p * 129 + 128] + 2.0f * (drx * o.nx + dry * o.ny + drz * o.nz);
  const float gnx = 2.0f * o.dot * drx - ddot * vx, gny = 2.0f * o.dot * dry - ddot * vy, gnz = 2.0f * o.dot * drz - ddot * vz;
  // n = -l2_normalize(p)
  float dpx, dpy, dpz;
  l2_normalize_bwd(a.p3[3 * p], a.p3[3 * p + 1], a.p3[3 * p + 2], -gnx, -gny, -gnz, dpx, dpy, dpz);
  a.dp3[3 * p] = dpx; a.dp3[3 * p + 1] = dpy; a.dp3[3 * p + 2] = dpz;
}

__global__ void __launch_bounds__(256) k_split_feature(const float* __restrict__ df96, int64_t C, float* __restrict__ dfeat,
                                                       float* __restrict__ dapp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= C * 96) return;
  const int64_t p = i / 96;
  const int f = (int)(i - p * 96);
  if (f < 64) dfeat[p * 64 + f] = df96[i];
  else dapp[p * 32 + f - 64] = df96[i];
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

void rc_launch_data_loss_bwd(const RcDataLossArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_data_loss_bwd, dim3((unsigned)((a.n + 3) / 4)), dim3(256), 0, st, a);
}

void rc_launch_gemm(const RcGemmArgs& a, int kparts, hipStream_t st) {
  if (a.M <= 0 || a.N <= 0) return;
  const int tiles = ((a.M + 31) / 32) * ((a.N + 31) / 32);
  hipLaunchKernelGGL(k_gemm, dim3((unsigned)((tiles + 3) / 4), (unsigned)kparts), dim3(256), 0, st, a);
}

void rc_launch_sum_parts(const float* part, int nparts, int64_t count, float* out, hipStream_t st) {
  if (count <= 0) return;
  hipLaunchKernelGGL(k_sum_parts, dim3(blocks_of(count)), dim3(256), 0, st, part, nparts, count, out);
}

void rc_launch_shader_stage(const RcShaderBwdArgs& a, int which, hipStream_t st) {
  if (a.C <= 0) return;
  const dim3 g(blocks_of(a.C)), b(256);
  switch (which) {
    case 0: hipLaunchKernelGGL(k_stage_feature, g, b, 0, st, a); break;
    case 1: hipLaunchKernelGGL(k_shader_glue_fwd, g, b, 0, st, a); break;
    case 2: hipLaunchKernelGGL(k_shader_out_bwd, g, b, 0, st, a); break;
    default: hipLaunchKernelGGL(k_shader_glue_bwd, g, b, 0, st, a); break;
  }
}

void rc_launch_split_feature(const float* df96, int64_t C, float* dfeat, float* dapp, hipStream_t st) {
  if (C <= 0) return;
  hipLaunchKernelGGL(k_split_feature, dim3(blocks_of(C * 96)), dim3(256), 0, st, df96, C, dfeat, dapp);
}
