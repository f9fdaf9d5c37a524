// Gradient THROUGH the analytic normals of the last sampler level, and the geometry smoothness loss that needs it
// (DESIGN.md §4.23).
//
// The forward (k_density_mlp<17, true>) produces n = nan_to_num(-l2_normalize(g)), g = J_c G / R, G[ax] = sum_i J[i][ax] gf[i],
// gf = d raw / d feature = W0 (m0 * (W1 (m1 * w_out))), J the trilinear Jacobian (linear in the tables), m0 / m1 the ReLU
// masks.  Given v = d L / d n this file computes d L / d (tables, W0, W1, w_out); the ReLU network is piecewise linear, so
// nothing flows through the features themselves and the three bias gradients are exact zeros.
//
//   k_normals_bwd        one wave per 32 points, the transposed fp32 MFMA formulation of rc_dev_mlp.h on a stream that
//                        carries [d0 | d1 | out | W1^T | W0^T | d0 | d1]: the forward and the backward chain to gf, G and n
//                        as k_density_mlp runs them; the pull-back of v through nan_to_num, the sign, l2_normalize's
//                        override gradient and the contraction's (symmetric) Jacobian to G^; u = J G^; then the two forward
//                        layers once more, bias slot zero, as W0^T u and W1^T a0 with the masks applied.  Emits point-major
//                        u, t0 = m0 * (W1 t1), a0 = m0 * (W0^T u), t1 = m1 * w_out, a2 = m1 * (W1^T a0) for the weight-gradient
//                        contraction (k_wgrad + k_grad_reduce, rc_train.hip: dW0 = u^T t0, dW1 = a0^T t1, dw_out = sum a2;
//                        fixed order, bias sums switched off), and gf (feature-major) and G^ for the scatter.
//   k_grid_scatter_jac   k_grid_scatter's lane mapping and index arithmetic with the directional derivative of the corner
//                        weight in place of the weight: corner c of level l takes
//                        precondition gf[(l, f)] s_l sum_ax G^[ax] d w_c / d loc_ax on hardware float atomics (order-dependent
//                        in the last bits).  Every level, the 16^3 one included, takes this path.
//   k_gsmooth_points     x' = fl(x + fl(noise * scale)) as SoA means and both point sets as [np][3].
//   k_gsmooth_loss       one wave per ray, one lane per sample: the last level's weights, c = lossmult * weights * S (stopped),
//                        the per-ray loss value and d L / d normals, d L / d density at x and (negated) at x'.
#include <hip/hip_runtime.h>

#include "rc_dev_bwd.h"
#include "rc_dev_grid.h"
#include "rc_dev_mlp.h"

using namespace rcdev;

namespace {

__global__ __launch_bounds__(kWaves * 64) void k_normals_bwd(RcNormalsBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float ring[kRingFloats];
  __shared__ float lds[kWaves][33 * 64];
  constexpr int KS0 = 17;
  constexpr int F_D0 = 0, F_D1 = rc_lfr32(KS0, 2), F_DO = F_D1 + rc_lfr32(33, 2), F_B1 = F_DO + rc_dfr32(1, 2), F_B0 = F_B1 + rc_lfr32(32, 2),
                F_R0 = F_B0 + rc_lfr32(32, 1), F_R1 = F_R0 + rc_lfr32(KS0, 2), NF = F_R1 + rc_lfr32(33, 2);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t tile = (int64_t)blockIdx.x * kWaves + wave;
  const int64_t p0 = tile * 32;
  const int j = lane & 31, h = lane >> 5;
  const int64_t p = p0 + j;
  const bool valid = p < a.n;        // waves past the end stay alive for the workgroup barriers
  const int64_t pp = valid ? p : 0;  // loads of the tail go to a valid address, their values are dropped
  float* act = &lds[wave][lane];
  WStream ws{a.wstream, ring, lane, wave};
  ws_begin<NF>(ws);

  // accumulator register (t, r) of this lane holds feature 32 t + 8 (r >> 2) + 4 h + (r & 3) (k_density_bwd's store_rows)
  auto store_rows = [&](float* dst, const float (&v)[32]) {
    if (!valid) return;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 o = make_float4(v[t * 16 + 4 * q], v[t * 16 + 4 * q + 1], v[t * 16 + 4 * q + 2], v[t * 16 + 4 * q + 3]);
        *reinterpret_cast<float4*>(dst + p * 64 + 32 * t + 8 * q + 4 * h) = o;
      }
  };

  // ---- the forward, as k_density_mlp<17, true>: masks of both hidden layers, w_out in accumulator layout
  {
    float fv[KS0 - 1];
#pragma unroll
    for (int s = 0; s < KS0 - 1; ++s) fv[s] = a.feat[(int64_t)(2 * s + h) * a.ld + pp];
#pragma unroll
    for (int s = 0; s < KS0 - 1; ++s) act[s * 64] = valid ? fv[s] : 0.0f;
  }
  act[(KS0 - 1) * 64] = h == 0 ? 1.0f : 0.0f;
  f32x16 acc[2];
  acc[0] = zero16(); acc[1] = zero16();
  mlp_layer_d<2, KS0, F_D0, NF>(ws, act, acc);
  uint32_t m0 = 0, m1 = 0;           // ReLU masks, bit t*16+r
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) m0 |= (acc[t][r] > 0.0f ? 1u : 0u) << (t * 16 + r);
  park<2, true>(acc, act, 0);
  act[32 * 64] = h == 0 ? 1.0f : 0.0f;
  acc[0] = zero16(); acc[1] = zero16();
  mlp_layer_d<2, 33, F_D1, NF>(ws, act, acc);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) m1 |= (acc[t][r] > 0.0f ? 1u : 0u) << (t * 16 + r);
  float out[1], wout[32];
  dot_out1<2, 1, F_DO, NF, true>(ws, acc, out, wout);

  // ---- the backward chain to gf = d raw / d feature: t1 = m1 * w_out, t0 = m0 * (W1 t1), gf = W0 t0
  float row[32];
#pragma unroll
  for (int s = 0; s < 32; ++s) row[s] = ((m1 >> s) & 1u) ? wout[s] : 0.0f;
  store_rows(a.t1, row);
#pragma unroll
  for (int s = 0; s < 32; ++s) act[s * 64] = row[s];
  f32x16 g[2];
  g[0] = zero16(); g[1] = zero16();
  mlp_layer_d<2, 32, F_B1, NF>(ws, act, g);             // W1 . t1
#pragma unroll
  for (int s = 0; s < 32; ++s) row[s] = ((m0 >> s) & 1u) ? g[s >> 4][s & 15] : 0.0f;
  store_rows(a.t0, row);
#pragma unroll
  for (int s = 0; s < 32; ++s) act[s * 64] = row[s];
  f32x16 gf[1];
  gf[0] = zero16();
  mlp_layer_d<1, 32, F_B0, NF>(ws, act, gf);            // W0 . t0 (32 features, accumulator layout)
  float gw[3] = {0.0f, 0.0f, 0.0f};
  {
    float jv[3][16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = (r & 3) + 8 * (r >> 2) + 4 * h;
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) jv[ax][r] = a.jac[(int64_t)(ax * 32 + i) * a.ld + pp];
    }
    if (valid) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * h;
        a.gf[(int64_t)i * a.ld + p] = gf[0][r];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) gw[ax] += gf[0][r] * jv[ax][r];
      }
    }
  }
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) gw[ax] += __shfl_xor(gw[ax], 32, 64);       // both half-waves hold G

  // ---- G -> g = J_c G / R -> n, and v = d L / d n back to G^ (both half-waves, the same values)
  float gh[3] = {0.0f, 0.0f, 0.0f};
  {
    float zx = 0.0f, zy = 0.0f, zz = 0.0f;   // x / radius
    float vx = 0.0f, vy = 0.0f, vz = 0.0f;
    if (valid) {
      zx = rc_div(a.points[3 * p], a.contract_radius); zy = rc_div(a.points[3 * p + 1], a.contract_radius);
      zz = rc_div(a.points[3 * p + 2], a.contract_radius);
      vx = a.d_normals[3 * p]; vy = a.d_normals[3 * p + 1]; vz = a.d_normals[3 * p + 2];
    }
    // Jacobian of contract at z: w = s(m) z, s = (2 sqrt(m) - 1) / m, m = max(1, |z|^2): s I + 2 s' z z^T, symmetric
    const float msq = zx * zx + zy * zy + zz * zz;
    const bool outer = msq > 1.0f;
    const float rt = sqrtf(msq);
    const float sc = outer ? (2.0f * rt - 1.0f) / msq : 1.0f;
    const float ds2 = outer ? 2.0f * ((1.0f - rt) / (msq * msq)) : 0.0f;
    float gzx = gw[0], gzy = gw[1], gzz = gw[2];
    if (outer) {
      const float gz_dot = gw[0] * zx + gw[1] * zy + gw[2] * zz;
      gzx = sc * gw[0] + ds2 * gz_dot * zx;
      gzy = sc * gw[1] + ds2 * gz_dot * zy;
      gzz = sc * gw[2] + ds2 * gz_dot * zz;
    }
    const float px = rc_div(gzx, a.contract_radius), py = rc_div(gzy, a.contract_radius), pz = rc_div(gzz, a.contract_radius);
    // nan_to_num(-l2_normalize(p)): the gradient passes where the value is finite, then the override gradient
    const float dsq = px * px + py * py + pz * pz;
    const float inv = sqrtf(fmaxf(RC_TINY, dsq));
    const float rx = -(px / inv), ry = -(py / inv), rz = -(pz / inv);
    const bool tiny = dsq < RC_TINY;
    auto finite = [](float x) { return fabsf(x) <= RC_FMAX; };
    const float ux = (!tiny && finite(rx)) ? -vx : 0.0f, uy = (!tiny && finite(ry)) ? -vy : 0.0f, uz = (!tiny && finite(rz)) ? -vz : 0.0f;
    float dpx, dpy, dpz;
    l2_normalize_bwd(px, py, pz, ux, uy, uz, dpx, dpy, dpz);
    const float qx = rc_div(dpx, a.contract_radius), qy = rc_div(dpy, a.contract_radius), qz = rc_div(dpz, a.contract_radius);
    gh[0] = qx; gh[1] = qy; gh[2] = qz;
    if (outer) {
      const float q_dot = qx * zx + qy * zy + qz * zz;
      gh[0] = sc * qx + ds2 * q_dot * zx;
      gh[1] = sc * qy + ds2 * q_dot * zy;
      gh[2] = sc * qz + ds2 * q_dot * zz;
    }
    if (!valid) { gh[0] = 0.0f; gh[1] = 0.0f; gh[2] = 0.0f; }
    if (h == 0 && valid) {
      a.ghat[3 * p] = gh[0]; a.ghat[3 * p + 1] = gh[1]; a.ghat[3 * p + 2] = gh[2];
      a.ones[p] = 1.0f;
      if (a.normals) {
        float nx = px, ny = py, nz = pz;
        neg_normalize(nx, ny, nz);
        a.normals[3 * p] = nx; a.normals[3 * p + 1] = ny; a.normals[3 * p + 2] = nz;
      }
    }
  }

  // ---- u = J G^ in the natural k pairs of layer 0, the bias slot zero
  {
    float jv[3][KS0 - 1];
#pragma unroll
    for (int s = 0; s < KS0 - 1; ++s)
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) jv[ax][s] = a.jac[(int64_t)(ax * 32 + 2 * s + h) * a.ld + pp];
#pragma unroll
    for (int s = 0; s < KS0 - 1; ++s) {
      const float u = valid ? (jv[0][s] * gh[0] + jv[1][s] * gh[1]) + jv[2][s] * gh[2] : 0.0f;
      act[s * 64] = u;
      if (valid) a.u[p * 32 + 2 * s + h] = u;
    }
  }
  act[(KS0 - 1) * 64] = 0.0f;
  acc[0] = zero16(); acc[1] = zero16();
  mlp_layer_d<2, KS0, F_R0, NF>(ws, act, acc);          // W0^T u
#pragma unroll
  for (int s = 0; s < 32; ++s) row[s] = ((m0 >> s) & 1u) ? acc[s >> 4][s & 15] : 0.0f;
  store_rows(a.a0, row);
#pragma unroll
  for (int s = 0; s < 32; ++s) act[s * 64] = row[s];
  act[32 * 64] = 0.0f;
  acc[0] = zero16(); acc[1] = zero16();
  mlp_layer_d<2, 33, F_R1, NF>(ws, act, acc);           // W1^T a0
#pragma unroll
  for (int s = 0; s < 32; ++s) row[s] = ((m1 >> s) & 1u) ? acc[s >> 4][s & 15] : 0.0f;
  store_rows(a.a2, row);
}

// k_grid_scatter (rc_train.hip) with d w_c / d loc in place of w_c: the same lanes per (point, level), the same index and
// weight arithmetic.  gl: G^ in the level's own axis order (dense levels: loc = (z, y, x)).
template <int F>
__global__ __launch_bounds__(256) void k_grid_scatter_jac(RcGridScatterArgs a, const float* __restrict__ ghat) {
  constexpr int G = F == 4 ? 4 : 2;                 // lanes per (point, level)
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t p = gid / G;
  const int sub = (int)(gid % G);
  const int l = blockIdx.y;
  if (p >= a.n) return;
  float x = a.points[3 * p], y = a.points[3 * p + 1], z = a.points[3 * p + 2];
  if (a.contract_radius > 0.0f) contract3(x, y, z, a.contract_radius);
  const RcGridLevel L = a.grid.lvl[l];
  float* __restrict__ gt = a.gtable[l];
  const int f = F == 4 ? sub : 0;
  const float N = (float)L.size;
  // d loc / d contracted coordinate with the precondition factor, as k_hashgrid_fwd<F, true> scales its Jacobian
  const float df = a.dfeat[(int64_t)(l * F + f) * a.ld + p] * (a.grid.precondition * N / (a.grid.bbox - (-a.grid.bbox)));
  const float hx = ghat[3 * p], hy = ghat[3 * p + 1], hz = ghat[3 * p + 2];
  const float cx = unit_box(a.grid.bbox, x) * N, cy = unit_box(a.grid.bbox, y) * N, cz = unit_box(a.grid.bbox, z) * N;
  float cw[3], gl[3];
  int base[3];
  if (L.dense) {
    const float loc[3] = {(cz - 0.5f) + 1.0f, (cy - 0.5f) + 1.0f, (cx - 0.5f) + 1.0f};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) { const float fl = floorf(loc[ax]); cw[ax] = loc[ax] - fl; base[ax] = (int)fl; }
    gl[0] = hz; gl[1] = hy; gl[2] = hx;
  } else {
    const float loc[3] = {cx - 0.5f, cy - 0.5f, cz - 0.5f};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) { const float fl = floorf(loc[ax]); cw[ax] = loc[ax] - fl; base[ax] = (int)fl; }
    gl[0] = hx; gl[1] = hy; gl[2] = hz;
  }
  const float fw[3] = {1.0f - cw[0], 1.0f - cw[1], 1.0f - cw[2]};
#pragma unroll
  for (int cnr = 0; cnr < 8; ++cnr) {
    const int b0 = (cnr >> 2) & 1, b1 = (cnr >> 1) & 1, b2 = cnr & 1;
    if (F == 1 && b0 != sub) continue;             // this lane's corners along the fastest axis
    const float w0 = b0 ? cw[0] : fw[0], w1 = b1 ? cw[1] : fw[1], w2 = b2 ? cw[2] : fw[2];
    const float d0 = w1 * w2, d1 = w0 * w2, d2 = w0 * w1;       // |d w_c / d loc_ax|: the two other axes' weights
    const float dw = ((b0 ? gl[0] : -gl[0]) * d0 + (b1 ? gl[1] : -gl[1]) * d1) + (b2 ? gl[2] : -gl[2]) * d2;
    uint32_t idx;
    bool zero = false;
    if (L.dense) {
      const int k0 = min(max(base[0] + b0, 0), L.size + 1), k1 = min(max(base[1] + b1, 0), L.size + 1),
                k2 = min(max(base[2] + b2, 0), L.size + 1);
      zero = (k0 < 1) | (k0 > L.size) | (k1 < 1) | (k1 > L.size) | (k2 < 1) | (k2 > L.size);   // zero padding: no parameter
      idx = ((uint32_t)(k2 - 1) * (uint32_t)L.size + (uint32_t)(k1 - 1)) * (uint32_t)L.size + (uint32_t)(k0 - 1);
    } else {
      const uint32_t hsh = ((uint32_t)base[0] + (uint32_t)b0) ^ (((uint32_t)base[1] + (uint32_t)b1) * kPi2) ^
                           (((uint32_t)base[2] + (uint32_t)b2) * kPi3);
      idx = L.mask ? (hsh & L.mask) : (hsh % L.entries);
    }
    if (zero) continue;
    unsafeAtomicAdd(gt + (size_t)idx * F + f, dw * df);
  }
}

__global__ __launch_bounds__(256) void k_gsmooth_points(const float* __restrict__ means, const float* __restrict__ noise, float scale,
                                                        int64_t np, float* __restrict__ means_p, float* __restrict__ points,
                                                        float* __restrict__ points_p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= np) return;
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    const float x = means[ax * np + i];
    const float xp = __fadd_rn(x, __fmul_rn(noise[3 * i + ax], scale));     // product and sum rounded separately
    means_p[ax * np + i] = xp;
    points[3 * i + ax] = x;
    points_p[3 * i + ax] = xp;
  }
}

__global__ void __launch_bounds__(256) k_gsmooth_loss(RcGSmoothLossArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= a.n) return;                     // wave-uniform
  const int S = a.S;
  const bool act = lane < S;
  const int64_t np = a.n * S;
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
  const float c = lm * (wt * (float)S);       // lossmult * stop_gradient(weights * S)
  auto sgn = [](float d) { return d >= 0.0f ? 1.0f : -1.0f; };      // lax.abs' JVP factor: +1 at 0
  float sn = 0.0f, dn[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float d = act ? a.normals[k * np + p] - fix_nan(a.normals_p[k * np + p]) : 0.0f;
    sn += d >= 0.0f ? d : -d;
    dn[k] = a.gn * c * sgn(d);
  }
  const float dd = act ? dens - fix_nan(a.density_p[p]) : 0.0f;
  const float sd = dd >= 0.0f ? dd : -dd;
  const float per = act ? c * (a.wn3 * sn + a.wd * sd) : 0.0f;
  const float total = wave_sum(per);
  if (lane == 0) a.loss_ray[ray] = total;
  if (!a.d_normals || !act) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) { a.d_normals[3 * p + k] = dn[k]; a.d_normals_p[3 * p + k] = -dn[k]; }
  if (a.wd != 0.0f) {
    const float g = a.gd * c * sgn(dd);
    a.d_density[p] = g; a.d_density_p[p] = -g;
  }
}

}  // namespace

void rc_launch_normals_bwd(const RcNormalsBwdArgs& a, hipStream_t stream) {
  if (a.n <= 0) return;
  const int64_t tiles = (a.n + 31) / 32;
  hipLaunchKernelGGL(k_normals_bwd, dim3((unsigned)((tiles + kWaves - 1) / kWaves)), dim3(kWaves * 64), 0, stream, a);
}

void rc_launch_grid_scatter_jac(const RcGridScatterArgs& s, const float* ghat, hipStream_t stream) {
  if (s.n <= 0) return;
  const int G = s.grid.num_features == 4 ? 4 : 2;
  dim3 grid((unsigned)((s.n * G + 255) / 256), (unsigned)s.grid.num_levels), block(256);
  if (s.grid.num_features == 4) hipLaunchKernelGGL((k_grid_scatter_jac<4>), grid, block, 0, stream, s, ghat);
  else hipLaunchKernelGGL((k_grid_scatter_jac<1>), grid, block, 0, stream, s, ghat);
}

void rc_launch_gsmooth_points(const float* means, const float* noise, float scale, int64_t np, float* means_p, float* points,
                              float* points_p, hipStream_t st) {
  if (np <= 0) return;
  hipLaunchKernelGGL(k_gsmooth_points, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, means, noise, scale, np, means_p, points,
                     points_p);
}

void rc_launch_gsmooth_loss(const RcGSmoothLossArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_gsmooth_loss, dim3((unsigned)((a.n + 3) / 4)), dim3(256), 0, st, a);
}
