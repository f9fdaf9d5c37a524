// Geometry losses of the cache stage on the last sampler level and the density-grid regularizer.
//
// Per ray, on ray_history[-1] (S <= 32 samples), w = weights * lossmult (sampling.py:645-647):
//   distortion   mean(lossfun_distortion(c, w)), c = power_ladder(tdist, p, premult)    loss_utils.py:108-123,
//                lossfun_distortion = sum_ij w_i w_j |u_i - u_j| + sum_i w_i^2 (c_{i+1} - c_i) / 3   stepfun.py:253-269
//   orientation  mean(| sum_i |w_i min(0, n^_i . v)^2| + 1e-5 |), v = -viewdir            loss_utils.py:126-165
//   predicted    mean(| sum_i |w_i (1 - n_i . n^_i)| + 1e-5 |), n = the analytic normals (stop_gradient), w through
//                stopgrad_with_weight(w, pn_wgrad)                                       loss_utils.py:168-201
//   reverse      the same value, stop_gradient(w)                                        train_utils.py:1073-1093
// n^ = normals_pred = nan_to_num(-l2_normalize(W_n h + b_n)); tdist carries no gradient (sampling.py:354-355).  JAX rules:
// lax.abs' JVP is select(x >= 0, g, -g); d min(0, y)^2 / dy = 2 min(0, y) (0 at the tie); nan_to_num passes the gradient
// where its input is finite; l2_normalize's override_gradient (rc_dev_bwd.h).
//
// Kernels:
//   k_geometry_loss_bwd  one wave per ray, one lane per sample: the last level's weights (written to the workspace: the
//                        training forward stops behind the density MLP), the four per-ray loss values (loss_ray [4][n], reduced
//                        in a fixed order by k_interlevel_reduce), d L / d weights of the three terms that reach w, then
//                        d L / d density by the reverse wave scan, and d L / d n^ -> d L / d pred_raw (pred_raw recomputed
//                        in fp32 from hbuf: 64 x 3 FMAs per sample).
//   k_stage_hidden       hbuf (accumulator order) -> h64 [C][64] in the reference's column order, for the
//                        pred_normals_layer weight gradient and d feature64 on k_gemm.
//   k_grid_l2_bwd        one table of a density grid: grad += mult x / numel, per-workgroup sums of x^2 (fixed order).
//   k_grid_l2_reduce     loss = sum over tables of mult * 0.5 * mean(x^2), the partials added in a fixed order.
#include <hip/hip_runtime.h>

#include "rc_dev_bwd.h"
#include "rc_internal.h"

using namespace rcdev;

namespace {

__device__ __forceinline__ float sgn_ge(float x) { return x >= 0.0f ? 1.0f : -1.0f; }     // lax.abs' JVP factor

__global__ void __launch_bounds__(256) k_geometry_loss_bwd(RcGeometryLossArgs a) {
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
  const float w = wt * lm;

  // --- distortion on c = power_ladder(tdist)
  const float c0 = power_ladder(t0, a.dist_p, a.dist_premult), c1 = power_ladder(t1, a.dist_p, a.dist_premult);
  const float ut = (c1 + c0) * 0.5f, dt = c1 - c0;
  float inner = 0.0f;                         // sum_j w_j |u_i - u_j|
  for (int j = 0; j < S; ++j) inner += readlane_f(w, j) * fabsf(ut - readlane_f(ut, j));
  const float dist = wave_sum(act ? w * inner : 0.0f) + wave_sum(act ? w * w * dt : 0.0f) / 3.0f;
  float gw = a.dist_coef * (2.0f * inner + 2.0f * w * dt / 3.0f);

  // --- orientation on n^ = normals_pred
  const float vx = -a.viewdirs[3 * ray], vy = -a.viewdirs[3 * ray + 1], vz = -a.viewdirs[3 * ray + 2];
  const float nx = act ? fix_nan(a.normals_pred[p]) : 0.0f, ny = act ? fix_nan(a.normals_pred[np + p]) : 0.0f,
              nz = act ? fix_nan(a.normals_pred[2 * np + p]) : 0.0f;
  const float ndv = nx * vx + ny * vy + nz * vz;
  const float mn = fminf(0.0f, ndv);
  const float xo = w * (mn * mn);
  const float so = wave_sum(act ? fabsf(xo) : 0.0f);
  const float go = a.orient_coef * sgn_ge(so + 1e-5f) * sgn_ge(xo);     // d L / d xo
  gw += go * (mn * mn);
  const float gdot_o = go * w * 2.0f * mn;                               // d L / d (n^ . v)

  // --- predicted normals (forward and reverse: the same value, n = the analytic normals, stopped)
  const float gx = act ? fix_nan(a.normals_grad[p]) : 0.0f, gy = act ? fix_nan(a.normals_grad[np + p]) : 0.0f,
              gz = act ? fix_nan(a.normals_grad[2 * np + p]) : 0.0f;
  const float e = 1.0f - (gx * nx + gy * ny + gz * nz);
  const float xp = w * e;
  const float sp = wave_sum(act ? fabsf(xp) : 0.0f);
  const float gp = sgn_ge(sp + 1e-5f) * sgn_ge(xp);                    // per unit of the term's coefficient
  gw += a.pn_coef * a.pn_wgrad * gp * e;
  const float gdot_p = -(a.pn_coef + a.pnr_coef) * gp * w;             // d L / d (n . n^)

  if (lane == 0) {
    a.loss_ray[ray] = dist;
    a.loss_ray[a.n + ray] = fabsf(so + 1e-5f);
    a.loss_ray[2 * a.n + ray] = fabsf(sp + 1e-5f);
    a.loss_ray[3 * a.n + ray] = fabsf(sp + 1e-5f);
  }
  if (!a.d_density) return;                   // wave-uniform: losses only

  // --- d L / d density: w = weights * lossmult, then compute_alpha_weights backward
  const float g = act ? gw * lm : 0.0f;
  const float adelta = act ? fabsf((t1 - t0) * dnorm) : 0.0f;
  const float x = act ? dens * adelta : 0.0f;
  const float dx_k = alpha_weights_bwd(g, act ? g * wt : 0.0f, x, lane);
  if (act) a.d_density[p] = dx_k * adelta;

  // --- d L / d pred_raw: n^ = nan_to_num(-l2_normalize(pred_raw))
  if (!act) return;
  const float gnx = gdot_o * vx + gdot_p * gx, gny = gdot_o * vy + gdot_p * gy, gnz = gdot_o * vz + gdot_p * gz;
  const float* hb = a.hbuf + (p >> 5) * (32 * 64) + (p & 31);
  float rx = 0.0f, ry = 0.0f, rz = 0.0f;
  for (int i = 0; i < 64; ++i) {
    const float hv = hb[hbuf_offset(i)];
    rx += hv * a.wn[3 * i]; ry += hv * a.wn[3 * i + 1]; rz += hv * a.wn[3 * i + 2];
  }
  rx += a.wn[192]; ry += a.wn[193]; rz += a.wn[194];
  float dpx, dpy, dpz;
  l2_normalize_bwd(rx, ry, rz, -gnx, -gny, -gnz, dpx, dpy, dpz);
  a.d_pred[3 * p] = dpx; a.d_pred[3 * p + 1] = dpy; a.d_pred[3 * p + 2] = dpz;
}

__global__ void __launch_bounds__(256) k_stage_hidden(const float* __restrict__ hbuf, int64_t c0, int64_t C, float* __restrict__ h64) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= C * 64) return;
  const int64_t p = i >> 6;
  const int col = (int)(i & 63);
  const int64_t g = c0 + p;
  h64[i] = hbuf[(g >> 5) * (32 * 64) + hbuf_offset(col) + (g & 31)];
}

constexpr int kL2Blocks = 256;                // workgroups per table (fixed: the partials' order does not depend on the GPU)

__global__ void __launch_bounds__(256) k_grid_l2_bwd(const float* __restrict__ x, int64_t count, float gscale,
                                                     float* __restrict__ grad, double* __restrict__ part) {
  __shared__ double s[256];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)kL2Blocks * 256) {
    const float v = x[i];
    acc += (double)v * (double)v;
    if (grad) grad[i] += gscale * v;
  }
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) s[threadIdx.x] += s[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}

__global__ void __launch_bounds__(256) k_grid_l2_reduce(const double* __restrict__ part, RcGridL2Reduce r, float* loss) {
  __shared__ double s[256];
  double total = 0.0;
  for (int t = 0; t < r.tables; ++t) {
    s[threadIdx.x] = part[t * kL2Blocks + threadIdx.x];
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if ((int)threadIdx.x < st) s[threadIdx.x] += s[threadIdx.x + st];
      __syncthreads();
    }
    if (threadIdx.x == 0) total += 0.5 * (s[0] / (double)r.count[t]);
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = (float)((double)r.mult * total);
}

}  // namespace

void rc_launch_geometry_loss_bwd(const RcGeometryLossArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_geometry_loss_bwd, dim3((unsigned)((a.n + 3) / 4)), dim3(256), 0, st, a);
}

void rc_launch_stage_hidden(const float* hbuf, int64_t c0, int64_t C, float* h64, hipStream_t st) {
  if (C <= 0) return;
  hipLaunchKernelGGL(k_stage_hidden, dim3((unsigned)((C * 64 + 255) / 256)), dim3(256), 0, st, hbuf, c0, C, h64);
}

int rc_grid_l2_blocks() { return kL2Blocks; }

void rc_launch_grid_l2_bwd(const float* x, int64_t count, float gscale, float* grad, double* part, hipStream_t st) {
  hipLaunchKernelGGL(k_grid_l2_bwd, dim3(kL2Blocks), dim3(256), 0, st, x, count, gscale, grad, part);
}

void rc_launch_grid_l2_reduce(const double* part, const RcGridL2Reduce& r, float* loss, hipStream_t st) {
  hipLaunchKernelGGL(k_grid_l2_reduce, dim3(1), dim3(256), 0, st, part, r, loss);
}
