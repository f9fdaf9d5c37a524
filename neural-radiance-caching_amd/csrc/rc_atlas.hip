// Texture atlas of a device mesh (rc_atlas_layout, rc_atlas_uvs, rc_atlas_points, rc_query_cache_diffuse, rc_bake_atlas;
// DESIGN.md §4.25).  include/rc_abi.h states the layout rule; tests/atlas_ref.py restates it in numpy.
//
//   k_atlas_uvs               one thread per triangle: the normalised uv of its three corners
//   k_atlas_points            one thread per texel of a range of the linear index y W + x (one texel per lane along x, so
//                             every store is contiguous): owner, barycentrics of the texel centre, the world point as rows
//                             [n][3] and / or as the SoA [3][n] the density MLP reads.  The three vertices of a triangle are
//                             shared by the ~r^2 / 2 texels it owns: the gathers are broadcasts inside a wavefront and hits
//                             in L1 / L2 across them.  No LDS.
//   k_atlas_store             one thread per texel of a chunk: zeros in every plane where the texel has no owner, coverage
//   k_shader_diffuse_points   one thread per point: the two Dense(96 -> 3) heads of the cache shader that need no view
//                             direction, on [hidden vector (k_density_mlp's hbuf) | appearance features], plain fp32
//                             multiply-adds in the reference's column order (576 per point; the weights are uniform and
//                             come through the scalar cache)
//
// The arithmetic is fp32 in the order of tests/atlas_ref.py (-ffp-contract=off keeps multiply and add apart).  No atomics.
#include <hip/hip_runtime.h>

#include "rc_dev_bwd.h"
#include "rc_internal.h"

using namespace rcdev;

namespace {

constexpr int kThreads = 256;

__global__ void __launch_bounds__(kThreads) k_atlas_uvs(RcAtlasLayout L, float* __restrict__ uvs) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= L.T) return;
  const uint32_t cell = (uint32_t)(t >> 1), half = (uint32_t)(t & 1);
  const uint32_t cy = cell / (uint32_t)L.cols, cx = cell - cy * (uint32_t)L.cols;
  const float x0 = (float)(cx * (uint32_t)L.r), y0 = (float)(cy * (uint32_t)L.r), r = (float)L.r;
  // corners in local texel units (exact in fp32: halves below 2^15)
  float lx[3], ly[3];
  if (half == 0) {
    lx[0] = 0.5f; ly[0] = 0.5f; lx[1] = r - 1.5f; ly[1] = 0.5f; lx[2] = 0.5f; ly[2] = r - 1.5f;
  } else {
    lx[0] = r - 0.5f; ly[0] = r - 0.5f; lx[1] = 2.5f; ly[1] = r - 0.5f; lx[2] = r - 0.5f; ly[2] = 2.5f;
  }
  float* o = uvs + 6 * t;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    o[2 * c] = (x0 + lx[c]) / (float)L.W;
    o[2 * c + 1] = 1.0f - (y0 + ly[c]) / (float)L.H;
  }
}

__global__ void __launch_bounds__(kThreads) k_atlas_points(RcAtlasPointsArgs a) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= a.n) return;
  const uint32_t r = (uint32_t)a.L.r, W = (uint32_t)a.L.W;
  const uint32_t lin = (uint32_t)(a.first + idx);                  // W H <= 2^28
  const uint32_t y = lin / W, x = lin - y * W;
  const uint32_t cx = x / r, cy = y / r, i = x - cx * r, j = y - cy * r;
  const int64_t cell = (int64_t)cy * a.L.cols + cx;
  const uint32_t half = i + j >= r ? 1u : 0u;
  const int64_t t = 2 * cell + half;
  int32_t owner = -1;
  float p[3] = {0.0f, 0.0f, 0.0f};
  if (cell < a.L.ncells && t < a.L.T) {
    const int32_t i0 = a.triangles[3 * t], i1 = a.triangles[3 * t + 1], i2 = a.triangles[3 * t + 2];
    // a triangle with an index outside the vertex array is never dereferenced
    const bool ok = i0 >= 0 && i1 >= 0 && i2 >= 0 && (int64_t)i0 < a.V && (int64_t)i1 < a.V && (int64_t)i2 < a.V;
    owner = ok ? (int32_t)t : -2;
    if (ok) {
      const float b1 = half ? (float)(r - 1u - i) / (float)(r - 3u) : (float)i / (float)(r - 2u);
      const float b2 = half ? (float)(r - 1u - j) / (float)(r - 3u) : (float)j / (float)(r - 2u);
      const float* v0 = a.vertices + 3 * (int64_t)i0, * v1 = a.vertices + 3 * (int64_t)i1, * v2 = a.vertices + 3 * (int64_t)i2;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float o = v0[c];
        p[c] = (o + b1 * (v1[c] - o)) + b2 * (v2[c] - o);
      }
    }
  }
  if (a.owner) a.owner[idx] = owner;
  if (a.rows) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a.rows[3 * idx + c] = p[c];
  }
  if (a.soa) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a.soa[c * a.n + idx] = p[c];
  }
}

__global__ void __launch_bounds__(kThreads) k_atlas_store(RcAtlasStoreArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.n) return;
  const bool owned = a.owner[i] >= 0;
  if (a.coverage) a.coverage[i] = owned ? 1 : 0;
  if (owned) return;
  if (a.density) a.density[i] = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (a.normals_pred) a.normals_pred[3 * i + c] = 0.0f;
    if (a.normals) a.normals[3 * i + c] = 0.0f;
  }
  if (a.material) {
#pragma unroll
    for (int c = 0; c < RC_MAT_CH; ++c) a.material[RC_MAT_CH * i + c] = 0.0f;
  }
  if (a.diffuse) {
#pragma unroll
    for (int c = 0; c < 6; ++c) a.diffuse[6 * i + c] = 0.0f;
  }
}

// nerf.py:965-969 (ambient_diffuse) and :1008-1012 (indirect_diffuse): clip(softplus(Dense(feature) + bias), 0, rgb_max)
__global__ void __launch_bounds__(kThreads) k_shader_diffuse_points(RcDiffuseArgs a) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= a.n) return;
  const float* __restrict__ wa = a.w;                      // [96][3] then bias [3]
  const float* __restrict__ wi = a.w + (96 * 3 + 3);
  const float* hb = a.hbuf + (p >> 5) * (32 * 64) + (p & 31);
  float acc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int i = 0; i < 96; ++i) {
    const float f = i < 64 ? hb[hbuf_offset(i)] : a.app[(int64_t)(i - 64) * a.ld + p];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      acc[c] += f * wa[3 * i + c];
      acc[3 + c] += f * wi[3 * i + c];
    }
  }
  float* o = a.out + 6 * p;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    o[c] = fminf(fmaxf(softplus_f((acc[c] + wa[96 * 3 + c]) + a.ambient_bias), 0.0f), a.rgb_max);
    o[3 + c] = fminf(fmaxf(softplus_f((acc[3 + c] + wi[96 * 3 + c]) + a.irradiance_bias), 0.0f), a.rgb_max);
  }
}

inline dim3 blocks_for(int64_t n) { return dim3((unsigned)((n + kThreads - 1) / kThreads)); }

}  // namespace

int rc_atlas_layout_of(int64_t T, int32_t r, RcAtlasLayout& L) {
  if (T < 1 || r < 4 || r > 64) return RC_ERR_INVALID_ARG;
  const int64_t ncells = T / 2 + (T & 1);
  constexpr int64_t kMaxSide = 16384;
  if (ncells > (kMaxSide / 4) * (kMaxSide / 4)) return RC_ERR_UNSUPPORTED;      // cols > 4096: W > 16384 at any r
  int64_t cols = (int64_t)sqrt((double)ncells);
  while (cols * cols < ncells) ++cols;
  while (cols > 1 && (cols - 1) * (cols - 1) >= ncells) --cols;
  const int64_t rows = (ncells + cols - 1) / cols;
  if (cols * r > kMaxSide || rows * r > kMaxSide) return RC_ERR_UNSUPPORTED;
  L.cols = (int32_t)cols; L.rows = (int32_t)rows; L.W = (int32_t)(cols * r); L.H = (int32_t)(rows * r); L.r = r;
  L.T = T; L.ncells = ncells;
  return RC_OK;
}

void rc_launch_atlas_uvs(const RcAtlasLayout& L, float* uvs, hipStream_t stream) {
  if (L.T > 0) hipLaunchKernelGGL(k_atlas_uvs, blocks_for(L.T), dim3(kThreads), 0, stream, L, uvs);
}
void rc_launch_atlas_points(const RcAtlasPointsArgs& a, hipStream_t stream) {
  if (a.n > 0) hipLaunchKernelGGL(k_atlas_points, blocks_for(a.n), dim3(kThreads), 0, stream, a);
}
void rc_launch_atlas_store(const RcAtlasStoreArgs& a, hipStream_t stream) {
  if (a.n > 0) hipLaunchKernelGGL(k_atlas_store, blocks_for(a.n), dim3(kThreads), 0, stream, a);
}
void rc_launch_shader_diffuse_points(const RcDiffuseArgs& a, hipStream_t stream) {
  if (a.n > 0) hipLaunchKernelGGL(k_shader_diffuse_points, blocks_for(a.n), dim3(kThreads), 0, stream, a);
}
