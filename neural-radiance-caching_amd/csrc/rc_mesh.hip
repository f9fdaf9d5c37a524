// Surface export on the device (rc_query_points, rc_density_lattice, rc_isosurface).
//
// The fields at points are the existing forward kernels (k_hashgrid_fwd, k_density_mlp, k_material_head); this file adds
// what stands around them and the extraction:
//
//   k_rows_to_soa, k_soa_to_rows   points [n][3] <-> the SoA [3][n] the density MLP reads and writes
//   k_lattice_points               a slab of the lattice as SoA points: axis point i at lo + (float)i * step, fp32, in this form
//   k_nan_to_num                   jnp.nan_to_num in place
//
// rc_isosurface: marching tetrahedra on the Kuhn decomposition of each lattice cell (reference: the lattice / threshold /
// OBJ contract of internal/mesh_network.py:48-72, 134-139; the triangulation is this project's, rc_iso_table.h).  A
// lattice point owns up to seven edges (rc_iso_table.h), a vertex sits on every owned edge whose ends differ in f >= iso.
//
//   k_iso_classify      one thread per lattice point, a workgroup per tile of 1024 consecutive points (iz runs fastest, so a
//                       wavefront reads contiguous runs of the field; the 7 neighbours of a point are its cell's other
//                       corners and come from rows the neighbouring wavefronts read too): the 7-bit mask of crossing owned
//                       edges, the triangle count of the point's cell, the tile's sums
//   k_iso_scan_tiles    one workgroup per group of 256 tiles: a tile's sums -> the sums of the tiles before it in the group
//   k_iso_scan_groups   one workgroup: the group sums -> 64-bit offsets, the counts {V, T}, and whether the capacities suffice
//   k_iso_vertices      a workgroup per tile, 4 consecutive points per thread: the exclusive scan of popcount(mask) inside
//                       the tile gives each point its first vertex index (kept in vbase where mask != 0); positions, normals
//   k_iso_triangles     the same over the triangle counts; a corner's index is vbase[owner] + popcount(mask[owner] below its edge)
//
// The field is read once in full (k_iso_classify); the emission kernels read one byte per point and the field only at the
// surface.  No float atomics and no atomics at all: every index comes from the scans, so two calls on one lattice are
// bitwise equal.  The arithmetic is fp32 in the order of tests/iso_ref.py (-ffp-contract=off keeps multiply and add apart).
#include <hip/hip_runtime.h>

#include "rc_internal.h"
#include "rc_iso_table.h"

namespace {

constexpr int kThreads = 256;
constexpr int kItems = kRcIsoTile / kThreads;      // lattice points per thread
static_assert(kItems == 4 && kRcIsoGroup == kThreads, "a thread takes one 32-bit word of masks; one thread per tile of a group");

__global__ void __launch_bounds__(kThreads) k_rows_to_soa(const float* rows, int64_t n, float* soa) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) soa[c * n + i] = rows[3 * i + c];
}

__global__ void __launch_bounds__(kThreads) k_soa_to_rows(const float* soa, int64_t n, float* rows) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) rows[3 * i + c] = soa[c * n + i];
}

__device__ __forceinline__ float axis_pos(const RcLatticeArgs& L, int a, uint32_t i) { return L.lo[a] + (float)i * L.step[a]; }

__global__ void __launch_bounds__(kThreads) k_lattice_points(RcLatticeArgs L, int64_t first, int64_t n, float* soa) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = (uint32_t)(first + i);
  const uint32_t iz = p % (uint32_t)L.nz, q = p / (uint32_t)L.nz, iy = q % (uint32_t)L.ny, ix = q / (uint32_t)L.ny;
  soa[i] = axis_pos(L, 0, ix);
  soa[n + i] = axis_pos(L, 1, iy);
  soa[2 * n + i] = axis_pos(L, 2, iz);
}

// jnp.nan_to_num: NaN -> 0, +-inf -> the largest finite float of that sign
__global__ void __launch_bounds__(kThreads) k_nan_to_num(float* x, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  x[i] = v != v ? 0.0f : fminf(fmaxf(v, -RC_FMAX), RC_FMAX);
}

// ---------------------------------------------------------------------------------------------
// rc_isosurface
// ---------------------------------------------------------------------------------------------
// The values of v before this thread in the workgroup, in thread order, and the workgroup's sum.  waves: 4 ints of LDS
// that nothing else touches until the next barrier.
__device__ __forceinline__ int block_scan(int v, int* waves, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int below = __shfl_up(inc, o, 64);
    if (lane >= o) inc += below;
  }
  if (lane == 63) waves[wave] = inc;
  __syncthreads();
  int before = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) before += w < wave ? waves[w] : 0;
  total = (waves[0] + waves[1]) + (waves[2] + waves[3]);
  return before + (inc - v);
}

struct Lattice {
  uint32_t nx, ny, nz, sx, sy;      // sx, sy: strides of ix and iy
  __device__ __forceinline__ explicit Lattice(const RcLatticeArgs& L)
      : nx((uint32_t)L.nx), ny((uint32_t)L.ny), nz((uint32_t)L.nz), sx((uint32_t)L.ny * (uint32_t)L.nz), sy((uint32_t)L.nz) {}
  __device__ __forceinline__ void split(uint32_t p, uint32_t& ix, uint32_t& iy, uint32_t& iz) const {
    iz = p % nz;
    const uint32_t q = p / nz;
    iy = q % ny; ix = q / ny;
  }
  // offset of the corner / direction with code dx | dy << 1 | dz << 2
  __device__ __forceinline__ uint32_t offset(uint32_t code) const { return (code & 1u) * sx + ((code >> 1) & 1u) * sy + (code >> 2); }
};

// edge number -> corner code of its direction (kRcIsoDirCode), three bits each
constexpr uint32_t kDirPack = 1u | 2u << 3 | 4u << 6 | 3u << 9 | 5u << 12 | 6u << 15 | 7u << 18;
static_assert(kRcIsoDirCode[3] == 3 && kRcIsoDirCode[4] == 5 && kRcIsoDirCode[6] == 7, "kDirPack packs kRcIsoDirCode");

// bit c: corner c of the cell at p lies in the lattice and is inside (f >= iso; a NaN is outside); `exists` likewise
__device__ __forceinline__ uint32_t cell_inside(const RcIsoArgs& a, const Lattice& G, uint32_t p, uint32_t& exists) {
  uint32_t ix, iy, iz;
  G.split(p, ix, iy, iz);
  const bool ox = ix + 1 < G.nx, oy = iy + 1 < G.ny, oz = iz + 1 < G.nz;
  uint32_t in = 0;
  exists = 0;
#pragma unroll
  for (uint32_t c = 0; c < 8; ++c) {
    const bool ok = ((c & 1u) == 0 || ox) && ((c & 2u) == 0 || oy) && ((c & 4u) == 0 || oz);
    const float f = ok ? a.field[p + G.offset(c)] : 0.0f;
    exists |= (ok ? 1u : 0u) << c;
    in |= ((ok && f >= a.iso) ? 1u : 0u) << c;
  }
  return in;
}

// inside mask (bit i: v_i) of tetrahedron k from the cell's corner bits
template <int K> __device__ __forceinline__ uint32_t tet_mask(uint32_t in) {
  return ((in >> kRcIso.vert[K][0]) & 1u) | ((in >> kRcIso.vert[K][1]) & 1u) << 1 | ((in >> kRcIso.vert[K][2]) & 1u) << 2 |
         ((in >> kRcIso.vert[K][3]) & 1u) << 3;
}
__device__ __forceinline__ uint32_t tet_triangles(uint32_t m) {      // kRcIso.ntri: 0, 1, 2, 1, 0 by the inside vertices
  const int c = __popc(m);
  return c == 2 ? 2u : ((c == 1 || c == 3) ? 1u : 0u);
}

__global__ void __launch_bounds__(kThreads) k_iso_classify(RcIsoArgs a) {
  __shared__ int waves_v[4], waves_t[4];
  const Lattice G(a.lat);
  const uint32_t tile0 = blockIdx.x * (uint32_t)kRcIsoTile;
  int nv = 0, nt = 0;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const uint32_t p = tile0 + (uint32_t)(j * kThreads) + threadIdx.x;
    uint32_t mask = 0, tris = 0;
    if (p < a.n) {
      uint32_t exists;
      const uint32_t in = cell_inside(a, G, p, exists);
      const uint32_t self = in & 1u;
#pragma unroll
      for (int e = 0; e < 7; ++e) {
        const uint32_t c = (uint32_t)kRcIsoDirCode[e];
        mask |= (((exists >> c) & 1u) & (((in >> c) & 1u) ^ self)) << e;
      }
      if (exists == 0xFFu)
        tris = tet_triangles(tet_mask<0>(in)) + tet_triangles(tet_mask<1>(in)) + tet_triangles(tet_mask<2>(in)) +
               tet_triangles(tet_mask<3>(in)) + tet_triangles(tet_mask<4>(in)) + tet_triangles(tet_mask<5>(in));
    }
    a.mask[p] = (uint8_t)mask;        // the buffers cover whole tiles: zeros behind the lattice
    a.tcount[p] = (uint8_t)tris;
    nv += __popc(mask); nt += (int)tris;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { nv += __shfl_xor(nv, o, 64); nt += __shfl_xor(nt, o, 64); }
  if ((threadIdx.x & 63) == 0) { waves_v[threadIdx.x >> 6] = nv; waves_t[threadIdx.x >> 6] = nt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.tile_v[blockIdx.x] = (waves_v[0] + waves_v[1]) + (waves_v[2] + waves_v[3]);
    a.tile_t[blockIdx.x] = (waves_t[0] + waves_t[1]) + (waves_t[2] + waves_t[3]);
  }
}

__global__ void __launch_bounds__(kThreads) k_iso_scan_tiles(RcIsoArgs a) {
  __shared__ int waves_v[4], waves_t[4];
  const uint32_t tile = blockIdx.x * (uint32_t)kRcIsoGroup + threadIdx.x;
  const bool live = tile < a.tiles;
  const int v = live ? a.tile_v[tile] : 0, t = live ? a.tile_t[tile] : 0;
  int sum_v, sum_t;
  const int before_v = block_scan(v, waves_v, sum_v), before_t = block_scan(t, waves_t, sum_t);
  if (live) { a.tile_v[tile] = before_v; a.tile_t[tile] = before_t; }
  if (threadIdx.x == 0) { a.group_v[blockIdx.x] = sum_v; a.group_t[blockIdx.x] = sum_t; }
}

// at most 2^30 / (1024 * 256) = 4096 groups: 16 rounds of one workgroup; a round's sum stays below 2^31, the running totals
// are 64-bit (7 vertices and 12 triangles per point of a 2^30 lattice do not fit 32 bits)
__global__ void __launch_bounds__(kThreads) k_iso_scan_groups(RcIsoArgs a) {
  __shared__ int waves_v[4], waves_t[4];
  int64_t carry_v = 0, carry_t = 0;
  for (uint32_t g0 = 0; g0 < a.groups; g0 += kThreads) {
    const uint32_t g = g0 + threadIdx.x;
    const bool live = g < a.groups;
    const int v = live ? a.group_v[g] : 0, t = live ? a.group_t[g] : 0;
    int sum_v, sum_t;
    const int before_v = block_scan(v, waves_v, sum_v), before_t = block_scan(t, waves_t, sum_t);
    if (live) { a.group_off[2 * g] = carry_v + before_v; a.group_off[2 * g + 1] = carry_t + before_t; }
    carry_v += sum_v; carry_t += sum_t;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    a.counts[0] = carry_v; a.counts[1] = carry_t;
    a.state->emit = (carry_v <= a.v_capacity && carry_t <= a.t_capacity) ? 1 : 0;
  }
}

// d f / d (world position) at lattice point (ix, iy, iz) = p: central differences, one-sided at the border
__device__ __forceinline__ void lattice_gradient(const RcIsoArgs& a, const Lattice& G, uint32_t p, uint32_t ix, uint32_t iy,
                                                 uint32_t iz, float g[3]) {
  const uint32_t i[3] = {ix, iy, iz}, n[3] = {G.nx, G.ny, G.nz}, s[3] = {G.sx, G.sy, 1u};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint32_t up = i[c] + 1 < n[c] ? 1u : 0u, down = i[c] > 0 ? 1u : 0u;
    g[c] = (a.field[p + up * s[c]] - a.field[p - down * s[c]]) / ((float)(up + down) * a.lat.step[c]);
  }
}

__global__ void __launch_bounds__(kThreads) k_iso_vertices(RcIsoArgs a) {
  __shared__ int waves[4];
  if (!a.state->emit) return;
  const Lattice G(a.lat);
  const uint32_t tile = blockIdx.x, p0 = tile * (uint32_t)kRcIsoTile + threadIdx.x * (uint32_t)kItems;
  const uint32_t masks = reinterpret_cast<const uint32_t*>(a.mask)[p0 >> 2];
  int total;
  const int before = block_scan(__popc(masks), waves, total);
  if (masks == 0) return;
  int64_t v = a.group_off[2 * (tile / (uint32_t)kRcIsoGroup)] + a.tile_v[tile] + before;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    uint32_t mask = (masks >> (8 * j)) & 0xFFu;
    if (mask == 0) continue;
    const uint32_t p = p0 + (uint32_t)j;
    a.vbase[p] = (int32_t)v;
    uint32_t ix, iy, iz;
    G.split(p, ix, iy, iz);
    const float f0 = a.field[p];
    const float P0[3] = {axis_pos(a.lat, 0, ix), axis_pos(a.lat, 1, iy), axis_pos(a.lat, 2, iz)};
    float g0[3] = {0.0f, 0.0f, 0.0f};
    if (a.normals) lattice_gradient(a, G, p, ix, iy, iz, g0);
    for (; mask; mask &= mask - 1u, ++v) {
      const uint32_t e = (uint32_t)__ffs((int)mask) - 1u, d = (kDirPack >> (3u * e)) & 7u;
      const uint32_t jx = ix + (d & 1u), jy = iy + ((d >> 1) & 1u), jz = iz + (d >> 2), q = p + G.offset(d);
      const float f1 = a.field[q];
      const float t = fminf(fmaxf((a.iso - f0) / (f1 - f0), 0.0f), 1.0f);      // a NaN becomes 0
      const float P1[3] = {axis_pos(a.lat, 0, jx), axis_pos(a.lat, 1, jy), axis_pos(a.lat, 2, jz)};
#pragma unroll
      for (int c = 0; c < 3; ++c) a.vertices[3 * v + c] = P0[c] + t * (P1[c] - P0[c]);
      if (a.normals) {
        float g1[3], g[3];
        lattice_gradient(a, G, q, jx, jy, jz, g1);
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] = g0[c] + t * (g1[c] - g0[c]);
        const float len = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) a.normals[3 * v + c] = len > 0.0f ? -(g[c] / len) : 0.0f;
      }
    }
  }
}

// the triangles of tetrahedron K of the cell at p, from triangle index `out` on
template <int K> __device__ __forceinline__ void emit_tet(const RcIsoArgs& a, const Lattice& G, uint32_t p, uint32_t in, int64_t& out) {
  const uint32_t m = tet_mask<K>(in), nt = tet_triangles(m);
  for (uint32_t t = 0; t < nt; ++t, ++out) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t ref = kRcIso.vref[K][m][t][c], owner = p + G.offset(ref & 7u), e = ref >> 3;
      a.triangles[3 * out + c] = a.vbase[owner] + __popc((uint32_t)a.mask[owner] & ((1u << e) - 1u));
    }
  }
}

__global__ void __launch_bounds__(kThreads) k_iso_triangles(RcIsoArgs a) {
  __shared__ int waves[4];
  if (!a.state->emit) return;
  const Lattice G(a.lat);
  const uint32_t tile = blockIdx.x, p0 = tile * (uint32_t)kRcIsoTile + threadIdx.x * (uint32_t)kItems;
  const uint32_t counts = reinterpret_cast<const uint32_t*>(a.tcount)[p0 >> 2];
  int total;
  const int mine = (int)((counts & 0xFFu) + ((counts >> 8) & 0xFFu) + ((counts >> 16) & 0xFFu) + (counts >> 24));
  const int before = block_scan(mine, waves, total);
  if (counts == 0) return;
  int64_t out = a.group_off[2 * (tile / (uint32_t)kRcIsoGroup) + 1] + a.tile_t[tile] + before;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    if (((counts >> (8 * j)) & 0xFFu) == 0) continue;
    const uint32_t p = p0 + (uint32_t)j;
    uint32_t exists;
    const uint32_t in = cell_inside(a, G, p, exists);      // a cell with triangles has all eight corners
    emit_tet<0>(a, G, p, in, out); emit_tet<1>(a, G, p, in, out); emit_tet<2>(a, G, p, in, out);
    emit_tet<3>(a, G, p, in, out); emit_tet<4>(a, G, p, in, out); emit_tet<5>(a, G, p, in, out);
  }
}

inline dim3 blocks_for(int64_t n) { return dim3((unsigned)((n + kThreads - 1) / kThreads)); }

}  // namespace

void rc_launch_rows_to_soa(const float* rows, int64_t n, float* soa, hipStream_t stream) {
  if (n > 0) hipLaunchKernelGGL(k_rows_to_soa, blocks_for(n), dim3(kThreads), 0, stream, rows, n, soa);
}
void rc_launch_soa_to_rows(const float* soa, int64_t n, float* rows, hipStream_t stream) {
  if (n > 0) hipLaunchKernelGGL(k_soa_to_rows, blocks_for(n), dim3(kThreads), 0, stream, soa, n, rows);
}
void rc_launch_lattice_points(const RcLatticeArgs& a, int64_t first, int64_t n, float* soa, hipStream_t stream) {
  if (n > 0) hipLaunchKernelGGL(k_lattice_points, blocks_for(n), dim3(kThreads), 0, stream, a, first, n, soa);
}
void rc_launch_nan_to_num(float* x, int64_t n, hipStream_t stream) {
  if (n > 0) hipLaunchKernelGGL(k_nan_to_num, blocks_for(n), dim3(kThreads), 0, stream, x, n);
}

void rc_launch_isosurface(const RcIsoArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_iso_classify, dim3(a.tiles), dim3(kThreads), 0, stream, a);
  hipLaunchKernelGGL(k_iso_scan_tiles, dim3(a.groups), dim3(kThreads), 0, stream, a);
  hipLaunchKernelGGL(k_iso_scan_groups, dim3(1), dim3(kThreads), 0, stream, a);
  if (a.v_capacity == 0 && a.t_capacity == 0) return;      // nothing can be written: an empty surface has nothing, any other exceeds them
  hipLaunchKernelGGL(k_iso_vertices, dim3(a.tiles), dim3(kThreads), 0, stream, a);
  hipLaunchKernelGGL(k_iso_triangles, dim3(a.tiles), dim3(kThreads), 0, stream, a);
}
