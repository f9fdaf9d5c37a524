// Shared by the two forms of the fused cache kernel: rc_fused.hip (one wavefront per ray) and rc_fused2.hip (two
// wavefronts per ray, two workgroups per CU).  Same weight stream, same LDS step map, same arguments, and one copy of the
// per-ray phases both run: load_ray, carve_scratch, analytic_normal, store3 / store1, distance_mean,
// distance_percentiles.  resample, mean_of, density_of, level2_combine / level2_jacobian and export_samples are the
// one-wave kernel's; the two-wave kernel keeps copies of its own, for its speed (see its head).
#pragma once
#include "rc_dev_grid.h"
#include "rc_dev_mlp.h"
#include "rc_dev_sample.h"

namespace rcfused {
using namespace rcdev;

constexpr int kTileStride = 33 * 64;          // floats between the two point-tiles of levels 0/1
constexpr int kScratch = 7 * 68;              // per-ray step-function scratch (floats): the seven slices of Scratch
constexpr int kAppTmp = 33;                   // act steps [33, 49): appearance features parked during the density MLP
constexpr int kFusedDense = kRcFusedDenseLevels;               // grid levels [0, 3) of every grid are dense (16, 32, 64 cells a side), the rest hashed: fused_geometry_ok
constexpr int kJac = 49;                      // act steps [49, 97): d feature / d position of the level-2 density grid

// fragments of the fused weight stream: DensFrags, F_L0 .. F_SH, NF_FUSED, FusedDens and FusedShader are rc_pack_host.h's
// (host-only, so that hostcheck prints them); the one-wave kernel of a split build reads the output rows as tables
// (kRcFusedRows), every other kernel the fragment form
static_assert(kChunk == kRcChunkFrags, "rc_rows_at places the row tables by the ring's chunk");

#ifdef RC_STAMPS
#define RC_FSTAMP(i) do { __builtin_amdgcn_sched_barrier(0); __builtin_amdgcn_s_waitcnt(0); stamps[i] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define RC_FSTAMP(i) do { } while (0)
#endif

#ifdef RC_STAMPS
#define RC_FSTAMP_NOWAIT(i) do { __builtin_amdgcn_sched_barrier(0); stamps[i] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define RC_FSTAMP_NOWAIT(i) do { } while (0)
#endif
// what a kernel hands to a function that stamps: its parameter is named `stamps`, as the kernel's array
#ifdef RC_STAMPS
#define RC_FSTAMP_BUF stamps
#else
#define RC_FSTAMP_BUF nullptr
#endif
// ---- per-phase argument records of the one-wave kernel: what ONE phase of the ray's chain reads of the arguments, side by
// side and 64-byte aligned, so that the phase's scalars arrive in two or three wide s_loads that the kernel issues one
// phase ahead of their use (rc_fused.hip, head).  rc_launch_fused fills them; the two-wave kernel reads the same fields.
// a lookup: the tables, sizes and masks of the grid's levels, with the scalars the proposal level needs around it
struct alignas(64) RcLookupRec {
  const float* table[RC_MAX_GRID_LEVELS];   // proposal grids 0 / 1: the cell table of a dense level, the hash table of a hashed one;
                                            // level 2: the interleaved [density | appearance] tables (RcFusedLaunch::pair_table)
  int32_t size[RC_MAX_GRID_LEVELS];
  uint32_t mask[RC_MAX_GRID_LEVELS];
  float bbox, precondition, contract_radius, density_bias;
};
// a resampling
struct alignas(32) RcResampleRec { const float* jitter; USpec us; float anneal, padding; };
// the shader and the compositing tail
struct alignas(64) RcShadeRec {
  ShaderConsts sh; float bg, density_bias, contract_radius;
  const float* lights; const float* viewdirs;
  float pct[3];
};

struct RcFusedArgs {
  const float* origins; const float* directions; const float* near; const float* far;
  int64_t n;
  RcResampleRec rs[3];
  RcLookupRec look[3];
  RcShadeRec shade;
  // the grids as every other kernel takes them: the two-wave kernel's lookups (level kinds, cell records) read these
  RcGridDev grid[4];
  const float* pair_table[RC_MAX_GRID_LEVELS];
  const float* cell_table[2][RC_MAX_GRID_LEVELS];
  const float* wstream; const float* ide_coef;
  rc_outputs out;
  unsigned long long* stamps;
  int32_t prio_mode;        // rc_fused2.hip: wave priorities of the workgroup that arrived second on its CU (see the kernel)
  // FRONT variant (time-resolved cache): the proposal sampler only; what the launch-per-stage front end leaves in the
  // workspace for the stages behind it, in its layouts (np = n * 32 shaded samples)
  int32_t use_raydist; float raydist_p, raydist_premult, y_max;      // power-ladder distances (coord.py:223-260)
  float* f_tdist;          // [n][33]
  float* f_density;        // [np]
  float* f_means;          // SoA [3][np]
  float* f_normals_pred;   // SoA [3][np]
  float* f_normals_grad;   // SoA [3][np] (GRAD) or nullptr
  float* f_hbuf;           // [n][32 steps][64 lanes]: hidden feature in accumulator layout, one tile per ray
  float* f_app;            // feature-major [32][np]
};

// ---- the per-ray phases both kernels run: same arithmetic, same order

// the ray's record
struct Ray { float ox, oy, oz, dx, dy, dz, near, far, dnorm; };
__device__ __forceinline__ Ray load_ray(const RcFusedArgs& a, int64_t ray) {
  Ray r;
  r.ox = a.origins[3 * ray]; r.oy = a.origins[3 * ray + 1]; r.oz = a.origins[3 * ray + 2];
  r.dx = a.directions[3 * ray]; r.dy = a.directions[3 * ray + 1]; r.dz = a.directions[3 * ray + 2];
  r.near = a.near[ray]; r.far = a.far[ray];
  r.dnorm = sqrtf(r.dx * r.dx + r.dy * r.dy + r.dz * r.dz);
  return r;
}

// the kScratch floats of a ray: sdist of the level before (two, alternating), tdist, and the resampler's work arrays
struct Scratch { float* sd[2]; float *td, *cw, *c, *v, *out; };
__device__ __forceinline__ Scratch carve_scratch(float* scr) {
  return Scratch{{scr, scr + 68}, scr + 2 * 68, scr + 3 * 68, scr + 4 * 68, scr + 5 * 68, scr + 6 * 68};
}

// a resampling's record in registers (the one-wave kernel reads it one phase ahead, rc_fused.hip)
struct ResampleRegs { const float* jitter; USpec us; float anneal, padding; };
__device__ __forceinline__ ResampleRegs fetch_resample(const RcResampleRec& q) { return ResampleRegs{q.jitter, q.us, q.anneal, q.padding}; }
#define RC_RESAMPLE_PINS(rs) "s"(rs.jitter), "s"(rs.us.start), "s"(rs.us.stop), "s"(rs.us.max_jitter), "s"(rs.anneal), "s"(rs.padding)

// resample S intervals from (prev sdist in s_prev [P+1], logit per bin): sdist -> s.out, tdist -> s.td
// (the ray index by reference, as the kernels' lambdas had it: by value the EXPORT instantiation without GRAD gets four
// more s_waitcnt in its level-2 resampling, profiles/r11_fused_shared_phases_ab.txt)
template <bool FRONT>
__device__ __forceinline__ void resample(const RcFusedArgs& a, const ResampleRegs& rs, const Ray& r, const int64_t& ray, const Scratch& s, int lane,
                                         int P, int S, float logit, const float* s_prev) {
  const bool hasj = rs.jitter != nullptr;
  const float jit = hasj ? rs.jitter[ray] : 0.0f;
#if defined(RC_ABL) && RC_ABL == 14
  for (int e2 = lane; e2 <= S; e2 += 64) s.out[e2] = (float)e2 / (float)S + 1e-9f * logit;
  lds_sync<false>();
#else
  sample_intervals_wave<false>(logit, P, S, rs.us, hasj, jit, s_prev, s.cw, s.c, s.v, s.out, lane);
#endif
  if constexpr (FRONT) {
    if (a.use_raydist) {      // TransientNeRFModel samples its primary rays in power-ladder distance (models.py:122, 183-191)
      const float s_near = power_ladder(r.near, a.raydist_p, a.raydist_premult), s_far = power_ladder(r.far, a.raydist_p, a.raydist_premult);
      for (int e2 = lane; e2 <= S; e2 += 64)
        s.td[e2] = inv_power_ladder(s.out[e2] * s_far + (1.0f - s.out[e2]) * s_near, a.raydist_p, a.raydist_premult, a.y_max);
      lds_sync<false>();
      return;
    }
  }
  for (int e2 = lane; e2 <= S; e2 += 64) s.td[e2] = s.out[e2] * r.far + (1.0f - s.out[e2]) * r.near;   // coord.py:259-260
  lds_sync<false>();
}

// fence posts and sample mean of interval `idx`
__device__ __forceinline__ void mean_of(const Ray& r, const float* s_td, int idx, float& mx, float& my, float& mz, float& t0, float& t1) {
  t0 = s_td[idx]; t1 = s_td[idx + 1];
  const float sm = t0 + t1, d = t1 - t0;
  const float ratio = (d * d) / fmaxf(RC_EPS * RC_EPS, 3.0f * (sm * sm) + d * d);
  const float tm = sm * (0.5f + ratio);
  mx = r.dx * tm + r.ox; my = r.dy * tm + r.oy; mz = r.dz * tm + r.oz;
}

__device__ __forceinline__ float density_of(float density_bias, float raw, float cx, float cy, float cz, float bbox) {
  const bool inside = (cx > -bbox) & (cx < bbox) & (cy > -bbox) & (cy < bbox) & (cz > -bbox) & (cz < bbox);
  const float d = rc_safe_exp(raw + density_bias);
  return inside ? d : 0.0f;
}

// (GRAD) d feature / d contracted coordinate of the level-2 density grid, 96 values per point, goes to LDS: element e of
// point j at step kJac + e / 2, lane j + 32 (e & 1); written and read back by the lane (j, 0) that owns the point
__device__ __forceinline__ float& jac_at(float* act_ray, int j, int e) { return act_ray[(kJac + (e >> 1)) * 64 + j + 32 * (e & 1)]; }

// level-2 combine of a grid level from its fetched corners: the four preconditioned features, and (GRAD) the raw
// derivatives level2_jacobian takes
template <bool GRAD>
__device__ __forceinline__ void level2_combine(float precondition, const Corners<4>& C, float (&f)[4], float (&jd)[GRAD ? 12 : 1]) {
  float v[4];
  grid_combine<4, GRAD>(C, v, jd);
#pragma unroll
  for (int c = 0; c < 4; ++c) f[c] = v[c] * precondition;
}
// half-wave 0 (the density grid) parks the three Jacobian rows of grid level l (a constant where it is called), a dense
// level's axes swapped; behind the caller's use of the features, as both kernels have it
__device__ __forceinline__ void level2_jacobian(float precondition, int size, float bbox, int l, const float (&jd)[12], float* act_ray, int j, int h) {
  const bool dense = l < kFusedDense;       // compile-time, as in the fetch
  const float s = precondition * (float)size / (2.0f * bbox);
  if (h == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      jac_at(act_ray, j, 0 * 32 + 4 * l + c) = (dense ? jd[2 * 4 + c] : jd[0 * 4 + c]) * s;
      jac_at(act_ray, j, 1 * 32 + 4 * l + c) = jd[1 * 4 + c] * s;
      jac_at(act_ray, j, 2 * 32 + 4 * l + c) = (dense ? jd[0 * 4 + c] : jd[2 * 4 + c]) * s;
    }
  }
}

// analytic normal of point j from gf = d raw / d feature (acc_feat(0, r, h) sits on lane (j, h)): each half-wave contracts
// ITS 16 features with the Jacobian rows parked in LDS, the two partial sums are added last (the order k_density_mlp
// uses); then the derivative of the contraction at z = mean / radius
__device__ __forceinline__ void analytic_normal(const f32x16& gf, float* act_ray, int j, int h, float zx, float zy, float zz, float radius,
                                                float& ngx, float& ngy, float& ngz) {
  float gp[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = (r & 3) + 8 * (r >> 2) + 4 * h;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) gp[ax] += gf[r] * jac_at(act_ray, j, ax * 32 + i);
  }
  float gw[3];
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    const float oth = __shfl_xor(gp[ax], 32, 64);
    gw[ax] = h == 0 ? gp[ax] + oth : oth + gp[ax];        // half 0's partial first on both halves
  }
  const float msq = zx * zx + zy * zy + zz * zz;
  float gzx = gw[0], gzy = gw[1], gzz = gw[2];
  if (msq > 1.0f) {
    const float rt = sqrtf(msq);
    const float s = (2.0f * rt - 1.0f) / msq;
    const float ds = (1.0f - rt) / (msq * msq);
    const float gz_dot = gw[0] * zx + gw[1] * zy + gw[2] * zz;
    gzx = s * gw[0] + 2.0f * ds * gz_dot * zx;
    gzy = s * gw[1] + 2.0f * ds * gz_dot * zy;
    gzz = s * gw[2] + 2.0f * ds * gz_dot * zz;
  }
  ngx = rc_div(gzx, radius); ngy = rc_div(gzy, radius); ngz = rc_div(gzz, radius);
  neg_normalize(ngx, ngy, ngz);
}

// the last level's per-sample results of a live ray into the workspace, in the layouts of the launch-per-stage plan:
// fence posts, and from the lanes (j, 0) density, sample mean, predicted normal and (NG, if asked for) analytic normal
template <bool NG>
__device__ __forceinline__ void export_samples(const RcFusedArgs& a, int64_t ray, int lane, const float* s_td, float density, float mx, float my,
                                               float mz, float npx, float npy, float npz, float ngx, float ngy, float ngz) {
  const int j = lane & 31, h = lane >> 5;
  const int64_t np = a.n * 32, p = ray * 32 + j;
  for (int e2 = lane; e2 <= 32; e2 += 64) a.f_tdist[ray * 33 + e2] = s_td[e2];
  if (h == 0) {
    a.f_density[p] = density;
    a.f_means[p] = mx; a.f_means[np + p] = my; a.f_means[2 * np + p] = mz;
    a.f_normals_pred[p] = npx; a.f_normals_pred[np + p] = npy; a.f_normals_pred[2 * np + p] = npz;
    if constexpr (NG) {
      if (a.f_normals_grad) { a.f_normals_grad[p] = ngx; a.f_normals_grad[np + p] = ngy; a.f_normals_grad[2 * np + p] = ngz; }
    }
  }
}

// per-ray outputs: `on` = lane 0 of a live ray
__device__ __forceinline__ void store3(float* dst, bool on, int64_t ray, float x, float y, float z) {
  if (on && dst) { dst[3 * ray] = x; dst[3 * ray + 1] = y; dst[3 * ray + 2] = z; }
}
__device__ __forceinline__ void store1(float* dst, bool on, int64_t ray, float x) { if (on && dst) dst[ray] = x; }

// distance_mean of the weighted log-distance sum, between the first and the last fence post
__device__ __forceinline__ float distance_mean(float logt, float accw, const float* s_td) {
  const float e = logt / fmaxf(RC_EPS, accw);
  float dm = expf(e);
  if (dm != dm) dm = 0.0f;                     // nan_to_num(x, copy=inf): nan -> 0.0 (rc_sample.hip, k_composite)
  dm = fminf(dm, RC_FMAX);
  return fminf(fmaxf(dm, s_td[0]), s_td[32]);
}

// the three distance percentiles: inclusive scan of the normalised weights into s_cw, lanes 0-2 interpolate one each
// (pct_of(lane): the percentile of lane 0, 1, 2)
template <class PCT>
__device__ __forceinline__ void distance_percentiles(const PCT& pct_of, int64_t ray, bool ray_ok, int lane, float wnf, float accw,
                                                     const float* s_td, float* s_cw, float* p5, float* median, float* p95) {
  const float wn = wnf / fmaxf(RC_EPS, accw);
  const float incl = wave_scan_incl(wn, lane);
  if (lane == 0) s_cw[0] = 0.0f;
  if (lane < 31) s_cw[lane + 1] = fminf(1.0f, incl);
  if (lane == 0) s_cw[32] = 1.0f;
  lds_sync<false>();
  if (lane < 3 && ray_ok) {
    const float ps = pct_of(lane) / 100.0f;
    const float v = interp1(ps, s_cw, s_td, 33);
    float* const dst = lane == 0 ? p5 : (lane == 1 ? median : p95);
    if (dst) dst[ray] = v;
  }
}


}  // namespace rcfused

// rc_fused2.hip: the plain cache pass with two wavefronts per ray (GRAD: analytic normals requested)
void rc_launch_fused_team(const rcfused::RcFusedArgs& a, bool grad, hipStream_t stream);
