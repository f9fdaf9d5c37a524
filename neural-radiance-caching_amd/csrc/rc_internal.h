// Internal declarations shared by the gfx950 kernels and the C-ABI host (rc_api.hip).
#pragma once
#include <atomic>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rc_abi.h"

#define RC_WAVE 64
#define RC_MAX_GRID_LEVELS 8

// x / d.  Every BASELINE config divides by powers of two here (contraction radius 2, bounding box [-1, 1] -> extent 2):
// the product with the exact reciprocal 2^-e is then the same correctly rounded value as the quotient, at one
// instruction instead of the ~11 of an IEEE fp32 division.  `d` is wave-uniform (a kernel argument): one branch.
__device__ __forceinline__ float rc_div(float x, float d) {
  const uint32_t b = __float_as_uint(d);
  const bool pow2 = (b & 0x807FFFFFu) == 0u && b >= 0x01000000u && b <= 0x7E000000u;      // +2^e, e in [-125, 125]
  return pow2 ? x * __uint_as_float(0x7F000000u - b) : x / d;
}

// float32 constants the reference hard-codes (internal/math.py:24-26).
#define RC_TINY 1.17549435e-38f
#define RC_FMAX 3.40282347e+38f
#define RC_EPS 1.1920929e-07f

// math.safe_exp (internal/math.py:186-192): exp(jnp.clip(x, finfo.min, 70)).  jnp.clip = minimum(maximum(x, lo), hi) and
// both PROPAGATE a NaN (v_max_f32 / v_min_f32 return the other operand): selects on ordered compares keep the NaN, so a
// NaN raw density stays NaN as in the reference (oracle/JAX_CALLS.md, row `jnp.clip`).
__device__ __forceinline__ float rc_safe_exp(float x) {
  return expf(x > 70.0f ? 70.0f : (x < -RC_FMAX ? -RC_FMAX : x));
}

// v_permlane32_swap: lanes 32-63 of the first operand <-> lanes 0-31 of the second; returns {first, second} afterwards
__device__ __forceinline__ void swap_halves(float& first, float& second) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(first), __float_as_uint(second), false, false);
  first = __uint_as_float(r[0]); second = __uint_as_float(r[1]);
}

// ---------------------------------------------------------------------------------------------
// Hash grid
// ---------------------------------------------------------------------------------------------
struct RcGridLevel {
  const float* table;   // dense: [N,N,N,F] indexed [x,y,z]; hash: [T,F]
  int32_t size;         // N
  int32_t dense;        // 1: dense grid, 0: hash table
  uint32_t entries;     // N^3 or T
  uint32_t mask;        // T-1 if T is a power of two, else 0
  const float* cell;    // dense F = 1 levels of the proposal grids: cell table ((N+3)^3 cells x 8 corners, zero padding
                        // baked in; built with the fused kernel's tables) or nullptr
  const float* rec;     // hashed levels [kRcFusedDenseLevels, + kRcRecLevels) of the F = 1 proposal grids, [.., + kRcRec4Levels)
                        // of the F = 4 density grid: cell records ((N+1)^3 cell origins x the 8 hashed corner entries,
                        // rc_launch_build_hrec) or nullptr
};

struct RcGridDev {
  RcGridLevel lvl[RC_MAX_GRID_LEVELS];
  int32_t num_levels;
  int32_t num_features;
  float bbox;
  float precondition;
};

// points: world-space [n,3] (AoS) or SoA [3][n] (soa_in != 0).  Output feature-major [L*F][ldo]
// (feature_major != 0) or row-major [n][L*F].  contract_radius <= 0 disables the contraction.
// interleaved [grid A | grid B] tables of two F = 4 grids with the same level geometry, one per level (rc_api.hip
// build_fused_tables)
struct RcPairTables { const float* t[RC_MAX_GRID_LEVELS]; };
void rc_launch_hashgrid_pair(const RcGridDev& g, const RcPairTables& pt, const float* points_soa, const int32_t* src,
                             int64_t n_src, int64_t n, float* out_a, float* out_b, int64_t ldo, float contract_radius,
                             hipStream_t stream);
// two F = 4 grids looked up at the same row-major [n,3] points in one launch (row-major [n, L*4] outputs)
void rc_launch_hashgrid_two(const RcGridDev& ga, const RcGridDev& gb, const float* points, int64_t n, float* out_a, float* out_b,
                            float contract_radius, hipStream_t stream);
void rc_launch_hashgrid(const RcGridDev& g, const float* points, int soa_in, int64_t n, float* out,
                        int feature_major, int64_t ldo, float contract_radius, float* jac_out,
                        hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// Sampling / compositing
// ---------------------------------------------------------------------------------------------
struct RcSampleArgs {
  // ray batch
  const float* origins; const float* directions; const float* viewdirs;
  const float* near; const float* far; const float* normals;
  int64_t n_rays;
  // previous level (P bins); level 0: prev_sdist == nullptr (sdist=[0,1], w=[1])
  const float* prev_sdist;    // [n, P+1]
  const float* prev_tdist;    // [n, P+1]
  const float* prev_density;  // [n*P]
  int32_t P;
  // outputs for the previous level
  float* prev_weights;        // [n*P] or nullptr
  // this level
  int32_t S;
  const float* jitter;        // [n] or nullptr
  float* sdist;               // [n, S+1]
  float* tdist;               // [n, S+1]
  float* means;               // SoA [3][n*S]
  // constants
  float anneal, padding;
  int32_t secondary;          // near replacement from the surface normal + far clamp (secondary rays)
  int32_t use_raydist;        // sample in power-ladder distance (Model.get_bg_and_raydist, models.py:183-191)
  float raydist_p, raydist_premult, eps_dot_min, far_clamp;
  // use_raydist with ONE (near, far) for the whole batch (the material stage's secondary rays): power_ladder(near),
  // power_ladder(far) computed once on the device (rc_launch_ladder_bounds) instead of by every wave; nullptr otherwise
  const float* s_bounds;
};
void rc_launch_sample(const RcSampleArgs& a, hipStream_t stream);

// Stand-alone stepfun.sample_intervals (parity tests): t [n,P+1], logits [n,P] -> out [n,S+1].
void rc_launch_sample_intervals(const float* t, const float* logits, int64_t n, int P, int S,
                                const float* jitter, float* out, hipStream_t stream);

struct RcCompositeArgs {
  const float* directions; const float* origins; const float* lights;
  int64_t n_rays;
  int32_t S;                  // samples of the last level
  const float* tdist;         // [n, S+1]
  const float* density;       // [n*S]
  const float* means;         // SoA [3][n*S]
  const float* normals_pred;  // SoA [3][n*S]
  const float* normals_grad;  // SoA [3][n*S] or nullptr
  const float* shade;         // SoA [RC_SHADE_CH][n*Sf] per shaded sample
  int32_t Sf;                 // shaded samples per ray: S (no resampling) or 1
  const int32_t* inds;        // [n] selected sample when Sf == 1
  const float* filt_weight;   // [n] importance weight w/(n*p+1e-8) when Sf == 1
  float* weights;             // [n*S] out
  float bg;
  float pct[3];
  rc_outputs out;
};
void rc_launch_composite(const RcCompositeArgs& a, hipStream_t stream);

// Categorical resampling of the last level (models.py:193-292), num_resample == 1.
struct RcResampleArgs {
  int64_t n_rays; int32_t S;
  const float* tdist; const float* density; const float* directions;
  const float* gumbel;        // [n,S] or nullptr (then inds_in must be given)
  const int32_t* inds_in;     // [n] or nullptr
  int32_t* inds_out;          // [n]
  float* filt_weight;         // [n]
  float* weights;             // [n*S] out (weights_no_filter)
  float* acc_out;             // [n] or nullptr: sum of the weights, added as k_composite adds it (rc_launch_composite_pick)
  int32_t* src_out;           // [n] or nullptr: flat index ray * S + pick of the picked sample (per-pick lookups read through it)
  // material stage: position and predicted normal of the picked sample, gathered here (all four or none)
  const float* means;         // SoA [3][n*S]
  const float* normals;       // SoA [3][n*S]
  float* pts_out;             // [n,3]
  float* nrm_out;             // [n,3]
};
void rc_launch_resample(const RcResampleArgs& a, hipStream_t stream);
// k_composite for the case "one resampled sample per ray, only rgb and acc wanted" (the batched secondary trace): the
// weights and their sum are k_resample's, the only non-zero filtered weight sits on the pick -- one thread per ray.
// shade_rgb: the three colour channels of the shader's output, [3][n].  Same values, bit for bit.
void rc_launch_composite_pick(int64_t n, const float* shade_rgb, const float* filt_weight, const float* acc, float bg,
                              float* out_rgb, float* out_acc, hipStream_t stream);
// out[0] = power_ladder(near'), out[1] = power_ladder(far') with near' / far' as sample_level_ray derives them from
// (near, far) for a secondary ray without a surface normal
void rc_launch_ladder_bounds(float near, float far, float far_clamp, float p, float premult, float* out, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// MFMA MLP kernels
// ---------------------------------------------------------------------------------------------
// Per-sample shader outputs (SoA channel-major).
enum { RC_SH_RGB = 0, RC_SH_AD = 3, RC_SH_ID = 6, RC_SH_IS = 9, RC_SH_TINT = 12, RC_SHADE_CH = 15 };

struct RcDensityMlpArgs {
  const float* feat;          // feature-major [K][ld]
  int64_t n; int64_t ld;
  int32_t K;                  // 6, 7 or 32
  const float* wstream;       // packed MFMA fragment stream [d0 | d1 | out]
  const float* means;         // SoA [3][n] (validity mask); with `src`: SoA [3][n_src], point p reads column src[p]
  const int32_t* src; int64_t n_src;
  float density_bias, contract_radius, bbox;
  int32_t last;               // 1: also write hidden feature + predicted normals
  float* density;             // [n]
  float* hbuf;                // [n/32][32 steps][64] hidden feature in accumulator layout
  float* normals_pred;        // SoA [3][n]
  const float* jac;           // [3][K][ld] d feature / d contracted coordinate (k_hashgrid_fwd<F, true>) or nullptr
  float* normals_grad;        // SoA [3][n] analytic normals (needs jac; the stream must carry the backward fragments)
};
void rc_launch_density_mlp(const RcDensityMlpArgs& a, hipStream_t stream);

// One proposal level as one launch (rc_level.hip): grid lookup + density MLP, density only.
struct RcLevelArgs {
  const RcGridDev* grid;
  const float* means;         // SoA [3][n]
  int64_t n;
  const float* wstream;       // the level's "dens_<l>" fragment stream
  float density_bias, contract_radius;
  float* density;             // [n]
  int cu_reserve = 0;         // CUs the launch leaves to a kernel released beside it (k_level_ray only)
};
bool rc_level_supported(const RcGridDev& g);
void rc_launch_level(const RcLevelArgs& a, hipStream_t stream);
// the level's sampling (rc_launch_sample) and the level itself as ONE launch, one ray per wave
bool rc_level_ray_supported(const RcGridDev& g, int S);
void rc_launch_level_ray(const RcLevelArgs& a, const RcSampleArgs& sa, hipStream_t stream);

struct RcShaderArgs {
  int64_t n;                  // shaded points
  int64_t n_src;              // points of the last level (stride of the SoA inputs)
  const int32_t* src;         // [n] source point index or nullptr (identity)
  int32_t samples_per_ray;    // shaded samples per ray (ray = point / samples_per_ray)
  const float* hbuf;          // hidden density feature, accumulator layout, indexed by source point
  const float* app;           // appearance features, feature-major [32][n] (already gathered per shaded point)
  const float* normals_pred;  // SoA [3][n_src]
  const float* viewdirs;      // [n_rays,3]
  const float* wstream;       // packed MFMA fragment stream [heads | s0 | i0 | i1 | io | s1 | s2 | sb | so]
  const float* ide_coef;      // IDE polynomial table (device)
  float roughness_bias, irradiance_bias, ambient_bias, rgb_max, slf_ambient_bias;
  float* shade;               // SoA [RC_SHADE_CH][n]
  void* debug;                // diagnostic builds (-DRC_STAMPS): per-tile cycle stamps
};
void rc_launch_shader(const RcShaderArgs& a, hipStream_t stream);

// Model-level EnvMap MLP on ray directions (secondary-ray background).
struct RcEnvMapArgs {
  int64_t n; const float* viewdirs;   // [n,3]
  const float* wstream;               // packed fragments [e0 | e1 | e2 | eb(x) | eb(inputs) | out]
  float rgb_bias; float* env_rgb;     // [n,3]
};
void rc_launch_envmap(const RcEnvMapArgs& a, hipStream_t stream);

// IDE table layout (built on the host, see rc_api.hip): for deg_view 5 there are 36 (l,m)
// terms; term i has polynomial coefficients in z of degree <= 16 and an xy power m.
#include "rc_pack_host.h"      // RC_IDE_TERMS, RC_IDE_ZPOW, RcIdeTable, rc_cell_corner (host-only header)
#include "rc_ide_coef.h"       // kRcIdeCoef: the table's coefficients as compile-time constants of the kernels

// ---------------------------------------------------------------------------------------------
// Material stage (rc_material.hip)
// ---------------------------------------------------------------------------------------------
enum { RC_MAT_CH = 5 };   // per point: albedo rgb, roughness, metalness
enum { RC_VMF_CH = 5 };   // per lobe: normalised mean xyz, kappa, softmax weight
enum { RC_SMP_CH = 5 };   // per secondary sample: local light dir xyz, pdf, MIS weight

struct RcMatHeadArgs {
  int64_t n; const float* feat;        // row-major [n,32] material-grid features
  const float* w0; const float* b0;    // Flax kernel [32,128], bias
  const float* w1; const float* b1;    // [128,10]
  float min_roughness; float* mat;     // [n, RC_MAT_CH]
};
void rc_launch_material_head(const RcMatHeadArgs& a, hipStream_t st);
void rc_launch_material_composite_all(int64_t n, int S, const float* weights, const float* mat, float* out_albedo,
                                      float* out_rough, float* out_metal, float* out_f0, float f0, hipStream_t st);

struct RcLightHeadArgs {
  int64_t n; const float* feat;        // [n,32] light-grid features
  const float* w0; const float* b0; const float* w1; const float* b1; const float* w2; const float* b2;
  const float* pts; const float* noise;   // [n,3], [n,128,3]
  float vmf_scale; float* vmf;         // [n,128,RC_VMF_CH]
  float* vmf_logit;                    // [n,128]: the lobe logits as the softmax sees them (the categorical lobe draw takes these)
};
void rc_launch_light_head(const RcLightHeadArgs& a, hipStream_t st);
void rc_launch_shading_heads(const RcMatHeadArgs& m, const RcLightHeadArgs& l, hipStream_t st);     // both in one launch

struct RcBrdfSampleArgs {
  int64_t n; int32_t Ks, Kd, Kc;
  const float* pts; const float* nrm; const float* viewdirs; const float* lights; const float* mat; const float* vmf;
  const float* spec_u1; const float* spec_u2; const float* cos_u1; const float* cos_u2;
  const int32_t* vmf_lobe; const float* vmf_v; const float* vmf_tmp;
  const float* vmf_lobe_gumbel;   // [n,128] or nullptr: lobe = argmax(logit + gumbel) when vmf_lobe is nullptr
  const float* vmf_logit;         // [n,128] lobe logits of the light head (read only for that draw)
  float normal_eps, near, far;
  float* sec_origins; float* sec_dirs; float* sec_near; float* sec_far; float* sec_lights;   // [n*(Ks+Kd), .]
  float* samples;       // [n, Ks+Kd, RC_SMP_CH]
  float* local_view;    // [n,3]
};
void rc_launch_brdf_sample(const RcBrdfSampleArgs& a, hipStream_t st);

struct RcMatIntegrateArgs {
  int64_t n; int32_t Ks, Kd, S;
  const float* mat; const float* samples; const float* local_view;
  const float* sec_rgb; const float* sec_acc; const float* sec_env;
  const float* weights;       // [n,S] unfiltered weights of the primary rays
  const float* filt_weight;   // [n]
  const float* pts; const float* nrm; const float* origins; const float* lights;
  float f0, rgb_max, bg;
  rc_mat_outputs out;
};
void rc_launch_material_integrate(const RcMatIntegrateArgs& a, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// Fused cache forward (rc_fused.hip): one launch per batch of primary rays
// ---------------------------------------------------------------------------------------------
struct RcFusedLaunch {
  rc_rays rays; int64_t n;
  const float* jitter[3]; int32_t num_samples[3];
  const RcGridDev* grid[4];            // proposal 0, 1, 2 + appearance
  const float* pair_table[RC_MAX_GRID_LEVELS];   // level-2 density and appearance tables interleaved entry by entry
                                                 // (dense levels: cell tables of interleaved pairs)
  const float* cell_table[2][RC_MAX_GRID_LEVELS]; // dense levels of proposal grids 0 / 1 as cell tables (else NULL)
  const float* wstream;                // [density MLP 0 | 1 | 2 (+ backward) | shader], see rc_fused_stream_offsets
  const float* ide_coef;
  float anneal, padding, density_bias, contract_radius, bg; float pct[3];
  float roughness_bias, irradiance_bias, ambient_bias, rgb_max, slf_ambient_bias;
  rc_outputs out;
  // front end only (time-resolved cache): stop behind the last proposal level, results into the workspace buffers of
  // the launch-per-stage plan (wstream then ends at the shader's offset)
  int32_t front, want_grad;
  int32_t export_samples;              // full kernel + f_tdist / f_density / f_means / f_normals_pred of the last level
  int32_t team;                        // two wavefronts per ray, two workgroups per CU (rc_fused2.hip); plain pass only
  int32_t prio_mode;                   // (team) priority scheme of the younger workgroup of a CU
  int32_t use_raydist; float raydist_p, raydist_premult;
  float* f_tdist; float* f_density; float* f_means; float* f_normals_pred; float* f_normals_grad; float* f_hbuf; float* f_app;
};
// the fused kernels are compiled for this level layout of every grid: levels [0, kRcFusedDenseLevels) dense (16, 32, 64
// cells a side against 2^19 entries), the others hashed
constexpr int kRcFusedDenseLevels = 3;
// ... and the first kRcRecLevels hashed levels of the F = 1 grids are read through cell RECORDS: one 32-byte record per
// cell origin with the 8 hashed corner values side by side, so a lookup is ONE sector instead of four (rc_dev_grid.h
// kLevelHRec).  69 MB per grid for the 128^3 level, 543 MB for 256^3, 4.3 GB for 512^3.  Measured (same box, builds with
// 0 | 1 | 2 record levels, profiles/r04_ab_cell_records.txt): fused kernel 124.8 | 124.3 | 123.5 us per 1024 rays, 1720 |
// 1707 | 1716 us per 16 384, material stage 1.437 | 1.414 | 1.422 ms -- one level is worth 0.5-1.7 %, the second nothing:
// four x-pair sectors out of a 2 MiB table (L2) cost what one sector out of a table behind the L2 costs
// (profiles/r04_gather_cell_records.txt: 65 G lookups/s against 54-59).  One level it is.
#ifndef RC_REC_LEVELS
#define RC_REC_LEVELS 1
#endif
constexpr int kRcRecLevels = RC_REC_LEVELS;
// The same for the F = 4 density grid of the last level, which the level kernels read on the lean pass (density of all
// 32 samples of a secondary ray before one is picked): its hashed tables are 8 MiB each, 40 MiB together -- every sector
// is a fabric read there (k_level_ray<4, 8, 32>: 22 M L2 misses per 32 768-ray trace, the memory system's random-sector
// rate), and a 128-byte record (8 corners x 16 bytes = one cache line) replaces ~4.4 sectors by 2.
// 275 MB for the 128^3 level, 2.2 GB for 256^3.
#ifndef RC_REC4_LEVELS
#define RC_REC4_LEVELS 2
#endif
constexpr int kRcRec4Levels = RC_REC4_LEVELS;
// dst[(N+1)^3][8]: record (qx, qy, qz) in [0, N]^3 = cell origin (qx - 1, qy - 1, qz - 1), corner c = 4 b0 + 2 b1 + b2 at
// origin + (b0, b1, b2) through the level's hash (power-of-two table)
void rc_launch_build_hrec(const float* table, int N, uint32_t mask, int F, float* dst, hipStream_t stream);
int rc_fused_stream_offsets(int* l0, int* l1, int* l2, int* sh);   // returns the total fragment count
void rc_launch_fused(const RcFusedLaunch& L, hipStream_t stream);
// dst[cell][corner][dst_stride floats, written F at dst_off]: the 8 corners of every cell of the zero-padded dense
// level `src` [N^3][F] (cells (N + 3)^3, corner order b0 b1 b2 as in grid_combine)
void rc_launch_build_cells(const float* src, int N, int F, float* dst, int dst_stride, int dst_off, hipStream_t stream);


// ---------------------------------------------------------------------------------------------
// Time-resolved cache (rc_transient.hip)
// ---------------------------------------------------------------------------------------------
// per-sample channels written by k_transient_shader ([RC_TS_COUNT][n], channel-major)
enum { RC_TS_DD = 0, RC_TS_DS = 3, RC_TS_ALBEDO = 6, RC_TS_TIB = 9, RC_TS_ROUGH = 12, RC_TS_NDOTL = 13, RC_TS_IRRAD = 14,
       RC_TS_OCC = 15, RC_TS_LDIST = 16, RC_TS_RDIST = 17, RC_TS_CAMDIST = 18, RC_TS_COUNT = 19 };
constexpr int kRcTdBins = 700, kRcTdHist = 3 * kRcTdBins;      // histogram entries of a ray: entry = 3 bin + channel

// What the integrator's kernels (k_transient_bins, k_transient_slice, k_transient_bins_bwd) read alike: the shader's
// per-sample buffers and the integrator's settings (rc_dev_transient.h; filled by transient_in, rc_transient_host.inc).
// The kernels' argument structs take it, and RcTransTaps, as a base: the fields keep their names in every struct.
struct RcTransIn {
  int64_t n_rays;
  const float* slf_feat; const float* irr_feat; const float* tshade; const float* weights;   // weights [n_rays][32]
  float exposure, shift, max_dists, irradiance_bias, slf_rgb_bias, indirect_scale, rgb_max, light_near;
  int32_t bin_zero_threshold_light, light_zero;
};
// the temporal filter of the direct part
struct RcTransTaps {
  int32_t n_taps;
  const float* taps;                       // device, n_taps entries
};

struct RcTransShaderArgs {
  int64_t n; int32_t samples_per_ray;
  const float* hbuf; const float* app; const float* means; const float* normals;   // means / normals: SoA [3][n]
  const float* origins; const float* viewdirs; const float* lights; const float* cam_origins;   // per ray [.,3]
  const float* occ;                        // optional: acc of the shadow ray of each sample [n] (nerf.py:1300-1340)
  float occ_threshold;
  const float* wstream; const float* ide_coef;
  float roughness_bias, albedo_bias, brdf_bias, rgb_max, contract_radius;
  float light_power, light_near; int32_t use_falloff, light_zero;
  float* irr_feat;                         // [tiles][32 steps][64 lanes]
  float* slf_feat;                         // [tiles][64 steps][64 lanes]
  float* tshade;                           // [RC_TS_COUNT][n]
};

struct RcTransBinsArgs : RcTransIn, RcTransTaps {
  unsigned long long* stamps;              // diagnostic builds (-DRC_STAMPS) only
  const float* wstream;                    // per column tile: 65 SLF output fragments | 33 transient_indirect fragments
  float* out_rgb; float* out_direct; float* out_indirect;               // [n_rays][700][3]
  float* out_ti_diffuse; float* out_ti_specular;                         // unshifted composites [n_rays][700][3]
  float* out_direct_rgb; float* out_indirect_rgb; float* out_integrated_rgb;
  float* out_diffuse_rgb; float* out_specular_rgb; float* out_albedo_rgb; float* out_occ; float* out_indirect_occ;
  float* out_irradiance_rgb; float* out_light_radiance_rgb; float* out_n_dot_l_rgb; float* out_direct_diffuse_rgb;
  float* out_direct_specular_rgb; float* out_indirect_diffuse_rgb; float* out_indirect_specular_rgb; float* out_direct_rgb_viz;
};
struct RcShadowRayArgs {
  int64_t n; int32_t samples_per_ray;      // n = shaded samples
  const float* means; const float* normals;            // SoA [3][n]
  const float* lights;                                 // per primary ray [.,3]
  float normal_eps, shadow_near, shadow_far, light_near;
  float* origins; float* dirs; float* near; float* far; float* out_normals; float* out_lights;   // AoS [n,3] / [n]
};
void rc_launch_shadow_rays(const RcShadowRayArgs& a, hipStream_t stream);
int rc_transient_shader_frags();
int rc_transient_bins_frags();
void rc_launch_transient_shader(const RcTransShaderArgs& a, hipStream_t stream);
void rc_launch_transient_bins(const RcTransBinsArgs& a, hipStream_t stream);

// Time slices of the histograms without the histograms (rc_transient_slice.hip): launched in place of
// k_transient_bins.  The two per-bin heads as plain columns: column f = 3 bin + channel of a head is kRcSliceStride*
// consecutive floats, value j = 2 step + half of the activation order k_transient_shader stores (the steps_acc tables),
// then the bias.
constexpr int kRcSliceMax = RC_TSLICE_MAX;
constexpr int kRcSliceStrideSlf = 132;     // 128 rows + bias, padded to whole float4
constexpr int kRcSliceStrideIrr = 68;      // 64 rows + bias, padded
struct RcTransSliceArgs : RcTransIn, RcTransTaps {
  const float* w_slf; const float* w_irr;  // [2100][kRcSliceStrideSlf], [2100][kRcSliceStrideIrr]
  int32_t count;                           // 1 .. kRcSliceMax
  float t[kRcSliceMax];                    // fractional bin index, 0 <= t <= 699
  float* out_rgb; float* out_direct; float* out_indirect;                // [n_rays][count][3], NULL = not wanted
};
void rc_launch_transient_slice(const RcTransSliceArgs& a, hipStream_t stream);


// ---------------------------------------------------------------------------------------------
// On-device ray generation (rc_camera.hip)
// ---------------------------------------------------------------------------------------------
// What every camera of a call shares (the reference's `cameras` tuple beyond the per-camera matrices)
struct RcCastShared {
  float near_v, far_v;
  int32_t camtype;                                  // 0 perspective, 1 panoramic, 2 fisheye, 3 fisheye (equisolid)
  int32_t has_distortion; float dist[6];            // k1 k2 k3 k4 p1 p2
  int32_t has_ndc; float ndc_xmult, ndc_ymult;      // 1 / pixtocam_ndc[0][2], 1 / pixtocam_ndc[1][2]
  int32_t has_z_range; float z_lo, z_hi;            // cast_ray_batch's z_range
};
struct RcCastOut {                                  // rc_cast_outputs; NULL = not wanted
  float* origins; float* directions; float* viewdirs; float* radii; float* imageplane; float* look; float* up;
  float* lights; float* near; float* far;
};
struct RcCastArgs {
  int64_t n;
  const int32_t* pix_x; const int32_t* pix_y;      // explicit pixel batch, or NULL: the rectangle below, row-major
  int32_t x0, y0, width;
  float pixtocam[9]; float rot[9]; float trans[3]; float light[3];
  RcCastShared s;
  const float* pix_dx; const float* pix_dy;         // sub-pixel jitter offsets [n] or NULL
  RcCastOut out;
};
void rc_launch_cast_rays(const RcCastArgs& a, hipStream_t stream);

// Rays of a batch that mixes cameras, and the training batch built from a PRNG key (rc_batch.hip)
struct RcCameraTables {
  int32_t count;                                    // C >= 1
  const float* pixtocams;                           // [C, 9]
  const float* camtoworlds;                         // [C, 12]
  const float* lights;                              // [C, 3] or NULL: the camera centre
};
struct RcCastMultiArgs {
  int64_t n;
  RcCameraTables cams; RcCastShared s;
  const int32_t* cam_idx; const int32_t* pix_x; const int32_t* pix_y;
  const float* pix_dx; const float* pix_dy;
  RcCastOut out;
};
struct RcTrainBatchArgs {
  int64_t n;                                        // P * p * p rays
  RcCameraTables cams; RcCastShared s;
  const void* images; int32_t image_u8;             // [C, H, W, 3] float32, or uint8 (value / 255)
  int32_t height, width;
  const float* cam_lossmult;                        // [C] or NULL (1)
  uint32_t key0, key1; uint32_t n_words;            // 3 P words of random_bits(key, (P, 3))
  int32_t patch, x_lo, x_range, y_lo, y_range;      // p; x in [x_lo, x_lo + x_range), y likewise
  int32_t single_image;
  const float* pix_dx; const float* pix_dy;
  RcCastOut out;
  float* rgb; float* lossmult; int32_t* cam_idx; int32_t* pix_x; int32_t* pix_y;
};
void rc_launch_cast_rays_multi(const RcCastMultiArgs& a, hipStream_t stream);
void rc_launch_train_batch(const RcTrainBatchArgs& a, hipStream_t stream);

// Training backward of one level's density field (rc_train.hip)
struct RcDensityBwdArgs {
  const float* feat;          // grid features, feature-major [K][ld] (k_hashgrid_fwd)
  int64_t n; int64_t ld;
  int32_t K;
  const float* wstream;       // [d0 | d1 | out | W1^T | W0^T] fragments
  const float* points;        // world-space [n,3]
  float density_bias, contract_radius, bbox;
  const float* d_density;     // [n] upstream
  const float* d_feature;     // [n,64] upstream or nullptr
  float* density;             // [n]
  float* graw;                // [n] d L / d raw density
  float* a1; float* a2; float* d2; float* d1;   // point-major [n,64]
  float* fe;                  // point-major [n,32] staged grid features
  float* dfeat;               // feature-major [K][ld] d L / d grid feature
};
void rc_launch_density_bwd(const RcDensityBwdArgs& a, hipStream_t stream);
struct RcWgradArgs {
  const float* a1; const float* d2; const float* fe; const float* d1; const float* a2; const float* graw;
  int64_t n; int32_t K; int64_t steps_per_wave;
  float* partial;             // [rc_wgrad_waves(n) / 4][partial stride]: one per workgroup
};
int rc_wgrad_waves(int64_t n);
int rc_wgrad_partial_floats(int nwaves);
// grads: [W0 K x 64 | b0 64 | W1 64 x 64 | b1 64 | Wout 64 | bout 1], accumulated into
// no_bias: the three bias segments are left as they are (rc_normals_backward: their gradient is an exact zero)
void rc_launch_wgrad(RcWgradArgs a, int K, float* grads, hipStream_t stream, bool no_bias = false);
struct RcGridScatterArgs {
  RcGridDev grid;             // geometry of the forward tables
  float* gtable[RC_MAX_GRID_LEVELS];   // gradient tables, same layout as the forward tables
  const float* points;        // world-space [n,3]
  int64_t n; int64_t ld;
  const float* dfeat;         // feature-major [L*F][ld], or point-major [n][L*F] (point_major != 0)
  float contract_radius;
  int32_t point_major;
  int32_t level0;             // first level of this launch (blockIdx.y = level - level0)
  uint32_t lds_levels;        // bit l: level l is summed through LDS by k_grid_scatter_small
};
void rc_launch_grid_scatter(const RcGridScatterArgs& a, hipStream_t stream);
bool rc_train_prepare();     // LDS opt-in of the scatter kernels (call once outside any stream capture)

// Gradient THROUGH the analytic normals of the last level and the geometry smoothness loss (rc_normals_bwd.hip)
struct RcNormalsBwdArgs {
  const float* feat;          // grid features, feature-major [32][ld] (k_hashgrid_fwd)
  const float* jac;           // [3][32][ld] d feature / d contracted coordinate (k_hashgrid_fwd<F, true>)
  int64_t n; int64_t ld;
  const float* wstream;       // [d0 | d1 | out | W1^T | W0^T | d0 | d1] fragments
  const float* points;        // world-space [n,3]
  float contract_radius;
  const float* d_normals;     // [n,3] upstream
  float* normals;             // [n,3] the analytic normals, or nullptr
  float* u;                   // point-major [n,32] d L / d (d raw / d feature)
  float* t0; float* a0; float* t1; float* a2;   // point-major [n,64]
  float* ones;                // [n] written: 1
  float* gf;                  // feature-major [32][ld] d raw / d grid feature
  float* ghat;                // [n,3] d L / d (sum_i J[i][.] gf[i]), contracted axes (x, y, z)
};
void rc_launch_normals_bwd(const RcNormalsBwdArgs& a, hipStream_t stream);
// the table gradients of the trilinear Jacobian: s's dfeat is gf (feature-major), every corner takes
// precondition gf s_l sum_ax ghat[ax] d w_c / d loc_ax
void rc_launch_grid_scatter_jac(const RcGridScatterArgs& s, const float* ghat, hipStream_t stream);
struct RcGSmoothLossArgs {
  int64_t n; int S;                        // rays, last-level intervals (<= 32)
  const float* density, * tdist, * directions;   // the training forward's last level
  const float* normals;                    // SoA [3][n S] analytic normals at the means
  const float* density_p, * normals_p;     // the same at the perturbed means
  const float* lossmult;                   // [n] or nullptr (1)
  float wn3, wd;                           // weight_normals / 3, weight_density: the per-sample loss sum
  float gn, gd;                            // weight_normals / (3 n S), weight_density / (n S): d loss / d |term|
  float* weights;                          // [n S] the last level's weights, written
  float* loss_ray;                         // [n] written
  float* d_normals, * d_normals_p;         // [n S][3] written, or nullptr (loss only)
  float* d_density, * d_density_p;         // [n S] written when wd != 0 and d_normals is given
};
// means_p (SoA [3][np]) = fl(means + fl(noise * scale)); points / points_p: both as [np][3]
void rc_launch_gsmooth_points(const float* means, const float* noise, float scale, int64_t np, float* means_p, float* points,
                              float* points_p, hipStream_t st);
void rc_launch_gsmooth_loss(const RcGSmoothLossArgs& a, hipStream_t st);

// Spline interlevel loss and d loss / d density of the proposal levels (rc_interlevel.hip)
struct RcInterlevelArgs {
  int64_t n;                               // rays
  int num_levels;                          // sampler levels; the last is the target, 0 .. num_levels - 2 get a loss
  int S[RC_MAX_LEVELS];                    // intervals per level
  const float* sdist[RC_MAX_LEVELS];       // [n][S + 1]
  const float* tdist[RC_MAX_LEVELS];       // [n][S + 1]
  const float* density[RC_MAX_LEVELS];     // [n][S]
  const float* directions;                 // [n][3]
  const float* lossmult;                   // [n] or nullptr (1)
  float blur[RC_MAX_LEVELS];               // halfwidth per proposal level
  float coef[RC_MAX_LEVELS];               // mult / (n S) per proposal level: d loss / d (per-sample term)
  float* d_density[RC_MAX_LEVELS];         // [n][S] per proposal level, written
  float* loss_ray;                         // [num_levels - 1][n] per-ray sums of the per-sample terms, written
};
struct RcInterlevelReduce { float mult[RC_MAX_LEVELS]; double count[RC_MAX_LEVELS]; };
bool rc_interlevel_supported(int num_levels, const int* S);
void rc_launch_interlevel_bwd(const RcInterlevelArgs& a, hipStream_t stream);
void rc_launch_interlevel_reduce(const float* loss_ray, int64_t n, int levels, const RcInterlevelReduce& r, float* losses,
                                 hipStream_t stream);
void rc_launch_points_aos(const float* soa, int64_t np, float* aos, hipStream_t stream);

// Data loss of the cache pass and the shader backward (rc_data.hip)
struct RcDataLossArgs {
  int64_t n; int S;                        // rays, last-level intervals (<= 32)
  const float* rgb;                        // [n][3] the composite
  const float* gt;                         // [n][3]
  const float* lossmult;                   // [n] or nullptr (1)
  const float* weights, * density, * tdist, * shade, * directions;   // the training forward's last level
  float bg, padding, coef;                 // background, charb padding, mult / (3 n)
  float* loss_ray;                         // [n] per-ray sums of lossmult * charb, written
  float* d_density;                        // [n S] written
  float* d_rgbs;                           // [n S][3] d L / d rgb_s, written
};
// C(i, j) (+)= sum_k A(i, k) B(k, j) (+ bias[j]), then ReLU, then zero where mask(i, j) <= 0.  A(i, k) = a[i sai + k sak],
// B(k, j) = b[k sbk + j sbj], C(i, j) = c[i sci + j scj] (+ z spart for K slice z of kslice values).
struct RcGemmArgs {
  int M, N; int64_t K;
  const float* a; int64_t sai, sak;
  const float* b; int64_t sbk, sbj;
  float* c; int64_t sci, scj;
  const float* bias;
  const float* mask; int64_t smi, smj;
  int relu, accumulate;
  int64_t kslice, spart;
};
// One chunk of C samples (global index c0 + p) of the shader backward: row-major per-sample buffers.
struct RcShaderBwdArgs {
  int64_t C, c0, np; int S;
  const float* hbuf, * app, * viewdirs;    // the training forward (hbuf: accumulator order, app: [32][np])
  const RcIdeTable* ide;
  float roughness_bias, ambient_bias, irradiance_bias, slf_ambient_bias, rgb_max;
  const float* d_rgbs;                     // [np][3]
  float* f96, * heads, * p3, * ib_in, * x328, * io, * so;                     // recompute
  float* dheads, * dio, * dso, * dib_in, * dx328, * db128, * dp3;             // gradients
};
void rc_launch_data_loss_bwd(const RcDataLossArgs& a, hipStream_t st);
void rc_launch_gemm(const RcGemmArgs& a, int kparts, hipStream_t st);
void rc_launch_sum_parts(const float* part, int nparts, int64_t count, float* out, hipStream_t st);
void rc_launch_shader_stage(const RcShaderBwdArgs& a, int which, hipStream_t st);   // 0 stage, 1 glue fwd, 2 out bwd, 3 glue bwd
void rc_launch_split_feature(const float* df96, int64_t C, float* dfeat, float* dapp, hipStream_t st);

// Geometry losses of the last level and the density-grid regularizer (rc_geometry.hip)
struct RcGeometryLossArgs {
  int64_t n; int S;                        // rays, last-level intervals (<= 32)
  const float* density, * tdist, * directions, * viewdirs;   // the training forward's last level
  float* weights;                          // [n S] the last level's weights, written
  const float* lossmult;                   // [n] or nullptr (1)
  const float* normals_pred, * normals_grad;   // SoA [3][n S]: n^ and the analytic normals
  const float* hbuf;                       // hidden vectors, accumulator order (k_density_mlp)
  const float* wn;                         // pred_normals_layer: kernel [64][3], then bias [3]
  float dist_p, dist_premult;              // distortion curve: power_ladder(tdist, p, premult)
  float dist_coef, orient_coef, pn_coef, pnr_coef;   // mult / n of each term
  float pn_wgrad;                          // stopgrad_with_weight of w in the predicted-normal term
  float* loss_ray;                         // [4][n] per-ray values, written
  float* d_density;                        // [n S] written, or nullptr (losses only)
  float* d_pred;                           // [n S][3] d L / d pred_raw, written with d_density
};
struct RcGridL2Reduce { float mult; int tables; int64_t count[RC_MAX_GRID_LEVELS]; };
void rc_launch_geometry_loss_bwd(const RcGeometryLossArgs& a, hipStream_t st);
void rc_launch_stage_hidden(const float* hbuf, int64_t c0, int64_t C, float* h64, hipStream_t st);
int rc_grid_l2_blocks();                   // partial sums per table of rc_launch_grid_l2_bwd
void rc_launch_grid_l2_bwd(const float* x, int64_t count, float gscale, float* grad, double* part, hipStream_t st);
void rc_launch_grid_l2_reduce(const double* part, const RcGridL2Reduce& r, float* loss, hipStream_t st);

// Mask loss of the last level's opacity and the rays of its backward term (rc_mask.hip)
struct RcBackwardMaskRaysArgs {
  int64_t n;
  const float* origins, * look;            // [n][3] the batch rays' origins and camera look vectors
  const float* u1, * u2;                   // [n] the uniform pair of each ray, in [0, 1)
  float shadow_near_max, normal_eps, far;
  float* o_origins, * o_directions;        // [n][3] written
  float* o_near, * o_far;                  // [n] written
};
struct RcMaskLossArgs {
  int64_t n; int S;                        // rays, last-level intervals (<= 32)
  const float* density, * tdist, * directions;   // the training forward's last level
  float* weights;                          // [n S] the last level's weights, written
  const float* masks;                      // [n], or nullptr: ones (zeros with zero_masks)
  const float* lossmult;                   // [n] or nullptr (1)
  float padding, weight_opaque, weight_empty;
  int zero_masks;
  float inv_n;                             // 1 / n: the mean over the rays
  float* loss_ray;                         // [n] lossmult * wt * charb per ray, written
  float* d_density;                        // [n S] written
};
void rc_launch_backward_mask_rays(const RcBackwardMaskRaysArgs& a, hipStream_t st);
void rc_launch_mask_loss_bwd(const RcMaskLossArgs& a, hipStream_t st);

// The light sampler's own loss (rc_light.hip)
struct RcLightLossArgs {
  int64_t n; int Ks, Kd;                   // shading points, secondary samples per suffix
  const float* vp;                         // [n][640] the light head's vmf_params
  const float* noise;                      // [n][128][3] the vMF mean noise
  const float* pts, * nrm;                 // [n][3] shading point, normals_to_use
  const float* sec_dirs, * sec_rgb;        // [n Ks | n Kd][3] the batched trace's directions and colours
  const float* samples;                    // [n][Ks + Kd][RC_SMP_CH] local direction, pdf, MIS weight
  const float* lossmult;                   // [n] or nullptr (1)
  float vmf_scale;
  int srgb;                                // linear_to_srgb on f and the likelihood
  float coef_spec, coef_diff;              // mult / 2 / (n K_s): d loss / d (per-sample term)
  float* loss_ray;                         // [n] per-point sum over s of (sum of the terms) / K_s, written
  float* dvp;                              // [n][640] d loss / d vmf_params, written, or nullptr (loss only)
};
void rc_launch_light_sampling_loss_bwd(const RcLightLossArgs& a, hipStream_t st);

// The material network's smoothness loss (rc_material_bwd.hip)
constexpr int kRcMatSmoothParts = 32 * 128 + 128 + 128 * 10 + 10;   // floats of one workgroup's weight-gradient partial
struct RcMatSmoothArgs {
  int64_t n;                               // shading points
  const float* feat_x, * feat_p;           // [n][32] material-grid features at x and at x'
  const float* w0, * b0, * w1, * b1;       // bottleneck_layer [32][128], [128]; pred_brdf_layer [128][10], [10]
  float min_roughness;
  const float* filt_weight;                // [n] the shading sample's weight
  const float* lossmult;                   // [n] or nullptr (1)
  int tensoir;                             // material_smoothness_tensoir_albedo
  float wa, wo;                            // weight_albedo / 3, weight_other: the per-point loss sum
  float ga, go;                            // mult weight_albedo / (3 n), mult weight_other / n: d loss / d |term|
  float* mat_x, * mat_p;                   // [n][RC_MAT_CH] the materials at x (bitwise m_mat) and at x', written
  float* loss_ray;                         // [n] per-point loss sums, written
  float* dfeat;                            // [2n][32] d loss / d features (x, then x'), written when part is given
  float* part;                             // [rc_mat_smooth_blocks(n)][kRcMatSmoothParts] or nullptr (loss only)
  double* loss_part;                       // [rc_mat_smooth_blocks(n)] per-workgroup loss sums, written
};
int rc_mat_smooth_blocks(int64_t n);
void rc_launch_material_smoothness_points(const float* pts, const float* noise, float scale, int64_t n, float* out,
                                          hipStream_t st);
void rc_launch_material_smoothness_bwd(const RcMatSmoothArgs& a, hipStream_t st);
// loss = mult * sum / n (fixed order); with grads: grads (the layout's four dense segments) += the partials, fixed order
void rc_launch_material_smoothness_reduce(const RcMatSmoothArgs& a, float* grads, float mult, float* loss, hipStream_t st);
// the same reduction for any caller of material_head_bwd: nparts (<= 1024) partials of kRcMatSmoothParts floats and
// per-workgroup loss sums; loss = mult * (sum) / count
void rc_launch_material_partials_reduce(const float* part, int nparts, const double* loss_part, float* grads, float mult,
                                        double count, float* loss, hipStream_t st);

// The material stage's data loss (rc_material_data.hip)
struct RcMatDataArgs {
  int64_t n; int32_t Ks, Kd, S;
  // rc_render_material's step-7 inputs (set 0), read as k_material_integrate reads them
  const float* mat; const float* samples; const float* local_view;
  const float* sec_rgb; const float* sec_acc; const float* sec_env;
  const float* weights;                    // [n][S] unfiltered weights of the primary rays
  const float* filt_weight;                // [n]
  float f0, rgb_max, bg;
  // the loss
  const float* gt;                         // [n][3]
  const float* lossmult;                   // [n] or nullptr (1)
  const float* cache_rgb;                  // [n][3] the primary cache pass's rgb (the rendering's "cache_rgb")
  float exponent, eps, clip_val, thresh;
  int use_gt, use_combined, use_norm;
  float coef;                              // weight * data_loss_mult / (3 n): d loss / d (per-element term)
  float* rgb;                              // [n][3] the rebuilt rgb, written
  float* loss_ray;                         // [n] per-point sums over the channels of lossmult 2 d sg(d) s, written
  float* dmat;                             // [n][5] d loss / d (albedo rgb, roughness, metalness), written, or nullptr
};
void rc_launch_material_data_bwd(const RcMatDataArgs& a, hipStream_t st);
struct RcMatDataHeadArgs {
  int64_t n;
  const float* feat;                       // [n][32] material-grid features at the shading points (m_feat)
  const float* w0, * b0, * w1, * b1;
  float min_roughness;
  const float* dmat;                       // [n][5] or nullptr (loss only)
  const float* loss_ray;                   // [n]
  float* dfeat;                            // [n][32] d loss / d features, written when part is given
  float* part;                             // [rc_mat_data_blocks(n)][kRcMatSmoothParts] or nullptr (loss only)
  double* loss_part;                       // [rc_mat_data_blocks(n)] per-workgroup loss sums, written
};
int rc_mat_data_blocks(int64_t n);
void rc_launch_material_data_head_bwd(const RcMatDataHeadArgs& a, hipStream_t st);
// k_material_data_env_bwd: k_material_data_bwd's recompute, then d loss / d (the EnvMap radiance of every secondary ray)
// times env_scale into d_env [n Ks | n Kd][3] (the sec_* ray order); a's rgb / loss_ray / dmat are not written
void rc_launch_material_data_env_bwd(const RcMatDataArgs& a, float env_scale, float* d_env, hipStream_t st);

// The EnvMap's gradient of the material data loss (rc_envmap_bwd.hip)
constexpr int kRcEnvIn = 27, kRcEnvWidth = 256, kRcEnvBott = 128;   // pos_enc(d, 0, 4) + identity, the trunk, layer_bottleneck
constexpr int kRcEnvLdx = 288;             // row stride of [layer_2's output (256) | the encoded direction (27) | 0 (5)]
// xb[p][256 .. 288) = [pos_enc(dirs[c0 + p], 0, 4, append_identity) | 0], k_envmap's sinf arguments; p < C
void rc_launch_envmap_stage(const float* dirs, int64_t c0, int64_t C, float* xb, hipStream_t st);
// d_raw[p][c] = d_env[c0 + p][c] max'(softplus(z), 0) sigmoid(z), z = raw[p][c] + rgb_bias (c < 3); d_raw[p][3] = 0
void rc_launch_envmap_out_bwd(const float* d_env, const float* raw, float rgb_bias, int64_t c0, int64_t C, float* d_raw,
                              hipStream_t st);
// RcGemmArgs' product on k_gemm_tile (a 128 x 128 tile of C per workgroup, the operand panels staged through LDS):
// kparts K slices on blockIdx.y as rc_launch_gemm.  Same results as k_gemm up to the order of the sum over k.
void rc_launch_gemm_tile(const RcGemmArgs& a, int kparts, hipStream_t st);

// The time-resolved cache's data loss and the backward of k_transient_bins (rc_transient_bwd.hip)
constexpr int kRcTdLdSlf = kRcTdHist + 4;                      // row stride of dZ_slf: the alpha column and 3 pad floats, zeros
constexpr int kRcTdChunkRays = 256;                            // rays whose dZ the workspace holds at a time
struct RcTransLossArgs : RcTransTaps {
  int64_t n;                                               // rays
  const float* rgb, * gt;                                  // [n][700][3]
  const float* rgb_nocorr, * gt_nocorr;                    // [n][700][3] or nullptr (rgb, gt)
  const float* lossmult;                                   // [n] or nullptr (1)
  float coef;                                              // data_loss_mult / (3 n): d loss / d (per ray-and-channel term)
  float gauss;                                             // 2 constant_scale^2 data_loss_gauss_mult
  float exponent, eps, clip_val, thresh;
  int32_t use_gt, use_combined;
  float* G, * Gt;                                          // [n][700][3] d loss / d rgb and the filter's transpose of it, written
  float* loss_ray;                                         // [2][n] per-ray sums of the loss terms and of lossmult (rgb - gt)^2
};
struct RcTransBinsBwdArgs : RcTransIn {                   // the batch: the forward's buffers and settings
  int64_t r0, C;                                           // this launch's rays [r0, r0 + C)
  const float* w_slf, * b_slf, * w_irr, * b_irr;           // output_rgba_layer [128][2101], [2101]; transient_indirect_layer [64][2100], [2100]
  const float* G, * Gt;                                    // [n_rays][2100]
  float* dz_irr, * dz_slf;                                 // [C 32][2100], [C 32][kRcTdLdSlf] written (zeros outside the live tiles)
  float* x_irr, * x_slf;                                   // [C 32][64], [C 32][128] the heads' inputs, reference column order, written
  float* d_tib, * d_direct, * d_weights;                   // [n_rays 32][3], [n_rays 32][3], [n_rays 32] written for the chunk's rays
};
// k_transient_loss_kinds: the same outputs under any rc_transient_loss_type, with or without use_itof
struct RcTransLossKindArgs {
  RcTransLossArgs base;                                    // as k_transient_loss reads it
  int32_t kind;                                            // rc_transient_loss_type
  int32_t use_itof;                                        // Config.use_itof: data_loss / rows, the mse stat in its iToF form
  int32_t n_rows;                                          // 2 n_pairs + 1 rows of W (read by the iToF types and under use_itof)
  float q;                                                 // 1 / rows under use_itof (n_rows or 700), else 1
  const float* W;                                          // [n_rows][700] the modulation table (rc_itof_host.h, device)
};
struct RcDtofToItofArgs {
  int64_t n; int32_t n_rows;
  const float* W;                                          // [n_rows][700]
  const float* x;                                          // [n][700][3]
  float* out;                                              // [n][n_rows][3] written
};
void rc_launch_transient_loss(const RcTransLossArgs& a, hipStream_t st);
void rc_launch_transient_loss_kinds(const RcTransLossKindArgs& a, hipStream_t st);
void rc_launch_dtof_to_itof(const RcDtofToItofArgs& a, hipStream_t st);
void rc_launch_transient_bins_bwd(const RcTransBinsBwdArgs& a, hipStream_t st);

// The data loss's gradient through the compositing weights of the last level (rc_transient_sampler.hip)
struct RcTransWeightsBwdArgs {
  int64_t n; int32_t S;                                    // rays, samples per ray (<= 32)
  const float* d_weights;                                  // [n S] d loss / d weights ("td:d_weights")
  const float* weights, * density;                         // [n S] the forward's compositing weights and density of the last level
  const float* tdist;                                      // [n][S + 1]
  const float* directions;                                 // [n][3]
  float* d_density;                                        // [n S] written
};
void rc_launch_transient_weights_bwd(const RcTransWeightsBwdArgs& a, hipStream_t st);

// Evaluation of a rendered view (rc_metrics.hip).  Partial sums are doubles, one slot set per workgroup.
struct RcEvalBinsArgs {
  const float* pred, * gt;                                 // [n_pix][n_bins][3]
  int64_t n_pix; int32_t n_bins;
  int32_t vec_ok;                                          // both arrays reach a 16-byte boundary after the same number of floats
  float* binsum_pred, * binsum_gt;                         // [n_pix][3] written
  double* part;                                            // [rc_eval_bins_blocks(n_pix)][2]: sum of min, sum of max
};
struct RcEvalPixelArgs {
  const float* pred, * gt;                                 // [n_pix][3]: the images, or the bin sums (bins != 0)
  const float* mask;                                       // [n_pix] or nullptr
  const float* acc, * normals, * normals_gt;               // [n_pix], [n_pix][3] x 2; all three or none
  const float* distance_mean, * distance_median, * depth_gt;   // [n_pix] each or nullptr
  int64_t n_pix;
  int32_t bins, clip_eval, skip;                           // skip: no post-process, the images as they are (times mask)
  float exposure, img_scale;
  float* post_pred, * post_gt;                             // [n_pix][3] written
  double* part;                                            // [rc_eval_pixel_blocks(n_pix)][rc_eval_pixel_parts()]
};
struct RcEvalSsimArgs {
  const float* a, * b;                                     // [height][width][3]
  int32_t height, width;
  float taps[11];                                          // the normalised Gaussian window
  float c1, c2;
  float* map;                                              // [height - 10][width - 10][3] or nullptr
  double* part;                                            // [3][tiles_y][tiles_x]
};
struct RcEvalFinishArgs {
  const double* part_pixels, * part_ssim, * part_bins;
  int64_t n_part_pixels, n_part_ssim, n_part_bins;         // workgroups of each kernel (0: the kernel did not run)
  int64_t n_pix;
  double ssim_count;                                       // (H - 10)(W - 10) 3
  int32_t masked, have_l1_mean, have_l1_median, have_mae;
  double* out;                                             // [RC_EVAL_COUNT] device doubles
};
int rc_eval_bins_blocks(int64_t n_pix);
int rc_eval_pixel_blocks(int64_t n_pix);
int rc_eval_pixel_parts();
void rc_eval_ssim_tiles(int height, int width, int* ty, int* tx);
void rc_launch_eval_bins(const RcEvalBinsArgs& a, hipStream_t stream);
void rc_launch_eval_pixels(const RcEvalPixelArgs& a, hipStream_t stream);
void rc_launch_eval_ssim(const RcEvalSsimArgs& a, hipStream_t stream);
void rc_launch_eval_finish(const RcEvalFinishArgs& a, hipStream_t stream);

// Shift-invariant PSNR / SSIM (rc_metrics.hip).  The shifts are processed one di row at a time: a group
// is the 2 radius_j + 1 shifts (di, -radius_j .. radius_j); the search state is carried between groups in [H][W] arrays.
enum RcSiKind { RC_SI_MSE = 0, RC_SI_SSIM = 1 };
struct RcSiMetricArgs {
  const float* pred, * gt;                                 // [height][width][3]
  int32_t height, width;
  int32_t di, radius_j;                                    // the group: dj = -radius_j .. radius_j
  float taps[11];                                          // ssim: the normalised Gaussian window
  float c1, c2;
  float* metric;                                           // [2 radius_j + 1][height][width] written
};
struct RcSiSelectArgs {
  const float* metric;                                     // [2 radius_j + 1][height][width]
  int32_t height, width;
  int32_t di, radius_j, halfwidth;
  int32_t first, last;                                     // the search's first group (no state yet) / its last one
  int32_t crop;                                            // the partial sums cover [crop, height - crop) x [crop, width - crop)
  float* best_pooled, * best_metric;                       // [height][width] the state, read (first == 0) and written
  int32_t* best_di, * best_dj;
  float* out_map;                                          // last only: [height][width] or nullptr
  int32_t* out_di, * out_dj;
  double* part;                                            // last only: one per workgroup
};
struct RcSiFinishArgs {
  const double* part_mse, * part_ssim;                     // part_ssim nullptr: no ssim search ran
  int64_t n_part;
  double n_mse, n_ssim;                                    // H W, (H - 10)(W - 10)
  double* out;                                             // [RC_EVAL_SI_COUNT] device doubles
};
void rc_si_tiles(int height, int width, int* ty, int* tx);
void rc_launch_si_metric(int kind, const RcSiMetricArgs& a, hipStream_t stream);
void rc_launch_si_select(int kind, const RcSiSelectArgs& a, hipStream_t stream);
void rc_launch_si_finish(const RcSiFinishArgs& a, hipStream_t stream);

// Evaluation of the albedo (rc_albedo.hip).  A pair row is (gt'[3], p[3]); a selection is one order
// statistic of one channel's ratios: selection 2 c is channel c's lower middle rank, 2 c + 1 its upper one.
constexpr int kRcAlbedoSelections = 6, kRcAlbedoDigits = 256;
struct RcAlbedoState {                                     // on the device, the "ea:" set's `state`
  int64_t base;                                            // the caller's *pairs_count before this view
  int64_t total;                                           // this view's valid rows
  int64_t rows;                                            // rows a ratio is taken over (0 on overflow)
  int32_t overflow;                                        // the count had passed the capacity
  uint32_t nan[3];                                         // NaN ratios per channel
  uint32_t prefix[kRcAlbedoSelections], rank[kRcAlbedoSelections];   // key bits fixed so far; rank among the keys that share them
  float ratio[3];                                          // the result of the select / the least squares
  uint32_t hist[kRcAlbedoSelections][kRcAlbedoDigits];     // zero between the passes
};
struct RcAlbedoPixelArgs {
  const float* albedo, * acc, * albedo_gt, * mask;         // [n_pix][3], [n_pix], [n_pix][3], [n_pix] or nullptr
  int64_t n_pix;
  int32_t* wg;                                             // [blocks]: valid pixels per workgroup, then (scan) those before it
  RcAlbedoState* state;
  float* own;                                              // [n_pix][6] the workspace's pair buffer, from row 0, or nullptr
  float* pairs; int64_t capacity; int64_t* count;          // the caller's pair buffer, appended to, or nullptr
  const float* ratio;                                      // [3] applied (k_albedo_score)
  float albedo_clip;
  float* post_pred, * post_gt, * ratio_im;                 // [n_pix][3] or nullptr
  double* part;                                            // [blocks]: squared errors
  double* out;                                             // [RC_ALBEDO_COUNT]
};
struct RcAlbedoRatioArgs {
  const float* pairs; int64_t capacity;
  const int64_t* count;                                    // device; nullptr: state->total rows (the workspace's buffer)
  RcAlbedoState* state;
  int32_t gamma;
  double* part;                                            // [rc_albedo_row_blocks(capacity)][6]: least squares
  float* ratio;                                            // [3] written besides state->ratio, or nullptr
};
int rc_albedo_pixel_blocks(int64_t n_pix);
int rc_albedo_row_blocks(int64_t capacity);
void rc_launch_albedo_compact(const RcAlbedoPixelArgs& a, hipStream_t stream);   // count, scan, write
void rc_launch_albedo_score(const RcAlbedoPixelArgs& a, hipStream_t stream);     // apply, score, finish
void rc_launch_albedo_median(const RcAlbedoRatioArgs& a, hipStream_t stream);
void rc_launch_albedo_lstsq(const RcAlbedoRatioArgs& a, hipStream_t stream);

// Visualisation of a view (rc_vis.hip).  A selection is one requested percentile of the weighted select.
constexpr int kRcVisSelections = 8, kRcVisDigits = 256, kRcVisMaxBlocks = 256, kRcVisItemsPerLaunch = 24;
struct RcVisState {                                        // on the device, the "vz:" set's `state`
  double total;                                            // W
  double t[kRcVisSelections];                              // p (W / 100)
  double below[kRcVisSelections];                          // the weight of the keys under the prefix: B after the last pass
  uint32_t prefix[kRcVisSelections];                       // key bits fixed so far: v1's key after the last pass
  int32_t found[kRcVisSelections];                         // some value has C(v) > t
  uint32_t lower[kRcVisSelections];                        // 1 + the largest key below v1's, 0: none (integer max)
  uint32_t first[kRcVisSelections];                        // the first element in pixel order with v1's key (integer min)
  uint32_t max_key;                                        // the largest key (integer max)
  int32_t bad;                                             // a negative, NaN or infinite weight was seen
};
struct RcVisSelectArgs {
  const float* value, * weight;                            // [n], [n] or nullptr: all ones
  int64_t n;
  int32_t n_ps;
  double ps[kRcVisSelections];
  RcVisState* state;
  double* part;                                            // [blocks][n_ps][kRcVisDigits]: weight sums per workgroup
  double* out;                                             // [n_ps]
};
struct RcVisMaxArgs { const float* src; int64_t n; float* part; float* out; };
struct RcVisBinsArgs { const float* src; int64_t n_pix; int32_t n_bins, channels; float* dst; };   // dst: [n_pix][channels]
struct RcVisDevItem {
  const float* src, * divisor, * acc, * mask;
  const double* bounds, * auto_bounds;
  float* out_f32; uint8_t* out_u8;
  int32_t channels, op, nan_to_num;
  float scale, divide, offset, exponent;
};
struct RcVisItemsArgs { RcVisDevItem item[kRcVisItemsPerLaunch]; int64_t n_pix; };
int rc_vis_select_blocks(int64_t n);
int rc_vis_max_blocks(int64_t n);
void rc_launch_vis_select(const RcVisSelectArgs& a, hipStream_t stream);
void rc_launch_vis_max(const RcVisMaxArgs& a, hipStream_t stream);
void rc_launch_vis_bins(const RcVisBinsArgs& a, hipStream_t stream);
void rc_launch_vis_items(const RcVisItemsArgs& a, int n_items, hipStream_t stream);
const float* rc_vis_turbo_host();

// The probe of a surface point (rc_probe.hip): the panorama of secondary rays cast from the hit points
// of P pixels of a rendered view, and the panorama of each pixel's vMF mixture.
constexpr int kRcProbeMax = RC_PROBE_MAX, kRcProbeMaxLobes = RC_PROBE_MAX_LOBES;
struct RcProbeRaysArgs {
  const float* origins, * directions, * distance_median, * normals;     // the view's rows
  const float* lights, * imageplane, * look, * up;                       // row 0 goes to every ray; nullptr: the cast's own
  int64_t pixel[kRcProbeMax];                                            // the row of each probe
  int32_t P, height, width, flip;
  int64_t n;                                                             // P * height * width
  float normal_offset, phi_offset, theta_offset;                         // pi / W and pi / (2 H), rounded from double
  float pixtocam[9], rot[9];                                             // diag(2 pi / W, pi / H, 1), the identity
  RcCastShared s;                                                        // camtype 1, near, far
  RcCastOut out;
  float* positions;                                                      // [P,3] or nullptr
};
struct RcVmfPanoramaArgs {
  const float* means, * kappas, * logits;                                // [P,V,3], [P,V], [P,V]
  int32_t V, height, width, flip;
  float phi_offset, theta_offset;
  float* out_linear, * out_srgb; uint8_t* out_u8;                        // [P,H,W], [P,H,W,3], [P,H,W,3]; nullptr: not wanted
};
void rc_launch_probe_rays(const RcProbeRaysArgs& a, hipStream_t stream);
void rc_launch_vmf_panorama(const RcVmfPanoramaArgs& a, int P, hipStream_t stream);

// Surface export (rc_mesh.hip): the plumbing of rc_query_points / rc_density_lattice around the forward
// kernels, and the marching tetrahedra of rc_isosurface.
// rows [n][3] -> SoA [3][n] and back (the density MLP reads and writes SoA)
void rc_launch_rows_to_soa(const float* rows, int64_t n, float* soa, hipStream_t stream);
void rc_launch_soa_to_rows(const float* soa, int64_t n, float* rows, hipStream_t stream);
// Lattice points first .. first + n of an [nx, ny, nz] lattice (iz fastest) as SoA [3][n]: axis a's point i sits at
// lo[a] + (float)i * step[a]
struct RcLatticeArgs { float lo[3], step[3]; int32_t nx, ny, nz; };
void rc_launch_lattice_points(const RcLatticeArgs& a, int64_t first, int64_t n, float* soa, hipStream_t stream);
void rc_launch_nan_to_num(float* x, int64_t n, hipStream_t stream);      // in place, jnp.nan_to_num's defaults
// rc_isosurface.  A tile is kRcIsoTile consecutive lattice points (one workgroup), a group kRcIsoGroup consecutive tiles.
constexpr int kRcIsoTile = 1024, kRcIsoGroup = 256;
struct RcIsoState { int32_t emit; };      // 1: both capacities suffice, the emission kernels write
struct RcIsoArgs {
  const float* field; RcLatticeArgs lat; float iso;
  uint32_t n;                              // nx ny nz <= 2^30
  uint32_t tiles, groups;
  uint8_t* mask;                           // [tiles kRcIsoTile] the 7 owned edges of each point that cross the surface
  uint8_t* tcount;                         // [tiles kRcIsoTile] triangles of the cell whose lowest corner the point is
  int32_t* tile_v, * tile_t;               // [tiles] vertices / triangles of a tile, then of the tiles before it in its group
  int32_t* group_v, * group_t;             // [groups] vertices / triangles of a group
  int64_t* group_off;                      // [groups][2] vertices / triangles of the groups before
  int32_t* vbase;                          // [n] index of a point's first vertex (written where mask != 0)
  RcIsoState* state;
  int64_t v_capacity, t_capacity;
  float* vertices, * normals; int32_t* triangles; int64_t* counts;
};
void rc_launch_isosurface(const RcIsoArgs& a, hipStream_t stream);

// Texture atlas (rc_atlas.hip; include/rc_abi.h states the layout rule).
struct RcAtlasLayout { int32_t cols, rows, W, H, r; int64_t T, ncells; };
// The rule's host side: RC_OK, or RC_ERR_INVALID_ARG (T < 1, r outside 4 .. 64) / RC_ERR_UNSUPPORTED (W or H above 16384)
int rc_atlas_layout_of(int64_t T, int32_t r, RcAtlasLayout& L);
void rc_launch_atlas_uvs(const RcAtlasLayout& L, float* uvs, hipStream_t stream);      // uvs [T][3][2]
struct RcAtlasPointsArgs {
  RcAtlasLayout L;
  const float* vertices; int64_t V;          // [V][3]
  const int32_t* triangles;                  // [T][3]
  int64_t first, n;                          // the texels with linear index first .. first + n
  float* rows;                               // [n][3] or nullptr
  float* soa;                                // SoA [3][n] (what the density MLP reads) or nullptr
  int32_t* owner;                            // [n] or nullptr: triangle, -1 empty, -2 a vertex index outside 0 .. V-1
};
void rc_launch_atlas_points(const RcAtlasPointsArgs& a, hipStream_t stream);
// Texels c0 .. c0 + n of the planes (already offset by the caller): zeros where owner < 0, coverage = owner >= 0
struct RcAtlasStoreArgs {
  const int32_t* owner; int64_t n;
  float* density, * normals_pred, * normals, * material, * diffuse; uint8_t* coverage;     // nullptr: not wanted
};
void rc_launch_atlas_store(const RcAtlasStoreArgs& a, hipStream_t stream);
// ambient_diffuse / indirect_diffuse of the cache shader at n points: hbuf in k_density_mlp's accumulator layout, app
// feature-major [32][ld], w = ambient_irradiance_layer kernel [96][3], bias [3], irradiance_layer kernel [96][3], bias [3]
constexpr int kRcDiffuseWeights = 2 * (96 * 3 + 3);
struct RcDiffuseArgs {
  int64_t n, ld; const float* hbuf, * app, * w;
  float ambient_bias, irradiance_bias, rgb_max;
  float* out;                                // [n][6]
};
void rc_launch_shader_diffuse_points(const RcDiffuseArgs& a, hipStream_t stream);

// The optimizer step on flat buffers (rc_optim.hip).  A run: consecutive elements of one buffer in one group.
constexpr int kRcAdamMaxBufs = 8, kRcAdamMaxRuns = 32, kRcAdamMaxGroups = 8;
struct RcAdamBuf { float* params, * grads, * mu, * nu; int64_t n, block0; int run0, nruns; };
struct RcAdamGroup { float lr, b1, b2, omb1, omb2, eps, bc1, bc2; };   // omb = 1 - b (rounded from the caller's double)
struct RcAdamArgs {
  RcAdamBuf buf[kRcAdamMaxBufs];
  int nbuf;
  int64_t run_end[kRcAdamMaxRuns];        // exclusive end of run r within its buffer
  int run_group[kRcAdamMaxRuns];
  RcAdamGroup group[kRcAdamMaxGroups];
  float max_val;                          // > 0: clip by value
  const float* mult;                      // the norm-clip multiplier on the device, or nullptr (no clip by norm)
  int zero_grads;
};
int64_t rc_adam_tile();                   // floats per workgroup tile of k_adam / k_adam_sumsq
void rc_launch_adam(const RcAdamArgs& a, int64_t blocks, hipStream_t st);
void rc_launch_adam_norm(const RcAdamArgs& a, int64_t blocks, float max_norm, double* part, float* mult, float* norm,
                         hipStream_t st);

// Random fill (rc_prng.hip)
enum { RC_PRNG_BITS = 0, RC_PRNG_UNIFORM = 1, RC_PRNG_NORMAL = 2, RC_PRNG_GUMBEL = 3 };
struct RcPrngArgs {
  uint32_t key0, key1;
  int mode;
  float lo, hi;
  int64_t n;
  uint32_t* out;
};
void rc_launch_prng_fill(const RcPrngArgs& a, hipStream_t stream);
// Several fills in one launch (k_prng_fill_segments): the table travels in the kernel arguments.  Workgroups
// [wg_end[s - 1], wg_end[s]) belong to row s; a row of n elements takes ceil(ceil(n / 2) / 256) of them.
struct RcPrngSegRow {
  uint32_t key0, key1;
  int32_t mode;
  float lo, hi;
  uint32_t n;
  int64_t off, off2;             // word offsets in the arena; off2 < 0: one plane
};
struct RcPrngSegArgs {
  RcPrngSegRow seg[RC_PRNG_MAX_SEGMENTS];
  uint32_t wg_end[RC_PRNG_MAX_SEGMENTS];
  int32_t n_segs;
  uint32_t* arena;
};
void rc_launch_prng_fill_segments(const RcPrngSegArgs& a, hipStream_t stream);

// Relighting under an explicit environment image (rc_relight.hip; the lookup itself: rc_dev_relight.h)
struct RcEnvImage { const float* padded; int32_t H, W; };   // [(H + 2)][(W + 2)][4]: zero border, 4th channel zero
struct RcEnvLookupArgs { RcEnvImage im; const float* viewdirs; int64_t n; float* out; };   // [n,3] -> [n,3]
struct RcEnvTablesArgs {
  const float* rgb; int32_t H, W; float scale;     // [H][W][3], read as rgb * scale
  float* pmf; float* pdf; float* dirs;             // [H W], [H W], [H W][3]
  double* part;                                    // [rc_env_tables_blocks(H W)] per-workgroup sums
};
struct RcEnvPickArgs {
  const float* logp; int64_t hw;                   // safe_log(pmf) [hw]
  uint32_t key0, key1; int32_t T;
  unsigned long long* best;                        // [T] (score, texel) maxima, zeroed by the launcher
  int32_t* picks;                                  // [T]
};
struct RcEnvSampleArgs {
  int64_t n; int32_t Ks, Kd;
  const float* pts; const float* nrm; const float* viewdirs; const float* lights;
  const float* pdf; const float* dirs; int64_t hw;             // the bound tables
  const int32_t* picks_spec; const int32_t* picks_diff; int32_t T_spec, T_diff;
  float normal_eps, near, far;
  float* sec_origins; float* sec_dirs; float* sec_near; float* sec_far; float* sec_lights;   // as RcBrdfSampleArgs
  float* samples; float* local_view;
};
void rc_launch_env_pad(const float* rgb, int H, int W, float* padded, hipStream_t st);
void rc_launch_env_lookup(const RcEnvLookupArgs& a, hipStream_t st);
int rc_env_tables_blocks(int64_t hw);
void rc_launch_env_tables(const RcEnvTablesArgs& a, hipStream_t st);
void rc_launch_env_logp(const float* pmf, int64_t hw, float* logp, hipStream_t st);
void rc_launch_env_pick(const RcEnvPickArgs& a, hipStream_t st);
void rc_launch_env_sample(const RcEnvSampleArgs& a, hipStream_t st);
void rc_launch_albedo_ratio(float* mat, int64_t n, const float* ratio, hipStream_t st);   // rows of RC_MAT_CH


// Kernel attributes (dynamic-LDS limit) are per device: true the first time the calling thread's current device
// shows up for this `mask` (one mask per kernel), so a process driving several GPUs sets them on each.
// CU count of the calling thread's current device, asked once per device (it sits on the launch path of the persistent
// level kernels).
inline int rc_device_cus() {
  static std::atomic<int> cached[64];
  int dev = 0;
  (void)hipGetDevice(&dev);
  int v = cached[dev & 63].load(std::memory_order_relaxed);
  if (v <= 0) {
    v = 256;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    cached[dev & 63].store(v, std::memory_order_relaxed);
  }
  return v;
}

inline bool rc_first_use_on_device(std::atomic<uint64_t>& mask) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t bit = 1ull << (dev & 63);
  return (mask.fetch_or(bit) & bit) == 0;
}
