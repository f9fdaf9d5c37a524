/*
 * rc_abi.h -- C ABI of the MI355X radiance-cache ray-batch renderer.
 *
 * The reference (benattal/neural-radiance-caching) has no FFI: the hot path sits
 * behind three Python call signatures.  These entry points are what
 * a host binding for that path would bind; each one cites the reference interface it
 * replaces (file:line relative to the reference tree).  Plain C types only: no torch,
 * no HIP types (a stream is passed as `void*` holding a hipStream_t).
 *
 * Conventions
 *   - every function returns 0 on success or a negative rc_status; the message is
 *     available through rc_last_error(); nothing aborts or throws across the ABI;
 *   - all ray / random / output buffers are DEVICE pointers owned by the caller
 *     (float32, row-major, leading dimension = rays); the handle owns its weight
 *     copies and its workspace; after the first call at a given n_rays no allocation
 *     happens inside rc_render_rays;
 *   - work is enqueued asynchronously on the caller's stream (mirrors pmap's async
 *     dispatch, internal/train_utils.py:3821-3830); synchronisation is the caller's;
 *   - a handle is bound to one device and is not thread-safe.
 */
#ifndef RC_ABI_H_
#define RC_ABI_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RC_ABI_VERSION 5
#define RC_MAX_LEVELS 3

typedef struct rc_handle rc_handle;

typedef enum {
  RC_OK = 0,
  RC_ERR_INVALID_ARG = -1,
  RC_ERR_HIP = -2,
  RC_ERR_MISSING_WEIGHT = -3,
  RC_ERR_SHAPE = -4,
  RC_ERR_UNSUPPORTED = -5,
  RC_ERR_NO_DEVICE = -6,
  RC_ERR_HOST = -7             /* a C++ exception (e.g. std::bad_alloc) caught at the boundary */
} rc_status;

/* One multiresolution dense+hash encoding.
 * Replaces HashEncoding's constructor fields (internal/grid_utils.py:739-805). */
typedef struct {
  int32_t hash_map_size;       /* T */
  int32_t max_grid_size;       /* N_max */
  int32_t min_grid_size;       /* N_min */
  int32_t num_features;        /* F: 1 or 4 */
  float bbox;                  /* bbox_scaling: cube [-bbox, bbox]^3 */
  float precondition_scaling;  /* x10 */
} rc_grid_config;

/* Resolved render-time configuration (the values the reference takes from its gin
 * chain; field provenance is listed in neural-radiance-caching_amd/config.py). */
typedef struct {
  uint32_t abi_version;        /* must be RC_ABI_VERSION */
  int32_t num_levels;          /* proposal rounds (3) */
  int32_t num_samples[RC_MAX_LEVELS];      /* (64, 64, 32): sampling_strategy, internal/sampling.py:53 */
  rc_grid_config proposal_grids[RC_MAX_LEVELS];
  rc_grid_config appearance_grid;
  rc_grid_config material_grid;
  rc_grid_config light_grid;
  float anneal;                /* sampling.py:326-339 */
  float resample_padding;
  float raydist_p;             /* power_ladder p (secondary rays) */
  float raydist_premult;
  float shadow_normal_eps_dot_min;
  float density_bias;          /* geometry.py:320 */
  float contract_radius;       /* coord.contract_radius_2 */
  float roughness_bias;
  float irradiance_bias;
  float ambient_irradiance_bias;
  float rgb_max;
  float slf_ambient_bias;
  float env_rgb_bias;
  float env_map_distance;
  float bg_intensity;          /* VolumeIntegrator.bg_intensity_range (equal ends) */
  float percentiles[3];        /* (5, 50, 95) */
  int32_t num_resample;        /* 1 */
  /* material stage */
  float diffuse_sample_fraction; /* MaterialMLP.diffuse_sample_fraction (0.5) */
  float secondary_normal_eps;    /* Config.secondary_normal_eps (1e-2) */
  float secondary_near;          /* MaterialMLP.near_min (5e-2) */
  float secondary_far;           /* Config.secondary_far (2) */
  float min_roughness;           /* 0.01 */
  float default_F_0;             /* 0.04 */
  float vmf_scale;               /* LightMLP.vmf_scale (20) */
  int32_t num_vmf;               /* LightMLP.num_components (128) */
} rc_config;

/* One named parameter tensor.  `name` is the Flax tree path
 * ("params/Cache/Sampler/MLP_0/density_grid/grid_016", ".../density_layers_0/kernel", ...),
 * i.e. what flax.training.checkpoints stores (internal/train_utils.py:4035-4088).
 * Dense kernels are [in, out]. */
typedef struct {
  const char* name;
  const void* data;            /* float32, contiguous */
  int32_t ndim;
  int64_t shape[4];
  int32_t on_device;           /* 0: host pointer, 1: device pointer */
} rc_tensor_desc;

/* Ray batch: the fields of utils.Rays (internal/utils.py:142-169) that the path reads. */
typedef struct {
  const float* origins;        /* [n,3] */
  const float* directions;     /* [n,3] */
  const float* viewdirs;       /* [n,3] */
  const float* near;           /* [n]   */
  const float* far;            /* [n]   */
  const float* lights;         /* [n,3] (light_dists extra) */
  const float* normals;        /* [n,3] or NULL; secondary rays only (sampling.py:182-205) */
} rc_rays;

/* Explicit random inputs standing in for jax.random (threefry is not reproduced).
 * A NULL rc_randoms*, or a NULL member, selects the reference's rng=None branch. */
typedef struct {
  const float* jitter[RC_MAX_LEVELS]; /* [n] U[0,1) per level: stepfun.sample single_jitter (stepfun.py:197-202) */
  const float* gumbel;                /* [n, S_last] standard Gumbel: jax.random.categorical (models.py:242-247) */
  const int32_t* resample_inds;       /* [n] optional: overrides the categorical draw (filtered_sampler_inds) */
} rc_randoms;

/* pass_mask bits */
#define RC_PASS_CACHE      0x1u   /* cache-only forward (BaseNeRFModel.__call__, internal/models.py:657-774) */
#define RC_PASS_SECONDARY  0x2u   /* is_secondary=True: far clamp, power-ladder distances, bg 0, resample, EnvMap */
#define RC_PASS_RESAMPLE   0x4u   /* force categorical resampling to num_resample samples (models.py:193-292) */
#define RC_PASS_NO_ENVMAP  0x8u   /* use_env_map=False for secondary rays (material.py:2191-2217) */
#define RC_PASS_ENV_IMAGE  0x10u  /* with RC_PASS_SECONDARY: the composite's EnvMap is the image bound by rc_set_env_image, looked up at
                                     rays->viewdirs (Model._handle_env_map with env_map=, models.py:382-393); no image bound:
                                     RC_ERR_INVALID_ARG.  Ignored with RC_PASS_NO_ENVMAP (use_env_map=False wins) */

/* Output slots: keys of the reference's `render` dict (integrator results,
 * internal/render.py:172-247, internal/integration.py:199-231, internal/models.py:2087-2158).
 * The `cache_<k>` keys of _finalize_outputs are aliases of these and are produced by the
 * host layer, not by extra device buffers. */
typedef enum {
  RC_OUT_RGB = 0,               /* [n,3] */
  RC_OUT_ACC,                   /* [n]   */
  RC_OUT_DISTANCE_MEAN,         /* [n]   */
  RC_OUT_DISTANCE_PERCENTILE_5, /* [n]   */
  RC_OUT_DISTANCE_MEDIAN,       /* [n]   */
  RC_OUT_DISTANCE_PERCENTILE_95,/* [n]   */
  RC_OUT_DIFFUSE_RGB,           /* [n,3] */
  RC_OUT_SPECULAR_RGB,
  RC_OUT_DIRECT_RGB,            /* == ambient_rgb == direct_diffuse_rgb == ambient_diffuse_rgb (+ exact 0) */
  RC_OUT_INDIRECT_RGB,
  RC_OUT_ALBEDO_RGB,
  RC_OUT_INDIRECT_DIFFUSE_RGB,
  RC_OUT_INDIRECT_SPECULAR_RGB,
  RC_OUT_INDIRECT_OCC,          /* [n,3] */
  RC_OUT_MEANS,                 /* [n,3] */
  RC_OUT_NORMALS,               /* [n,3] analytic (density gradient) */
  RC_OUT_NORMALS_PRED,          /* [n,3] == normals_to_use */
  RC_OUT_RAY_DISTS,             /* [n]   */
  RC_OUT_LIGHT_DISTS,           /* [n]   */
  RC_OUT_ENV_MAP_RGB,           /* [n,3] secondary rays only */
  RC_OUT_RGB_NO_ENV,            /* [n,3] secondary: rgb before the EnvMap composite (rgb_no_stopgrad - env) */
  RC_OUT_COUNT
} rc_output_id;

typedef struct {
  float* ptr[RC_OUT_COUNT];    /* device pointers; NULL = not requested */
} rc_outputs;

/* ---- material stage (config 3): BaseMaterialModel.__call__ with use_material / use_light_sampler
 * (internal/models.py:1144-1254, 1398-1694).  Explicit random inputs for everything the reference
 * draws with jax.random on that path.  Member sizes: Ks = round(K (1 - diffuse_fraction)), Kd = round(K diffuse_fraction),
 * Kc = round(Kd / 2), Kl = Kd - Kc, every round() Python's (half to even: K = 10 at 0.5 gives Kd = 5, Kc = 2, Kl = 3), as
 * rc_material_randoms_plan sizes them.  A K whose Ks + Kd != K (K = 5 at 0.5) is refused with RC_ERR_UNSUPPORTED. */
typedef struct {
  const float* gumbel;            /* [n, S_last]  categorical pick of the shading sample (models.py:1418-1438) */
  const float* vmf_noise;         /* [n, 128, 3]  N(0,1): LightMLP.get_vmfs means_random (light_sampler.py:142-144) */
  const float* spec_u1;           /* [n, Ks]      RandomGenerator2D.sample for the GGX sampler (render_utils.py:322-352) */
  const float* spec_u2;           /* [n, Ks] */
  const float* cos_u1;            /* [n, Kc]      ... for the cosine sampler */
  const float* cos_u2;            /* [n, Kc] */
  const int32_t* vmf_lobe;        /* [n]          categorical lobe pick of sample_vmf_vars (render_utils.py:1360-1372) */
  const float* vmf_v;             /* [n, Kd-Kc, 2] N(0,1) (render_utils.py:1409-1410) */
  const float* vmf_tmp;           /* [n, Kd-Kc]   U[0,1) (render_utils.py:1413) */
  const float* sec_jitter[RC_MAX_LEVELS];  /* [n*(Ks+Kd)] per level: jitter of the secondary rays, block [n*Ks | n*Kd] */
  const float* sec_gumbel;        /* [n*(Ks+Kd), S_last] */
  /* optional (NULL: draw from the Gumbel noise above): the categorical picks themselves, as rc_randoms.resample_inds
   * does for rc_render_rays -- filtered_sampler_inds of the primary rays (models.py:1418-1438) and of the batched
   * secondary trace (material.py:2191-2217 -> models.py:193-292).  With both given the noise members may be NULL. */
  const int32_t* resample_inds;     /* [n]          */
  const int32_t* sec_resample_inds; /* [n*(Ks+Kd)]  block [n*Ks | n*Kd] like sec_jitter */
  /* optional, instead of vmf_lobe (then NULL): standard Gumbel noise [n, 128]; the lobe is drawn on the device as
   * argmax_j(logit_j + g_j), which is jax.random.categorical(key, logits) of sample_vmf_vars (render_utils.py:1357-1372)
   * when g = jax.random.gumbel(key, [n, 128]) */
  const float* vmf_lobe_gumbel;
} rc_material_randoms;

typedef enum {
  RC_MOUT_RGB = 0,                 /* [n,3] material_rgb */
  RC_MOUT_ACC,                     /* [n]   */
  RC_MOUT_DIRECT_RGB, RC_MOUT_INDIRECT_RGB, RC_MOUT_DIFFUSE_RGB, RC_MOUT_SPECULAR_RGB,
  RC_MOUT_DIRECT_DIFFUSE_RGB, RC_MOUT_DIRECT_SPECULAR_RGB, RC_MOUT_INDIRECT_DIFFUSE_RGB,
  RC_MOUT_INDIRECT_SPECULAR_RGB,   /* [n,3] each */
  RC_MOUT_INDIRECT_OCC,            /* [n]   */
  RC_MOUT_LIGHTING_IRRADIANCE,     /* [n,3] */
  RC_MOUT_MATERIAL_ALBEDO,         /* [n,3] composited over all samples (models.py:1845-1912) */
  RC_MOUT_MATERIAL_ROUGHNESS,      /* [n]   */
  RC_MOUT_MATERIAL_METALNESS,      /* [n]   */
  RC_MOUT_MATERIAL_F_0,            /* [n]   */
  RC_MOUT_MEANS,                   /* [n,3] of the filtered sample */
  RC_MOUT_NORMALS_TO_USE,          /* [n,3] */
  RC_MOUT_RAY_DISTS,               /* [n]   */
  RC_MOUT_LIGHT_DISTS,             /* [n]   */
  RC_MOUT_COUNT
} rc_mat_output_id;

typedef struct {
  float* ptr[RC_MOUT_COUNT];
} rc_mat_outputs;

/* -- lifecycle: replaces models.construct_model / model.init (internal/models.py:2323-2358) */
int rc_create(const rc_config* cfg, int device, rc_handle** out);
void rc_destroy(rc_handle* h);
const char* rc_last_error(const rc_handle* h);   /* h may be NULL: last error of rc_create */
int rc_abi_version(void);
/* Arithmetic of the shader / EnvMap MLP layers this library was built with (csrc/rc_pack_host.h RC_SPLIT_MFMA):
 * 0 = fp32 MFMA (v_mfma_f32_32x32x2_f32, the exact fp32 chain); 1 = every fp32 operand split exactly into three bf16
 * pieces, six products per 16 k on v_mfma_f32_32x32x16_bf16, fp32 accumulation (same error against fp64 as the fp32 chain:
 * tests/test_gpu_parity.py, the noise-floor test).  The density MLPs of the proposal levels are fp32 MFMA in both. */
int rc_mlp_arithmetic(void);

/* -- weights: replaces flax `variables` passed to model.apply (internal/train_utils.py:3796-3814)
 * May be called several times; tensors with unknown names are rejected.
 * Ordering contract: the copies are blocking hipMemcpy calls on the null stream.  Device-resident sources
 * (on_device = 1) must be complete when the call is made -- work still running on a non-blocking stream is not
 * waited for; synchronise that stream (or the device) first, as the Python binding does.  The call returns after
 * the copies have finished, and later render calls on any stream see the new weights. */
int rc_load_weights(rc_handle* h, const rc_tensor_desc* descs, int32_t n);

/* -- the hot path: replaces model.apply(variables, rng, rays, ...)["render"] for the cache stage
 * (BaseMaterialModel.__call__ -> BaseNeRFModel.__call__, internal/models.py:1144-1254, 657-774). */
int rc_render_rays(rc_handle* h, const rc_rays* rays, int64_t n_rays, const rc_randoms* rnd,
                   uint32_t pass_mask, const rc_outputs* out, void* stream);

/* -- the chunk loop of models.render_image (internal/models.py:2412-2514) for passes that need no random inputs:
 * n_chunks consecutive batches of `chunk` rays out of the arrays `rays` points to (the caller has edge-padded the last
 * one: utils.shard / np.pad(mode="edge"), internal/utils.py:333-343, models.py:2437-2441), chunk i enqueued on
 * streams[i % n_streams] with its outputs at out0->ptr[k] + i * out_stride floats (k over the requested outputs).
 * Exactly n_chunks calls of rc_render_rays(rnd = NULL) -- same kernels, same results, same stream semantics per chunk --
 * without a trip through the caller's language per chunk.  (ABI v4.) */
int rc_render_chunks(rc_handle* h, const rc_rays* rays, int64_t chunk, int64_t n_chunks, uint32_t pass_mask,
                     const rc_outputs* out0, int64_t out_stride, void* const* streams, int32_t n_streams);

/* -- model.apply(..., passes=("cache","light","material")) for the material stage: the cache pass on the
 * primary rays (-> cache_out, the `cache_<k>` keys), one resampled shading point per ray, light sampler,
 * BRDF importance sampling of K secondary rays per point, ONE batched secondary trace of n*K rays through
 * the same cache kernels (is_secondary, resample, no env map) + the model-level EnvMap along the same
 * rays, Monte-Carlo BRDF integration and the MaterialIntegrator composite (-> mat_out).
 * rnd->jitter[] drives the primary rays (NULL: deterministic branch).
 * Stream semantics: the call is ordered on `stream` like every other entry point.  Inside it, work the secondary
 * trace does not wait for (light sampler, material-only composite, EnvMap) runs on a stream the handle owns, forked
 * from and joined back to `stream` with events before the call's last kernel: nothing for the caller to synchronise. */
int rc_render_material(rc_handle* h, const rc_rays* rays, int64_t n_rays, const rc_randoms* rnd,
                       const rc_material_randoms* mrnd, int32_t num_secondary_samples,
                       const rc_outputs* cache_out, const rc_mat_outputs* mat_out, void* stream);

/* -- the all-gather of the rendered pixels across the GPUs of one node: replaces
 * jax.lax.all_gather(render_dict, axis_name="batch") inside render_eval_fn (internal/train_utils.py:3795-3815) for a
 * host that drives RCCL itself (the Python host layer uses torch.distributed instead).
 *   nccl_comm   an ncclComm_t of the caller (one rank per GPU, this handle's device), passed as void*
 *   local       this rank's outputs, n_local rays each ([n_local,3] / [n_local] per slot)
 *   full        [world * n_local, .] per slot; only slots non-NULL in BOTH structs are gathered
 * Every rank must pass the same n_local and the same slot set (pad the last shard, as models.render_image pads its
 * last chunk).  All slots go out as ONE grouped collective (ncclGroupStart/End) on `stream`, asynchronously.
 * RCCL is resolved at run time from the library the process has already loaded (librccl.so, else RC_RCCL_LIBRARY):
 * the comm and the calls then belong to the same RCCL instance.  RC_ERR_UNSUPPORTED when no RCCL can be found. */
int rc_allgather_outputs(rc_handle* h, void* nccl_comm, const rc_outputs* local, int64_t n_local, const rc_outputs* full,
                         void* stream);

/* -- single operators on the path (used by the parity tests and by the roofline bench)
 * HashEncoding.__call__ incl. the contraction (internal/grid_utils.py:808-905, coord.py:37-69):
 * grid_id: 0..2 proposal density grids, 3 appearance, 4 material, 5 light.
 * points [n,3] world coordinates; features_out [n, L*F] row-major. */
int rc_hashgrid_lookup(rc_handle* h, int32_t grid_id, const float* points, int64_t n,
                       float* features_out, int32_t apply_contraction, void* stream);
/* stepfun.sample_intervals (internal/stepfun.py:207-250): t [n,P+1], logits [n,P] -> out [n,S+1];
 * jitter [n] U[0,1) or NULL. */
int rc_sample_intervals(rc_handle* h, const float* t, const float* logits, int64_t n, int32_t num_bins,
                        int32_t num_samples, const float* jitter, float* out, void* stream);

/* -- introspection for tests / profiling: a named workspace buffer as the last call that used its set left it.
 * name = [prefix]<buffer>.  Prefix: none = set 0 (rc_render_rays on the first caller stream, rc_render_material,
 * rc_render_transient), "p1:" .. "p3:" = the sets of rc_render_rays on further caller streams, "s:" = the batched
 * secondary trace of rc_render_material / the shadow rays of rc_render_transient, "t:" = rc_density_backward,
 * "i:" = rc_interlevel_backward, "d:" = rc_data_backward, "g:" = rc_geometry_backward / rc_density_regularizer,
 * "o:" = rc_adam_update / rc_load_params_flat, "ls:" = rc_light_sampling_backward / rc_light_regularizer,
 * "ms:" = rc_material_smoothness_backward / rc_material_regularizer, "md:" = rc_material_data_backward / rc_material_data_backward_env,
 * "td:" = rc_transient_data_backward, "mk:" = rc_mask_backward, "nb:" = rc_normals_backward,
 * "gs:" = rc_geometry_smoothness_backward, "q:" = rc_query_points / rc_density_lattice, "iso:" = rc_isosurface,
 * "atlas:" = rc_query_cache_diffuse / rc_bake_atlas (their buffers are listed at those calls).
 * Buffers of the render sets (no prefix, "p1:" .. "p3:", "s:"): per level, with the level 0 .. num_levels-1 appended,
 * "sdist", "tdist", "means", "feat", "density", "weights" (e.g. "sdist0", "weights2"); "hbuf", "normals_pred",
 * "normals_grad", "jac", "app", "shade", "debug", "env_rgb", "rgb_noenv", "acc_ws", "inds", "src_idx", "filt_weight",
 * "acc_sel", "feat_sel", "hbuf_sel", "normals_sel", "density_sel"; "t_irr", "t_slf", "tshade" (set 0 of a time-resolved
 * handle).  Set 0 only: "m_*", "l_*", "sec_*" (rc_render_material), "sh_*" (rc_render_transient with occlusions).
 * "t:": "feat", "dfeat", "a1", "a2", "d1", "d2", "fe", "graw", "density", "partial".
 * "i:": the training forward's per-level "sdist", "tdist", "means", "feat", "density", "weights" (levels 0 .. num_levels-1,
 * as above), and per proposal level 0 .. num_levels-2 "d_density" (d loss / d density, [n][S]) and "points" (the
 * means as [n S][3], the points of that level's density backward); "loss_ray" ([num_levels-1][n] per-ray sums).
 * "d:": the training forward's buffers (the render-set names above) and "rgb" ([n][3] ray colour), "loss_ray" ([n]),
 * "d_density" ([n S]), "d_rgbs" ([n S][3]), "points" ([n S][3]); of the last sample chunk of the shader backward
 * (row-major per sample): "f96", "heads", "p3" (pred_raw), "ib_in", "x328", "s0", "s1", "sb", "i1", "i2", "io", "so", their
 * gradients "dheads", "dio", "dso", "dsb", "dx328", "ds1", "ds0", "di2", "di1", "dib_in", "db128", "dp3", "df96", and
 * "dfeat" ([C][64] d loss / d feature64), "dapp" ([C][32]), "part", "ones".
 * "g:": the training forward's buffers (the render-set names above; the last level's "weights" written by the loss kernel, "hbuf", "normals_pred",
 * "normals_grad", "jac" included) and "loss_ray" ([4][n] per-ray values of the four terms), "d_density" ([n S]),
 * "d_pred" ([n S][3] d loss / d pred_raw), "points" ([n S][3]); of the last sample chunk: "h64" ([C][64] hidden vectors in
 * the reference's column order), "dfeat" ([C][64] d loss / d feature64), "part", "ones"; rc_density_regularizer's
 * "reg_part" (per-table partial sums, doubles).
 * "o:": "part" (per-tile sums of g^2 of the norm clip, doubles), "norm" ([1] the global norm), "mult" ([1] the clip
 * multiplier), "stage" (the dense segments of rc_load_params_flat gathered when they are not contiguous).
 * "ls:": "cache_rgb" ([n][3]), "cache_acc" ([n]) (the primary pass's composite, not read), "h0", "h1" ([n][64] the light
 * head's hidden layers, recomputed), "vp" ([n][640] its vmf_params), "dvp" ([n][640] d loss / d vmf_params), "dh1",
 * "dh0" ([n][64]), "dfeat" ([n][32] d loss / d light-grid features), "loss_ray" ([n] per-ray sums), "part" (weight-gradient
 * K slices), "ones", "reg_part" (rc_light_regularizer's per-table partial sums, doubles).  The forward's own buffers
 * keep their set-0 / "s:" names ("m_pts", "m_nrm", "l_feat", "l_vmf", "l_vmf_logit", "sec_dirs", "sec_samples", "sec_rgb").
 * "ms:": "cache_rgb" ([n][3]), "cache_acc" ([n]) (the primary pass's composite, not read), "pts" ([2n][3] the shading
 * points x, then x' = x + noise_scale nu), "feat" ([2n][32] their material-grid features),
 * "mat_p" ([n][5] the material at x', before nan_to_num), "loss_ray" ([n] per-point sums), "loss_part" (per-workgroup
 * loss sums, doubles), "dfeat" ([2n][32] d loss / d features), "part" (per-workgroup partials of the dense layers'
 * gradients), "reg_part" (rc_material_regularizer's per-table partial sums, doubles).  The forward's own buffers keep
 * their set-0 names ("m_pts", "m_nrm", "m_mat", "filt_weight").
 * "td:": "rgb" ([n][700][3] the rendered histograms), "G" ([n][700][3] d loss / d rgb), "Gt" ([n][700][3] the temporal
 * filter's transpose applied to G: d loss / d the unfiltered direct histogram), "loss_ray" ([2][n] per-ray sums of the loss
 * terms, then of lossmult (rgb - gt)^2); of the last chunk of C <= 256 rays of the heads' backward: "dz_irr" ([32 C][2100]
 * d loss / d transient_indirect_layer's output), "dz_slf" ([32 C][2104] d loss / d output_rgba_layer's output, the alpha
 * column and three pad floats zero), "x_irr" ([32 C][64]), "x_slf" ([32 C][128]) (the heads' inputs, row-major in the
 * reference's column order), "part" (weight-gradient K slices), "ones"; for all n rays, row-major per shaded sample in the
 * reference's column order: "d_t_irr" ([32 n][64] d loss / d the irradiance trunk's output), "d_t_slf" ([32 n][128] d loss /
 * d the surface light field trunk's output), "d_tint_ibrdf" ([32 n][3]), "d_direct" ([32 n][3] d loss / d direct_rgb),
 * "d_weights" ([32 n] d loss / d the compositing weights); after rc_transient_data_backward_sampler with sampler_grads also
 * "d_density" ([32 n] d loss / d the last level's density through those weights) and "points" ([32 n][3] the sample means).
 * The forward's own buffers keep their set-0 names ("t_irr", "t_slf", "tshade", "weights2").
 * "mk:" = rc_mask_backward: the training forward's per-level "sdist", "tdist", "means", "feat", "density", "weights" (the
 * last level's "weights" written by the loss kernel), "loss_ray" ([n] per-ray terms), "d_density" ([n S]), "points"
 * ([n S][3]).
 * Returns RC_ERR_INVALID_ARG for an unknown name or a buffer no call has allocated yet.
 * count = number of float32 (or int32) elements of the last request. */
int rc_workspace_ptr(rc_handle* h, const char* name, void** ptr, int64_t* count);
/* Per-stage device time (ms, hipEvents recorded on the launch stream), averaged over the calls
 * issued since profiling was last (re)enabled (ring of 16).  mode 0 off, 1 every stage,
 * 2 only the dominant kernel (cache shader / the fused kernel; two events per call), 3 like 2 on every 8th call
 * (the last 16 sampled calls span 128 calls; an event record costs ~1.3 us of stream time).  Profiled calls launch eagerly. */
int rc_set_profiling(rc_handle* h, int32_t mode);
/* Launch mode of rc_render_rays: 0 = eager kernel launches, 1 = capture a hipGraph the second time
 * an identical call (same sizes and pointers) is seen and replay it afterwards (default),
 * 2 = capture on first sight.  Applies to the launch-per-stage plan; the one-launch fused plan (rc_set_fused) is always
 * launched plainly (a one-node graph replays with a larger gap between launches than a plain launch). */
int rc_set_graph_mode(rc_handle* h, int32_t mode);
/* Kernel plan.  1 (default): the plain cache pass (pass_mask == RC_PASS_CACHE) is one fused launch per batch, all
 * intermediates on chip (no workspace: rc_workspace_ptr then has nothing to show) -- TWO wavefronts per ray in 4-wave
 * workgroups of two rays, two workgroups per CU (csrc/rc_fused2.hip); every other pass runs one launch per stage, where
 * a proposal level whose samples only hand their density on is ONE launch (grid lookup + density MLP, weights resident
 * in LDS; from 24 576 rays on also the level's sampling, one ray per wave), and rc_render_material renders its primary
 * rays with the fused launch (one wavefront per ray, per-sample results exported).  3: like 1 with the plain cache pass
 * on the one-wavefront-per-ray form of the fused kernel (csrc/rc_fused.hip, the round-1/2 kernel).  2: like 1 with the
 * plain cache pass on the launch-per-stage plan too and the sampling always in its own kernel.  0: the plain
 * launch-per-stage plan everywhere, grid lookup and density MLP as separate kernels (materialises
 * sdist/tdist/means/features/density/weights per level in the workspace).  All plans evaluate the same arithmetic in
 * the same order: results are bitwise equal
 * (internal/models.py:1237-1386 / sampling.py:155-353 / nerf.py:426-693). */
int rc_set_fused(rc_handle* h, int32_t mode);
int rc_stage_count(void);
const char* rc_stage_name(int32_t stage);
int rc_stage_times_ms(rc_handle* h, float* out_ms, int32_t n);

/* ------------------------------------------------------------------------------------------------
 * Time-resolved cache (BASELINE configs[4]): TransientNeRFModel.__call__ for primary rays
 * (internal/models.py:912-985 over BaseNeRFModel.__call__ :657-774) = ProposalVolumeSampler ->
 * TransientNeRFMLP (internal/nerf.py:561-938, 1656-1797) -> TransientVolumeIntegrator
 * (internal/integration.py:343-551, internal/render.py:250-507).
 * ------------------------------------------------------------------------------------------------ */
typedef struct rc_transient_config {
  int32_t n_bins;                   /* Config.n_bins (700 is the only compiled size)                   */
  float exposure_time;              /* Config.exposure_time                                             */
  float tfilter_sigma;              /* Config.tfilter_sigma (0: no temporal filter)                     */
  float transient_shift;            /* Config.transient_shift                                           */
  int32_t bin_zero_threshold_light; /* Config.bin_zero_threshold_light                                  */
  float light_near;                 /* Config.light_near                                                */
  int32_t light_zero;               /* Config.light_zero                                                */
  int32_t use_falloff;              /* Config.use_falloff                                               */
  float indirect_scale;             /* TransientNeRFMLP.indirect_scale                                  */
  float rgb_max;                    /* TransientNeRFMLP.rgb_max                                         */
  float albedo_bias;                /* TransientNeRFMLP.albedo_bias (activation softplus)               */
  float brdf_bias;                  /* BaseNeRFMLP.brdf_bias                                            */
  float irradiance_bias;            /* TransientNeRFMLP.irradiance_bias                                 */
  float slf_rgb_bias;               /* TransientSurfaceLightFieldMLP.rgb_bias                           */
  int32_t use_occlusions;           /* Config.use_occlusions for every ray (the Trainer's vis_only override,
                                       engine/trainer.py:198-202): one weights-only shadow ray per shaded
                                       sample through the cache (internal/nerf.py:1193-1342)              */
  float occ_threshold;              /* Config.occ_threshold_min (== _max)                               */
  float shadow_near;                /* Config.shadow_near_min (== _max)                                 */
  float shadow_far;                 /* Config.secondary_far                                             */
  int32_t reserved[6];
} rc_transient_config;

/* Switches a freshly created handle to the transient model: rc_load_weights then expects the
 * TransientNeRFMLP inventory (direct_tint_layer, albedo_layer, brdf_layers_*, irradiance_layers_*,
 * transient_indirect_layer, light_power, SurfaceLightField with lights and 3 n_bins + 1 outputs) and
 * rc_render_transient becomes available (rc_render_rays / rc_render_material are then refused). */
int rc_set_transient(rc_handle* h, const rc_transient_config* t);

typedef enum rc_transient_output_id {
  RC_TOUT_RGB = 0,                 /* [n, n_bins, 3]  transient_direct (filtered) + transient_indirect   */
  RC_TOUT_TRANSIENT_DIRECT_VIZ,    /* [n, n_bins, 3]                                                     */
  RC_TOUT_TRANSIENT_INDIRECT_VIZ,  /* [n, n_bins, 3]  (= the reference's final "transient_indirect")     */
  RC_TOUT_TRANSIENT_INDIRECT_DIFFUSE,   /* [n, n_bins, 3] unshifted composite (integration.py extras)    */
  RC_TOUT_TRANSIENT_INDIRECT_SPECULAR,  /* [n, n_bins, 3]                                                */
  RC_TOUT_INTEGRATED_RGB,          /* [n, 3] sum of RGB over bins                                        */
  RC_TOUT_DIRECT_RGB, RC_TOUT_INDIRECT_RGB,
  RC_TOUT_DIFFUSE_RGB, RC_TOUT_SPECULAR_RGB, RC_TOUT_ALBEDO_RGB, RC_TOUT_OCC, RC_TOUT_INDIRECT_OCC,
  RC_TOUT_IRRADIANCE_RGB, RC_TOUT_LIGHT_RADIANCE_RGB, RC_TOUT_N_DOT_L_RGB, RC_TOUT_DIRECT_DIFFUSE_RGB,
  RC_TOUT_DIRECT_SPECULAR_RGB, RC_TOUT_INDIRECT_DIFFUSE_RGB, RC_TOUT_INDIRECT_SPECULAR_RGB,
  RC_TOUT_DIRECT_RGB_VIZ,          /* [n, 3] each                                                        */
  RC_TOUT_ACC, RC_TOUT_DISTANCE_MEAN, RC_TOUT_DISTANCE_MEDIAN, RC_TOUT_DISTANCE_PERCENTILE_5,
  RC_TOUT_DISTANCE_PERCENTILE_95,  /* [n]                                                                */
  RC_TOUT_MEANS, RC_TOUT_NORMALS, RC_TOUT_NORMALS_PRED,   /* [n, 3]                                       */
  RC_TOUT_RAY_DISTS, RC_TOUT_LIGHT_DISTS,                 /* [n]                                          */
  RC_TOUT_COUNT
} rc_transient_output_id;
typedef struct rc_transient_outputs { float* ptr[RC_TOUT_COUNT]; } rc_transient_outputs;   /* NULL = not wanted */

/* rays->lights is required; cam_origins [n,3] is the camera centre of each ray (Rays.cam_origins,
 * internal/inverse_render/render_utils.py:1733-1740).  Direct-light bins beyond n_bins spill into the
 * next ray of THIS call's batch exactly as the reference's flattened scatter does (internal/render.py:447-475).
 * shadow_rnd (use_occlusions only): per-level jitter of the n * 32 shadow rays, NULL = deterministic branch. */
int rc_render_transient(rc_handle* h, const rc_rays* rays, const float* cam_origins, int64_t n, const rc_randoms* rnd,
                        const rc_randoms* shadow_rnd, const rc_transient_outputs* out, void* stream);

/* Time slices of the histograms (the trainer's light-in-flight frames, engine/trainer.py:1693-1726) without the
 * histograms: for every ray and every time t the value  w * v[ceil t] + (1 - w) * v[floor t],  w = t - floor t,  of
 * v = rgb / the filtered direct part / the indirect part, computed from the bins that reach floor t and ceil t only
 * (DESIGN.md section 4.22).  Same contract as rc_render_transient: same rays (lights and cam_origins required), same
 * randoms, same workspace set, use_occlusions handles included; the direct part spills into the next ray of the batch in
 * the same way.  `extra` (nullable) may ask for the outputs of the steady-state composite -- RC_TOUT_ACC, the four
 * RC_TOUT_DISTANCE_*, MEANS, NORMALS, NORMALS_PRED, RAY_DISTS, LIGHT_DISTS; any other non-NULL pointer of it needs every
 * bin and returns RC_ERR_UNSUPPORTED.  Each call repeats the whole trace up to the per-bin heads. */
#define RC_TSLICE_MAX 8
typedef struct rc_transient_slices {
  int32_t count;                 /* 1 .. RC_TSLICE_MAX */
  float t[RC_TSLICE_MAX];        /* fractional bin index, 0 <= t <= n_bins - 1 */
  float* rgb; float* direct; float* indirect;   /* device, [n][count][3]; NULL = not wanted, at least one set */
} rc_transient_slices;
int rc_render_transient_slices(rc_handle* h, const rc_rays* rays, const float* cam_origins, int64_t n, const rc_randoms* rnd,
                               const rc_randoms* shadow_rnd, const rc_transient_slices* s,
                               const rc_transient_outputs* extra /* nullable */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * On-device ray generation: camera_utils.pixels_to_rays + cast_ray_batch
 * (internal/camera_utils.py:896-1072, 1225-1329) for one camera: ProjectionType.PERSPECTIVE / FISHEYE /
 * FISHEYE_EQUISOLID / PANORAMIC, optional radial + tangential distortion (:795-890, Newton undistortion, 10 steps),
 * optional NDC (convert_to_ndc, :50-111; radii then from the offsets between NDC origins, :1058-1066), optional
 * sub-pixel jitter offsets (:943-957, handed over as explicit random tensors like rc_randoms) and optional z_range
 * cropping (cast_ray_batch, :1291-1299; rays_planes_intersection, :1143-1164).  The outputs are the device arrays
 * rc_cast_outputs points to.
 * ------------------------------------------------------------------------------------------------ */
typedef struct rc_camera {
  float pixtocam[9];     /* inverse intrinsics, row-major [3,3] (camera_utils.get_pixtocam)              */
  float camtoworld[12];  /* extrinsics, row-major [3,4]                                                  */
  float light[3];        /* lights[cam_idx] (camera_utils.py:1288)                                       */
  float near, far;       /* Pixels.near / Pixels.far                                                     */
  int32_t camtype;       /* 0 ProjectionType.PERSPECTIVE, 1 PANORAMIC (cast_spherical_rays, camera_utils.py:1415-1443,
                          * 1013-1024: pixtocam = diag(2 pi / W, pi / H, 1), (theta, phi) -> direction),
                          * 2 FISHEYE (equidistant, theta = min(pi, r)), 3 FISHEYE_EQUISOLID (theta = 2 asin(r / 2)) (:991-1011) */
  /* -- ABI v3 -- */
  int32_t has_distortion;   /* distortion_params is not None (:981-989)                                  */
  float distortion[6];      /* k1, k2, k3, k4, p1, p2                                                    */
  int32_t has_ndc;          /* pixtocam_ndc is not None (:1052-1066)                                     */
  float pixtocam_ndc[9];    /* inverse intrinsics of the NDC projection, row-major [3,3]                 */
  /* -- ABI v4 -- */
  int32_t has_z_range;      /* z_range is not None: origins += directions * t_min, directions *= t_max - t_min for
                             * the slab z in [z_range[0], z_range[1]] (camera_utils.py:1291-1299)                 */
  float z_range[2];
  const float* pix_dx;      /* [n] device arrays or NULL (jitter = 0): the offsets pixels_to_rays adds to the pixel     */
  const float* pix_dy;      /* coordinates when jitter > 0 -- U(-0.5, 0.5) or N(0, 0.25), plus a second uniform when
                             * jitter_scale > 1 (:943-957); the caller draws them (rc_prng_fill + prng.py)         */
} rc_camera;
typedef struct rc_cast_outputs {
  float* origins; float* directions; float* viewdirs;   /* [n,3] */
  float* radii;                                         /* [n]   */
  float* imageplane;                                    /* [n,2] */
  float* look; float* up; float* lights;                /* [n,3] */
  float* near; float* far;                              /* [n]   */
} rc_cast_outputs;                                      /* NULL = not wanted */
/* pix_x / pix_y: int32 device arrays [n] (Pixels.pix_x_int / pix_y_int), or both NULL for the rectangle
 * [x0, x0 + width) x [y0, y0 + height) in row-major order (n = width * height). */
int rc_cast_rays(rc_handle* h, const rc_camera* cam, const int32_t* pix_x, const int32_t* pix_y, int64_t n,
                 int32_t x0, int32_t y0, int32_t width, int32_t height, const rc_cast_outputs* out, void* stream);

/* ---- rays of a batch that mixes cameras, and the training batch of one step ----------------
 * rc_camera_set: the reference's `cameras` tuple on the device -- per-camera tables, and what all cameras share
 * (camera_utils.cast_ray_batch reads pixtocams[cam_idx], camtoworlds[cam_idx], lights[cam_idx] per ray and ONE
 * camtype / distortion_params / pixtocam_ndc / z_range, internal/camera_utils.py:1266-1299).  The tables are
 * device arrays that stay valid until the call's work on `stream` is done; the shared fields mean what they mean in
 * rc_camera. */
typedef struct rc_camera_set {
  int32_t count;             /* C >= 1 cameras                                                             */
  const float* pixtocams;    /* [C, 9]  inverse intrinsics, row-major [3,3] each                           */
  const float* camtoworlds;  /* [C, 12] extrinsics, row-major [3,4] each                                   */
  const float* lights;       /* [C, 3]  lights[cam_idx], or NULL: the camera centre camtoworld[:3, 3]      */
  float near, far;
  int32_t camtype;
  int32_t has_distortion;
  float distortion[6];
  int32_t has_ndc;
  float pixtocam_ndc[9];
  int32_t has_z_range;
  float z_range[2];
  const float* pix_dx;       /* rc_train_batch only: [n] sub-pixel jitter offsets or NULL, as rc_camera.pix_dx / pix_dy; */
  const float* pix_dy;       /* rc_cast_rays_multi takes its own as arguments and does not read these      */
} rc_camera_set;

/* cast_ray_batch for pixels of several cameras in one launch; replaces a host loop of one rc_cast_rays per distinct
 * camera (camera_utils.py:1225-1329 with the per-ray lookup of :1266-1288).
 * cam_idx / pix_x / pix_y: int32 device arrays [n] (Pixels.cam_idx / pix_x_int / pix_y_int), all required.
 * cam_idx[i] must lie in [0, set->count): the kernel clamps it so that no table is read out of bounds, but a clamped
 * ray is the ray of the wrong camera -- a contract violation like a pix_x outside the image, not an error code.
 * pix_dx / pix_dy: [n] sub-pixel jitter offsets, both or neither.  Every output of ray i is bitwise what rc_cast_rays
 * writes for camera cam_idx[i] and that pixel.  n == 0 succeeds and launches nothing. */
int rc_cast_rays_multi(rc_handle* h, const rc_camera_set* set, const int32_t* cam_idx, const int32_t* pix_x,
                       const int32_t* pix_y, int64_t n, const float* pix_dx, const float* pix_dy,
                       const rc_cast_outputs* out, void* stream);

/* The batch of one train step from a PRNG key; replaces Dataset._next_train + _make_ray_batch for image-shaped data
 * (internal/datasets.py:948-993, 850-946) + cast_ray_batch.  n = P * patch_size^2 rays, ray i = pixel i % patch_size^2
 * (row-major in the patch, camera_utils.pixel_coordinates(p, p)) of patch i / patch_size^2.
 * Index rule (this package's own; the reference draws from numpy's global Mersenne Twister, datasets.py:969-981):
 * w = random_bits(key, (P, 3)) of jax's threefry2x32 (what rc_prng_fill(key, RC_PRNG_MODE_BITS, n = 3 P) holds); patch
 * q takes  cam = (w[q][0] * C) >> 32,  x0 = border + (w[q][1] * (W - 2 border - p + 1)) >> 32,  y0 likewise with H and
 * w[q][2], in 64-bit integers (bias <= range / 2^32).  batching RC_BATCHING_SINGLE_IMAGE: every patch takes the camera
 * of w[0][0] (datasets.py:981).
 * images: device [C, H, W, 3], RC_IMAGE_F32 float32 or RC_IMAGE_U8 uint8 (read as (float)u / 255.0f, an IEEE division).
 * cam_lossmult: device [C] or NULL (datasets.py:989-990; NULL: lossmult = 1).  key: host uint32[2].
 * Errors (nothing is launched): n != P p^2 for every P, i.e. n % p^2 != 0; count < 1; W - 2 border - p + 1 < 1 or the
 * same with H; a NULL table, image or key; 3 P >= 2^32 - 1.  n == 0 succeeds and launches nothing.
 * A NULL handle is an error as well, reported after the argument checks above (rc_last_error(NULL) has their text),
 * so that a host can validate a call's shape without a device. */
typedef enum rc_image_dtype { RC_IMAGE_F32 = 0, RC_IMAGE_U8 = 1 } rc_image_dtype;
typedef enum rc_batching { RC_BATCHING_ALL_IMAGES = 0, RC_BATCHING_SINGLE_IMAGE = 1 } rc_batching;
typedef struct rc_train_batch_outputs {
  rc_cast_outputs rays;      /* the rays of the n pixels                                                    */
  float* rgb;                /* [n,3] images[cam, y, x]                                                     */
  float* lossmult;           /* [n]                                                                         */
  int32_t* cam_idx;          /* [n]   the picks: camera, pixel column, pixel row                            */
  int32_t* pix_x;
  int32_t* pix_y;
} rc_train_batch_outputs;    /* NULL = not wanted */
int rc_train_batch(rc_handle* h, const rc_camera_set* set, const void* images, int32_t image_dtype, int32_t height,
                   int32_t width, const float* cam_lossmult, const uint32_t key[2], int32_t patch_size, int32_t border,
                   int32_t batching, int64_t n, const rc_train_batch_outputs* out_batch, void* stream);

/* ---- jax.random-compatible random tensors, generated in HBM ----------------------
 * Replaces the reference's jax.random.uniform / normal / categorical(gumbel) draws on the path
 * (internal/stepfun.py:200-202 per-ray jitter, internal/models.py:240-247 resampling noise,
 * internal/light_sampler.py:140-142 constant vMF mean noise) for the PRNG the reference pins (jax==0.4.16,
 * requirements.txt:2: threefry2x32, uint32[2] keys, non-partitionable counters).  Key derivation
 * (jax.random.split through internal/utils.py:118-123 random_split) is 2-4 blocks per call and stays on the host
 * (neural-radiance-caching_amd/prng.py).
 * out: device array of n 32-bit words -- uint32 for RC_PRNG_BITS, float otherwise; element i is what
 * jax.random.{bits,uniform,normal,gumbel}(key, (n,)) holds at i (any shape with n elements, row-major).
 * minval/maxval: uniform only (normal and gumbel use jax's own ranges). */
typedef enum rc_prng_mode { RC_PRNG_MODE_BITS = 0, RC_PRNG_MODE_UNIFORM = 1, RC_PRNG_MODE_NORMAL = 2,
                            RC_PRNG_MODE_GUMBEL = 3 } rc_prng_mode;
int rc_prng_fill(rc_handle* h, const uint32_t key[2], int32_t mode, float minval, float maxval, int64_t n, void* out,
                 void* stream);

/* ---- every random tensor of one material-stage forward from one key, in one launch ------------------------
 * rc_material_randoms_plan walks the reference's random_split sites of BaseMaterialModel.__call__ on the host (the tree
 * prng.material_stage_plan restates in Python; csrc/rc_prng_host.h is its C twin) and returns one rc_prng_segment per
 * jax.random draw: the key, the distribution, the element count and where the tensor lies in ONE arena of 32-bit words.
 * rc_prng_fill_segments fills the arena in one launch; every value is the rc_prng_fill of the same key, mode and count.
 * Needs no GPU and no handle.  Like every key path of the package the ORDER of the splits is restated from the source
 * and is not pinned against a jax run.
 *
 * The arena holds the members of rc_randoms / rc_material_randoms in the layout those structs take: sec_jitter[l] is one
 * block [n Ks | n Kd] (the specular and the diffuse trace's segments are adjacent), sec_gumbel one [n (Ks + Kd), S_last].
 * The two [m, 2] uniform draws of RandomGenerator2D.sample are split into their columns: even elements go to `offset`
 * (spec_u1 / cos_u1), odd ones to `offset2` (spec_u2 / cos_u2); everywhere else offset2 is -1.  Members start at
 * multiples of 64 words.  Sizes: Ks = round(K (1 - f)), Kd = round(K f), Kc = round(Kd / 2), Kl = Kd - Kc with Python's
 * round (half to even), the host twin's; a K with Ks + Kd != K is RC_ERR_UNSUPPORTED.  A member of zero elements (Kc = 0
 * at K = 2) keeps its segment, with n = 0.  The two RC_PRNG_MEMBER_PICKS_KEY_* rows of RC_PRNG_PLAN_ENV_SAMPLER carry a
 * key only (n = 0): the texel draws of rc_render_relight take keys, not tensors. */
typedef enum rc_prng_member {
  RC_PRNG_MEMBER_JITTER = 0,          /* + level: rc_randoms.jitter[level] [n]                                       */
  RC_PRNG_MEMBER_GUMBEL = 8,          /* rc_material_randoms.gumbel [n, S_last]                                      */
  RC_PRNG_MEMBER_VMF_NOISE = 9,       /* vmf_noise [n, num_vmf, 3]: the PRNGKey(1) constant, RC_PRNG_PLAN_VMF_NOISE  */
  RC_PRNG_MEMBER_SPEC_U = 10,         /* spec_u1 | spec_u2 [n, Ks] each (two planes)                                 */
  RC_PRNG_MEMBER_COS_U = 11,          /* cos_u1 | cos_u2 [n, Kc] each (two planes)                                   */
  RC_PRNG_MEMBER_VMF_LOBE_GUMBEL = 12,/* vmf_lobe_gumbel [n, num_vmf]                                                */
  RC_PRNG_MEMBER_VMF_V = 13,          /* vmf_v [n, Kl, 2], interleaved                                               */
  RC_PRNG_MEMBER_VMF_TMP = 14,        /* vmf_tmp [n, Kl]                                                             */
  RC_PRNG_MEMBER_SPEC_GUMBEL = 15,    /* sec_gumbel rows [0, n Ks)                                                   */
  RC_PRNG_MEMBER_DIFF_GUMBEL = 16,    /* sec_gumbel rows [n Ks, n (Ks + Kd))                                         */
  RC_PRNG_MEMBER_NOISE = 17,          /* rc_material_smoothness_backward's noise [n, 3] (loss_key given)             */
  RC_PRNG_MEMBER_PICKS_KEY_SPEC = 18, /* key of the specular leg's texel draw (n = 0)                                */
  RC_PRNG_MEMBER_PICKS_KEY_DIFF = 19,
  RC_PRNG_MEMBER_SPEC_JITTER = 24,    /* + level: sec_jitter[level] elements [0, n Ks)                               */
  RC_PRNG_MEMBER_DIFF_JITTER = 32     /* + level: sec_jitter[level] elements [n Ks, n (Ks + Kd))                     */
} rc_prng_member;

typedef struct {
  uint32_t key[2];
  int32_t mode;      /* rc_prng_mode */
  int32_t id;        /* rc_prng_member */
  float lo, hi;      /* RC_PRNG_MODE_UNIFORM's range (the other modes fix their own) */
  int64_t n;         /* elements of the tensor jax draws: the counters are cut at half = (n + 1) / 2, as in rc_prng_fill */
  int64_t offset;    /* word offset in the arena of element 0; two planes: of the even elements */
  int64_t offset2;   /* -1; two planes: word offset of the odd elements (element i lands at plane[i & 1][i >> 1]) */
} rc_prng_segment;

#define RC_PRNG_MAX_SEGMENTS 32
#define RC_PRNG_PLAN_TRAIN        0x1u   /* the secondary traces' sampler jitter from each trace's own key (train=True);
                                            otherwise from PRNGKey(0), internal/sampling.py:170-179 */
#define RC_PRNG_PLAN_ENV_SAMPLER  0x2u   /* EnvironmentSampler in both sampler sets (prng.relight_pass_randoms) */
#define RC_PRNG_PLAN_VMF_NOISE    0x4u   /* add the vmf_noise constant (depends on n alone: callers cache it) */

/* model_key: the rng of the model's __call__; loss_key: the key material_smoothness receives, or NULL (no noise row).
 * level_samples[n_levels]: samples per sampler level (the last one is S_last).  Writes at most `capacity` rows to segs,
 * the number of rows to *count and the arena's size in words to *arena_words.  RC_ERR_INVALID_ARG for a NULL pointer,
 * n_rays < 1, K < 2, a capacity too small or a tensor of 2^32 - 1 elements or more; no rc_last_error (no handle). */
int rc_material_randoms_plan(const uint32_t model_key[2], const uint32_t* loss_key, int64_t n_rays, int32_t K,
                             float diffuse_fraction, int32_t num_vmf, const int32_t* level_samples, int32_t n_levels,
                             uint32_t flags, rc_prng_segment* segs, int32_t capacity, int32_t* count, int64_t* arena_words);

/* Fills every segment of segs[n_segs] into arena (arena_words 32-bit words on the device) in ONE launch on `stream`.
 * RC_ERR_INVALID_ARG, with nothing launched, for n_segs > RC_PRNG_MAX_SEGMENTS, an unknown mode, a segment of
 * 2^32 - 1 elements or more, a destination outside [0, arena_words) or two destinations that overlap. */
int rc_prng_fill_segments(rc_handle* h, const rc_prng_segment* segs, int32_t n_segs, void* arena, int64_t arena_words,
                          void* stream);

/* ---- training backward of one proposal level's density field ----------------------
 * Replaces, for the parameters of Cache/Sampler/MLP_<level>, the gradients jax.value_and_grad(loss_fn) yields in
 * train_step (internal/train_utils.py:3128-3131) for the sub-graph HashEncoding.__call__
 * (internal/grid_utils.py:808-905) -> DensityMLP.run_network (internal/geometry.py:155-168) ->
 * convert_raw_density (internal/geometry.py:318-341), given the upstream gradients of its two outputs.
 *   points     [n,3] world-space sample means (device)
 *   d_density  [n]    d L / d density            d_feature  [n,64] d L / d feature (the hidden vector the shader
 *                                                 reads) or NULL
 *   grads      device buffer of rc_density_grad_size floats, layout rc_density_grad_layout (tensor names, offsets
 *              and shapes of the reference's parameter tree); gradients are ACCUMULATED into it (zero it per step)
 *   density_out [n] or NULL: the forward value, for the caller's loss
 * Table gradients use hardware float atomics (order-dependent in the last bits); the MLP gradients are reduced in a
 * fixed order.  Across ranks the caller averages `grads` (jax.lax.pmean, train_utils.py:3133-3135) with one
 * all-reduce over RCCL (nrc_amd.train.allreduce_grads). */
typedef struct rc_grad_segment {
  char name[160];          /* e.g. params/Cache/Sampler/MLP_2/density_grid/hash_2048 */
  int64_t offset, size;    /* in floats */
  int32_t ndim;
  int64_t shape[4];
} rc_grad_segment;
int64_t rc_density_grad_size(rc_handle* h, int32_t level);
int rc_density_grad_layout(rc_handle* h, int32_t level, rc_grad_segment* segs, int32_t capacity, int32_t* count);
int rc_density_backward(rc_handle* h, int32_t level, const float* points, int64_t n, const float* d_density,
                        const float* d_feature, float* grads, float* density_out, void* stream);

/* Transpose of rc_hashgrid_lookup for any grid of the handle (0-2 proposal density grids, 3 appearance, 4 material,
 * 5 light): d_features [n, L*F] (the layout rc_hashgrid_lookup writes) is scattered into `grads`, a device buffer of
 * `total` floats holding the grid's tables in level order, each laid out like the loaded tensor
 * (rc_hashgrid_grad_layout; names = the reference's parameter paths).  Accumulates; hardware float atomics.
 * What jax's autodiff emits for HashEncoding.__call__ (internal/grid_utils.py:808-905) inside train_step. */
int rc_hashgrid_grad_layout(rc_handle* h, int32_t grid_id, rc_grad_segment* segs, int32_t capacity, int32_t* count, int64_t* total);
int rc_hashgrid_backward(rc_handle* h, int32_t grid_id, const float* points, int64_t n, const float* d_features, float* grads,
                         int32_t apply_contraction, void* stream);

/* Spline interlevel loss of the proposal samplers and the exact gradients of both proposal networks
 * (loss_utils.spline_interlevel_loss, internal/loss_utils.py:74-104, with ProposalVolumeSampler.stop_level_grad,
 * sampling.py:354-355: each proposal level's loss reaches only its own density).  One call:
 *   1. the training forward: the three sampler levels (sampling + grid lookup + density MLP; no shader) of rc_render_rays'
 *      launch plan, with the caller's jitter (rnd->jitter; rnd NULL = the deterministic sampler) and `anneal`
 *      (the train-time clip(bias(train_frac / anneal_end, anneal_slope), 0, anneal_clip), sampling.py:326-335; the
 *      handle's rc_config.anneal is the render-time value), on a workspace set of its own ("i:");
 *   2. per proposal level l < num_levels-1: the last level's weights * lossmult blurred by blurs[l] and resampled onto
 *      level l's intervals (stepfun.blur_and_resample_weights, stepfun.py:463-483; linspline.py:95-222), the term
 *      losses[l] = mults[l] * mean over the n x S_l samples of max(0, w_blur - wp)^2 / (wp + 1e-5), wp = weights_l *
 *      lossmult, and its d / d density_l through compute_alpha_weights (render.py:134-169);
 *   3. per proposal level whose grads[l] is not NULL: rc_density_backward of that level at the forward's own sample
 *      means with that d_density, ACCUMULATED into grads[l] (layout rc_density_grad_layout(l)).
 * rays: origins, directions, viewdirs, near, far as for rc_render_rays.  lossmult: [n] device floats or NULL (1).
 * mults, blurs: HOST arrays of num_levels-1 floats (the hotdog gin: mults (0.01, 0.01), blurs (0.03, 0.003);
 * configs/ngp_yobo.gin:245-247).  losses: DEVICE array of num_levels-1 floats, written (bitwise reproducible).
 * The mean is over the local batch; a data-parallel trainer all-reduces (averages) grads afterwards, as pmean.
 * Scaling by (not finetune_cache) (train_utils.py:3193-3202) is the caller's.  Everything is ordered on `stream`.
 * The last level must have <= 32 intervals, the proposal levels <= 64 (RC_ERR_UNSUPPORTED otherwise); the time-resolved
 * cache handle is unsupported.  n == 0 returns RC_OK and writes nothing.
 * Buffers of the call: rc_workspace_ptr "i:" names. */
int rc_interlevel_backward(rc_handle* h, const rc_rays* rays, const float* lossmult, int64_t n, const rc_randoms* rnd,
                           float anneal, const float* mults, const float* blurs, float* const* grads, float* losses,
                           void* stream);

/* Data loss of the cache pass and the exact gradients of the parameters it reaches (train_utils.compute_data_loss,
 * internal/train_utils.py:402-528, loss_type 'charb' for the cache stage):
 *   loss = mult * mean over the n x 3 channels of lossmult * sqrt((rgb - gt)^2 + charb_padding^2),
 *   rgb  = the level-2 composite sum w rgb_s + max(0, 1 - acc) bg (render.py:172-247), no sRGB conversion.
 * sdist carries no gradient (sampling.py:354-355): the loss reaches MLP_<num_levels-1> and Cache/Shader only.  One call:
 *   1. the training forward: rc_render_rays' launch-per-stage cache pass (the rc_set_fused(0) plan; no analytic normals)
 *      with the caller's jitter and `anneal` (as rc_interlevel_backward) on a workspace set of its own ("d:");
 *   2. the loss (written to `loss`, a DEVICE float; bitwise reproducible) and d loss / d density, d loss / d rgb_s;
 *   3-5. only when density_grads or shader_grads is given: the shader's recompute and backward, its weight gradients
 *      (fixed reduction order), d feature += W_n^T d pred_raw, rc_density_backward of the last level into density_grads
 *      (layout rc_density_grad_layout(num_levels-1)) and rc_hashgrid_backward of the appearance grid into its segment of
 *      shader_grads (layout rc_shader_grad_layout).  Both are ACCUMULATED into.
 * gt_rgb: [n,3] device; lossmult: [n] device or NULL (1).  Cache/Shader/EnvMap, SurfaceLightField/output_rgba_layer and
 * the model-level Cache/EnvMap get an exact 0 and are not in the layout.  The reference counts the term twice ("main"
 * and "cache_main", models.py:2065-2071); this call returns one copy, scaled by `mult`.  Everything is ordered on
 * `stream`.  The last level must have <= 32 intervals (RC_ERR_UNSUPPORTED otherwise); the time-resolved cache handle is
 * unsupported.  n == 0 returns RC_OK and writes nothing.  Buffers of the call: rc_workspace_ptr "d:" names. */
int64_t rc_shader_grad_size(rc_handle* h);
int rc_shader_grad_layout(rc_handle* h, rc_grad_segment* segs, int32_t capacity, int32_t* count);
int rc_data_backward(rc_handle* h, const rc_rays* rays, const float* gt_rgb, const float* lossmult, int64_t n,
                     const rc_randoms* rnd, float anneal, float charb_padding, float mult, float* density_grads,
                     float* shader_grads, float* loss, void* stream);

/* Geometry losses of the cache stage on the last sampler level and their exact gradients (first order: the analytic
 * normals are stop-gradiented, tdist carries none).  With w = weights * lossmult of the last level, v = -viewdirs,
 * n^ = normals_pred = nan_to_num(-l2_normalize(pred_normals_layer(h))) and n the analytic normals:
 *   losses[0] distortion   distortion_mult * mean over rays of lossfun_distortion(power_ladder(tdist, distortion_p,
 *                          distortion_premult), w)          (loss_utils.py:108-123, stepfun.py:253-269); reaches w
 *   losses[1] orientation  orientation_mult * mean |sum |w min(0, n^.v)^2| + 1e-5|  (loss_utils.py:126-165); w and n^
 *   losses[2] predicted    pred_normal_mult * mean |sum |w (1 - n.n^)| + 1e-5|      (loss_utils.py:168-201); n^, and w
 *                          at pred_normal_w_grad_weight of its gradient (utils.stopgrad_with_weight)
 *   losses[3] reverse      pred_normal_reverse_mult times the same value; n^ only (train_utils.py:1073-1093)
 * One call:
 *   1. the training forward: the sampler levels of rc_render_rays' launch-per-stage plan, the last level with its
 *      hidden vector, predicted and analytic normals (no shader), with the caller's jitter and `anneal` (as
 *      rc_interlevel_backward) on a workspace set of its own ("g:");
 *   2. the four losses (DEVICE [4], written; bitwise reproducible), d loss / d density and d loss / d pred_raw;
 *   3. only when density_grads or shader_grads is given: pred_normals_layer's gradient into its segment of
 *      shader_grads (layout rc_shader_grad_layout; nothing else of it is touched), d feature64 = W_n^T d pred_raw and
 *      rc_density_backward of the last level into density_grads (layout rc_density_grad_layout(num_levels-1)).  Both
 *      are ACCUMULATED into.  Both NULL: the losses only.
 * cfg: HOST struct, one copy of each term; the multipliers already include the normal-weight ease / decay.  lossmult:
 * [n] device or NULL (1).  The reference counts these terms twice ("main" and "cache_main"); the caller scales.
 * Everything is ordered on `stream`.  The last level must have <= 32 intervals (RC_ERR_UNSUPPORTED otherwise); the
 * time-resolved cache handle is unsupported.  n == 0 returns RC_OK and writes nothing.  Buffers: "g:" names. */
typedef struct {
  float distortion_mult, distortion_p, distortion_premult;
  float orientation_mult;
  float pred_normal_mult, pred_normal_w_grad_weight, pred_normal_reverse_mult;
} rc_geometry_loss;
int rc_geometry_backward(rc_handle* h, const rc_rays* rays, const float* lossmult, int64_t n, const rc_randoms* rnd,
                         float anneal, const rc_geometry_loss* cfg, float* density_grads, float* shader_grads,
                         float* losses, void* stream);

/* param_regularizer_loss for one density grid (train_utils.py:1169-1214; the hotdog gin's 'density_grid':
 * (mult, jnp.mean, 2, 1), nerf_ngp_yobo.gin:47-51): loss = mult * sum over the level's tables of 0.5 * mean(x^2),
 * written to `loss` (DEVICE float; fixed reduction order); when density_grads is given, mult * x / numel(table) is
 * ACCUMULATED into each table's segment of it (layout rc_density_grad_layout(level)); the MLP segments are untouched.
 * Ordered on `stream`; the time-resolved cache handle is unsupported. */
int rc_density_regularizer(rc_handle* h, int32_t level, float mult, float* density_grads, float* loss, void* stream);

/* Gradient THROUGH the analytic normals of the last sampler level (second order in the density field): for
 * n(x) = nan_to_num(-l2_normalize(d raw / d x)) (geometry.py:421-460, no stop-gradient) the gradient of
 * sum(d_normals * n(points)) with respect to the last level's tables and the kernels of density_layers_0,
 * density_layers_1 and output_density_layer, ACCUMULATED into `grads` (layout rc_density_grad_layout(num_levels-1)).
 * The three bias gradients are exact zeros (the ReLU network is piecewise linear): the bias segments are not touched.
 * points: [n,3] world-space, d_normals: [n,3], normals_out: [n,3] or NULL (the normals themselves), all device.
 * l2_normalize's override gradient (the backward divides by sqrt(max(float32 eps, |g|^2))) and nan_to_num's rule (the
 * gradient passes where the value is finite) are the reference's.  The weight gradients have a fixed reduction order
 * (bitwise reproducible); the table gradients are float atomics (order-dependent in the last bits).
 * Any handle whose last level has 32 grid features (RC_ERR_UNSUPPORTED otherwise), the time-resolved one included.
 * RC_ERR_INVALID_ARG for n < 0, NULL grads, NULL points / d_normals with n > 0; n == 0 returns RC_OK and launches nothing.
 * Ordered on `stream`.  Buffers: "nb:" names ("feat", "jac", "gf", "ghat", "u", "t0", "a0", "t1", "a2", "ones", "partial",
 * "normals"). */
int rc_normals_backward(rc_handle* h, const float* points, int64_t n, const float* d_normals, float* grads, float* normals_out,
                        void* stream);

/* geometry_smoothness_loss of the cache stage (train_utils.py:2703-2812; added to "main" at trainer.py:316-320 when
 * Config.use_geometry_smoothness is set and the stage has no material) and its exact gradient.  On the last sampler
 * level (S intervals), with x the training forward's sample means (no gradient), x' = x + noise * cfg->noise (fp32, product
 * and sum rounded separately; noise: DEVICE [n, S, 3] standard normals, prng.geometry_smoothness_noise) and
 * c = lossmult * stop_gradient(weights * S):
 *   loss = weight_normals * mean over [n, S, 3] of |n(x) - n(x')| c + weight_density * mean over [n, S] of |d(x) - d(x')| c,
 * n the analytic normals (differentiable at both point sets), d the converted density with its bounding-box mask,
 * nan_to_num on the perturbed results, lax.abs' derivative (+1 at 0).  One call:
 *   1. the training forward of the sampler levels with the analytic normals (as rc_geometry_backward) on a workspace set
 *      of its own ("gs:"), the perturbed points, the last level once more at x';
 *   2. the loss (ONE DEVICE float, written; fixed reduction order, bitwise reproducible), d loss / d normals at x and
 *      (negated) at x', d loss / d density at both when weight_density != 0;
 *   3. only when density_grads is given, per chunk of 32 768 samples: rc_normals_backward at x and at x', and
 *      rc_density_backward at both when weight_density != 0, all ACCUMULATED into density_grads (layout
 *      rc_density_grad_layout(num_levels-1)).
 * cfg: HOST struct; the weights already carry the caller's mult.  weight_normals_pred != 0 is RC_ERR_UNSUPPORTED before
 * any launch (no config uses it), and so is a time-resolved cache handle, a last level of more than 32 intervals or of
 * other than 32 grid features.  RC_ERR_INVALID_ARG for NULL rays / cfg / loss, NULL noise with n > 0, a non-finite setting
 * or anneal.  n == 0 returns RC_OK and writes nothing.  Ordered on `stream`.  Buffers: "gs:" names (the training forward's,
 * and "means_p" SoA [3][n S], "feat_p", "jac_p", "density_p", "normals_p" SoA, "points", "points_p" [n S][3], "d_normals",
 * "d_normals_p" [n S][3], "d_density", "d_density_p", "loss_ray"). */
typedef struct { float noise, weight_normals, weight_normals_pred, weight_density; } rc_geometry_smoothness;
int rc_geometry_smoothness_backward(rc_handle* h, const rc_rays* rays, const float* lossmult, int64_t n, const rc_randoms* rnd,
                                    float anneal, const float* noise, const rc_geometry_smoothness* cfg, float* density_grads,
                                    float* loss, void* stream);

/* Mask loss of the cache stage on the last sampler level's opacity and its exact gradient (train_utils.compute_mask_loss,
 * internal/train_utils.py:785-836, called at :2919-2927 whenever not config.is_material), with acc = the sum of the
 * last level's weights (render.py:202):
 *   loss = mean over the n rays of lossmult * wt * sqrt((acc - m)^2 + charb_padding^2),
 *   wt   = m > 0.5 ? weight_opaque : weight_empty.
 * masks: [n] device or NULL (ones: batch.masks is None, :801-804).  The main term takes (weight_opaque, weight_empty) =
 * (opaque_loss_weight, empty_loss_weight); the backward term (losses["mask_backwards"], :2929-2945) is the
 * empty_loss_weight= branch (:821-826): zero_masks with weights (0, backward_mask_loss_weight) on the rays of
 * rc_backward_mask_rays.  The mask-weight decay / ease (:897-932) and (not finetune_cache) are folded into the two
 * weights by the caller.  sdist carries no gradient (sampling.py:354-355): the loss reaches MLP_<num_levels-1> only.
 * One call:
 *   1. the training forward: the sampler levels only, no shader (weights_only=True, models.py:476-486; what
 *      rc_interlevel_backward's step 1 runs) with the caller's jitter and `anneal`, on a workspace set of its own ("mk:");
 *   2. the loss (a DEVICE float, written; bitwise reproducible) and d loss / d density of the last level;
 *   3. only when density_grads is given: rc_density_backward of the last level at the forward's own means, ACCUMULATED
 *      into density_grads (layout rc_density_grad_layout(num_levels-1)).
 * cfg: HOST struct.  lossmult: [n] device or NULL (1).  One copy of the term; the reference computes it per output key
 * ("main" and "cache_main"), the caller scales.  Everything is ordered on `stream`.  The last level must have <= 32
 * intervals (RC_ERR_UNSUPPORTED otherwise); the time-resolved cache handle is unsupported; charb_padding <= 0 or
 * non-finite is RC_ERR_UNSUPPORTED before any launch (JAX's gradient is NaN there).  A NULL loss, cfg or rays, or n < 0:
 * RC_ERR_INVALID_ARG.  n == 0 returns RC_OK and writes nothing.  Buffers: "mk:" names. */
typedef struct {
  float charb_padding;   /* Config.charb_padding (1e-3); must be > 0 */
  float weight_opaque;   /* applied where mask > 0.5 (strict) */
  float weight_empty;    /* applied elsewhere */
  int32_t zero_masks;    /* nonzero: masks are all 0 and `masks` is not read (the backward term) */
} rc_mask_loss;
int rc_mask_backward(rc_handle* h, const rc_rays* rays, const float* masks, const float* lossmult, int64_t n,
                     const rc_randoms* rnd, float anneal, const rc_mask_loss* cfg, float* density_grads, float* loss,
                     void* stream);

/* The rays of the backward mask term (train_utils._compute_backward_mask_loss, internal/train_utils.py:3348-3401: its
 * call of render_utils.get_secondary_rays, render_utils.py:927-1056, with one sample of UniformHemisphereSampler
 * (:395-403), no MIS and the unstratified RandomGenerator2D(1, 1, False), :322-352), one per batch ray, in fp32:
 *   normal     = -look
 *   origin     = (origins + look * shadow_near_max) + normal * normal_eps
 *   direction  = local_to_global((sin t cos p, sin t sin p, cos t), get_rotation_matrix(normal))   (:145-168),
 *                cos t = 1 - u1, sin t = sqrt((2 - u1) u1), p = 2 pi u2 - pi;   viewdirs = directions
 *   near       = shadow_near_max (:3381-3383), far = `far` (Config.secondary_far)
 * origins, look, u1, u2: device [n,3], [n,3], [n], [n] (u1, u2 in [0, 1): the two columns of one uniform(key, (n, 2))).
 * out_*: device [n,3], [n,3], [n], [n], the fields rc_rays reads (out_directions serves as viewdirs as well); lossmult
 * passes through unchanged and radii are not read on this path.  Ordered on `stream`, allocates nothing, any handle.
 * RC_ERR_INVALID_ARG with nothing launched for a NULL pointer, n < 0 or a non-finite scalar; n == 0 launches nothing. */
int rc_backward_mask_rays(rc_handle* h, const float* origins, const float* look, const float* u1, const float* u2, int64_t n,
                          float shadow_near_max, float normal_eps, float far, float* out_origins, float* out_directions,
                          float* out_near, float* out_far, void* stream);

/* ---- the optimizer step of the cache stage -------------------------------------------------------
 * rc_adam_update: what train_step does with the gradients after pmean (internal/train_utils.py:3154-3161):
 * tree_map(nan_to_num) (NaN -> 0, +-inf -> +-FLT_MAX), clip_gradients (train_utils.py:1274-1298: clip by value when
 * grad_max_val > 0, then by the global norm when grad_max_norm > 0, mult = min(1, grad_max_norm / (FLT_EPSILON + norm)),
 * norm = sqrt(sum g^2) over ALL buffers of the call -- pass one top-level module per call), then optax.adam
 * (scale_by_adam with eps_root = 0, scale_by_learning_rate) and apply_updates, per element in float32:
 *   mu = (1-b1) g + b1 mu;  nu = (1-b2) (g g) + b2 nu;  p = p + ((mu / bc1) / (sqrt(nu / bc2) + eps)) * (-lr)
 * with the scalars of the element's group.  ONE launch over all buffers (two more with the norm clip: per-tile sums of
 * g^2 in double and a fixed-order reduce that leaves the multiplier on the device, rc_workspace_ptr "o:mult" / "o:norm";
 * bitwise reproducible).  Dense: every element moves every step.  zero_grads != 0 writes g = 0 afterwards, so the next
 * step's backward calls can accumulate into the same buffers.  Everything is ordered on `stream`; no host sync.
 *   bufs[k]: DEVICE float32 arrays of n elements each, 16-byte aligned; the HOST arrays seg_offset / seg_size /
 *            seg_group (nseg entries) cover [0, n) in order without gaps (a gradient layout's segments, each with the
 *            optimizer group of its tensor); at most RC_ADAM_MAX_BUFFERS buffers and 32 runs of consecutive segments
 *            of one group over all of them.
 *   step:    HOST struct.  Per group g < ngroups: lr at this step's count t (the caller's schedule), the decays, 1 - b
 *            rounded from the caller's (double) value as optax does, eps, and the bias corrections 1 - b^(t+1). */
#define RC_ADAM_MAX_BUFFERS 8
#define RC_ADAM_MAX_GROUPS 8
typedef struct {
  float* params;
  float* grads;
  float* mu;
  float* nu;
  int64_t n;
  int32_t nseg;
  const int64_t* seg_offset;
  const int64_t* seg_size;
  const int32_t* seg_group;
} rc_adam_buffer;
typedef struct {
  int32_t ngroups;
  float lr[RC_ADAM_MAX_GROUPS];
  float b1[RC_ADAM_MAX_GROUPS], b2[RC_ADAM_MAX_GROUPS];
  float one_minus_b1[RC_ADAM_MAX_GROUPS], one_minus_b2[RC_ADAM_MAX_GROUPS];
  float eps[RC_ADAM_MAX_GROUPS];
  float bias_correction1[RC_ADAM_MAX_GROUPS], bias_correction2[RC_ADAM_MAX_GROUPS];
  float grad_max_val;          /* <= 0: off */
  float grad_max_norm;         /* <= 0: off */
  int32_t zero_grads;
} rc_adam_step;
int rc_adam_update(rc_handle* h, const rc_adam_buffer* bufs, int32_t nbuf, const rc_adam_step* step, void* stream);

/* rc_load_params_flat: rc_load_weights of every tensor of one gradient layout, from a DEVICE buffer in that layout
 * (layout = density level l: rc_density_grad_layout(l); RC_LAYOUT_SHADER: rc_shader_grad_layout; RC_LAYOUT_LIGHT:
 * rc_light_grad_layout; RC_LAYOUT_MATERIAL: rc_material_grad_layout; RC_LAYOUT_ENVMAP: rc_envmap_grad_layout;
 * RC_LAYOUT_TRANSIENT_HEADS: rc_transient_head_grad_layout).  The grid tables
 * are copied device to device into the handle's table buffers, ordered on `stream`; the dense-layer segments go to
 * the host in ONE copy (gathered on the device first when they are not contiguous), after which the call waits for
 * `stream` (the host repack needs them).  The derived tables (cell tables, level-2 pairs, cell records) and packs are
 * marked stale and captured graphs dropped, as rc_load_weights does: the next render or backward call on any stream
 * computes bitwise what it would after rc_load_weights of the same tensors.  A time-resolved cache handle loads
 * RC_LAYOUT_TRANSIENT_HEADS and RC_LAYOUT_TRANSIENT_SAMPLER only (every other layout: RC_ERR_UNSUPPORTED); those two
 * layouts need such a handle. */
#define RC_LAYOUT_SHADER (-1)
#define RC_LAYOUT_LIGHT (-2)   /* rc_light_grad_layout */
#define RC_LAYOUT_MATERIAL (-3)   /* rc_material_grad_layout */
#define RC_LAYOUT_ENVMAP (-4)   /* rc_envmap_grad_layout */
#define RC_LAYOUT_TRANSIENT_HEADS (-5)   /* rc_transient_head_grad_layout */
#define RC_LAYOUT_TRANSIENT_SAMPLER (-6)   /* rc_transient_sampler_grad_layout */
int rc_load_params_flat(rc_handle* h, int32_t layout, const float* params, void* stream);

/* ---- the light sampler's own loss -----------------------------------------------------------------
 * light_sampling (train_utils.light_sampling_loss, internal/train_utils.py:1985-2067 -> render_utils.vmf_loss_fn,
 * internal/inverse_render/render_utils.py:1493-1547) and its exact first-order gradient of the params/LightSampler tensors.
 * Per suffix s of the batched secondary trace (indirect_specular: the Ks GGX rays, indirect_diffuse: the Kd cosine + vMF
 * rays), over the n x K_s samples:
 *   L_s  = mean of (f - l) sg(f - l) w (lossmult_r / K_s) / max(pdf, 1e-2)       (the reference divides by K_s twice)
 *   f    = srgb(max(|radiance_in|, 1e-5)), radiance_in = nan_to_num(the trace's rgb), |.| the 2-norm (no gradient)
 *   l    = srgb(max(sum_j safe_exp(logit_j) eval_vmf(d, l2_normalize(mean_j, grad_eps = 1e-5), kappa_j), 1e-5))
 *   w    = clip(weight, 0, 10), 0 where d . n <= 0 (n = the shading point's normals_to_use)
 *   loss = mult (L_spec + L_diff) / 2, srgb = image.linear_to_srgb when linear_to_srgb != 0, else the identity.
 * mean_j, kappa_j, logit_j: get_vmfs of the light head at the shading point (vmf_scale, the caller's vmf_noise and the
 * point itself are constants).  Everything else the loss reads is stop-gradiented: the gradient reaches only the
 * LightSampler parameters.  One call:
 *   1. rc_render_material's forward with the same rnd / mrnd / num_secondary_samples (the primary cache pass, the shading
 *      point's pick, the shading heads, BRDF importance sampling, the batched secondary trace; no integration, no EnvMap,
 *      no material-only composite) on rc_render_material's workspace sets (set 0 and "s:"): m_pts, l_vmf, l_vmf_logit,
 *      sec_dirs, sec_samples and sec_rgb are bitwise what rc_render_material leaves there for the same inputs;
 *   2. the light head's recompute (h0, h1, vmf_params), the loss (DEVICE float, written; fixed reduction order, bitwise
 *      reproducible) and, when light_grads is given, d loss / d vmf_params;
 *   3. only when light_grads is given: the three dense layers' backward (weight gradients reduced over fixed slices of
 *      points: bitwise reproducible) and rc_hashgrid_backward of the light grid (grid 5, contracted) at the shading
 *      points; ACCUMULATED into light_grads (layout rc_light_grad_layout).  NULL: the loss only.
 * lossmult: [n] device or NULL (1).  The mean is over the local batch; a data-parallel trainer averages light_grads.
 * Argument checks, the num_secondary_samples split and the refusals are rc_render_material's (missing material or light
 * weights: RC_ERR_MISSING_WEIGHT; the EnvMap is not needed); the time-resolved cache handle is unsupported.  n == 0
 * returns RC_OK and writes nothing.  Everything is ordered on `stream`.  Buffers of the call: set-0 / "s:" / "ls:" names.
 * Not covered: the gradient the LightSampler receives from the material data loss through the vMF-sampled directions. */
typedef struct {
  float mult;                  /* the extra loss's multiplier (trainer.gin: 1.0) */
  int32_t linear_to_srgb;      /* Config.light_sampling_linear_to_srgb (ngp_yobo.gin: True) */
} rc_light_sampling_loss;
/* The light layout: params/LightSampler/light_grid tables in level order (as rc_hashgrid_grad_layout(5)), then layers_0,
 * layers_1 and output_layer, kernel [in, out] then bias [out] each. */
int64_t rc_light_grad_size(rc_handle* h);
int rc_light_grad_layout(rc_handle* h, rc_grad_segment* segs, int32_t capacity, int32_t* count);
int rc_light_sampling_backward(rc_handle* h, const rc_rays* rays, const float* lossmult, int64_t n, const rc_randoms* rnd,
                               const rc_material_randoms* mrnd, int32_t num_secondary_samples,
                               const rc_light_sampling_loss* cfg, float* light_grads, float* loss, void* stream);
/* param_regularizer_loss for 'light_grid' (train_utils.py:1169-1214; nerf_ngp_yobo.gin:47-51, (mult, jnp.mean, 2, 1)):
 * loss = mult * sum over the light grid's tables of 0.5 * mean(x^2), written to `loss` (DEVICE float; fixed reduction
 * order); when light_grads is given, mult * x / numel(table) is ACCUMULATED into each table's segment of it (layout
 * rc_light_grad_layout); the MLP segments are untouched.  Ordered on `stream`; the time-resolved cache handle is
 * unsupported.  Buffers: "ls:reg_part". */
int rc_light_regularizer(rc_handle* h, float mult, float* light_grads, float* loss, void* stream);

/* ---- the material network's smoothness loss ------------------------------------------------------
 * material_smoothness (train_utils.material_smoothness_loss, internal/train_utils.py:2505-2700, with the hotdog values
 * configs/nerf_ngp_yobo.gin:400-408) and its exact first-order gradient of the params/MaterialShader tensors.  With x the
 * shading point of each ray (rc_render_material's pick, weight w = filt_weight), x' = x + noise_scale nu (stopped),
 * m = material_mlp (material grid -> bottleneck_layer -> pred_brdf_layer -> albedo, roughness, metalness) and
 * m' = nan_to_num(m at x'), lambda = lossmult_r w (no gradient):
 *   loss = mult (weight_albedo mean_{n x 3} |(a - a') / max(1e-6, max(a, a'))| lambda      (tensoir_albedo; else |a - a'|)
 *                + weight_other mean_n |r - r'| lambda + weight_other mean_n |m_metal - m_metal'| lambda)
 * Both evaluations carry parameter gradients; nothing reaches the geometry.  JAX rules: max ties split the gradient,
 * d|x|/dx = +1 at 0.  One call:
 *   1. rc_render_material's steps 1-2 (the primary cache pass, the shading point's pick) with the same rnd / mrnd (only
 *      mrnd's gumbel / resample_inds are read) on set 0, and its material lookup and head at the shading points:
 *      m_pts, filt_weight and m_mat are bitwise what rc_render_material leaves there for the same inputs (no light head,
 *      no BRDF sampling, no secondary trace; the material features go to "ms:feat", not to m_feat);
 *   2. the loss (DEVICE float, written; fixed reduction order, bitwise reproducible);
 *   3. only when material_grads is given: the exact gradient, ACCUMULATED into material_grads (layout
 *      rc_material_grad_layout): the dense segments reduced over fixed per-workgroup partials (bitwise reproducible),
 *      the material grid's tables through rc_hashgrid_backward at the 2n points.  NULL: the loss only.
 * noise: [n][3] device floats (nu ~ N(0, 1)).  lossmult: [n] device or NULL (1).  The mean is over the local batch; a
 * data-parallel trainer averages material_grads.  Missing material weights: RC_ERR_MISSING_WEIGHT; the time-resolved
 * cache handle is unsupported.  n == 0 returns RC_OK and writes nothing.  Everything is ordered on `stream`.  Buffers of
 * the call: set-0 / "ms:" names.
 * The material data loss: rc_material_data_backward. */
typedef struct {
  float mult;                  /* the extra loss's multiplier (trainer.gin: 1.0) */
  float weight_albedo;         /* Config.material_smoothness_weight_albedo (nerf_ngp_yobo.gin: 1e-4) */
  float weight_other;          /* Config.material_smoothness_weight_other (nerf_ngp_yobo.gin: 1e-4) */
  float noise;                 /* Config.material_smoothness_noise (nerf_ngp_yobo.gin: 0.01) */
  int32_t tensoir_albedo;      /* Config.material_smoothness_tensoir_albedo (nerf_ngp_yobo.gin: True) */
} rc_material_smoothness_loss;
/* The material layout: params/MaterialShader/material_grid tables in level order (as rc_hashgrid_grad_layout(4)), then
 * bottleneck_layer and pred_brdf_layer, kernel [in, out] then bias [out] each. */
int64_t rc_material_grad_size(rc_handle* h);
int rc_material_grad_layout(rc_handle* h, rc_grad_segment* segs, int32_t capacity, int32_t* count);
int rc_material_smoothness_backward(rc_handle* h, const rc_rays* rays, const float* lossmult, int64_t n, const rc_randoms* rnd,
                                    const rc_material_randoms* mrnd, const float* noise, const rc_material_smoothness_loss* cfg,
                                    float* material_grads, float* loss, void* stream);
/* param_regularizer_loss for 'material_grid' (train_utils.py:1169-1234; nerf_ngp_yobo.gin:47-51, (1.0, jnp.mean, 2, 1)):
 * loss = mult * sum over the material grid's tables of 0.5 * mean(x^2), written to `loss` (DEVICE float; fixed
 * reduction order); when material_grads is given, mult * x / numel(table) is ACCUMULATED into each table's segment of
 * it (layout rc_material_grad_layout); the MLP segments are untouched.  The reference's ease factor for the prefix
 * "material" is 1 in the material stages (use_material_weight_ease = False) and is the caller's (folded into mult).
 * Ordered on `stream`; the time-resolved cache handle is unsupported.  Buffers: "ms:reg_part". */
int rc_material_regularizer(rc_handle* h, float mult, float* material_grads, float* loss, void* stream);

/* ---- the material stage's data loss --------------------------------------------------------------
 * The "data" term of the material_light_from_scratch stage: train_utils.compute_data_loss on the MaterialIntegrator's
 * rgb (internal/train_utils.py:402-528) with loss_type 'rawnerf_transient_unbiased', which _select_data_loss_function
 * maps to compute_unbiased_loss_rawnerf (:173-197), and its exact gradient of the params/MaterialShader tensors.  With
 * rgb = w sh_rgb + max(0, 1 - acc) bg (rc_render_material's "rgb"), c = the primary cache pass's rgb (the rendering's
 * "cache_rgb", which _get_rgb_clip_for_rawnerf reads first), gt_c = clip(c, 0, clip_val) (or clip(gt, 0, clip_val) when
 * use_gt_rawnerf), then clip(max(., gt), 0, clip_val) when use_combined_rawnerf, then its norm over the channels when
 * use_norm_rawnerf, s = 1 / (sg(gt_c) ** exponent + eps) per ray and channel, lossmult_rc = 0 where gt > thresh:
 *   loss = weight * mult * mean_{n x 3}(lossmult * 2 (rgb - gt) sg(rgb - gt) s)
 * The gradient is the one of the reference's Trainer.stopgrad = True reading (MaterialMLP.stopgrad_rays =
 * stopgrad_samples = True): path (a), through the material grid, bottleneck_layer, pred_brdf_layer, the heads, F0, GGX D,
 * Smith G (k = a / 2), Lambert, the clip of radiance * lobe, the means over the samples and rgb; every input of the
 * integration read from the secondary trace (directions, pdf, MIS weight, cache radiance, acc, EnvMap radiance), w and
 * the primary geometry are constants.  Not covered: the default hotdog reading's path (b) (roughness -> GGX-sampled
 * direction), and the gradients of the Cache, EnvMap and LightSampler through this loss.  One call:
 *   1. rc_render_material itself with the same rnd / mrnd / num_secondary_samples (set 0, "s:"): its buffers are
 *      bitwise what a plain rc_render_material call leaves; its primary composite goes to "md:cache_rgb" / "md:cache_acc";
 *   2. the loss (DEVICE float, written; fixed reduction order, bitwise reproducible); "md:rgb" = the rebuilt rgb, bitwise
 *      rc_render_material's;
 *   3. only when material_grads is given: the gradient, ACCUMULATED into material_grads (layout rc_material_grad_layout):
 *      the dense segments reduced over fixed per-workgroup partials (bitwise reproducible), the material grid's tables
 *      through rc_hashgrid_backward at the shading points.  NULL: the loss only.
 * gt_rgb: [n][3] device floats.  lossmult: [n] device or NULL (1); a caller with masks folds them in (mask_lossmult).
 * The mean is over the local batch; a data-parallel trainer averages material_grads.  Missing material or EnvMap weights:
 * RC_ERR_MISSING_WEIGHT; the time-resolved cache handle is unsupported.  n == 0 returns RC_OK and writes nothing.
 * Everything is ordered on `stream`.  Buffers of the call: set-0 / "s:" / "md:" names. */
typedef struct {
  float mult;                  /* Config.data_loss_mult (ngp_yobo.gin: 1.0) */
  float weight;                /* MaterialModel.loss_weight (nerf_ngp_yobo.gin: 0.1) times material_loss_weight_ease (1) */
  float exponent;              /* Config.rawnerf_exponent_material (nerf_ngp_yobo.gin: 1) */
  float eps;                   /* Config.rawnerf_eps_material (nerf_ngp_yobo.gin: 1e-2) */
  float clip_val;              /* compute_unbiased_loss_rawnerf's clip_val (1e4) */
  float thresh;                /* Config.loss_thresh (configs.py: 1e6) */
  int32_t use_gt_rawnerf;      /* Config.use_gt_rawnerf (configs.py: False) */
  int32_t use_combined_rawnerf; /* Config.use_combined_rawnerf (configs.py: True) */
  int32_t use_norm_rawnerf;    /* Config.use_norm_rawnerf (configs.py: False) */
} rc_material_data_loss;
int rc_material_data_backward(rc_handle* h, const rc_rays* rays, const float* gt_rgb, const float* lossmult, int64_t n,
                              const rc_randoms* rnd, const rc_material_randoms* mrnd, int32_t num_secondary_samples,
                              const rc_material_data_loss* cfg, float* material_grads, float* loss, void* stream);

/* ---- the EnvMap's gradient of the material stage's data loss --------------------------------------
 * rc_material_data_backward_env is rc_material_data_backward (same forward, loss, material_grads, refusals and buffers,
 * bit for bit) and, when envmap_grads is given, the exact gradient of the same loss w.r.t. the params/Cache/EnvMap tensors
 * that the model-level path reads (Model._handle_env_map, internal/models.py:360-421), under the same
 * Trainer.stopgrad = True reading.  Per secondary ray k of shading point r and channel c:
 *   env   = max(max(softplus(raw + env_rgb_bias), 0), 0)       the EnvMap's clip, then env_map_fn's jnp.maximum
 *   ein   = nan_to_num(env (1 - acc_k))
 *   direct = clip(ein lobe, 0, rgb_max) weight_k / max(pdf_k, 1e-5), averaged over the Ks / Kd samples of its pass
 *   d loss / d env = env_scale g_rc w_r (1 / K_pass) weight_k / max(pdf_k, 1e-5) clip'(ein lobe) lobe (1 - acc_k) max'(.)
 * with g_rc = d loss / d rgb of rc_material_data_backward; the lobe, acc, the directions, pdf, the MIS weight and w are
 * constants.  env_scale: MaterialMLP.stopgrad_env_map_weight[1] (nerf_ngp_yobo.gin:420: 1), stopgrad_with_weight's
 * factor on the gradient (the value is not scaled).  JAX rules: clip / maximum ties pass half, nan_to_num passes where
 * finite, softplus' = sigmoid.  The MLP's backward runs at the trace's own directions ("sec_dirs"), which are stopped:
 * pos_enc has no gradient; the alpha column of output_rgba_layer gets exact zeros; output_ambient_rgb_layer is not read
 * on this path and is not in the layout.  Not covered: the indirect terms, the Cache, the LightSampler, path (b).
 * The EnvMap layout: params/Cache/EnvMap/{layer_0, layer_1, layer_2, layer_bottleneck, output_rgba_layer}, kernel
 * [in, out] then bias [out] each (hotdog: 10 segments, 175 620 floats).  rc_load_params_flat(RC_LAYOUT_ENVMAP) loads it.
 * envmap_grads: ACCUMULATED into; dense gradients are reduced over fixed slices of rows in a fixed order (bitwise
 * reproducible).  Either gradient pointer may be NULL.  The recompute is fp32 whatever rc_mlp_arithmetic() says of the
 * forward.  Everything is ordered on `stream`.  Buffers: rc_material_data_backward's, "md:d_env" ([n Ks | n Kd][3], the
 * sec_* ray order) and one chunk of rows of the EnvMap's backward ("md:e_*"). */
int64_t rc_envmap_grad_size(rc_handle* h);
int rc_envmap_grad_layout(rc_handle* h, rc_grad_segment* segs, int32_t capacity, int32_t* count);
int rc_material_data_backward_env(rc_handle* h, const rc_rays* rays, const float* gt_rgb, const float* lossmult, int64_t n,
                                  const rc_randoms* rnd, const rc_material_randoms* mrnd, int32_t num_secondary_samples,
                                  const rc_material_data_loss* cfg, float env_scale, float* material_grads,
                                  float* envmap_grads, float* loss, void* stream);

/* ---- the time-resolved cache's data loss and its per-bin heads -------------------------------------
 * rc_transient_data_backward: train_utils.compute_transient_data_loss (internal/train_utils.py:531-640) with loss type
 * 'rawnerf_transient_unbiased' (:725-732) on rc_render_transient's own rgb [n][n_bins][3], and its exact gradient of the
 * two per-bin head layers.  With d = rgb - gt, dn = sg(rgb_nocorr - gt_nocorr) (both default to rgb, gt), c =
 * _get_rgb_clip_for_rawnerf of the pass's own rgb (the cache stage's rendering has no "cache_rgb"), s_rc = 1 / (sg(sum over
 * the bins of c) ** exponent + eps) per ray and channel, lossmult_rc = 0 where any bin of gt exceeds thresh:
 *   losses[0] = mult * mean_{n x 3}(lossmult s (sum_b 2 d dn + 2 (k sum_b d)(k sum_b dn) gauss_mult))     k = gauss_constant_scale
 *   losses[1] = mult * mean_{n x 3}(lossmult sum_b d^2)                                                   (the "mses" stat)
 * (transient_gauss_sigma_scales = []: dtof_to_gauss is its constant row; the row is divided by n_bins and added to every
 * bin, so it counts once).  The gradient reading is the one of rc_data_backward / rc_geometry_backward: sample positions,
 * tdist, means and with them every travel time and time shift are constants.  One call:
 *   1. rc_render_transient itself with the same rays / cam_origins / rnd, its "rgb" to "td:rgb";
 *   2. losses (DEVICE floats [2], written; fixed reduction order), "td:G" = d loss / d rgb, "td:Gt";
 *   3. the adjoint of the TransientVolumeIntegrator (the direct scatter, next-ray spill included; the time shift; the
 *      clamps with JAX's tie rule; zero_invalid_bins; indirect_scale; softplus') and of the two heads, whose outputs are
 *      recomputed in fp32 whatever rc_mlp_arithmetic() says and never stored beyond a chunk of 256 rays: "td:d_t_irr",
 *      "td:d_t_slf", "td:d_tint_ibrdf", "td:d_direct", "td:d_weights" (see rc_workspace_ptr) feed the backward of the rest
 *      of the shader, which is not part of this call;
 *   4. only when head_grads is given: the heads' gradient, ACCUMULATED into head_grads (rc_transient_head_grad_layout:
 *      params/Cache/Shader/transient_indirect_layer/{kernel [64, 3 n_bins], bias}, then
 *      params/Cache/Shader/SurfaceLightField/output_rgba_layer/{kernel [128, 3 n_bins + 1], bias}; the alpha column gets
 *      exact zeros), reduced over fixed slices of rows in a fixed order: two calls on the same inputs are bitwise equal.
 * gt, rgb_nocorr, gt_nocorr: [n][n_bins][3] device floats (the latter two may be NULL).  lossmult: [n] device or NULL (1).
 * Needs a time-resolved handle without occlusions (RC_ERR_UNSUPPORTED otherwise).  n == 0 returns RC_OK and writes
 * nothing.  Everything is ordered on `stream`; no allocation once the workspace has seen the batch size.
 * rc_load_params_flat(RC_LAYOUT_TRANSIENT_HEADS) loads the layout. */
typedef struct {
  float mult;                  /* Config.data_loss_mult (cornell.gin:62: 1.0) */
  float gauss_mult;            /* Config.data_loss_gauss_mult (cornell.gin:63: 0.01) */
  float gauss_constant_scale;  /* Config.transient_gauss_constant_scale (cornell.gin:64: 0.5) */
  float exponent;              /* Config.rawnerf_exponent (cornell.gin:55: 1) */
  float eps;                   /* Config.rawnerf_eps (cornell.gin:58: 1e-2) */
  float clip_val;              /* compute_unbiased_loss_rawnerf_transient's clip_val (1e4) */
  float thresh;                /* Config.loss_thresh (configs.py:447: 1e6) */
  int32_t use_gt_rawnerf;      /* Config.use_gt_rawnerf (configs.py:587: False) */
  int32_t use_combined_rawnerf; /* Config.use_combined_rawnerf (configs.py:588: True) */
} rc_transient_data_loss;
int64_t rc_transient_head_grad_size(rc_handle* h);
int rc_transient_head_grad_layout(rc_handle* h, rc_grad_segment* segs, int32_t capacity, int32_t* count);
int rc_transient_data_backward(rc_handle* h, const rc_rays* rays, const float* cam_origins, int64_t n, const rc_randoms* rnd,
                               const float* gt, const float* rgb_nocorr, const float* gt_nocorr, const float* lossmult,
                               const rc_transient_data_loss* cfg, float* head_grads, float* losses, void* stream);

/* rc_transient_data_backward_kind: the same call under every loss type of _select_transient_data_loss_function
 * (internal/train_utils.py:686-750) that the transient gins use, with or without Config.use_itof.  Notation as above, and
 *   I_r(x) = sum_b W_r[b] x_b per channel, the rows of render_utils.dtof_to_itof (inverse_render/render_utils.py:1648-1676):
 *   per (frequency, phase_shift) pair a cos row W[b] = cos(2 pi f t_b + phi) + 1 and a sin row sin(..) + 1, then one constant
 *   row W[b] = 1/2; Nr = 2 n_pairs + 1; t_b = b exposure_time / 299792458 with the handle's own exposure_time.  The table is
 *   evaluated on the host in double and rounded once to float32.
 * data_loss per type (rows = bins for the first four, the Nr iToF rows for the last four), summed over its rows:
 *   RAWNERF_TRANSIENT_UNBIASED       s (sum_b 2 d dn + 2 (k sum d)(k sum dn) gauss_mult)          (the entry above)
 *   RAWNERF_TRANSIENT                s (sum_b d^2 + (k sum d)^2 gauss_mult)                       (:717-724, :329-347)
 *   MSE / MSE_UNBIASED               sum_b d^2 / sum_b 2 d dn
 *   MSE_ITOF / MSE_ITOF_UNBIASED     sum_r I_r(d)^2 / sum_r 2 I_r(d) I_r(dn)
 *   RAWNERF_TRANSIENT_ITOF / .._UNBIASED   the same two times s
 * With use_itof the data loss is divided by its number of rows (n_bins or Nr; :622-623) and losses[1], the "mses" stat,
 * becomes mult * mean_{n x 3}(lossmult sum_r I_r(d)^2 / Nr) (:595-601).  losses[0] = mult * mean_{n x 3}(lossmult data_loss).
 * s and dn carry no gradient.  transient_gauss_sigma_scales stays [] (base.gauss_* is read by the two per-bin rawnerf types
 * only).  Ordering, allocation, n == 0, the handle it needs and the accumulation into head_grads are those of
 * rc_transient_data_backward; steps 1, 3 and 4 are the same code.  loss_type 0 without use_itof runs that entry's own
 * kernel: losses, "td:G" and the gradient are bitwise its.  Refused on the host, nothing launched (RC_ERR_INVALID_ARG): a
 * null cfg, loss_type outside [0, RC_TLOSS_COUNT), n_pairs outside [0, RC_ITOF_MAX_PAIRS], a non-finite frequency or phase.
 * rc_dtof_to_itof: dtof [n][n_bins][3] -> itof [n][2 n_pairs + 1][3] (device floats) with the same table and the same
 * reduction, on any time-resolved handle: an iToF or steady-state measurement of a rendered or ground-truth histogram. */
#define RC_ITOF_MAX_PAIRS 8
typedef enum {
  RC_TLOSS_RAWNERF_TRANSIENT_UNBIASED = 0,
  RC_TLOSS_RAWNERF_TRANSIENT,
  RC_TLOSS_MSE,
  RC_TLOSS_MSE_UNBIASED,
  RC_TLOSS_MSE_ITOF,
  RC_TLOSS_MSE_ITOF_UNBIASED,
  RC_TLOSS_RAWNERF_TRANSIENT_ITOF,
  RC_TLOSS_RAWNERF_TRANSIENT_ITOF_UNBIASED,
  RC_TLOSS_COUNT
} rc_transient_loss_type;
typedef struct {
  rc_transient_data_loss base;
  int32_t loss_type;           /* rc_transient_loss_type: TransientMaterialModel.cache_loss (cornell_itof.gin:6, ngp_yobo.gin:280) */
  int32_t use_itof;            /* Config.use_itof (cornell_itof.gin:5; configs.py:717: False) */
  int32_t n_pairs;             /* len(Config.itof_frequency_phase_shifts) (cornell_itof.gin:4: 4; *_steady_state.gin: 0) */
  int32_t pad;
  double frequency[RC_ITOF_MAX_PAIRS];    /* Hz */
  double phase_shift[RC_ITOF_MAX_PAIRS];  /* radians */
} rc_transient_data_loss_kind;
int rc_transient_data_backward_kind(rc_handle* h, const rc_rays* rays, const float* cam_origins, int64_t n, const rc_randoms* rnd,
                                    const float* gt, const float* rgb_nocorr, const float* gt_nocorr, const float* lossmult,
                                    const rc_transient_data_loss_kind* cfg, float* head_grads, float* losses, void* stream);
int rc_dtof_to_itof(rc_handle* h, const float* dtof, int64_t n, int32_t n_pairs, const double* frequency,
                    const double* phase_shift, float* itof, void* stream);

/* ---- the time-resolved cache's density fields and proposal samplers -------------------------------
 * The sampler side of a time-resolved handle: the three density fields (grid tables and density MLP of every level) and
 * MLP_<last>/pred_normals_layer in ONE flat buffer, RC_LAYOUT_TRANSIENT_SAMPLER = the segments of rc_density_grad_layout(0),
 * then level 1, then level 2, each in its own order, then params/Cache/Sampler/MLP_<last>/pred_normals_layer/{kernel
 * [64, 3], bias [3]}.  rc_transient_sampler_grad_size / _layout describe it, rc_load_params_flat loads it; a steady-state
 * handle has no such layout (RC_ERR_UNSUPPORTED).
 *
 * rc_transient_interlevel_backward, rc_transient_geometry_backward, rc_transient_mask_backward and
 * rc_transient_density_regularizer are rc_interlevel_backward, rc_geometry_backward, rc_mask_backward and
 * rc_density_regularizer on a time-resolved handle: the same host code, kernels, workspace sets ("i:", "g:", "mk:"),
 * reduction order, argument checks and loss slots.  What differs:
 *   - the training forward is this handle's own sampler (power-ladder distances on every ray, its contract radius and
 *     grids), with the caller's jitter and anneal;
 *   - every gradient is ACCUMULATED into `sampler_grads` (RC_LAYOUT_TRANSIENT_SAMPLER; NULL: the losses only): a level's
 *     density gradient into that level's segments, pred_normals_layer's into the tail.  rc_transient_geometry_backward
 *     with a buffer always computes both of its gradients;
 *   - a handle without rc_set_transient and a use_occlusions handle are refused (RC_ERR_UNSUPPORTED), before any other
 *     check of the handle's state; the argument checks in front of that are the counterpart's.
 * The rays of the backward mask term (rc_backward_mask_rays) are passed to rc_transient_mask_backward like any others:
 * on this handle the primary and the secondary sampler differ only by the clamp of `far` at env_map_distance, which is
 * NOT applied (the same rays as long as far <= env_map_distance; the cornell gin's secondary_far is 1).
 *
 * rc_transient_data_backward_sampler: rc_transient_data_backward_kind (the same code: losses, "td:G", the "td:" adjoints
 * and head_grads are bitwise its), then, with `sampler_grads`, the data loss's gradient of MLP_<last> THROUGH THE
 * COMPOSITING WEIGHTS: "td:d_density" = alpha_weights_bwd("td:d_weights") |delta| with the forward's density, tdist and
 * weights of the last level (delta = (t1 - t0) |direction|, the forward compositing's own), and rc_density_backward of the
 * last level at the forward's sample means, accumulated into the level's segments of sampler_grads.  This is the weights
 * path ONLY: the paths through the geometry feature and the predicted normals into the shader need the shader's backward
 * and are not part of the call (the gin weighs them with stopgrad_geometry_feature_weight =
 * stopgrad_geometry_normals_weight = 1.0).  sampler_grads == NULL: nothing beyond rc_transient_data_backward_kind runs. */
int64_t rc_transient_sampler_grad_size(rc_handle* h);
int rc_transient_sampler_grad_layout(rc_handle* h, rc_grad_segment* segs, int32_t capacity, int32_t* count);
int rc_transient_interlevel_backward(rc_handle* h, const rc_rays* rays, const float* lossmult, int64_t n, const rc_randoms* rnd,
                                     float anneal, const float* mults, const float* blurs, float* sampler_grads, float* losses,
                                     void* stream);
int rc_transient_geometry_backward(rc_handle* h, const rc_rays* rays, const float* lossmult, int64_t n, const rc_randoms* rnd,
                                   float anneal, const rc_geometry_loss* cfg, float* sampler_grads, float* losses, void* stream);
int rc_transient_mask_backward(rc_handle* h, const rc_rays* rays, const float* masks, const float* lossmult, int64_t n,
                               const rc_randoms* rnd, float anneal, const rc_mask_loss* cfg, float* sampler_grads, float* loss,
                               void* stream);
int rc_transient_density_regularizer(rc_handle* h, int32_t level, float mult, float* sampler_grads, float* loss, void* stream);
int rc_transient_data_backward_sampler(rc_handle* h, const rc_rays* rays, const float* cam_origins, int64_t n, const rc_randoms* rnd,
                                       const float* gt, const float* rgb_nocorr, const float* gt_nocorr, const float* lossmult,
                                       const rc_transient_data_loss_kind* cfg, float* head_grads, float* sampler_grads,
                                       float* losses, void* stream);

/* ---- evaluation of a rendered view -------------------------------------------------------------------
 * rc_eval_image: what the reference's trainer computes per test view, on images that stay on the device.
 *   post-process (engine/trainer.py:617-637) of pred and gt alike: with n_bins > 0 the arrays are [H][W][n_bins][3] and
 *     x = clip(sum over the bins / img_scale, 0, 1), otherwise [H][W][3]; then linear_to_srgb(x * exposure)
 *     (internal/image_utils.py:192-198, eps = float32's), clipped to [0, 1] only under clip_eval, times mask when given;
 *   mse, psnr = -10 / ln 10 * ln(mse) (image_utils.py:464; the mean runs over all H W 3 values, masked ones included;
 *     mse = 0 gives +inf) and ssim = dm_pix.ssim at its defaults (11 taps, sigma 1.5, k1 0.01, k2 0.03, max_val 1; the
 *     mean of the map over the valid window [H - 10][W - 10][3]) of the two post-processed images;
 *   transient_iou = sum min(pred, gt) / sum max(pred, gt) over the raw histograms (trainer.py:1633-1636), n_bins > 0 only;
 *   l1_mean, l1_median = sum |distance - depth_gt| mask / sum mask, plain means without a mask (trainer.py:1766-1779);
 *   mae: the angle in degrees between normalize(normals_gt + (1 - mask)) and normalize(normals + (1 - acc)), either one
 *     zero where its norm is below 1e-5, times mask, averaged over ALL pixels (trainer.py:1810-1855).
 * Every pointer is a device pointer to float32; mask, acc, the distances and depth_gt are [H][W], the normals [H][W][3].
 * out: DEVICE doubles [RC_EVAL_COUNT], written; a slot whose inputs are NULL is NaN.  Every sum is taken over
 * per-workgroup partials in a fixed order in double: two calls on the same inputs are bitwise equal.  Optional outputs:
 * post_pred / post_gt [H][W][3] (the post-processed images), ssim_map [H - 10][W - 10][3].
 * RC_ERR_INVALID_ARG: NULL images / pred / gt / out, height or width < 11 (no valid window), non-finite or non-positive
 * img_scale, normals without normals_gt or acc, skip_postprocess with n_bins > 0; RC_ERR_UNSUPPORTED: clip_eval with
 * n_bins > 0 (the reference's clip_eval post-process does not sum bins).  Everything is ordered on `stream`; no allocation once the workspace has seen the
 * largest image.  Works on any handle; no weights are needed. */
typedef enum {
  RC_EVAL_MSE = 0,
  RC_EVAL_PSNR,
  RC_EVAL_SSIM,
  RC_EVAL_TRANSIENT_IOU,
  RC_EVAL_L1_MEAN,
  RC_EVAL_L1_MEDIAN,
  RC_EVAL_MAE,
  RC_EVAL_COUNT
} rc_eval_slot;
typedef struct {
  const float* pred;            /* [H][W][3], or [H][W][n_bins][3] with n_bins > 0 */
  const float* gt;              /* as pred */
  const float* mask;            /* [H][W] or NULL */
  const float* acc;             /* [H][W]; needed with normals */
  const float* normals;         /* [H][W][3] or NULL */
  const float* normals_gt;      /* [H][W][3]; needed with normals */
  const float* distance_mean;   /* [H][W] or NULL */
  const float* distance_median; /* [H][W] or NULL */
  const float* depth_gt;        /* [H][W] or NULL (no depth errors) */
  float* post_pred;             /* [H][W][3] written, or NULL */
  float* post_gt;               /* [H][W][3] written, or NULL */
  float* ssim_map;              /* [H - 10][W - 10][3] written, or NULL */
  int32_t height;
  int32_t width;
  int32_t n_bins;               /* 0: pred and gt are images */
  float exposure;               /* Dataset.exposure (1 when the data set has none) */
  float img_scale;              /* Config.img_scale; read with n_bins > 0 only */
  int32_t clip_eval;            /* Config.clip_eval */
  int32_t skip_postprocess;     /* nonzero: pred and gt are compared as they are (image.MetricHarness is called on
                                   post-processed images); n_bins must be 0, exposure and clip_eval are not read */
} rc_eval_images;
int rc_eval_image(rc_handle* h, const rc_eval_images* images, double* out, void* stream);

/* ---- shift-invariant PSNR and SSIM ------------------------------------------------------------------
 * rc_eval_shift_invariant: image_utils.shift_invariant_mse / shift_invariant_ssim (internal/image_utils.py:74-189) of two
 * post-processed images, compared as they are; pred is the reference's im0 (the image that is shifted), gt its im1.
 *   for di = -radius_i .. radius_i (outer), dj = -radius_j .. radius_j (inner):
 *     shifted[y][x] = pred[R_H(y + di)][R_W(x + dj)], R_n(i) = -i below 0 and 2 (n - 1) - i above n - 1 (numpy "reflect");
 *     metric [H][W]: mse: ((d_0^2 + d_1^2) + d_2^2) / 3 of d = shifted - gt; ssim: both images reflect-padded by 5,
 *       dm_pix.ssim's map at its defaults (rc_eval_image's arithmetic) on the [H + 10][W + 10] pair, ((s_0 + s_1) + s_2) / 3;
 *     pooled = the sum of metric over the (2 hw + 1)^2 window, zeros outside the image, along H then along W, taps in
 *       increasing order, divided once by (2 hw + 1)^2;
 *     the first shift is taken; a later one replaces the best at a pixel where pooled >= best (ssim) / pooled <= best
 *       (mse): an exact tie goes to the LATER shift.  A comparison with NaN is false: the earlier shift stays (inputs are
 *       finite by contract).
 *   mse = mean over [H][W] of the chosen shifts' unpooled metric, psnr = -10 / ln 10 * ln(mse) (mse = 0 gives +inf),
 *   ssim = mean of the chosen shifts' unpooled metric over [5, H - 5) x [5, W - 5).
 * out: DEVICE doubles [RC_EVAL_SI_COUNT], written; the SSIM slot is NaN without want_ssim.  Optional DEVICE outputs, each
 * [H][W] or NULL: mse_map / ssim_map (float32, the chosen shifts' unpooled metric), mse_di / mse_dj / ssim_di / ssim_dj
 * (int32, the chosen shift); the ssim ones are not written without want_ssim.  Every sum is taken over per-workgroup
 * partials in a fixed order in double: two calls on the same inputs are bitwise equal, maps and picks included.
 * RC_ERR_INVALID_ARG: NULL images / pred / gt / out, height or width < 11, a negative radius or halfwidth, radius_i >=
 * height or radius_j >= width (one reflection must do); RC_ERR_UNSUPPORTED: a radius above RC_EVAL_SI_MAX_RADIUS or a
 * halfwidth above RC_EVAL_SI_MAX_HALFWIDTH.  Everything is ordered on `stream`; no allocation once the workspace has seen
 * the largest case.  Works on any handle; no weights are needed. */
#define RC_EVAL_SI_MAX_RADIUS 8
#define RC_EVAL_SI_MAX_HALFWIDTH 16
typedef enum {
  RC_EVAL_SI_MSE = 0,
  RC_EVAL_SI_PSNR,
  RC_EVAL_SI_SSIM,
  RC_EVAL_SI_COUNT
} rc_eval_si_slot;
typedef struct {
  const float* pred;            /* [H][W][3] */
  const float* gt;              /* [H][W][3] */
  float* mse_map;               /* [H][W] written, or NULL */
  float* ssim_map;              /* [H][W] written, or NULL */
  int32_t* mse_di;              /* [H][W] written, or NULL */
  int32_t* mse_dj;
  int32_t* ssim_di;
  int32_t* ssim_dj;
  int32_t height;
  int32_t width;
  int32_t radius_i;             /* search_radii[0], along H */
  int32_t radius_j;             /* search_radii[1], along W */
  int32_t window_halfwidth;
  int32_t want_ssim;            /* 0: only the mse search runs */
} rc_eval_si_images;
int rc_eval_shift_invariant(rc_handle* h, const rc_eval_si_images* images, double* out, void* stream);

/* ---- evaluation of the albedo ------------------------------------------------------------------------
 * rc_eval_albedo: Trainer._compute_and_log_albedo_metrics (engine/trainer.py:1499-1567) of one view, on the device.
 *   per pixel, in fp32: in = mask > 0 (no mask: every pixel, mask value 1); valid = in && acc > 0.5; gt' = in ? gt : 1;
 *     p = in ? albedo + (1 - acc) : 1.  The valid rows (gt'[3], p[3]) are compacted in pixel order (numpy's a[mask]).
 *   ratio: the caller's float[3], or (NULL) this view's own per-channel median of gt' / clip(p, 1e-6, 1) over its valid
 *     rows.  The median is exact: (sorted[(M - 1) / 2] + sorted[M / 2]) / 2 in fp32 for an even M, the middle value for
 *     an odd one, NaN for M = 0 or when a ratio of the channel is NaN (np.median of float32).
 *   p = valid ? clip(p ratio, 0, albedo_clip) : p; a = p^(1/2.2), g = gt'^(1/2.2) (powf; a negative base gives NaN);
 *     mse = mean over all 3 H W values of (a m - g m)^2 with the raw mask value m; psnr = -10 / ln 10 * ln(mse).
 *   Every clip hands a NaN on, as np.clip does.
 * out: DEVICE doubles [RC_ALBEDO_COUNT]: mse, psnr, the ratio that was applied, this view's number of valid rows.
 * Optional outputs: post_pred / post_gt [H][W][3] (a and g), ratio_im [H][W][3] = clip(gt' / p, 0, 1) of the uncorrected p.
 * pairs: a caller's buffer [pairs_capacity][6] to which this view's valid rows are APPENDED from row *pairs_count on;
 *   pairs_count is a DEVICE int64 that the call reads and advances by the view's valid rows, and the host never learns it.
 *   A row at an index >= pairs_capacity is not written but still counted: *pairs_count > pairs_capacity afterwards means
 *   overflow, and nothing is stored behind the buffer.  The view is scored either way.
 * rc_albedo_ratio: Trainer._compute_albedo_ratio's ratio (trainer.py:2207-2234) over rows [0, *pairs_count) of such a
 *   buffer -> ratio, DEVICE float[3].  use_median: the exact median as above.  Otherwise the least squares of the
 *   reference's block-diagonal lstsq system in closed form, sums in double: with gamma
 *   (sum p^g gt^g / sum (p^g)^2)^2.2 with g = 1/2.2, without sum p gt / sum p^2.  No rows: NaN.  *pairs_count >
 *   pairs_capacity (overflow): NaN in all three channels, decided on the device.
 * Both calls are ordered on `stream`, never synchronise, allocate nothing once the "ea:" workspace has seen the largest
 * size, use no float atomics (integer counts and double sums in a fixed order: two calls are bitwise equal) and work on
 * any handle.  RC_ERR_INVALID_ARG, with nothing launched: a NULL required pointer, height or width < 1, H W or a
 * capacity >= 2^31, a negative capacity, a non-finite albedo_clip, pairs without pairs_count. */
typedef enum {
  RC_ALBEDO_MSE = 0,
  RC_ALBEDO_PSNR,
  RC_ALBEDO_RATIO_R,
  RC_ALBEDO_RATIO_G,
  RC_ALBEDO_RATIO_B,
  RC_ALBEDO_VALID,              /* this view's valid rows */
  RC_ALBEDO_COUNT
} rc_albedo_slot;
typedef struct {
  const float* albedo;          /* [H][W][3]: the rendering's albedo_rgb / material_albedo */
  const float* acc;             /* [H][W] */
  const float* albedo_gt;       /* [H][W][3] */
  const float* mask;            /* [H][W] or NULL */
  int32_t height;
  int32_t width;
  float albedo_clip;            /* Trainer.albedo_clip */
  const float* ratio;           /* DEVICE float[3], or NULL: this view's own median is used */
  float* post_pred;             /* [H][W][3] written, or NULL */
  float* post_gt;               /* [H][W][3] written, or NULL */
  float* ratio_im;              /* [H][W][3] written, or NULL */
  float* pairs;                 /* [pairs_capacity][6] appended to, or NULL */
  int64_t pairs_capacity;       /* rows */
  int64_t* pairs_count;         /* DEVICE int64, read and advanced; required with pairs */
} rc_albedo_images;
int rc_eval_albedo(rc_handle* h, const rc_albedo_images* images, double* out, void* stream);
int rc_albedo_ratio(rc_handle* h, const float* pairs, int64_t pairs_capacity, const int64_t* pairs_count,
                    int32_t use_median, int32_t gamma, float* ratio, void* stream);

/* ---- visualisation of a rendered view ------------------------------------------------------------------
 * The reference's vis.visualize_suite / visualize_transient_suite (internal/vis.py:319-743) and utils.save_img_u8
 * (internal/utils.py:394-400) on images that stay on the device.
 *
 * rc_weighted_percentile: vis.weighted_percentile (vis.py:50-58) of `n` values with weights, read in float64 with a STABLE
 *   sort (ties stay in pixel order), without a sort.  weight NULL: all ones.  ps: n_ps <= 8 HOST doubles (read before
 *   the call returns); out: DEVICE doubles [n_ps].  With C(v) the weight of the elements
 *   <= v, W the total weight, t = p (W / 100): v1 is the smallest value with C(v1) > t, or, if there is none, the result
 *   is the largest value; B = C(< v1); w_f the weight of the first element in pixel order that equals v1; the result is
 *   v1 if B + w_f <= t or nothing is smaller than v1, otherwise (v1 - v0) / ((B + w_f) - B) * (t - B) + v0 with v0 the
 *   largest value below v1 whatever its weight -- np.interp's arithmetic, in double.  NaN values sort last (one key), -0
 *   and +0 are one key.  A negative, NaN or infinite weight: every result is NaN, decided on the device.
 * rc_image_max: np.max of n floats -> DEVICE float; a NaN is handed on.
 * rc_vis_images: n_items pictures of one view in one call.  Item i reads src ([H][W][channels], or
 *   [H][W][n_bins][channels] for the two bin-summing operations) and computes per value, in fp32,
 *     x = ((src * scale) / divide) / *divisor                  (*divisor: a device float, e.g. an rc_image_max result)
 *     RC_VIS_SRGB              linear_to_srgb(x)                 (image.linear_to_srgb; a NaN is handed on, as jnp.maximum does)
 *     RC_VIS_BINSUM_SRGB       the same of x taken from the sum over the bins
 *     RC_VIS_BINSUM_CLIP_SRGB  linear_to_srgb(clip(x, 0, 1)) of that sum
 *     RC_VIS_MATTE             (exponent != 1 ? x^exponent : x) + offset + (acc ? 1 - acc : 0)      (vis.matte; plain copies)
 *     RC_VIS_ABS               |src| scale / divide / *divisor
 *     RC_VIS_TURBO             vis.visualize_cmap with the depth curve c(x) = -log(x + eps): v = nan_to_num(clip((c(src) -
 *                              min(c(lo), c(hi))) / |c(hi) - c(lo)|, 0, 1)), colour = turbo[min(trunc(256 v), 255)];
 *                              (lo, hi) = bounds[0..1], DEVICE doubles rounded to fp32; a bound that is exactly 0 is
 *                              replaced by auto_bounds[0] - eps / auto_bounds[1] + eps (Python's `lo or ...`) when
 *                              auto_bounds is given.  channels must be 1.
 *   then nan_to_num (when set), then 1 where mask is given and not > 0 (the trainer's masking of the depth pictures).
 *   A one-channel result is broadcast to three.  out_f32 [H][W][3] and / or out_u8 [H][W][3] =
 *   uint8(rint(clip(nan_to_num(y), 0, 1) * 255)) (round half to even) are written.
 * rc_vis_turbo_lut: the 256 x 3 table (matplotlib's "turbo", float32) the device uses.
 * The three device calls are ordered on `stream`, never synchronise, allocate nothing once the "vz:" workspace has seen
 * the largest size, use no float atomics (integer max / min only; floating sums in a fixed order: two calls are bitwise
 * equal) and work on any handle.  RC_ERR_INVALID_ARG, with nothing launched: a NULL required pointer, n < 1, height or
 * width < 1, n or H W >= 2^31, n_ps outside [1, 8], n_items < 1, an item with no output, channels other than 1 or 3,
 * an unknown operation, n_bins > 0 on an operation that does not sum bins (and < 1 on one that does), RC_VIS_TURBO without
 * bounds or with three channels. */
typedef enum {
  RC_VIS_SRGB = 0,
  RC_VIS_BINSUM_SRGB,
  RC_VIS_BINSUM_CLIP_SRGB,
  RC_VIS_MATTE,
  RC_VIS_ABS,
  RC_VIS_TURBO,
  RC_VIS_OP_COUNT
} rc_vis_op;
typedef struct {
  const float* src;             /* [H][W][channels] or [H][W][n_bins][channels] */
  int32_t channels;             /* 1 or 3 */
  int32_t n_bins;               /* > 0 exactly for the bin-summing operations */
  int32_t op;                   /* rc_vis_op */
  int32_t nan_to_num;           /* visualize_suite's closing nan_to_num of the float picture */
  float scale;                  /* multiplied */
  float divide;                 /* divided by (1: none) */
  float offset;                 /* RC_VIS_MATTE */
  float exponent;               /* RC_VIS_MATTE (1: none) */
  const float* divisor;         /* DEVICE float divided by, or NULL */
  const float* acc;             /* [H][W] or NULL: RC_VIS_MATTE adds 1 - acc */
  const float* mask;            /* [H][W] or NULL: the picture is 1 where mask is not > 0 */
  const double* bounds;         /* DEVICE double[2]: RC_VIS_TURBO's lo, hi */
  const double* auto_bounds;    /* DEVICE double[2] or NULL: the drawn image's own 0.5 / 99.5 percentiles */
  float* out_f32;               /* [H][W][3] written, or NULL */
  uint8_t* out_u8;              /* [H][W][3] written, or NULL */
} rc_vis_item;
int rc_weighted_percentile(rc_handle* h, const float* value, const float* weight, int64_t n, const double* ps, int32_t n_ps,
                           double* out, void* stream);
int rc_image_max(rc_handle* h, const float* src, int64_t n, float* out, void* stream);
int rc_vis_images(rc_handle* h, const rc_vis_item* items, int32_t n_items, int32_t height, int32_t width, void* stream);
int rc_vis_turbo_lut(float* out);

/* ---- relighting under an explicit HDR environment image -------------------------------------------------
 * The reference's relighting path: render_eval_fn hands dataset.env_map / env_map_pmf / env_map_pdf / env_map_dirs and
 * albedo_ratio to model.apply (internal/train_utils.py:3796-3812); Model._handle_env_map reads the image through
 * render_utils.get_environment_color instead of the EnvMap MLP (internal/models.py:382-393); under
 * Config.compute_relight_metrics both importance-sampler sets are EnvironmentSampler (render_utils.py:191-252).  Single
 * illumination only (L = 1).
 *
 * rc_set_env_image: binds an image rgb [H][W][3] (DEVICE floats) and, optionally, its sampling tables pmf [H W], pdf [H W],
 *   dirs [H W][3] (all three or none) to the handle.  The handle COPIES what it is given into allocations of its own on
 *   `stream` (the image as a zero-padded RGBA copy, the tables, and safe_log(pmf)), so the caller may free its buffers once
 *   the stream has passed the call.  rgb = NULL unbinds (height, width ignored).  A bind of the size already bound
 *   allocates nothing.  Calls that read the bound image on ANOTHER stream are the caller's to order behind the bind.
 * rc_env_tables: the tables of the reference's dataset loader (internal/datasets.py:2113-2154) from rgb * scale:
 *   pmf = I sin(theta_row) / sum, I = r + g + b, sin(theta_row) = sin(linspace(0.5 / H, pi - 0.5 / H, H)) (the loader's
 *   h_interval is 1 / H; kept), pdf = pmf H W / (2 pi^2 sin(theta_row)), dirs = (cos lng cos lat, sin lng cos lat, sin lat)
 *   on the loader's grid.  The normaliser is summed in double in a fixed order: two calls on one image are bitwise equal.
 * rc_env_lookup: get_environment_color (render_utils.py:1552-1598) of n directions on the bound image -> out_rgb [n][3]:
 *   (x, y, z) <- (d.x, d.z, -d.y), s = sqrt(x^2 + y^2 + 1e-8), phi = atan2(y / (s + 1e-8), x / (s + 1e-8)), theta = atan2(s, z),
 *   row = theta / pi H, col = (-phi + pi) / (2 pi) W, bilinear with zero padding and pixel centres at integer coordinates
 *   (grid_utils.jax_resample_2d, CONSTANT_OUTSIDE).  Texel row i therefore sits at polar angle i pi / H, the last row fades
 *   into the padding, and there is a dark seam at phi = +-pi: the image does not wrap.  A non-finite direction gives a NaN
 *   colour and never a read outside the image.
 * rc_env_pick: jax.random.categorical(key, safe_log(pmf), axis=-2, shape=(1, T, 1)) over the bound pmf -> picks [T] (DEVICE
 *   int32): per pick the argmax over the H W texels of safe_log(pmf) + gumbel, the Gumbel noise of flat element k H W + t of
 *   jax.random.gumbel(key, (1, T, H W, 1)) computed in registers, ties to the lowest texel.  T H W < 2^32, T <= 65535.
 * rc_render_relight: rc_render_material under the bound image.  Same rays, randoms, workspaces, trace and outputs; `args`:
 *   RC_RELIGHT_BRDF  the stage's own importance samplers; only the EnvMap along the secondary rays is replaced by the image
 *                    lookup.  The EnvMap weights are not needed.
 *   RC_RELIGHT_ENV   EnvironmentSampler in both sampler sets (compute_relight_metrics): sample (b, k) of a leg with K samples
 *                    per point takes texel picks[(b K + k) % T], direction dirs[pick] (global, brought into the shading frame
 *                    and back), pdf max(pdf[pick], 0), weight 1, 0 below the horizon.  T must be 256 when (n K) % 256 == 0 and
 *                    n K otherwise, per leg (K = Ks for picks_spec, Kd for picks_diff); the tables must be bound.  The BRDF
 *                    and vMF members of rc_material_randoms and the LightSampler weights are not read.
 *   albedo_ratio     DEVICE float[3] or NULL: albedo <- clip(albedo ratio, 0, 1) at the shading point and in the
 *                    material-only composite (material.py:2106-2116).
 * RC_PASS_ENV_IMAGE (rc_render_rays) composites the bound image on secondary rays the same way.
 * Every call is ordered on `stream`, never synchronises, allocates nothing once the sizes have been seen ("rl:" workspace),
 * uses no float atomics (rc_env_pick: one integer max per wave and pick, order-free) and is refused on a time-resolved
 * handle (RC_ERR_UNSUPPORTED).  n == 0 / T == 0 return RC_OK and write nothing.  RC_ERR_INVALID_ARG: a NULL required pointer,
 * height or width < 1, H W >= 2^31, tables given in part, no image (or no tables) bound where one is read, a non-finite
 * scale, an unknown mode, a T that breaks the rule above (the message names the expected T). */
int rc_set_env_image(rc_handle* h, const float* rgb, const float* pmf, const float* pdf, const float* dirs, int32_t height,
                     int32_t width, void* stream);
int rc_env_tables(rc_handle* h, const float* rgb, int32_t height, int32_t width, float scale, float* pmf, float* pdf,
                  float* dirs, void* stream);
int rc_env_lookup(rc_handle* h, const float* viewdirs, int64_t n, float* out_rgb, void* stream);
int rc_env_pick(rc_handle* h, const uint32_t key[2], int32_t T, int32_t* picks, void* stream);
typedef enum { RC_RELIGHT_BRDF = 0, RC_RELIGHT_ENV = 1 } rc_relight_mode;
typedef struct {
  uint32_t mode;                 /* rc_relight_mode */
  const int32_t* picks_spec;     /* DEVICE [T_spec] texel indices of the specular leg (RC_RELIGHT_ENV) */
  const int32_t* picks_diff;     /* DEVICE [T_diff] texel indices of the diffuse leg (RC_RELIGHT_ENV) */
  int32_t T_spec, T_diff;
  const float* albedo_ratio;     /* DEVICE [3] or NULL */
} rc_relight_args;
int rc_render_relight(rc_handle* h, const rc_rays* rays, int64_t n_rays, const rc_randoms* rnd,
                      const rc_material_randoms* mr, int32_t num_secondary_samples, const rc_relight_args* args,
                      const rc_outputs* cache_out, const rc_mat_outputs* mat_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The probe of a surface point: the `vis_secondary` block of the reference's evaluation loop
 * (engine/trainer.py:848-1069) for P <= RC_PROBE_MAX selected pixels of a rendered view in one launch each.
 *
 * rc_probe_rays: the rays of P latitude-longitude panoramas of height x width pixels, probe-major (ray
 *   (p height + row) width + col), cast from the hit points of the view's rows pixel[0 .. P):
 *     position = origins + directions * distance_median + normal_offset * normals      (trainer.py:863-871; the
 *                reference's offset is 4e-1);  origins = position, near / far as given;
 *     radii    = those of camera_utils.cast_spherical_rays around `position` with the identity rotation (the reference
 *                overwrites its rotation matrix with np.eye(3), :874-882): bitwise what rc_cast_rays writes for camtype 1,
 *                pixtocam = diag(2 pi / width, pi / height, 1).  They belong to the panoramic direction of the pixel, not
 *                to the direction the ray carries: the reference's mismatch, kept;
 *     directions = viewdirs = utils.get_sphere_directions(height, width, flip) (internal/utils.py:55-83;
 *                _update_secondary_rays, :934-942);
 *     lights, imageplane, look, up = row 0 of the view's arrays (:944-1012); for a NULL member of rc_probe_view the
 *                panoramic cast's own value stays: its image plane, look (0, 0, -1), up (0, 1, 0), and `position` as the
 *                light (the camera centre, as rc_camera_set's NULL lights).
 *   `pixel` is a HOST array of P rows of the view; `out` members may be NULL (not wanted), `positions` too.
 * rc_vmf_panorama: render_vmf (:1026-1069) of P mixtures of V <= RC_PROBE_MAX_LOBES lobes over the same panorama:
 *     mean_j = means_j / max(|means_j|, 1e-5),  w_j = safe_exp(logits_j) / sum_j safe_exp(logits_j)  (math.safe_exp, the
 *     clip at 70),  L = sum_j w_j eval_vmf(xyz, mean_j, kappas_j)  (render_utils.py:1335-1346: 1 / 4 pi for kappa <=
 *     FLT_EPSILON, its own safe_exp = exp(min(x, 80))), summed over j ascending in fp32;
 *     out_linear = L, out_srgb = image.linear_to_srgb(L) in three channels, out_u8 = utils.save_img_u8's 8-bit form of
 *     out_srgb.  Each output may be NULL, not all of them; one requested alone is bitwise what it is with the others.
 * Both calls work on any handle, are ordered on `stream`, never synchronise, allocate nothing and use no atomics.
 * RC_ERR_INVALID_ARG, with nothing launched: P < 1 or P > RC_PROBE_MAX, a pixel outside [0, n_view), height or width < 1,
 * P height width >= 2^31, V < 1 or V > RC_PROBE_MAX_LOBES, a NULL required pointer (view, its first four members, pixel,
 * out; means, kappas, logits), no output requested.
 * ------------------------------------------------------------------------------------------------ */
#define RC_PROBE_MAX 16
#define RC_PROBE_MAX_LOBES 128
typedef struct rc_probe_view {        /* DEVICE arrays of the rendered view, or of any subset of its pixels */
  const float* origins;               /* [n_view,3] primary rays                                            */
  const float* directions;            /* [n_view,3]                                                         */
  const float* distance_median;       /* [n_view]   rendering["distance_median"]                            */
  const float* normals;               /* [n_view,3] rendering["normals_to_use"]                             */
  const float* lights;                /* [>= 1,3] or NULL                                                   */
  const float* imageplane;            /* [>= 1,2] or NULL                                                   */
  const float* look;                  /* [>= 1,3] or NULL                                                   */
  const float* up;                    /* [>= 1,3] or NULL                                                   */
  int64_t n_view;
} rc_probe_view;
int rc_probe_rays(rc_handle* h, const rc_probe_view* view, const int64_t* pixel, int32_t P, int32_t height, int32_t width,
                  float near, float far, float normal_offset, int32_t flip, const rc_cast_outputs* out, float* positions,
                  void* stream);
int rc_vmf_panorama(rc_handle* h, const float* means, const float* kappas, const float* logits, int32_t P, int32_t V,
                    int32_t height, int32_t width, int32_t flip, float* out_linear, float* out_srgb, uint8_t* out_u8,
                    void* stream);

/* -- surface export: the handle's fields at arbitrary points, the density on a lattice, and the
 * isosurface of any device lattice as a triangle mesh.
 *
 * rc_query_points: points [n,3] world coordinates on the device; every output is nullable.
 *   density [n]         predict_density of sampler level `level` (level < 0: the last): the grid lookup with the
 *                       contraction, density_layers_*, output_density_layer, safe_exp(raw + density_bias), gated to 0 outside
 *                       the contracted box -- what the launch-per-stage level path computes for its sample means
 *   normals_pred [n,3]  nan_to_num(-l2_normalize(pred_normals_layer(h))), last level only
 *   normals [n,3]       the analytic normals nan_to_num(-l2_normalize(d raw / d x)), last level only; neither is rectified
 *                       (there is no view direction)
 *   material [n,5]      albedo rgb, roughness, metalness of the material head on the material grid's features
 * The existing forward kernels run on chunks of 131 072 points, so the workspace ("q:" names of rc_workspace_ptr: "means"
 * (SoA [3][C] of the last chunk), "feat", "jac", "density", "normals_pred", "normals_grad", "m_feat") is bounded whatever n is.
 * RC_ERR_INVALID_ARG: n < 0, NULL points with n > 0, level >= num_levels.  RC_ERR_UNSUPPORTED: normals_pred / normals on
 * another level than the last, material on a time-resolved handle (which is accepted for the other three outputs).
 * RC_ERR_MISSING_WEIGHT: material without the material weights, a missing grid table.  n == 0 returns RC_OK and launches
 * nothing.  Everything is ordered on `stream`.
 *
 * rc_density_lattice: field [nx,ny,nz] on the device, row-major with iz fastest (the `ij` meshgrid of the reference's
 * mesh script); lo / hi: HOST float[3].  Point i of axis a sits at lo[a] + (float)i * ((hi[a] - lo[a]) / (float)(n_a - 1)),
 * evaluated in fp32 in exactly this form (linspace up to its last bits; torch.linspace's two-sided formula differs there, on
 * purpose).  The value is rc_query_points' density with nan_to_num applied; the points are generated on the device slab by
 * slab ("q:" workspace, it does not grow with the lattice).  RC_ERR_INVALID_ARG: a dimension outside 2 .. 1024,
 * hi[a] <= lo[a], level >= num_levels, NULL field.
 *
 * rc_isosurface: marching tetrahedra on the Kuhn decomposition of every lattice cell (csrc/rc_iso_table.h states the
 * rule).  field: ANY device lattice in the layout above.  A point is inside when f >= iso (a NaN is outside).  One vertex per
 * lattice edge, face diagonal or body diagonal of the decomposition whose ends differ, numbered by (lower end's linear index,
 * direction number); position by linear interpolation with the parameter clamped to [0, 1]; normals (nullable, [V,3]) =
 * -normalize of the lattice's central-difference gradient (one-sided at the border) interpolated the same way, (0,0,0) for a
 * zero gradient.  Triangles [T,3] int32 in cell order, oriented so that their normals point towards lower field values.
 * counts: device int64[2] = {V, T}, always written.  vertices / normals / triangles are written only if V <= v_capacity and
 * T <= t_capacity; otherwise only counts is written and the call still returns RC_OK -- call with capacities 0, read
 * counts, allocate, call again.  No atomics: two calls on one lattice give bitwise the same arrays.
 * RC_ERR_INVALID_ARG: a dimension outside 2 .. 1024, hi[a] <= lo[a], NULL field / counts, a NaN iso, a negative capacity,
 * v_capacity > INT32_MAX, a NULL array with a non-zero capacity.  Workspace: "iso:" names "mask", "tcount" (bytes per lattice
 * point), "vbase" (int32 per point), "tile_v", "tile_t", "group_v", "group_t", "group_off", "state". */
int rc_query_points(rc_handle* h, const float* points, int64_t n, int32_t level, float* density, float* normals_pred,
                    float* normals, float* material, void* stream);
int rc_density_lattice(rc_handle* h, const float* lo, const float* hi, int32_t nx, int32_t ny, int32_t nz, int32_t level,
                       float* field, void* stream);
int rc_isosurface(rc_handle* h, const float* field, int32_t nx, int32_t ny, int32_t nz, float iso, const float* lo,
                  const float* hi, float* vertices, float* normals, int64_t v_capacity, int32_t* triangles,
                  int64_t t_capacity, int64_t* counts, void* stream);

/* -- textured export: a per-triangle texture atlas of a device mesh, baked from the handle's fields.
 *
 * The layout, for T >= 1 triangles and a cell of r x r texels, 4 <= r <= 64.  Two triangles share one square cell:
 * ncells = ceil(T / 2), cols = the smallest integer with cols^2 >= ncells, rows = ceil(ncells / cols), W = cols r,
 * H = rows r (both at most 16384).  Texel (x, y), x from the left and y from the top, is image element [y, x] and linear
 * index y W + x.  cx = x / r, cy = y / r, cell = cy cols + cx, i = x - cx r, j = y - cy r, half = (i + j >= r),
 * t = 2 cell + half; the texel is empty when cell >= ncells or t >= T.  Barycentrics of the texel centre: half 0
 * b1 = i / (r - 2), b2 = j / (r - 2); half 1 b1 = (r - 1 - i) / (r - 3), b2 = (r - 1 - j) / (r - 3) (one fp32 division
 * each); its world point p = V0 + b1 (V1 - V0) + b2 (V2 - V0) in fp32 in this form.  Corners in local texel units (a
 * texel's centre at (i + 0.5, j + 0.5)): half 0 (0.5, 0.5), (r - 1.5, 0.5), (0.5, r - 1.5); half 1 (r - 0.5, r - 0.5),
 * (2.5, r - 0.5), (r - 0.5, 2.5).  Every bilinear tap of non-zero weight at a uv inside a triangle's uv triangle falls
 * on a texel that triangle owns, so nearest and bilinear sampling never mix two triangles (mip-mapping would).
 *
 * rc_atlas_layout: host only; dims = {cols, rows, W, H}.  RC_ERR_INVALID_ARG: NULL dims, T < 1, r outside 4 .. 64;
 *   RC_ERR_UNSUPPORTED: W or H above 16384.  The other calls refuse the same way.
 * rc_atlas_uvs: uvs [T,3,2] on the device, the normalised (u, v) = (X / W, 1 - Y / H) of each triangle's corners at
 *   global texel coordinates (X, Y) -- the `vt` lines of an OBJ file.
 * rc_atlas_points: the texels with linear index first .. first + count - 1: points [count,3] (nullable) and owner [count]
 *   (nullable): the triangle index, -1 for an empty texel, -2 where the triangle has a vertex index outside 0 .. V - 1
 *   (such a triangle is never dereferenced); the point of a texel without an owner is (0, 0, 0).  vertices [V,3] float,
 *   triangles [T,3] int32 on the device.  RC_ERR_INVALID_ARG: a NULL mesh array, V < 1, first < 0, count < 0,
 *   first + count > W H.  count == 0 returns RC_OK and launches nothing.
 * rc_query_cache_diffuse: diffuse [n,6] = ambient_diffuse rgb, indirect_diffuse rgb of the cache's shader at points [n,3]:
 *   clip(softplus(Dense(96 -> 3)(feature) + bias), 0, rgb_max) of ambient_irradiance_layer / irradiance_layer on the feature
 *   [the last sampler level's hidden vector (64) | the appearance grid's features at the contracted point (32)] -- what the
 *   launch-per-stage plan's shader computes as ambient_diffuse_rgb / indirect_diffuse_rgb for a sample with that mean.  No
 *   gate: like that shader, a point beyond the contracted box gets the heads' value on the features looked up at its
 *   contracted position (only the density is gated there).  RC_ERR_UNSUPPORTED on a time-resolved handle.
 * rc_bake_atlas: every non-NULL plane of `out` for the whole atlas, chunk by chunk of rc_query_points' chunk size: the
 *   texels' points, the launches of rc_query_points / rc_query_cache_diffuse on them, zeros where a texel has no owner.  A
 *   baked texel equals rc_query_points (rc_query_cache_diffuse) at that texel's point bit for bit.  `level` as in
 *   rc_query_points.  Workspace: the "q:" names and "atlas:" names "points", "owner", "hidden", "app_feat", none of which grows
 *   with the atlas.  No atomics; everything is ordered on `stream`, nothing waits for the device. */
typedef struct {
  float* density;          /* [H,W] */
  float* normals_pred;     /* [H,W,3] */
  float* normals;          /* [H,W,3] */
  float* material;         /* [H,W,5] */
  float* diffuse;          /* [H,W,6] */
  uint8_t* coverage;       /* [H,W]: 1 where a triangle owns the texel */
} rc_atlas_outputs;
int rc_atlas_layout(int64_t T, int32_t r, int32_t dims[4]);
int rc_atlas_uvs(rc_handle* h, int64_t T, int32_t r, float* uvs, void* stream);
int rc_atlas_points(rc_handle* h, const float* vertices, int64_t V, const int32_t* triangles, int64_t T, int32_t r,
                    int64_t first, int64_t count, float* points, int32_t* owner, void* stream);
int rc_query_cache_diffuse(rc_handle* h, const float* points, int64_t n, float* diffuse, void* stream);
int rc_bake_atlas(rc_handle* h, const float* vertices, int64_t V, const int32_t* triangles, int64_t T, int32_t r,
                  int32_t level, const rc_atlas_outputs* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RC_ABI_H_ */
