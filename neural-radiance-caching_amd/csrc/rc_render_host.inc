// The render sequencer (included by rc_api.hip): which kernels one cache pass launches, in which order.
//
// RenderArgs describes a pass; enqueue_all picks its launch plan and runs it stage by stage: 3 x [resample -> grid lookup
// -> density MLP] -> (categorical resample) -> appearance grid -> cache shader -> volume compositing (BaseNeRFModel.__call__,
// internal/models.py:657-774), or the fused kernel in their place.  rc_render_rays / rc_render_chunks are its entry points;
// the material stage, the time-resolved cache and the cache losses' training forwards enqueue their passes through it too.

namespace {

// Where a pass stops.
enum RenderStop {
  RENDER_FULL,
  RENDER_WEIGHTS,   // weights_only=True (models.py:944-982): no shader; only acc = sum of the last level's weights is consumed
  RENDER_LEVELS,    // rc_geometry_backward's training forward: the sampler levels with the last level's hidden vector,
                    // predicted and analytic normals (force_grad), nothing behind them
  RENDER_SAMPLER    // rc_interlevel_backward's / rc_mask_backward's training forward: the sampler levels only (sdist / tdist /
                    // means / density / weights of every level in the workspace, nothing behind them)
};

// Work released on a side stream behind what the caller's stream holds so far: the EnvMap MLP (or, `lookup` set, the bound
// image's lookup) along the material stage's secondary rays.  material_render owns it; handed to the trace (RenderArgs::env)
// it is released when the LAST proposal level is launched, which leaves `reserve` CUs to it (both kernels keep a CU's LDS
// to themselves; see material_render).
struct SideEnv {
  RcEnvMapArgs map; const RcEnvLookupArgs* lookup;
  hipStream_t side; hipEvent_t ready, done;
  int reserve;
  bool released;     // set by side_release (the trace's launch plan may not have the spot: the owner releases it itself then)
};
// Record on the caller's stream, make the side stream wait, launch, record on the side stream.
hipError_t side_release(SideEnv& e, hipStream_t st) {
  hipError_t err;
  if ((err = hipEventRecord(e.ready, st)) != hipSuccess || (err = hipStreamWaitEvent(e.side, e.ready, 0)) != hipSuccess) return err;
  if (e.lookup) rc_launch_env_lookup(*e.lookup, e.side); else rc_launch_envmap(e.map, e.side);
  e.released = true;
  return hipEventRecord(e.done, e.side);
}

struct RenderArgs {
  rc_rays rays; rc_randoms rnd; bool have_rnd; int64_t n; uint32_t mask; rc_outputs out; int slot; bool fused;
  const rc_transient_outputs* tout = nullptr; const float* cam_origins = nullptr;
  const rc_randoms* shadow_rnd = nullptr; bool force_grad = false;
  const rc_transient_slices* tslices = nullptr;   // rc_render_transient_slices: k_transient_slice in place of k_transient_bins
  RenderStop stop = RENDER_FULL;
  float anneal = -1.0f;            // resampling at `anneal` (< 0: the config's render-time value)
  bool export_samples = false;     // fused plan: leave tdist / density / means / normals_pred of the last level in the workspace
  const float* s_bounds = nullptr; // secondary rays with ONE (near, far): power-ladder bounds computed once (RcSampleArgs)
  SideEnv* env = nullptr;          // material stage: released beside the last proposal level (SideEnv)
};

// The cache pass on these rays with these randoms: RC_PASS_CACHE, launch per stage, no profiling slot, no output yet.
RenderArgs cache_pass(const rc_rays* rays, const rc_randoms* rnd, int64_t n) {
  RenderArgs A{};
  A.rays = *rays;
  A.have_rnd = rnd != nullptr;
  if (rnd) A.rnd = *rnd;
  A.n = n; A.mask = RC_PASS_CACHE; A.slot = -1; A.fused = false;
  return A;
}

// What the stages of one pass share besides its RenderArgs.
struct RenderPlan {
  bool secondary, resample;
  bool lean;      // no per-sample consumer of the last level's hidden feature / predicted normals besides the shader
};

void enqueue_transient_tail(rc_handle* h, const RenderArgs& A, RenderWs& w, hipStream_t st);      // rc_transient_host.inc

// Secondary rays: rgb += env * (1 - acc) (Model._composite_env_map, internal/models.py:423-460).
__global__ void k_env_combine(int64_t n, const float* rgb_noenv, const float* acc, const float* env, float* rgb_out,
                              float* acc_out, float* env_out, float* noenv_out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const float a = acc[r];
  if (acc_out) acc_out[r] = a;
  for (int c = 0; c < 3; ++c) {
    const float base = rgb_noenv[3 * r + c];
    const float e = env ? env[3 * r + c] : 0.0f;
    if (rgb_out) rgb_out[3 * r + c] = env ? base + e * (1.0f - a) : base;
    if (env_out) env_out[3 * r + c] = e;
    if (noenv_out) noenv_out[3 * r + c] = base;
  }
}

// The compositing kernel's arguments over the last level in `w`: `picked` = the one resampled sample per ray is shaded
// (all S otherwise), `pred` = the predicted normals of all samples are in the workspace.
RcCompositeArgs composite_args(rc_handle* h, const RenderArgs& A, RenderWs& w, bool picked, bool pred, float bg) {
  const rc_config& c = h->cfg;
  const int NL = c.num_levels;
  const int S2 = c.num_samples[NL - 1];
  RcCompositeArgs ca{};
  ca.directions = A.rays.directions; ca.origins = A.rays.origins; ca.lights = A.rays.lights; ca.n_rays = A.n; ca.S = S2;
  ca.tdist = w.tdist[NL - 1].p; ca.density = w.density[NL - 1].p; ca.means = w.means[NL - 1].p;
  ca.normals_pred = pred ? w.normals_pred.p : nullptr;
  ca.normals_grad = A.out.ptr[RC_OUT_NORMALS] ? w.normals_grad.p : nullptr;
  ca.shade = w.shade.p; ca.Sf = picked ? 1 : S2;
  ca.inds = picked ? (const int32_t*)w.inds.p : nullptr; ca.filt_weight = picked ? w.filt_weight.p : nullptr;
  ca.weights = w.weights[NL - 1].p;
  ca.bg = bg;
  ca.pct[0] = c.percentiles[0]; ca.pct[1] = c.percentiles[1]; ca.pct[2] = c.percentiles[2];
  ca.out = A.out;
  return ca;
}

// What every fused launch takes from the pass: rays, n, jitter.
void fused_pass(RcFusedLaunch& F, const RenderArgs& A) {
  F.rays = A.rays; F.n = A.n;
  for (int l = 0; l < 3; ++l) F.jitter[l] = A.have_rnd ? A.rnd.jitter[l] : nullptr;
}

// The fused whole-pass launch.
void stage_fused(rc_handle* h, const RenderArgs& A, RenderWs& w, hipStream_t st) {
  const int NL = h->cfg.num_levels;
  // everything of the launch that only changes when weights are (re)packed was resolved then (build_fused_template)
  RcFusedLaunch F = h->fused_tmpl;
  fused_pass(F, A);
  F.out = A.out;
  // mode 3: the one-wavefront-per-ray form.  Builds with the split-MFMA shader (RC_SPLIT_MFMA) run it for mode 1 as well:
  // the two-wave kernel was unstable with the split form in every layer (rc_dev_mlp.h INSTABILITY; cause not found)
  // (a split build compiles the two-wave kernel only under -DRC_TEAM_SPLIT_DIAG, for diagnosis: rc_pack_host.h RC_TEAM_KERNEL)
  F.team = (h->fused_mode == 1 && RC_TEAM_KERNEL) ? 1 : 0;
  F.prio_mode = h->fused_prio;
  if (A.export_samples) {
    F.export_samples = 1;
    F.f_tdist = w.tdist[NL - 1].p; F.f_density = w.density[NL - 1].p; F.f_means = w.means[NL - 1].p; F.f_normals_pred = w.normals_pred.p;
  }
  // profiling: the single launch is reported as the "shader" stage, every other stage as 0
  for (int i = 0; i <= ST_SHADER; ++i) stage_mark(h, A.slot, i, st);
  roctx_stage(F.team ? "k_cache_fused_team" : "k_cache_fused");
  rc_launch_fused(F, st);
  for (int i = ST_SHADER + 1; i <= ST_COUNT; ++i) stage_mark(h, A.slot, i, st);
}

// The fused front end (time-resolved cache on primary rays): the whole proposal sampler + appearance lookup as ONE launch
// (the FRONT variant of the fused kernel), results in the workspace buffers the stages behind it read.
void stage_fused_front(rc_handle* h, const RenderArgs& A, RenderWs& w, hipStream_t st) {
  const rc_config& c = h->cfg;
  const int NL = c.num_levels;
  RcFusedLaunch F = fused_front_end(h);
  fused_pass(F, A);
  F.wstream = h->packs.fused_front.p;
  F.front = 1;
  F.want_grad = (A.out.ptr[RC_OUT_NORMALS] != nullptr || A.force_grad) ? 1 : 0;
  F.use_raydist = 1; F.raydist_p = c.raydist_p; F.raydist_premult = c.raydist_premult;   // TransientNeRFModel (see sample_args)
  F.f_tdist = w.tdist[NL - 1].p; F.f_density = w.density[NL - 1].p; F.f_means = w.means[NL - 1].p;
  F.f_normals_pred = w.normals_pred.p; F.f_normals_grad = w.normals_grad.p; F.f_hbuf = w.hbuf.p; F.f_app = w.app.p;
  rc_launch_fused(F, st);
}

// Level l's resampling of the level before (level 0: of the ray's [near, far]).
RcSampleArgs sample_args(rc_handle* h, const RenderArgs& A, const RenderPlan& P, RenderWs& w, int l) {
  const rc_config& c = h->cfg;
  const rc_rays* rays = &A.rays;
  RcSampleArgs sa{};
  sa.origins = rays->origins; sa.directions = rays->directions; sa.viewdirs = rays->viewdirs;
  sa.near = rays->near; sa.far = rays->far; sa.normals = rays->normals; sa.n_rays = A.n;
  if (l > 0) {
    sa.prev_sdist = w.sdist[l - 1].p; sa.prev_tdist = w.tdist[l - 1].p; sa.prev_density = w.density[l - 1].p;
    sa.P = c.num_samples[l - 1]; sa.prev_weights = w.weights[l - 1].p;
  } else {
    sa.P = 1;
  }
  sa.S = c.num_samples[l];
  sa.jitter = A.have_rnd ? A.rnd.jitter[l] : nullptr;
  sa.sdist = w.sdist[l].p; sa.tdist = w.tdist[l].p; sa.means = w.means[l].p;
  sa.anneal = A.anneal >= 0.0f ? A.anneal : c.anneal; sa.padding = c.resample_padding;
  sa.secondary = P.secondary ? 1 : 0;
  sa.use_raydist = (P.secondary || h->transient) ? 1 : 0;     // TransientNeRFModel: use_raydist_for_secondary_only = False
  sa.raydist_p = c.raydist_p; sa.raydist_premult = c.raydist_premult;
  sa.eps_dot_min = c.shadow_normal_eps_dot_min; sa.far_clamp = c.env_map_distance;
  sa.s_bounds = (P.secondary && !rays->normals) ? A.s_bounds : nullptr;
  return sa;
}

// Level l's grid lookup + density MLP as one launch (rc_level.hip), on its np samples.
RcLevelArgs level_args(rc_handle* h, RenderWs& w, int l, int64_t np) {
  const rc_config& c = h->cfg;
  RcLevelArgs la{};
  la.grid = &h->grids[l].dev; la.means = w.means[l].p; la.n = np; la.wstream = h->packs.dens[l].p;
  la.density_bias = c.density_bias; la.contract_radius = c.contract_radius; la.density = w.density[l].p;
  return la;
}

// Level l's density MLP behind the launch-per-stage grid lookup; `per_sample`: the last level also leaves its hidden
// feature and predicted normals for all samples.
RcDensityMlpArgs density_args(rc_handle* h, RenderWs& w, int l, int64_t np, bool per_sample, bool want_grad) {
  const rc_config& c = h->cfg;
  RcDensityMlpArgs da{};
  da.feat = w.feat[l].p; da.n = np; da.ld = np;
  da.K = h->grids[l].dev.num_levels * h->grids[l].dev.num_features;
  da.wstream = h->packs.dens[l].p; da.means = w.means[l].p;
  da.density_bias = c.density_bias; da.contract_radius = c.contract_radius; da.bbox = h->grids[l].cfg.bbox;
  da.last = (l == c.num_levels - 1) ? 1 : 0; da.density = w.density[l].p;
  da.hbuf = (da.last && per_sample) ? w.hbuf.p : nullptr;
  da.normals_pred = (da.last && per_sample) ? w.normals_pred.p : nullptr;
  da.jac = want_grad ? w.jac.p : nullptr; da.normals_grad = want_grad ? w.normals_grad.p : nullptr;
  return da;
}

// The level loop: per level sampling, grid lookup and density MLP, as one, two or three launches.
void stage_levels(rc_handle* h, const RenderArgs& A, const RenderPlan& P, RenderWs& w, hipStream_t st) {
  const rc_config& c = h->cfg;
  const int NL = c.num_levels;
  const int64_t n = A.n;
  const int slot = A.slot;
  for (int l = 0; l < NL; ++l) {
    const int S = c.num_samples[l];
    const int64_t np = n * S;
    const RcSampleArgs sa = sample_args(h, A, P, w, l);
    const bool want_grad = (l == NL - 1) && (A.out.ptr[RC_OUT_NORMALS] != nullptr || A.force_grad);
    // only the density of this level's samples is consumed behind it (proposal levels; the last level on the lean
    // resampling pass): grid lookup + density MLP as ONE launch, weights resident in LDS (rc_level.hip) -- and on the
    // default plan (rc_set_fused 1) the level's sampling in front of it in the same launch, one ray per wave
    const bool level_kernel = h->fused_mode != 0 && !h->profiling && rc_level_supported(h->grids[l].dev) && !want_grad &&
                              (l < NL - 1 || (P.lean && !A.tout));
    RcLevelArgs la = level_args(h, w, l, np);
    // (one ray per wave pays from ~100 rays per CU on: measured break-even of the whole pass near 32 k rays, +27 us at 1-4 k)
    if (level_kernel && (h->fused_mode == 1 || h->fused_mode == 3) && n >= 24576 && rc_level_ray_supported(h->grids[l].dev, S)) {
      roctx_stage(l == 0 ? "level0 (sample+grid+mlp)" : (l == 1 ? "level1 (sample+grid+mlp)" : "level2 (sample+grid+mlp)"));
      if (A.env && l == NL - 1) {
        (void)side_release(*A.env, st);
        la.cu_reserve = A.env->reserve;
      }
      rc_launch_level_ray(la, sa, st);
      continue;
    }
    stage_mark(h, slot, ST_SAMPLE0 + 3 * l, st);
    rc_launch_sample(sa, st);

    stage_mark(h, slot, ST_GRID0 + 3 * l, st);
    if (level_kernel) {
      stage_mark(h, slot, ST_MLP0 + 3 * l, st);
      rc_launch_level(la, st);
      continue;
    }
    rc_launch_hashgrid(h->grids[l].dev, w.means[l].p, 1, np, w.feat[l].p, 1, np, c.contract_radius, want_grad ? w.jac.p : nullptr, st);

    // lean resampling pass: the hidden feature / predicted normals are only needed at the ONE sample per ray picked
    // behind the levels, so they are not written for all of them here (256 + 12 bytes per sample) but recomputed for the picks
    const RcDensityMlpArgs da = density_args(h, w, l, np, !P.lean && A.stop != RENDER_SAMPLER, want_grad);
    stage_mark(h, slot, ST_MLP0 + 3 * l, st);
    rc_launch_density_mlp(da, st);
  }
}

// The pick: the categorical resample, on the lean pass the last level's density MLP once more on the picked samples, and
// the appearance lookup (with the pair tables: both lookups in one pass).
void stage_pick(rc_handle* h, const RenderArgs& A, const RenderPlan& P, RenderWs& w, hipStream_t st) {
  const rc_config& c = h->cfg;
  const int NL = c.num_levels;
  const int S2 = c.num_samples[NL - 1];
  const int64_t n = A.n, np2 = n * S2;
  stage_mark(h, A.slot, ST_RESAMPLE, st);
  const int32_t* src = nullptr;
  if (P.resample) {
    RcResampleArgs ra{};
    ra.n_rays = n; ra.S = S2; ra.tdist = w.tdist[NL - 1].p; ra.density = w.density[NL - 1].p;
    ra.directions = A.rays.directions; ra.gumbel = A.rnd.gumbel; ra.inds_in = A.rnd.resample_inds;
    ra.inds_out = (int32_t*)w.inds.p; ra.filt_weight = w.filt_weight.p; ra.weights = w.weights[NL - 1].p;
    ra.acc_out = w.acc_sel.p; ra.src_out = (int32_t*)w.src_idx.p;
    rc_launch_resample(ra, st);
    src = (const int32_t*)w.src_idx.p;
  }
  const int64_t nsh = P.resample ? n : np2;
  bool pair_lookup = false;
  if (P.lean) {
    // density MLP of the last level once more, on the picked samples only (same kernel, same per-point arithmetic:
    // bitwise the values the full pass would have stored), compact outputs
    const int l2 = NL - 1;
    const int K2 = h->grids[l2].dev.num_levels * h->grids[l2].dev.num_features;
    // with the fused plan's interleaved tables at hand: this lookup and the appearance lookup below in one pass
    pair_lookup = h->fused_ok && l2 == 2 && nsh == n && h->fused_mode != 0;
    if (pair_lookup) {
      RcPairTables pt{};
      for (int l = 0; l < h->grids[2].dev.num_levels; ++l) pt.t[l] = h->fused_tmpl.pair_table[l];
      rc_launch_hashgrid_pair(h->grids[2].dev, pt, w.means[NL - 1].p, src, np2, n, w.feat_sel.p, w.app.p, n, c.contract_radius, st);
    } else {
      rc_launch_hashgrid_src(h->grids[l2].dev, w.means[NL - 1].p, 1, src, np2, n, w.feat_sel.p, 1, n, c.contract_radius, nullptr, st);
    }
    RcDensityMlpArgs ds{};
    ds.feat = w.feat_sel.p; ds.n = n; ds.ld = n; ds.K = K2; ds.wstream = h->packs.dens[NL - 1].p;
    ds.means = w.means[NL - 1].p; ds.src = src; ds.n_src = np2;
    ds.density_bias = c.density_bias; ds.contract_radius = c.contract_radius; ds.bbox = h->grids[l2].cfg.bbox;
    ds.last = 1; ds.density = w.density_sel.p; ds.hbuf = w.hbuf_sel.p; ds.normals_pred = w.normals_sel.p;
    rc_launch_density_mlp(ds, st);
  }
  stage_mark(h, A.slot, ST_GRID_APP, st);
  if (!pair_lookup)
    rc_launch_hashgrid_src(h->grids[3].dev, w.means[NL - 1].p, 1, src, np2, nsh, w.app.p, 1, nsh, c.contract_radius, nullptr, st);
}

// Shade (the picked sample of each ray, or all samples) and composite.
void stage_shade_composite(rc_handle* h, const RenderArgs& A, const RenderPlan& P, RenderWs& w, hipStream_t st) {
  const rc_config& c = h->cfg;
  const int S2 = c.num_samples[c.num_levels - 1];
  const int64_t n = A.n, np2 = n * S2;
  const bool lean = P.lean;
  stage_mark(h, A.slot, ST_SHADER, st);
  {
    RcShaderArgs s{};
    s.n = P.resample ? n : np2; s.n_src = lean ? n : np2; s.samples_per_ray = P.resample ? 1 : S2;
    s.src = (lean || !P.resample) ? nullptr : (const int32_t*)w.src_idx.p;
    s.hbuf = (lean ? w.hbuf_sel : w.hbuf).p; s.app = w.app.p;
    s.normals_pred = (lean ? w.normals_sel : w.normals_pred).p; s.viewdirs = A.rays.viewdirs;
    s.wstream = h->packs.shader.p; s.ide_coef = h->ide_table.p;
    s.roughness_bias = c.roughness_bias; s.irradiance_bias = c.irradiance_bias; s.ambient_bias = c.ambient_irradiance_bias;
    s.rgb_max = c.rgb_max; s.slf_ambient_bias = c.slf_ambient_bias;
    s.shade = w.shade.p; s.debug = w.debug.p;
    rc_launch_shader(s, st);
  }
  stage_mark(h, A.slot, ST_COMPOSITE, st);
  RcCompositeArgs ca = composite_args(h, A, w, P.resample, !lean, P.secondary ? 0.0f : c.bg_intensity);
  if (P.secondary) { ca.out.ptr[RC_OUT_RGB] = w.rgb_noenv.p; ca.out.ptr[RC_OUT_ACC] = w.acc_ws.p; }
  // one resampled sample per ray and nothing but rgb / acc wanted (the batched secondary trace): the weights and their
  // sum are k_resample's, one thread per ray finishes (17 -> 3 us for 32 768 rays; same bits)
  bool pick_only = P.resample;
  for (int id = 0; id < RC_OUT_COUNT && pick_only; ++id)
    if (ca.out.ptr[id] && id != RC_OUT_RGB && id != RC_OUT_ACC) pick_only = false;
  if (pick_only) rc_launch_composite_pick(n, w.shade.p, w.filt_weight.p, w.acc_sel.p, ca.bg, ca.out.ptr[RC_OUT_RGB], ca.out.ptr[RC_OUT_ACC], st);
  else rc_launch_composite(ca, st);
}

// The secondary rays' environment: the EnvMap MLP, the bound image or none along the view directions, then k_env_combine.
void stage_env(rc_handle* h, const RenderArgs& A, RenderWs& w, hipStream_t st) {
  const int64_t n = A.n;
  const bool use_env = !(A.mask & RC_PASS_NO_ENVMAP);
  if (use_env && (A.mask & RC_PASS_ENV_IMAGE)) {
    // an explicit image instead of the EnvMap MLP (Model._handle_env_map, models.py:382-393)
    rc_launch_env_lookup(RcEnvLookupArgs{RcEnvImage{h->env_padded.p, h->env_img_h, h->env_img_w}, A.rays.viewdirs, n, w.env_rgb.p}, st);
  } else if (use_env) {
    RcEnvMapArgs ea{};
    ea.n = n; ea.viewdirs = A.rays.viewdirs; ea.wstream = h->packs.envmap.p; ea.rgb_bias = h->cfg.env_rgb_bias; ea.env_rgb = w.env_rgb.p;
    rc_launch_envmap(ea, st);
  }
  hipLaunchKernelGGL(k_env_combine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n,
                     (const float*)w.rgb_noenv.p, (const float*)w.acc_ws.p, use_env ? (const float*)w.env_rgb.p : (const float*)nullptr,
                     A.out.ptr[RC_OUT_RGB], A.out.ptr[RC_OUT_ACC], A.out.ptr[RC_OUT_ENV_MAP_RGB], A.out.ptr[RC_OUT_RGB_NO_ENV]);
}

// Enqueue the whole launch sequence of pass `A` on `st` (also used under stream capture) with workspace set `w`.
void enqueue_all(rc_handle* h, const RenderArgs& A, RenderWs& w, hipStream_t st) {
  RenderPlan P;
  P.secondary = (A.mask & RC_PASS_SECONDARY) != 0;
  P.resample = P.secondary || (A.mask & RC_PASS_RESAMPLE);
  P.lean = P.resample && !A.tout && A.stop != RENDER_WEIGHTS && !A.force_grad && !A.out.ptr[RC_OUT_NORMALS_PRED] &&
           !A.out.ptr[RC_OUT_NORMALS];
  if (A.fused) {
    stage_fused(h, A, w, st);
    return;
  }
  if (A.tout && h->fused_front_ok && h->fused_mode != 0 && !P.secondary && !P.resample && A.stop != RENDER_WEIGHTS) {
    stage_fused_front(h, A, w, st);
    enqueue_transient_tail(h, A, w, st);
    return;
  }
  stage_levels(h, A, P, w, st);
  if (A.stop == RENDER_SAMPLER || A.stop == RENDER_LEVELS) return;
  if (A.stop == RENDER_WEIGHTS) {
    RcCompositeArgs ca = composite_args(h, A, w, false, true, 0.0f);
    ca.normals_grad = nullptr;
    rc_launch_composite(ca, st);
    return;
  }
  stage_pick(h, A, P, w, st);
  if (A.tout) {
    enqueue_transient_tail(h, A, w, st);
    return;
  }
  stage_shade_composite(h, A, P, w, st);
  if (P.secondary) stage_env(h, A, w, st);
  stage_mark(h, A.slot, ST_COUNT, st);
}

// rc_render_rays, part 1: the checks behind the entry point's own, in the order a caller sees their errors.
int render_rays_check(rc_handle* h, const rc_randoms* rnd, uint32_t pass_mask) {
  int rc;
  if (h->transient) return fail(h, RC_ERR_UNSUPPORTED, "rc_render_rays: this handle renders the time-resolved cache (rc_render_transient)");
  if (!(pass_mask & RC_PASS_CACHE)) return fail(h, RC_ERR_UNSUPPORTED, "rc_render_rays: pass_mask must include RC_PASS_CACHE");
  const bool secondary = (pass_mask & RC_PASS_SECONDARY) != 0;
  const bool resample = secondary || (pass_mask & RC_PASS_RESAMPLE);
  if (resample && h->cfg.num_resample != 1) return fail(h, RC_ERR_UNSUPPORTED, "rc_render_rays: num_resample must be 1");
  if (resample && !(rnd && (rnd->gumbel || rnd->resample_inds)))
    return fail(h, RC_ERR_INVALID_ARG, "rc_render_rays: resampling needs rc_randoms.gumbel or .resample_inds");
  RC_HIP(h, hipSetDevice(h->device));
  if ((rc = ensure_packed(h))) return rc;
  const bool env_image = secondary && (pass_mask & RC_PASS_ENV_IMAGE) && !(pass_mask & RC_PASS_NO_ENVMAP);
  if (env_image && h->env_img_h == 0)
    return fail(h, RC_ERR_INVALID_ARG, "rc_render_rays: RC_PASS_ENV_IMAGE without a bound image (rc_set_env_image)");
  if (secondary && !(pass_mask & RC_PASS_NO_ENVMAP) && !env_image && !h->have_envmap)
    return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: params/Cache/EnvMap/* (secondary rays composite the model-level EnvMap)");
  return RC_OK;
}

// Everything that is baked into the kernel arguments of the pass: the key of its captured graph.
RenderKey render_key(const RenderArgs& A, int ws_slot) {
  RenderKey key;
  memset(&key, 0, sizeof(key));
  key.n = A.n; key.mask = A.mask; key.slot = A.slot; key.ws_slot = ws_slot;
  const void* rp[7] = {A.rays.origins, A.rays.directions, A.rays.viewdirs, A.rays.near, A.rays.far, A.rays.lights, A.rays.normals};
  memcpy(key.rays, rp, sizeof(rp));
  if (A.have_rnd) {
    for (int l = 0; l < RC_MAX_LEVELS; ++l) key.rnd[l] = A.rnd.jitter[l];
    key.rnd[RC_MAX_LEVELS] = A.rnd.gumbel; key.rnd[RC_MAX_LEVELS + 1] = A.rnd.resample_inds;
  }
  for (int i = 0; i < RC_OUT_COUNT; ++i) key.out[i] = A.out.ptr[i];
  return key;
}

// rc_render_rays, part 3: replay the pass's captured graph, capture it (when the call repeats, or always under graph mode
// 2) or launch it eagerly.
int render_rays_launch(rc_handle* h, const RenderArgs& A, int ws_slot, hipStream_t st) {
  RenderWs& w = h->ws[ws_slot].r;
  // event records are not replayable graph nodes: profile eagerly.  The fused plan is ONE launch: a plain launch
  // queues back to back with the previous one (gap < 1 us), the replay of a one-node graph leaves ~5 us between them.
  if (h->graph_mode != 0 && !h->profiling && !A.fused) {
    const RenderKey key = render_key(A, ws_slot);
    for (auto& g : h->graphs)
      if (g.key == key) {
        RC_HIP(h, hipGraphLaunch(g.exec, st));
        return RC_OK;
      }
    const bool capture = h->graph_mode == 2 || (h->have_last_key && h->last_key == key);
    h->last_key = key;
    h->have_last_key = true;
    if (capture) {
      // capture on a private stream (the caller's may be the legacy default stream), replay on the caller's
      if (!h->cap_stream) RC_HIP(h, hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
      if (h->graphs.size() >= 64) drop_graphs(h);
      GraphEntry e;
      e.key = key;
      RC_HIP(h, hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
      enqueue_all(h, A, w, h->cap_stream);
      const hipError_t ce = hipStreamEndCapture(h->cap_stream, &e.graph);
      if (ce == hipSuccess && e.graph) {
        RC_HIP(h, hipGraphInstantiate(&e.exec, e.graph, nullptr, nullptr, 0));
        h->graphs.push_back(e);
        RC_HIP(h, hipGraphLaunch(e.exec, st));
        return RC_OK;
      }
      // capture unsupported for this sequence: eager launches for good
      (void)hipGetLastError();
      h->graph_mode = 0;
    }
  }
  enqueue_all(h, A, w, st);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
}

}  // namespace

int rc_render_rays(rc_handle* h, const rc_rays* rays, int64_t n, const rc_randoms* rnd, uint32_t pass_mask,
                   const rc_outputs* out, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (!rays || !out) return fail(h, RC_ERR_INVALID_ARG, "rc_render_rays: null rays/outputs");
  if (n < 0) return fail(h, RC_ERR_INVALID_ARG, "rc_render_rays: negative n_rays");
  if (n == 0) return RC_OK;
  int rc;
  if ((rc = check_rays(h, rays, "rc_render_rays"))) return rc;
  RoctxScope roctx_call("rc_render_rays");
  if ((rc = render_rays_check(h, rnd, pass_mask))) return rc;

  // part 2, plan and workspace: one workspace set per caller stream (up to 4), so calls on different streams do not share
  // buffers.  The fused kernel keeps every intermediate on chip: no workspace, no set.
  hipStream_t st = (hipStream_t)stream_v;
  RenderArgs A = cache_pass(rays, rnd, n);
  A.mask = pass_mask; A.out = *out;
  A.fused = (h->fused_mode == 1 || h->fused_mode == 3) && h->fused_ok && pass_mask == RC_PASS_CACHE;
  const int ws_slot = A.fused ? WS_RENDER0 : ws_pick(h, st);
  WsUse use(h, ws_slot, st, !A.fused);
  if ((rc = use.rc)) return rc;
  if (!A.fused && (rc = ensure_workspace(h, use.s.r, n))) return rc;      // a reallocation drops the captured graphs (ws_alloc)
  rc_shader_prepare();
  if (h->profiling) {
    // mode 3: events around the dominant kernel of every 8th call only (an event record costs ~1.3 us of stream time)
    const int64_t call = h->prof_calls++;
    if (h->profiling != 3 || call % 8 == 0) {
      A.slot = (int)((h->profiling == 3 ? call / 8 : call) % kEvSlots);
      h->ev_used[A.slot] = true;
    }
  }
  return render_rays_launch(h, A, ws_slot, st);
  RC_CATCH(h)
}

// The chunk loop of render_image in native code: n_chunks x rc_render_rays on alternating streams (include/rc_abi.h).
int rc_render_chunks(rc_handle* h, const rc_rays* rays, int64_t chunk, int64_t n_chunks, uint32_t pass_mask,
                     const rc_outputs* out0, int64_t out_stride, void* const* streams, int32_t n_streams) {
  if (!h) return RC_ERR_INVALID_ARG;
  if (!rays || !out0 || !streams) return fail(h, RC_ERR_INVALID_ARG, "rc_render_chunks: null rays/outputs/streams");
  if (chunk <= 0 || n_chunks < 0 || n_streams <= 0 || out_stride < 0)
    return fail(h, RC_ERR_INVALID_ARG, "rc_render_chunks: chunk, n_chunks, n_streams, out_stride out of range");
  if ((pass_mask & RC_PASS_SECONDARY) || (pass_mask & RC_PASS_RESAMPLE))
    return fail(h, RC_ERR_UNSUPPORTED, "rc_render_chunks: passes that draw random numbers go through rc_render_rays per chunk");
  for (int64_t i = 0; i < n_chunks; ++i) {
    rc_rays r = *rays;
    const int64_t o = i * chunk;
    auto adv = [&](const float*& p, int w) { if (p) p += o * w; };
    adv(r.origins, 3); adv(r.directions, 3); adv(r.viewdirs, 3); adv(r.near, 1); adv(r.far, 1); adv(r.lights, 3); adv(r.normals, 3);
    rc_outputs out = *out0;
    for (int k = 0; k < RC_OUT_COUNT; ++k)
      if (out.ptr[k]) out.ptr[k] += i * out_stride;
    const int rc = rc_render_rays(h, &r, chunk, nullptr, pass_mask, &out, streams[i % n_streams]);
    if (rc) return rc;
  }
  return RC_OK;
}
