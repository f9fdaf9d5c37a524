// The material stage (included by rc_api.hip): rc_render_material's launch sequence, shared with rc_render_relight
// (rc_relight_host.inc) and, step by step, with the training forwards of the material losses.

namespace {

// rc_render_material's forward, shared with rc_light_sampling_backward (rc_light_host.inc): the argument checks behind
// the entry point's own, the workspace, and steps 1-2 (the primary cache pass, the shading point), 3a-4 (the shading
// heads), 5 (BRDF importance sampling) and the arguments of step 6 (the batched secondary trace).  Each step launches
// what rc_render_material launched before, in the same order.
struct MatSplit { int Ks, Kd, Kc; };

int material_check(rc_handle* h, const rc_rays* rays, const rc_material_randoms* mr, int32_t K, const char* who, MatSplit& sp,
                   bool own_samplers = true) {
  int rc;
  const std::string w = who;
  if ((rc = check_rays(h, rays, who))) return rc;
  const rc_config& c = h->cfg;
  // Python's round (half to even), as importance_sample_rays and everything that sizes the random tensors
  sp.Ks = rc_round_half_even(K * (1.0 - (double)c.diffuse_sample_fraction));
  sp.Kd = rc_round_half_even(K * (double)c.diffuse_sample_fraction);
  sp.Kc = rc_round_half_even(0.5 * sp.Kd);
  const int Ks = sp.Ks, Kd = sp.Kd, Kc = sp.Kc;
  if (Ks + Kd != K)
    return fail(h, RC_ERR_UNSUPPORTED, w + ": num_secondary_samples does not split into Ks + Kd (round half to even)");
  if (K < 2 || Ks < 1 || Kd < 2 || Kc < 1 || Kd - Kc < 1 || Ks + Kd > 64)
    return fail(h, RC_ERR_UNSUPPORTED, w + ": num_secondary_samples must give 1 <= Ks, 2 <= Kd, Ks + Kd <= 64");
  if (c.num_vmf != 128) return fail(h, RC_ERR_UNSUPPORTED, w + ": num_vmf must be 128");
  // (own_samplers = false: rc_render_relight's RC_RELIGHT_ENV, which reads neither the BRDF nor the vMF members)
  if (own_samplers)
  if (!mr->vmf_noise || !mr->spec_u1 || !mr->spec_u2 || !mr->cos_u1 || !mr->cos_u2 || !mr->vmf_v || !mr->vmf_tmp ||
      !(mr->vmf_lobe || mr->vmf_lobe_gumbel))
    return fail(h, RC_ERR_INVALID_ARG, w + ": every sampler member of rc_material_randoms is required "
                                           "(vmf_lobe or vmf_lobe_gumbel)");
  if (!(mr->gumbel || mr->resample_inds) || !(mr->sec_gumbel || mr->sec_resample_inds))
    return fail(h, RC_ERR_INVALID_ARG, w + ": the categorical picks need gumbel or resample_inds (primary) and "
                                           "sec_gumbel or sec_resample_inds (secondary trace)");
  return RC_OK;
}

int material_workspace(rc_handle* h, RenderWs& w, ExtraWs& x, RenderWs& ws_sec, int64_t n, const MatSplit& sp) {
  const rc_config& c = h->cfg;
  const int64_t np2 = n * c.num_samples[c.num_levels - 1], nsec = n * (sp.Ks + sp.Kd);
  int rc;
  if ((rc = ensure_workspace(h, w, n))) return rc;
  if ((rc = ws_alloc(h, {{x.m_pts, 3 * n}, {x.m_nrm, 3 * n}, {x.m_feat, 32 * n}, {x.m_mat, RC_MAT_CH * n}, {x.m_feat_all, 32 * np2},
                         {x.m_mat_all, RC_MAT_CH * np2}, {x.l_feat, 32 * n}, {x.l_vmf, (int64_t)128 * RC_VMF_CH * n},
                         {x.l_vmf_logit, (int64_t)128 * n}, {x.sec_origins, 3 * nsec}, {x.sec_dirs, 3 * nsec}, {x.sec_near, nsec},
                         {x.sec_far, nsec}, {x.sec_lights, 3 * nsec}, {x.sec_samples, RC_SMP_CH * nsec}, {x.m_local_view, 3 * n},
                         {x.sec_rgb, 3 * nsec}, {x.sec_acc, nsec}, {x.sec_env, 3 * nsec}})) ||
      (rc = ensure_workspace(h, ws_sec, nsec)))
    return rc;
  return RC_OK;
}

// 1. cache pass on the primary rays (all samples shaded) -> cache_out; 2. one shading sample per ray
void material_primary(rc_handle* h, const rc_rays* rays, int64_t n, const rc_randoms* rnd, const rc_material_randoms* mr,
                      const rc_outputs* cache_out, RenderWs& w, ExtraWs& x, hipStream_t st) {
  const rc_config& c = h->cfg;
  const int NL = c.num_levels;
  const int S2 = c.num_samples[NL - 1];
  RenderArgs A = cache_pass(rays, rnd, n);
  A.out = *cache_out;
  // the fused kernel when the handle runs it (rc_set_fused mode 1): one launch, its per-sample results exported for
  // steps 2-3 below; bitwise the launch-per-stage pass (tests/test_gpu_parity.py)
  A.fused = (h->fused_mode == 1 || h->fused_mode == 3) && h->fused_ok && !h->profiling && c.num_samples[NL - 1] == 32;
  A.export_samples = A.fused;
  enqueue_all(h, A, w, st);

  // 2. one shading sample per ray (MaterialModel.resample_render, models.py:1430-1439)
  RcResampleArgs ra{};
  ra.n_rays = n; ra.S = S2; ra.tdist = w.tdist[NL - 1].p; ra.density = w.density[NL - 1].p;
  ra.directions = rays->directions; ra.gumbel = mr->gumbel; ra.inds_in = mr->resample_inds;
  ra.inds_out = (int32_t*)w.inds.p; ra.filt_weight = w.filt_weight.p; ra.weights = w.weights[NL - 1].p; ra.src_out = (int32_t*)w.src_idx.p;
  // position and predicted normal of the picked sample = the shading point
  ra.means = w.means[NL - 1].p; ra.normals = w.normals_pred.p; ra.pts_out = x.m_pts.p; ra.nrm_out = x.m_nrm.p;
  rc_launch_resample(ra, st);
}

// The material head on n points: features in, materials out.
RcMatHeadArgs material_head_args(rc_handle* h, int64_t n, const float* feat, float* mat) {
  const auto& raw = h->packs.raw;
  RcMatHeadArgs ma{};
  ma.n = n; ma.feat = feat; ma.mat = mat;
  ma.w0 = raw[RAW_MAT_BOTTLENECK].kernel.p; ma.b0 = raw[RAW_MAT_BOTTLENECK].bias.p;
  ma.w1 = raw[RAW_MAT_BRDF].kernel.p; ma.b1 = raw[RAW_MAT_BRDF].bias.p;
  ma.min_roughness = h->cfg.min_roughness;
  return ma;
}

// 3a. material head and 4. light sampler (128 vMF lobes) at the shading point: one lookup launch + one head launch on the
// caller's stream
void material_heads(rc_handle* h, int64_t n, const rc_material_randoms* mr, ExtraWs& x, hipStream_t st) {
  const rc_config& c = h->cfg;
  const auto& raw = h->packs.raw;
  roctx_stage("material: heads + light sampler");
  RcLightHeadArgs la{};
  la.n = n; la.feat = x.l_feat.p;
  la.w0 = raw[RAW_LIGHT_0].kernel.p; la.b0 = raw[RAW_LIGHT_0].bias.p;
  la.w1 = raw[RAW_LIGHT_1].kernel.p; la.b1 = raw[RAW_LIGHT_1].bias.p;
  la.w2 = raw[RAW_LIGHT_OUT].kernel.p; la.b2 = raw[RAW_LIGHT_OUT].bias.p;
  la.pts = x.m_pts.p; la.noise = mr->vmf_noise; la.vmf_scale = c.vmf_scale; la.vmf = x.l_vmf.p; la.vmf_logit = x.l_vmf_logit.p;
  // caller's stream, the critical path: both grids at the shading points in one launch, both heads in one launch (as
  // four launches on two streams the BRDF sampler waited ~12 us for the event behind the light head)
  rc_launch_hashgrid_two(h->grids[4].dev, h->grids[5].dev, x.m_pts.p, n, x.m_feat.p, x.l_feat.p, c.contract_radius, st);
  rc_launch_shading_heads(material_head_args(h, n, x.m_feat.p, x.m_mat.p), la, st);
}

// 5. BRDF importance sampling -> secondary rays
void material_brdf_sample(rc_handle* h, const rc_rays* rays, int64_t n, const rc_material_randoms* mr, const MatSplit& sp,
                          ExtraWs& x, hipStream_t st) {
  const rc_config& c = h->cfg;
  roctx_stage("material: brdf sample");
  RcBrdfSampleArgs sa{};
  sa.n = n; sa.Ks = sp.Ks; sa.Kd = sp.Kd; sa.Kc = sp.Kc;
  sa.pts = x.m_pts.p; sa.nrm = x.m_nrm.p; sa.viewdirs = rays->viewdirs; sa.lights = rays->lights;
  sa.mat = x.m_mat.p; sa.vmf = x.l_vmf.p; sa.vmf_logit = x.l_vmf_logit.p;
  sa.spec_u1 = mr->spec_u1; sa.spec_u2 = mr->spec_u2; sa.cos_u1 = mr->cos_u1; sa.cos_u2 = mr->cos_u2;
  sa.vmf_lobe = mr->vmf_lobe; sa.vmf_v = mr->vmf_v; sa.vmf_tmp = mr->vmf_tmp; sa.vmf_lobe_gumbel = mr->vmf_lobe_gumbel;
  sa.normal_eps = c.secondary_normal_eps; sa.near = c.secondary_near; sa.far = c.secondary_far;
  sa.sec_origins = x.sec_origins.p; sa.sec_dirs = x.sec_dirs.p; sa.sec_near = x.sec_near.p; sa.sec_far = x.sec_far.p;
  sa.sec_lights = x.sec_lights.p; sa.samples = x.sec_samples.p; sa.local_view = x.m_local_view.p;
  rc_launch_brdf_sample(sa, st);
}

// 6. the arguments of the ONE batched secondary trace through the cache (is_secondary, resample, use_env_map=False;
//    ref_rays.normals = None since MaterialMLP.shadow_eps_indirect = False) -> sec_rgb, sec_acc
int material_trace_args(rc_handle* h, const rc_material_randoms* mr, int64_t nsec, ExtraWs& x, hipStream_t st, RenderArgs& B) {
  const rc_config& c = h->cfg;
  B = RenderArgs{};
  B.rays.origins = x.sec_origins.p; B.rays.directions = x.sec_dirs.p; B.rays.viewdirs = x.sec_dirs.p;
  B.rays.near = x.sec_near.p; B.rays.far = x.sec_far.p; B.rays.lights = x.sec_lights.p; B.rays.normals = nullptr;
  B.have_rnd = true;
  for (int l = 0; l < RC_MAX_LEVELS; ++l) B.rnd.jitter[l] = mr->sec_jitter[l];
  B.rnd.gumbel = mr->sec_gumbel; B.rnd.resample_inds = mr->sec_resample_inds;
  B.n = nsec; B.mask = RC_PASS_CACHE | RC_PASS_SECONDARY | RC_PASS_NO_ENVMAP; B.slot = -1;
  // every secondary ray of this trace has the same (near, far) (k_brdf_sample writes the two constants): the
  // power-ladder image of the pair is computed once instead of by each of the 3 x 32 768 sampler waves
  // ... and once per handle: the five inputs are constants of the configuration (same device function, a buffer of
  // the handle's own; 5 us + a 6 us gap in every step before)
  if (!h->sec_sbounds) {
    RC_HIP(h, hipMalloc((void**)&h->sec_sbounds, 2 * sizeof(float)));
    rc_launch_ladder_bounds(c.secondary_near, c.secondary_far, c.env_map_distance, c.raydist_p, c.raydist_premult, h->sec_sbounds, st);
    RC_HIP(h, hipStreamSynchronize(st));       // later calls may come on other streams
  }
  B.s_bounds = h->sec_sbounds;
  memset(&B.out, 0, sizeof(B.out));
  B.out.ptr[RC_OUT_RGB] = x.sec_rgb.p; B.out.ptr[RC_OUT_ACC] = x.sec_acc.p;
  return RC_OK;
}

int relight_check(rc_handle* h, const rc_relight_args* rl, int64_t n, const MatSplit& sp);      // rc_relight_host.inc

// The material stage: rc_render_material (rl == nullptr) and rc_render_relight (rc_relight_host.inc), which replaces the
// EnvMap along the secondary rays by the bound image's lookup, in RC_RELIGHT_ENV the light head and the BRDF sampler by the
// environment sampler, and scales the albedo; every other launch is the same code in the same order.
int material_render(rc_handle* h, const rc_rays* rays, int64_t n, const rc_randoms* rnd, const rc_material_randoms* mr, int32_t K,
                    const rc_relight_args* rl, const rc_outputs* cache_out, const rc_mat_outputs* mat_out, void* stream_v,
                    const char* who_c) {
  const std::string who = who_c;
  if (h->transient) return fail(h, RC_ERR_UNSUPPORTED, who + ": this handle renders the time-resolved cache (rc_render_transient)");
  if (!rays || !mr || !cache_out || !mat_out) return fail(h, RC_ERR_INVALID_ARG, who + ": null argument");
  if (n < 0) return fail(h, RC_ERR_INVALID_ARG, who + ": negative n_rays");
  if (n == 0) return RC_OK;
  int rc;
  MatSplit sp;
  const bool env_mode = rl && rl->mode == RC_RELIGHT_ENV;
  if ((rc = material_check(h, rays, mr, K, who_c, sp, !env_mode))) return rc;
  if (rl && (rc = relight_check(h, rl, n, sp))) return rc;
  const float* ratio = rl ? rl->albedo_ratio : nullptr;
  const rc_config& c = h->cfg;
  const int Ks = sp.Ks, Kd = sp.Kd;
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  if ((rc = ensure_packed(h))) return rc;
  if (!h->have_material) return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: params/MaterialShader/* or params/LightSampler/*");
  if (!rl && !h->have_envmap) return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: params/Cache/EnvMap/*");
  const int NL = c.num_levels;
  const int S2 = c.num_samples[NL - 1];
  const int64_t np2 = n * S2, nsec = n * (Ks + Kd);
  WsUse use(h, WS_RENDER0, st);          // shares set 0 (and the secondary set) with the other entry points
  if ((rc = use.rc)) return rc;
  RenderWs& w = use.s.r;
  ExtraWs& x = ws_extra<ExtraWs>(use.s);
  RenderWs& ws_sec = h->ws[WS_SECONDARY].r;
  if ((rc = material_workspace(h, w, x, ws_sec, n, sp))) return rc;
  rc_shader_prepare();

  // 1. cache pass on the primary rays (all samples shaded) -> cache_out; 2. one shading sample per ray
  material_primary(h, rays, n, rnd, mr, cache_out, w, x, st);
  // Side stream: the material-only composite over all samples (step 3b) and the EnvMap along the secondary rays (step 6b)
  // feed only the outputs / the final integration, so they leave the critical path sampler -> trace -> integrate and
  // fill the gaps of its latency-bound kernels.  Forked from and joined to the caller's stream with events: to the
  // caller the call is still ordered on `st` alone.
  { int rcs = ensure_side_stream(h); if (rcs) return rcs; }
  hipStream_t side = h->side_stream;
  // Whatever way this function is left once work has been forked onto the side stream, the caller's stream is joined
  // to it again BEFORE the workspace set is released (declared after `use`: destroyed first): an early error
  // return must not leave side-stream kernels writing mat_out / sec_env behind a caller that believes `st` orders
  // everything of the call.
  struct SideJoin {
    rc_handle* h; hipStream_t st, side; bool forked;
    ~SideJoin() {
      if (!forked) return;
      if (hipEventRecord(h->ev_side[2], side) != hipSuccess || hipStreamWaitEvent(st, h->ev_side[2], 0) != hipSuccess)
        (void)hipStreamSynchronize(side);
    }
  } side_join{h, st, side, false};
  // 3a. material head and 4. light sampler (128 vMF lobes) at the shading point
  if (env_mode) {
    // _handle_light_sampling_pass hands the image's tables on: the LightSampler is not evaluated
    roctx_stage("material: head");
    rc_launch_hashgrid(h->grids[4].dev, x.m_pts.p, 0, n, x.m_feat.p, 0, 32, c.contract_radius, nullptr, st);
    rc_launch_material_head(material_head_args(h, n, x.m_feat.p, x.m_mat.p), st);
  } else {
    material_heads(h, n, mr, x, st);
  }
  // albedo <- clip(albedo ratio, 0, 1) (_predict_material_and_feature, material.py:2106-2116)
  if (ratio) rc_launch_albedo_ratio(x.m_mat.p, n, ratio, st);
  // 5. BRDF importance sampling -> secondary rays
  if (env_mode) {
    roctx_stage("material: environment sample");
    RcEnvSampleArgs sa{};
    sa.n = n; sa.Ks = Ks; sa.Kd = Kd;
    sa.pts = x.m_pts.p; sa.nrm = x.m_nrm.p; sa.viewdirs = rays->viewdirs; sa.lights = rays->lights;
    sa.pdf = h->env_pdf.p; sa.dirs = h->env_dirs.p; sa.hw = (int64_t)h->env_img_h * h->env_img_w;
    sa.picks_spec = rl->picks_spec; sa.picks_diff = rl->picks_diff; sa.T_spec = rl->T_spec; sa.T_diff = rl->T_diff;
    sa.normal_eps = c.secondary_normal_eps; sa.near = c.secondary_near; sa.far = c.secondary_far;
    sa.sec_origins = x.sec_origins.p; sa.sec_dirs = x.sec_dirs.p; sa.sec_near = x.sec_near.p; sa.sec_far = x.sec_far.p;
    sa.sec_lights = x.sec_lights.p; sa.samples = x.sec_samples.p; sa.local_view = x.m_local_view.p;
    rc_launch_env_sample(sa, st);
  } else {
    material_brdf_sample(h, rays, n, mr, sp, x, st);
  }
  // 3b. side stream: the material head on ALL samples and the material-only composite (outputs only).  Forked HERE, behind
  // the BRDF sampler: beside the small latency-bound kernels above they doubled those kernels' times (heads 18 -> 35 us,
  // sampler 19 -> 33 us); beside the first level of the trace they fit into what its workgroups leave of a CU (no LDS /
  // 11 KB) and cost it little.
  {
    RC_HIP(h, hipEventRecord(h->ev_side[0], st));
    RC_HIP(h, hipStreamWaitEvent(side, h->ev_side[0], 0));
    side_join.forked = true;
    rc_launch_hashgrid(h->grids[4].dev, w.means[NL - 1].p, 1, np2, x.m_feat_all.p, 0, 32, c.contract_radius, nullptr, side);
    rc_launch_material_head(material_head_args(h, np2, x.m_feat_all.p, x.m_mat_all.p), side);
    if (ratio) rc_launch_albedo_ratio(x.m_mat_all.p, np2, ratio, side);
    rc_launch_material_composite_all(n, S2, w.weights[NL - 1].p, x.m_mat_all.p, mat_out->ptr[RC_MOUT_MATERIAL_ALBEDO],
                                     mat_out->ptr[RC_MOUT_MATERIAL_ROUGHNESS], mat_out->ptr[RC_MOUT_MATERIAL_METALNESS],
                                     mat_out->ptr[RC_MOUT_MATERIAL_F_0], c.default_F_0, side);
  }
  // 6. ONE batched secondary trace through the cache (is_secondary, resample, use_env_map=False;
  //    ref_rays.normals = None since MaterialMLP.shadow_eps_indirect = False) + EnvMap along the same rays
  {
    RenderArgs B;
    if ((rc = material_trace_args(h, mr, nsec, x, st, B))) return rc;
    const RcEnvLookupArgs la{RcEnvImage{h->env_padded.p, h->env_img_h, h->env_img_w}, x.sec_dirs.p, nsec, x.sec_env.p};
    SideEnv env{};
    env.map.n = nsec; env.map.viewdirs = x.sec_dirs.p; env.map.wstream = h->packs.envmap.p; env.map.rgb_bias = c.env_rgb_bias;
    env.map.env_rgb = x.sec_env.p;
    env.lookup = rl ? &la : nullptr;            // rc_render_relight: the bound image's lookup in the EnvMap's place
    env.side = side; env.ready = h->ev_side[1]; env.done = h->ev_side[2];
    // 6b. EnvMap of the secondary directions, on the side stream.  It is MFMA-bound and keeps a CU's LDS to itself, as the
    // level kernels of the trace do: next to a level kernel it only gets the CUs that kernel's persistent workgroups
    // leave.  Beside the first two levels (F = 1: bound by their own instruction issue) every CU it takes is a CU they
    // miss; the LAST level (F = 4) is bound by the fabric's random-sector rate, not by CUs.  So the EnvMap is released when
    // that level is launched, and that launch leaves it a quarter of the CUs (RC_ENV_RESERVE overrides; 0 = beside the
    // first level as before): 1.48 -> 1.45 ms per step (reserve 32 / 64 / 96 of 256: 1.463 / 1.447-1.456 / 1.508).
    // (split-MFMA build: the EnvMap takes 0.7 of the time on the bf16 pipe and an eighth of the CUs is enough -- 16 ... 40 of
    // 256 measure 1.315-1.33 ms per step, 64: 1.36, 80: 1.38)
    static const int env_reserve = getenv("RC_ENV_RESERVE") ? atoi(getenv("RC_ENV_RESERVE")) : rc_device_cus() / (kRcSplit ? 8 : 4);
    // (rc_render_relight: the image lookup is memory-bound and short; it never takes that spot)
    const bool beside_last = !rl && env_reserve > 0 && nsec >= 24576 && (h->fused_mode == 1 || h->fused_mode == 3);
    env.reserve = env_reserve;
    if (beside_last) B.env = &env;
    else RC_HIP(h, side_release(env, st));                        // secondary rays are in place
    enqueue_all(h, B, ws_sec, st);
    // the trace took a launch plan without that spot (per-stage profiling on, a grid layout the level kernels do not
    // cover): the EnvMap behind the trace
    if (!env.released) RC_HIP(h, side_release(env, st));
    RC_HIP(h, hipStreamWaitEvent(st, h->ev_side[2], 0));          // join: everything of this call is ordered on st again
    side_join.forked = false;
  }
  // 7. Monte-Carlo BRDF integration + MaterialIntegrator composite
  roctx_stage("material: integrate");
  {
    RcMatIntegrateArgs ia{};
    ia.n = n; ia.Ks = Ks; ia.Kd = Kd; ia.S = S2;
    ia.mat = x.m_mat.p; ia.samples = x.sec_samples.p; ia.local_view = x.m_local_view.p; ia.sec_rgb = x.sec_rgb.p;
    ia.sec_acc = x.sec_acc.p; ia.sec_env = x.sec_env.p; ia.weights = w.weights[NL - 1].p; ia.filt_weight = w.filt_weight.p;
    ia.pts = x.m_pts.p; ia.nrm = x.m_nrm.p; ia.origins = rays->origins; ia.lights = rays->lights;
    ia.f0 = c.default_F_0; ia.rgb_max = c.rgb_max; ia.bg = c.bg_intensity;
    ia.out = *mat_out;
    rc_launch_material_integrate(ia, st);
  }
  RC_HIP(h, hipGetLastError());
  return RC_OK;
}

}  // namespace

int rc_render_material(rc_handle* h, const rc_rays* rays, int64_t n, const rc_randoms* rnd,
                       const rc_material_randoms* mr, int32_t K, const rc_outputs* cache_out,
                       const rc_mat_outputs* mat_out, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  RoctxScope roctx_call("rc_render_material");
  return material_render(h, rays, n, rnd, mr, K, nullptr, cache_out, mat_out, stream_v, "rc_render_material");
  RC_CATCH(h)
}
