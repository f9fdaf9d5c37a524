// Host side of rc_material_data_backward (rc_material_data.hip); included by rc_api.hip.
//
// One call = rc_render_material itself (every step, kernels and launch order unchanged; its primary composite to
// "md:cache_rgb" / "md:cache_acc", its "rgb" not written) -> k_material_data_bwd (the integration's recompute, the rebuilt
// rgb to "md:rgb", the loss terms, with a gradient buffer d loss / d material per point) -> k_material_data_head_bwd (the
// loss sums; with a gradient buffer the head's backward, d loss / d features, the per-workgroup partials) ->
// rc_launch_material_partials_reduce (the loss; the dense segments in workgroup order) -> with a gradient buffer:
// rc_hashgrid_backward of the material grid at the shading points.

extern "C" int rc_material_data_backward(rc_handle* h, const rc_rays* rays, const float* gt_rgb, const float* lossmult, int64_t n,
                                         const rc_randoms* rnd, const rc_material_randoms* mr, int32_t K,
                                         const rc_material_data_loss* cfg, float* material_grads, float* loss, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  RoctxScope roctx_call("rc_material_data_backward");
  const std::string who = "rc_material_data_backward";
  if (h->transient) return fail(h, RC_ERR_UNSUPPORTED, who + ": not available on a time-resolved cache handle");
  if (!rays || !mr || !cfg) return fail(h, RC_ERR_INVALID_ARG, who + ": null argument");
  if (n < 0) return fail(h, RC_ERR_INVALID_ARG, who + ": negative n_rays");
  if (!std::isfinite(cfg->mult) || !std::isfinite(cfg->weight) || !std::isfinite(cfg->exponent) || !std::isfinite(cfg->eps) ||
      !std::isfinite(cfg->clip_val) || !(cfg->thresh == cfg->thresh))
    return fail(h, RC_ERR_INVALID_ARG, who + ": mult, weight, exponent, eps and clip_val must be finite, thresh not NaN");
  if (n == 0) return RC_OK;
  if (!loss) return fail(h, RC_ERR_INVALID_ARG, who + ": null loss");
  if (!gt_rgb) return fail(h, RC_ERR_INVALID_ARG, who + ": null gt_rgb");
  int rc;
  MatSplit sp;
  if ((rc = material_check(h, rays, mr, K, who.c_str(), sp))) return rc;
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  if ((rc = ensure_packed(h))) return rc;
  if (!h->have_material) return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: params/MaterialShader/* or params/LightSampler/*");
  const GridState& mg = h->grids[kMaterialGrid];
  if ((int)mg.sizes.size() * mg.cfg.num_features != kMaterialWidth ||
      dense_inventory(h->cfg, nullptr).at("params/MaterialShader/bottleneck_layer").second != 128)
    return fail(h, RC_ERR_UNSUPPORTED, who + ": the material grid must have 32 features and the bottleneck 128 outputs");
  WsUse use_d(h, WS_MATDATA, st);
  if ((rc = use_d.rc)) return rc;
  MatDataWs& y = ws_extra<MatDataWs>(use_d.s);
  const bool grads = material_grads != nullptr;
  const int G = rc_mat_data_blocks(n);
  if ((rc = ws_alloc(h, {{y.cache_rgb, 3 * n}, {y.cache_acc, n}, {y.rgb, 3 * n}, {y.loss_ray, n},
                         {y.loss_part, 2 * (int64_t)G}})))     // loss_part: doubles
    return rc;
  if (grads && (rc = ws_alloc(h, {{y.dmat, 5 * n}, {y.dfeat, kMaterialWidth * n}, {y.part, (int64_t)G * kRcMatSmoothParts}})))
    return rc;

  // 1. rc_render_material's forward, the call itself: the primary composite is the loss's "cache_rgb"
  rc_outputs co;
  memset(&co, 0, sizeof(co));
  co.ptr[RC_OUT_RGB] = y.cache_rgb.p; co.ptr[RC_OUT_ACC] = y.cache_acc.p;
  rc_mat_outputs mo;
  memset(&mo, 0, sizeof(mo));
  if ((rc = rc_render_material(h, rays, n, rnd, mr, K, &co, &mo, stream_v))) return rc;

  // 2. the integration's recompute, the loss terms and d loss / d material per point (its inputs: set 0's buffers)
  roctx_stage("material data loss");
  WsUse use(h, WS_RENDER0, st);
  if ((rc = use.rc)) return rc;
  RenderWs& w = use.s.r;
  ExtraWs& x = ws_extra<ExtraWs>(use.s);
  const rc_config& c = h->cfg;
  const int NL = c.num_levels;
  RcMatDataArgs a{};
  a.n = n; a.Ks = sp.Ks; a.Kd = sp.Kd; a.S = c.num_samples[NL - 1];
  a.mat = x.m_mat.p; a.samples = x.sec_samples.p; a.local_view = x.m_local_view.p; a.sec_rgb = x.sec_rgb.p;
  a.sec_acc = x.sec_acc.p; a.sec_env = x.sec_env.p; a.weights = w.weights[NL - 1].p; a.filt_weight = w.filt_weight.p;
  a.f0 = c.default_F_0; a.rgb_max = c.rgb_max; a.bg = c.bg_intensity;
  a.gt = gt_rgb; a.lossmult = lossmult; a.cache_rgb = y.cache_rgb.p;
  a.exponent = cfg->exponent; a.eps = cfg->eps; a.clip_val = cfg->clip_val; a.thresh = cfg->thresh;
  a.use_gt = cfg->use_gt_rawnerf != 0; a.use_combined = cfg->use_combined_rawnerf != 0; a.use_norm = cfg->use_norm_rawnerf != 0;
  const double mult = (double)cfg->weight * (double)cfg->mult;
  a.coef = (float)(mult / (3.0 * (double)n));                      // the mean over n x 3, weight, data_loss_mult
  a.rgb = y.rgb.p; a.loss_ray = y.loss_ray.p; a.dmat = grads ? y.dmat.p : nullptr;
  rc_launch_material_data_bwd(a, st);

  // 3. the loss sums and, with a gradient buffer, the head's backward
  const auto& raw = h->packs.raw;
  RcMatDataHeadArgs b{};
  b.n = n; b.feat = x.m_feat.p;
  b.w0 = raw[RAW_MAT_BOTTLENECK].kernel.p; b.b0 = raw[RAW_MAT_BOTTLENECK].bias.p;
  b.w1 = raw[RAW_MAT_BRDF].kernel.p; b.b1 = raw[RAW_MAT_BRDF].bias.p;
  b.min_roughness = c.min_roughness;
  b.dmat = a.dmat; b.loss_ray = y.loss_ray.p;
  b.dfeat = grads ? y.dfeat.p : nullptr; b.part = grads ? y.part.p : nullptr;
  b.loss_part = reinterpret_cast<double*>(y.loss_part.p);
  rc_launch_material_data_head_bwd(b, st);

  // 4. the loss and, with a gradient buffer, the dense segments (contiguous after the tables), both in a fixed order
  const std::vector<GradSeg> segs = material_grad_segments(h);
  rc_launch_material_partials_reduce(b.part, G, b.loss_part, grads ? material_grads + segs[mg.sizes.size()].offset : nullptr,
                                     (float)mult, 3.0 * (double)n, loss, st);
  RC_HIP(h, hipGetLastError());
  if (!grads) return RC_OK;
  // 5. the material grid's tables at the shading points (contracted as rc_render_material's lookup), at the layout's head
  return rc_hashgrid_backward(h, kMaterialGrid, x.m_pts.p, n, y.dfeat.p, material_grads, 1, stream_v);
  RC_CATCH(h)
}
