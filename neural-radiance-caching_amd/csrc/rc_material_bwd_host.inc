// Host side of rc_material_smoothness_backward and rc_material_regularizer (rc_material_bwd.hip); included by rc_api.hip.
//
// One rc_material_smoothness_backward call = rc_render_material's steps 1-2 (material_primary in rc_material_host.inc, on set 0) ->
// k_material_smoothness_points (x, x' = x + noise_scale nu; "ms:pts") -> one material-grid lookup over the 2n points
// ("ms:feat"; the same device function as rc_render_material's k_hashgrid_two) -> k_material_smoothness_bwd (both heads,
// m(x) into m_mat, the loss terms and per-workgroup loss sums, with a gradient buffer the head's backward, d loss /
// d features and per-workgroup partials of the dense gradients) -> k_material_smoothness_reduce (the loss; the partials
// in workgroup order) -> with a gradient buffer: rc_hashgrid_backward of the material grid at the 2n points.

int rc_material_smoothness_backward(rc_handle* h, const rc_rays* rays, const float* lossmult, int64_t n, const rc_randoms* rnd,
                                    const rc_material_randoms* mr, const float* noise, const rc_material_smoothness_loss* cfg,
                                    float* material_grads, float* loss, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  RoctxScope roctx_call("rc_material_smoothness_backward");
  const std::string who = "rc_material_smoothness_backward";
  if (h->transient) return fail(h, RC_ERR_UNSUPPORTED, who + ": not available on a time-resolved cache handle");
  if (!rays || !mr || !cfg) return fail(h, RC_ERR_INVALID_ARG, who + ": null argument");
  if (n < 0) return fail(h, RC_ERR_INVALID_ARG, who + ": negative n_rays");
  if (!std::isfinite(cfg->mult) || !std::isfinite(cfg->weight_albedo) || !std::isfinite(cfg->weight_other) ||
      !std::isfinite(cfg->noise))
    return fail(h, RC_ERR_INVALID_ARG, who + ": mult, weights and noise must be finite");
  if (n == 0) return RC_OK;
  if (!loss) return fail(h, RC_ERR_INVALID_ARG, who + ": null loss");
  if (!noise) return fail(h, RC_ERR_INVALID_ARG, who + ": null noise");
  int rc;
  if ((rc = check_rays(h, rays, who.c_str()))) return rc;
  if (!(mr->gumbel || mr->resample_inds))
    return fail(h, RC_ERR_INVALID_ARG, who + ": the shading point's pick needs gumbel or resample_inds");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  if ((rc = ensure_packed(h))) return rc;
  if (!h->have_material) return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: params/MaterialShader/* or params/LightSampler/*");
  const GridState& mg = h->grids[kMaterialGrid];
  if ((int)mg.sizes.size() * mg.cfg.num_features != kMaterialWidth ||
      dense_inventory(h->cfg, nullptr).at("params/MaterialShader/bottleneck_layer").second != 128)
    return fail(h, RC_ERR_UNSUPPORTED, who + ": the material grid must have 32 features and the bottleneck 128 outputs");
  WsUse use(h, WS_RENDER0, st);          // rc_render_material's set: the forward's buffers keep their names
  if ((rc = use.rc)) return rc;
  RenderWs& w = use.s.r;
  ExtraWs& x = ws_extra<ExtraWs>(use.s);
  if ((rc = ensure_workspace(h, w, n))) return rc;
  if ((rc = ws_alloc(h, {{x.m_pts, 3 * n}, {x.m_nrm, 3 * n}, {x.m_mat, RC_MAT_CH * n}}))) return rc;
  WsUse use_m(h, WS_MATERIAL, st);
  if ((rc = use_m.rc)) return rc;
  MaterialWs& y = ws_extra<MaterialWs>(use_m.s);
  const bool grads = material_grads != nullptr;
  const int G = rc_mat_smooth_blocks(n);
  if ((rc = ws_alloc(h, {{y.cache_rgb, 3 * n}, {y.cache_acc, n}, {y.pts, 6 * n}, {y.feat, 2 * kMaterialWidth * n},
                         {y.mat_p, RC_MAT_CH * n}, {y.loss_ray, n}, {y.loss_part, 2 * (int64_t)G}})))     // loss_part: doubles
    return rc;
  if (grads && (rc = ws_alloc(h, {{y.dfeat, 2 * kMaterialWidth * n}, {y.part, (int64_t)G * kRcMatSmoothParts}}))) return rc;
  rc_shader_prepare();

  // 1. rc_render_material's steps 1-2: the primary pass (its composite to "ms:" buffers, not read) and the shading point
  rc_outputs co;
  memset(&co, 0, sizeof(co));
  co.ptr[RC_OUT_RGB] = y.cache_rgb.p; co.ptr[RC_OUT_ACC] = y.cache_acc.p;
  material_primary(h, rays, n, rnd, mr, &co, w, x, st);

  // 2. the lookup points x, x' and the material grid's features at both, in one launch
  roctx_stage("material smoothness");
  const rc_config& c = h->cfg;
  rc_launch_material_smoothness_points(x.m_pts.p, noise, cfg->noise, n, y.pts.p, st);
  rc_launch_hashgrid(mg.dev, y.pts.p, 0, 2 * n, y.feat.p, 0, kMaterialWidth, c.contract_radius, nullptr, st);

  // 3. both heads, the loss terms and (with a gradient buffer) the backward
  const auto& raw = h->packs.raw;
  RcMatSmoothArgs a{};
  a.n = n; a.feat_x = y.feat.p; a.feat_p = y.feat.p + kMaterialWidth * n;
  a.w0 = raw[RAW_MAT_BOTTLENECK].kernel.p; a.b0 = raw[RAW_MAT_BOTTLENECK].bias.p;
  a.w1 = raw[RAW_MAT_BRDF].kernel.p; a.b1 = raw[RAW_MAT_BRDF].bias.p;
  a.min_roughness = c.min_roughness;
  a.filt_weight = w.filt_weight.p; a.lossmult = lossmult;
  a.tensoir = cfg->tensoir_albedo != 0;
  a.wa = (float)((double)cfg->weight_albedo / 3.0); a.wo = cfg->weight_other;
  a.ga = (float)((double)cfg->mult * cfg->weight_albedo / (3.0 * (double)n));     // the mean over n x 3, mult
  a.go = (float)((double)cfg->mult * cfg->weight_other / (double)n);
  a.mat_x = x.m_mat.p; a.mat_p = y.mat_p.p; a.loss_ray = y.loss_ray.p;
  a.dfeat = grads ? y.dfeat.p : nullptr; a.part = grads ? y.part.p : nullptr;
  a.loss_part = reinterpret_cast<double*>(y.loss_part.p);
  rc_launch_material_smoothness_bwd(a, st);
  // 4. the loss and, with a gradient buffer, the dense segments (contiguous after the tables), both in a fixed order
  const std::vector<GradSeg> segs = material_grad_segments(h);
  rc_launch_material_smoothness_reduce(a, grads ? material_grads + segs[mg.sizes.size()].offset : nullptr, cfg->mult, loss, st);
  RC_HIP(h, hipGetLastError());
  if (!grads) return RC_OK;
  // 5. the material grid's tables (contracted points x, then x'), at the head of the layout
  return rc_hashgrid_backward(h, kMaterialGrid, y.pts.p, 2 * n, y.dfeat.p, material_grads, 1, stream_v);
  RC_CATCH(h)
}

int rc_material_regularizer(rc_handle* h, float mult, float* material_grads, float* loss, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  return grid_l2_regularizer<MaterialWs>(h, kMaterialGrid, WS_MATERIAL, mult, material_grads, loss, stream_v,
                                         "rc_material_regularizer");
  RC_CATCH(h)
}
