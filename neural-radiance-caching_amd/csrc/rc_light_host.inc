// Host side of rc_light_sampling_backward and rc_light_regularizer (rc_light.hip); included by rc_api.hip.
//
// One rc_light_sampling_backward call = rc_render_material's forward up to the batched secondary trace (material_* in
// rc_material_host.inc, on set 0 and WS_SECONDARY) -> the light head's recompute on k_gemm (h0, h1, vmf_params; "ls:" buffers) ->
// k_light_sampling_loss_bwd (per-point loss sums, d loss / d vmf_params) -> k_interlevel_reduce (the loss, fixed order) ->
// with a gradient buffer: the three dense layers' backward on k_gemm (input gradients masked by ReLU', weight gradients
// over fixed K slices of points, added up by k_sum_parts in slice order) and rc_hashgrid_backward of the light grid.

int rc_light_sampling_backward(rc_handle* h, const rc_rays* rays, const float* lossmult, int64_t n, const rc_randoms* rnd,
                               const rc_material_randoms* mr, int32_t K, const rc_light_sampling_loss* cfg,
                               float* light_grads, float* loss, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  RoctxScope roctx_call("rc_light_sampling_backward");
  if (h->transient) return fail(h, RC_ERR_UNSUPPORTED, "rc_light_sampling_backward: not available on a time-resolved cache handle");
  if (!rays || !mr || !cfg) return fail(h, RC_ERR_INVALID_ARG, "rc_light_sampling_backward: null argument");
  if (n < 0) return fail(h, RC_ERR_INVALID_ARG, "rc_light_sampling_backward: negative n_rays");
  if (!std::isfinite(cfg->mult)) return fail(h, RC_ERR_INVALID_ARG, "rc_light_sampling_backward: mult must be finite");
  if (n == 0) return RC_OK;
  if (!loss) return fail(h, RC_ERR_INVALID_ARG, "rc_light_sampling_backward: null loss");
  int rc;
  MatSplit sp;
  if ((rc = material_check(h, rays, mr, K, "rc_light_sampling_backward", sp))) return rc;
  const rc_config& c = h->cfg;
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  if ((rc = ensure_packed(h))) return rc;
  if (!h->have_material) return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: params/MaterialShader/* or params/LightSampler/*");
  const GridState& lg = h->grids[kLightGrid];
  if ((int)lg.sizes.size() * lg.cfg.num_features != kLightWidth)
    return fail(h, RC_ERR_UNSUPPORTED, "rc_light_sampling_backward: the light grid must have 32 features");
  const int64_t nsec = n * (sp.Ks + sp.Kd);
  WsUse use(h, WS_RENDER0, st);          // rc_render_material's sets: the forward's buffers keep their names
  if ((rc = use.rc)) return rc;
  RenderWs& w = use.s.r;
  ExtraWs& x = ws_extra<ExtraWs>(use.s);
  RenderWs& ws_sec = h->ws[WS_SECONDARY].r;
  if ((rc = material_workspace(h, w, x, ws_sec, n, sp))) return rc;
  WsUse use_l(h, WS_LIGHT, st);
  if ((rc = use_l.rc)) return rc;
  LightWs& y = ws_extra<LightWs>(use_l.s);
  const bool grads = light_grads != nullptr;
  const int64_t Z = (n + kDataKSlice - 1) / kDataKSlice;     // K slices of a weight gradient
  if ((rc = ws_alloc(h, {{y.cache_rgb, 3 * n}, {y.cache_acc, n}, {y.h0, 64 * n}, {y.h1, 64 * n}, {y.vp, 640 * n}, {y.loss_ray, n}})))
    return rc;
  if (grads && (rc = ws_alloc(h, {{y.dvp, 640 * n}, {y.dh1, 64 * n}, {y.dh0, 64 * n}, {y.dfeat, kLightWidth * n},
                                  {y.part, Z * 64 * 640}, {y.ones, 1}})))
    return rc;
  rc_shader_prepare();

  // 1. rc_render_material's forward: the primary pass (its composite to "ls:" buffers), the shading point, the heads,
  //    BRDF importance sampling, the batched secondary trace (no EnvMap: the loss does not read it)
  rc_outputs co;
  memset(&co, 0, sizeof(co));
  co.ptr[RC_OUT_RGB] = y.cache_rgb.p; co.ptr[RC_OUT_ACC] = y.cache_acc.p;
  material_primary(h, rays, n, rnd, mr, &co, w, x, st);
  material_heads(h, n, mr, x, st);
  material_brdf_sample(h, rays, n, mr, sp, x, st);
  {
    RenderArgs B;
    if ((rc = material_trace_args(h, mr, nsec, x, st, B))) return rc;
    enqueue_all(h, B, ws_sec, st);
  }

  // 2. the light head's recompute: h0 = relu(feat W0 + b0), h1 = relu(h0 W1 + b1), vp = h1 W2 + b2 (row-major per point)
  roctx_stage("light sampling: loss");
  const auto& raw = h->packs.raw;
  const Dense L[3] = {{kLightWidth, 64, raw[RAW_LIGHT_0].kernel.p, raw[RAW_LIGHT_0].bias.p},
                      {64, 64, raw[RAW_LIGHT_1].kernel.p, raw[RAW_LIGHT_1].bias.p},
                      {64, 640, raw[RAW_LIGHT_OUT].kernel.p, raw[RAW_LIGHT_OUT].bias.p}};
  const float* xin[3] = {x.l_feat.p, y.h0.p, y.h1.p};
  float* yout[3] = {y.h0.p, y.h1.p, y.vp.p};
  for (int l = 0; l < 3; ++l) dense_fwd(L[l], n, xin[l], L[l].in, yout[l], L[l].out, l < 2, st);
  // 3. the loss and d loss / d vmf_params
  RcLightLossArgs la{};
  la.n = n; la.Ks = sp.Ks; la.Kd = sp.Kd;
  la.vp = y.vp.p; la.noise = mr->vmf_noise; la.pts = x.m_pts.p; la.nrm = x.m_nrm.p;
  la.sec_dirs = x.sec_dirs.p; la.sec_rgb = x.sec_rgb.p; la.samples = x.sec_samples.p; la.lossmult = lossmult;
  la.vmf_scale = c.vmf_scale; la.srgb = cfg->linear_to_srgb != 0;
  la.coef_spec = (float)((double)cfg->mult / 2.0 / ((double)n * sp.Ks));      // mean over the n Ks samples, / 2, mult
  la.coef_diff = (float)((double)cfg->mult / 2.0 / ((double)n * sp.Kd));
  la.loss_ray = y.loss_ray.p; la.dvp = grads ? y.dvp.p : nullptr;
  rc_launch_light_sampling_loss_bwd(la, st);
  RcInterlevelReduce r{};
  r.mult[0] = 0.5f * cfg->mult; r.count[0] = (double)n;
  rc_launch_interlevel_reduce(y.loss_ray.p, n, 1, r, loss, st);
  RC_HIP(h, hipGetLastError());
  if (!grads) return RC_OK;

  // 4. the dense layers' backward, output layer first; weight gradients X^T dY over fixed K slices of points
  roctx_stage("light sampling: backward");
  RC_HIP(h, hipMemsetD32Async((hipDeviceptr_t)y.ones.p, 0x3f800000, 1, st));     // 1.0f: the A operand of a bias gradient
  const std::vector<GradSeg> segs = light_grad_segments(h);
  const size_t T = lg.sizes.size();                             // the tables lead the layout, then kernel / bias per layer
  const float* dyl[3] = {y.dh0.p, y.dh1.p, y.dvp.p};
  float* dxl[3] = {y.dfeat.p, y.dh0.p, y.dh1.p};
  const float* hmask[3] = {nullptr, y.h0.p, y.h1.p};           // ReLU' of the layer's input
  for (int l = 2; l >= 0; --l) {
    dense_wgrad(L[l], n, xin[l], L[l].in, dyl[l], L[l].out, y.ones.p, y.part.p, light_grads, &segs[T + 2 * l], st);
    dense_dx(L[l], n, dyl[l], L[l].out, dxl[l], L[l].in, 0, L[l].in, hmask[l], false, st);     // zero where the input's ReLU was off
  }
  RC_HIP(h, hipGetLastError());
  // 5. the light grid's tables (contracted shading points), at the head of the layout
  return rc_hashgrid_backward(h, kLightGrid, x.m_pts.p, n, y.dfeat.p, light_grads, 1, stream_v);
  RC_CATCH(h)
}

int rc_light_regularizer(rc_handle* h, float mult, float* light_grads, float* loss, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  return grid_l2_regularizer<LightWs>(h, kLightGrid, WS_LIGHT, mult, light_grads, loss, stream_v, "rc_light_regularizer");
  RC_CATCH(h)
}
