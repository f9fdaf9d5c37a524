// Host side of rc_light_sampling_backward and rc_light_regularizer (rc_light.hip) and the light layout; included by
// rc_api.hip after rc_geometry_host.inc (rc_optim_host.inc's rc_load_params_flat reads light_grad_segments).
//
// One rc_light_sampling_backward call = rc_render_material's forward up to the batched secondary trace (material_* in
// rc_api.hip, on set 0 and WS_SECONDARY) -> the light head's recompute on k_gemm (h0, h1, vmf_params; "ls:" buffers) ->
// k_light_sampling_loss_bwd (per-point loss sums, d loss / d vmf_params) -> k_interlevel_reduce (the loss, fixed order) ->
// with a gradient buffer: the three dense layers' backward on k_gemm (input gradients masked by ReLU', weight gradients
// over fixed K slices of points, added up by k_sum_parts in slice order) and rc_hashgrid_backward of the light grid.

namespace {

constexpr int kLightGrid = 5;                  // the handle's grid id of params/LightSampler/light_grid
constexpr int kLightWidth = 32;                // the light head's input: the light grid's features (RcLightHeadArgs)

// params/LightSampler: light_grid tables in level order, then layers_0, layers_1, output_layer (kernel, bias each)
std::vector<GradSeg> light_grad_segments(rc_handle* h) {
  const GridState& gs = h->grids[kLightGrid];
  int64_t off = 0;
  std::vector<GradSeg> v = grid_grad_segments(gs, off);
  dense_grad_segments(v, off, "params/LightSampler/layers_0", (int)gs.sizes.size() * gs.cfg.num_features, 64);
  dense_grad_segments(v, off, "params/LightSampler/layers_1", 64, 64);
  dense_grad_segments(v, off, "params/LightSampler/output_layer", 64, 5 * h->cfg.num_vmf);
  return v;
}

}  // namespace

int64_t rc_light_grad_size(rc_handle* h) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (h->grids[kLightGrid].sizes.empty()) return fail(h, RC_ERR_UNSUPPORTED, "rc_light_grad_size: no light grid");
  return grad_size(light_grad_segments(h));
  RC_CATCH(h)
}

int rc_light_grad_layout(rc_handle* h, rc_grad_segment* segs, int32_t capacity, int32_t* count) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (h->grids[kLightGrid].sizes.empty()) return fail(h, RC_ERR_UNSUPPORTED, "rc_light_grad_layout: no light grid");
  return copy_segments(h, light_grad_segments(h), segs, capacity, count, "rc_light_grad_layout");
  RC_CATCH(h)
}

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
  const float* Wl[3] = {raw[RAW_LIGHT_0].kernel.p, raw[RAW_LIGHT_1].kernel.p, raw[RAW_LIGHT_OUT].kernel.p};
  const float* bl[3] = {raw[RAW_LIGHT_0].bias.p, raw[RAW_LIGHT_1].bias.p, raw[RAW_LIGHT_OUT].bias.p};
  const int din[3] = {kLightWidth, 64, 64}, dout[3] = {64, 64, 640};
  const float* xin[3] = {x.l_feat.p, y.h0.p, y.h1.p};
  float* yout[3] = {y.h0.p, y.h1.p, y.vp.p};
  for (int l = 0; l < 3; ++l) {
    RcGemmArgs g{};
    g.M = (int)n; g.N = dout[l]; g.K = din[l];
    g.a = xin[l]; g.sai = din[l]; g.sak = 1; g.b = Wl[l]; g.sbk = dout[l]; g.sbj = 1;
    g.c = yout[l]; g.sci = dout[l]; g.scj = 1; g.bias = bl[l]; g.relu = l < 2; g.kslice = g.K;
    rc_launch_gemm(g, 1, st);
  }
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
    for (int pass = 0; pass < 2; ++pass) {
      RcGemmArgs g{};
      g.M = pass == 0 ? din[l] : 1; g.N = dout[l]; g.K = n;
      g.a = pass == 0 ? xin[l] : y.ones.p; g.sai = pass == 0 ? 1 : 0; g.sak = pass == 0 ? din[l] : 0;
      g.b = dyl[l]; g.sbk = dout[l]; g.sbj = 1; g.c = y.part.p; g.sci = dout[l]; g.scj = 1;
      g.kslice = kDataKSlice; g.spart = (int64_t)g.M * dout[l];
      rc_launch_gemm(g, (int)Z, st);
      rc_launch_sum_parts(y.part.p, (int)Z, g.spart, light_grads + segs[T + 2 * l + pass].offset, st);
    }
    // d input = dY W^T (zero where the input's ReLU was off)
    RcGemmArgs g{};
    g.M = (int)n; g.N = din[l]; g.K = dout[l];
    g.a = dyl[l]; g.sai = dout[l]; g.sak = 1; g.b = Wl[l]; g.sbk = 1; g.sbj = dout[l];
    g.c = dxl[l]; g.sci = din[l]; g.scj = 1; g.kslice = g.K;
    g.mask = hmask[l]; g.smi = din[l]; g.smj = 1;
    rc_launch_gemm(g, 1, st);
  }
  RC_HIP(h, hipGetLastError());
  // 5. the light grid's tables (contracted shading points), at the head of the layout
  return rc_hashgrid_backward(h, kLightGrid, x.m_pts.p, n, y.dfeat.p, light_grads, 1, stream_v);
  RC_CATCH(h)
}

int rc_light_regularizer(rc_handle* h, float mult, float* light_grads, float* loss, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (!std::isfinite(mult)) return fail(h, RC_ERR_INVALID_ARG, "rc_light_regularizer: mult must be finite");
  if (!loss) return fail(h, RC_ERR_INVALID_ARG, "rc_light_regularizer: null loss");
  if (h->transient) return fail(h, RC_ERR_UNSUPPORTED, "rc_light_regularizer: not available on a time-resolved cache handle");
  const GridState& gs = h->grids[kLightGrid];
  const int T = (int)gs.sizes.size();
  if (T < 1 || T > RC_MAX_GRID_LEVELS) return fail(h, RC_ERR_UNSUPPORTED, "rc_light_regularizer: unexpected grid levels");
  for (int t = 0; t < T; ++t)
    if (!gs.loaded[t]) return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: " + gs.prefix + "/" + level_name(gs.cfg, gs.sizes, gs.sizes[t]));
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  WsUse use(h, WS_LIGHT, st);
  int rc;
  if ((rc = use.rc)) return rc;
  LightWs& y = ws_extra<LightWs>(use.s);
  const int B = rc_grid_l2_blocks();
  if ((rc = ws_alloc(h, y.reg_part, 2 * (int64_t)T * B))) return rc;     // doubles
  double* part = reinterpret_cast<double*>(y.reg_part.p);
  int64_t off = 0;
  const std::vector<GradSeg> segs = grid_grad_segments(gs, off);     // the tables lead the light layout
  RcGridL2Reduce rr{};
  rr.mult = mult; rr.tables = T;
  for (int t = 0; t < T; ++t) {
    const int64_t count = segs[t].size;
    rr.count[t] = count;
    rc_launch_grid_l2_bwd(gs.dev.lvl[t].table, count, (float)((double)mult / (double)count),
                          light_grads ? light_grads + segs[t].offset : nullptr, part + (int64_t)t * B, st);
  }
  rc_launch_grid_l2_reduce(part, rr, loss, st);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}
