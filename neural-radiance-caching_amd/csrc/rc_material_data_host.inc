// Host side of rc_material_data_backward and rc_material_data_backward_env (rc_material_data.hip, rc_envmap_bwd.hip);
// included by rc_api.hip.
//
// One call = rc_render_material itself (every step, kernels and launch order unchanged; its primary composite to
// "md:cache_rgb" / "md:cache_acc", its "rgb" not written) -> k_material_data_bwd (the integration's recompute, the rebuilt
// rgb to "md:rgb", the loss terms, with a gradient buffer d loss / d material per point) -> k_material_data_head_bwd (the
// loss sums; with a gradient buffer the head's backward, d loss / d features, the per-workgroup partials) ->
// rc_launch_material_partials_reduce (the loss; the dense segments in workgroup order) -> with a gradient buffer:
// rc_hashgrid_backward of the material grid at the shading points.  With an EnvMap gradient buffer (DESIGN.md §4.13), after
// all of that: k_material_data_env_bwd (d loss / d EnvMap radiance per secondary ray, "md:d_env") -> per chunk of
// kDataChunk secondary rays the EnvMap's fp32 recompute and backward as dense layers on k_gemm_tile (k_envmap_stage,
// dense_*_tile, k_envmap_out_bwd; the thin output layer on k_gemm), the weight gradients over fixed K slices.

namespace {

enum { EL_0, EL_1, EL_2, EL_B, EL_O, EL_COUNT };

int upload_env_weights(rc_handle* h, const std::vector<GradSeg>& segs) {
  std::string missing;
  std::vector<float> v;
  for (int i = 0; i < EL_COUNT; ++i) {
    const std::string path = std::string("params/Cache/EnvMap/") + kEnvLayers[i];
    const HostLayer* L = need(h, path, missing);
    if (!L) continue;
    if (L->in != segs[2 * i].shape[0] || L->out != segs[2 * i].shape[1])
      return fail(h, RC_ERR_UNSUPPORTED, "rc_material_data_backward_env: unexpected shape of " + path);
    v.insert(v.end(), L->kernel.begin(), L->kernel.end());
    v.insert(v.end(), L->bias.begin(), L->bias.end());
  }
  if (!missing.empty()) return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: " + missing);
  return upload(h, h->env_w, v);
}

// The EnvMap's backward over the nsec secondary rays: dirs [nsec][3], d_env [nsec][3] -> envmap_grads += .
int envmap_backward(rc_handle* h, MatDataWs& y, const float* dirs, int64_t nsec, float* envmap_grads, hipStream_t st) {
  const std::vector<GradSeg> segs = envmap_grad_segments(h);
  if (segs[0].shape[0] != kRcEnvIn || segs[0].shape[1] != kRcEnvWidth || segs[6].shape[0] != kRcEnvWidth + kRcEnvIn ||
      segs[6].shape[1] != kRcEnvBott || segs[8].shape[1] != 4)
    return fail(h, RC_ERR_UNSUPPORTED, "rc_material_data_backward_env: unexpected EnvMap widths");
  int rc;
  if (h->env_gen != h->layers_gen) {
    if ((rc = upload_env_weights(h, segs))) return rc;
    h->env_gen = h->layers_gen;
  }
  Dense L[EL_COUNT];                     // h->env_w: every layer's kernel then bias, the layout's order and offsets
  for (int l = 0; l < EL_COUNT; ++l)
    L[l] = Dense{(int)segs[2 * l].shape[0], (int)segs[2 * l].shape[1], h->env_w.p + segs[2 * l].offset, h->env_w.p + segs[2 * l + 1].offset};
  constexpr int W = kRcEnvWidth, B = kRcEnvBott, LX = kRcEnvLdx;
  const int64_t CH = nsec < kDataChunk ? nsec : kDataChunk;
  const int64_t nslices = (CH + kDataKSlice - 1) / kDataKSlice;
  if ((rc = ws_alloc(h, {{y.e_h0, CH * W}, {y.e_h1, CH * W}, {y.e_xb, CH * LX}, {y.e_hb, CH * B}, {y.e_raw, CH * 4},
                         {y.e_draw, CH * 4}, {y.e_dhb, CH * B}, {y.e_dxb, CH * W}, {y.e_dh1, CH * W}, {y.e_dh0, CH * W},
                         {y.e_part, nslices * (int64_t)W * W}, {y.e_ones, 1}})))
    return rc;
  static_assert((kRcEnvWidth + kRcEnvIn) * kRcEnvBott <= kRcEnvWidth * kRcEnvWidth, "e_part holds every layer's K slices");
  RC_HIP(h, hipMemsetD32Async((hipDeviceptr_t)y.e_ones.p, 0x3f800000, 1, st));   // 1.0f: the A operand of a bias gradient
  float* const enc = y.e_xb.p + W;       // the encoded direction's columns of xb
  for (int64_t c0 = 0; c0 < nsec; c0 += CH) {
    const int64_t C = nsec - c0 < CH ? nsec - c0 : CH;
    // recompute (fp32)
    rc_launch_envmap_stage(dirs, c0, C, y.e_xb.p, st);
    dense_fwd_tile(L[EL_0], C, enc, LX, y.e_h0.p, W, true, st);
    dense_fwd_tile(L[EL_1], C, y.e_h0.p, W, y.e_h1.p, W, true, st);
    dense_fwd_tile(L[EL_2], C, y.e_h1.p, W, y.e_xb.p, LX, true, st);
    dense_fwd_tile(L[EL_B], C, y.e_xb.p, LX, y.e_hb.p, B, true, st);
    dense_fwd(L[EL_O], C, y.e_hb.p, B, y.e_raw.p, 4, false, st);        // the thin output layer stays on k_gemm
    // backward: the directions are stopped, so layer_bottleneck's input gradient is needed on layer_2's columns only
    rc_launch_envmap_out_bwd(y.d_env.p, y.e_raw.p, h->cfg.env_rgb_bias, c0, C, y.e_draw.p, st);
    dense_dx(L[EL_O], C, y.e_draw.p, 4, y.e_dhb.p, B, 0, B, y.e_hb.p, false, st);
    {
      // dX[:, 0 .. 256) of the 283-wide input: mask = layer_2's output in xb (row stride 288), dX's row stride 256
      RcGemmArgs g{};
      g.M = (int)C; g.N = W; g.K = B;
      g.a = y.e_dhb.p; g.sai = B; g.sak = 1; g.b = L[EL_B].w; g.sbk = 1; g.sbj = B;
      g.c = y.e_dxb.p; g.sci = W; g.scj = 1; g.mask = y.e_xb.p; g.smi = LX; g.smj = 1; g.kslice = g.K;
      rc_launch_gemm_tile(g, 1, st);
    }
    dense_dx_tile(L[EL_2], C, y.e_dxb.p, W, y.e_dh1.p, W, 0, W, y.e_h1.p, false, st);
    dense_dx_tile(L[EL_1], C, y.e_dh1.p, W, y.e_dh0.p, W, 0, W, y.e_h0.p, false, st);
    auto wgrad = [&](int l, const float* X, int64_t ldx, const float* dY, int64_t ldy) {
      (l == EL_O ? dense_wgrad : dense_wgrad_tile)(L[l], C, X, ldx, dY, ldy, y.e_ones.p, y.e_part.p, envmap_grads, &segs[2 * l], st);
    };
    wgrad(EL_O, y.e_hb.p, B, y.e_draw.p, 4);
    wgrad(EL_B, y.e_xb.p, LX, y.e_dhb.p, B);
    wgrad(EL_2, y.e_h1.p, W, y.e_dxb.p, W);
    wgrad(EL_1, y.e_h0.p, W, y.e_dh1.p, W);
    wgrad(EL_0, enc, LX, y.e_dh0.p, W);
    RC_HIP(h, hipGetLastError());
  }
  return RC_OK;
}

int material_data_backward(rc_handle* h, const rc_rays* rays, const float* gt_rgb, const float* lossmult, int64_t n,
                           const rc_randoms* rnd, const rc_material_randoms* mr, int32_t K, const rc_material_data_loss* cfg,
                           float env_scale, float* material_grads, float* envmap_grads, float* loss, void* stream_v,
                           const std::string& who) {
  if (h->transient) return fail(h, RC_ERR_UNSUPPORTED, who + ": not available on a time-resolved cache handle");
  if (!rays || !mr || !cfg) return fail(h, RC_ERR_INVALID_ARG, who + ": null argument");
  if (n < 0) return fail(h, RC_ERR_INVALID_ARG, who + ": negative n_rays");
  if (!std::isfinite(cfg->mult) || !std::isfinite(cfg->weight) || !std::isfinite(cfg->exponent) || !std::isfinite(cfg->eps) ||
      !std::isfinite(cfg->clip_val) || !(cfg->thresh == cfg->thresh))
    return fail(h, RC_ERR_INVALID_ARG, who + ": mult, weight, exponent, eps and clip_val must be finite, thresh not NaN");
  if (!std::isfinite(env_scale)) return fail(h, RC_ERR_INVALID_ARG, who + ": env_scale must be finite");
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
  // 5. the material grid's tables at the shading points (contracted as rc_render_material's lookup), at the layout's head
  if (grads && (rc = rc_hashgrid_backward(h, kMaterialGrid, x.m_pts.p, n, y.dfeat.p, material_grads, 1, stream_v))) return rc;
  if (!envmap_grads) return RC_OK;
  // 6. d loss / d (EnvMap radiance) of every secondary ray, then the EnvMap's backward at the trace's directions
  roctx_stage("material data loss: EnvMap backward");
  const int64_t nsec = n * (int64_t)(sp.Ks + sp.Kd);
  if ((rc = ws_alloc(h, y.d_env, 3 * nsec))) return rc;
  rc_launch_material_data_env_bwd(a, env_scale, y.d_env.p, st);
  return envmap_backward(h, y, x.sec_dirs.p, nsec, envmap_grads, st);
}

}  // namespace

extern "C" int rc_material_data_backward(rc_handle* h, const rc_rays* rays, const float* gt_rgb, const float* lossmult, int64_t n,
                                         const rc_randoms* rnd, const rc_material_randoms* mr, int32_t K,
                                         const rc_material_data_loss* cfg, float* material_grads, float* loss, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  RoctxScope roctx_call("rc_material_data_backward");
  return material_data_backward(h, rays, gt_rgb, lossmult, n, rnd, mr, K, cfg, 1.0f, material_grads, nullptr, loss, stream_v,
                                "rc_material_data_backward");
  RC_CATCH(h)
}

extern "C" int rc_material_data_backward_env(rc_handle* h, const rc_rays* rays, const float* gt_rgb, const float* lossmult,
                                             int64_t n, const rc_randoms* rnd, const rc_material_randoms* mr, int32_t K,
                                             const rc_material_data_loss* cfg, float env_scale, float* material_grads,
                                             float* envmap_grads, float* loss, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  RoctxScope roctx_call("rc_material_data_backward_env");
  return material_data_backward(h, rays, gt_rgb, lossmult, n, rnd, mr, K, cfg, env_scale, material_grads, envmap_grads, loss,
                                stream_v, "rc_material_data_backward_env");
  RC_CATCH(h)
}
