// Host side of rc_data_backward (rc_data.hip); included by rc_api.hip.
//
// One call = the training forward (enqueue_all's launch-per-stage cache pass on the workspace set WS_DATA, the caller's
// jitter and anneal) -> k_data_loss_bwd (per-ray charb sums, d loss / d density and d loss / d rgb_s of every last-level sample) ->
// k_interlevel_reduce (the loss, fixed order) -> with a gradient buffer, per chunk of kDataChunk samples: the shader
// recompute and backward as dense layers on k_gemm (rc_train_host.inc), their weight gradients (K = the chunk's samples),
// d feature64 += W_n^T d pred_raw, rc_density_backward of the last level and rc_hashgrid_backward of the appearance grid.

namespace {

int upload_data_weights(rc_handle* h) {
  std::string missing;
  std::vector<float> v;
  for (int i = 0; i < DL_COUNT; ++i) {
    const HostLayer* L = need(h, data_layer_path(h, i), missing);
    if (!L) continue;
    if (L->in != kDataLayers[i].in || L->out != kDataLayers[i].out)
      return fail(h, RC_ERR_UNSUPPORTED, "rc_data_backward: unexpected shape of " + data_layer_path(h, i));
    v.insert(v.end(), L->kernel.begin(), L->kernel.end());
    v.insert(v.end(), L->bias.begin(), L->bias.end());
  }
  if (!missing.empty()) return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: " + missing);
  return upload(h, h->data_w, v);
}

}  // namespace

int rc_data_backward(rc_handle* h, const rc_rays* rays, const float* gt_rgb, const float* lossmult, int64_t n,
                     const rc_randoms* rnd, float anneal, float charb_padding, float mult, float* density_grads,
                     float* shader_grads, float* loss, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const rc_config& c = h->cfg;
  const int NL = c.num_levels;
  if (n < 0) return fail(h, RC_ERR_INVALID_ARG, "rc_data_backward: negative n_rays");
  if (!rays) return fail(h, RC_ERR_INVALID_ARG, "rc_data_backward: null rays");
  if (!(anneal >= 0.0f) || !std::isfinite(anneal)) return fail(h, RC_ERR_INVALID_ARG, "rc_data_backward: anneal must be finite and >= 0");
  if (!std::isfinite(charb_padding) || !std::isfinite(mult)) return fail(h, RC_ERR_INVALID_ARG, "rc_data_backward: charb_padding and mult must be finite");
  if (h->transient) return fail(h, RC_ERR_UNSUPPORTED, "rc_data_backward: not available on a time-resolved cache handle");
  if (n == 0) return RC_OK;
  if (!gt_rgb || !loss) return fail(h, RC_ERR_INVALID_ARG, "rc_data_backward: null gt_rgb/loss");
  int rc;
  if ((rc = check_rays(h, rays, "rc_data_backward"))) return rc;
  const int S2 = c.num_samples[NL - 1];
  if (S2 < 1 || S2 > 32) return fail(h, RC_ERR_UNSUPPORTED, "rc_data_backward: needs <= 32 samples on the last level");
  if (h->grids[NL - 1].dev.num_levels * h->grids[NL - 1].dev.num_features != 32 ||
      h->grids[3].dev.num_levels * h->grids[3].dev.num_features != 32)
    return fail(h, RC_ERR_UNSUPPORTED, "rc_data_backward: needs 32 features on the last density grid and the appearance grid");
  RoctxScope roctx_call("rc_data_backward");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  if ((rc = ensure_packed(h))) return rc;
  const bool grads = density_grads || shader_grads;
  if (grads && h->data_gen != h->layers_gen) {
    if ((rc = upload_data_weights(h))) return rc;
    h->data_gen = h->layers_gen;
  }
  WsUse use(h, WS_DATA, st);
  if ((rc = use.rc)) return rc;
  RenderWs& w = use.s.r;
  DataWs& x = ws_extra<DataWs>(use.s);
  const int64_t np = n * S2;
  if ((rc = ensure_workspace(h, w, n)) || (rc = ws_alloc(h, {{x.rgb, 3 * n}, {x.loss_ray, n}, {x.d_density, np}, {x.d_rgbs, 3 * np}})))
    return rc;

  // 1. the training forward: rc_render_rays' launch-per-stage cache pass, no analytic normals
  RenderArgs A = cache_pass(rays, rnd, n);
  A.anneal = anneal;
  A.out.ptr[RC_OUT_RGB] = x.rgb.p;
  enqueue_all(h, A, w, st);

  // 2. the charb term, d loss / d rgb_s and d loss / d density
  RcDataLossArgs la{};
  la.n = n; la.S = S2; la.rgb = x.rgb.p; la.gt = gt_rgb; la.lossmult = lossmult;
  la.weights = w.weights[NL - 1].p; la.density = w.density[NL - 1].p; la.tdist = w.tdist[NL - 1].p; la.shade = w.shade.p;
  la.directions = rays->directions; la.bg = c.bg_intensity; la.padding = charb_padding;
  la.coef = (float)((double)mult / (3.0 * (double)n));
  la.loss_ray = x.loss_ray.p; la.d_density = x.d_density.p; la.d_rgbs = x.d_rgbs.p;
  rc_launch_data_loss_bwd(la, st);
  RcInterlevelReduce rr{};
  rr.mult[0] = mult; rr.count[0] = 3.0 * (double)n;
  rc_launch_interlevel_reduce(x.loss_ray.p, n, 1, rr, loss, st);
  RC_HIP(h, hipGetLastError());
  if (!grads) return RC_OK;

  // 3-5. the shader backward, chunk by chunk
  const int64_t CH = np < kDataChunk ? np : kDataChunk;
  const int64_t nslices = (CH + kDataKSlice - 1) / kDataKSlice;
  if ((rc = ws_alloc(h, {{x.f96, CH * 96}, {x.heads, CH * 10}, {x.p3, CH * 3}, {x.ib_in, CH * 129}, {x.x328, CH * 328},
                         {x.s0, CH * 128}, {x.s1, CH * 128}, {x.sb, CH * 128}, {x.i1, CH * 64}, {x.i2, CH * 64}, {x.io, CH * 1},
                         {x.so, CH * 3}, {x.dheads, CH * 10}, {x.dio, CH * 1}, {x.dso, CH * 3}, {x.dsb, CH * 128},
                         {x.dx328, CH * 328}, {x.ds1, CH * 128}, {x.ds0, CH * 128}, {x.di2, CH * 64}, {x.di1, CH * 64},
                         {x.dib_in, CH * 129}, {x.db128, CH * 128}, {x.dp3, CH * 3}, {x.df96, CH * 96}, {x.dfeat, CH * 64},
                         {x.dapp, CH * 32}, {x.part, nslices * 328 * 128}, {x.ones, 1}, {x.points, 3 * np}})))
    return rc;
  RC_HIP(h, hipMemsetD32Async((hipDeviceptr_t)x.ones.p, 0x3f800000, 1, st));     // 1.0f: the A operand of a bias gradient
  rc_launch_points_aos(w.means[NL - 1].p, np, x.points.p, st);
  int kseg[DL_COUNT];
  int64_t app_off = 0;
  const std::vector<GradSeg> segs = shader_grad_segments(h, kseg, &app_off);
  Dense L[DL_COUNT];                     // h->data_w: every layer's kernel then bias, in layer order
  for (int64_t l = 0, at = 0; l < DL_COUNT; ++l) {
    const int in = kDataLayers[l].in, out = kDataLayers[l].out;
    L[l] = Dense{in, out, h->data_w.p + at, h->data_w.p + at + in * out};
    at += in * out + out;
  }

  for (int64_t c0 = 0; c0 < np; c0 += CH) {
    const int64_t C = np - c0 < CH ? np - c0 : CH;
    RcShaderBwdArgs sa{};
    sa.C = C; sa.c0 = c0; sa.np = np; sa.S = S2;
    sa.hbuf = w.hbuf.p; sa.app = w.app.p; sa.viewdirs = rays->viewdirs;
    sa.ide = reinterpret_cast<const RcIdeTable*>(h->ide_table.p);
    sa.roughness_bias = c.roughness_bias; sa.ambient_bias = c.ambient_irradiance_bias; sa.irradiance_bias = c.irradiance_bias;
    sa.slf_ambient_bias = c.slf_ambient_bias; sa.rgb_max = c.rgb_max; sa.d_rgbs = x.d_rgbs.p;
    sa.f96 = x.f96.p; sa.heads = x.heads.p; sa.p3 = x.p3.p; sa.ib_in = x.ib_in.p; sa.x328 = x.x328.p; sa.io = x.io.p; sa.so = x.so.p;
    sa.dheads = x.dheads.p; sa.dio = x.dio.p; sa.dso = x.dso.p; sa.dib_in = x.dib_in.p; sa.dx328 = x.dx328.p;
    sa.db128 = x.db128.p; sa.dp3 = x.dp3.p;

    // recompute: feature96, heads, pred_raw, bottleneck, IDE, integrated BRDF, SLF
    rc_launch_shader_stage(sa, 0, st);
    dense_fwd(L[DL_ROUGH], C, x.f96.p, 96, x.heads.p + 0, 10, false, st);
    dense_fwd(L[DL_AMB], C, x.f96.p, 96, x.heads.p + 1, 10, false, st);
    dense_fwd(L[DL_TINT], C, x.f96.p, 96, x.heads.p + 4, 10, false, st);
    dense_fwd(L[DL_IRR], C, x.f96.p, 96, x.heads.p + 7, 10, false, st);
    dense_fwd(L[DL_PRED], C, x.f96.p, 96, x.p3.p, 3, false, st);
    dense_fwd(L[DL_BOTT], C, x.f96.p, 96, x.x328.p + 128, 328, false, st);
    dense_fwd(L[DL_BOTT], C, x.f96.p, 96, x.ib_in.p, 129, false, st);
    rc_launch_shader_stage(sa, 1, st);
    dense_fwd(L[DL_I0], C, x.ib_in.p, 129, x.i1.p, 64, true, st);
    dense_fwd(L[DL_I1], C, x.i1.p, 64, x.i2.p, 64, true, st);
    dense_fwd(L[DL_IO], C, x.i2.p, 64, x.io.p, 1, false, st);
    dense_fwd(L[DL_S0], C, x.x328.p + 128, 328, x.s0.p, 128, true, st);
    dense_fwd(L[DL_S1], C, x.s0.p, 128, x.s1.p, 128, true, st);
    dense_fwd(L[DL_S2], C, x.s1.p, 128, x.x328.p, 328, true, st);
    dense_fwd(L[DL_SB], C, x.x328.p, 328, x.sb.p, 128, true, st);
    dense_fwd(L[DL_SO], C, x.sb.p, 128, x.so.p, 3, false, st);
    // backward
    rc_launch_shader_stage(sa, 2, st);
    dense_dx(L[DL_SO], C, x.dso.p, 3, x.dsb.p, 128, 0, 128, x.sb.p, false, st);
    dense_dx(L[DL_SB], C, x.dsb.p, 128, x.dx328.p, 328, 0, 128, x.x328.p, false, st);
    dense_dx(L[DL_SB], C, x.dsb.p, 128, x.dx328.p, 328, 128, 200, nullptr, false, st);
    dense_dx(L[DL_S2], C, x.dx328.p, 328, x.ds1.p, 128, 0, 128, x.s1.p, false, st);
    dense_dx(L[DL_S1], C, x.ds1.p, 128, x.ds0.p, 128, 0, 128, x.s0.p, false, st);
    dense_dx(L[DL_S0], C, x.ds0.p, 128, x.dx328.p + 128, 328, 0, 200, nullptr, true, st);
    dense_dx(L[DL_IO], C, x.dio.p, 1, x.di2.p, 64, 0, 64, x.i2.p, false, st);
    dense_dx(L[DL_I1], C, x.di2.p, 64, x.di1.p, 64, 0, 64, x.i1.p, false, st);
    dense_dx(L[DL_I0], C, x.di1.p, 64, x.dib_in.p, 129, 0, 129, nullptr, false, st);
    rc_launch_shader_stage(sa, 3, st);
    dense_dx(L[DL_BOTT], C, x.db128.p, 128, x.df96.p, 96, 0, 96, nullptr, false, st);
    dense_dx(L[DL_ROUGH], C, x.dheads.p + 0, 10, x.df96.p, 96, 0, 96, nullptr, true, st);
    dense_dx(L[DL_AMB], C, x.dheads.p + 1, 10, x.df96.p, 96, 0, 96, nullptr, true, st);
    dense_dx(L[DL_TINT], C, x.dheads.p + 4, 10, x.df96.p, 96, 0, 96, nullptr, true, st);
    dense_dx(L[DL_IRR], C, x.dheads.p + 7, 10, x.df96.p, 96, 0, 96, nullptr, true, st);
    dense_dx(L[DL_PRED], C, x.dp3.p, 3, x.df96.p, 96, 0, 64, nullptr, true, st);
    rc_launch_split_feature(x.df96.p, C, x.dfeat.p, x.dapp.p, st);
    RC_HIP(h, hipGetLastError());
    if (shader_grads) {
      auto wgrad = [&](int l, const float* X, int64_t ldx, const float* dY, int64_t ldy) {
        dense_wgrad(L[l], C, X, ldx, dY, ldy, x.ones.p, x.part.p, shader_grads, &segs[kseg[l]], st);
      };
      wgrad(DL_PRED, x.f96.p, 96, x.dp3.p, 3);
      wgrad(DL_BOTT, x.f96.p, 96, x.db128.p, 128);
      wgrad(DL_ROUGH, x.f96.p, 96, x.dheads.p + 0, 10);
      wgrad(DL_AMB, x.f96.p, 96, x.dheads.p + 1, 10);
      wgrad(DL_TINT, x.f96.p, 96, x.dheads.p + 4, 10);
      wgrad(DL_IRR, x.f96.p, 96, x.dheads.p + 7, 10);
      wgrad(DL_I0, x.ib_in.p, 129, x.di1.p, 64);
      wgrad(DL_I1, x.i1.p, 64, x.di2.p, 64);
      wgrad(DL_IO, x.i2.p, 64, x.dio.p, 1);
      wgrad(DL_S0, x.x328.p + 128, 328, x.ds0.p, 128);
      wgrad(DL_S1, x.s0.p, 128, x.ds1.p, 128);
      wgrad(DL_S2, x.s1.p, 128, x.dx328.p, 328);
      wgrad(DL_SB, x.x328.p, 328, x.dsb.p, 128);
      wgrad(DL_SO, x.sb.p, 128, x.dso.p, 3);
      RC_HIP(h, hipGetLastError());
      if ((rc = rc_hashgrid_backward(h, 3, x.points.p + 3 * c0, C, x.dapp.p, shader_grads + app_off, 1, stream_v))) return rc;
    }
    if (density_grads &&
        (rc = rc_density_backward(h, NL - 1, x.points.p + 3 * c0, C, x.d_density.p + c0, x.dfeat.p, density_grads, nullptr, stream_v)))
      return rc;
  }
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}
