// Host side of rc_transient_data_backward, _kind, _sampler (rc_transient_sampler.hip) and rc_dtof_to_itof (rc_transient_bwd.hip); included by rc_api.hip.
//
// One call = rc_render_transient itself (its "rgb" histograms to "td:rgb") -> k_transient_loss[_kinds] (G, the filter's transpose
// Gt, the per-ray loss and mse sums) -> k_interlevel_reduce (the two scalars, fixed order) -> per chunk of kRcTdChunkRays
// rays: k_transient_bins_bwd (the integrator's adjoint, the heads' recompute, dZ of both heads into the chunk's buffers,
// the per-sample adjoints) and, on k_gemm_tile, dX = dZ W^T of both heads into "td:d_t_irr" / "td:d_t_slf" and, with a
// gradient buffer, dW += X^T dZ and db over fixed K slices (rc_train_host.inc's dense_*_tile).

namespace {

enum { TH_IRR, TH_SLF, TH_COUNT };

int upload_transient_heads(rc_handle* h, const std::vector<GradSeg>& segs) {
  std::string missing;
  std::vector<float> v;
  const char* const paths[TH_COUNT] = {"params/Cache/Shader/transient_indirect_layer",
                                       "params/Cache/Shader/SurfaceLightField/output_rgba_layer"};
  for (int i = 0; i < TH_COUNT; ++i) {
    const HostLayer* L = need(h, paths[i], missing);
    if (!L) continue;
    if (L->in != segs[2 * i].shape[0] || L->out != segs[2 * i].shape[1])
      return fail(h, RC_ERR_UNSUPPORTED, std::string("rc_transient_data_backward: unexpected shape of ") + paths[i]);
    v.insert(v.end(), L->kernel.begin(), L->kernel.end());
    v.insert(v.end(), L->bias.begin(), L->bias.end());
  }
  if (!missing.empty()) return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: " + missing);
  return upload(h, h->thead_w, v);
}

int check_transient_loss_kind(rc_handle* h, const std::string& who, const rc_transient_data_loss_kind* kind);
int launch_transient_loss(rc_handle* h, const rc_transient_data_loss_kind* kind, const RcTransLossArgs& la, hipStream_t st);   // below

// Both entries: `kind` is null for rc_transient_data_backward.  Steps 1 and 3 do not depend on it.
int transient_data_backward_impl(rc_handle* h, const std::string& who, const rc_rays* rays, const float* cam_origins, int64_t n,
                                 const rc_randoms* rnd, const float* gt, const float* rgb_nocorr, const float* gt_nocorr, const float* lossmult,
                                 const rc_transient_data_loss* cfg, const rc_transient_data_loss_kind* kind, float* head_grads, float* losses, void* stream_v) {
  if (!h->transient) return fail(h, RC_ERR_UNSUPPORTED, who + ": needs a time-resolved cache handle (rc_set_transient)");
  if (h->tcfg.use_occlusions) return fail(h, RC_ERR_UNSUPPORTED, who + ": the occlusion variant is not offered (a vis_only feature)");
  if (!rays || !cfg) return fail(h, RC_ERR_INVALID_ARG, who + ": null rays/cfg");
  if (n < 0) return fail(h, RC_ERR_INVALID_ARG, who + ": negative n_rays");
  if (!std::isfinite(cfg->mult) || !std::isfinite(cfg->gauss_mult) || !std::isfinite(cfg->gauss_constant_scale) ||
      !std::isfinite(cfg->exponent) || !std::isfinite(cfg->eps) || !std::isfinite(cfg->clip_val) || !(cfg->thresh == cfg->thresh))
    return fail(h, RC_ERR_INVALID_ARG, who + ": the loss constants must be finite, thresh not NaN");
  if (int rc = check_transient_loss_kind(h, who, kind)) return rc;
  if (n == 0) return RC_OK;
  if (!gt || !losses) return fail(h, RC_ERR_INVALID_ARG, who + ": null gt/losses");
  const rc_transient_config& t = h->tcfg;
  const int64_t np = n * 32;
  const std::vector<GradSeg> segs = transient_head_segments(h);
  if (t.n_bins != kRcTdBins || segs[0].shape[0] != 64 || segs[0].shape[1] != kRcTdHist || segs[2].shape[0] != 128 ||
      segs[2].shape[1] != kRcTdHist + 1)
    return fail(h, RC_ERR_UNSUPPORTED, who + ": unexpected head widths");
  RoctxScope roctx_call(who.c_str());
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  int rc;
  WsUse use_d(h, WS_TRANSDATA, st);
  if ((rc = use_d.rc)) return rc;
  TransDataWs& y = ws_extra<TransDataWs>(use_d.s);
  const int64_t CH = n < kRcTdChunkRays ? n : kRcTdChunkRays, rows = CH * 32;
  const int64_t nslices = (rows + kDataKSlice - 1) / kDataKSlice;
  if ((rc = ws_alloc(h, {{y.rgb, n * kRcTdHist}, {y.G, n * kRcTdHist}, {y.Gt, n * kRcTdHist}, {y.loss_ray, 2 * n},
                         {y.dz_irr, rows * kRcTdHist}, {y.dz_slf, rows * kRcTdLdSlf}, {y.x_irr, rows * 64}, {y.x_slf, rows * 128},
                         {y.part, nslices * 128 * (int64_t)(kRcTdHist + 1)}, {y.ones, 1}, {y.d_t_irr, np * 64},
                         {y.d_t_slf, np * 128}, {y.d_tint_ibrdf, np * 3}, {y.d_direct, np * 3}, {y.d_weights, np}})))
    return rc;

  // 1. rc_render_transient's forward, the call itself
  rc_transient_outputs to;
  memset(&to, 0, sizeof(to));
  to.ptr[RC_TOUT_RGB] = y.rgb.p;
  if ((rc = rc_render_transient(h, rays, cam_origins, n, rnd, nullptr, &to, stream_v))) return rc;

  // 2. the loss, G and the filter's transpose of it
  roctx_stage("transient data loss");
  RcTransLossArgs la{};
  la.n = n; transient_taps(h, la);
  la.rgb = y.rgb.p; la.gt = gt; la.rgb_nocorr = rgb_nocorr; la.gt_nocorr = gt_nocorr; la.lossmult = lossmult;
  la.coef = (float)((double)cfg->mult / (3.0 * (double)n));
  la.gauss = (float)(2.0 * (double)cfg->gauss_constant_scale * (double)cfg->gauss_constant_scale * (double)cfg->gauss_mult);
  la.exponent = cfg->exponent; la.eps = cfg->eps; la.clip_val = cfg->clip_val; la.thresh = cfg->thresh;
  la.use_gt = cfg->use_gt_rawnerf != 0; la.use_combined = cfg->use_combined_rawnerf != 0;
  la.G = y.G.p; la.Gt = y.Gt.p; la.loss_ray = y.loss_ray.p;
  if ((rc = launch_transient_loss(h, kind, la, st))) return rc;      // k_transient_loss or k_transient_loss_kinds
  RcInterlevelReduce rr{};
  rr.mult[0] = rr.mult[1] = cfg->mult; rr.count[0] = rr.count[1] = 3.0 * (double)n;
  rc_launch_interlevel_reduce(y.loss_ray.p, n, 2, rr, losses, st);
  RC_HIP(h, hipGetLastError());

  // 3. the integrator's adjoint and the heads, chunk by chunk (the forward's buffers: set 0)
  if (h->thead_gen != h->layers_gen) {
    if ((rc = upload_transient_heads(h, segs))) return rc;
    h->thead_gen = h->layers_gen;
  }
  WsUse use(h, WS_RENDER0, st);
  if ((rc = use.rc)) return rc;
  RenderWs& w = use.s.r;
  Dense L[TH_COUNT];                     // h->thead_w: kernel then bias of each layer, the layout's order and offsets
  for (int l = 0; l < TH_COUNT; ++l)
    L[l] = Dense{(int)segs[2 * l].shape[0], (int)segs[2 * l].shape[1], h->thead_w.p + segs[2 * l].offset, h->thead_w.p + segs[2 * l + 1].offset};
  RC_HIP(h, hipMemsetD32Async((hipDeviceptr_t)y.ones.p, 0x3f800000, 1, st));     // 1.0f: the A operand of a bias gradient
  RcTransBinsBwdArgs b{};
  transient_in(h, w, n, b);
  b.w_irr = L[TH_IRR].w; b.b_irr = L[TH_IRR].b; b.w_slf = L[TH_SLF].w; b.b_slf = L[TH_SLF].b;
  b.G = y.G.p; b.Gt = y.Gt.p;
  b.dz_irr = y.dz_irr.p; b.dz_slf = y.dz_slf.p; b.x_irr = y.x_irr.p; b.x_slf = y.x_slf.p;
  b.d_tib = y.d_tint_ibrdf.p; b.d_direct = y.d_direct.p; b.d_weights = y.d_weights.p;
  roctx_stage("transient data loss: integrator and heads backward");
  for (int64_t r0 = 0; r0 < n; r0 += CH) {
    const int64_t C = n - r0 < CH ? n - r0 : CH, M = C * 32;
    b.r0 = r0; b.C = C;
    rc_launch_transient_bins_bwd(b, st);
    // dX = dZ W^T (the alpha column of dZ_slf holds zeros)
    dense_dx_tile(L[TH_IRR], M, y.dz_irr.p, kRcTdHist, y.d_t_irr.p + r0 * 32 * 64, 64, 0, 64, nullptr, false, st);
    dense_dx_tile(L[TH_SLF], M, y.dz_slf.p, kRcTdLdSlf, y.d_t_slf.p + r0 * 32 * 128, 128, 0, 128, nullptr, false, st);
    if (head_grads) {
      dense_wgrad_tile(L[TH_IRR], M, y.x_irr.p, 64, y.dz_irr.p, kRcTdHist, y.ones.p, y.part.p, head_grads, &segs[2 * TH_IRR], st);
      dense_wgrad_tile(L[TH_SLF], M, y.x_slf.p, 128, y.dz_slf.p, kRcTdLdSlf, y.ones.p, y.part.p, head_grads, &segs[2 * TH_SLF], st);
    }
    RC_HIP(h, hipGetLastError());
  }
  return RC_OK;
}

// The modulation table of (n_pairs, frequency, phase_shift) at the handle's exposure_time in h->itof_w: built and uploaded
// when the pairs or the exposure_time differ from the cached ones.  The calls that read the previous table are waited for.
int ensure_itof_table(rc_handle* h, int n_pairs, const double* frequency, const double* phase_shift, hipStream_t st) {
  std::vector<double> key{(double)h->tcfg.exposure_time};
  for (int p = 0; p < n_pairs; ++p) { key.push_back(frequency[p]); key.push_back(phase_shift[p]); }
  if (h->itof_w.p && key == h->itof_key) return RC_OK;
  RC_HIP(h, hipStreamSynchronize(st));
  h->itof_key.clear();
  if (int rc = upload(h, h->itof_w, rc_itof_table(kRcTdBins, (double)h->tcfg.exposure_time, n_pairs, frequency, phase_shift)))
    return rc;
  h->itof_key = key;
  return RC_OK;
}

int check_itof_pairs(rc_handle* h, const std::string& who, int n_pairs, const double* frequency, const double* phase_shift) {
  if (n_pairs < 0 || n_pairs > RC_ITOF_MAX_PAIRS)
    return fail(h, RC_ERR_INVALID_ARG, who + ": n_pairs outside [0, RC_ITOF_MAX_PAIRS]");
  if (n_pairs > 0 && (!frequency || !phase_shift)) return fail(h, RC_ERR_INVALID_ARG, who + ": null frequency/phase_shift");
  for (int p = 0; p < n_pairs; ++p)
    if (!std::isfinite(frequency[p]) || !std::isfinite(phase_shift[p]))
      return fail(h, RC_ERR_INVALID_ARG, who + ": the frequencies and phase shifts must be finite");
  return RC_OK;
}

// The refusals of rc_transient_data_backward_kind's own fields (nothing is launched); no kind, nothing to refuse.
int check_transient_loss_kind(rc_handle* h, const std::string& who, const rc_transient_data_loss_kind* kind) {
  if (!kind) return RC_OK;
  if (kind->loss_type < 0 || kind->loss_type >= RC_TLOSS_COUNT) return fail(h, RC_ERR_INVALID_ARG, who + ": unknown loss_type");
  return check_itof_pairs(h, who, kind->n_pairs, kind->frequency, kind->phase_shift);
}

// Step 2's kernel: the default reading goes to k_transient_loss whichever entry asks for it (bitwise the same results),
// every other one to k_transient_loss_kinds with the modulation table where it is read.
int launch_transient_loss(rc_handle* h, const rc_transient_data_loss_kind* kind, const RcTransLossArgs& la, hipStream_t st) {
  if (!kind || (kind->loss_type == RC_TLOSS_RAWNERF_TRANSIENT_UNBIASED && !kind->use_itof)) {
    rc_launch_transient_loss(la, st);
    return RC_OK;
  }
  RcTransLossKindArgs ka{};
  ka.base = la; ka.kind = kind->loss_type; ka.use_itof = kind->use_itof != 0;
  ka.n_rows = 2 * kind->n_pairs + 1;
  const bool itof_kind = kind->loss_type >= RC_TLOSS_MSE_ITOF;
  ka.q = kind->use_itof ? (float)(1.0 / (double)(itof_kind ? ka.n_rows : kRcTdBins)) : 1.0f;      // train_utils.py:622-623
  if (itof_kind || kind->use_itof) {
    if (int rc = ensure_itof_table(h, kind->n_pairs, kind->frequency, kind->phase_shift, st)) return rc;
    ka.W = h->itof_w.p;
  }
  rc_launch_transient_loss_kinds(ka, st);
  return RC_OK;
}

}  // namespace

int rc_transient_data_backward(rc_handle* h, const rc_rays* rays, const float* cam_origins, int64_t n, const rc_randoms* rnd,
                               const float* gt, const float* rgb_nocorr, const float* gt_nocorr, const float* lossmult,
                               const rc_transient_data_loss* cfg, float* head_grads, float* losses, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  return transient_data_backward_impl(h, "rc_transient_data_backward", rays, cam_origins, n, rnd, gt, rgb_nocorr, gt_nocorr,
                                      lossmult, cfg, nullptr, head_grads, losses, stream_v);
  RC_CATCH(h)
}

int rc_transient_data_backward_kind(rc_handle* h, const rc_rays* rays, const float* cam_origins, int64_t n, const rc_randoms* rnd,
                                    const float* gt, const float* rgb_nocorr, const float* gt_nocorr, const float* lossmult,
                                    const rc_transient_data_loss_kind* cfg, float* head_grads, float* losses, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_transient_data_backward_kind";
  // a null cfg: the handle's refusals first, as the other entry orders them
  if (!cfg && h->transient && !h->tcfg.use_occlusions) return fail(h, RC_ERR_INVALID_ARG, who + ": null rays/cfg");
  return transient_data_backward_impl(h, who, rays, cam_origins, n, rnd, gt, rgb_nocorr, gt_nocorr, lossmult,
                                      cfg ? &cfg->base : nullptr, cfg, head_grads, losses, stream_v);
  RC_CATCH(h)
}

// rc_transient_data_backward_kind, then the weights path of its gradient into the last level's segments of the sampler
// layout: k_transient_weights_bwd ("td:d_weights" -> "td:d_density" on the forward's density, tdist and weights of set 0)
// and rc_density_backward of the last level at the forward's means (density_backward_chunks).
// The launch order is the one it always had; "td:points" is requested inside density_backward_chunks, behind the launch of
// k_transient_weights_bwd (a buffer that has to grow is reallocated there, as in the mask loss).
int rc_transient_data_backward_sampler(rc_handle* h, const rc_rays* rays, const float* cam_origins, int64_t n, const rc_randoms* rnd,
                                       const float* gt, const float* rgb_nocorr, const float* gt_nocorr, const float* lossmult,
                                       const rc_transient_data_loss_kind* cfg, float* head_grads, float* sampler_grads,
                                       float* losses, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_transient_data_backward_sampler";
  if (!cfg && h->transient && !h->tcfg.use_occlusions) return fail(h, RC_ERR_INVALID_ARG, who + ": null rays/cfg");
  int rc;
  if ((rc = transient_data_backward_impl(h, who, rays, cam_origins, n, rnd, gt, rgb_nocorr, gt_nocorr, lossmult,
                                         cfg ? &cfg->base : nullptr, cfg, head_grads, losses, stream_v)))
    return rc;
  if (n == 0 || !sampler_grads) return RC_OK;
  const int NL = h->cfg.num_levels;
  const int S2 = h->cfg.num_samples[NL - 1];               // 32 (rc_set_transient)
  const int64_t np = n * S2;
  hipStream_t st = (hipStream_t)stream_v;
  int64_t off[RC_MAX_LEVELS] = {};
  (void)transient_sampler_segments(h, off);
  WsUse use_d(h, WS_TRANSDATA, st);
  if ((rc = use_d.rc)) return rc;
  TransDataWs& y = ws_extra<TransDataWs>(use_d.s);
  if ((rc = ws_alloc(h, y.d_density, np))) return rc;
  WsUse use(h, WS_RENDER0, st);          // the forward's buffers, as step 3 of the shared body reads them
  if ((rc = use.rc)) return rc;
  RenderWs& w = use.s.r;
  RcTransWeightsBwdArgs a{};
  a.n = n; a.S = S2; a.d_weights = y.d_weights.p; a.weights = w.weights[NL - 1].p; a.density = w.density[NL - 1].p;
  a.tdist = w.tdist[NL - 1].p; a.directions = rays->directions; a.d_density = y.d_density.p;
  rc_launch_transient_weights_bwd(a, st);
  return density_backward_chunks(h, NL - 1, w.means[NL - 1].p, np, y.points, y.d_density.p, nullptr, sampler_grads + off[NL - 1], st);
  RC_CATCH(h)
}

int rc_dtof_to_itof(rc_handle* h, const float* dtof, int64_t n, int32_t n_pairs, const double* frequency,
                    const double* phase_shift, float* itof, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_dtof_to_itof";
  if (!h->transient) return fail(h, RC_ERR_UNSUPPORTED, who + ": needs a time-resolved cache handle (rc_set_transient)");
  if (h->tcfg.n_bins != kRcTdBins) return fail(h, RC_ERR_UNSUPPORTED, who + ": unexpected n_bins");
  if (n < 0) return fail(h, RC_ERR_INVALID_ARG, who + ": negative n");
  if (int rc = check_itof_pairs(h, who, n_pairs, frequency, phase_shift)) return rc;
  if (n == 0) return RC_OK;
  if (!dtof || !itof) return fail(h, RC_ERR_INVALID_ARG, who + ": null dtof/itof");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  if (int rc = ensure_itof_table(h, n_pairs, frequency, phase_shift, st)) return rc;
  RcDtofToItofArgs a{};
  a.n = n; a.n_rows = 2 * n_pairs + 1; a.W = h->itof_w.p; a.x = dtof; a.out = itof;
  rc_launch_dtof_to_itof(a, st);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}
