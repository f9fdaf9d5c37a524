// Host side of rc_eval_shift_invariant (the k_si_* kernels of rc_metrics.hip, DESIGN.md §4.16.1); included by rc_api.hip.
//
// One call = for each search (mse, then ssim under want_ssim), for each di row in the reference's order: k_si_metric (the
// 2 radius_j + 1 metric maps of the row) -> k_si_select (pooling, comparison, the state carried in [H][W] arrays; the last
// row writes the maps and the per-workgroup partial sums); then k_si_finish.  Both searches share the metric buffer: the
// launches are ordered on the stream.

int rc_eval_shift_invariant(rc_handle* h, const rc_eval_si_images* im, double* out, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_eval_shift_invariant";
  if (!im || !out) return fail(h, RC_ERR_INVALID_ARG, who + ": null images/out");
  if (!im->pred || !im->gt) return fail(h, RC_ERR_INVALID_ARG, who + ": pred and gt are required");
  if (im->height < 11 || im->width < 11)
    return fail(h, RC_ERR_INVALID_ARG, who + ": the 11 x 11 SSIM window does not fit into a " + std::to_string(im->height) +
                                           " x " + std::to_string(im->width) + " image");
  if (im->radius_i < 0 || im->radius_j < 0) return fail(h, RC_ERR_INVALID_ARG, who + ": negative search radius");
  if (im->window_halfwidth < 0) return fail(h, RC_ERR_INVALID_ARG, who + ": negative window_halfwidth");
  if (im->radius_i >= im->height || im->radius_j >= im->width)
    return fail(h, RC_ERR_INVALID_ARG, who + ": a search radius reaches the image size (one reflection must do)");
  if (im->radius_i > RC_EVAL_SI_MAX_RADIUS || im->radius_j > RC_EVAL_SI_MAX_RADIUS)
    return fail(h, RC_ERR_UNSUPPORTED, who + ": search radius above " + std::to_string(RC_EVAL_SI_MAX_RADIUS));
  if (im->window_halfwidth > RC_EVAL_SI_MAX_HALFWIDTH)
    return fail(h, RC_ERR_UNSUPPORTED, who + ": window_halfwidth above " + std::to_string(RC_EVAL_SI_MAX_HALFWIDTH));
  RoctxScope roctx_call("rc_eval_shift_invariant");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  int rc;
  WsUse use(h, WS_EVAL, st);
  if ((rc = use.rc)) return rc;
  EvalWs& y = ws_extra<EvalWs>(use.s);
  const int64_t n_pix = (int64_t)im->height * im->width;
  const int nj = 2 * im->radius_j + 1;
  int ty, tx;
  rc_si_tiles(im->height, im->width, &ty, &tx);
  const int64_t n_part = (int64_t)ty * tx;
  // si_state: best pooled, best metric (float32) and the two picks (int32), [H][W] each; si_part: doubles, both searches
  if ((rc = ws_alloc(h, {{y.si_metric, nj * n_pix}, {y.si_state, 4 * n_pix}, {y.si_part, 2 * 2 * n_part}})))
    return rc;
  double* part = reinterpret_cast<double*>(y.si_part.p);

  RcSiMetricArgs m{};
  m.pred = im->pred; m.gt = im->gt; m.height = im->height; m.width = im->width; m.radius_j = im->radius_j;
  {
    // dm_pix.ssim's window, as rc_eval_image builds it: computed in double and rounded once
    double w[11], sum = 0.0;
    for (int i = 0; i < 11; ++i) { const double f = (i - 5) / 1.5; w[i] = std::exp(-0.5 * (f * f)); sum += w[i]; }
    for (int i = 0; i < 11; ++i) m.taps[i] = (float)(w[i] / sum);
  }
  m.c1 = (float)((0.01 * 1.0) * (0.01 * 1.0)); m.c2 = (float)((0.03 * 1.0) * (0.03 * 1.0));
  m.metric = y.si_metric.p;
  RcSiSelectArgs s{};
  s.metric = y.si_metric.p; s.height = im->height; s.width = im->width; s.radius_j = im->radius_j;
  s.halfwidth = im->window_halfwidth;
  s.best_pooled = y.si_state.p; s.best_metric = y.si_state.p + n_pix;
  s.best_di = reinterpret_cast<int32_t*>(y.si_state.p + 2 * n_pix); s.best_dj = reinterpret_cast<int32_t*>(y.si_state.p + 3 * n_pix);

  for (int kind = RC_SI_MSE; kind <= (im->want_ssim ? RC_SI_SSIM : RC_SI_MSE); ++kind) {
    roctx_stage(kind == RC_SI_MSE ? "eval si: mse search" : "eval si: ssim search");
    const bool ssim = kind == RC_SI_SSIM;
    s.crop = ssim ? 5 : 0;
    s.out_map = ssim ? im->ssim_map : im->mse_map;
    s.out_di = ssim ? im->ssim_di : im->mse_di;
    s.out_dj = ssim ? im->ssim_dj : im->mse_dj;
    s.part = part + (ssim ? n_part : 0);
    for (int di = -im->radius_i; di <= im->radius_i; ++di) {
      m.di = di;
      rc_launch_si_metric(kind, m, st);
      s.di = di; s.first = di == -im->radius_i; s.last = di == im->radius_i;
      rc_launch_si_select(kind, s, st);
    }
  }
  RcSiFinishArgs f{};
  f.part_mse = part; f.part_ssim = im->want_ssim ? part + n_part : nullptr; f.n_part = n_part;
  f.n_mse = (double)n_pix; f.n_ssim = (double)(im->height - 10) * (double)(im->width - 10);
  f.out = out;
  rc_launch_si_finish(f, st);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}
