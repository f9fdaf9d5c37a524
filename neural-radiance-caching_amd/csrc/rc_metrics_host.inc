// Host side of rc_eval_image (rc_metrics.hip); included by rc_api.hip.
//
// One call = k_eval_bins (n_bins > 0 only: the bin sums of both histograms and the IoU's partial sums) -> k_eval_pixels
// (post-process, squared error, depth and normal errors) -> k_eval_ssim on the two post-processed images ->
// k_eval_finish (every partial sum in a fixed order, the result array on the device).

int rc_eval_image(rc_handle* h, const rc_eval_images* im, double* out, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_eval_image";
  if (!im || !out) return fail(h, RC_ERR_INVALID_ARG, who + ": null images/out");
  if (!im->pred || !im->gt) return fail(h, RC_ERR_INVALID_ARG, who + ": pred and gt are required");
  if (im->n_bins < 0) return fail(h, RC_ERR_INVALID_ARG, who + ": negative n_bins");
  if (im->height < 11 || im->width < 11)
    return fail(h, RC_ERR_INVALID_ARG, who + ": the 11 x 11 SSIM window does not fit into a " + std::to_string(im->height) +
                                           " x " + std::to_string(im->width) + " image");
  if (im->clip_eval && im->n_bins > 0)
    return fail(h, RC_ERR_UNSUPPORTED, who + ": clip_eval with bins (the reference's clip_eval post-process does not sum bins)");
  if (im->skip_postprocess && im->n_bins > 0)
    return fail(h, RC_ERR_INVALID_ARG, who + ": skip_postprocess with bins");
  if (im->normals && (!im->normals_gt || !im->acc))
    return fail(h, RC_ERR_INVALID_ARG, who + ": normals need normals_gt and acc");
  if (!std::isfinite(im->exposure) || (im->n_bins > 0 && !(std::isfinite(im->img_scale) && im->img_scale > 0.0f)))
    return fail(h, RC_ERR_INVALID_ARG, who + ": exposure must be finite, img_scale finite and positive");
  RoctxScope roctx_call("rc_eval_image");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  int rc;
  WsUse use(h, WS_EVAL, st);
  if ((rc = use.rc)) return rc;
  EvalWs& y = ws_extra<EvalWs>(use.s);
  const int64_t n_pix = (int64_t)im->height * im->width;
  const bool bins = im->n_bins > 0;
  int ty, tx;
  rc_eval_ssim_tiles(im->height, im->width, &ty, &tx);
  const int64_t nb_bins = bins ? rc_eval_bins_blocks(n_pix) : 0, nb_pix = rc_eval_pixel_blocks(n_pix), nb_ssim = 3 * (int64_t)ty * tx;
  const int64_t part_doubles = 2 * nb_bins + rc_eval_pixel_parts() * nb_pix + nb_ssim;
  // requests of 0 floats keep what an earlier call allocated (ws_alloc only grows)
  if ((rc = ws_alloc(h, {{y.binsum_pred, bins ? 3 * n_pix : 0}, {y.binsum_gt, bins ? 3 * n_pix : 0},
                         {y.post_pred, im->post_pred ? 0 : 3 * n_pix}, {y.post_gt, im->post_gt ? 0 : 3 * n_pix},
                         {y.part, 2 * part_doubles}})))
    return rc;
  double* part_bins = reinterpret_cast<double*>(y.part.p);
  double* part_pix = part_bins + 2 * nb_bins;
  double* part_ssim = part_pix + rc_eval_pixel_parts() * nb_pix;
  float* post_pred = im->post_pred ? im->post_pred : y.post_pred.p;
  float* post_gt = im->post_gt ? im->post_gt : y.post_gt.p;

  if (bins) {
    roctx_stage("eval: bin sums and IoU");
    RcEvalBinsArgs b{};
    b.pred = im->pred; b.gt = im->gt; b.n_pix = n_pix; b.n_bins = im->n_bins;
    b.vec_ok = (((uintptr_t)im->pred ^ (uintptr_t)im->gt) & 15u) == 0;
    b.binsum_pred = y.binsum_pred.p; b.binsum_gt = y.binsum_gt.p; b.part = part_bins;
    rc_launch_eval_bins(b, st);
  }
  roctx_stage("eval: pixels");
  RcEvalPixelArgs p{};
  p.pred = bins ? y.binsum_pred.p : im->pred; p.gt = bins ? y.binsum_gt.p : im->gt;
  p.mask = im->mask; p.acc = im->acc; p.normals = im->normals; p.normals_gt = im->normals_gt;
  p.distance_mean = im->distance_mean; p.distance_median = im->distance_median; p.depth_gt = im->depth_gt;
  p.n_pix = n_pix; p.bins = bins; p.clip_eval = im->clip_eval != 0; p.skip = im->skip_postprocess != 0; p.exposure = im->exposure; p.img_scale = im->img_scale;
  p.post_pred = post_pred; p.post_gt = post_gt; p.part = part_pix;
  rc_launch_eval_pixels(p, st);

  roctx_stage("eval: ssim");
  RcEvalSsimArgs s{};
  s.a = post_pred; s.b = post_gt; s.height = im->height; s.width = im->width;
  {
    // dm_pix.ssim's window: exp(-0.5 ((i - 5) / 1.5)^2), normalised; computed in double and rounded once
    double w[11], sum = 0.0;
    for (int i = 0; i < 11; ++i) { const double f = (i - 5) / 1.5; w[i] = std::exp(-0.5 * (f * f)); sum += w[i]; }
    for (int i = 0; i < 11; ++i) s.taps[i] = (float)(w[i] / sum);
  }
  s.c1 = (float)((0.01 * 1.0) * (0.01 * 1.0)); s.c2 = (float)((0.03 * 1.0) * (0.03 * 1.0));
  s.map = im->ssim_map; s.part = part_ssim;
  rc_launch_eval_ssim(s, st);

  RcEvalFinishArgs f{};
  f.part_pixels = part_pix; f.part_ssim = part_ssim; f.part_bins = part_bins;
  f.n_part_pixels = nb_pix; f.n_part_ssim = nb_ssim; f.n_part_bins = nb_bins;
  f.n_pix = n_pix; f.ssim_count = 3.0 * (double)(im->height - 10) * (double)(im->width - 10);
  f.masked = im->mask != nullptr;
  f.have_l1_mean = im->depth_gt && im->distance_mean; f.have_l1_median = im->depth_gt && im->distance_median;
  f.have_mae = im->normals != nullptr;
  f.out = out;
  rc_launch_eval_finish(f, st);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}
