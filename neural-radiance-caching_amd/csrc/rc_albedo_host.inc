// Host side of rc_eval_albedo and rc_albedo_ratio (rc_albedo.hip); included by rc_api.hip.
//
// rc_eval_albedo = count, scan, write (the valid rows: into the workspace's buffer when the view's own median is wanted,
// and appended to the caller's buffer when one is given) -> the median over the workspace's rows (no ratio handed in) ->
// score, finish.  rc_albedo_ratio = begin -> four radix passes, or the least squares.  Nothing here reads device memory:
// row counts stay on the device, and launches are sized by the capacities.

namespace {
constexpr int64_t kAlbedoMaxRows = (int64_t)1 << 31;       // rows are counted in 32-bit histograms
constexpr int64_t kAlbedoStateFloats = (sizeof(RcAlbedoState) + sizeof(float) - 1) / sizeof(float);
}  // namespace

int rc_eval_albedo(rc_handle* h, const rc_albedo_images* im, double* out, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_eval_albedo";
  if (!im || !out) return fail(h, RC_ERR_INVALID_ARG, who + ": null images/out");
  if (!im->albedo || !im->acc || !im->albedo_gt) return fail(h, RC_ERR_INVALID_ARG, who + ": albedo, acc and albedo_gt are required");
  if (im->height < 1 || im->width < 1) return fail(h, RC_ERR_INVALID_ARG, who + ": height and width must be at least 1");
  const int64_t n_pix = (int64_t)im->height * im->width;
  if (n_pix >= kAlbedoMaxRows) return fail(h, RC_ERR_INVALID_ARG, who + ": 2^31 pixels or more");
  if (!std::isfinite(im->albedo_clip)) return fail(h, RC_ERR_INVALID_ARG, who + ": albedo_clip must be finite");
  if (im->pairs && !im->pairs_count) return fail(h, RC_ERR_INVALID_ARG, who + ": pairs need pairs_count");
  if (im->pairs && (im->pairs_capacity < 0 || im->pairs_capacity >= kAlbedoMaxRows))
    return fail(h, RC_ERR_INVALID_ARG, who + ": pairs_capacity must be in [0, 2^31)");
  RoctxScope roctx_call("rc_eval_albedo");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  int rc;
  WsUse use(h, WS_ALBEDO, st);
  if ((rc = use.rc)) return rc;
  AlbedoWs& y = ws_extra<AlbedoWs>(use.s);
  const bool own = im->ratio == nullptr;                   // the view's own median: its rows go to the workspace
  const int64_t blocks = rc_albedo_pixel_blocks(n_pix);
  // requests of 0 floats keep what an earlier call allocated (ws_alloc only grows)
  if ((rc = ws_alloc(h, {{y.pairs, own ? 6 * n_pix : 0}, {y.wg, blocks}, {y.state, kAlbedoStateFloats}, {y.part, 2 * blocks}})))
    return rc;
  RcAlbedoState* state = reinterpret_cast<RcAlbedoState*>(y.state.p);

  roctx_stage("albedo: compact");
  RcAlbedoPixelArgs p{};
  p.albedo = im->albedo; p.acc = im->acc; p.albedo_gt = im->albedo_gt; p.mask = im->mask; p.n_pix = n_pix;
  p.wg = reinterpret_cast<int32_t*>(y.wg.p); p.state = state;
  p.own = own ? y.pairs.p : nullptr;
  p.pairs = im->pairs; p.capacity = im->pairs ? im->pairs_capacity : 0; p.count = im->pairs ? im->pairs_count : nullptr;
  p.ratio = own ? state->ratio : im->ratio; p.albedo_clip = im->albedo_clip;
  p.post_pred = im->post_pred; p.post_gt = im->post_gt; p.ratio_im = im->ratio_im;
  p.part = reinterpret_cast<double*>(y.part.p); p.out = out;
  rc_launch_albedo_compact(p, st);
  if (own) {
    roctx_stage("albedo: median");
    RcAlbedoRatioArgs r{};
    r.pairs = y.pairs.p; r.capacity = n_pix; r.count = nullptr; r.state = state;
    rc_launch_albedo_median(r, st);
  }
  roctx_stage("albedo: score");
  rc_launch_albedo_score(p, st);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

int rc_albedo_ratio(rc_handle* h, const float* pairs, int64_t pairs_capacity, const int64_t* pairs_count, int32_t use_median,
                    int32_t gamma, float* ratio, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_albedo_ratio";
  if (!pairs || !pairs_count || !ratio) return fail(h, RC_ERR_INVALID_ARG, who + ": null pairs/pairs_count/ratio");
  if (pairs_capacity < 0 || pairs_capacity >= kAlbedoMaxRows)
    return fail(h, RC_ERR_INVALID_ARG, who + ": pairs_capacity must be in [0, 2^31)");
  RoctxScope roctx_call("rc_albedo_ratio");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  int rc;
  WsUse use(h, WS_ALBEDO, st);
  if ((rc = use.rc)) return rc;
  AlbedoWs& y = ws_extra<AlbedoWs>(use.s);
  const int64_t blocks = rc_albedo_row_blocks(pairs_capacity);
  if ((rc = ws_alloc(h, {{y.state, kAlbedoStateFloats}, {y.part, use_median ? 0 : 2 * 6 * blocks}}))) return rc;
  RcAlbedoRatioArgs r{};
  r.pairs = pairs; r.capacity = pairs_capacity; r.count = pairs_count; r.state = reinterpret_cast<RcAlbedoState*>(y.state.p);
  r.gamma = gamma != 0; r.part = reinterpret_cast<double*>(y.part.p); r.ratio = ratio;
  if (use_median) rc_launch_albedo_median(r, st);
  else rc_launch_albedo_lstsq(r, st);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}
