// Host side of rc_geometry_backward and rc_density_regularizer (rc_geometry.hip); included by rc_api.hip.
//
// One rc_geometry_backward call = the training forward (enqueue_all's sampler levels with the last level's hidden vector,
// predicted and analytic normals, on the workspace set WS_GEOMETRY, the caller's jitter and anneal; no shader) ->
// k_geometry_loss_bwd (per-ray values of the four terms, d loss / d density, d loss / d pred_raw) -> k_interlevel_reduce
// (the four losses, fixed order) -> with a gradient buffer, per chunk of kDataChunk samples: h64 staged in the reference's
// column order, pred_normals_layer's weight gradient on k_gemm (K = the chunk's samples, fixed slices), d feature64 =
// d pred_raw W_n^T, and rc_density_backward of the last level.
// rc_transient_geometry_backward and rc_transient_density_regularizer are the same bodies on a time-resolved handle, their
// gradients at offsets of the one sampler buffer (RC_LAYOUT_TRANSIENT_SAMPLER, DESIGN.md §4.15b).
// (tests/gemm_ref.py lists the dense_* call sites of this file by line.)

namespace {

int upload_geometry_weights(rc_handle* h) {
  std::string missing;
  const std::string path = data_layer_path(h, DL_PRED);
  const HostLayer* L = need(h, path, missing);
  if (!L) return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: " + missing);
  if (L->in != 64 || L->out != 3) return fail(h, RC_ERR_UNSUPPORTED, "rc_geometry_backward: unexpected shape of " + path);
  std::vector<float> v(L->kernel.begin(), L->kernel.end());
  v.insert(v.end(), L->bias.begin(), L->bias.end());
  return upload(h, h->geom_w, v);
}

// The body of rc_geometry_backward and rc_transient_geometry_backward.  density_grads: the last level's density layout
// (null: none); pn_grads + pn_seg[0 / 1].offset: where pred_normals_layer's kernel / bias gradient goes (pn_grads null:
// none); allow_transient: a time-resolved handle runs (its own sampler's forward).
int geometry_backward_impl(rc_handle* h, const std::string& who, bool allow_transient, const rc_rays* rays, const float* lossmult,
                           int64_t n, const rc_randoms* rnd, float anneal, const rc_geometry_loss* cfg, float* density_grads,
                           float* pn_grads, const GradSeg* pn_seg, float* losses, void* stream_v) {
  const rc_config& c = h->cfg;
  const int NL = c.num_levels;
  if (n < 0) return fail(h, RC_ERR_INVALID_ARG, who + ": negative n_rays");
  if (!rays || !cfg) return fail(h, RC_ERR_INVALID_ARG, who + ": null rays/cfg");
  if (!(anneal >= 0.0f) || !std::isfinite(anneal)) return fail(h, RC_ERR_INVALID_ARG, who + ": anneal must be finite and >= 0");
  const float f[] = {cfg->distortion_mult, cfg->distortion_p, cfg->distortion_premult, cfg->orientation_mult,
                     cfg->pred_normal_mult, cfg->pred_normal_w_grad_weight, cfg->pred_normal_reverse_mult};
  for (float v : f)
    if (!std::isfinite(v)) return fail(h, RC_ERR_INVALID_ARG, who + ": the loss settings must be finite");
  if (cfg->distortion_p == 0.0f || cfg->distortion_p == 1.0f)
    return fail(h, RC_ERR_UNSUPPORTED, who + ": distortion_p must not be 0 or 1");
  if (h->transient && !allow_transient) return fail(h, RC_ERR_UNSUPPORTED, who + ": not available on a time-resolved cache handle");
  if (n == 0) return RC_OK;
  if (!losses) return fail(h, RC_ERR_INVALID_ARG, who + ": null losses");
  int rc;
  if ((rc = check_rays(h, rays, who.c_str()))) return rc;
  const int S2 = c.num_samples[NL - 1];
  if (S2 < 1 || S2 > 32) return fail(h, RC_ERR_UNSUPPORTED, who + ": needs <= 32 samples on the last level");
  RoctxScope roctx_call(who.c_str());
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  if ((rc = ensure_packed(h))) return rc;
  const bool grads = density_grads || pn_grads;
  if (grads && h->geom_gen != h->layers_gen) {
    if ((rc = upload_geometry_weights(h))) return rc;
    h->geom_gen = h->layers_gen;
  }
  WsUse use(h, WS_GEOMETRY, st);
  if ((rc = use.rc)) return rc;
  RenderWs& w = use.s.r;
  GeometryWs& x = ws_extra<GeometryWs>(use.s);
  const int64_t np = n * S2;
  if ((rc = ensure_workspace(h, w, n)) || (rc = ws_alloc(h, x.loss_ray, 4 * n))) return rc;
  if (grads && (rc = ws_alloc(h, {{x.d_density, np}, {x.d_pred, 3 * np}}))) return rc;

  // 1. the training forward: the sampler levels, the last with hbuf, normals_pred and the analytic normals
  RenderArgs A = cache_pass(rays, rnd, n);
  A.anneal = anneal; A.stop = RENDER_LEVELS; A.force_grad = true;
  enqueue_all(h, A, w, st);

  // 2. the four terms, d loss / d density and d loss / d pred_raw
  RcGeometryLossArgs ga{};
  ga.n = n; ga.S = S2;
  ga.weights = w.weights[NL - 1].p; ga.density = w.density[NL - 1].p; ga.tdist = w.tdist[NL - 1].p;
  ga.directions = rays->directions; ga.viewdirs = rays->viewdirs; ga.lossmult = lossmult;
  ga.normals_pred = w.normals_pred.p; ga.normals_grad = w.normals_grad.p; ga.hbuf = w.hbuf.p; ga.wn = h->geom_w.p;
  ga.dist_p = cfg->distortion_p; ga.dist_premult = cfg->distortion_premult;
  ga.dist_coef = (float)((double)cfg->distortion_mult / (double)n);       // jnp.mean over the rays, times the mult
  ga.orient_coef = (float)((double)cfg->orientation_mult / (double)n);
  ga.pn_coef = (float)((double)cfg->pred_normal_mult / (double)n);
  ga.pnr_coef = (float)((double)cfg->pred_normal_reverse_mult / (double)n);
  ga.pn_wgrad = cfg->pred_normal_w_grad_weight;
  ga.loss_ray = x.loss_ray.p;
  ga.d_density = grads ? x.d_density.p : nullptr; ga.d_pred = grads ? x.d_pred.p : nullptr;
  rc_launch_geometry_loss_bwd(ga, st);
  // k_interlevel_reduce adds up to RC_MAX_LEVELS terms per launch: terms 0-2, then term 3
  static_assert(RC_MAX_LEVELS == 3, "the four losses are reduced in two launches");
  const float mults[4] = {cfg->distortion_mult, cfg->orientation_mult, cfg->pred_normal_mult, cfg->pred_normal_reverse_mult};
  RcInterlevelReduce r0{}, r1{};
  for (int k = 0; k < 3; ++k) { r0.mult[k] = mults[k]; r0.count[k] = (double)n; }
  r1.mult[0] = mults[3]; r1.count[0] = (double)n;
  rc_launch_interlevel_reduce(x.loss_ray.p, n, 3, r0, losses, st);
  rc_launch_interlevel_reduce(x.loss_ray.p + 3 * n, n, 1, r1, losses + 3, st);
  RC_HIP(h, hipGetLastError());
  if (!grads) return RC_OK;

  // 3. per chunk: pred_normals_layer's gradient, d feature64, the density backward of the last level
  const int64_t CH = np < kDataChunk ? np : kDataChunk;
  const int64_t nslices = (CH + kDataKSlice - 1) / kDataKSlice;
  if ((rc = ws_alloc(h, {{x.points, 3 * np}, {x.h64, CH * 64}, {x.dfeat, CH * 64}, {x.part, nslices * 64 * 3}, {x.ones, 1}})))
    return rc;
  RC_HIP(h, hipMemsetD32Async((hipDeviceptr_t)x.ones.p, 0x3f800000, 1, st));     // 1.0f: the A operand of a bias gradient
  rc_launch_points_aos(w.means[NL - 1].p, np, x.points.p, st);
  const Dense Wn{64, 3, h->geom_w.p, nullptr};
  for (int64_t c0 = 0; c0 < np; c0 += CH) {
    const int64_t C = np - c0 < CH ? np - c0 : CH;
    const float* dp = x.d_pred.p + 3 * c0;
    rc_launch_stage_hidden(w.hbuf.p, c0, C, x.h64.p, st);
    if (pn_grads) dense_wgrad(Wn, C, x.h64.p, 64, dp, 3, x.ones.p, x.part.p, pn_grads, pn_seg, st);
    if (density_grads) {
      dense_dx(Wn, C, dp, 3, x.dfeat.p, 64, 0, 64, nullptr, false, st);     // d feature64 = d pred_raw W_n^T
      RC_HIP(h, hipGetLastError());
      if ((rc = rc_density_backward(h, NL - 1, x.points.p + 3 * c0, C, x.d_density.p + c0, x.dfeat.p, density_grads, nullptr, stream_v)))
        return rc;
    }
  }
  RC_HIP(h, hipGetLastError());
  return RC_OK;
}

}  // namespace

int rc_geometry_backward(rc_handle* h, const rc_rays* rays, const float* lossmult, int64_t n, const rc_randoms* rnd,
                         float anneal, const rc_geometry_loss* cfg, float* density_grads, float* shader_grads, float* losses,
                         void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  int kseg[DL_COUNT];
  std::vector<GradSeg> segs;
  if (shader_grads && !h->transient) segs = shader_grad_segments(h, kseg);
  return geometry_backward_impl(h, "rc_geometry_backward", false, rays, lossmult, n, rnd, anneal, cfg, density_grads, shader_grads,
                                segs.empty() ? nullptr : &segs[kseg[DL_PRED]], losses, stream_v);
  RC_CATCH(h)
}

int rc_transient_geometry_backward(rc_handle* h, const rc_rays* rays, const float* lossmult, int64_t n, const rc_randoms* rnd,
                                   float anneal, const rc_geometry_loss* cfg, float* sampler_grads, float* losses, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_transient_geometry_backward";
  if (int rc = transient_sampler_handle(h, who)) return rc;
  int64_t off[RC_MAX_LEVELS] = {};
  int pred = 0;
  const std::vector<GradSeg> segs = transient_sampler_segments(h, off, &pred);
  return geometry_backward_impl(h, who, true, rays, lossmult, n, rnd, anneal, cfg,
                                sampler_grads ? sampler_grads + off[h->cfg.num_levels - 1] : nullptr, sampler_grads, &segs[pred], losses,
                                stream_v);
  RC_CATCH(h)
}

int rc_density_regularizer(rc_handle* h, int32_t level, float mult, float* density_grads, float* loss, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (level < 0 || level >= h->cfg.num_levels) return fail(h, RC_ERR_INVALID_ARG, "rc_density_regularizer: bad level");
  return grid_l2_regularizer<GeometryWs>(h, level, WS_GEOMETRY, mult, density_grads, loss, stream_v, "rc_density_regularizer");
  RC_CATCH(h)
}

int rc_transient_density_regularizer(rc_handle* h, int32_t level, float mult, float* sampler_grads, float* loss, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_transient_density_regularizer";
  if (int rc = transient_sampler_handle(h, who)) return rc;
  if (level < 0 || level >= h->cfg.num_levels) return fail(h, RC_ERR_INVALID_ARG, who + ": bad level");
  int64_t off[RC_MAX_LEVELS] = {};
  (void)transient_sampler_segments(h, off);
  return grid_l2_regularizer<GeometryWs>(h, level, WS_GEOMETRY, mult, sampler_grads ? sampler_grads + off[level] : nullptr, loss,
                                         stream_v, who, true);
  RC_CATCH(h)
}
