// Host side of rc_interlevel_backward (rc_interlevel.hip); included by rc_api.hip after rc_train_host.inc.
//
// One call = the training forward (enqueue_all's sampler levels on the workspace set WS_INTERLEVEL, the caller's jitter
// and anneal) -> k_interlevel_bwd (losses' per-ray sums, d loss / d density of every proposal level) ->
// k_interlevel_reduce (the losses, fixed order) -> per proposal level with a gradient buffer: the means copied from the
// workspace's SoA [3][n S] into the AoS [n S][3] rc_density_backward takes (an exact copy: the backward evaluates the
// forward's points; 24 bytes per sample moved, against the ~2 KB per sample the density backward itself moves), then
// rc_density_backward of that level.  rc_transient_interlevel_backward is the same body on a time-resolved handle (its own
// sampler's forward), the levels' gradients at their offsets of the one sampler buffer (DESIGN.md §4.15b).

namespace {

// The body of rc_interlevel_backward and rc_transient_interlevel_backward.  grads: per proposal level where its density
// gradient goes (null, or a null entry: none); allow_transient: a time-resolved handle runs (its own sampler's forward).
int interlevel_backward_impl(rc_handle* h, const std::string& who, bool allow_transient, const rc_rays* rays, const float* lossmult,
                             int64_t n, const rc_randoms* rnd, float anneal, const float* mults, const float* blurs,
                             float* const* grads, float* losses, void* stream_v) {
  const rc_config& c = h->cfg;
  const int NL = c.num_levels;
  if (n < 0) return fail(h, RC_ERR_INVALID_ARG, who + ": negative n_rays");
  if (!rays || !mults || !blurs) return fail(h, RC_ERR_INVALID_ARG, who + ": null rays/mults/blurs");
  if (!(anneal >= 0.0f) || !std::isfinite(anneal)) return fail(h, RC_ERR_INVALID_ARG, who + ": anneal must be finite and >= 0");
  for (int l = 0; l < NL - 1; ++l) {
    if (!std::isfinite(mults[l])) return fail(h, RC_ERR_INVALID_ARG, who + ": mults must be finite");
    if (!(blurs[l] >= 0.0f) || !std::isfinite(blurs[l])) return fail(h, RC_ERR_INVALID_ARG, who + ": blurs must be finite and >= 0");
  }
  if (n == 0) return RC_OK;
  if (!losses) return fail(h, RC_ERR_INVALID_ARG, who + ": null losses");
  int rc;
  if ((rc = check_rays(h, rays, who.c_str()))) return rc;
  if (h->transient && !allow_transient) return fail(h, RC_ERR_UNSUPPORTED, who + ": not available on a time-resolved cache handle");
  if (!rc_interlevel_supported(NL, c.num_samples))
    return fail(h, RC_ERR_UNSUPPORTED, who + ": needs >= 2 levels, <= 64 samples per proposal level, <= 32 on the last");
  RoctxScope roctx_call(who.c_str());
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  if ((rc = ensure_packed(h))) return rc;
  WsUse use(h, WS_INTERLEVEL, st);
  if ((rc = use.rc)) return rc;
  RenderWs& w = use.s.r;
  InterlevelWs& x = ws_extra<InterlevelWs>(use.s);
  for (int l = 0; l < NL; ++l) {
    const int64_t S = c.num_samples[l];
    if ((rc = ws_sampler_level(h, w, l, n))) return rc;
    if (l < NL - 1) {
      if ((rc = ws_alloc(h, x.d_density[l], n * S))) return rc;
      if (grads && grads[l] && (rc = ws_alloc(h, x.points[l], 3 * n * S))) return rc;
    }
  }
  if ((rc = ws_alloc(h, x.loss_ray, (int64_t)(NL - 1) * n))) return rc;

  // 1. the training forward: rc_render_rays' own sampler loop, stopped behind the last level's density
  RenderArgs A = cache_pass(rays, rnd, n);
  A.stop = RENDER_SAMPLER; A.anneal = anneal;
  enqueue_all(h, A, w, st);

  // 2. the loss and d loss / d density of every proposal level
  RcInterlevelArgs ia{};
  ia.n = n; ia.num_levels = NL; ia.directions = rays->directions; ia.lossmult = lossmult; ia.loss_ray = x.loss_ray.p;
  RcInterlevelReduce rr{};
  for (int l = 0; l < NL; ++l) {
    ia.S[l] = c.num_samples[l];
    ia.sdist[l] = w.sdist[l].p; ia.tdist[l] = w.tdist[l].p; ia.density[l] = w.density[l].p;
    if (l < NL - 1) {
      const double count = (double)n * c.num_samples[l];
      ia.blur[l] = blurs[l];
      ia.coef[l] = (float)((double)mults[l] / count);      // jnp.mean: 1 / (n S) per sample, times the mult
      ia.d_density[l] = x.d_density[l].p;
      rr.mult[l] = mults[l]; rr.count[l] = count;
    }
  }
  rc_launch_interlevel_bwd(ia, st);
  rc_launch_interlevel_reduce(x.loss_ray.p, n, NL - 1, rr, losses, st);
  RC_HIP(h, hipGetLastError());

  // 3. the density backward of each proposal level at the forward's sample means
  for (int l = 0; l < NL - 1; ++l) {
    if (!grads || !grads[l]) continue;
    const int64_t np = n * c.num_samples[l];
    rc_launch_points_aos(w.means[l].p, np, x.points[l].p, st);
    if ((rc = rc_density_backward(h, l, x.points[l].p, np, x.d_density[l].p, nullptr, grads[l], nullptr, stream_v))) return rc;
  }
  RC_HIP(h, hipGetLastError());
  return RC_OK;
}

// rc_transient_*: the handle's kind, checked in front of the shared body's own checks of the handle's state
int transient_sampler_handle(rc_handle* h, const std::string& who) {
  if (!h->transient) return fail(h, RC_ERR_UNSUPPORTED, who + ": needs a time-resolved cache handle (rc_set_transient)");
  if (h->tcfg.use_occlusions) return fail(h, RC_ERR_UNSUPPORTED, who + ": the occlusion variant is not offered (a vis_only feature)");
  return RC_OK;
}

}  // namespace

int rc_interlevel_backward(rc_handle* h, const rc_rays* rays, const float* lossmult, int64_t n, const rc_randoms* rnd,
                           float anneal, const float* mults, const float* blurs, float* const* grads, float* losses,
                           void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  return interlevel_backward_impl(h, "rc_interlevel_backward", false, rays, lossmult, n, rnd, anneal, mults, blurs, grads, losses,
                                  stream_v);
  RC_CATCH(h)
}

int rc_transient_interlevel_backward(rc_handle* h, const rc_rays* rays, const float* lossmult, int64_t n, const rc_randoms* rnd,
                                     float anneal, const float* mults, const float* blurs, float* sampler_grads, float* losses,
                                     void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_transient_interlevel_backward";
  if (int rc = transient_sampler_handle(h, who)) return rc;
  int64_t off[RC_MAX_LEVELS] = {};
  (void)transient_sampler_segments(h, off);
  float* grads[RC_MAX_LEVELS] = {};
  for (int l = 0; l < h->cfg.num_levels - 1; ++l) grads[l] = sampler_grads ? sampler_grads + off[l] : nullptr;
  return interlevel_backward_impl(h, who, true, rays, lossmult, n, rnd, anneal, mults, blurs, grads, losses, stream_v);
  RC_CATCH(h)
}
