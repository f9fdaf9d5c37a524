// Host side of rc_backward_mask_rays and rc_mask_backward (rc_mask.hip); included by rc_api.hip after rc_train_host.inc
// and rc_interlevel_host.inc.
//
// One rc_mask_backward call = the training forward (enqueue_all's sampler levels on the workspace set WS_MASK, the
// caller's jitter and anneal; rc_interlevel_backward's step 1: nothing behind the last level's density) ->
// k_mask_loss_bwd (the last level's weights, the per-ray terms, d loss / d density) -> k_interlevel_reduce (the loss,
// fixed order) -> with a gradient buffer: rc_density_backward of the last level at the forward's own means
// (density_backward_chunks).  rc_transient_mask_backward is the same body on a time-resolved handle, the gradient at the last
// level's offset of the one sampler buffer (DESIGN.md §4.15b).

int rc_backward_mask_rays(rc_handle* h, const float* origins, const float* look, const float* u1, const float* u2, int64_t n,
                          float shadow_near_max, float normal_eps, float far, float* out_origins, float* out_directions,
                          float* out_near, float* out_far, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (n < 0) return fail(h, RC_ERR_INVALID_ARG, "rc_backward_mask_rays: negative n");
  if (!origins || !look || !u1 || !u2 || !out_origins || !out_directions || !out_near || !out_far)
    return fail(h, RC_ERR_INVALID_ARG, "rc_backward_mask_rays: null buffer");
  if (!std::isfinite(shadow_near_max) || !std::isfinite(normal_eps) || !std::isfinite(far))
    return fail(h, RC_ERR_INVALID_ARG, "rc_backward_mask_rays: shadow_near_max, normal_eps and far must be finite");
  if (n == 0) return RC_OK;
  RC_HIP(h, hipSetDevice(h->device));
  RcBackwardMaskRaysArgs a{};
  a.n = n; a.origins = origins; a.look = look; a.u1 = u1; a.u2 = u2;
  a.shadow_near_max = shadow_near_max; a.normal_eps = normal_eps; a.far = far;
  a.o_origins = out_origins; a.o_directions = out_directions; a.o_near = out_near; a.o_far = out_far;
  rc_launch_backward_mask_rays(a, (hipStream_t)stream_v);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

namespace {

// The body of rc_mask_backward and rc_transient_mask_backward.  density_grads: the last level's density layout (null:
// the loss only); allow_transient: a time-resolved handle runs (its own sampler's forward).
int mask_backward_impl(rc_handle* h, const std::string& who, bool allow_transient, const rc_rays* rays, const float* masks,
                       const float* lossmult, int64_t n, const rc_randoms* rnd, float anneal, const rc_mask_loss* cfg,
                       float* density_grads, float* loss, void* stream_v) {
  const rc_config& c = h->cfg;
  const int NL = c.num_levels;
  if (n < 0) return fail(h, RC_ERR_INVALID_ARG, who + ": negative n_rays");
  if (!rays || !cfg || !loss) return fail(h, RC_ERR_INVALID_ARG, who + ": null rays/cfg/loss");
  if (!(anneal >= 0.0f) || !std::isfinite(anneal)) return fail(h, RC_ERR_INVALID_ARG, who + ": anneal must be finite and >= 0");
  if (!std::isfinite(cfg->weight_opaque) || !std::isfinite(cfg->weight_empty))
    return fail(h, RC_ERR_INVALID_ARG, who + ": the weights must be finite");
  // d sqrt(x^2 + pad^2) / d x at pad = 0 and x = 0 is NaN in JAX: not restated
  if (!(cfg->charb_padding > 0.0f) || !std::isfinite(cfg->charb_padding))
    return fail(h, RC_ERR_UNSUPPORTED, who + ": charb_padding must be finite and > 0");
  if (h->transient && !allow_transient) return fail(h, RC_ERR_UNSUPPORTED, who + ": not available on a time-resolved cache handle");
  if (n == 0) return RC_OK;
  int rc;
  if ((rc = check_rays(h, rays, who.c_str()))) return rc;
  const int S2 = c.num_samples[NL - 1];
  if (S2 < 1 || S2 > 32) return fail(h, RC_ERR_UNSUPPORTED, who + ": needs <= 32 samples on the last level");
  RoctxScope roctx_call(who.c_str());
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  if ((rc = ensure_packed(h))) return rc;
  WsUse use(h, WS_MASK, st);
  if ((rc = use.rc)) return rc;
  RenderWs& w = use.s.r;
  MaskWs& x = ws_extra<MaskWs>(use.s);
  const int64_t np = n * S2;
  for (int l = 0; l < NL; ++l)
    if ((rc = ws_sampler_level(h, w, l, n))) return rc;
  if ((rc = ws_alloc(h, {{x.loss_ray, n}, {x.d_density, np}}))) return rc;

  // 1. the training forward: the sampler levels only (weights_only=True, models.py:476-486), stopped behind the last
  //    level's density
  RenderArgs A = cache_pass(rays, rnd, n);
  A.stop = RENDER_SAMPLER; A.anneal = anneal;
  enqueue_all(h, A, w, st);

  // 2. the loss and d loss / d density of the last level
  RcMaskLossArgs ma{};
  ma.n = n; ma.S = S2;
  ma.density = w.density[NL - 1].p; ma.tdist = w.tdist[NL - 1].p; ma.directions = rays->directions;
  ma.weights = w.weights[NL - 1].p;
  ma.masks = cfg->zero_masks ? nullptr : masks; ma.lossmult = lossmult;
  ma.padding = cfg->charb_padding; ma.weight_opaque = cfg->weight_opaque; ma.weight_empty = cfg->weight_empty;
  ma.zero_masks = cfg->zero_masks ? 1 : 0;
  ma.inv_n = (float)(1.0 / (double)n);                         // jnp.mean over the rays
  ma.loss_ray = x.loss_ray.p; ma.d_density = x.d_density.p;
  rc_launch_mask_loss_bwd(ma, st);
  RcInterlevelReduce rr{};
  rr.mult[0] = 1.0f; rr.count[0] = (double)n;
  rc_launch_interlevel_reduce(x.loss_ray.p, n, 1, rr, loss, st);
  RC_HIP(h, hipGetLastError());
  if (!density_grads) return RC_OK;

  // 3. the density backward of the last level at the forward's sample means
  return density_backward_chunks(h, NL - 1, w.means[NL - 1].p, np, x.points, x.d_density.p, nullptr, density_grads, st);
}

}  // namespace

int rc_mask_backward(rc_handle* h, const rc_rays* rays, const float* masks, const float* lossmult, int64_t n,
                     const rc_randoms* rnd, float anneal, const rc_mask_loss* cfg, float* density_grads, float* loss,
                     void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  return mask_backward_impl(h, "rc_mask_backward", false, rays, masks, lossmult, n, rnd, anneal, cfg, density_grads, loss, stream_v);
  RC_CATCH(h)
}

int rc_transient_mask_backward(rc_handle* h, const rc_rays* rays, const float* masks, const float* lossmult, int64_t n,
                               const rc_randoms* rnd, float anneal, const rc_mask_loss* cfg, float* sampler_grads, float* loss,
                               void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_transient_mask_backward";
  if (int rc = transient_sampler_handle(h, who)) return rc;
  int64_t off[RC_MAX_LEVELS] = {};
  (void)transient_sampler_segments(h, off);
  return mask_backward_impl(h, who, true, rays, masks, lossmult, n, rnd, anneal, cfg,
                            sampler_grads ? sampler_grads + off[h->cfg.num_levels - 1] : nullptr, loss, stream_v);
  RC_CATCH(h)
}
