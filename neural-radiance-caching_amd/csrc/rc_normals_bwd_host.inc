// Host side of rc_normals_backward and rc_geometry_smoothness_backward (rc_normals_bwd.hip); included by rc_api.hip behind
// rc_train_host.inc (layouts, build_train_stream) and rc_geometry_host.inc.
//
// One rc_normals_backward call = the last level's lookup with its Jacobian -> k_normals_bwd -> k_wgrad + k_grad_reduce
// without the bias sums -> k_grid_scatter_jac, on the workspace set WS_NORMALS, everything on the caller's stream.
// One rc_geometry_smoothness_backward call = the training forward (enqueue_all's sampler levels with the analytic normals,
// on the workspace set WS_GSMOOTH) -> k_gsmooth_points -> the last level once more at the perturbed means (lookup with
// Jacobian, k_density_mlp<17, true>) -> k_gsmooth_loss -> k_interlevel_reduce (the loss, fixed order) -> with a gradient
// buffer, per chunk of kDataChunk samples: rc_normals_backward at x and at x', and rc_density_backward at both when the
// density term is on.

namespace {

// Stream of k_normals_bwd: k_density_bwd's, then the two forward layers once more (read with a zero in the bias slot).
int pack_normals_stream(rc_handle* h) {
  std::vector<float> stream;
  size_t replay = 0;
  if (int rc = build_train_stream(h, h->cfg.num_levels - 1, stream, &replay)) return rc;
  const std::vector<float> fwd(stream.begin(), stream.begin() + (ptrdiff_t)replay);
  append(stream, fwd);
  return upload(h, h->packs.nbwd, pad_stream(stream));
}

}  // namespace

int rc_normals_backward(rc_handle* h, const float* points, int64_t n, const float* d_normals, float* grads, float* normals_out,
                        void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (n < 0 || (n > 0 && (!points || !d_normals)) || !grads) return fail(h, RC_ERR_INVALID_ARG, "rc_normals_backward: null buffer or negative n");
  const int level = h->cfg.num_levels - 1;
  GridState& gs = h->grids[level];
  const int F = gs.dev.num_features, K = gs.dev.num_levels * F;
  if (K != 32) return fail(h, RC_ERR_UNSUPPORTED, "rc_normals_backward: the last level needs 32 grid features");
  if (n == 0) return RC_OK;
  for (size_t l = 0; l < gs.sizes.size(); ++l)
    if (!gs.loaded[l]) return fail(h, RC_ERR_MISSING_WEIGHT, "rc_normals_backward: missing " + gs.prefix + "/" + level_name(gs.cfg, gs.sizes, gs.sizes[l]));
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  int rc;
  // the layers may have been reloaded since the last call (an optimizer step): repack the stream then
  if (h->nbwd_gen != h->layers_gen) {
    if ((rc = pack_normals_stream(h))) return rc;
    h->nbwd_gen = h->layers_gen;
  }
  const int64_t ld = (n + 63) / 64 * 64;
  WsUse use(h, WS_NORMALS, st);
  if ((rc = use.rc)) return rc;
  NormalsWs& t = ws_extra<NormalsWs>(use.s);
  const int nwaves = rc_wgrad_waves(n);
  if ((rc = ws_alloc(h, {{t.feat, (int64_t)K * ld}, {t.jac, 3 * (int64_t)K * ld}, {t.gf, (int64_t)K * ld}, {t.ghat, 3 * n}, {t.u, n * 32},
                         {t.t0, n * 64}, {t.a0, n * 64}, {t.t1, n * 64}, {t.a2, n * 64}, {t.ones, n}, {t.normals, 3 * n},
                         {t.partial, rc_wgrad_partial_floats(nwaves)}})))
    return rc;
  const std::vector<GradSeg> segs = density_grad_segments(h, level);

  rc_launch_hashgrid(gs.dev, points, 0, n, t.feat.p, 1, ld, h->cfg.contract_radius, t.jac.p, st);
  RcNormalsBwdArgs b{};
  b.feat = t.feat.p; b.jac = t.jac.p; b.n = n; b.ld = ld; b.wstream = h->packs.nbwd.p;
  b.points = points; b.contract_radius = h->cfg.contract_radius; b.d_normals = d_normals;
  b.normals = normals_out ? normals_out : t.normals.p;
  b.u = t.u.p; b.t0 = t.t0.p; b.a0 = t.a0.p; b.t1 = t.t1.p; b.a2 = t.a2.p; b.ones = t.ones.p; b.gf = t.gf.p; b.ghat = t.ghat.p;
  rc_launch_normals_bwd(b, st);

  // dW0 = u^T t0, dW1 = a0^T t1, dw_out = sum_p a2: k_wgrad's contractions (fe := u, d1 := t0; a1 := a0, d2 := t1; a2, graw := 1)
  RcWgradArgs w{};
  w.a1 = t.a0.p; w.d2 = t.t1.p; w.fe = t.u.p; w.d1 = t.t0.p; w.a2 = t.a2.p; w.graw = t.ones.p; w.n = n; w.partial = t.partial.p;
  rc_launch_wgrad(w, K, grads + segs[gs.sizes.size()].offset, st, true);

  RcGridScatterArgs sa{};
  sa.grid = gs.dev;
  for (size_t l = 0; l < gs.sizes.size(); ++l) sa.gtable[l] = grads + segs[l].offset;
  sa.points = points; sa.n = n; sa.ld = ld; sa.dfeat = t.gf.p; sa.contract_radius = h->cfg.contract_radius;
  rc_launch_grid_scatter_jac(sa, t.ghat.p, st);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

int rc_geometry_smoothness_backward(rc_handle* h, const rc_rays* rays, const float* lossmult, int64_t n, const rc_randoms* rnd,
                                    float anneal, const float* noise, const rc_geometry_smoothness* cfg, float* density_grads,
                                    float* loss, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const rc_config& c = h->cfg;
  const int NL = c.num_levels;
  if (n < 0) return fail(h, RC_ERR_INVALID_ARG, "rc_geometry_smoothness_backward: negative n_rays");
  if (!rays || !cfg) return fail(h, RC_ERR_INVALID_ARG, "rc_geometry_smoothness_backward: null rays/cfg");
  if (!(anneal >= 0.0f) || !std::isfinite(anneal))
    return fail(h, RC_ERR_INVALID_ARG, "rc_geometry_smoothness_backward: anneal must be finite and >= 0");
  for (float v : {cfg->noise, cfg->weight_normals, cfg->weight_normals_pred, cfg->weight_density})
    if (!std::isfinite(v)) return fail(h, RC_ERR_INVALID_ARG, "rc_geometry_smoothness_backward: the loss settings must be finite");
  if (cfg->weight_normals_pred != 0.0f)
    return fail(h, RC_ERR_UNSUPPORTED, "rc_geometry_smoothness_backward: weight_normals_pred must be 0");
  if (h->transient) return fail(h, RC_ERR_UNSUPPORTED, "rc_geometry_smoothness_backward: not available on a time-resolved cache handle");
  if (n == 0) return RC_OK;
  if (!loss) return fail(h, RC_ERR_INVALID_ARG, "rc_geometry_smoothness_backward: null loss");
  if (!noise) return fail(h, RC_ERR_INVALID_ARG, "rc_geometry_smoothness_backward: null noise");
  int rc;
  if ((rc = check_rays(h, rays, "rc_geometry_smoothness_backward"))) return rc;
  const int S2 = c.num_samples[NL - 1];
  if (S2 < 1 || S2 > 32) return fail(h, RC_ERR_UNSUPPORTED, "rc_geometry_smoothness_backward: needs <= 32 samples on the last level");
  const GridState& gs = h->grids[NL - 1];
  const int K = gs.dev.num_levels * gs.dev.num_features;
  if (K != 32) return fail(h, RC_ERR_UNSUPPORTED, "rc_geometry_smoothness_backward: the last level needs 32 grid features");
  RoctxScope roctx_call("rc_geometry_smoothness_backward");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  if ((rc = ensure_packed(h))) return rc;
  const bool grads = density_grads != nullptr;
  const bool dens_term = cfg->weight_density != 0.0f;
  WsUse use(h, WS_GSMOOTH, st);
  if ((rc = use.rc)) return rc;
  RenderWs& w = use.s.r;
  GSmoothWs& x = ws_extra<GSmoothWs>(use.s);
  const int64_t np = n * S2;
  if ((rc = ensure_workspace(h, w, n)) ||
      (rc = ws_alloc(h, {{x.means_p, 3 * np}, {x.feat_p, (int64_t)K * np}, {x.jac_p, 3 * (int64_t)K * np}, {x.density_p, np},
                         {x.normals_p, 3 * np}, {x.points, 3 * np}, {x.points_p, 3 * np}, {x.loss_ray, n}})))
    return rc;
  if (grads && (rc = ws_alloc(h, {{x.d_normals, 3 * np}, {x.d_normals_p, 3 * np}, {x.d_density, np}, {x.d_density_p, np}}))) return rc;

  // 1. the training forward: the sampler levels, the last with the analytic normals
  RenderArgs A = cache_pass(rays, rnd, n);
  A.anneal = anneal; A.stop = RENDER_LEVELS; A.force_grad = true;
  enqueue_all(h, A, w, st);

  // 2. x' = x + noise * cfg->noise, 3. the last level at x'
  rc_launch_gsmooth_points(w.means[NL - 1].p, noise, cfg->noise, np, x.means_p.p, x.points.p, x.points_p.p, st);
  rc_launch_hashgrid(gs.dev, x.means_p.p, 1, np, x.feat_p.p, 1, np, c.contract_radius, x.jac_p.p, st);
  RcDensityMlpArgs da{};
  da.feat = x.feat_p.p; da.n = np; da.ld = np; da.K = K;
  da.wstream = h->packs.dens[NL - 1].p; da.means = x.means_p.p;
  da.density_bias = c.density_bias; da.contract_radius = c.contract_radius; da.bbox = gs.cfg.bbox;
  da.last = 1; da.density = x.density_p.p;
  da.jac = x.jac_p.p; da.normals_grad = x.normals_p.p;
  rc_launch_density_mlp(da, st);

  // 4. the per-ray values and the upstream gradients, 5. the loss
  RcGSmoothLossArgs ga{};
  ga.n = n; ga.S = S2;
  ga.density = w.density[NL - 1].p; ga.tdist = w.tdist[NL - 1].p; ga.directions = rays->directions;
  ga.normals = w.normals_grad.p; ga.density_p = x.density_p.p; ga.normals_p = x.normals_p.p; ga.lossmult = lossmult;
  ga.wn3 = (float)((double)cfg->weight_normals / 3.0); ga.wd = cfg->weight_density;
  ga.gn = (float)((double)cfg->weight_normals / (3.0 * (double)np));      // jnp.mean over [n, S, 3]
  ga.gd = (float)((double)cfg->weight_density / (double)np);              // jnp.mean over [n, S]
  ga.weights = w.weights[NL - 1].p; ga.loss_ray = x.loss_ray.p;
  ga.d_normals = grads ? x.d_normals.p : nullptr; ga.d_normals_p = grads ? x.d_normals_p.p : nullptr;
  ga.d_density = grads ? x.d_density.p : nullptr; ga.d_density_p = grads ? x.d_density_p.p : nullptr;
  rc_launch_gsmooth_loss(ga, st);
  RcInterlevelReduce r{};
  r.mult[0] = 1.0f; r.count[0] = (double)np;
  rc_launch_interlevel_reduce(x.loss_ray.p, n, 1, r, loss, st);
  RC_HIP(h, hipGetLastError());
  if (!grads) return RC_OK;

  // 6. per chunk: through the normals at x and at x', through the density at both when that term is on
  const int64_t CH = np < kDataChunk ? np : kDataChunk;
  for (int64_t c0 = 0; c0 < np; c0 += CH) {
    const int64_t C = np - c0 < CH ? np - c0 : CH;
    if ((rc = rc_normals_backward(h, x.points.p + 3 * c0, C, x.d_normals.p + 3 * c0, density_grads, nullptr, stream_v))) return rc;
    if ((rc = rc_normals_backward(h, x.points_p.p + 3 * c0, C, x.d_normals_p.p + 3 * c0, density_grads, nullptr, stream_v))) return rc;
    if (dens_term) {
      if ((rc = rc_density_backward(h, NL - 1, x.points.p + 3 * c0, C, x.d_density.p + c0, nullptr, density_grads, nullptr, stream_v)))
        return rc;
      if ((rc = rc_density_backward(h, NL - 1, x.points_p.p + 3 * c0, C, x.d_density_p.p + c0, nullptr, density_grads, nullptr, stream_v)))
        return rc;
    }
  }
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}
