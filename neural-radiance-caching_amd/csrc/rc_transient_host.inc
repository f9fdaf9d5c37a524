// Host side of the time-resolved cache (included at the end of rc_api.hip): weight packing for
// rc_transient.hip, the launch tail after the proposal sampler, rc_set_transient / rc_render_transient.
namespace {

// 16 activation slots fed as 8 natural steps: rows base .. base + 14, slot 15 = bias row (or nothing)
void steps_slots16(std::vector<Step>& s, int base, bool bias_in_slot15) {
  for (int i = 0; i < 8; ++i) s.push_back({{base + 2 * i, i < 7 ? base + 2 * i + 1 : (bias_in_slot15 ? -2 : -1)}});
}

int repack_transient(rc_handle* h) {
  std::string missing;
  const std::string sh = "params/Cache/Shader";
  const HostLayer* bott = need(h, sh + "/bottleneck_layer", missing);
  const HostLayer* rough = need(h, sh + "/roughness_layer", missing);
  const HostLayer* tint = need(h, sh + "/tint_layer", missing);
  const HostLayer* dtint = need(h, sh + "/direct_tint_layer", missing);
  const HostLayer* alb = need(h, sh + "/albedo_layer", missing);
  const HostLayer* i0 = need(h, sh + "/integrated_brdf_layers_0", missing);
  const HostLayer* i1 = need(h, sh + "/integrated_brdf_layers_1", missing);
  const HostLayer* io = need(h, sh + "/output_integrated_brdf_layer", missing);
  const HostLayer* b0 = need(h, sh + "/brdf_layers_0", missing);
  const HostLayer* b1 = need(h, sh + "/brdf_layers_1", missing);
  const HostLayer* bo = need(h, sh + "/output_brdf_layer", missing);
  const HostLayer* r0 = need(h, sh + "/irradiance_layers_0", missing);
  const HostLayer* r1 = need(h, sh + "/irradiance_layers_1", missing);
  const HostLayer* ro = need(h, sh + "/transient_indirect_layer", missing);
  const std::string sl = sh + "/SurfaceLightField";
  const HostLayer* l0 = need(h, sl + "/layer_0", missing);
  const HostLayer* l1 = need(h, sl + "/layer_1", missing);
  const HostLayer* l2 = need(h, sl + "/layer_2", missing);
  const HostLayer* lb = need(h, sl + "/layer_bottleneck", missing);
  const HostLayer* lo = need(h, sl + "/output_rgba_layer", missing);
  if (!missing.empty()) return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: " + missing);
  if (!h->have_light_power) return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: " + sh + "/light_power");
  {
    // k_transient_shader, in TFrags order
    std::vector<float> stream;
    std::vector<Step> s;
    // the linear bottleneck is folded into its consumers (fp64 products), see rc_api.hip repack()
    const int FE = bott->in, BW = bott->out;
    auto fold = [&](const HostLayer* L, int row0, int extra_rows) {
      HostLayer f;
      f.in = FE + extra_rows; f.out = L->out;
      f.kernel.assign((size_t)f.in * f.out, 0.0f); f.bias.assign(f.out, 0.0f);
      f.have_kernel = f.have_bias = true;
      for (int o = 0; o < L->out; ++o) {
        for (int i = 0; i < FE; ++i) {
          double a = 0.0;
          for (int m = 0; m < BW; ++m) a += (double)bott->kernel[(size_t)i * BW + m] * (double)L->kernel[(size_t)(row0 + m) * L->out + o];
          f.kernel[(size_t)i * f.out + o] = (float)a;
        }
        double b = (double)L->bias[o];
        for (int m = 0; m < BW; ++m) b += (double)bott->bias[m] * (double)L->kernel[(size_t)(row0 + m) * L->out + o];
        f.bias[o] = (float)b;
        for (int e = 0; e < extra_rows; ++e) f.kernel[(size_t)(FE + e) * f.out + o] = L->kernel[(size_t)(row0 + BW + e) * L->out + o];
      }
      return f;
    };
    HostLayer l0f = fold(l0, 0, 87), lbf = fold(lb, 128, 87), i0f = fold(i0, 0, 1), b0f = fold(b0, 0, 15);
    // heads on [hidden (acc order) | appearance | bias]: (roughness, tint, direct tint, albedo)
    steps_acc(s, 2, 0); steps_natural(s, 32, 64); step_bias(s);
    std::vector<Col> regs = {Col{rough, 0}, Col{tint, 0}, Col{tint, 1}, Col{tint, 2}, Col{dtint, 0},
                             Col{dtint, 1}, Col{dtint, 2}, Col{alb, 0},  Col{alb, 1},  Col{alb, 2}};
    append(stream, pack(s, {tile_by_reg(regs)}));
    // irradiance trunk: the same 49 steps + pos_enc(lights) (rows 96..110)
    steps_slots16(s, 96, false);
    append(stream, pack(s, {tile_full(r0, 0), tile_full(r0, 1)}));
    s.clear(); steps_acc(s, 2, 0); step_bias(s);
    append(stream, pack(s, {tile_full(r1, 0), tile_full(r1, 1)}));
    // SLF layer_0 + input part of layer_bottleneck (folded) over [feature | IDE (real | imag) | pos_enc(contract(lights)) + bias]
    s.clear(); steps_acc(s, 2, 0); steps_natural(s, 32, 64);
    for (int i = 0; i < 36; ++i) s.push_back({{FE + i, FE + 36 + i}});
    steps_slots16(s, FE + 72, true);
    append(stream, pack(s, {tile_full(&l0f, 0), tile_full(&l0f, 1), tile_full(&l0f, 2), tile_full(&l0f, 3),
                            tile_full(&lbf, 0), tile_full(&lbf, 1), tile_full(&lbf, 2), tile_full(&lbf, 3)}));
    // integrated BRDF (first layer folded)
    s.clear(); steps_acc(s, 2, 0); steps_natural(s, 32, 64); s.push_back({{FE, -2}});
    append(stream, pack(s, {tile_full(&i0f, 0), tile_full(&i0f, 1)}));
    s.clear(); steps_acc(s, 2, 0); step_bias(s);
    append(stream, pack(s, {tile_full(i1, 0), tile_full(i1, 1)}));
    append(stream, pack(s, {tile_by_reg({Col{io, 0}})}));
    // BRDF towards the light (first layer folded): [feature | pos_enc(sorted dots, n.h) + bias]
    s.clear(); steps_acc(s, 2, 0); steps_natural(s, 32, 64); steps_slots16(s, FE, true);
    append(stream, pack(s, {tile_full(&b0f, 0), tile_full(&b0f, 1)}));
    s.clear(); steps_acc(s, 2, 0); step_bias(s);
    append(stream, pack(s, {tile_full(b1, 0), tile_full(b1, 1)}));
    append(stream, pack(s, {tile_by_reg({Col{bo, 0}})}));
    // SLF trunk
    s.clear(); steps_acc(s, 4, 0); step_bias(s);
    append(stream, pack(s, {tile_full(l1, 0), tile_full(l1, 1), tile_full(l1, 2), tile_full(l1, 3)}));
    append(stream, pack(s, {tile_full(l2, 0), tile_full(l2, 1), tile_full(l2, 2), tile_full(l2, 3)}));
    std::vector<Step> sb; steps_acc(sb, 4, 0);
    append(stream, pack(sb, {tile_full(lb, 0, 0, false), tile_full(lb, 1, 0, false), tile_full(lb, 2, 0, false),
                             tile_full(lb, 3, 0, false)}));
    if ((int)(stream.size() / 64) != rc_transient_shader_frags())
      return fail(h, RC_ERR_INVALID_ARG, "internal: transient shader stream length mismatch");
    int rc = upload(h, h->packs.t_shader, pad_stream(stream));
    if (rc) return rc;
  }
  {
    // k_transient_bins: per column tile of 32 histogram entries [output_rgba_layer (128 + bias) | transient_indirect_layer (64 + bias)],
    // every tile padded to whole chunks of the kernel's LDS ring (rc_pack_host.h pack_bins_stream)
    const int cols = 3 * h->tcfg.n_bins, tiles = (cols + 31) / 32;
    const std::vector<float> stream = pack_bins_stream(*lo, *ro, cols, rc_transient_bins_frags() / tiles);
    if ((int)(stream.size() / 64) != rc_transient_bins_frags())
      return fail(h, RC_ERR_INVALID_ARG, "internal: transient bins stream length mismatch");
    int rc = upload(h, h->packs.t_bins, pad_stream(stream));
    if (rc) return rc;
  }
  {
    // k_transient_slice (rc_transient_slice.hip): the same two heads as plain columns (rc_pack_host.h pack_slice_columns)
    const int cols = 3 * h->tcfg.n_bins;
    static_assert(kRcSliceStrideSlf >= 2 * 64 + 1 && kRcSliceStrideIrr >= 2 * 32 + 1, "a column holds every row and the bias");
    int rc = upload(h, h->packs.t_slice_slf, pack_slice_columns(*lo, 4, cols, kRcSliceStrideSlf));
    if (rc) return rc;
    if ((rc = upload(h, h->packs.t_slice_irr, pack_slice_columns(*ro, 2, cols, kRcSliceStrideIrr)))) return rc;
  }
  {
    // temporal filter (render.py:411-413, rc_pack_host.h temporal_taps)
    const std::vector<float> taps = temporal_taps(h->tcfg.tfilter_sigma);
    h->n_taps = (int)taps.size();
    if (h->n_taps) {
      int rc = upload(h, h->packs.t_taps, taps);
      if (rc) return rc;
    }
  }
  h->fused_ok = false;
  h->packed_dirty = false;
  return RC_OK;
}

void enqueue_transient_slice(rc_handle* h, const RenderArgs& A, RenderWs& w, hipStream_t st);      // rc_transient_slice_host.inc

// What the integrator's kernels read alike, from the handle's settings: the shader's buffers of n rays in workspace set `w`
void transient_in(const rc_handle* h, const RenderWs& w, int64_t n, RcTransIn& b) {
  const rc_transient_config& t = h->tcfg;
  b.n_rays = n;
  b.slf_feat = w.t_slf.p; b.irr_feat = w.t_irr.p; b.tshade = w.tshade.p; b.weights = w.weights[h->cfg.num_levels - 1].p;
  b.exposure = t.exposure_time; b.shift = t.transient_shift;
  b.max_dists = (float)((double)(t.n_bins - 1) * (double)t.exposure_time);       // render_utils.py:1730
  b.irradiance_bias = t.irradiance_bias; b.slf_rgb_bias = t.slf_rgb_bias; b.indirect_scale = t.indirect_scale;
  b.rgb_max = t.rgb_max; b.light_near = t.light_near;
  b.bin_zero_threshold_light = t.bin_zero_threshold_light; b.light_zero = t.light_zero;
}
void transient_taps(const rc_handle* h, RcTransTaps& f) { f.n_taps = h->n_taps; f.taps = h->n_taps ? h->packs.t_taps.p : nullptr; }

// After the proposal sampler and the appearance-grid lookup: shader, per-bin heads + compositing, scalar composites.
// `w` is workspace set 0 (the shadow rays use its extras and the secondary set).
void enqueue_transient_tail(rc_handle* h, const RenderArgs& A, RenderWs& w, hipStream_t st) {
  const rc_config& c = h->cfg;
  const rc_transient_config& t = h->tcfg;
  const int NL = c.num_levels;
  const int S2 = c.num_samples[NL - 1];
  const int64_t n = A.n, np2 = n * S2;
  const rc_transient_outputs& o = *A.tout;
  stage_mark(h, A.slot, ST_COMPOSITE, st);
  {
    // acc, distances and the geometry composites are those of the steady-state integrator (render.py:283-330);
    // this kernel also leaves the alpha-compositing weights of the last level in the workspace for the bins kernel
    rc_launch_composite(composite_args(h, A, w, false, true, 0.0f), st);
  }
  const float* occ = nullptr;
  if (t.use_occlusions) {
    // _compute_occlusions: n * S2 shadow rays through the secondary-ray sampler, weights only
    const int64_t nsec = np2;
    const ExtraWs& x = ws_extra<ExtraWs>(h->ws[WS_RENDER0]);
    RcShadowRayArgs sr{};
    sr.n = np2; sr.samples_per_ray = S2; sr.means = w.means[NL - 1].p; sr.normals = w.normals_grad.p; sr.lights = A.rays.lights;
    sr.normal_eps = c.secondary_normal_eps; sr.shadow_near = t.shadow_near; sr.shadow_far = t.shadow_far; sr.light_near = t.light_near;
    sr.origins = x.sh_origins.p; sr.dirs = x.sh_dirs.p; sr.near = x.sh_near.p; sr.far = x.sh_far.p;
    sr.out_normals = x.sh_normals.p; sr.out_lights = x.sh_lights.p;
    rc_launch_shadow_rays(sr, st);
    rc_rays shadow{};
    shadow.origins = sr.origins; shadow.directions = sr.dirs; shadow.viewdirs = sr.dirs; shadow.near = sr.near; shadow.far = sr.far;
    shadow.lights = sr.out_lights; shadow.normals = sr.out_normals;
    RenderArgs B = cache_pass(&shadow, A.shadow_rnd, nsec);
    B.mask = RC_PASS_CACHE | RC_PASS_SECONDARY; B.stop = RENDER_WEIGHTS;
    B.out.ptr[RC_OUT_ACC] = x.sh_acc.p;
    enqueue_all(h, B, h->ws[WS_SECONDARY].r, st);
    occ = x.sh_acc.p;
  }
  stage_mark(h, A.slot, ST_SHADER, st);
  {
    RcTransShaderArgs s{};
    s.n = np2; s.samples_per_ray = S2;
    s.hbuf = w.hbuf.p; s.app = w.app.p; s.means = w.means[NL - 1].p; s.normals = w.normals_pred.p;
    s.origins = A.rays.origins; s.viewdirs = A.rays.viewdirs; s.lights = A.rays.lights; s.cam_origins = A.cam_origins;
    s.occ = occ; s.occ_threshold = t.occ_threshold;
    s.wstream = h->packs.t_shader.p; s.ide_coef = h->ide_table.p;
    s.roughness_bias = c.roughness_bias; s.albedo_bias = t.albedo_bias; s.brdf_bias = t.brdf_bias; s.rgb_max = t.rgb_max;
    s.contract_radius = c.contract_radius;
    s.light_power = h->light_power; s.light_near = t.light_near; s.use_falloff = t.use_falloff; s.light_zero = t.light_zero;
    s.irr_feat = w.t_irr.p; s.slf_feat = w.t_slf.p; s.tshade = w.tshade.p;
    rc_launch_transient_shader(s, st);
  }
  if (A.tslices) {
    enqueue_transient_slice(h, A, w, st);       // rc_render_transient_slices: the bins that reach the asked times only
  } else {
    RcTransBinsArgs b{};
    transient_in(h, w, n, b); transient_taps(h, b); b.wstream = h->packs.t_bins.p;
    b.out_rgb = o.ptr[RC_TOUT_RGB]; b.out_direct = o.ptr[RC_TOUT_TRANSIENT_DIRECT_VIZ]; b.out_indirect = o.ptr[RC_TOUT_TRANSIENT_INDIRECT_VIZ];
    b.out_ti_diffuse = o.ptr[RC_TOUT_TRANSIENT_INDIRECT_DIFFUSE]; b.out_ti_specular = o.ptr[RC_TOUT_TRANSIENT_INDIRECT_SPECULAR];
    b.out_direct_rgb = o.ptr[RC_TOUT_DIRECT_RGB]; b.out_indirect_rgb = o.ptr[RC_TOUT_INDIRECT_RGB];
    b.out_integrated_rgb = o.ptr[RC_TOUT_INTEGRATED_RGB];
    b.out_diffuse_rgb = o.ptr[RC_TOUT_DIFFUSE_RGB]; b.out_specular_rgb = o.ptr[RC_TOUT_SPECULAR_RGB];
    b.out_albedo_rgb = o.ptr[RC_TOUT_ALBEDO_RGB]; b.out_occ = o.ptr[RC_TOUT_OCC]; b.out_indirect_occ = o.ptr[RC_TOUT_INDIRECT_OCC];
    b.out_irradiance_rgb = o.ptr[RC_TOUT_IRRADIANCE_RGB]; b.out_light_radiance_rgb = o.ptr[RC_TOUT_LIGHT_RADIANCE_RGB];
    b.out_n_dot_l_rgb = o.ptr[RC_TOUT_N_DOT_L_RGB]; b.out_direct_diffuse_rgb = o.ptr[RC_TOUT_DIRECT_DIFFUSE_RGB];
    b.out_direct_specular_rgb = o.ptr[RC_TOUT_DIRECT_SPECULAR_RGB]; b.out_indirect_diffuse_rgb = o.ptr[RC_TOUT_INDIRECT_DIFFUSE_RGB];
    b.out_indirect_specular_rgb = o.ptr[RC_TOUT_INDIRECT_SPECULAR_RGB]; b.out_direct_rgb_viz = o.ptr[RC_TOUT_DIRECT_RGB_VIZ];
    rc_launch_transient_bins(b, st);
  }
  stage_mark(h, A.slot, ST_COUNT, st);
}

}  // namespace

int rc_set_transient(rc_handle* h, const rc_transient_config* t) {
  RC_TRY
  if (!h || !t) return RC_ERR_INVALID_ARG;
  if (t->n_bins != 700) return fail(h, RC_ERR_UNSUPPORTED, "rc_set_transient: n_bins must be 700");
  if (!(t->exposure_time > 0.0f)) return fail(h, RC_ERR_INVALID_ARG, "rc_set_transient: exposure_time must be positive");
  if (h->cfg.num_levels < 1 || h->cfg.num_samples[h->cfg.num_levels - 1] != 32)
    return fail(h, RC_ERR_UNSUPPORTED, "rc_set_transient: the last sampling level must take 32 samples");
  if (!h->layers.empty()) return fail(h, RC_ERR_INVALID_ARG, "rc_set_transient: call before rc_load_weights");
  h->transient = true;
  h->tcfg = *t;
  h->packed_dirty = true;
  return RC_OK;
  RC_CATCH(h)
}

namespace {

// rc_render_transient and rc_render_transient_slices (`slices` non-NULL: k_transient_slice in place of k_transient_bins;
// `out` then holds the composite outputs asked for besides): checks of the rays, workspace, launch sequence
int render_transient_impl(rc_handle* h, const rc_rays* rays, const float* cam_origins, int64_t n, const rc_randoms* rnd,
                          const rc_randoms* shadow_rnd, const rc_transient_outputs* out, const rc_transient_slices* slices,
                          void* stream_v, const std::string& who) {
  if (!rays || !out) return fail(h, RC_ERR_INVALID_ARG, who + ": null rays/outputs");
  if (n < 0) return fail(h, RC_ERR_INVALID_ARG, who + ": negative n_rays");
  if (n == 0) return RC_OK;
  int rc;
  if ((rc = check_rays(h, rays, who.c_str()))) return rc;
  if (!rays->lights || !cam_origins) return fail(h, RC_ERR_INVALID_ARG, who + ": lights and cam_origins are required");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  if ((rc = ensure_packed(h))) return rc;
  WsUse use(h, WS_RENDER0, st);          // set 0 (and the secondary set) of the other entry points
  if ((rc = use.rc)) return rc;
  RenderWs& w = use.s.r;
  ExtraWs& x = ws_extra<ExtraWs>(use.s);
  if ((rc = ensure_workspace(h, w, n))) return rc;
  if (h->tcfg.use_occlusions) {
    const int64_t nsec = n * h->cfg.num_samples[h->cfg.num_levels - 1];
    if ((rc = ws_alloc(h, {{x.sh_origins, 3 * nsec}, {x.sh_dirs, 3 * nsec}, {x.sh_near, nsec}, {x.sh_far, nsec},
                           {x.sh_normals, 3 * nsec}, {x.sh_lights, 3 * nsec}, {x.sh_acc, nsec}})) ||
        (rc = ensure_workspace(h, h->ws[WS_SECONDARY].r, nsec)))
      return rc;
  }
  rc_shader_prepare();
  RenderArgs A = cache_pass(rays, rnd, n);
  A.tout = out; A.tslices = slices; A.cam_origins = cam_origins; A.shadow_rnd = shadow_rnd; A.force_grad = h->tcfg.use_occlusions != 0;
  // outputs shared with the steady-state compositing kernel
  A.out.ptr[RC_OUT_ACC] = out->ptr[RC_TOUT_ACC];
  A.out.ptr[RC_OUT_DISTANCE_MEAN] = out->ptr[RC_TOUT_DISTANCE_MEAN];
  A.out.ptr[RC_OUT_DISTANCE_MEDIAN] = out->ptr[RC_TOUT_DISTANCE_MEDIAN];
  A.out.ptr[RC_OUT_DISTANCE_PERCENTILE_5] = out->ptr[RC_TOUT_DISTANCE_PERCENTILE_5];
  A.out.ptr[RC_OUT_DISTANCE_PERCENTILE_95] = out->ptr[RC_TOUT_DISTANCE_PERCENTILE_95];
  A.out.ptr[RC_OUT_MEANS] = out->ptr[RC_TOUT_MEANS];
  A.out.ptr[RC_OUT_NORMALS] = out->ptr[RC_TOUT_NORMALS];
  A.out.ptr[RC_OUT_NORMALS_PRED] = out->ptr[RC_TOUT_NORMALS_PRED];
  A.out.ptr[RC_OUT_RAY_DISTS] = out->ptr[RC_TOUT_RAY_DISTS];
  A.out.ptr[RC_OUT_LIGHT_DISTS] = out->ptr[RC_TOUT_LIGHT_DISTS];
  enqueue_all(h, A, w, st);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
}

}  // namespace

int rc_render_transient(rc_handle* h, const rc_rays* rays, const float* cam_origins, int64_t n, const rc_randoms* rnd,
                        const rc_randoms* shadow_rnd, const rc_transient_outputs* out, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  RoctxScope roctx_call("rc_render_transient");
  if (!h->transient) return fail(h, RC_ERR_UNSUPPORTED, "rc_render_transient: call rc_set_transient first");
  return render_transient_impl(h, rays, cam_origins, n, rnd, shadow_rnd, out, nullptr, stream_v, "rc_render_transient");
  RC_CATCH(h)
}
