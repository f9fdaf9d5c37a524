// Host side of the training backward of one level's density field (rc_train.hip); included by rc_api.hip.  Also the
// gradient-buffer layouts (GradSeg, dense_grad_segments, copy_segments) that rc_data_host.inc builds on.

namespace {

// Gradient buffer of level l: the grid tables in level order, each in the layout of the loaded tensor
// (dense [N,N,N,F] indexed [x,y,z], hashed [T,F]), then the density MLP
// [density_layers_0/kernel K x 64 | bias 64 | density_layers_1/kernel 64 x 64 | bias 64 |
//  output_density_layer/kernel 64 x 1 | bias 1].
struct GradSeg { std::string name; int64_t offset, size; int ndim; int64_t shape[4]; };

// tables of one grid in level order
std::vector<GradSeg> grid_grad_segments(const GridState& gs, int64_t& off) {
  std::vector<GradSeg> v;
  const int F = gs.cfg.num_features;
  for (size_t l = 0; l < gs.sizes.size(); ++l) {
    const int n = gs.sizes[l];
    GradSeg s{};
    s.name = gs.prefix + "/" + level_name(gs.cfg, gs.sizes, n);
    s.offset = off;
    if (is_dense(gs.cfg, n)) { s.ndim = 4; s.shape[0] = s.shape[1] = s.shape[2] = n; s.shape[3] = F; s.size = (int64_t)n * n * n * F; }
    else { s.ndim = 2; s.shape[0] = gs.cfg.hash_map_size; s.shape[1] = F; s.size = (int64_t)gs.cfg.hash_map_size * F; }
    off += s.size;
    v.push_back(s);
  }
  return v;
}

// dense layer `path`: kernel [in, out], then bias [out]
void dense_grad_segments(std::vector<GradSeg>& v, int64_t& off, const std::string& path, int in, int out) {
  GradSeg k{}; k.name = path + "/kernel"; k.offset = off; k.size = (int64_t)in * out; k.ndim = 2; k.shape[0] = in; k.shape[1] = out;
  off += k.size; v.push_back(k);
  GradSeg b{}; b.name = path + "/bias"; b.offset = off; b.size = out; b.ndim = 1; b.shape[0] = out;
  off += b.size; v.push_back(b);
}

// floats of a gradient buffer
int64_t grad_size(const std::vector<GradSeg>& v) { return v.back().offset + v.back().size; }

std::vector<GradSeg> density_grad_segments(rc_handle* h, int level) {
  const GridState& gs = h->grids[level];
  int64_t off = 0;
  std::vector<GradSeg> v = grid_grad_segments(gs, off);
  const int K = (int)gs.sizes.size() * gs.cfg.num_features;
  const std::string base = "params/Cache/Sampler/MLP_" + std::to_string(level);
  dense_grad_segments(v, off, base + "/density_layers_0", K, 64);
  dense_grad_segments(v, off, base + "/density_layers_1", 64, 64);
  dense_grad_segments(v, off, base + "/output_density_layer", 64, 1);
  return v;
}

// rc_*_grad_layout: the segments into the caller's array
int copy_segments(rc_handle* h, const std::vector<GradSeg>& v, rc_grad_segment* segs, int32_t capacity, int32_t* count, const char* who) {
  if (!count) return fail(h, RC_ERR_INVALID_ARG, std::string(who) + ": null count");
  *count = (int32_t)v.size();
  if (!segs) return RC_OK;
  if (capacity < (int32_t)v.size()) return fail(h, RC_ERR_INVALID_ARG, std::string(who) + ": capacity too small");
  for (size_t i = 0; i < v.size(); ++i) {
    memset(&segs[i], 0, sizeof(rc_grad_segment));
    snprintf(segs[i].name, sizeof(segs[i].name), "%s", v[i].name.c_str());
    segs[i].offset = v[i].offset; segs[i].size = v[i].size; segs[i].ndim = v[i].ndim;
    for (int d = 0; d < 4; ++d) segs[i].shape[d] = v[i].shape[d];
  }
  return RC_OK;
}

// Stream of k_density_bwd: the forward fragments of every level followed by W1^T, W0^T.
int pack_train_stream(rc_handle* h, int level) {
  std::string missing;
  const std::string base = "params/Cache/Sampler/MLP_" + std::to_string(level);
  const HostLayer* d0 = need(h, base + "/density_layers_0", missing);
  const HostLayer* d1 = need(h, base + "/density_layers_1", missing);
  const HostLayer* dout = need(h, base + "/output_density_layer", missing);
  if (!missing.empty()) return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: " + missing);
  std::vector<Step> s;
  steps_natural(s, d0->in, 0); step_bias(s);
  std::vector<float> stream = pack_f32(s, {tile_full(d0, 0), tile_full(d0, 1)});
  s.clear(); steps_acc(s, 2, 0); step_bias(s);
  append(stream, pack_f32(s, {tile_full(d1, 0), tile_full(d1, 1)}));
  append(stream, pack_dot({Col{dout, 0}}, 2, false));
  HostLayer w1t, w0t;
  w1t.in = d1->out; w1t.out = d1->in; w1t.kernel.resize(d1->kernel.size()); w1t.bias.assign(w1t.out, 0.0f);
  for (int r = 0; r < d1->in; ++r) for (int c2 = 0; c2 < d1->out; ++c2) w1t.kernel[(size_t)c2 * w1t.out + r] = d1->kernel[(size_t)r * d1->out + c2];
  w0t.in = d0->out; w0t.out = d0->in; w0t.kernel.resize(d0->kernel.size()); w0t.bias.assign(w0t.out, 0.0f);
  for (int r = 0; r < d0->in; ++r) for (int c2 = 0; c2 < d0->out; ++c2) w0t.kernel[(size_t)c2 * w0t.out + r] = d0->kernel[(size_t)r * d0->out + c2];
  std::vector<Step> sb; steps_acc(sb, 2, 0);
  append(stream, pack_f32(sb, {tile_full(&w1t, 0, 0, false), tile_full(&w1t, 1, 0, false)}));
  append(stream, pack_f32(sb, {tile_full(&w0t, 0, 0, false)}));
  return upload(h, h->packs.train[level], pad_stream(stream));
}

}  // namespace

int64_t rc_density_grad_size(rc_handle* h, int32_t level) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (level < 0 || level >= h->cfg.num_levels) return fail(h, RC_ERR_INVALID_ARG, "rc_density_grad_size: bad level");
  return grad_size(density_grad_segments(h, level));
  RC_CATCH(h)
}

int rc_density_grad_layout(rc_handle* h, int32_t level, rc_grad_segment* segs, int32_t capacity, int32_t* count) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (level < 0 || level >= h->cfg.num_levels) return fail(h, RC_ERR_INVALID_ARG, "rc_density_grad_layout: bad level");
  return copy_segments(h, density_grad_segments(h, level), segs, capacity, count, "rc_density_grad_layout");
  RC_CATCH(h)
}

int rc_density_backward(rc_handle* h, int32_t level, const float* points, int64_t n, const float* d_density,
                        const float* d_feature, float* grads, float* density_out, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (level < 0 || level >= h->cfg.num_levels) return fail(h, RC_ERR_INVALID_ARG, "rc_density_backward: bad level");
  if (n < 0 || (n > 0 && (!points || !d_density)) || !grads) return fail(h, RC_ERR_INVALID_ARG, "rc_density_backward: null buffer");
  if (n == 0) return RC_OK;
  GridState& gs = h->grids[level];
  for (size_t l = 0; l < gs.sizes.size(); ++l)
    if (!gs.loaded[l]) return fail(h, RC_ERR_MISSING_WEIGHT, "rc_density_backward: missing " + gs.prefix + "/" + level_name(gs.cfg, gs.sizes, gs.sizes[l]));
  const int F = gs.dev.num_features, K = gs.dev.num_levels * F;
  const int ks0 = (K + 1) / 2 + 1;
  if (ks0 != 4 && ks0 != 5 && ks0 != 17) return fail(h, RC_ERR_UNSUPPORTED, "rc_density_backward: unsupported feature count");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  int rc;
  // the layers may have been reloaded since the last call (an optimizer step): repack this level's stream then
  if (h->train_gen[level] != h->layers_gen) {
    if ((rc = pack_train_stream(h, level))) return rc;
    h->train_gen[level] = h->layers_gen;
  }
  const int64_t ld = (n + 63) / 64 * 64;
  WsUse use(h, WS_TRAIN, st);
  if ((rc = use.rc)) return rc;
  TrainWs& t = ws_extra<TrainWs>(use.s);
  const int nwaves = rc_wgrad_waves(n);
  if ((rc = ws_alloc(h, {{t.feat, (int64_t)K * ld}, {t.dfeat, (int64_t)K * ld}, {t.a1, n * 64}, {t.a2, n * 64}, {t.d2, n * 64},
                         {t.d1, n * 64}, {t.fe, n * 32}, {t.graw, n}, {t.density, n}, {t.partial, rc_wgrad_partial_floats(nwaves)}})))
    return rc;

  if (!h->train_stream) {
    h->train_stream = rc_helper_stream(1);
    bool ok = h->train_stream != nullptr;
    for (hipEvent_t& e : h->ev_train) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
      h->train_stream = nullptr;
      for (hipEvent_t& e : h->ev_train) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    }
  }
  (void)rc_train_prepare();
  const float* const wstream = h->packs.train[level].p;
  const std::vector<GradSeg> segs = density_grad_segments(h, level);

  // The whole call as launches on `q` (the caller's stream, or the capture stream of the graph below).
  // The weight gradients (k_wgrad + k_grad_reduce: matrix cores, 40 us) and the table gradients (memory-side atomics) both
  // read what k_density_bwd left and write disjoint segments of `grads`: for an F = 1 grid the former run on a stream of the
  // handle's own beside the scatter (highest priority and launched first: k_wgrad is one workgroup per CU, the scatter's
  // threads would otherwise hold every CU until they have drained), forked from and joined to `q` with events, so to the
  // caller everything of the call is ordered on its stream.
  auto enqueue = [&](hipStream_t q) {
    rc_launch_hashgrid(gs.dev, points, 0, n, t.feat.p, 1, ld, h->cfg.contract_radius, nullptr, q);
    RcDensityBwdArgs b{};
    b.feat = t.feat.p; b.n = n; b.ld = ld; b.K = K; b.wstream = wstream;
    b.points = points; b.density_bias = h->cfg.density_bias; b.contract_radius = h->cfg.contract_radius; b.bbox = gs.cfg.bbox;
    b.d_density = d_density; b.d_feature = d_feature;
    b.density = density_out ? density_out : t.density.p; b.graw = t.graw.p;
    b.a1 = t.a1.p; b.a2 = t.a2.p; b.d2 = t.d2.p; b.d1 = t.d1.p; b.fe = t.fe.p; b.dfeat = t.dfeat.p;
    rc_launch_density_bwd(b, q);

    RcWgradArgs w{};
    w.a1 = t.a1.p; w.d2 = t.d2.p; w.fe = t.fe.p; w.d1 = t.d1.p; w.a2 = t.a2.p; w.graw = t.graw.p; w.n = n; w.partial = t.partial.p;
    // F = 1 grids: k_wgrad beside k_grid_scatter_sliced (-25 us per call).  F = 4 grids: no fork -- beside k_grid_scatter<4>
    // the weight gradients stretch to the scatter's own length (0.194 ms per call on one stream, 0.198 forked), and a call
    // that forked TWO helper streams (the second one for the LDS-accumulated levels) was measured at 0.37 ms in a process
    // that had run the material stage before it (every kernel of the call 2-3x slower, 100 us of host time between calls).
    const bool forked = F != 4 && h->train_stream && hipEventRecord(h->ev_train[0], q) == hipSuccess &&
                        hipStreamWaitEvent(h->train_stream, h->ev_train[0], 0) == hipSuccess;
    rc_launch_wgrad(w, K, grads + segs[gs.sizes.size()].offset, forked ? h->train_stream : q);

    RcGridScatterArgs sa{};
    sa.grid = gs.dev;
    for (size_t l = 0; l < gs.sizes.size(); ++l) sa.gtable[l] = grads + segs[l].offset;
    sa.points = points; sa.n = n; sa.ld = ld; sa.dfeat = t.dfeat.p; sa.contract_radius = h->cfg.contract_radius;
    rc_launch_grid_scatter(sa, q);
    if (forked &&       // join (before the workspace set is released)
        (hipEventRecord(h->ev_train[1], h->train_stream) != hipSuccess || hipStreamWaitEvent(q, h->ev_train[1], 0) != hipSuccess))
      (void)hipStreamSynchronize(h->train_stream);
  };

  // (Replaying the call as one hipGraph -- fork and join captured -- was tried against its ~140 us of host time per call:
  // 0.28-0.40 ms per call instead of 0.16-0.20, a three-branch graph launches slower than its six plain launches.)
  enqueue(st);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

// ---------------------------------------------------------------------------------------------------------
// rc_hashgrid_backward: the transpose of rc_hashgrid_lookup for any of the handle's grids
// ---------------------------------------------------------------------------------------------------------
int rc_hashgrid_grad_layout(rc_handle* h, int32_t grid_id, rc_grad_segment* segs, int32_t capacity, int32_t* count, int64_t* total) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (grid_id < 0 || grid_id >= 6 || h->grids[grid_id].sizes.empty()) return fail(h, RC_ERR_INVALID_ARG, "rc_hashgrid_grad_layout: bad grid_id");
  int64_t off = 0;
  const std::vector<GradSeg> v = grid_grad_segments(h->grids[grid_id], off);
  if (total) *total = off;
  return copy_segments(h, v, segs, capacity, count, "rc_hashgrid_grad_layout");
  RC_CATCH(h)
}

int rc_hashgrid_backward(rc_handle* h, int32_t grid_id, const float* points, int64_t n, const float* d_features, float* grads,
                         int32_t apply_contraction, void* stream) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (grid_id < 0 || grid_id >= 6 || h->grids[grid_id].sizes.empty()) return fail(h, RC_ERR_INVALID_ARG, "rc_hashgrid_backward: bad grid_id");
  if (n < 0 || (n > 0 && (!points || !d_features)) || !grads) return fail(h, RC_ERR_INVALID_ARG, "rc_hashgrid_backward: null buffer");
  if (n == 0) return RC_OK;
  GridState& gs = h->grids[grid_id];
  RC_HIP(h, hipSetDevice(h->device));
  int64_t off = 0;
  const std::vector<GradSeg> segs = grid_grad_segments(gs, off);
  RcGridScatterArgs sa{};
  sa.grid = gs.dev;
  for (size_t l = 0; l < gs.sizes.size(); ++l) sa.gtable[l] = grads + segs[l].offset;
  sa.points = points; sa.n = n; sa.ld = n; sa.dfeat = d_features; sa.point_major = 1;
  sa.contract_radius = apply_contraction ? h->cfg.contract_radius : 0.0f;
  rc_launch_grid_scatter(sa, (hipStream_t)stream);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}
