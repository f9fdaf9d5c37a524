// Host side of rc_adam_update (rc_optim.hip) and rc_load_params_flat; included by rc_api.hip.
//
// rc_adam_update: the call's buffers and their segments -> runs (consecutive segments of one group) and the tile table of
// k_adam -> with the norm clip, k_adam_sumsq + k_adam_norm on the workspace set WS_OPTIM -> k_adam.  rc_load_params_flat:
// the table segments of a layout device to device into the handle's tables, the dense segments in one copy to a
// page-locked host buffer, then the host layers and the stale marks of rc_load_weights.

namespace {

bool finite_all(const float* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

}  // namespace

int rc_adam_update(rc_handle* h, const rc_adam_buffer* bufs, int32_t nbuf, const rc_adam_step* step, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (!bufs || !step) return fail(h, RC_ERR_INVALID_ARG, "rc_adam_update: null bufs/step");
  if (nbuf < 1 || nbuf > RC_ADAM_MAX_BUFFERS || nbuf > kRcAdamMaxBufs)
    return fail(h, RC_ERR_INVALID_ARG, "rc_adam_update: nbuf must be in [1, RC_ADAM_MAX_BUFFERS]");
  const int G = step->ngroups;
  if (G < 1 || G > RC_ADAM_MAX_GROUPS || G > kRcAdamMaxGroups)
    return fail(h, RC_ERR_INVALID_ARG, "rc_adam_update: ngroups must be in [1, RC_ADAM_MAX_GROUPS]");
  if (!finite_all(step->lr, G) || !finite_all(step->b1, G) || !finite_all(step->b2, G) || !finite_all(step->one_minus_b1, G) ||
      !finite_all(step->one_minus_b2, G) || !finite_all(step->eps, G) || !finite_all(step->bias_correction1, G) ||
      !finite_all(step->bias_correction2, G) || !std::isfinite(step->grad_max_val) || !std::isfinite(step->grad_max_norm))
    return fail(h, RC_ERR_INVALID_ARG, "rc_adam_update: the step's scalars must be finite");
  RcAdamArgs a{};
  const int64_t tile = rc_adam_tile();
  int64_t blocks = 0;
  int runs = 0;
  for (int k = 0; k < nbuf; ++k) {
    const rc_adam_buffer& b = bufs[k];
    const std::string who = "rc_adam_update: buffer " + std::to_string(k);
    if (b.n < 1) return fail(h, RC_ERR_INVALID_ARG, who + ": n must be positive");
    const float* ptrs[4] = {b.params, b.grads, b.mu, b.nu};
    for (const float* p : ptrs)
      if (!p || (reinterpret_cast<uintptr_t>(p) & 15) != 0)
        return fail(h, RC_ERR_INVALID_ARG, who + ": params/grads/mu/nu must be non-null and 16-byte aligned");
    if (b.nseg < 1 || !b.seg_offset || !b.seg_size || !b.seg_group) return fail(h, RC_ERR_INVALID_ARG, who + ": no segments");
    RcAdamBuf& d = a.buf[k];
    d.params = b.params; d.grads = b.grads; d.mu = b.mu; d.nu = b.nu; d.n = b.n;
    d.block0 = blocks; d.run0 = runs;
    int64_t at = 0;
    for (int s = 0; s < b.nseg; ++s) {
      if (b.seg_offset[s] != at || b.seg_size[s] < 1) return fail(h, RC_ERR_INVALID_ARG, who + ": segments must cover [0, n) in order");
      const int grp = b.seg_group[s];
      if (grp < 0 || grp >= G) return fail(h, RC_ERR_INVALID_ARG, who + ": segment group out of range");
      at += b.seg_size[s];
      if (runs > d.run0 && a.run_group[runs - 1] == grp) { a.run_end[runs - 1] = at; continue; }
      if (runs == kRcAdamMaxRuns) return fail(h, RC_ERR_UNSUPPORTED, "rc_adam_update: more than 32 runs of one group");
      a.run_end[runs] = at; a.run_group[runs] = grp; ++runs;
    }
    if (at != b.n) return fail(h, RC_ERR_INVALID_ARG, who + ": segments must cover [0, n) in order");
    d.nruns = runs - d.run0;
    blocks += (b.n + tile - 1) / tile;
  }
  a.nbuf = nbuf;
  for (int g = 0; g < G; ++g)
    a.group[g] = RcAdamGroup{step->lr[g], step->b1[g], step->b2[g], step->one_minus_b1[g], step->one_minus_b2[g],
                             step->eps[g], step->bias_correction1[g], step->bias_correction2[g]};
  a.max_val = step->grad_max_val > 0.0f ? step->grad_max_val : 0.0f;
  a.zero_grads = step->zero_grads != 0;
  RoctxScope roctx_call("rc_adam_update");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  WsUse use(h, WS_OPTIM, st);
  int rc;
  if ((rc = use.rc)) return rc;
  OptimWs& x = ws_extra<OptimWs>(use.s);
  if (step->grad_max_norm > 0.0f) {
    if ((rc = ws_alloc(h, {{x.part, 2 * blocks}, {x.norm, 1}, {x.mult, 1}}))) return rc;     // part: doubles
    rc_launch_adam_norm(a, blocks, step->grad_max_norm, reinterpret_cast<double*>(x.part.p), x.mult.p, x.norm.p, st);
    a.mult = x.mult.p;
  }
  rc_launch_adam(a, blocks, st);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

int rc_load_params_flat(rc_handle* h, int32_t layout, const float* params, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (!params) return fail(h, RC_ERR_INVALID_ARG, "rc_load_params_flat: null params");
  // a time-resolved handle loads its per-bin heads and its sampler side only (the other layouts' trainers do not run on it)
  if (h->transient && layout != RC_LAYOUT_TRANSIENT_HEADS && layout != RC_LAYOUT_TRANSIENT_SAMPLER)
    return fail(h, RC_ERR_UNSUPPORTED, "rc_load_params_flat: not available on a time-resolved cache handle");
  if (layout != RC_LAYOUT_SHADER && layout != RC_LAYOUT_LIGHT && layout != RC_LAYOUT_MATERIAL && layout != RC_LAYOUT_ENVMAP &&
      layout != RC_LAYOUT_TRANSIENT_HEADS && layout != RC_LAYOUT_TRANSIENT_SAMPLER && (layout < 0 || layout >= h->cfg.num_levels))
    return fail(h, RC_ERR_INVALID_ARG, "rc_load_params_flat: layout must be a density level, RC_LAYOUT_SHADER, RC_LAYOUT_LIGHT, "
                                       "RC_LAYOUT_MATERIAL, RC_LAYOUT_ENVMAP, RC_LAYOUT_TRANSIENT_HEADS or RC_LAYOUT_TRANSIENT_SAMPLER");
  int rc;
  if ((rc = layout_check(h, layout, "rc_load_params_flat"))) return rc;
  const std::vector<GradSeg> segs = layout_segments(h, layout);
  const auto inv = dense_inventory(h->cfg, h->transient ? &h->tcfg : nullptr);
  // classify: grid table (grid, level) or dense layer (checked against the inventory)
  struct Dst { int g = -1, l = -1; };
  std::vector<Dst> dst(segs.size());
  std::vector<size_t> dense;
  for (size_t i = 0; i < segs.size(); ++i) {
    const GradSeg& s = segs[i];
    for (int g = 0; g < 6 && dst[i].g < 0; ++g) {
      const GridState& gs = h->grids[g];
      if (s.name.compare(0, gs.prefix.size() + 1, gs.prefix + "/") != 0) continue;
      for (size_t l = 0; l < gs.sizes.size(); ++l)
        if (s.name.substr(gs.prefix.size() + 1) == level_name(gs.cfg, gs.sizes, gs.sizes[l])) { dst[i].g = g; dst[i].l = (int)l; }
    }
    if (dst[i].g >= 0) continue;
    const size_t slash = s.name.rfind('/');
    auto it = inv.find(s.name.substr(0, slash));
    if (it == inv.end()) return fail(h, RC_ERR_INVALID_ARG, "rc_load_params_flat: unknown tensor " + s.name);
    dense.push_back(i);
  }
  RoctxScope roctx_call("rc_load_params_flat");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  WsUse use(h, WS_OPTIM, st);
  if ((rc = use.rc)) return rc;
  OptimWs& x = ws_extra<OptimWs>(use.s);
  // 1. the tables, device to device on the caller's stream
  for (size_t i = 0; i < segs.size(); ++i) {
    if (dst[i].g < 0) continue;
    GridState& gs = h->grids[dst[i].g];
    const int l = dst[i].l;
    DevBuf& b = gs.tables[l];
    const size_t bytes = (size_t)segs[i].size * sizeof(float);
    if (!b.p) { RC_HIP(h, hipMalloc((void**)&b.p, bytes)); b.bytes = bytes; }
    RC_HIP(h, hipMemcpyAsync(b.p, params + segs[i].offset, bytes, hipMemcpyDeviceToDevice, st));
    gs.dev.lvl[l].table = b.p;
    gs.dev.lvl[l].cell = nullptr;    // the derived tables are stale until the next repack
    gs.dev.lvl[l].rec = nullptr;
    gs.loaded[l] = true;
    h->packed_dirty = true;
  }
  // 2. the dense segments: runs of consecutive segments, gathered on the device when there is more than one run
  if (!dense.empty()) {
    std::vector<std::pair<int64_t, int64_t>> runs;     // (offset, floats) in the layout
    int64_t total = 0;
    for (size_t i : dense) {
      if (!runs.empty() && runs.back().first + runs.back().second == segs[i].offset) runs.back().second += segs[i].size;
      else runs.push_back({segs[i].offset, segs[i].size});
      total += segs[i].size;
    }
    const float* src = params + runs[0].first;
    if (runs.size() > 1) {
      if ((rc = ws_alloc(h, x.stage, total))) return rc;
      int64_t at = 0;
      for (const auto& r : runs) {
        RC_HIP(h, hipMemcpyAsync(x.stage.p + at, params + r.first, (size_t)r.second * sizeof(float), hipMemcpyDeviceToDevice, st));
        at += r.second;
      }
      src = x.stage.p;
    }
    const size_t bytes = (size_t)total * sizeof(float);
    if (h->pinned_bytes < bytes) {
      if (h->pinned) RC_HIP(h, hipHostFree(h->pinned));
      h->pinned = nullptr; h->pinned_bytes = 0;
      RC_HIP(h, hipHostMalloc((void**)&h->pinned, bytes, hipHostMallocDefault));
      h->pinned_bytes = bytes;
    }
    RC_HIP(h, hipMemcpyAsync(h->pinned, src, bytes, hipMemcpyDeviceToHost, st));
    RC_HIP(h, hipStreamSynchronize(st));
    int64_t at = 0;
    for (size_t i : dense) {
      const GradSeg& s = segs[i];
      const size_t slash = s.name.rfind('/');
      const std::string path = s.name.substr(0, slash), leaf = s.name.substr(slash + 1);
      const auto& io = inv.at(path);
      HostLayer& L = h->layers[path];
      L.in = io.first;
      L.out = io.second;
      std::vector<float>& v = leaf == "kernel" ? L.kernel : L.bias;
      v.assign(h->pinned + at, h->pinned + at + s.size);
      (leaf == "kernel" ? L.have_kernel : L.have_bias) = true;
      at += s.size;
    }
    h->packed_dirty = true;
    ++h->layers_gen;
  }
  drop_graphs(h);   // table pointers / packed fragments are baked into captured kernel arguments
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}
