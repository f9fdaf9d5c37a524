// Host side of the training backward of one level's density field (rc_train.hip); included by rc_api.hip before the other
// training files.  Also what those files share: the gradient-buffer layouts (GradSeg, one builder per layout,
// layout_segments, behind every rc_*_grad_size / rc_*_grad_layout and rc_load_params_flat), the dense layers on k_gemm
// (dense_fwd, dense_dx, dense_wgrad) and on k_gemm_tile (dense_*_tile), the body of the three grid-L2 regularizers and,
// behind rc_density_backward, the chunked tail of the losses that end in it (density_backward_chunks).

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

// The dense layers of the shader layout (pred_normals_layer first, the appearance tables between it and the rest).
enum { DL_PRED, DL_BOTT, DL_ROUGH, DL_AMB, DL_TINT, DL_IRR, DL_I0, DL_I1, DL_IO, DL_S0, DL_S1, DL_S2, DL_SB, DL_SO, DL_COUNT };
struct DataLayer { const char* name; int in, out; };
constexpr DataLayer kDataLayers[DL_COUNT] = {
    {"pred_normals_layer", 64, 3},           {"bottleneck_layer", 96, 128},     {"roughness_layer", 96, 1},
    {"ambient_irradiance_layer", 96, 3},     {"tint_layer", 96, 3},             {"irradiance_layer", 96, 3},
    {"integrated_brdf_layers_0", 129, 64},   {"integrated_brdf_layers_1", 64, 64}, {"output_integrated_brdf_layer", 64, 1},
    {"SurfaceLightField/layer_0", 200, 128}, {"SurfaceLightField/layer_1", 128, 128}, {"SurfaceLightField/layer_2", 128, 128},
    {"SurfaceLightField/layer_bottleneck", 328, 128}, {"SurfaceLightField/output_ambient_rgb_layer", 128, 3}};

std::string data_layer_path(rc_handle* h, int i) {
  return i == DL_PRED ? "params/Cache/Sampler/MLP_" + std::to_string(h->cfg.num_levels - 1) + "/pred_normals_layer"
                      : std::string("params/Cache/Shader/") + kDataLayers[i].name;
}

// Segments of the shader gradient buffer; kernel_seg[i] = index of layer i's kernel segment (its bias follows).
std::vector<GradSeg> shader_grad_segments(rc_handle* h, int* kernel_seg = nullptr, int64_t* app_off = nullptr) {
  std::vector<GradSeg> v;
  int64_t off = 0;
  for (int i = 0; i < DL_COUNT; ++i) {
    if (i == DL_BOTT) {
      if (app_off) *app_off = off;
      for (const GradSeg& g : grid_grad_segments(h->grids[3], off)) v.push_back(g);
    }
    if (kernel_seg) kernel_seg[i] = (int)v.size();
    dense_grad_segments(v, off, data_layer_path(h, i), kDataLayers[i].in, kDataLayers[i].out);
  }
  return v;
}

constexpr int kLightGrid = 5;                  // the handle's grid id of params/LightSampler/light_grid
constexpr int kLightWidth = 32;                // the light head's input: the light grid's features (RcLightHeadArgs)
constexpr int kMaterialGrid = 4;               // the handle's grid id of params/MaterialShader/material_grid
constexpr int kMaterialWidth = 32;             // the material head's input: the material grid's features (RcMatHeadArgs)

// params/LightSampler: light_grid tables in level order, then layers_0, layers_1, output_layer (kernel, bias each)
std::vector<GradSeg> light_grad_segments(rc_handle* h) {
  const GridState& gs = h->grids[kLightGrid];
  int64_t off = 0;
  std::vector<GradSeg> v = grid_grad_segments(gs, off);
  dense_grad_segments(v, off, "params/LightSampler/layers_0", (int)gs.sizes.size() * gs.cfg.num_features, 64);
  dense_grad_segments(v, off, "params/LightSampler/layers_1", 64, 64);
  dense_grad_segments(v, off, "params/LightSampler/output_layer", 64, 5 * h->cfg.num_vmf);
  return v;
}

// params/MaterialShader: material_grid tables in level order, then bottleneck_layer, pred_brdf_layer (kernel, bias each)
std::vector<GradSeg> material_grad_segments(rc_handle* h) {
  const GridState& gs = h->grids[kMaterialGrid];
  int64_t off = 0;
  std::vector<GradSeg> v = grid_grad_segments(gs, off);
  const auto inv = dense_inventory(h->cfg, nullptr);
  const auto& bott = inv.at("params/MaterialShader/bottleneck_layer");
  dense_grad_segments(v, off, "params/MaterialShader/bottleneck_layer", bott.first, bott.second);
  dense_grad_segments(v, off, "params/MaterialShader/pred_brdf_layer", bott.second, 10);
  return v;
}

// params/Cache/EnvMap, the layers the model-level path reads (output_ambient_rgb_layer is not one of them): layer_0,
// layer_1, layer_2, layer_bottleneck, output_rgba_layer (kernel, bias each)
constexpr const char* kEnvLayers[5] = {"layer_0", "layer_1", "layer_2", "layer_bottleneck", "output_rgba_layer"};
std::vector<GradSeg> envmap_grad_segments(rc_handle* h) {
  const auto inv = dense_inventory(h->cfg, nullptr);
  std::vector<GradSeg> v;
  int64_t off = 0;
  for (const char* l : kEnvLayers) {
    const std::string path = std::string("params/Cache/EnvMap/") + l;
    const auto& io = inv.at(path);
    dense_grad_segments(v, off, path, io.first, io.second);
  }
  return v;
}

// The two per-bin head layers of the time-resolved cache (rc_transient_data_backward): transient_indirect_layer
// [64, 3 n_bins], SurfaceLightField/output_rgba_layer [128, 3 n_bins + 1] (kernel, bias each)
std::vector<GradSeg> transient_head_segments(rc_handle* h) {
  const auto inv = dense_inventory(h->cfg, &h->tcfg);
  std::vector<GradSeg> v;
  int64_t off = 0;
  for (const char* l : {"transient_indirect_layer", "SurfaceLightField/output_rgba_layer"}) {
    const std::string path = std::string("params/Cache/Shader/") + l;
    const auto& io = inv.at(path);
    dense_grad_segments(v, off, path, io.first, io.second);
  }
  return v;
}

// The sampler side of the time-resolved cache in one buffer (rc_transient_*_backward): the segments of
// density_grad_segments(0), (1), ... in their order, then MLP_<last>/pred_normals_layer [64, 3] (kernel, bias).
// level_off[l]: where level l's segments start; *pred_seg: the index of pred_normals_layer's kernel segment.
std::vector<GradSeg> transient_sampler_segments(rc_handle* h, int64_t* level_off = nullptr, int* pred_seg = nullptr) {
  std::vector<GradSeg> v;
  int64_t off = 0;
  for (int l = 0; l < h->cfg.num_levels; ++l) {
    if (level_off) level_off[l] = off;
    const std::vector<GradSeg> lv = density_grad_segments(h, l);
    for (GradSeg g : lv) { g.offset += off; v.push_back(g); }
    off += grad_size(lv);
  }
  if (pred_seg) *pred_seg = (int)v.size();
  dense_grad_segments(v, off, data_layer_path(h, DL_PRED), kDataLayers[DL_PRED].in, kDataLayers[DL_PRED].out);
  return v;
}

// Layout ids of the ABI: a density level >= 0, RC_LAYOUT_SHADER, RC_LAYOUT_LIGHT, RC_LAYOUT_MATERIAL, RC_LAYOUT_ENVMAP,
// RC_LAYOUT_TRANSIENT_HEADS, RC_LAYOUT_TRANSIENT_SAMPLER.  `who`'s check that
// the handle has the layout (a density export maps a negative level to kNoLayout, so that it names no other layout).
constexpr int kNoLayout = INT32_MIN;
int layout_check(rc_handle* h, int layout, const std::string& who) {
  if (layout == RC_LAYOUT_SHADER) {
    if (h->transient) return fail(h, RC_ERR_UNSUPPORTED, who + ": not available on a time-resolved cache handle");
  } else if (layout == RC_LAYOUT_LIGHT) {
    if (h->grids[kLightGrid].sizes.empty()) return fail(h, RC_ERR_UNSUPPORTED, who + ": no light grid");
  } else if (layout == RC_LAYOUT_MATERIAL) {
    if (h->grids[kMaterialGrid].sizes.empty()) return fail(h, RC_ERR_UNSUPPORTED, who + ": no material grid");
  } else if (layout == RC_LAYOUT_ENVMAP) {
    if (h->transient) return fail(h, RC_ERR_UNSUPPORTED, who + ": not available on a time-resolved cache handle");
  } else if (layout == RC_LAYOUT_TRANSIENT_HEADS || layout == RC_LAYOUT_TRANSIENT_SAMPLER) {
    if (!h->transient) return fail(h, RC_ERR_UNSUPPORTED, who + ": needs a time-resolved cache handle (rc_set_transient)");
  } else if (layout < 0 || layout >= h->cfg.num_levels) {
    return fail(h, RC_ERR_INVALID_ARG, who + ": bad level");
  }
  return RC_OK;
}

// the segments of a layout that passed layout_check
std::vector<GradSeg> layout_segments(rc_handle* h, int layout) {
  switch (layout) {
    case RC_LAYOUT_SHADER: return shader_grad_segments(h);
    case RC_LAYOUT_LIGHT: return light_grad_segments(h);
    case RC_LAYOUT_MATERIAL: return material_grad_segments(h);
    case RC_LAYOUT_ENVMAP: return envmap_grad_segments(h);
    case RC_LAYOUT_TRANSIENT_HEADS: return transient_head_segments(h);
    case RC_LAYOUT_TRANSIENT_SAMPLER: return transient_sampler_segments(h);
    default: return density_grad_segments(h, layout);
  }
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

// The bodies of rc_*_grad_size and rc_*_grad_layout.
int64_t layout_grad_size(rc_handle* h, int layout, const char* who) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  int rc;
  if ((rc = layout_check(h, layout, who))) return rc;
  return grad_size(layout_segments(h, layout));
  RC_CATCH(h)
}

int layout_grad_layout(rc_handle* h, int layout, rc_grad_segment* segs, int32_t capacity, int32_t* count, const char* who) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  // rc_shader_grad_layout checks `count` before the handle's kind, the others after it (copy_segments)
  if (layout == RC_LAYOUT_SHADER && !count) return fail(h, RC_ERR_INVALID_ARG, std::string(who) + ": null count");
  int rc;
  if ((rc = layout_check(h, layout, who))) return rc;
  return copy_segments(h, layout_segments(h, layout), segs, capacity, count, who);
  RC_CATCH(h)
}

// Dense layers on k_gemm, M rows (points or samples) each; X, Y, dX, dY row-major with row strides ld*.
constexpr int64_t kDataChunk = 32768;      // samples per chunk of a shader backward (bounds its workspace)
constexpr int64_t kDataKSlice = 1024;      // rows per K slice of a weight gradient

struct Dense { int in, out; const float* w; const float* b; };    // kernel [in, out], bias [out]

// Y = X W + b, ReLU'd when `relu`
void dense_fwd(const Dense& L, int64_t M, const float* X, int64_t ldx, float* Y, int64_t ldy, bool relu, hipStream_t st) {
  RcGemmArgs g{};
  g.M = (int)M; g.N = L.out; g.K = L.in;
  g.a = X; g.sai = ldx; g.sak = 1; g.b = L.w; g.sbk = L.out; g.sbj = 1;
  g.c = Y; g.sci = ldy; g.scj = 1; g.bias = L.b; g.relu = relu ? 1 : 0; g.kslice = g.K;
  rc_launch_gemm(g, 1, st);
}

// dX[:, j0 .. j0 + nj) (+)= dY W^T, zero where mask <= 0 (the forward's ReLU output, row stride ldx like dX)
void dense_dx(const Dense& L, int64_t M, const float* dY, int64_t ldy, float* dX, int64_t ldx, int j0, int nj, const float* mask,
              bool accumulate, hipStream_t st) {
  RcGemmArgs g{};
  g.M = (int)M; g.N = nj; g.K = L.out;
  g.a = dY; g.sai = ldy; g.sak = 1; g.b = L.w + (int64_t)j0 * L.out; g.sbk = 1; g.sbj = L.out;
  g.c = dX + j0; g.sci = ldx; g.scj = 1; g.mask = mask ? mask + j0 : nullptr; g.smi = ldx; g.smj = 1;
  g.accumulate = accumulate ? 1 : 0; g.kslice = g.K;
  rc_launch_gemm(g, 1, st);
}

// grads[kb[0]] += X^T dY, grads[kb[1]] += column sums of dY (kb: the layer's kernel segment, its bias segment after it):
// K = the M rows in fixed slices of kDataKSlice, their partials in `part` added up by k_sum_parts in slice order; `ones`:
// a 1.0f, the A operand of the bias pass
void dense_wgrad(const Dense& L, int64_t M, const float* X, int64_t ldx, const float* dY, int64_t ldy, const float* ones,
                 float* part, float* grads, const GradSeg* kb, hipStream_t st) {
  const int64_t Z = (M + kDataKSlice - 1) / kDataKSlice;
  for (int pass = 0; pass < 2; ++pass) {
    RcGemmArgs g{};
    g.M = pass == 0 ? L.in : 1; g.N = L.out; g.K = M;
    g.a = pass == 0 ? X : ones; g.sai = pass == 0 ? 1 : 0; g.sak = pass == 0 ? ldx : 0;
    g.b = dY; g.sbk = ldy; g.sbj = 1; g.c = part; g.sci = L.out; g.scj = 1;
    g.kslice = kDataKSlice; g.spart = (int64_t)g.M * L.out;
    rc_launch_gemm(g, (int)Z, st);
    rc_launch_sum_parts(part, (int)Z, g.spart, grads + kb[pass].offset, st);
  }
}

// The same three on k_gemm_tile (rc_envmap_bwd.hip), same arguments and results up to the order of the sums over k.
void dense_fwd_tile(const Dense& L, int64_t M, const float* X, int64_t ldx, float* Y, int64_t ldy, bool relu, hipStream_t st) {
  RcGemmArgs g{};
  g.M = (int)M; g.N = L.out; g.K = L.in;
  g.a = X; g.sai = ldx; g.sak = 1; g.b = L.w; g.sbk = L.out; g.sbj = 1;
  g.c = Y; g.sci = ldy; g.scj = 1; g.bias = L.b; g.relu = relu ? 1 : 0; g.kslice = g.K;
  rc_launch_gemm_tile(g, 1, st);
}

void dense_dx_tile(const Dense& L, int64_t M, const float* dY, int64_t ldy, float* dX, int64_t ldx, int j0, int nj,
                   const float* mask, bool accumulate, hipStream_t st) {
  RcGemmArgs g{};
  g.M = (int)M; g.N = nj; g.K = L.out;
  g.a = dY; g.sai = ldy; g.sak = 1; g.b = L.w + (int64_t)j0 * L.out; g.sbk = 1; g.sbj = L.out;
  g.c = dX + j0; g.sci = ldx; g.scj = 1; g.mask = mask ? mask + j0 : nullptr; g.smi = ldx; g.smj = 1;
  g.accumulate = accumulate ? 1 : 0; g.kslice = g.K;
  rc_launch_gemm_tile(g, 1, st);
}

void dense_wgrad_tile(const Dense& L, int64_t M, const float* X, int64_t ldx, const float* dY, int64_t ldy, const float* ones,
                      float* part, float* grads, const GradSeg* kb, hipStream_t st) {
  const int64_t Z = (M + kDataKSlice - 1) / kDataKSlice;
  for (int pass = 0; pass < 2; ++pass) {
    RcGemmArgs g{};
    g.M = pass == 0 ? L.in : 1; g.N = L.out; g.K = M;
    g.a = pass == 0 ? X : ones; g.sai = pass == 0 ? 1 : 0; g.sak = pass == 0 ? ldx : 0;
    g.b = dY; g.sbk = ldy; g.sbj = 1; g.c = part; g.sci = L.out; g.scj = 1;
    g.kslice = kDataKSlice; g.spart = (int64_t)g.M * L.out;
    rc_launch_gemm_tile(g, (int)Z, st);
    rc_launch_sum_parts(part, (int)Z, g.spart, grads + kb[pass].offset, st);
  }
}

// rc_{density,light,material}_regularizer after the export's own checks: mult * sum over the tables of grid `grid` of
// 0.5 * mean(x^2) into `loss`, and mult * x / numel added into the layout `grads` (whose head is the grid's tables), on
// the workspace set `set` (X: its extra buffers, reg_part the per-table partial sums).
// `allow_transient`: rc_transient_density_regularizer (every other caller refuses a time-resolved handle).
template <class X>
int grid_l2_regularizer(rc_handle* h, int grid, int set, float mult, float* grads, float* loss, void* stream_v, const std::string& who,
                        bool allow_transient = false) {
  if (!std::isfinite(mult)) return fail(h, RC_ERR_INVALID_ARG, who + ": mult must be finite");
  if (!loss) return fail(h, RC_ERR_INVALID_ARG, who + ": null loss");
  if (h->transient && !allow_transient) return fail(h, RC_ERR_UNSUPPORTED, who + ": not available on a time-resolved cache handle");
  const GridState& gs = h->grids[grid];
  const int T = (int)gs.sizes.size();
  if (T < 1 || T > RC_MAX_GRID_LEVELS) return fail(h, RC_ERR_UNSUPPORTED, who + ": unexpected grid levels");
  for (int t = 0; t < T; ++t)
    if (!gs.loaded[t]) return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: " + gs.prefix + "/" + level_name(gs.cfg, gs.sizes, gs.sizes[t]));
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  WsUse use(h, set, st);
  int rc;
  if ((rc = use.rc)) return rc;
  X& y = ws_extra<X>(use.s);
  const int B = rc_grid_l2_blocks();
  if ((rc = ws_alloc(h, y.reg_part, 2 * (int64_t)T * B))) return rc;     // doubles
  double* part = reinterpret_cast<double*>(y.reg_part.p);
  int64_t off = 0;
  const std::vector<GradSeg> segs = grid_grad_segments(gs, off);
  RcGridL2Reduce rr{};
  rr.mult = mult; rr.tables = T;
  for (int t = 0; t < T; ++t) {
    const int64_t count = segs[t].size;
    rr.count[t] = count;
    rc_launch_grid_l2_bwd(gs.dev.lvl[t].table, count, (float)((double)mult / (double)count),
                          grads ? grads + segs[t].offset : nullptr, part + (int64_t)t * B, st);
  }
  rc_launch_grid_l2_reduce(part, rr, loss, st);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
}

// Stream of k_density_bwd: the forward fragments of every level followed by W1^T, W0^T.  `replay`: the floats of the two
// forward layers, appended once more by the caller that runs them again (rc_normals_backward).
int build_train_stream(rc_handle* h, int level, std::vector<float>& stream, size_t* replay = nullptr) {
  std::string missing;
  const std::string base = "params/Cache/Sampler/MLP_" + std::to_string(level);
  const HostLayer* d0 = need(h, base + "/density_layers_0", missing);
  const HostLayer* d1 = need(h, base + "/density_layers_1", missing);
  const HostLayer* dout = need(h, base + "/output_density_layer", missing);
  if (!missing.empty()) return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: " + missing);
  std::vector<Step> s;
  steps_natural(s, d0->in, 0); step_bias(s);
  stream = pack_f32(s, {tile_full(d0, 0), tile_full(d0, 1)});
  s.clear(); steps_acc(s, 2, 0); step_bias(s);
  append(stream, pack_f32(s, {tile_full(d1, 0), tile_full(d1, 1)}));
  if (replay) *replay = stream.size();
  append(stream, pack_dot({Col{dout, 0}}, 2, false));
  HostLayer w1t, w0t;
  w1t.in = d1->out; w1t.out = d1->in; w1t.kernel.resize(d1->kernel.size()); w1t.bias.assign(w1t.out, 0.0f);
  for (int r = 0; r < d1->in; ++r) for (int c2 = 0; c2 < d1->out; ++c2) w1t.kernel[(size_t)c2 * w1t.out + r] = d1->kernel[(size_t)r * d1->out + c2];
  w0t.in = d0->out; w0t.out = d0->in; w0t.kernel.resize(d0->kernel.size()); w0t.bias.assign(w0t.out, 0.0f);
  for (int r = 0; r < d0->in; ++r) for (int c2 = 0; c2 < d0->out; ++c2) w0t.kernel[(size_t)c2 * w0t.out + r] = d0->kernel[(size_t)r * d0->out + c2];
  std::vector<Step> sb; steps_acc(sb, 2, 0);
  append(stream, pack_f32(sb, {tile_full(&w1t, 0, 0, false), tile_full(&w1t, 1, 0, false)}));
  append(stream, pack_f32(sb, {tile_full(&w0t, 0, 0, false)}));
  return RC_OK;
}

int pack_train_stream(rc_handle* h, int level) {
  std::vector<float> stream;
  if (int rc = build_train_stream(h, level, stream)) return rc;
  return upload(h, h->packs.train[level], pad_stream(stream));
}

}  // namespace

int64_t rc_density_grad_size(rc_handle* h, int32_t level) {
  return layout_grad_size(h, level < 0 ? kNoLayout : level, "rc_density_grad_size");
}
int64_t rc_shader_grad_size(rc_handle* h) { return layout_grad_size(h, RC_LAYOUT_SHADER, "rc_shader_grad_size"); }
int64_t rc_light_grad_size(rc_handle* h) { return layout_grad_size(h, RC_LAYOUT_LIGHT, "rc_light_grad_size"); }
int64_t rc_material_grad_size(rc_handle* h) { return layout_grad_size(h, RC_LAYOUT_MATERIAL, "rc_material_grad_size"); }
int64_t rc_envmap_grad_size(rc_handle* h) { return layout_grad_size(h, RC_LAYOUT_ENVMAP, "rc_envmap_grad_size"); }

int64_t rc_transient_head_grad_size(rc_handle* h) {
  return layout_grad_size(h, RC_LAYOUT_TRANSIENT_HEADS, "rc_transient_head_grad_size");
}
int rc_transient_head_grad_layout(rc_handle* h, rc_grad_segment* segs, int32_t capacity, int32_t* count) {
  return layout_grad_layout(h, RC_LAYOUT_TRANSIENT_HEADS, segs, capacity, count, "rc_transient_head_grad_layout");
}
int64_t rc_transient_sampler_grad_size(rc_handle* h) {
  return layout_grad_size(h, RC_LAYOUT_TRANSIENT_SAMPLER, "rc_transient_sampler_grad_size");
}
int rc_transient_sampler_grad_layout(rc_handle* h, rc_grad_segment* segs, int32_t capacity, int32_t* count) {
  return layout_grad_layout(h, RC_LAYOUT_TRANSIENT_SAMPLER, segs, capacity, count, "rc_transient_sampler_grad_layout");
}

int rc_density_grad_layout(rc_handle* h, int32_t level, rc_grad_segment* segs, int32_t capacity, int32_t* count) {
  return layout_grad_layout(h, level < 0 ? kNoLayout : level, segs, capacity, count, "rc_density_grad_layout");
}
int rc_shader_grad_layout(rc_handle* h, rc_grad_segment* segs, int32_t capacity, int32_t* count) {
  return layout_grad_layout(h, RC_LAYOUT_SHADER, segs, capacity, count, "rc_shader_grad_layout");
}
int rc_light_grad_layout(rc_handle* h, rc_grad_segment* segs, int32_t capacity, int32_t* count) {
  return layout_grad_layout(h, RC_LAYOUT_LIGHT, segs, capacity, count, "rc_light_grad_layout");
}
int rc_material_grad_layout(rc_handle* h, rc_grad_segment* segs, int32_t capacity, int32_t* count) {
  return layout_grad_layout(h, RC_LAYOUT_MATERIAL, segs, capacity, count, "rc_material_grad_layout");
}

int rc_envmap_grad_layout(rc_handle* h, rc_grad_segment* segs, int32_t capacity, int32_t* count) {
  return layout_grad_layout(h, RC_LAYOUT_ENVMAP, segs, capacity, count, "rc_envmap_grad_layout");
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

namespace {

// The tail of a per-ray loss whose gradient reaches level `level` through d loss / d density alone (and d loss / d feature64
// where d_feature is given): the forward's sample means (SoA [3][np]) copied into `points` as rows [np][3], then
// rc_density_backward at them in chunks of kDataChunk samples.
int density_backward_chunks(rc_handle* h, int level, const float* means_soa, int64_t np, WsBuf& points, const float* d_density,
                            const float* d_feature, float* grads, hipStream_t st) {
  if (int rc = ws_alloc(h, points, 3 * np)) return rc;
  rc_launch_points_aos(means_soa, np, points.p, st);
  RC_HIP(h, hipGetLastError());
  for (int64_t c0 = 0; c0 < np; c0 += kDataChunk) {
    const int64_t C = np - c0 < kDataChunk ? np - c0 : kDataChunk;
    if (int rc = rc_density_backward(h, level, points.p + 3 * c0, C, d_density + c0, d_feature ? d_feature + 64 * c0 : nullptr, grads,
                                     nullptr, st))
      return rc;
  }
  RC_HIP(h, hipGetLastError());
  return RC_OK;
}

}  // namespace

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
