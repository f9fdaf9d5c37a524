// C-ABI host of the radiance-cache renderer (see include/rc_abi.h).
//
// Owns: the handle, device copies of the hash/dense tables, the MFMA-fragment-packed MLP weights,
// the per-batch workspace (its sets and buffer names: rc_ws.h) and the small entry points.  The launch sequence that replaces
// BaseNeRFModel.__call__ is rc_render_host.inc, the material stage rc_material_host.inc; like
// every other *_host.inc they are included at the end of this file.
#include <dlfcn.h>
#include <math.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <array>
#include <map>
#include <memory>
#include <string>
#include <variant>
#include <vector>

#include "rc_internal.h"
#include "rc_pack_host.h"
#include "rc_itof_host.h"
#include "rc_ws.h"
#include "rc_prng_host.h"     // rc_round_half_even: the split of K, as the randoms plan sizes its members

void rc_launch_hashgrid_src(const RcGridDev& g, const float* points, int soa_in, const int32_t* src, int64_t n_src,
                            int64_t n, float* out, int feature_major, int64_t ldo, float contract_radius,
                            float* jac_out, hipStream_t stream);
int rc_shader_lds_bytes();
int rc_weight_chunk_floats();
void rc_shader_prepare();

using namespace rcpack;

namespace {

thread_local std::string g_create_error;

enum Stage {
  ST_SAMPLE0 = 0, ST_GRID0, ST_MLP0, ST_SAMPLE1, ST_GRID1, ST_MLP1, ST_SAMPLE2, ST_GRID2, ST_MLP2,
  ST_RESAMPLE, ST_GRID_APP, ST_SHADER, ST_COMPOSITE, ST_COUNT
};
const char* kStageNames[ST_COUNT] = {"sample0", "grid0", "mlp0", "sample1", "grid1", "mlp1", "sample2",
                                     "grid2", "mlp2", "resample", "grid_app", "shader", "composite"};

struct DevBuf {
  float* p = nullptr;
  size_t bytes = 0;
};

// Device copies of the packed weights and of the derived tables (repack).
enum RawLayer { RAW_MAT_BOTTLENECK, RAW_MAT_BRDF, RAW_LIGHT_0, RAW_LIGHT_1, RAW_LIGHT_OUT, RAW_COUNT };
const char* const kRawPaths[RAW_COUNT] = {"params/MaterialShader/bottleneck_layer", "params/MaterialShader/pred_brdf_layer",
                                          "params/LightSampler/layers_0", "params/LightSampler/layers_1",
                                          "params/LightSampler/output_layer"};
struct Packs {
  DevBuf dens[RC_MAX_LEVELS], train[RC_MAX_LEVELS];
  DevBuf nbwd;                           // rc_normals_backward: the last level's training stream + the two replayed forward layers
  DevBuf shader, fused, fused_front, envmap, t_shader, t_bins, t_taps;
  DevBuf t_slice_slf, t_slice_irr;       // k_transient_slice: the two per-bin heads as plain columns (repack_transient)
  DevBuf pair[RC_MAX_GRID_LEVELS];       // level-2 density + appearance tables interleaved (cell tables on dense levels)
  DevBuf cell[2][RC_MAX_GRID_LEVELS];    // dense levels of proposal grids 0 / 1 as cell tables
  DevBuf rec[3][RC_MAX_GRID_LEVELS];     // hashed levels of grids 0-2 as cell records (kLevelHRec)
  struct { DevBuf kernel, bias; } raw[RAW_COUNT];   // material / light-sampler layers on the Flax layout
};

// A workspace set (rc_ws.h: its buffers, the registry of their names) and who used it last: a call whose stream differs
// from the previous user's first waits for that user's last call (event), so two streams never run on one set at the same
// time (WsUse).
struct WsSet : WsBufs {
  hipStream_t stream = nullptr;
  bool used = false;
  hipEvent_t done = nullptr;
  uint64_t last_use = 0;
};
// The extra buffers of a set, of the kind its entry point uses (fixed by that entry point's first call).
template <class X> X& ws_extra(WsSet& s) {
  if (X* p = std::get_if<X>(&s.x)) return *p;
  return s.x.template emplace<X>();
}

constexpr int kEvSlots = 16;

// Everything that is baked into the kernel arguments of one rc_render_rays call.
struct RenderKey {
  int64_t n; uint32_t mask; int slot; int ws_slot;
  const void* rays[7]; const void* rnd[RC_MAX_LEVELS + 2]; const void* out[RC_OUT_COUNT];
  bool operator==(const RenderKey& o) const { return memcmp(this, &o, sizeof(RenderKey)) == 0; }
};
struct GraphEntry {
  RenderKey key;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
};

struct GridState {
  rc_grid_config cfg{};
  std::string prefix;
  std::vector<int> sizes;
  std::vector<DevBuf> tables;
  std::vector<bool> loaded;
  RcGridDev dev{};
};

}  // namespace

struct rc_handle {
  rc_config cfg{};
  int device = 0;
  std::string err;
  GridState grids[6];
  std::map<std::string, HostLayer> layers;   // key: path without /kernel|/bias
  bool packed_dirty = true;
  uint64_t layers_gen = 1;                   // bumped whenever a dense layer is (re)loaded
  uint64_t train_gen[RC_MAX_LEVELS] = {};    // layers_gen the training stream of a level was packed at
  uint64_t data_gen = 0;                     // layers_gen data_w was uploaded at
  DevBuf data_w;                             // rc_data_backward: the shader's dense layers on the Flax layout
  uint64_t nbwd_gen = 0;                     // layers_gen packs.nbwd was packed at
  uint64_t geom_gen = 0;                     // layers_gen geom_w was uploaded at
  DevBuf geom_w;                             // rc_geometry_backward: pred_normals_layer kernel [64][3] + bias [3]
  uint64_t diffuse_gen = 0;                  // layers_gen diffuse_w was uploaded at
  DevBuf diffuse_w;                          // rc_query_cache_diffuse: ambient_irradiance_layer and irradiance_layer on the Flax layout
  uint64_t env_gen = 0;                      // layers_gen env_w was uploaded at
  DevBuf env_w;                              // rc_material_data_backward_env: the EnvMap's dense layers on the Flax layout
  uint64_t thead_gen = 0;                    // layers_gen thead_w was uploaded at
  DevBuf thead_w;                            // rc_transient_data_backward: the two per-bin head layers on the Flax layout
  DevBuf itof_w;                             // rc_transient_data_backward_kind, rc_dtof_to_itof: the modulation table (rc_itof_host.h)
  std::vector<double> itof_key;              // what itof_w was built from: exposure_time, then the (frequency, phase) pairs
  float* pinned = nullptr;                   // rc_load_params_flat: page-locked landing buffer of the dense segments
  size_t pinned_bytes = 0;
  bool have_envmap = false;
  bool have_material = false;
  // packed MFMA fragments (device)
  Packs packs;
  DevBuf ide_table;
  WsSet ws[WS_COUNT];                        // workspace sets (WsSetId)
  uint64_t use_clock = 0;
  // profiling: ring of event sets, one set per render call (slot = call % kEvSlots)
  // mode 0 off, 1 every stage, 2 only the dominant kernel (cache shader), 3 like 2 on every 8th call
  int profiling = 0;
  hipEvent_t ev[kEvSlots][ST_COUNT + 1]{};
  bool ev_used[kEvSlots]{};
  bool ev_created = false;
  int64_t prof_calls = 0;
  // time-resolved cache (rc_set_transient): TransientNeRFMLP inventory + rc_render_transient
  bool transient = false;
  rc_transient_config tcfg{};
  float light_power = 0.0f;
  bool have_light_power = false;
  int n_taps = 0;
  // fused per-ray kernel for the plain cache pass (fused_mode: 0 never, 1 whenever eligible)
  int fused_mode = 1;
  RcFusedLaunch fused_tmpl{};      // launch descriptor of the fused plan, resolved at repack (build_fused_template)
  int fused_prio = getenv("RC_FUSED_PRIO") ? atoi(getenv("RC_FUSED_PRIO")) : 1;             // rc_fused2.hip: 1 = the younger workgroup of a CU leads through the lookups
  bool fused_ok = false;
  bool fused_front_ok = false;               // transient handles: the FRONT variant of the fused kernel is usable
  // hipGraph replay of the launch sequence (graph_mode: 0 off, 1 capture when a call repeats, 2 always)
  int graph_mode = 1;
  hipStream_t cap_stream = nullptr;
  // rc_render_material: work that the secondary trace does not wait for (material-only composite over all samples,
  // EnvMap along the secondary rays) runs on this stream, forked from / joined to the caller's with events
  float* sec_sbounds = nullptr;            // power-ladder image of the secondary rays' (near, far): constants of the config
  hipStream_t side_stream = nullptr;
  hipEvent_t ev_side[4] = {nullptr, nullptr, nullptr, nullptr};
  // rc_density_backward: the weight gradients beside the table-gradient scatter on the caller's stream (highest priority;
  // events: fork, join)
  hipStream_t train_stream = nullptr;
  hipEvent_t ev_train[2] = {nullptr, nullptr};
  // rc_set_env_image: the handle's own copies of the bound image (zero-padded RGBA, RcEnvImage) and of its tables
  // (pmf, pdf, dirs and safe_log(pmf)); env_img_h == 0: nothing bound
  DevBuf env_padded, env_pmf, env_pdf, env_dirs, env_logp;
  int32_t env_img_h = 0, env_img_w = 0;
  bool env_tables = false;
  std::vector<GraphEntry> graphs;
  RenderKey last_key{};
  bool have_last_key = false;
};

namespace {

#define RC_HIP(h, call)                                                                      \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                          \
      return RC_ERR_HIP;                                                                     \
    }                                                                                        \
  } while (0)

int fail(rc_handle* h, int code, const std::string& msg) {
  h->err = msg;
  return code;
}

// Nothing may propagate out of an extern "C" entry point (include/rc_abi.h): std::bad_alloc / std::length_error of the
// host-side containers end up here and come back as a status code.
int rc_caught(rc_handle* h, const char* what) noexcept {
  try {
    const std::string msg = std::string("exception in the host layer: ") + (what ? what : "unknown");
    if (h) h->err = msg; else g_create_error = msg;
  } catch (...) {
  }
  return RC_ERR_HOST;
}
#define RC_TRY try {
#define RC_CATCH(h)                                                       \
  } catch (const std::exception& e_) { return rc_caught((h), e_.what()); } \
  catch (...) { return rc_caught((h), nullptr); }

std::vector<int> grid_sizes(const rc_grid_config& g) {
  // grid_utils.py:773-794 with scale_supersample = 1
  const int n = 1 + (int)lround(log2((double)g.max_grid_size / g.min_grid_size));
  std::vector<int> s;
  for (int i = 0; i < n; ++i) s.push_back((int)lround(g.min_grid_size * pow(2.0, i)));
  return s;
}
bool is_dense(const rc_grid_config& g, int n) { return (int64_t)n * n * n <= g.hash_map_size; }
std::string level_name(const rc_grid_config& g, const std::vector<int>& sizes, int n) {
  const int width = (int)std::to_string(sizes.back()).size();
  std::string d = std::to_string(n);
  while ((int)d.size() < width) d = "0" + d;
  return std::string(is_dense(g, n) ? "grid_" : "hash_") + d;
}

void init_grid(GridState& gs, const rc_grid_config& cfg, const std::string& prefix) {
  gs.cfg = cfg;
  gs.prefix = prefix;
  gs.sizes = grid_sizes(cfg);
  gs.tables.assign(gs.sizes.size(), DevBuf{});
  gs.loaded.assign(gs.sizes.size(), false);
  memset(&gs.dev, 0, sizeof(gs.dev));
  gs.dev.num_levels = (int)gs.sizes.size();
  gs.dev.num_features = cfg.num_features;
  gs.dev.bbox = cfg.bbox;
  gs.dev.precondition = cfg.precondition_scaling;
  for (size_t l = 0; l < gs.sizes.size(); ++l) {
    const int n = gs.sizes[l];
    RcGridLevel& L = gs.dev.lvl[l];
    L.size = n;
    L.dense = is_dense(cfg, n) ? 1 : 0;
    L.entries = L.dense ? (uint32_t)n * n * n : (uint32_t)cfg.hash_map_size;
    const uint32_t t = (uint32_t)cfg.hash_map_size;
    L.mask = (!L.dense && (t & (t - 1)) == 0) ? t - 1 : 0;
  }
}

// The dense layers the cache path reads: path -> (in, out).
std::map<std::string, std::pair<int, int>> dense_inventory(const rc_config& c, const rc_transient_config* tc = nullptr) {
  std::map<std::string, std::pair<int, int>> m;
  const int W = 64, B = 128;
  for (int l = 0; l < c.num_levels; ++l) {
    const std::string base = "params/Cache/Sampler/MLP_" + std::to_string(l);
    const int K = (int)grid_sizes(c.proposal_grids[l]).size() * c.proposal_grids[l].num_features;
    m[base + "/density_layers_0"] = {K, W};
    m[base + "/density_layers_1"] = {W, W};
    m[base + "/output_density_layer"] = {W, 1};
    if (l == c.num_levels - 1) m[base + "/pred_normals_layer"] = {W, 3};
  }
  const std::string sh = "params/Cache/Shader";
  const int feat = W + (int)grid_sizes(c.appearance_grid).size() * c.appearance_grid.num_features;
  if (tc) {
    // TransientNeRFMLP + TransientSurfaceLightFieldMLP (nerf.py:232-414, surface_light_field.py:343-403):
    // pos_enc degree 2 for lights and BRDF dots (15 values), IDE degree 5 (72 values)
    m[sh + "/bottleneck_layer"] = {feat, B};
    m[sh + "/roughness_layer"] = {feat, 1};
    m[sh + "/tint_layer"] = {feat, 3};
    m[sh + "/direct_tint_layer"] = {feat, 3};
    m[sh + "/albedo_layer"] = {feat, 3};
    m[sh + "/integrated_brdf_layers_0"] = {B + 1, 64};
    m[sh + "/integrated_brdf_layers_1"] = {64, 64};
    m[sh + "/output_integrated_brdf_layer"] = {64, 1};
    m[sh + "/brdf_layers_0"] = {B + 15, 64};
    m[sh + "/brdf_layers_1"] = {64, 64};
    m[sh + "/output_brdf_layer"] = {64, 1};
    m[sh + "/irradiance_layers_0"] = {feat + 15, 64};
    m[sh + "/irradiance_layers_1"] = {64, 64};
    m[sh + "/transient_indirect_layer"] = {64, 3 * tc->n_bins};
    const std::string sl = sh + "/SurfaceLightField";
    const int in = B + 72 + 15;
    m[sl + "/layer_0"] = {in, 128};
    m[sl + "/layer_1"] = {128, 128};
    m[sl + "/layer_2"] = {128, 128};
    m[sl + "/layer_bottleneck"] = {128 + in, 128};
    m[sl + "/output_rgba_layer"] = {128, 3 * tc->n_bins + 1};
    return m;
  }
  m[sh + "/bottleneck_layer"] = {feat, B};
  m[sh + "/roughness_layer"] = {feat, 1};
  m[sh + "/tint_layer"] = {feat, 3};
  m[sh + "/ambient_irradiance_layer"] = {feat, 3};
  m[sh + "/irradiance_layer"] = {feat, 3};
  m[sh + "/integrated_brdf_layers_0"] = {B + 1, 64};
  m[sh + "/integrated_brdf_layers_1"] = {64, 64};
  m[sh + "/output_integrated_brdf_layer"] = {64, 1};
  auto slf = [&](const std::string& p, int in, int w, int bott) {
    m[p + "/layer_0"] = {in, w};
    m[p + "/layer_1"] = {w, w};
    m[p + "/layer_2"] = {w, w};
    m[p + "/layer_bottleneck"] = {w + in, bott};
    m[p + "/output_rgba_layer"] = {bott, 4};
    m[p + "/output_ambient_rgb_layer"] = {bott, 3};
  };
  slf(sh + "/SurfaceLightField", B + 72, 128, 128);
  slf(sh + "/EnvMap", 38, 128, 128);          // dead work in the reference; accepted, never read
  slf("params/Cache/EnvMap", 27, 256, 128);
  // material / light stages (accepted so that one checkpoint loads; used by later passes)
  m["params/MaterialShader/bottleneck_layer"] = {32, B};
  m["params/MaterialShader/pred_brdf_layer"] = {B, 10};
  m["params/LightSampler/layers_0"] = {32, 64};
  m["params/LightSampler/layers_1"] = {64, 64};
  m["params/LightSampler/output_layer"] = {64, 640};
  return m;
}

void append(std::vector<float>& dst, const std::vector<float>& v) { dst.insert(dst.end(), v.begin(), v.end()); }
// The kernels pull the stream in whole chunks: pad with zero fragments.
std::vector<float> pad_stream(std::vector<float> v) {
  const size_t c = (size_t)rc_weight_chunk_floats();
  v.resize((v.size() + c - 1) / c * c, 0.0f);
  return v;
}

// (Re)allocate a pack to exactly `floats` elements.
int pack_alloc(rc_handle* h, DevBuf& b, size_t floats) {
  if (b.bytes != floats * sizeof(float)) {
    if (b.p) RC_HIP(h, hipFree(b.p));
    b = DevBuf{};
    RC_HIP(h, hipMalloc((void**)&b.p, floats * sizeof(float)));
    b.bytes = floats * sizeof(float);
  }
  return RC_OK;
}
int upload(rc_handle* h, DevBuf& b, const std::vector<float>& v) {
  if (int rc = pack_alloc(h, b, v.size())) return rc;
  RC_HIP(h, hipMemcpy(b.p, v.data(), b.bytes, hipMemcpyHostToDevice));
  return RC_OK;
}
template <class Buf> void free_buf(Buf& b) { if (b.p) (void)hipFree(b.p); b = Buf{}; }
void free_packs(Packs& P) {
  for (DevBuf* b : {&P.shader, &P.fused, &P.fused_front, &P.envmap, &P.t_shader, &P.t_bins, &P.t_taps, &P.t_slice_slf,
                    &P.t_slice_irr}) free_buf(*b);
  for (int l = 0; l < RC_MAX_LEVELS; ++l) { free_buf(P.dens[l]); free_buf(P.train[l]); }
  free_buf(P.nbwd);
  for (int l = 0; l < RC_MAX_GRID_LEVELS; ++l) {
    free_buf(P.pair[l]);
    for (int g = 0; g < 2; ++g) free_buf(P.cell[g][l]);
    for (int g = 0; g < 3; ++g) free_buf(P.rec[g][l]);
  }
  for (auto& r : P.raw) { free_buf(r.kernel); free_buf(r.bias); }
}

const HostLayer* need(rc_handle* h, const std::string& path, std::string& missing) {
  auto it = h->layers.find(path);
  if (it == h->layers.end() || !it->second.have_kernel || !it->second.have_bias) {
    if (missing.empty()) missing = path;
    return nullptr;
  }
  return &it->second;
}

// Geometry the fused per-ray kernel is written for: 3 proposal levels of 64 / 64 / 32 samples on grids of 6 / 7 / 8
// levels, the level-2 density grid and the appearance grid with identical level geometry, power-of-two hash tables.
bool fused_geometry_ok(rc_handle* h) {
  const rc_config& c = h->cfg;
  bool ok = c.num_levels == 3 && c.num_samples[0] == 64 && c.num_samples[1] == 64 && c.num_samples[2] == 32;
  const int want_lv[4] = {6, 7, 8, 8}, want_f[4] = {1, 1, 4, 4};
  for (int g = 0; g < 4 && ok; ++g)
    ok = h->grids[g].dev.num_levels == want_lv[g] && h->grids[g].dev.num_features == want_f[g];
  // the two half-waves of the last level look up the density / appearance grid with shared level geometry
  ok = ok && h->grids[2].dev.bbox == h->grids[3].dev.bbox && h->grids[2].dev.precondition == h->grids[3].dev.precondition;
  for (int l = 0; l < 8 && ok; ++l) {
    const RcGridLevel &A = h->grids[2].dev.lvl[l], &B = h->grids[3].dev.lvl[l];
    ok = A.dense == B.dense && A.size == B.size && A.mask == B.mask && A.entries == B.entries;
  }
  for (int g = 0; g < 4 && ok; ++g)        // hashed levels: power-of-two tables only (index = hash & mask)
    for (int l = 0; l < h->grids[g].dev.num_levels && ok; ++l)
      ok = h->grids[g].dev.lvl[l].dense || h->grids[g].dev.lvl[l].mask != 0;
  // the kernels are compiled for the reference's level layout (16 ... 2048 cells a side against 2^19 entries): the
  // first kRcFusedDenseLevels levels dense, the others hashed (the kind of a level is a compile-time constant there)
  for (int g = 0; g < 4 && ok; ++g)
    for (int l = 0; l < h->grids[g].dev.num_levels && ok; ++l)
      ok = (h->grids[g].dev.lvl[l].dense != 0) == (l < kRcFusedDenseLevels);
  return ok;
}

// Derived table copies of the fused kernel: interleaved level-2 pairs, cell tables of the dense levels.
int build_fused_tables(rc_handle* h) {
  int rc;
  {
    // level-2 density + appearance tables interleaved entry by entry (same index in both grids): [dens 4 | app 4]
    for (int l = 0; l < h->grids[2].dev.num_levels; ++l) {
      if (h->grids[2].dev.lvl[l].dense) continue;          // dense levels: cell tables below
      const size_t entries = h->grids[2].dev.lvl[l].entries;
      DevBuf& b = h->packs.pair[l];
      if ((rc = pack_alloc(h, b, entries * 8))) return rc;
      RC_HIP(h, hipMemcpy2D(b.p, 32, h->grids[2].dev.lvl[l].table, 16, 16, entries, hipMemcpyDeviceToDevice));
      RC_HIP(h, hipMemcpy2D(b.p + 4, 32, h->grids[3].dev.lvl[l].table, 16, 16, entries, hipMemcpyDeviceToDevice));
    }
    // dense levels as cell tables (the 8 corners of every cell of the zero-padded volume side by side):
    // proposal grids 0 / 1: 8 floats per cell; level-2 pair: 8 x [density 4 | appearance 4] per cell
    for (int g = 0; g < 3; ++g)
      for (int l = 0; l < h->grids[g].dev.num_levels; ++l) {
        const RcGridLevel& L = h->grids[g].dev.lvl[l];
        if (!L.dense) {
          // the first hashed levels of the F = 1 grids as cell records (kLevelHRec): (N + 1)^3 records of 8 floats
          // g == 2: the F = 4 density grid (level kernels' lean pass).  Its records are 2.5 GB per handle: RC_REC4_TABLES=0 in
          // the environment leaves them out (the level kernels test L.rec at run time; the material step is 2.4 % slower)
          static const bool rec4_on = !(getenv("RC_REC4_TABLES") && getenv("RC_REC4_TABLES")[0] == '0');
          const int nrl = g < 2 ? kRcRecLevels : (rec4_on ? kRcRec4Levels : 0);
          if (l < kRcFusedDenseLevels + nrl && L.mask != 0) {
            const int F = h->grids[g].dev.num_features;
            const size_t nrec = (size_t)(L.size + 1) * (L.size + 1) * (L.size + 1);
            if ((rc = pack_alloc(h, h->packs.rec[g][l], nrec * 8 * F))) return rc;
            float* dst = h->packs.rec[g][l].p;
            rc_launch_build_hrec(L.table, L.size, L.mask, F, dst, nullptr);
            h->grids[g].dev.lvl[l].rec = dst;
          }
          continue;
        }
        const size_t ncell = (size_t)(L.size + 3) * (L.size + 3) * (L.size + 3);
        DevBuf& b = g < 2 ? h->packs.cell[g][l] : h->packs.pair[l];      // the level-2 pair: replaces the flat pair table
        if ((rc = pack_alloc(h, b, ncell * (g < 2 ? 8 : 64)))) return rc;
        float* dst = b.p;
        if (g < 2) {
          rc_launch_build_cells(L.table, L.size, 1, dst, 1, 0, nullptr);
          h->grids[g].dev.lvl[l].cell = dst;       // the launch-per-stage gather reads it as well
        } else {
          rc_launch_build_cells(L.table, L.size, 4, dst, 8, 0, nullptr);
          rc_launch_build_cells(h->grids[3].dev.lvl[l].table, L.size, 4, dst, 8, 4, nullptr);
        }
      }
  }
  RC_HIP(h, hipDeviceSynchronize());
  return RC_OK;
}

// What the fused plan and its FRONT variant share: grids, derived tables and the constants of the proposal sampler.
RcFusedLaunch fused_front_end(rc_handle* h) {
  const rc_config& c = h->cfg;
  RcFusedLaunch F{};
  for (int l = 0; l < 3; ++l) F.num_samples[l] = c.num_samples[l];
  for (int g = 0; g < 4; ++g) F.grid[g] = &h->grids[g].dev;
  for (int l = 0; l < h->grids[2].dev.num_levels; ++l) F.pair_table[l] = h->packs.pair[l].p;
  for (int g = 0; g < 2; ++g)
    for (int l = 0; l < h->grids[g].dev.num_levels; ++l)
      F.cell_table[g][l] = h->grids[g].dev.lvl[l].dense ? h->packs.cell[g][l].p
                                                        : h->grids[g].dev.lvl[l].rec;      // cell records of a kLevelHRec level, or NULL
  F.anneal = c.anneal; F.padding = c.resample_padding; F.density_bias = c.density_bias;
  F.contract_radius = c.contract_radius; F.bg = c.bg_intensity;
  return F;
}

// The per-batch launch descriptor of the fused plan with every pointer and constant that only changes with the weights.
void build_fused_template(rc_handle* h) {
  const rc_config& c = h->cfg;
  RcFusedLaunch F = fused_front_end(h);
  F.wstream = h->packs.fused.p; F.ide_coef = h->ide_table.p;
  for (int i = 0; i < 3; ++i) F.pct[i] = c.percentiles[i];
  F.roughness_bias = c.roughness_bias; F.irradiance_bias = c.irradiance_bias; F.ambient_bias = c.ambient_irradiance_bias;
  F.rgb_max = c.rgb_max; F.slf_ambient_bias = c.slf_ambient_bias;
  h->fused_tmpl = F;
}

// The handle's side stream (work that only feeds a call's outputs, forked from / joined to the caller's stream with events)
// at the lowest priority: the kernels on the caller's stream -- the critical path -- get the CUs first.
// Helper streams are per PROCESS and device, created together by the first rc_create and never destroyed: [0] lowest
// priority (the material stage's side work), [1], [2] highest priority ([1]: rc_density_backward; [2]: no user now, still
// created with the others).  Measured on this runtime (ROCm 7.2, profiles/r04_helper_streams.txt): with streams that come
// and go with their handles, whichever multi-stream call ran SECOND in a process was slow -- every kernel of the call
// +50 us or 2-3x, ~100 us of host time between calls: bench.py's train line after its material line 0.20 -> 0.37 ms per
// level-2 call, the other order the material stage 1.39 -> 1.95 ms.  Sharing the streams across handles did not cure it, creating all of them before any work did.
// Handles are driven by one host thread per GPU; every call forks from and joins to the caller's stream with the
// handle's own events, so sharing the streams only orders the helper work of two handles.
hipStream_t rc_helper_stream(int which) {
  static hipStream_t pool[64][3] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  hipStream_t& s = pool[dev & 63][which];
  if (!s) {
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    if (hipStreamCreateWithPriority(&s, hipStreamNonBlocking, which == 0 ? prio_lo : prio_hi) != hipSuccess) s = nullptr;
  }
  return s;
}

int ensure_side_stream(rc_handle* h) {
  if (h->side_stream) return RC_OK;
  h->side_stream = rc_helper_stream(0);
  if (!h->side_stream) return fail(h, RC_ERR_HIP, "side stream");
  for (hipEvent_t& e : h->ev_side) RC_HIP(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return RC_OK;
}

int repack_transient(rc_handle* h);

// What the fused streams (packs.fused, packs.fused_front) are put together from.  They are packed on their own: where the
// one-wave kernel reads its output rows as tables (rc_pack_host.h kRcFusedRows) the five output blocks take pack_dot_rows
// and the offsets of FusedDens / FusedShader; every other stream of the library keeps pack_dot's fragments.
struct FusedParts {
  std::vector<float> head[3], tail[3];       // a density MLP's layers in front of its output block, and behind it (backward fragments)
  std::vector<Col> rows[3];                  // its output rows
  std::vector<float> sh_head, sh_trunk;      // the shader's layers in front of the IBRDF's output block, and between the two blocks
  std::vector<Col> io, so;                   // the two output blocks of the shader
};
// `v` at fragment `at` of the stream; a gap in front of it (at most max_gap fragments: the padding to a piece or of a row
// table, rc_rows_at) is zeros
bool put_at(std::vector<float>& stream, int at, const std::vector<float>& v, int max_gap) {
  const int have = (int)(stream.size() / 64);
  if (stream.size() % 64 != 0 || have > at || at - have > max_gap) return false;
  stream.resize((size_t)at * 64, 0.0f);
  append(stream, v);
  return true;
}
std::vector<float> fused_dot(const std::vector<Col>& outs, int ntiles, bool pad_to_piece) {
  return kRcFusedRows ? pack_dot_rows(outs, ntiles, pad_to_piece) : pack_dot(outs, ntiles, pad_to_piece);
}
// [density MLP 0 | 1 | 2 (+ backward)] up to F_SH, then (with_shader) the shader: false if a part misses its offset
bool build_fused_stream(const FusedParts& P, bool with_shader, std::vector<float>& stream) {
  using namespace rcfused;
  const int row_gap = kRcFusedRows ? kRcChunkFrags - 1 : 0;
  bool ok = true;
  auto level = [&](int l, int fb, int d_o, int b1) {
    ok = ok && put_at(stream, fb, P.head[l], 0) && put_at(stream, fb + d_o, fused_dot(P.rows[l], 2, false), row_gap) &&
         put_at(stream, fb + b1, P.tail[l], 0);
  };
  level(0, F_L0, FusedDens<4, F_L0>::DO, FusedDens<4, F_L0>::B1);
  level(1, F_L1, FusedDens<5, F_L1>::DO, FusedDens<5, F_L1>::B1);
  level(2, F_L2, FusedDens<17, F_L2>::DO, FusedDens<17, F_L2>::B1);
  ok = ok && put_at(stream, F_SH, {}, 3);                    // split layers start on a whole piece
  if (!with_shader) return ok;
  using SF = FusedShader;
  ok = ok && put_at(stream, F_SH + SF::F_H, P.sh_head, 0) && put_at(stream, F_SH + SF::F_IO, fused_dot(P.io, 2, kRcSplit), row_gap) &&
       put_at(stream, F_SH + SF::F_S1, P.sh_trunk, 0) && put_at(stream, F_SH + SF::F_SO, fused_dot(P.so, 4, kRcSplit), row_gap);
  return ok && (int)(stream.size() / 64) == NF_FUSED;
}

int repack(rc_handle* h) {
  std::string missing;
  const rc_config& c = h->cfg;
  FusedParts fused_parts;
  if (!h->ide_table.p) {      // directional-encoding coefficients of the cache shaders (both kinds of handle)
    RcIdeTable tb;
    build_ide_table(tb);
    RC_HIP(h, hipMalloc((void**)&h->ide_table.p, sizeof(tb)));
    h->ide_table.bytes = sizeof(tb);
    RC_HIP(h, hipMemcpy(h->ide_table.p, &tb, sizeof(tb), hipMemcpyHostToDevice));
  }
  // all grids of the cache path must be loaded
  for (int g = 0; g < 4; ++g)
    for (size_t l = 0; l < h->grids[g].sizes.size(); ++l)
      if (!h->grids[g].loaded[l])
        return fail(h, RC_ERR_MISSING_WEIGHT,
                    "missing weight: " + h->grids[g].prefix + "/" + level_name(h->grids[g].cfg, h->grids[g].sizes, h->grids[g].sizes[l]));
  for (int l = 0; l < c.num_levels; ++l) {
    const std::string base = "params/Cache/Sampler/MLP_" + std::to_string(l);
    const HostLayer* d0 = need(h, base + "/density_layers_0", missing);
    const HostLayer* d1 = need(h, base + "/density_layers_1", missing);
    const HostLayer* dout = need(h, base + "/output_density_layer", missing);
    const HostLayer* dn = (l == c.num_levels - 1) ? need(h, base + "/pred_normals_layer", missing) : nullptr;
    if (!missing.empty()) return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: " + missing);
    std::vector<Step> s;
    steps_natural(s, d0->in, 0); step_bias(s);
    // density MLPs: fp32 fragments in every build (rc_pack_host.h rc_lfr32, rc_dev_mlp.h mlp_layer_d)
    std::vector<float> stream = pack_f32(s, {tile_full(d0, 0), tile_full(d0, 1)});
    s.clear(); steps_acc(s, 2, 0); step_bias(s);
    append(stream, pack_f32(s, {tile_full(d1, 0), tile_full(d1, 1)}));
    std::vector<Col> regs = {Col{dout, 0}};
    if (dn) { regs.push_back(Col{dn, 0}); regs.push_back(Col{dn, 1}); regs.push_back(Col{dn, 2}); }
    if (l < 3) { fused_parts.head[l] = stream; fused_parts.rows[l] = regs; }
    append(stream, pack_dot(regs, 2, false));
    const size_t tail_at = stream.size();
    if (dn) {
      // backward fragments for the analytic normals (last level): W1^T, W0^T (w_out is kept from the forward dot)
      HostLayer w1t, w0t;
      w1t.in = d1->out; w1t.out = d1->in; w1t.kernel.resize(d1->kernel.size()); w1t.bias.assign(w1t.out, 0.0f);
      for (int r = 0; r < d1->in; ++r) for (int c2 = 0; c2 < d1->out; ++c2) w1t.kernel[(size_t)c2 * w1t.out + r] = d1->kernel[(size_t)r * d1->out + c2];
      w0t.in = d0->out; w0t.out = d0->in; w0t.kernel.resize(d0->kernel.size()); w0t.bias.assign(w0t.out, 0.0f);
      for (int r = 0; r < d0->in; ++r) for (int c2 = 0; c2 < d0->out; ++c2) w0t.kernel[(size_t)c2 * w0t.out + r] = d0->kernel[(size_t)r * d0->out + c2];
      std::vector<Step> sb; steps_acc(sb, 2, 0);
      append(stream, pack_f32(sb, {tile_full(&w1t, 0, 0, false), tile_full(&w1t, 1, 0, false)}));
      append(stream, pack_f32(sb, {tile_full(&w0t, 0, 0, false)}));
    }
    if (l < 3) fused_parts.tail[l].assign(stream.begin() + tail_at, stream.end());
    int rc = upload(h, h->packs.dens[l], pad_stream(stream));
    if (rc) return rc;
  }
  if (h->transient) {
    // front end of the time-resolved cache through the fused kernel's FRONT variant: [dens 0 | dens 1 | dens 2 (+ bwd)]
    int off[4];
    rc_fused_stream_offsets(&off[0], &off[1], &off[2], &off[3]);
    std::vector<float> stream;
    const bool ok = fused_geometry_ok(h) && off[3] == rcfused::F_SH && build_fused_stream(fused_parts, false, stream);
    h->fused_front_ok = ok;
    if (ok) {
      int rc = upload(h, h->packs.fused_front, pad_stream(stream));
      if (rc) return rc;
      if ((rc = build_fused_tables(h))) return rc;
    }
    return repack_transient(h);
  }
  const std::string sh = "params/Cache/Shader";
  const HostLayer* bott = need(h, sh + "/bottleneck_layer", missing);
  const HostLayer* rough = need(h, sh + "/roughness_layer", missing);
  const HostLayer* tint = need(h, sh + "/tint_layer", missing);
  const HostLayer* amb = need(h, sh + "/ambient_irradiance_layer", missing);
  const HostLayer* irr = need(h, sh + "/irradiance_layer", missing);
  const HostLayer* i0 = need(h, sh + "/integrated_brdf_layers_0", missing);
  const HostLayer* i1 = need(h, sh + "/integrated_brdf_layers_1", missing);
  const HostLayer* io = need(h, sh + "/output_integrated_brdf_layer", missing);
  const std::string sl = sh + "/SurfaceLightField";
  const HostLayer* l0 = need(h, sl + "/layer_0", missing);
  const HostLayer* l1 = need(h, sl + "/layer_1", missing);
  const HostLayer* l2 = need(h, sl + "/layer_2", missing);
  const HostLayer* lb = need(h, sl + "/layer_bottleneck", missing);
  const HostLayer* la = need(h, sl + "/output_ambient_rgb_layer", missing);
  if (!missing.empty()) return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: " + missing);
  {
    std::vector<float> stream;
    std::vector<Step> s;
    // The shader bottleneck is linear and only feeds linear layers: fold it (fp64 products) into SLF layer_0, the
    // input part of SLF layer_bottleneck and integrated_brdf_layers_0 (see rc_dev_mlp.h, kShActSteps).
    const int FE = bott->in;                                 // 96 (the bottleneck is 96 -> 128)
    auto fold = [&](const HostLayer* L, int row0, int extra_rows) { return rcpack::fold_linear(*bott, *L, row0, extra_rows); };
    HostLayer l0f = fold(l0, 0, 72), lbf = fold(lb, 128, 72), i0f = fold(i0, 0, 1);
    for (int o = 0; o < l0->out; ++o) l0f.bias[o] = (float)((double)l0f.bias[o] + (double)l0->bias[o]);
    for (int o = 0; o < lb->out; ++o) lbf.bias[o] = (float)((double)lbf.bias[o] + (double)lb->bias[o]);
    for (int o = 0; o < i0->out; ++o) i0f.bias[o] = (float)((double)i0f.bias[o] + (double)i0->bias[o]);
    // heads: feature = [density feature (acc order) | appearance (natural)] + bias
    steps_acc(s, 2, 0); steps_natural(s, 32, 64); step_bias(s);
    std::vector<Col> regs = {Col{rough, 0}, Col{tint, 0}, Col{tint, 1}, Col{tint, 2}, Col{amb, 0},
                             Col{amb, 1},   Col{amb, 2},  Col{irr, 0},  Col{irr, 1},  Col{irr, 2}};
    append(stream, pack(s, {tile_by_reg(regs)}));
    // s0: folded SLF layer_0 + folded input part of layer_bottleneck over [feature | IDE (real | imag) | bias]
    s.clear(); steps_acc(s, 2, 0); steps_natural(s, 32, 64);
    for (int i = 0; i < 36; ++i) s.push_back({{FE + i, FE + 36 + i}});
    step_bias(s);
    append(stream, pack(s, {tile_full(&l0f, 0), tile_full(&l0f, 1), tile_full(&l0f, 2), tile_full(&l0f, 3),
                            tile_full(&lbf, 0), tile_full(&lbf, 1), tile_full(&lbf, 2), tile_full(&lbf, 3)}));
    // integrated BRDF: folded first layer on [feature | (n.v | bias)]
    s.clear(); steps_acc(s, 2, 0); steps_natural(s, 32, 64); s.push_back({{FE, -2}});
    append(stream, pack(s, {tile_full(&i0f, 0), tile_full(&i0f, 1)}));
    s.clear(); steps_acc(s, 2, 0); step_bias(s);
    append(stream, pack(s, {tile_full(i1, 0), tile_full(i1, 1)}));
    fused_parts.sh_head = stream;
    fused_parts.io = {Col{io, 0}};
    append(stream, pack_dot(fused_parts.io, 2));
    const size_t trunk_at = stream.size();
    // SLF trunk
    s.clear(); steps_acc(s, 4, 0); step_bias(s);
    append(stream, pack(s, {tile_full(l1, 0), tile_full(l1, 1), tile_full(l1, 2), tile_full(l1, 3)}));
    append(stream, pack(s, {tile_full(l2, 0), tile_full(l2, 1), tile_full(l2, 2), tile_full(l2, 3)}));
    std::vector<Step> sb; steps_acc(sb, 4, 0);
    append(stream, pack(sb, {tile_full(lb, 0, 0, false), tile_full(lb, 1, 0, false), tile_full(lb, 2, 0, false),
                             tile_full(lb, 3, 0, false)}));
    fused_parts.sh_trunk.assign(stream.begin() + trunk_at, stream.end());
    fused_parts.so = {Col{la, 0}, Col{la, 1}, Col{la, 2}};
    append(stream, pack_dot(fused_parts.so, 4));
    int rc = upload(h, h->packs.shader, pad_stream(stream));
    if (rc) return rc;
  }
  {
    // fused per-ray kernel (rc_fused.hip): one stream [density MLP 0 | 1 | 2 | shader]; compiled for the
    // hotdog layout only (3 levels of 64/64/32 samples, 6/7/32 density features, 32 appearance features)
    int off[4];
    const int nf = rc_fused_stream_offsets(&off[0], &off[1], &off[2], &off[3]);
    std::vector<float> stream;
    const bool ok = fused_geometry_ok(h) && nf == rcfused::NF_FUSED && build_fused_stream(fused_parts, true, stream);
    h->fused_ok = ok;
    if (ok) {
      int rc = upload(h, h->packs.fused, pad_stream(stream));
      if (rc) return rc;
      if ((rc = build_fused_tables(h))) return rc;
    }
  }
  {
    // model-level EnvMap (secondary-ray background); optional until a secondary pass is requested
    std::string miss;
    const std::string ep = "params/Cache/EnvMap";
    const HostLayer* e0 = need(h, ep + "/layer_0", miss);
    const HostLayer* e1 = need(h, ep + "/layer_1", miss);
    const HostLayer* e2 = need(h, ep + "/layer_2", miss);
    const HostLayer* eb = need(h, ep + "/layer_bottleneck", miss);
    const HostLayer* eo = need(h, ep + "/output_rgba_layer", miss);
    h->have_envmap = miss.empty();
    if (h->have_envmap) {
      std::vector<float> stream;
      std::vector<Step> s;
      auto tiles8 = [&](const HostLayer* L) {
        std::vector<Tile> t;
        for (int i = 0; i < 8; ++i) t.push_back(tile_full(L, i));
        return t;
      };
      steps_natural(s, 27, 0); step_bias(s);
      append(stream, pack(s, tiles8(e0)));
      s.clear(); steps_acc(s, 8, 0); step_bias(s);
      append(stream, pack(s, tiles8(e1)));
      append(stream, pack(s, tiles8(e2)));
      s.clear(); steps_acc(s, 8, 0);
      append(stream, pack(s, {tile_full(eb, 0, 0, false), tile_full(eb, 1, 0, false), tile_full(eb, 2, 0, false),
                              tile_full(eb, 3, 0, false)}));
      s.clear(); steps_natural(s, 27, 0); step_bias(s);
      append(stream, pack(s, {tile_full(eb, 0, 256), tile_full(eb, 1, 256), tile_full(eb, 2, 256), tile_full(eb, 3, 256)}));
      s.clear(); steps_acc(s, 4, 0); step_bias(s);
      append(stream, pack(s, {tile_by_reg({Col{eo, 0}, Col{eo, 1}, Col{eo, 2}})}));
      int rc = upload(h, h->packs.envmap, pad_stream(stream));
      if (rc) return rc;
    }
  }
  {
    // material / light heads run as plain per-point kernels on the Flax layout
    h->have_material = true;
    for (int i = 0; i < RAW_COUNT; ++i) {
      std::string miss;
      const HostLayer* L = need(h, kRawPaths[i], miss);
      if (!L) { h->have_material = false; continue; }
      int rc = upload(h, h->packs.raw[i].kernel, L->kernel);
      if (rc) return rc;
      if ((rc = upload(h, h->packs.raw[i].bias, L->bias))) return rc;
    }
    for (int g = 4; g < 6; ++g)
      for (size_t l = 0; l < h->grids[g].sizes.size(); ++l)
        if (!h->grids[g].loaded[l]) h->have_material = false;
  }
  if (h->fused_ok) build_fused_template(h);
  h->packed_dirty = false;
  return RC_OK;
}

// ---------------------------------------------------------------------------------------------
// Workspace
// ---------------------------------------------------------------------------------------------
void drop_graphs(rc_handle* h);

int ws_alloc(rc_handle* h, WsBuf& b, int64_t count) {
  const size_t bytes = (size_t)count * sizeof(float);
  if (b.bytes < bytes) {
    // captured graphs have workspace pointers baked into their kernel arguments: none survives a reallocation
    // (whichever entry point grew the buffer), so this is the one place that invalidates them
    drop_graphs(h);
    if (b.p) RC_HIP(h, hipFree(b.p));
    b = WsBuf{};
    RC_HIP(h, hipMalloc((void**)&b.p, bytes));
    b.bytes = bytes;
  }
  b.count = count;
  return RC_OK;
}

// Requests in order; the first failure is returned.
struct WsReq { WsBuf& b; int64_t count; };
int ws_alloc(rc_handle* h, std::initializer_list<WsReq> reqs) {
  for (const WsReq& q : reqs)
    if (int rc = ws_alloc(h, q.b, q.count)) return rc;
  return RC_OK;
}

// The proposal sampler's buffers of level l in set `w`.
int ws_sampler_level(rc_handle* h, RenderWs& w, int l, int64_t n) {
  const int64_t S = h->cfg.num_samples[l];
  const int LF = h->grids[l].dev.num_levels * h->grids[l].dev.num_features;
  return ws_alloc(h, {{w.sdist[l], n * (S + 1)}, {w.tdist[l], n * (S + 1)}, {w.means[l], 3 * n * S}, {w.feat[l], (int64_t)LF * n * S},
                      {w.density[l], n * S}, {w.weights[l], n * S}});
}

int ensure_workspace(rc_handle* h, RenderWs& w, int64_t n) {
  // ws_alloc only (re)allocates when a buffer is too small and always records the current element
  // count, so after the largest batch has been seen this is allocation-free.
  const rc_config& c = h->cfg;
  int rc;
  for (int l = 0; l < c.num_levels; ++l)
    if ((rc = ws_sampler_level(h, w, l, n))) return rc;
  const int64_t S2 = c.num_samples[c.num_levels - 1];
  const int64_t np = n * S2;
  if ((rc = ws_alloc(h, {{w.hbuf, ((np + 31) / 32) * 32 * 64}, {w.normals_pred, 3 * np}, {w.normals_grad, 3 * np}, {w.jac, 3 * 32 * np},
                         {w.app, 32 * np}, {w.shade, RC_SHADE_CH * np}, {w.debug, 32 * ((np + 31) / 32) + 64}, {w.env_rgb, 3 * n},
                         {w.rgb_noenv, 3 * n}, {w.acc_ws, n}, {w.inds, n}, {w.src_idx, n}, {w.filt_weight, n}, {w.acc_sel, n}})))
    return rc;
  // lean resampling pass: last-level features / hidden vector / predicted normals of the picked samples only
  if ((rc = ws_alloc(h, {{w.feat_sel, 32 * n}, {w.hbuf_sel, ((n + 31) / 32) * 32 * 64}, {w.normals_sel, 3 * n}, {w.density_sel, n}})))
    return rc;
  if (h->transient && &w == &h->ws[WS_RENDER0].r) {
    const int64_t tiles = (np + 31) / 32;
    return ws_alloc(h, {{w.t_irr, tiles * 32 * 64}, {w.t_slf, tiles * 64 * 64}, {w.tshade, (int64_t)RC_TS_COUNT * np}});
  }
  return RC_OK;
}

void free_workspace(rc_handle* h) {
  for (WsSet& s : h->ws) ws_for_each(s, [](WsBuf& b) { free_buf(b); });
}

// rc_workspace_ptr: "<set prefix><name>[level]" -> the buffer (nullptr for an unknown name)
WsBuf* ws_find(rc_handle* h, const char* name) {
  std::string leaf;
  const int set = ws_split(name, leaf);
  return set < 0 ? nullptr : ws_lookup(h->ws[set], leaf, h->cfg.num_levels);
}

// roctx ranges around the stages (tracing), for `rocprofv3 --marker-trace`.  The marker library is resolved at run
// time and only when RC_ROCTX=1 is set (no link dependency, nothing on the launch path otherwise); a range covers the
// host-side enqueue of a stage -- the kernels run asynchronously and carry their own names in the kernel trace.
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  bool tried = false, open = false;
};
Roctx g_roctx;
bool roctx_on() {
  if (!g_roctx.tried) {
    g_roctx.tried = true;
    const char* env = getenv("RC_ROCTX");
    if (env && atoi(env) != 0) {
      void* lib = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
      if (!lib) lib = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
      if (lib) {
        g_roctx.push = reinterpret_cast<int (*)(const char*)>(dlsym(lib, "roctxRangePushA"));
        g_roctx.pop = reinterpret_cast<int (*)()>(dlsym(lib, "roctxRangePop"));
        if (!g_roctx.push || !g_roctx.pop) { g_roctx.push = nullptr; g_roctx.pop = nullptr; }
      }
    }
  }
  return g_roctx.push != nullptr;
}
// close the open stage range (if any) and open `name` (nullptr: only close)
void roctx_stage(const char* name) {
  if (!roctx_on()) return;
  if (g_roctx.open) { (void)g_roctx.pop(); g_roctx.open = false; }
  if (name) { (void)g_roctx.push(name); g_roctx.open = true; }
}
struct RoctxScope {       // a whole ABI call
  bool on;
  explicit RoctxScope(const char* name) : on(roctx_on()) { if (on) (void)g_roctx.push(name); }
  ~RoctxScope() { if (on) { roctx_stage(nullptr); (void)g_roctx.pop(); } }
};

void stage_mark(rc_handle* h, int slot, int idx, hipStream_t s) {
  roctx_stage(idx < ST_COUNT ? kStageNames[idx] : nullptr);
  if (slot < 0) return;
  if (h->profiling >= 2 && idx != ST_SHADER && idx != ST_SHADER + 1) return;
  (void)hipEventRecord(h->ev[slot][idx], s);
}

// One entry point's use of a workspace set on stream `st`: entering orders it behind the set's previous user on another
// stream; every exit of the scope then records the set's "done" event.  `rc`: the status of the entry (on = false: the
// call uses no set).
struct WsUse {
  rc_handle* h; WsSet& s; hipStream_t st; bool on; int rc;
  WsUse(rc_handle* h_, int set, hipStream_t st_, bool on_ = true) : h(h_), s(h_->ws[set]), st(st_), on(on_), rc(on ? enter() : RC_OK) {}
  ~WsUse() { if (on && rc == RC_OK) (void)hipEventRecord(s.done, st); }
  int enter() {
    if (!s.done) RC_HIP(h, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    if (s.used && s.stream != st) RC_HIP(h, hipStreamWaitEvent(st, s.done, 0));
    s.stream = st; s.used = true; s.last_use = ++h->use_clock;
    return RC_OK;
  }
};
// Workspace set of rc_render_rays for caller stream `st`: its own, else a free one, else the least recently used.
int ws_pick(rc_handle* h, hipStream_t st) {
  int free_i = -1, lru = 0;
  for (int i = WS_RENDER0; i <= WS_RENDER3; ++i) {
    if (h->ws[i].used && h->ws[i].stream == st) return i;
    if (!h->ws[i].used && free_i < 0) free_i = i;
    if (h->ws[i].last_use < h->ws[lru].last_use) lru = i;
  }
  return free_i >= 0 ? free_i : lru;
}

void drop_graphs(rc_handle* h) {
  for (auto& g : h->graphs) {
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (g.graph) (void)hipGraphDestroy(g.graph);
  }
  h->graphs.clear();
  h->have_last_key = false;
}

// The ray fields every ray-taking entry point requires.
int check_rays(rc_handle* h, const rc_rays* rays, const char* who) {
  if (!rays->origins || !rays->directions || !rays->viewdirs || !rays->near || !rays->far)
    return fail(h, RC_ERR_INVALID_ARG, std::string(who) + ": origins/directions/viewdirs/near/far are required");
  return RC_OK;
}

// Repack the weights if a load changed them (captured graphs hold the old packs' pointers: dropped first).
int ensure_packed(rc_handle* h) {
  if (!h->packed_dirty) return RC_OK;
  drop_graphs(h);
  return repack(h);
}

}  // namespace

extern "C" {

int rc_abi_version(void) { return RC_ABI_VERSION; }
int rc_mlp_arithmetic(void) { return kRcSplit ? 1 : 0; }
int rc_stage_count(void) { return ST_COUNT; }
const char* rc_stage_name(int32_t s) { return (s >= 0 && s < ST_COUNT) ? kStageNames[s] : ""; }

const char* rc_last_error(const rc_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int rc_create(const rc_config* cfg, int device, rc_handle** out) {
  RC_TRY
  if (!cfg || !out) { g_create_error = "rc_create: null argument"; return RC_ERR_INVALID_ARG; }
  if (cfg->abi_version != RC_ABI_VERSION) { g_create_error = "rc_create: abi_version mismatch"; return RC_ERR_INVALID_ARG; }
  if (cfg->num_levels < 1 || cfg->num_levels > RC_MAX_LEVELS) { g_create_error = "rc_create: num_levels out of range"; return RC_ERR_INVALID_ARG; }
  for (int l = 0; l < cfg->num_levels; ++l)
    if (cfg->num_samples[l] < 2 || cfg->num_samples[l] > 64) { g_create_error = "rc_create: num_samples must be in [2, 64]"; return RC_ERR_UNSUPPORTED; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { g_create_error = "rc_create: no HIP device"; return RC_ERR_NO_DEVICE; }
  if (device < 0 || device >= ndev) { g_create_error = "rc_create: bad device index"; return RC_ERR_INVALID_ARG; }
  if (hipSetDevice(device) != hipSuccess) { g_create_error = "rc_create: hipSetDevice failed"; return RC_ERR_HIP; }
  std::unique_ptr<rc_handle> hp(new rc_handle());
  rc_handle* h = hp.get();
  h->cfg = *cfg;
  h->device = device;
  // all helper streams of the process now, in a fixed order, before any work (rc_helper_stream: a low-priority stream
  // first created AFTER the high-priority ones had run took the material stage from 1.39 to 1.95 ms)
  for (int i = 0; i < 3; ++i) (void)rc_helper_stream(i);
  const rc_grid_config* gcfgs[6] = {&cfg->proposal_grids[0], &cfg->proposal_grids[1], &cfg->proposal_grids[2],
                                    &cfg->appearance_grid, &cfg->material_grid, &cfg->light_grid};
  const char* prefixes[6] = {"params/Cache/Sampler/MLP_0/density_grid", "params/Cache/Sampler/MLP_1/density_grid",
                             "params/Cache/Sampler/MLP_2/density_grid", "params/Cache/Shader/appearance_grid",
                             "params/MaterialShader/material_grid", "params/LightSampler/light_grid"};
  for (int g = 0; g < 6; ++g) {
    if (gcfgs[g]->num_features != 1 && gcfgs[g]->num_features != 4) {
      g_create_error = "rc_create: num_features must be 1 or 4";
      return RC_ERR_UNSUPPORTED;
    }
    if ((int)grid_sizes(*gcfgs[g]).size() > RC_MAX_GRID_LEVELS) {
      g_create_error = "rc_create: too many grid levels";
      return RC_ERR_UNSUPPORTED;
    }
    init_grid(h->grids[g], *gcfgs[g], prefixes[g]);
  }
  // shapes the MFMA kernels are written for
  const int K0 = h->grids[0].dev.num_levels * h->grids[0].dev.num_features;
  const int K1 = h->grids[1].dev.num_levels * h->grids[1].dev.num_features;
  const int K2 = h->grids[2].dev.num_levels * h->grids[2].dev.num_features;
  const int KA = h->grids[3].dev.num_levels * h->grids[3].dev.num_features;
  auto ks_ok = [](int K) { const int ks = (K + 1) / 2 + 1; return ks == 4 || ks == 5 || ks == 17; };
  if (cfg->num_levels != 3 || !ks_ok(K0) || !ks_ok(K1) || K2 != 32 || KA != 32) {
    g_create_error = "rc_create: unsupported grid feature widths (kernels are built for the hotdog/ngp_yobo shapes)";
    return RC_ERR_UNSUPPORTED;
  }
  *out = hp.release();
  return RC_OK;
  RC_CATCH(nullptr)
}

void rc_destroy(rc_handle* h) {
  if (!h) return;
  try {
  (void)hipSetDevice(h->device);
  for (auto& g : h->grids)
    for (auto& t : g.tables) free_buf(t);
  free_packs(h->packs);
  free_workspace(h);
  if (h->ide_table.p) (void)hipFree(h->ide_table.p);
  free_buf(h->data_w);
  free_buf(h->geom_w);
  free_buf(h->diffuse_w);
  free_buf(h->env_w);
  free_buf(h->thead_w);
  free_buf(h->itof_w);
  free_buf(h->env_padded); free_buf(h->env_pmf); free_buf(h->env_pdf); free_buf(h->env_dirs); free_buf(h->env_logp);
  if (h->pinned) (void)hipHostFree(h->pinned);
  drop_graphs(h);
  for (WsSet& s : h->ws) if (s.done) (void)hipEventDestroy(s.done);
  if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
  // side_stream / train_stream belong to the process (rc_helper_stream)
  if (h->sec_sbounds) (void)hipFree(h->sec_sbounds);
  for (hipEvent_t e : h->ev_train) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->ev_side) if (e) (void)hipEventDestroy(e);
  if (h->ev_created)
    for (int s = 0; s < kEvSlots; ++s)
      for (int i = 0; i <= ST_COUNT; ++i) (void)hipEventDestroy(h->ev[s][i]);
  } catch (...) {
  }
  delete h;
}

int rc_load_weights(rc_handle* h, const rc_tensor_desc* descs, int32_t n) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (!descs && n > 0) return fail(h, RC_ERR_INVALID_ARG, "rc_load_weights: null descs");
  RC_HIP(h, hipSetDevice(h->device));
  const auto inv = dense_inventory(h->cfg, h->transient ? &h->tcfg : nullptr);
  for (int i = 0; i < n; ++i) {
    const rc_tensor_desc& d = descs[i];
    if (!d.name || !d.data) return fail(h, RC_ERR_INVALID_ARG, "rc_load_weights: null name/data");
    const std::string name = d.name;
    int64_t count = 1;
    for (int k = 0; k < d.ndim; ++k) count *= d.shape[k];
    bool handled = false;
    // grid tables
    for (int g = 0; g < 6 && !handled; ++g) {
      GridState& gs = h->grids[g];
      if (name.compare(0, gs.prefix.size() + 1, gs.prefix + "/") != 0) continue;
      const std::string leaf = name.substr(gs.prefix.size() + 1);
      for (size_t l = 0; l < gs.sizes.size(); ++l) {
        if (leaf != level_name(gs.cfg, gs.sizes, gs.sizes[l])) continue;
        const RcGridLevel& L = gs.dev.lvl[l];
        const int64_t expect = (int64_t)L.entries * gs.cfg.num_features;
        bool shape_ok = count == expect && d.shape[d.ndim - 1] == gs.cfg.num_features;
        if (L.dense) shape_ok = shape_ok && d.ndim == 4 && d.shape[0] == L.size && d.shape[1] == L.size && d.shape[2] == L.size;
        else shape_ok = shape_ok && d.ndim == 2 && d.shape[0] == gs.cfg.hash_map_size;
        if (!shape_ok) return fail(h, RC_ERR_SHAPE, "rc_load_weights: bad shape for " + name);
        DevBuf& b = gs.tables[l];
        const size_t bytes = (size_t)expect * sizeof(float);
        if (!b.p) { RC_HIP(h, hipMalloc((void**)&b.p, bytes)); b.bytes = bytes; }
        RC_HIP(h, hipMemcpy(b.p, d.data, bytes, d.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        gs.dev.lvl[l].table = b.p;
        gs.dev.lvl[l].cell = nullptr;    // the derived cell table is stale until the next repack
        gs.dev.lvl[l].rec = nullptr;
        gs.loaded[l] = true;
        h->packed_dirty = true;          // derived device copies (interleaved level-2 tables) follow the tables
        handled = true;
        break;
      }
      if (!handled) return fail(h, RC_ERR_INVALID_ARG, "rc_load_weights: unknown grid level " + name);
    }
    if (handled) continue;
    if (h->transient && name == "params/Cache/Shader/light_power") {     // nerf.py:400-409
      if (count != 1) return fail(h, RC_ERR_SHAPE, "rc_load_weights: bad shape for " + name);
      if (d.on_device) RC_HIP(h, hipMemcpy(&h->light_power, d.data, sizeof(float), hipMemcpyDeviceToHost));
      else memcpy(&h->light_power, d.data, sizeof(float));
      h->have_light_power = true;
      continue;
    }
    // dense layers
    const size_t slash = name.rfind('/');
    if (slash == std::string::npos) return fail(h, RC_ERR_INVALID_ARG, "rc_load_weights: unknown tensor " + name);
    const std::string path = name.substr(0, slash), leaf = name.substr(slash + 1);
    auto it = inv.find(path);
    if (it == inv.end() || (leaf != "kernel" && leaf != "bias"))
      return fail(h, RC_ERR_INVALID_ARG, "rc_load_weights: unknown tensor " + name);
    HostLayer& L = h->layers[path];
    L.in = it->second.first;
    L.out = it->second.second;
    std::vector<float>& dst = leaf == "kernel" ? L.kernel : L.bias;
    if (leaf == "kernel") {
      if (d.ndim != 2 || d.shape[0] != L.in || d.shape[1] != L.out) return fail(h, RC_ERR_SHAPE, "rc_load_weights: bad shape for " + name);
    } else {
      if (d.ndim != 1 || d.shape[0] != L.out) return fail(h, RC_ERR_SHAPE, "rc_load_weights: bad shape for " + name);
    }
    dst.resize((size_t)count);
    if (d.on_device) RC_HIP(h, hipMemcpy(dst.data(), d.data, count * sizeof(float), hipMemcpyDeviceToHost));
    else memcpy(dst.data(), d.data, count * sizeof(float));
    (leaf == "kernel" ? L.have_kernel : L.have_bias) = true;
    h->packed_dirty = true;
    ++h->layers_gen;
  }
  drop_graphs(h);   // table pointers / packed fragments are baked into captured kernel arguments
  return RC_OK;
  RC_CATCH(h)
}

int rc_set_profiling(rc_handle* h, int32_t enabled) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  RC_HIP(h, hipSetDevice(h->device));
  if (enabled && !h->ev_created) {
    for (int s = 0; s < kEvSlots; ++s)
      for (int i = 0; i <= ST_COUNT; ++i) RC_HIP(h, hipEventCreate(&h->ev[s][i]));
    h->ev_created = true;
  }
  if (enabled < 0 || enabled > 3) return fail(h, RC_ERR_INVALID_ARG, "rc_set_profiling: mode must be 0, 1, 2 or 3");
  h->profiling = enabled;
  h->prof_calls = 0;
  for (int s = 0; s < kEvSlots; ++s) h->ev_used[s] = false;
  return RC_OK;
  RC_CATCH(h)
}

int rc_set_fused(rc_handle* h, int32_t mode) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (mode < 0 || mode > 3) return fail(h, RC_ERR_INVALID_ARG, "rc_set_fused: mode must be 0, 1, 2 or 3");
  if (mode != h->fused_mode) drop_graphs(h);
  h->fused_mode = mode;
  return RC_OK;
  RC_CATCH(h)
}

int rc_set_graph_mode(rc_handle* h, int32_t mode) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (mode < 0 || mode > 2) return fail(h, RC_ERR_INVALID_ARG, "rc_set_graph_mode: mode must be 0, 1 or 2");
  h->graph_mode = mode;
  if (mode == 0) drop_graphs(h);
  return RC_OK;
  RC_CATCH(h)
}

int rc_stage_times_ms(rc_handle* h, float* out_ms, int32_t n) {
  RC_TRY
  if (!h || !out_ms) return RC_ERR_INVALID_ARG;
  if (!h->ev_created) return fail(h, RC_ERR_INVALID_ARG, "rc_stage_times_ms: profiling was not enabled");
  RC_HIP(h, hipSetDevice(h->device));
  // mean over the event sets recorded since profiling was (re)enabled (at most the last kEvSlots calls)
  double sum[ST_COUNT] = {0};
  int used = 0;
  for (int s = 0; s < kEvSlots; ++s) {
    if (!h->ev_used[s]) continue;
    RC_HIP(h, hipEventSynchronize(h->ev[s][h->profiling == 1 ? ST_COUNT : ST_SHADER + 1]));
    for (int i = 0; i < ST_COUNT; ++i) {
      float ms = 0.0f;
      if (h->profiling == 1 || i == ST_SHADER) RC_HIP(h, hipEventElapsedTime(&ms, h->ev[s][i], h->ev[s][i + 1]));
      sum[i] += ms;
    }
    ++used;
  }
  if (!used) return fail(h, RC_ERR_INVALID_ARG, "rc_stage_times_ms: no profiled render call yet");
  for (int i = 0; i < ST_COUNT && i < n; ++i) out_ms[i] = (float)(sum[i] / used);
  return RC_OK;
  RC_CATCH(h)
}

int rc_workspace_ptr(rc_handle* h, const char* name, void** ptr, int64_t* count) {
  RC_TRY
  if (!h || !name || !ptr || !count) return RC_ERR_INVALID_ARG;
  const WsBuf* b = ws_find(h, name);
  if (!b || !b->p) return fail(h, RC_ERR_INVALID_ARG, std::string("rc_workspace_ptr: unknown buffer ") + name);
  *ptr = b->p;
  *count = b->count;
  return RC_OK;
  RC_CATCH(h)
}

int rc_hashgrid_lookup(rc_handle* h, int32_t grid_id, const float* points, int64_t n, float* features_out,
                       int32_t apply_contraction, void* stream) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (grid_id < 0 || grid_id >= 6) return fail(h, RC_ERR_INVALID_ARG, "rc_hashgrid_lookup: bad grid_id");
  if (n < 0 || (n > 0 && (!points || !features_out))) return fail(h, RC_ERR_INVALID_ARG, "rc_hashgrid_lookup: null buffer");
  GridState& gs = h->grids[grid_id];
  for (size_t l = 0; l < gs.sizes.size(); ++l)
    if (!gs.loaded[l]) return fail(h, RC_ERR_MISSING_WEIGHT, "rc_hashgrid_lookup: missing " + gs.prefix + "/" + level_name(gs.cfg, gs.sizes, gs.sizes[l]));
  RC_HIP(h, hipSetDevice(h->device));
  const int LF = gs.dev.num_levels * gs.dev.num_features;
  rc_launch_hashgrid(gs.dev, points, 0, n, features_out, 0, LF, apply_contraction ? h->cfg.contract_radius : 0.0f,
                     nullptr, (hipStream_t)stream);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

int rc_sample_intervals(rc_handle* h, const float* t, const float* logits, int64_t n, int32_t num_bins,
                        int32_t num_samples, const float* jitter, float* out, void* stream) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (num_bins < 1 || num_bins > 64 || num_samples < 2 || num_samples > 64)
    return fail(h, RC_ERR_UNSUPPORTED, "rc_sample_intervals: bins/samples must be <= 64 (samples >= 2)");
  if (n < 0 || (n > 0 && (!t || !logits || !out))) return fail(h, RC_ERR_INVALID_ARG, "rc_sample_intervals: null buffer");
  RC_HIP(h, hipSetDevice(h->device));
  rc_launch_sample_intervals(t, logits, n, num_bins, num_samples, jitter, out, (hipStream_t)stream);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

namespace {
// RCCL entry points, resolved from the instance the process already has (torch ships its own librccl.so: linking a
// second copy into this library would split the communicator state between two instances).
struct RcclApi {
  int (*all_gather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*group_start)() = nullptr;
  int (*group_end)() = nullptr;
  const char* (*error_string)(int) = nullptr;
  bool tried = false;
};
RcclApi g_rccl;
bool load_rccl() {
  if (g_rccl.tried) return g_rccl.all_gather != nullptr;
  g_rccl.tried = true;
  void* lib = nullptr;
  const char* env = getenv("RC_RCCL_LIBRARY");
  if (env && *env) lib = dlopen(env, RTLD_NOW | RTLD_GLOBAL);
  for (const char* nm : {"librccl.so", "librccl.so.1"}) if (!lib) lib = dlopen(nm, RTLD_NOW | RTLD_NOLOAD);
  for (const char* nm : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) if (!lib) lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
  if (!lib) return false;
  g_rccl.all_gather = (decltype(g_rccl.all_gather))dlsym(lib, "ncclAllGather");
  g_rccl.group_start = (decltype(g_rccl.group_start))dlsym(lib, "ncclGroupStart");
  g_rccl.group_end = (decltype(g_rccl.group_end))dlsym(lib, "ncclGroupEnd");
  g_rccl.error_string = (decltype(g_rccl.error_string))dlsym(lib, "ncclGetErrorString");
  if (!g_rccl.group_start || !g_rccl.group_end) g_rccl.all_gather = nullptr;
  return g_rccl.all_gather != nullptr;
}
const int kOutWidth[RC_OUT_COUNT] = {3, 1, 1, 1, 1, 1, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 1, 1, 3, 3};
}  // namespace

int rc_allgather_outputs(rc_handle* h, void* nccl_comm, const rc_outputs* local, int64_t n_local, const rc_outputs* full,
                         void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (!nccl_comm || !local || !full) return fail(h, RC_ERR_INVALID_ARG, "rc_allgather_outputs: null argument");
  if (n_local < 0) return fail(h, RC_ERR_INVALID_ARG, "rc_allgather_outputs: negative n_local");
  if (n_local == 0) return RC_OK;
  if (!load_rccl()) return fail(h, RC_ERR_UNSUPPORTED, "rc_allgather_outputs: no RCCL in this process (librccl.so / RC_RCCL_LIBRARY)");
  RC_HIP(h, hipSetDevice(h->device));
  const int kNcclFloat = 7;                                   // ncclFloat32 (rccl.h)
  int rc = g_rccl.group_start();
  for (int i = 0; i < RC_OUT_COUNT && rc == 0; ++i)
    if (local->ptr[i] && full->ptr[i])
      rc = g_rccl.all_gather(local->ptr[i], full->ptr[i], (size_t)n_local * kOutWidth[i], kNcclFloat, nccl_comm, (hipStream_t)stream_v);
  const int rc_end = g_rccl.group_end();
  if (rc == 0) rc = rc_end;
  if (rc != 0) return fail(h, RC_ERR_HIP, std::string("rc_allgather_outputs: RCCL: ") + (g_rccl.error_string ? g_rccl.error_string(rc) : "error"));
  return RC_OK;
  RC_CATCH(h)
}

}  // extern "C"

#include "rc_render_host.inc"
#include "rc_material_host.inc"
#include "rc_transient_host.inc"
#include "rc_transient_slice_host.inc"
#include "rc_batch_host.inc"
#include "rc_train_host.inc"
#include "rc_interlevel_host.inc"
#include "rc_data_host.inc"
#include "rc_geometry_host.inc"
#include "rc_normals_bwd_host.inc"
#include "rc_mask_host.inc"
#include "rc_light_host.inc"
#include "rc_material_bwd_host.inc"
#include "rc_material_data_host.inc"
#include "rc_transient_bwd_host.inc"
#include "rc_optim_host.inc"
#include "rc_metrics_host.inc"
#include "rc_metrics_si_host.inc"
#include "rc_albedo_host.inc"
#include "rc_vis_host.inc"
#include "rc_relight_host.inc"
#include "rc_prng_host.inc"
#include "rc_probe_host.inc"
#include "rc_mesh_host.inc"
#include "rc_atlas_host.inc"
