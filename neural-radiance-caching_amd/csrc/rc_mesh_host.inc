// Host side of rc_query_points, rc_density_lattice and rc_isosurface (rc_mesh.hip, DESIGN.md §4.24); included by
// rc_api.hip.
//
// rc_query_points and rc_density_lattice run the existing forward kernels on chunks of kQueryChunk points of the workspace
// set WS_QUERY ("q:"), so the workspace does not grow with n or with the lattice: per chunk the points as SoA
// (k_rows_to_soa, or k_lattice_points for a slab of the lattice), the level's lookup (with its Jacobian when the analytic
// normals are wanted) and k_density_mlp; the normals back to rows; the material grid's lookup and k_material_head.
// Both calls go through the same two density launches, so a lattice equals rc_query_points at its points bit for bit.
// rc_isosurface sizes the buffers of WS_ISO ("iso:") from the lattice and enqueues rc_launch_isosurface.
// Everything is ordered on the caller's stream; nothing here waits for the device.

namespace {

constexpr int64_t kQueryChunk = 1 << 17;

// What stands in the way of level `level`'s density at points, as a status (RC_OK: nothing)
int query_level_check(rc_handle* h, const std::string& who, int level, bool analytic_normals) {
  const GridState& gs = h->grids[level];
  for (size_t l = 0; l < gs.sizes.size(); ++l)
    if (!gs.loaded[l]) return fail(h, RC_ERR_MISSING_WEIGHT, who + ": missing " + gs.prefix + "/" + level_name(gs.cfg, gs.sizes, gs.sizes[l]));
  const int K = gs.dev.num_levels * gs.dev.num_features, ks0 = (K + 1) / 2 + 1;
  if (ks0 != 4 && ks0 != 5 && ks0 != 17) return fail(h, RC_ERR_UNSUPPORTED, who + ": unsupported feature count");
  if (analytic_normals && K != 32) return fail(h, RC_ERR_UNSUPPORTED, who + ": the analytic normals need 32 grid features");
  return RC_OK;
}

int query_alloc(rc_handle* h, QueryWs& q, int level, int64_t C, bool density, bool pred, bool grad, bool material) {
  const int K = h->grids[level].dev.num_levels * h->grids[level].dev.num_features;
  int rc;
  if ((density || pred || grad) && (rc = ws_alloc(h, {{q.means, 3 * C}, {q.feat, (int64_t)K * C}, {q.density, C}}))) return rc;
  if (pred && (rc = ws_alloc(h, q.normals_pred, 3 * C))) return rc;
  if (grad && (rc = ws_alloc(h, {{q.jac, 3 * (int64_t)K * C}, {q.normals_grad, 3 * C}}))) return rc;
  if (material && (rc = ws_alloc(h, q.m_feat, (int64_t)kMaterialWidth * C))) return rc;
  return RC_OK;
}

// predict_density of level `level` at the C points of q.means: the lookup (contraction included), the density MLP with
// the gate of the contracted box; on the last level the predicted and (with the Jacobian) the analytic normals as SoA, and
// with `hbuf` the hidden vector as the shader reads it (rc_atlas_host.inc)
void query_density_chunk(rc_handle* h, QueryWs& q, int level, int64_t C, float* density, bool pred, bool grad, hipStream_t st,
                         float* hbuf = nullptr) {
  const rc_config& c = h->cfg;
  const GridState& gs = h->grids[level];
  rc_launch_hashgrid(gs.dev, q.means.p, 1, C, q.feat.p, 1, C, c.contract_radius, grad ? q.jac.p : nullptr, st);
  RcDensityMlpArgs da{};
  da.feat = q.feat.p; da.n = C; da.ld = C; da.K = gs.dev.num_levels * gs.dev.num_features;
  da.wstream = h->packs.dens[level].p; da.means = q.means.p;
  da.density_bias = c.density_bias; da.contract_radius = c.contract_radius; da.bbox = gs.cfg.bbox;
  da.last = level == c.num_levels - 1 ? 1 : 0;
  da.density = density ? density : q.density.p;
  da.normals_pred = pred ? q.normals_pred.p : nullptr; da.hbuf = hbuf;
  da.jac = grad ? q.jac.p : nullptr; da.normals_grad = grad ? q.normals_grad.p : nullptr;
  rc_launch_density_mlp(da, st);
}

// lo / hi / dims of a lattice -> RcLatticeArgs, or what is wrong with them
const char* lattice_args(const float* lo, const float* hi, int32_t nx, int32_t ny, int32_t nz, RcLatticeArgs& L) {
  if (!lo || !hi) return "null lo / hi";
  const int32_t n[3] = {nx, ny, nz};
  for (int a = 0; a < 3; ++a) {
    if (n[a] < 2 || n[a] > 1024) return "each lattice dimension must be in [2, 1024]";
    if (!(hi[a] > lo[a]) || !std::isfinite(lo[a]) || !std::isfinite(hi[a])) return "hi must exceed lo on every axis, both finite";
    L.lo[a] = lo[a];
    L.step[a] = (hi[a] - lo[a]) / (float)(n[a] - 1);
  }
  L.nx = nx; L.ny = ny; L.nz = nz;
  return nullptr;
}

}  // namespace

int rc_query_points(rc_handle* h, const float* points, int64_t n, int32_t level, float* density, float* normals_pred,
                    float* normals, float* material, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_query_points";
  const int NL = h->cfg.num_levels;
  if (n < 0 || (n > 0 && !points)) return fail(h, RC_ERR_INVALID_ARG, who + ": null points or negative n");
  if (level >= NL) return fail(h, RC_ERR_INVALID_ARG, who + ": bad level");
  if (level < 0) level = NL - 1;
  if ((normals_pred || normals) && level != NL - 1) return fail(h, RC_ERR_UNSUPPORTED, who + ": normals exist on the last level only");
  if (material && h->transient) return fail(h, RC_ERR_UNSUPPORTED, who + ": no material on a time-resolved cache handle");
  if (n == 0) return RC_OK;
  const bool dens = density || normals_pred || normals;
  if (!dens && !material) return RC_OK;
  int rc;
  if (dens && (rc = query_level_check(h, who, level, normals != nullptr))) return rc;
  RoctxScope roctx_call("rc_query_points");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  if ((rc = ensure_packed(h))) return rc;
  if (material && !h->have_material) return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: params/MaterialShader/* or params/LightSampler/*");
  WsUse use(h, WS_QUERY, st);
  if ((rc = use.rc)) return rc;
  QueryWs& q = ws_extra<QueryWs>(use.s);
  const int64_t CH = n < kQueryChunk ? n : kQueryChunk;
  if ((rc = query_alloc(h, q, level, CH, dens, normals_pred != nullptr, normals != nullptr, material != nullptr))) return rc;
  for (int64_t c0 = 0; c0 < n; c0 += CH) {
    const int64_t C = n - c0 < CH ? n - c0 : CH;
    const float* pts = points + 3 * c0;
    if (dens) {
      rc_launch_rows_to_soa(pts, C, q.means.p, st);
      query_density_chunk(h, q, level, C, density ? density + c0 : nullptr, normals_pred != nullptr, normals != nullptr, st);
      if (normals_pred) rc_launch_soa_to_rows(q.normals_pred.p, C, normals_pred + 3 * c0, st);
      if (normals) rc_launch_soa_to_rows(q.normals_grad.p, C, normals + 3 * c0, st);
    }
    if (material) {
      rc_launch_hashgrid(h->grids[4].dev, pts, 0, C, q.m_feat.p, 0, kMaterialWidth, h->cfg.contract_radius, nullptr, st);
      rc_launch_material_head(material_head_args(h, C, q.m_feat.p, material + (int64_t)RC_MAT_CH * c0), st);
    }
  }
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

int rc_density_lattice(rc_handle* h, const float* lo, const float* hi, int32_t nx, int32_t ny, int32_t nz, int32_t level,
                       float* field, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_density_lattice";
  const int NL = h->cfg.num_levels;
  RcLatticeArgs L{};
  if (const char* bad = lattice_args(lo, hi, nx, ny, nz, L)) return fail(h, RC_ERR_INVALID_ARG, who + ": " + bad);
  if (!field) return fail(h, RC_ERR_INVALID_ARG, who + ": null field");
  if (level >= NL) return fail(h, RC_ERR_INVALID_ARG, who + ": bad level");
  if (level < 0) level = NL - 1;
  int rc;
  if ((rc = query_level_check(h, who, level, false))) return rc;
  RoctxScope roctx_call("rc_density_lattice");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  if ((rc = ensure_packed(h))) return rc;
  WsUse use(h, WS_QUERY, st);
  if ((rc = use.rc)) return rc;
  QueryWs& q = ws_extra<QueryWs>(use.s);
  const int64_t n = (int64_t)nx * ny * nz;
  const int64_t CH = n < kQueryChunk ? n : kQueryChunk;
  if ((rc = query_alloc(h, q, level, CH, true, false, false, false))) return rc;
  for (int64_t c0 = 0; c0 < n; c0 += CH) {
    const int64_t C = n - c0 < CH ? n - c0 : CH;
    rc_launch_lattice_points(L, c0, C, q.means.p, st);
    query_density_chunk(h, q, level, C, field + c0, false, false, st);
  }
  rc_launch_nan_to_num(field, n, st);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

int rc_isosurface(rc_handle* h, const float* field, int32_t nx, int32_t ny, int32_t nz, float iso, const float* lo,
                  const float* hi, float* vertices, float* normals, int64_t v_capacity, int32_t* triangles,
                  int64_t t_capacity, int64_t* counts, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_isosurface";
  RcIsoArgs a{};
  if (const char* bad = lattice_args(lo, hi, nx, ny, nz, a.lat)) return fail(h, RC_ERR_INVALID_ARG, who + ": " + bad);
  if (!field || !counts) return fail(h, RC_ERR_INVALID_ARG, who + ": null field / counts");
  if (iso != iso) return fail(h, RC_ERR_INVALID_ARG, who + ": iso is NaN");
  if (v_capacity < 0 || t_capacity < 0 || v_capacity > INT32_MAX) return fail(h, RC_ERR_INVALID_ARG, who + ": v_capacity must be in [0, 2^31), t_capacity >= 0");
  if ((v_capacity > 0 && !vertices) || (t_capacity > 0 && !triangles)) return fail(h, RC_ERR_INVALID_ARG, who + ": null vertices / triangles with a capacity");
  RoctxScope roctx_call("rc_isosurface");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  WsUse use(h, WS_ISO, st);
  int rc;
  if ((rc = use.rc)) return rc;
  IsoWs& w = ws_extra<IsoWs>(use.s);
  const int64_t n = (int64_t)nx * ny * nz;
  const int64_t tiles = (n + kRcIsoTile - 1) / kRcIsoTile, groups = (tiles + kRcIsoGroup - 1) / kRcIsoGroup;
  // byte buffers in units of a float: a tile's 1024 bytes are 256 of them
  if ((rc = ws_alloc(h, {{w.mask, tiles * (kRcIsoTile / 4)}, {w.tcount, tiles * (kRcIsoTile / 4)}, {w.tile_v, tiles}, {w.tile_t, tiles},
                         {w.group_v, groups}, {w.group_t, groups}, {w.group_off, 4 * groups}, {w.vbase, n}, {w.state, 1}})))
    return rc;
  a.field = field; a.iso = iso; a.n = (uint32_t)n; a.tiles = (uint32_t)tiles; a.groups = (uint32_t)groups;
  a.mask = reinterpret_cast<uint8_t*>(w.mask.p); a.tcount = reinterpret_cast<uint8_t*>(w.tcount.p);
  a.tile_v = reinterpret_cast<int32_t*>(w.tile_v.p); a.tile_t = reinterpret_cast<int32_t*>(w.tile_t.p);
  a.group_v = reinterpret_cast<int32_t*>(w.group_v.p); a.group_t = reinterpret_cast<int32_t*>(w.group_t.p);
  a.group_off = reinterpret_cast<int64_t*>(w.group_off.p); a.vbase = reinterpret_cast<int32_t*>(w.vbase.p);
  a.state = reinterpret_cast<RcIsoState*>(w.state.p);
  a.v_capacity = v_capacity; a.t_capacity = t_capacity;
  a.vertices = vertices; a.normals = normals; a.triangles = triangles; a.counts = counts;
  rc_launch_isosurface(a, st);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}
