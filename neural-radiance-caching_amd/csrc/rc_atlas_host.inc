// Host side of rc_atlas_layout, rc_atlas_uvs, rc_atlas_points, rc_query_cache_diffuse and rc_bake_atlas (rc_atlas.hip,
// DESIGN.md §4.25); included by rc_api.hip behind rc_mesh_host.inc, whose chunk helpers it shares.
//
// rc_query_cache_diffuse runs the "q:" path's lookup and density-MLP launches of the last level with the hidden vector kept
// (hbuf), the appearance grid's lookup at the same points and k_shader_diffuse_points.  rc_bake_atlas loops over texel
// chunks of kQueryChunk: k_atlas_points writes the chunk's points as rows (the material lookup reads rows) and as the SoA
// the density MLP reads, the launches of rc_query_points / rc_query_cache_diffuse write straight into the planes (a plane
// is [H W][channels] in the texels' linear order), k_atlas_store zeroes the texels without an owner.  The buffers of
// WS_ATLAS ("atlas:") and WS_QUERY ("q:") are sized by the chunk, not by the atlas.  Nothing here waits for the device.

namespace {

// ambient_irradiance_layer and irradiance_layer on the Flax layout (kernel then bias, each): h->diffuse_w
int upload_diffuse_weights(rc_handle* h, const std::string& who) {
  std::string missing;
  std::vector<float> v;
  for (const char* name : {"params/Cache/Shader/ambient_irradiance_layer", "params/Cache/Shader/irradiance_layer"}) {
    const HostLayer* L = need(h, name, missing);
    if (!L) continue;
    if (L->in != 96 || L->out != 3) return fail(h, RC_ERR_UNSUPPORTED, who + ": unexpected shape of " + name);
    v.insert(v.end(), L->kernel.begin(), L->kernel.end());
    v.insert(v.end(), L->bias.begin(), L->bias.end());
  }
  if (!missing.empty()) return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: " + missing);
  if ((int)v.size() != kRcDiffuseWeights) return fail(h, RC_ERR_UNSUPPORTED, who + ": unexpected size of the diffuse heads");
  return upload(h, h->diffuse_w, v);
}

// What stands in the way of the diffuse heads on a steady-state handle (the callers refuse a time-resolved one), as a
// status; uploads their weights when a layer changed
int diffuse_check(rc_handle* h, const std::string& who) {
  const int NL = h->cfg.num_levels;
  int rc;
  if ((rc = query_level_check(h, who, NL - 1, false))) return rc;
  const GridState& ga = h->grids[3];
  for (size_t l = 0; l < ga.sizes.size(); ++l)
    if (!ga.loaded[l]) return fail(h, RC_ERR_MISSING_WEIGHT, who + ": missing " + ga.prefix + "/" + level_name(ga.cfg, ga.sizes, ga.sizes[l]));
  if (h->grids[NL - 1].dev.num_levels * h->grids[NL - 1].dev.num_features != 32 || ga.dev.num_levels * ga.dev.num_features != 32)
    return fail(h, RC_ERR_UNSUPPORTED, who + ": needs 32 features on the last density grid and the appearance grid");
  if (h->diffuse_gen != h->layers_gen) {
    if ((rc = upload_diffuse_weights(h, who))) return rc;
    h->diffuse_gen = h->layers_gen;
  }
  return RC_OK;
}

int diffuse_alloc(rc_handle* h, AtlasWs& w, int64_t C) {
  return ws_alloc(h, {{w.hidden, ((C + 31) / 32) * 32 * 64}, {w.app_feat, 32 * C}});
}

// The two heads at the C points whose SoA is q.means and whose hidden vectors the last level's density MLP left in w.hidden
void diffuse_chunk(rc_handle* h, QueryWs& q, AtlasWs& w, int64_t C, float* diffuse, hipStream_t st) {
  const rc_config& c = h->cfg;
  rc_launch_hashgrid(h->grids[3].dev, q.means.p, 1, C, w.app_feat.p, 1, C, c.contract_radius, nullptr, st);
  RcDiffuseArgs a{};
  a.n = C; a.ld = C; a.hbuf = w.hidden.p; a.app = w.app_feat.p; a.w = h->diffuse_w.p;
  a.ambient_bias = c.ambient_irradiance_bias; a.irradiance_bias = c.irradiance_bias; a.rgb_max = c.rgb_max;
  a.out = diffuse;
  rc_launch_shader_diffuse_points(a, st);
}

int atlas_layout_checked(rc_handle* h, const std::string& who, int64_t T, int32_t r, RcAtlasLayout& L) {
  const int rc = rc_atlas_layout_of(T, r, L);
  if (rc == RC_ERR_INVALID_ARG) return fail(h, rc, who + ": T must be >= 1 and the cell size in [4, 64]");
  if (rc) return fail(h, rc, who + ": the atlas would be wider or taller than 16384 texels");
  return RC_OK;
}

}  // namespace

int rc_atlas_layout(int64_t T, int32_t r, int32_t dims[4]) {
  if (!dims) return RC_ERR_INVALID_ARG;
  RcAtlasLayout L{};
  if (const int rc = rc_atlas_layout_of(T, r, L)) return rc;
  dims[0] = L.cols; dims[1] = L.rows; dims[2] = L.W; dims[3] = L.H;
  return RC_OK;
}

int rc_atlas_uvs(rc_handle* h, int64_t T, int32_t r, float* uvs, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_atlas_uvs";
  RcAtlasLayout L{};
  if (const int rc = atlas_layout_checked(h, who, T, r, L)) return rc;
  if (!uvs) return fail(h, RC_ERR_INVALID_ARG, who + ": null uvs");
  RC_HIP(h, hipSetDevice(h->device));
  rc_launch_atlas_uvs(L, uvs, (hipStream_t)stream_v);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

int rc_atlas_points(rc_handle* h, const float* vertices, int64_t V, const int32_t* triangles, int64_t T, int32_t r,
                    int64_t first, int64_t count, float* points, int32_t* owner, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_atlas_points";
  RcAtlasPointsArgs a{};
  if (const int rc = atlas_layout_checked(h, who, T, r, a.L)) return rc;
  if (!vertices || !triangles || V < 1) return fail(h, RC_ERR_INVALID_ARG, who + ": null vertices / triangles or V < 1");
  if (first < 0 || count < 0 || first > (int64_t)a.L.W * a.L.H - count)
    return fail(h, RC_ERR_INVALID_ARG, who + ": first .. first + count must lie inside the atlas");
  if (count == 0 || (!points && !owner)) return RC_OK;
  RC_HIP(h, hipSetDevice(h->device));
  a.vertices = vertices; a.V = V; a.triangles = triangles; a.first = first; a.n = count; a.rows = points; a.owner = owner;
  rc_launch_atlas_points(a, (hipStream_t)stream_v);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

int rc_query_cache_diffuse(rc_handle* h, const float* points, int64_t n, float* diffuse, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_query_cache_diffuse";
  if (n < 0 || (n > 0 && !points)) return fail(h, RC_ERR_INVALID_ARG, who + ": null points or negative n");
  if (h->transient) return fail(h, RC_ERR_UNSUPPORTED, who + ": no diffuse heads on a time-resolved cache handle");
  if (n == 0 || !diffuse) return RC_OK;
  RoctxScope roctx_call("rc_query_cache_diffuse");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  int rc;
  if ((rc = ensure_packed(h)) || (rc = diffuse_check(h, who))) return rc;
  WsUse use(h, WS_QUERY, st), use_a(h, WS_ATLAS, st);
  if ((rc = use.rc) || (rc = use_a.rc)) return rc;
  QueryWs& q = ws_extra<QueryWs>(use.s);
  AtlasWs& w = ws_extra<AtlasWs>(use_a.s);
  const int level = h->cfg.num_levels - 1;
  const int64_t CH = n < kQueryChunk ? n : kQueryChunk;
  if ((rc = query_alloc(h, q, level, CH, true, false, false, false)) || (rc = diffuse_alloc(h, w, CH))) return rc;
  for (int64_t c0 = 0; c0 < n; c0 += CH) {
    const int64_t C = n - c0 < CH ? n - c0 : CH;
    rc_launch_rows_to_soa(points + 3 * c0, C, q.means.p, st);
    query_density_chunk(h, q, level, C, nullptr, false, false, st, w.hidden.p);
    diffuse_chunk(h, q, w, C, diffuse + 6 * c0, st);
  }
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

int rc_bake_atlas(rc_handle* h, const float* vertices, int64_t V, const int32_t* triangles, int64_t T, int32_t r,
                  int32_t level, const rc_atlas_outputs* out, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_bake_atlas";
  const int NL = h->cfg.num_levels;
  RcAtlasPointsArgs pa{};
  int rc;
  if ((rc = atlas_layout_checked(h, who, T, r, pa.L))) return rc;
  if (!vertices || !triangles || V < 1) return fail(h, RC_ERR_INVALID_ARG, who + ": null vertices / triangles or V < 1");
  if (!out) return fail(h, RC_ERR_INVALID_ARG, who + ": null outputs");
  if (level >= NL) return fail(h, RC_ERR_INVALID_ARG, who + ": bad level");
  if (level < 0) level = NL - 1;
  const rc_atlas_outputs o = *out;
  if ((o.normals_pred || o.normals) && level != NL - 1) return fail(h, RC_ERR_UNSUPPORTED, who + ": normals exist on the last level only");
  if ((o.material || o.diffuse) && h->transient) return fail(h, RC_ERR_UNSUPPORTED, who + ": no material and no diffuse heads on a time-resolved cache handle");
  const bool dens = o.density || o.normals_pred || o.normals;
  if (!dens && !o.material && !o.diffuse && !o.coverage) return RC_OK;
  // the diffuse heads read the last level's hidden vector: the density launch of the planes leaves it behind when it is
  // the last level's (with or without the analytic normals' backward: the forward layers are the same code)
  const bool share = o.diffuse && dens && level == NL - 1;
  if (dens && (rc = query_level_check(h, who, level, o.normals != nullptr))) return rc;
  RoctxScope roctx_call("rc_bake_atlas");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  if ((rc = ensure_packed(h))) return rc;
  if (o.material && !h->have_material) return fail(h, RC_ERR_MISSING_WEIGHT, "missing weight: params/MaterialShader/* or params/LightSampler/*");
  if (o.diffuse && (rc = diffuse_check(h, who))) return rc;
  WsUse use(h, WS_QUERY, st), use_a(h, WS_ATLAS, st);
  if ((rc = use.rc) || (rc = use_a.rc)) return rc;
  QueryWs& q = ws_extra<QueryWs>(use.s);
  AtlasWs& w = ws_extra<AtlasWs>(use_a.s);
  const int64_t n = (int64_t)pa.L.W * pa.L.H;
  const int64_t CH = n < kQueryChunk ? n : kQueryChunk;
  // the rows feed the material lookup, the SoA the density MLP and the appearance lookup: each only where it is read
  if ((rc = ws_alloc(h, w.owner, CH)) || (o.material && (rc = ws_alloc(h, w.points, 3 * CH)))) return rc;
  if ((rc = query_alloc(h, q, level, CH, dens, o.normals_pred != nullptr, o.normals != nullptr, o.material != nullptr))) return rc;
  if (o.diffuse && ((rc = diffuse_alloc(h, w, CH)) || (rc = query_alloc(h, q, NL - 1, CH, true, false, false, false)))) return rc;
  pa.vertices = vertices; pa.V = V; pa.triangles = triangles;
  pa.rows = o.material ? w.points.p : nullptr; pa.soa = (dens || o.diffuse) ? q.means.p : nullptr;
  pa.owner = reinterpret_cast<int32_t*>(w.owner.p);
  for (int64_t c0 = 0; c0 < n; c0 += CH) {
    const int64_t C = n - c0 < CH ? n - c0 : CH;
    pa.first = c0; pa.n = C;
    rc_launch_atlas_points(pa, st);
    if (dens) {
      query_density_chunk(h, q, level, C, o.density ? o.density + c0 : nullptr, o.normals_pred != nullptr, o.normals != nullptr, st,
                          share ? w.hidden.p : nullptr);
      if (o.normals_pred) rc_launch_soa_to_rows(q.normals_pred.p, C, o.normals_pred + 3 * c0, st);
      if (o.normals) rc_launch_soa_to_rows(q.normals_grad.p, C, o.normals + 3 * c0, st);
    }
    if (o.material) {
      rc_launch_hashgrid(h->grids[4].dev, w.points.p, 0, C, q.m_feat.p, 0, kMaterialWidth, h->cfg.contract_radius, nullptr, st);
      rc_launch_material_head(material_head_args(h, C, q.m_feat.p, o.material + (int64_t)RC_MAT_CH * c0), st);
    }
    if (o.diffuse) {
      if (!share) query_density_chunk(h, q, NL - 1, C, nullptr, false, false, st, w.hidden.p);
      diffuse_chunk(h, q, w, C, o.diffuse + 6 * c0, st);
    }
    RcAtlasStoreArgs sa{};
    sa.owner = pa.owner; sa.n = C;
    sa.density = o.density ? o.density + c0 : nullptr;
    sa.normals_pred = o.normals_pred ? o.normals_pred + 3 * c0 : nullptr;
    sa.normals = o.normals ? o.normals + 3 * c0 : nullptr;
    sa.material = o.material ? o.material + (int64_t)RC_MAT_CH * c0 : nullptr;
    sa.diffuse = o.diffuse ? o.diffuse + 6 * c0 : nullptr;
    sa.coverage = o.coverage ? o.coverage + c0 : nullptr;
    rc_launch_atlas_store(sa, st);
  }
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}
