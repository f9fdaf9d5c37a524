// Host side of rc_set_env_image, rc_env_tables, rc_env_lookup, rc_env_pick and rc_render_relight (rc_relight.hip);
// included by rc_api.hip.
//
// rc_set_env_image = pad kernel + three device-to-device copies + safe_log(pmf), all into the handle's own allocations.
// rc_env_tables = per-workgroup sums -> tables.  rc_env_pick = zero the maxima -> draw -> finish.  rc_render_relight =
// material_render (rc_material_host.inc) with the relight arguments.  Nothing here reads device memory.

namespace {

// Grow-only device buffer of the handle's own (count floats).
int env_buf(rc_handle* h, DevBuf& b, int64_t count) {
  const size_t bytes = (size_t)count * sizeof(float);
  if (b.bytes >= bytes && b.p) return RC_OK;
  free_buf(b);
  RC_HIP(h, hipMalloc((void**)&b.p, bytes));
  b.bytes = bytes;
  return RC_OK;
}

int relight_common(rc_handle* h, const std::string& who) {
  if (h->transient) return fail(h, RC_ERR_UNSUPPORTED, who + ": this handle renders the time-resolved cache (rc_render_transient)");
  return RC_OK;
}

// EnvironmentSampler.sample_directions (render_utils.py:208-213): 256 picks when the leg's sample count divides by it
int64_t relight_expected_T(int64_t n, int K) { return (n * K) % 256 == 0 ? 256 : n * K; }

int relight_check(rc_handle* h, const rc_relight_args* rl, int64_t n, const MatSplit& sp) {
  const std::string who = "rc_render_relight";
  if (rl->mode != RC_RELIGHT_BRDF && rl->mode != RC_RELIGHT_ENV) return fail(h, RC_ERR_INVALID_ARG, who + ": unknown mode");
  if (h->env_img_h == 0) return fail(h, RC_ERR_INVALID_ARG, who + ": no image bound (rc_set_env_image)");
  if (rl->mode != RC_RELIGHT_ENV) return RC_OK;
  if (!h->env_tables) return fail(h, RC_ERR_INVALID_ARG, who + ": RC_RELIGHT_ENV needs the image's tables (rc_set_env_image with pmf, pdf, dirs)");
  if (!rl->picks_spec || !rl->picks_diff) return fail(h, RC_ERR_INVALID_ARG, who + ": RC_RELIGHT_ENV needs picks_spec and picks_diff");
  const int64_t ts = relight_expected_T(n, sp.Ks), td = relight_expected_T(n, sp.Kd);
  if (rl->T_spec != ts)
    return fail(h, RC_ERR_INVALID_ARG, who + ": T_spec must be " + std::to_string(ts) + " for " + std::to_string(n) + " rays x " +
                                           std::to_string(sp.Ks) + " specular samples (got " + std::to_string(rl->T_spec) + ")");
  if (rl->T_diff != td)
    return fail(h, RC_ERR_INVALID_ARG, who + ": T_diff must be " + std::to_string(td) + " for " + std::to_string(n) + " rays x " +
                                           std::to_string(sp.Kd) + " diffuse samples (got " + std::to_string(rl->T_diff) + ")");
  return RC_OK;
}

}  // namespace

extern "C" {

int rc_set_env_image(rc_handle* h, const float* rgb, const float* pmf, const float* pdf, const float* dirs, int32_t height,
                     int32_t width, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_set_env_image";
  RoctxScope roctx_call("rc_set_env_image");
  int rc;
  if ((rc = relight_common(h, who))) return rc;
  // captured graphs of rc_render_rays hold the bound image's address and size
  if (!rgb) { drop_graphs(h); h->env_img_h = 0; h->env_img_w = 0; h->env_tables = false; return RC_OK; }
  if (height < 1 || width < 1 || (int64_t)height * width >= (1ll << 31)) return fail(h, RC_ERR_INVALID_ARG, who + ": height, width must be >= 1 and H W < 2^31");
  const bool tables = pmf || pdf || dirs;
  if (tables && !(pmf && pdf && dirs)) return fail(h, RC_ERR_INVALID_ARG, who + ": pmf, pdf and dirs are given together or not at all");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  const int64_t hw = (int64_t)height * width;
  drop_graphs(h);
  h->env_img_h = 0; h->env_img_w = 0; h->env_tables = false;      // an allocation failure below leaves nothing bound
  if ((rc = env_buf(h, h->env_padded, 4 * ((int64_t)height + 2) * ((int64_t)width + 2)))) return rc;
  if (tables && ((rc = env_buf(h, h->env_pmf, hw)) || (rc = env_buf(h, h->env_pdf, hw)) || (rc = env_buf(h, h->env_dirs, 3 * hw)) ||
                 (rc = env_buf(h, h->env_logp, hw))))
    return rc;
  rc_launch_env_pad(rgb, height, width, h->env_padded.p, st);
  if (tables) {
    RC_HIP(h, hipMemcpyAsync(h->env_pmf.p, pmf, hw * sizeof(float), hipMemcpyDeviceToDevice, st));
    RC_HIP(h, hipMemcpyAsync(h->env_pdf.p, pdf, hw * sizeof(float), hipMemcpyDeviceToDevice, st));
    RC_HIP(h, hipMemcpyAsync(h->env_dirs.p, dirs, 3 * hw * sizeof(float), hipMemcpyDeviceToDevice, st));
    rc_launch_env_logp(h->env_pmf.p, hw, h->env_logp.p, st);
  }
  RC_HIP(h, hipGetLastError());
  h->env_img_h = height; h->env_img_w = width; h->env_tables = tables;
  return RC_OK;
  RC_CATCH(h)
}

int rc_env_tables(rc_handle* h, const float* rgb, int32_t height, int32_t width, float scale, float* pmf, float* pdf,
                  float* dirs, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_env_tables";
  RoctxScope roctx_call("rc_env_tables");
  int rc;
  if ((rc = relight_common(h, who))) return rc;
  if (!rgb || !pmf || !pdf || !dirs) return fail(h, RC_ERR_INVALID_ARG, who + ": null rgb/pmf/pdf/dirs");
  if (height < 1 || width < 1 || (int64_t)height * width >= (1ll << 31)) return fail(h, RC_ERR_INVALID_ARG, who + ": height, width must be >= 1 and H W < 2^31");
  if (!std::isfinite(scale)) return fail(h, RC_ERR_INVALID_ARG, who + ": scale must be finite");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  WsUse use(h, WS_RELIGHT, st);
  if ((rc = use.rc)) return rc;
  RelightWs& y = ws_extra<RelightWs>(use.s);
  const int64_t hw = (int64_t)height * width;
  if ((rc = ws_alloc(h, y.part, 2 * (int64_t)rc_env_tables_blocks(hw)))) return rc;       // doubles
  rc_launch_env_tables(RcEnvTablesArgs{rgb, height, width, scale, pmf, pdf, dirs, reinterpret_cast<double*>(y.part.p)}, st);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

int rc_env_lookup(rc_handle* h, const float* viewdirs, int64_t n, float* out_rgb, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_env_lookup";
  RoctxScope roctx_call("rc_env_lookup");
  int rc;
  if ((rc = relight_common(h, who))) return rc;
  if (n < 0) return fail(h, RC_ERR_INVALID_ARG, who + ": negative n");
  if (n == 0) return RC_OK;
  if (!viewdirs || !out_rgb) return fail(h, RC_ERR_INVALID_ARG, who + ": null viewdirs/out_rgb");
  if (h->env_img_h == 0) return fail(h, RC_ERR_INVALID_ARG, who + ": no image bound (rc_set_env_image)");
  RC_HIP(h, hipSetDevice(h->device));
  rc_launch_env_lookup(RcEnvLookupArgs{RcEnvImage{h->env_padded.p, h->env_img_h, h->env_img_w}, viewdirs, n, out_rgb}, (hipStream_t)stream_v);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

int rc_env_pick(rc_handle* h, const uint32_t key[2], int32_t T, int32_t* picks, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_env_pick";
  RoctxScope roctx_call("rc_env_pick");
  int rc;
  if ((rc = relight_common(h, who))) return rc;
  if (T < 0) return fail(h, RC_ERR_INVALID_ARG, who + ": negative T");
  if (T == 0) return RC_OK;
  if (!key || !picks) return fail(h, RC_ERR_INVALID_ARG, who + ": null key/picks");
  if (h->env_img_h == 0 || !h->env_tables) return fail(h, RC_ERR_INVALID_ARG, who + ": no pmf bound (rc_set_env_image with pmf, pdf, dirs)");
  const int64_t hw = (int64_t)h->env_img_h * h->env_img_w;
  if (T > 65535 || (int64_t)T * hw >= (1ll << 32)) return fail(h, RC_ERR_INVALID_ARG, who + ": T <= 65535 and T H W < 2^32 are required");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  WsUse use(h, WS_RELIGHT, st);
  if ((rc = use.rc)) return rc;
  RelightWs& y = ws_extra<RelightWs>(use.s);
  if ((rc = ws_alloc(h, y.best, 2 * (int64_t)T))) return rc;                                 // 64-bit integers
  RcEnvPickArgs a{};
  a.logp = h->env_logp.p; a.hw = hw; a.key0 = key[0]; a.key1 = key[1]; a.T = T;
  a.best = reinterpret_cast<unsigned long long*>(y.best.p); a.picks = picks;
  rc_launch_env_pick(a, st);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

int rc_render_relight(rc_handle* h, const rc_rays* rays, int64_t n, const rc_randoms* rnd, const rc_material_randoms* mr,
                      int32_t K, const rc_relight_args* args, const rc_outputs* cache_out, const rc_mat_outputs* mat_out,
                      void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  RoctxScope roctx_call("rc_render_relight");
  if (!args) return fail(h, RC_ERR_INVALID_ARG, "rc_render_relight: null argument");
  return material_render(h, rays, n, rnd, mr, K, args, cache_out, mat_out, stream_v, "rc_render_relight");
  RC_CATCH(h)
}

}  // extern "C"
