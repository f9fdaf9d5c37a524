// Host side of rc_weighted_percentile, rc_image_max and rc_vis_images (rc_vis.hip); included by rc_api.hip.
//
// rc_weighted_percentile = begin -> four radix passes (hist, narrow) -> neighbours -> finish.  rc_image_max = partial
// maxima -> finish.  rc_vis_images = one bin sum per distinct histogram (rc_vis_plan.h) -> the item kernel, the item
// table copied with the launch.  Nothing here reads device memory.

#include "rc_vis_plan.h"

namespace {
constexpr int64_t kVisStateFloats = (sizeof(RcVisState) + sizeof(float) - 1) / sizeof(float);
}  // namespace

int rc_weighted_percentile(rc_handle* h, const float* value, const float* weight, int64_t n, const double* ps, int32_t n_ps,
                           double* out, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_weighted_percentile";
  if (!value || !ps || !out) return fail(h, RC_ERR_INVALID_ARG, who + ": null value/ps/out");
  if (n < 1 || n >= rcvis::kMaxElems) return fail(h, RC_ERR_INVALID_ARG, who + ": n must be in [1, 2^31)");
  if (n_ps < 1 || n_ps > kRcVisSelections) return fail(h, RC_ERR_INVALID_ARG, who + ": n_ps must be in [1, 8]");
  RoctxScope roctx_call("rc_weighted_percentile");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  int rc;
  WsUse use(h, WS_VIS, st);
  if ((rc = use.rc)) return rc;
  VisWs& y = ws_extra<VisWs>(use.s);
  const int64_t blocks = rc_vis_select_blocks(n);
  if ((rc = ws_alloc(h, {{y.state, kVisStateFloats}, {y.part, 2 * blocks * n_ps * kRcVisDigits}}))) return rc;
  RcVisSelectArgs a{};
  a.value = value; a.weight = weight; a.n = n; a.n_ps = n_ps;
  for (int k = 0; k < n_ps; ++k) a.ps[k] = ps[k];
  a.state = reinterpret_cast<RcVisState*>(y.state.p); a.part = reinterpret_cast<double*>(y.part.p); a.out = out;
  rc_launch_vis_select(a, st);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

int rc_image_max(rc_handle* h, const float* src, int64_t n, float* out, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  const std::string who = "rc_image_max";
  if (!src || !out) return fail(h, RC_ERR_INVALID_ARG, who + ": null src/out");
  if (n < 1 || n >= rcvis::kMaxElems) return fail(h, RC_ERR_INVALID_ARG, who + ": n must be in [1, 2^31)");
  RoctxScope roctx_call("rc_image_max");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  int rc;
  WsUse use(h, WS_VIS, st);
  if ((rc = use.rc)) return rc;
  VisWs& y = ws_extra<VisWs>(use.s);
  if ((rc = ws_alloc(h, y.maxpart, rc_vis_max_blocks(n)))) return rc;
  rc_launch_vis_max(RcVisMaxArgs{src, n, y.maxpart.p, out}, st);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

int rc_vis_images(rc_handle* h, const rc_vis_item* items, int32_t n_items, int32_t height, int32_t width, void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  rcvis::Plan plan;
  const std::string wrong = rcvis::plan_items(items, n_items, height, width, plan);
  if (!wrong.empty()) return fail(h, RC_ERR_INVALID_ARG, "rc_vis_images: " + wrong);
  RoctxScope roctx_call("rc_vis_images");
  RC_HIP(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream_v;
  int rc;
  WsUse use(h, WS_VIS, st);
  if ((rc = use.rc)) return rc;
  VisWs& y = ws_extra<VisWs>(use.s);
  const int64_t n_pix = (int64_t)height * width;
  // a request of 0 floats keeps what an earlier call allocated (ws_alloc only grows)
  if ((rc = ws_alloc(h, y.binsum, 3 * n_pix * (int64_t)plan.sums.size()))) return rc;
  for (size_t s = 0; s < plan.sums.size(); ++s)
    rc_launch_vis_bins(RcVisBinsArgs{plan.sums[s].src, n_pix, plan.sums[s].n_bins, plan.sums[s].channels, y.binsum.p + 3 * n_pix * (int64_t)s}, st);
  for (int32_t i0 = 0; i0 < n_items; i0 += kRcVisItemsPerLaunch) {
    const int m = std::min<int>(kRcVisItemsPerLaunch, n_items - i0);
    RcVisItemsArgs a{};
    a.n_pix = n_pix;
    for (int j = 0; j < m; ++j) {
      const rc_vis_item& it = items[i0 + j];
      RcVisDevItem& d = a.item[j];
      const int slot = plan.slot[(size_t)(i0 + j)];
      d.src = slot < 0 ? it.src : y.binsum.p + 3 * n_pix * (int64_t)slot;
      d.divisor = it.divisor; d.acc = it.acc; d.mask = it.mask; d.bounds = it.bounds; d.auto_bounds = it.auto_bounds;
      d.out_f32 = it.out_f32; d.out_u8 = it.out_u8;
      d.channels = it.channels; d.op = it.op; d.nan_to_num = it.nan_to_num;
      d.scale = it.scale; d.divide = it.divide; d.offset = it.offset; d.exponent = it.exponent;
    }
    rc_launch_vis_items(a, m, st);
  }
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

int rc_vis_turbo_lut(float* out) {
  if (!out) return RC_ERR_INVALID_ARG;
  const float* lut = rc_vis_turbo_host();
  for (int i = 0; i < 256 * 3; ++i) out[i] = lut[i];
  return RC_OK;
}
