// Host side of rc_render_transient_slices (included at the end of rc_api.hip, DESIGN.md §4.22): the launch of
// k_transient_slice (rc_transient_slice.hip) in place of k_transient_bins, and the entry point's checks.  The trace, the
// workspace and the launch sequence up to k_transient_shader are rc_render_transient's (render_transient_impl).
namespace {

void enqueue_transient_slice(rc_handle* h, const RenderArgs& A, RenderWs& w, hipStream_t st) {
  const rc_transient_slices& sl = *A.tslices;
  RcTransSliceArgs b{};
  transient_in(h, w, A.n, b); transient_taps(h, b);
  b.w_slf = h->packs.t_slice_slf.p; b.w_irr = h->packs.t_slice_irr.p;
  b.count = sl.count;
  for (int i = 0; i < kRcSliceMax; ++i) b.t[i] = i < sl.count ? sl.t[i] : 0.0f;
  b.out_rgb = sl.rgb; b.out_direct = sl.direct; b.out_indirect = sl.indirect;
  rc_launch_transient_slice(b, st);
}

}  // namespace

int rc_render_transient_slices(rc_handle* h, const rc_rays* rays, const float* cam_origins, int64_t n, const rc_randoms* rnd,
                               const rc_randoms* shadow_rnd, const rc_transient_slices* s, const rc_transient_outputs* extra,
                               void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  RoctxScope roctx_call("rc_render_transient_slices");
  const std::string who = "rc_render_transient_slices";
  if (!h->transient) return fail(h, RC_ERR_UNSUPPORTED, who + ": call rc_set_transient first");
  if (!s) return fail(h, RC_ERR_INVALID_ARG, who + ": null slices");
  if (s->count < 1 || s->count > RC_TSLICE_MAX)
    return fail(h, RC_ERR_INVALID_ARG, who + ": count must be 1 .. " + std::to_string(RC_TSLICE_MAX));
  for (int i = 0; i < s->count; ++i)
    if (!(s->t[i] >= 0.0f && s->t[i] <= (float)(h->tcfg.n_bins - 1)))        // (a NaN fails both comparisons)
      return fail(h, RC_ERR_INVALID_ARG, who + ": t[" + std::to_string(i) + "] must lie in [0, n_bins - 1]");
  if (!s->rgb && !s->direct && !s->indirect) return fail(h, RC_ERR_INVALID_ARG, who + ": rgb, direct and indirect are all NULL");
  // the outputs of the steady-state composite come with the trace; everything else of rc_transient_outputs needs every bin
  rc_transient_outputs out{};
  if (extra) {
    static const int kComposite[] = {RC_TOUT_ACC, RC_TOUT_DISTANCE_MEAN, RC_TOUT_DISTANCE_MEDIAN, RC_TOUT_DISTANCE_PERCENTILE_5,
                                     RC_TOUT_DISTANCE_PERCENTILE_95, RC_TOUT_MEANS, RC_TOUT_NORMALS, RC_TOUT_NORMALS_PRED,
                                     RC_TOUT_RAY_DISTS, RC_TOUT_LIGHT_DISTS};
    for (int id : kComposite) out.ptr[id] = extra->ptr[id];
    for (int id = 0; id < RC_TOUT_COUNT; ++id)
      if (extra->ptr[id] && !out.ptr[id])
        return fail(h, RC_ERR_UNSUPPORTED, who + ": extra output " + std::to_string(id) + " needs every bin (rc_render_transient)");
  }
  return render_transient_impl(h, rays, cam_origins, n, rnd, shadow_rnd, &out, s, stream_v, who);
  RC_CATCH(h)
}
