// rc_material_randoms_plan / rc_prng_fill_segments (include/rc_abi.h, DESIGN.md §4.20): the material stage's random_split
// tree as a segment table (rc_prng_host.h, host only) and the one launch that fills it.  Included by rc_api.hip.

#include <algorithm>

#include "rc_prng_host.h"

int rc_material_randoms_plan(const uint32_t model_key[2], const uint32_t* loss_key, int64_t n_rays, int32_t K,
                             float diffuse_fraction, int32_t num_vmf, const int32_t* level_samples, int32_t n_levels,
                             uint32_t flags, rc_prng_segment* segs, int32_t capacity, int32_t* count, int64_t* arena_words) {
  return rc_material_randoms_plan_host(model_key, loss_key, n_rays, K, diffuse_fraction, num_vmf, level_samples, n_levels,
                                       flags, segs, capacity, count, arena_words);
}

int rc_prng_fill_segments(rc_handle* h, const rc_prng_segment* segs, int32_t n_segs, void* arena, int64_t arena_words,
                          void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (n_segs < 0 || n_segs > RC_PRNG_MAX_SEGMENTS)
    return fail(h, RC_ERR_INVALID_ARG, "rc_prng_fill_segments: n_segs must be in [0, 32]");
  if ((!segs && n_segs > 0) || arena_words < 0) return fail(h, RC_ERR_INVALID_ARG, "rc_prng_fill_segments: null table / negative size");
  RcPrngSegArgs a{};
  struct Span { int64_t lo, hi; };
  std::vector<Span> spans;
  uint32_t wgs = 0;
  for (int32_t s = 0; s < n_segs; ++s) {
    const rc_prng_segment& g = segs[s];
    const std::string who = "rc_prng_fill_segments: segment " + std::to_string(s);
    if (g.mode < RC_PRNG_BITS || g.mode > RC_PRNG_GUMBEL) return fail(h, RC_ERR_INVALID_ARG, who + ": unknown mode");
    if (g.n < 0 || g.n >= 0xFFFFFFFFll) return fail(h, RC_ERR_INVALID_ARG, who + ": n must be in [0, 2^32 - 1)");
    const int64_t n0 = g.offset2 < 0 ? g.n : (g.n + 1) / 2, n1 = g.offset2 < 0 ? 0 : g.n / 2;
    if (g.offset2 < -1 || g.offset < 0 || g.offset > arena_words || n0 > arena_words - g.offset ||
        (n1 > 0 && (g.offset2 > arena_words || n1 > arena_words - g.offset2)))
      return fail(h, RC_ERR_INVALID_ARG, who + ": destination outside the arena");
    if (n0 > 0) spans.push_back({g.offset, g.offset + n0});
    if (n1 > 0) spans.push_back({g.offset2, g.offset2 + n1});
    RcPrngSegRow& r = a.seg[s];
    r.key0 = g.key[0]; r.key1 = g.key[1]; r.mode = g.mode; r.n = (uint32_t)g.n;
    // jax.random.normal / gumbel fix their own range, as in rc_prng_fill
    r.lo = g.mode == RC_PRNG_NORMAL ? -0.99999994f : (g.mode == RC_PRNG_GUMBEL ? 1.17549435e-38f : g.lo);
    r.hi = (g.mode == RC_PRNG_NORMAL || g.mode == RC_PRNG_GUMBEL) ? 1.0f : g.hi;
    r.off = g.offset; r.off2 = n1 > 0 || g.offset2 >= 0 ? g.offset2 : -1;
    wgs += (uint32_t)(((g.n + 1) / 2 + 255) / 256);
    a.wg_end[s] = wgs;
  }
  std::sort(spans.begin(), spans.end(), [](const Span& x, const Span& y) { return x.lo < y.lo; });
  for (size_t i = 1; i < spans.size(); ++i)
    if (spans[i].lo < spans[i - 1].hi) return fail(h, RC_ERR_INVALID_ARG, "rc_prng_fill_segments: two destinations overlap");
  if (wgs == 0) return RC_OK;
  if (!arena) return fail(h, RC_ERR_INVALID_ARG, "rc_prng_fill_segments: null arena");
  RC_HIP(h, hipSetDevice(h->device));
  a.n_segs = n_segs; a.arena = (uint32_t*)arena;
  rc_launch_prng_fill_segments(a, (hipStream_t)stream_v);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}

// ---------------------------------------------------------------------------------------------------------
// rc_prng_fill: jax.random-compatible random tensors generated in HBM (../prng.py is the host twin)
// ---------------------------------------------------------------------------------------------------------
int rc_prng_fill(rc_handle* h, const uint32_t key[2], int32_t mode, float minval, float maxval, int64_t n, void* out,
                 void* stream_v) {
  RC_TRY
  if (!h) return RC_ERR_INVALID_ARG;
  if (!key || (!out && n > 0)) return fail(h, RC_ERR_INVALID_ARG, "rc_prng_fill: null key/output");
  if (mode < RC_PRNG_BITS || mode > RC_PRNG_GUMBEL) return fail(h, RC_ERR_INVALID_ARG, "rc_prng_fill: unknown mode");
  if (n < 0 || n >= 0xFFFFFFFFll) return fail(h, RC_ERR_INVALID_ARG, "rc_prng_fill: n must be in [0, 2^32 - 1)");
  if (n == 0) return RC_OK;
  RC_HIP(h, hipSetDevice(h->device));
  RcPrngArgs a{};
  a.key0 = key[0]; a.key1 = key[1]; a.mode = mode; a.n = n; a.out = (uint32_t*)out;
  // jax.random.normal / gumbel fix their own range: (nextafter(-1, 0), 1) and (tiny, 1)
  a.lo = mode == RC_PRNG_NORMAL ? -0.99999994f : (mode == RC_PRNG_GUMBEL ? 1.17549435e-38f : minval);
  a.hi = (mode == RC_PRNG_NORMAL || mode == RC_PRNG_GUMBEL) ? 1.0f : maxval;
  rc_launch_prng_fill(a, (hipStream_t)stream_v);
  RC_HIP(h, hipGetLastError());
  return RC_OK;
  RC_CATCH(h)
}
