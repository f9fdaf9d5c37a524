// Device pieces of the TransientVolumeIntegrator, one definition each, shared by its kernels: k_transient_bins
// (rc_transient.hip), k_transient_slice (rc_transient_slice.hip), k_transient_bins_bwd, k_transient_loss and
// k_transient_loss_kinds (rc_transient_bwd.hip).  Three guarantees rest on the callers running the same arithmetic: the
// direct slice is bitwise the full render's, the backward's exact zeros outside the forward's live tiles
// (§4.15), and the two loss kernels' bitwise equal filter transpose.  Every function takes plain values and the shared
// argument blocks (RcTransIn, RcTransTaps: bases of the kernels' argument structs); none knows its caller.
#pragma once
#include <hip/hip_runtime.h>

#include "rc_internal.h"

namespace rcdev {

constexpr int kBins = kRcTdBins;
constexpr int kHist = kRcTdHist;                 // 2100 histogram entries per ray, entry = bin * 3 + channel
constexpr int kMaxTaps = 32;                     // temporal filter taps handled by the unrolled window
constexpr int kPadD = 3 * (kMaxTaps / 2);        // zeros on both sides of the direct histogram: the filter window needs no range test

__device__ __forceinline__ float clip0(float x, float hi) { return fminf(fmaxf(x, 0.0f), hi); }

// ---- one sample's inputs and the bins it keeps ---------------------------------------------------------------------
struct TdSample {
  float w, ld, cdist, rd, tib[3];
  float d_ind;                                   // bins_move / exposure_time (render.py:483): ray_dist + shift, divided by the exposure
};
// sample p of n: the eight inputs in one batch of loads (as "LDS slot = load" they were eight dependent round trips in
// k_transient_bins: the loads were not moved over the LDS stores between them)
__device__ __forceinline__ TdSample td_sample(const RcTransIn& a, int64_t n, int64_t p) {
  TdSample s;
  s.ld = a.tshade[RC_TS_LDIST * n + p]; s.w = a.weights[p]; s.cdist = a.tshade[RC_TS_CAMDIST * n + p];
  s.tib[0] = a.tshade[(RC_TS_TIB + 0) * n + p]; s.tib[1] = a.tshade[(RC_TS_TIB + 1) * n + p];
  s.tib[2] = a.tshade[(RC_TS_TIB + 2) * n + p]; s.rd = a.tshade[RC_TS_RDIST * n + p];
  s.d_ind = (s.rd + a.shift) / a.exposure;
  return s;
}

// Window [lo, hi] of bins that survive zero_invalid_bins (render_utils.py:1699-1767) for a sample; lo > hi: none.
// Both travel-time tests are monotone in the bin index, so each is a bound: bins >= lo pass
// "(b + thr) * e < light_dist" (too close), bins <= hi pass "b * e + cam_dist > max_dists" (too far); the bounds
// are settled with the very comparisons of the reference.
struct TdWindow { int lo, hi; bool kill; };
__device__ __forceinline__ TdWindow td_window(const RcTransIn& a, float ld, float cdist) {
  TdWindow v;
  v.kill = a.light_zero && ld < a.light_near;                                          // render_utils.py:1750-1760
  auto close = [&](int b) { return (float)(b + a.bin_zero_threshold_light) * a.exposure < ld; };
  auto far = [&](int b) { return ((float)b * a.exposure + cdist) > a.max_dists; };
  int lo = (int)ceilf(ld / a.exposure) - a.bin_zero_threshold_light;
  lo = min(max(lo, 0), kBins);
  while (lo > 0 && !close(lo - 1)) --lo;
  while (lo < kBins && close(lo)) ++lo;
  int hi = (int)floorf((a.max_dists - cdist) / a.exposure);
  hi = min(max(hi, -1), kBins - 1);
  while (hi < kBins - 1 && !far(hi + 1)) ++hi;
  while (hi >= 0 && far(hi)) --hi;
  if (v.kill) { lo = kBins; hi = -1; }
  v.lo = lo; v.hi = hi;
  return v;
}

// ---- direct light: scatter at (ray_dist + light_dist) / exposure with floor / ceil weights (render.py:436-477) ------
// The reference indexes the flattened [rays * bins] array: bins >= 700 of a ray land at the start of the next ray's
// histogram.  il / ih: the sample's two bins as seen from the histogram `off` bins further on (0: the sample's own ray,
// kBins: the next ray of the batch), -1 outside it.  The floats are held inside the int range before the conversion, which
// is then defined for every distance: a bin far outside the histogram is dropped either way.  (k_transient_bins once
// converted unclamped; the two forms give the same bins for every distance but a NaN one, whose `high` the bare conversion
// put into bin 0 and this one drops.  The reference pins neither.)
struct TdDirect { int il, ih; float w_low, w_high; };
__device__ __forceinline__ TdDirect td_direct(const RcTransIn& a, float ld, float rd, int off) {
  TdDirect t;
  const float d = (ld + rd) / a.exposure + a.shift / a.exposure;
  const float low = fmaxf(floorf(d), 0.0f), high = ceilf(d);
  t.w_high = d - low; t.w_low = 1.0f - t.w_high;
  t.il = (int)fminf(low, 4.0f * kBins) - off; t.ih = (int)fminf(fmaxf(high, -1.0f), 4.0f * kBins) - off;
  if (t.il < 0 || t.il >= kBins) t.il = -1;
  if (t.ih < 0 || t.ih >= kBins) t.ih = -1;
  return t;
}
// Sample fl of ray sr (none when sr < 0) into the zero-padded LDS histogram hist_d of the ray `off` bins further on.
// One LDS float add per (target kind, channel) for all 64 samples of a wave at once: lane = sample, all the low targets
// first, then all the high ones -- the order of the reference's two scatter-adds (render.py:453-477: `.at[indices_low].add`,
// then `.at[indices_high].add`).  Lanes that hit one address are served one after the other by the LDS.  (Rounds 1-3 of
// k_transient_bins walked the 64 samples in order, eight v_readlane broadcasts and two three-lane adds each: 512 + 128
// instructions.)  Every lane of the wave calls it.
__device__ __forceinline__ void td_direct_scatter(const RcTransIn& a, int64_t n, int64_t sr, int fl, int off, float* hist_d) {
  int il = -1, ih = -1;
  float vl[3] = {0.0f, 0.0f, 0.0f}, vh[3] = {0.0f, 0.0f, 0.0f};
  if (sr >= 0) {
    const int64_t p = sr * 32 + fl;
    const TdDirect t = td_direct(a, a.tshade[RC_TS_LDIST * n + p], a.tshade[RC_TS_RDIST * n + p], off);
    il = t.il; ih = t.ih;
    const float w = a.weights[p];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float val = w * (a.tshade[(RC_TS_DD + c) * n + p] + a.tshade[(RC_TS_DS + c) * n + p]);
      vl[c] = val * t.w_low; vh[c] = val * t.w_high;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (il >= 0) atomicAdd(&hist_d[il * 3 + c], vl[c]);
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (ih >= 0) atomicAdd(&hist_d[ih * 3 + c], vh[c]);
}

// ---- temporal filter on the direct part (render.py:406-417) --------------------------------------------------------
// the taps in registers (wave-uniform loads)
__device__ __forceinline__ void td_load_taps(const RcTransTaps& f, float (&tp)[kMaxTaps]) {
#pragma unroll
  for (int k = 0; k < kMaxTaps; ++k) tp[k] = k < f.n_taps ? f.taps[k] : 0.0f;
}
// Entry (bin b, channel c) of the filtered histogram.  Up to kMaxTaps taps the window is n_taps LDS reads 3 floats apart
// around the entry; the zero padding of hist_d stands in for the bins outside [0, 700) (adding tap * 0 leaves the sum
// unchanged).  More taps: from memory, with a range test.  No taps: the entry itself.
__device__ __forceinline__ float td_filter_entry(const RcTransTaps& f, const float (&tp)[kMaxTaps], const float* hist_d, int b, int c) {
  const int half_taps = (f.n_taps - 1) / 2;
  const int e = b * 3 + c;
  float dv = 0.0f;
  if (f.n_taps > kMaxTaps) {
    for (int k = 0; k < f.n_taps; ++k) {
      const int yb = b - (k - half_taps);
      if (yb >= 0 && yb < kBins) dv += f.taps[k] * hist_d[yb * 3 + c];
    }
  } else if (f.n_taps > 0) {
    const float* win = hist_d + e + 3 * half_taps;        // tap k reads bin b - (k - half)
    if (f.n_taps == 25) {
#pragma unroll
      for (int k = 0; k < 25; ++k) dv += tp[k] * win[-3 * k];
    } else {
#pragma unroll
      for (int k = 0; k < kMaxTaps; ++k)
        if (k < f.n_taps) dv += tp[k] * win[-3 * k];
    }
  } else {
    dv = hist_d[e];
  }
  return dv;
}
// The filter's transpose of a ray's row sg [kHist] (LDS), written to gt_row when it is given: the forward's filter is a true
// 'same' convolution, out[b] = sum_k taps[k] in[b - (k - half)]  ->  d in[j] = sum_k taps[k] G[j + (k - half)].
// A wave's 64 lanes share the row's entries.
__device__ __forceinline__ void td_filter_transpose_row(const RcTransTaps& f, const float* sg, int lane, float* gt_row) {
  const int half = (f.n_taps - 1) / 2;
  for (int e = lane; e < kHist; e += 64) {
    float v;
    if (f.n_taps > 0) {
      v = 0.0f;
      for (int k = 0; k < f.n_taps; ++k) {
        const int j = e + 3 * (k - half);
        if (j >= 0 && j < kHist) v += f.taps[k] * sg[j];
      }
    } else {
      v = sg[e];
    }
    if (gt_row) gt_row[e] = v;
  }
}

// ---- the per-bin heads ---------------------------------------------------------------------------------------------
// softplus on the hardware transcendentals (v_exp_f32 / v_log_f32, about 1 ulp each): the per-bin heads evaluate
// 2 x 2100 of them per sample, which is what bounds k_transient_bins.
// The per-bin heads' form: max(x, 0) + log(1 + exp(-|x|)) on the two hardware transcendentals, WITHOUT the series branch
// for tiny exp(-|x|).  1 + e rounds e away below 6e-8 and carries an absolute error of <= 6e-8 below 1e-3: 4e-8 on a
// softplus that is then scaled by indirect_scale (0.05) into per-bin radiance compared at 2e-6 -- three orders of
// magnitude inside the budget, for 4 vector instructions less per evaluation (2 x 16 x 2100 evaluations per ray).
__device__ __forceinline__ float softplus_bins(float x) {
  const float e = __builtin_amdgcn_exp2f(-fabsf(x) * 1.44269504088896341f);
  return fmaxf(x, 0.0f) + __builtin_amdgcn_logf(1.0f + e) * 0.693147180559945309f;
}
// Indirect diffuse and specular radiance of one (sample, entry) from the two heads' pre-activations ai, as:
// nerf.py:1795-1797 and :1712-1719: softplus(. + irradiance_bias) * indirect_scale;
// surface_light_field.py:1037-1058 and nerf.py:1721-1723: tint * ibrdf * clip(softplus(. + rgb_bias), 0) * scale.
// jnp.clip(x, 0, rgb_max) (nerf.py:1757-1758) as ONE v_med3_f32: the median of (x, 0, rgb_max) is the clamp for
// 0 <= rgb_max and an ordered x (softplus >= 0 is never NaN here); fmaxf + fminf were two instructions plus a
// canonicalising v_max of the scalar bound each
__device__ __forceinline__ void td_head_value(const RcTransIn& a, float ai, float as, float tib, float& diff, float& spec) {
  diff = softplus_bins(ai + a.irradiance_bias) * a.indirect_scale;
  const float ref = fmaxf(softplus_bins(1.0f * as + a.slf_rgb_bias), 0.0f);
  spec = (tib * ref) * a.indirect_scale;
  diff = __builtin_amdgcn_fmed3f(diff, 0.0f, a.rgb_max);
  spec = __builtin_amdgcn_fmed3f(spec, 0.0f, a.rgb_max);
}

// ---- the data loss -------------------------------------------------------------------------------------------------
// _get_rgb_clip_for_rawnerf (train_utils.py:369-393) of an entry, rendered r and ground truth g: the cache stage's rendering
// has no "cache_rgb": the pass's own rgb
__device__ __forceinline__ float td_rawnerf_clip(const RcTransLossArgs& a, float r, float g) {
  if (a.use_gt) return clip0(g, a.clip_val);
  float cl = clip0(r, a.clip_val);
  if (a.use_combined) cl = clip0(fmaxf(cl, g), a.clip_val);
  return cl;
}

}  // namespace rcdev
