// Time slices of the time-resolved cache without the histograms (rc_render_transient_slices): the
// trainer's light-in-flight frame (engine/trainer.py:1693-1726, _save_path_evaluation)
//     cache_time_slice = w * cache_rgb[..., ceil t, :] + (1 - w) * cache_rgb[..., floor t, :],   w = t - floor t
// from the bins that reach floor t and ceil t only.
//
//   k_transient_slice   launched in place of k_transient_bins (rc_transient.hip) behind the unchanged k_transient_shader,
//                       one wavefront per ray, up to RC_TSLICE_MAX times per launch.
//
// Indirect part at target bin y (shift_map_coordinates, render.py:480-507, the arithmetic of k_transient_bins' tile
// epilogue): sample s with time shift d reaches y from the source bins i0 = floor(y - d) and i0 + 1.  The two targets of
// a time share a source, so a sample needs at most 3 source bins x 3 channels of each head: a lane takes ONE (time,
// sample, source bin, channel), evaluates the two head values as plain fp32 dot products of the sample's stored
// activations (LDS, one row per sample) with one weight column (global, contiguous), and leaves weight * value in LDS;
// a second pass adds the 32 samples of each (time, target, channel) in sample order.
// Direct part: the floor / ceil scatter of this ray's and the previous ray's samples into the ray's LDS histogram and the
// temporal filter of k_transient_bins (rc_dev_transient.h), the filter for the 2 x 3 entries of each time only.
// Nothing is reduced across lanes and every sum has a fixed order: two launches are bitwise equal, and a time's result
// does not depend on the other times of the launch.
#include "rc_internal.h"
#include "rc_dev_sample.h"
#include "rc_dev_transient.h"

using namespace rcdev;

namespace {

constexpr int kSliceWaves = 4;                   // rays of a workgroup (the waves share nothing)
constexpr int kItems = 32 * 9;                   // (sample, source bin slot, channel) of one time
constexpr int kHistD = kHist + 2 * kPadD;
constexpr int kRegion = kRcSliceMax * kItems > kHistD ? kRcSliceMax * kItems : kHistD;   // direct histogram, then the items' values
constexpr int kSP = 7;
constexpr int kSliceWaveLds = 32 * kRcSliceStrideSlf + 32 * kRcSliceStrideIrr + kRegion + kSP * 32;   // floats
static_assert(kSliceWaves * kSliceWaveLds * 4 <= 160 * 1024, "a workgroup's rays fit the LDS of a compute unit");
static_assert(kRcSliceMax * 6 <= 64, "one lane per (time, target, channel)");

// floor(y - d) as a bin index; far outside the histogram it is held at -8 / 708 (every bin next to it is outside too)
__device__ __forceinline__ int src_bin(float y, float d) { return (int)fminf(fmaxf(floorf(y - d), -8.0f), (float)(kBins + 8)); }

__global__ __launch_bounds__(kSliceWaves * 64) void k_transient_slice(RcTransSliceArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds_dyn[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int fl = lane & 31, h = lane >> 5;
  const int64_t ray = (int64_t)blockIdx.x * kSliceWaves + wave;
  if (ray >= a.n_rays) return;                     // no workgroup barrier below: the waves share nothing
  const int64_t n = a.n_rays * 32;                 // samples
  float* xs = lds_dyn + wave * kSliceWaveLds;      // [32 samples][kRcSliceStrideSlf]: value j = 2 step + half
  float* xi = xs + 32 * kRcSliceStrideSlf;         // [32 samples][kRcSliceStrideIrr]
  float* region = xi + 32 * kRcSliceStrideIrr;
  float* hist_d = region + kPadD;                  // direct histogram (before the temporal filter), zero padded
  float* vals = region;                            // afterwards: [time][sample][slot][channel] weight * value
  float* sp = region + kRegion;                    // [kSP][32] per-sample parameters
  enum { P_W = 0, P_TIB0, P_TIB1, P_TIB2, P_DIND, P_LO, P_HI };
  const bool want_direct = a.out_rgb || a.out_direct, want_indirect = a.out_rgb || a.out_indirect;

  for (int e = lane; e < kHistD; e += 64) region[e] = 0.0f;
  if (lane < 32) {
    const int64_t p = ray * 32 + lane;
    const TdSample in = td_sample(a, n, p);
    sp[P_W * 32 + lane] = in.w;
    sp[P_TIB0 * 32 + lane] = in.tib[0];
    sp[P_TIB1 * 32 + lane] = in.tib[1];
    sp[P_TIB2 * 32 + lane] = in.tib[2];
    sp[P_DIND * 32 + lane] = in.d_ind;
    const TdWindow win = td_window(a, in.ld, in.cdist);
    sp[P_LO * 32 + lane] = __int_as_float(win.lo);
    sp[P_HI * 32 + lane] = __int_as_float(win.hi);
  }
  if (want_indirect) {
    // this ray's activations of the two head layers, one row per sample (lane & 31 = sample, lane >> 5 = which of the
    // step's two values)
#pragma unroll 8
    for (int s = 0; s < 64; ++s) xs[fl * kRcSliceStrideSlf + 2 * s + h] = a.slf_feat[(ray * 64 + s) * 64 + lane];
#pragma unroll 8
    for (int s = 0; s < 32; ++s) xi[fl * kRcSliceStrideIrr + 2 * s + h] = a.irr_feat[(ray * 32 + s) * 64 + lane];
  }
  lds_sync<false>();

  // this lane's (time, target, channel): lanes 6 ti + 2 c + g, g = 0 the floor bin, g = 1 the ceil bin
  const int o_ti = lane / 6, o_c = (lane - 6 * o_ti) >> 1, o_g = lane & 1;
  const bool o_ok = o_ti < a.count;
  float o_t = a.t[0];
#pragma unroll
  for (int k = 1; k < kRcSliceMax; ++k) o_t = k == o_ti ? a.t[k] : o_t;
  const int o_y0 = (int)floorf(o_t), o_y1 = (int)ceilf(o_t);
  const int o_y = o_g ? o_y1 : o_y0;

  float dv = 0.0f;
  if (want_direct) {
    // ---- direct light: lanes 0-31 take the samples of the previous ray (their bins >= 700), lanes 32-63 those of this ray
    td_direct_scatter(a, n, ray - 1 + h, fl, h == 0 ? kBins : 0, hist_d);
    lds_sync<false>();
    // ---- temporal filter of this lane's entry
    float tp[kMaxTaps];
    td_load_taps(a, tp);
    if (o_ok) dv = td_filter_entry(a, tp, hist_d, o_y, o_c);
    lds_sync<false>();                             // the histogram is read: its LDS now takes the items' values
  }

  float iv = 0.0f;
  if (want_indirect) {
    // ---- one (time, sample, source bin slot, channel) per lane: weight * value of source bin floor(y0 - d) + slot
    const int total = a.count * kItems;
    for (int it0 = 0; it0 < total; it0 += 64) {
      const int it = it0 + lane;
      const bool valid = it < total;
      const int ti = it / kItems, rem = it - ti * kItems;
      const int s = rem / 9, q = rem - 9 * s, j = q / 3, c = q - 3 * j;
      float tsel = a.t[0];
#pragma unroll
      for (int k = 1; k < kRcSliceMax; ++k) tsel = k == ti ? a.t[k] : tsel;
      const float y0 = floorf(tsel), y1 = ceilf(tsel);
      const float d = sp[P_DIND * 32 + s], w = sp[P_W * 32 + s];
      const int lo = __float_as_int(sp[P_LO * 32 + s]), hi = __float_as_int(sp[P_HI * 32 + s]);
      const int ia = src_bin(y0, d), ib = src_bin(y1, d);
      const int b = ia + j;
      // a pair outside the histogram, outside the sample's window, read by neither target or with weight 0 is an exact zero
      const bool need = valid && w != 0.0f && b >= 0 && b < kBins && b >= lo && b <= hi &&
                        (b == ia || b == ia + 1 || b == ib || b == ib + 1);
      float val = 0.0f;
      if (need) {
        const int col = 3 * b + c;
        const float* ws = a.w_slf + (size_t)col * kRcSliceStrideSlf;
        const float* wi = a.w_irr + (size_t)col * kRcSliceStrideIrr;
        const float4* ws4 = reinterpret_cast<const float4*>(ws);
        const float4* wi4 = reinterpret_cast<const float4*>(wi);
        const float4* xs4 = reinterpret_cast<const float4*>(xs + s * kRcSliceStrideSlf);
        const float4* xi4 = reinterpret_cast<const float4*>(xi + s * kRcSliceStrideIrr);
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll 8
        for (int g = 0; g < 32; ++g) {
          const float4 wv = ws4[g], xv = xs4[g];
          s0 = __builtin_fmaf(xv.x, wv.x, s0); s1 = __builtin_fmaf(xv.y, wv.y, s1);
          s2 = __builtin_fmaf(xv.z, wv.z, s2); s3 = __builtin_fmaf(xv.w, wv.w, s3);
        }
        const float as = ((s0 + s1) + (s2 + s3)) + ws[128];
        float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f, r3 = 0.0f;
#pragma unroll 8
        for (int g = 0; g < 16; ++g) {
          const float4 wv = wi4[g], xv = xi4[g];
          r0 = __builtin_fmaf(xv.x, wv.x, r0); r1 = __builtin_fmaf(xv.y, wv.y, r1);
          r2 = __builtin_fmaf(xv.z, wv.z, r2); r3 = __builtin_fmaf(xv.w, wv.w, r3);
        }
        const float ai = ((r0 + r1) + (r2 + r3)) + wi[64];
        const float tib = sp[(P_TIB0 + c) * 32 + s];
        float diff, spec;
        td_head_value(a, ai, as, tib, diff, spec);
        val = w * (diff + spec);
      }
      if (valid) vals[it] = val;
    }
    lds_sync<false>();
    // ---- this lane's target: the 32 samples in order, each with the weights the target computes (coordinate y - d,
    //      i0 = floor, fw = y - d - i0: 1 - fw to source bin i0, fw to i0 + 1)
    if (o_ok) {
      const float yf = (float)o_y, y0f = (float)o_y0;
      const float* v = vals + o_ti * kItems + o_c;
      for (int s = 0; s < 32; ++s) {
        const float d = sp[P_DIND * 32 + s];
        const float t = yf - d;
        const float fw = t - floorf(t);
        const int jj = src_bin(yf, d) - src_bin(y0f, d);      // slot of i0; 1 or 2 for the ceil bin (2 only with fw == 0)
        const float v0 = v[s * 9 + 3 * min(max(jj, 0), 2)], v1 = v[s * 9 + 3 * min(max(jj + 1, 0), 2)];
        const float lo_v = (jj >= 0 && jj <= 2) ? v0 : 0.0f, hi_v = (jj + 1 >= 0 && jj + 1 <= 2) ? v1 : 0.0f;
        iv += hi_v * fw + lo_v * (1.0f - fw);
      }
    }
  }

  // ---- w * v[ceil t] + (1 - w) * v[floor t]: the ceil bin sits on the next lane
  const float rgb = dv + iv;
  const float rgb_hi = __shfl_xor(rgb, 1, 64), dv_hi = __shfl_xor(dv, 1, 64), iv_hi = __shfl_xor(iv, 1, 64);
  if (o_ok && o_g == 0) {
    const float w = o_t - floorf(o_t);
    const int64_t at = (ray * a.count + o_ti) * 3 + o_c;
    if (a.out_rgb) a.out_rgb[at] = w * rgb_hi + (1.0f - w) * rgb;
    if (a.out_direct) a.out_direct[at] = w * dv_hi + (1.0f - w) * dv;
    if (a.out_indirect) a.out_indirect[at] = w * iv_hi + (1.0f - w) * iv;
  }
}

}  // namespace

void rc_launch_transient_slice(const RcTransSliceArgs& a, hipStream_t stream) {
  if (a.n_rays <= 0) return;
  static std::atomic<uint64_t> prepared{0};
  const int lds = kSliceWaves * kSliceWaveLds * (int)sizeof(float);
  if (rc_first_use_on_device(prepared)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_transient_slice), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  }
  hipLaunchKernelGGL(k_transient_slice, dim3((unsigned)((a.n_rays + kSliceWaves - 1) / kSliceWaves)), dim3(kSliceWaves * 64), lds,
                     stream, a);
}
