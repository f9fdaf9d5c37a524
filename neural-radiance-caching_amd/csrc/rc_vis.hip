// Visualisation of a rendered view on the device (rc_weighted_percentile, rc_image_max, rc_vis_images):
// the reference's vis.weighted_percentile / visualize_cmap / visualize_suite / visualize_transient_suite
// (internal/vis.py:50-137, 319-743) and utils.save_img_u8 (internal/utils.py:394-400).
//
//   k_vis_select_begin       the select's state
//   k_vis_select_hist        one radix pass of 8 bits over the order-preserving keys: a workgroup stages a tile of (digit,
//                            weight) in LDS, thread b adds bin b's weights in tile order into a double, and the workgroup
//                            writes its 256 sums per selection to its own slot
//   k_vis_select_narrow      one workgroup per selection: the slots added in workgroup order, the digit in which the
//                            cumulative weight passes t, the weight below it
//   k_vis_select_neighbours  the largest key below v1's, the first element with v1's key, the largest key (integer max / min)
//   k_vis_select_finish      the closed form of np.interp, in double
//   k_vis_max, k_vis_max_finish   np.max with a NaN handed on
//   k_vis_bins               one wave per pixel: the sum over the bins of a histogram image
//   k_vis_items              one thread per pixel, blockIdx.y the item: the picture as floats and / or 8-bit values
//
// The only atomics are integer max, min and or, whose results do not depend on the order; every floating sum is taken in
// an order fixed by the sizes alone.  Two calls on the same inputs are therefore bitwise equal.  The element-wise
// arithmetic is fp32 in the order of tests/vis_ref.py (-ffp-contract=off keeps multiply and add apart).
#include <hip/hip_runtime.h>

#include "rc_dev_reduce.h"
#include "rc_dev_vis.h"
#include "rc_internal.h"

namespace {

constexpr int kThreads = kReduceThreads;
constexpr int kPasses = 4, kDigitBits = 8;                // 4 x 8 bits of the 32-bit key
constexpr int kSel = kRcVisSelections;
static_assert((1 << kDigitBits) == kRcVisDigits && kRcVisDigits == kThreads, "one thread per digit");

__constant__ float kTurbo[256 * 3] = {
#include "rc_turbo_lut.inc"
};
const float kTurboHost[256 * 3] = {
#include "rc_turbo_lut.inc"
};

__device__ __forceinline__ float nan_f() { return __uint_as_float(0x7fc00000u); }
__device__ __forceinline__ double nan_d() { return __longlong_as_double(0x7ff8000000000000LL); }

// Unsigned keys in the order of numpy's sort: negative values with every bit flipped, the others with the sign bit set;
// -0 and +0 share a key, and every NaN has the largest one.
__device__ __forceinline__ uint32_t float_key(float x) {
  if (x != x) return 0xffffffffu;
  const uint32_t u = __float_as_uint(x == 0.0f ? 0.0f : x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__device__ __forceinline__ float weight_of(const RcVisSelectArgs& a, int64_t i) { return a.weight ? a.weight[i] : 1.0f; }

__global__ void __launch_bounds__(kThreads) k_vis_select_begin(RcVisSelectArgs a) {
  RcVisState* s = a.state;
  if (threadIdx.x == 0) {
    s->total = 0.0;
    s->max_key = 0u;
    s->bad = 0;
  }
  if (threadIdx.x < kSel) {
    const int k = threadIdx.x;
    s->t[k] = 0.0;
    s->below[k] = 0.0;
    s->prefix[k] = 0u;
    s->found[k] = 1;
    s->lower[k] = 0u;
    s->first[k] = 0xffffffffu;
    if (k < a.n_ps) a.out[k] = nan_d();
  }
}

// Pass `pass` (0: the top 8 bits).  In pass 0 no bit is fixed yet and every selection sees the same histogram: it is taken
// once, as selection 0's.
__global__ void __launch_bounds__(kThreads) k_vis_select_hist(RcVisSelectArgs a, int pass) {
  __shared__ __attribute__((aligned(16))) double w_s[kThreads];
  __shared__ __attribute__((aligned(16))) uint16_t dig[kSel][kThreads];
  RcVisState* s = a.state;
  const int t = threadIdx.x;
  const int shift = 32 - kDigitBits * (pass + 1);
  const int nk = pass == 0 ? 1 : a.n_ps;
  uint32_t prefix[kSel];
  double sum[kSel];
#pragma unroll
  for (int k = 0; k < kSel; ++k) {
    prefix[k] = s->prefix[k];
    sum[k] = 0.0;
  }
  const int64_t tiles = (a.n + kThreads - 1) / kThreads;
  bool bad = false;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i = tile * kThreads + t;
    float w = 0.0f;
    uint32_t key = 0u;
    const bool in = i < a.n;
    if (in) {
      w = weight_of(a, i);
      if (!(w >= 0.0f) || w > kF32Max) bad = true;
      key = float_key(a.value[i]);
    }
    w_s[t] = (double)w;
#pragma unroll
    for (int k = 0; k < kSel; ++k) {
      if (k < nk) {
        // bits above this pass's digit: a 64-bit shift, since pass 0 shifts by 32
        const bool match = in && ((uint64_t)(key ^ prefix[k]) >> (shift + kDigitBits)) == 0;
        dig[k][t] = match ? (uint16_t)((key >> shift) & (kRcVisDigits - 1)) : (uint16_t)0xffffu;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kSel; ++k) {
      if (k < nk) {
        // Tile order; every lane reads the same LDS words (broadcast).  Eight digits and eight weights are fetched by
        // five wide reads before they are used, and a weight is kept or dropped by a multiplication with 1 or 0 (exact;
        // a branch here makes every step wait for its own LDS read: one wave per SIMD has nothing to hide that behind).
        double acc = sum[k];
        const uint4* dq = reinterpret_cast<const uint4*>(dig[k]);
        const double2* wq = reinterpret_cast<const double2*>(w_s);
#pragma unroll 2
        for (int j = 0; j < kThreads / 8; ++j) {
          const uint4 d = dq[j];
          const double2 w0 = wq[4 * j], w1 = wq[4 * j + 1], w2 = wq[4 * j + 2], w3 = wq[4 * j + 3];
          const uint32_t me = (uint32_t)t;
          acc += w0.x * ((d.x & 0xffffu) == me ? 1.0 : 0.0);
          acc += w0.y * ((d.x >> 16) == me ? 1.0 : 0.0);
          acc += w1.x * ((d.y & 0xffffu) == me ? 1.0 : 0.0);
          acc += w1.y * ((d.y >> 16) == me ? 1.0 : 0.0);
          acc += w2.x * ((d.z & 0xffffu) == me ? 1.0 : 0.0);
          acc += w2.y * ((d.z >> 16) == me ? 1.0 : 0.0);
          acc += w3.x * ((d.w & 0xffffu) == me ? 1.0 : 0.0);
          acc += w3.y * ((d.w >> 16) == me ? 1.0 : 0.0);
        }
        sum[k] = acc;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < kSel; ++k)
    if (k < nk) a.part[((int64_t)blockIdx.x * nk + k) * kRcVisDigits + t] = sum[k];
  if (pass == 0 && bad) atomicOr(&s->bad, 1);
}

// Workgroup k serves selection k: bin b's sums of the `blocks` workgroups added in their order by thread b, then thread 0
// walks the bins to the digit in which below + (weights so far) passes t.  A bin without weight is never taken: values
// of weight 0 cannot be v1.
__global__ void __launch_bounds__(kThreads) k_vis_select_narrow(RcVisSelectArgs a, int pass, int blocks) {
  __shared__ double h[kRcVisDigits];
  RcVisState* s = a.state;
  const int k = blockIdx.x, t = threadIdx.x;
  const int nk = pass == 0 ? 1 : a.n_ps, kk = pass == 0 ? 0 : k;
  const int shift = 32 - kDigitBits * (pass + 1);
  double v = 0.0;
#pragma unroll 8
  for (int b = 0; b < blocks; ++b) v += a.part[((int64_t)b * nk + kk) * kRcVisDigits + t];   // loads ahead, adds in order
  h[t] = v;
  __syncthreads();
  if (t != 0) return;
  if (pass == 0) {
    double W = 0.0;
    for (int d = 0; d < kRcVisDigits; ++d) W += h[d];
    s->t[k] = a.ps[k] * (W / 100.0);
    if (k == 0) s->total = W;
  }
  if (!s->found[k]) return;
  const double target = s->t[k];
  double c = s->below[k], c_last = c;
  int chosen = -1, last = -1;
  for (int d = 0; d < kRcVisDigits; ++d) {
    const double hd = h[d];
    if (hd > 0.0) {
      last = d;
      c_last = c;
    }
    if (c + hd > target) {
      chosen = d;
      break;
    }
    c += hd;
  }
  if (chosen < 0) {
    if (pass == 0 || last < 0) {                           // t >= W or all weights zero (or NaN sums: `bad` is set)
      s->found[k] = 0;
      return;
    }
    chosen = last;                                         // sums that rounded differently from the pass before
    c = c_last;
  }
  s->prefix[k] |= (uint32_t)chosen << shift;
  s->below[k] = c;
}

__global__ void __launch_bounds__(kThreads) k_vis_select_neighbours(RcVisSelectArgs a) {
  __shared__ uint32_t lower_s[kSel], first_s[kSel], max_s;
  RcVisState* s = a.state;
  if (threadIdx.x < kSel) {
    lower_s[threadIdx.x] = 0u;
    first_s[threadIdx.x] = 0xffffffffu;
  }
  if (threadIdx.x == 0) max_s = 0u;
  __syncthreads();
  uint32_t v1[kSel], lower[kSel], first[kSel], mx = 0u;
#pragma unroll
  for (int k = 0; k < kSel; ++k) {
    v1[k] = s->prefix[k];
    lower[k] = 0u;
    first[k] = 0xffffffffu;
  }
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kThreads) {
    const uint32_t key = float_key(a.value[i]);
    mx = key > mx ? key : mx;
#pragma unroll
    for (int k = 0; k < kSel; ++k) {
      if (key < v1[k] && key + 1u > lower[k]) lower[k] = key + 1u;   // key + 1 <= v1's key: no overflow
      if (key == v1[k] && (uint32_t)i < first[k]) first[k] = (uint32_t)i;
    }
  }
#pragma unroll
  for (int k = 0; k < kSel; ++k) {
    if (k < a.n_ps && lower[k]) atomicMax(&lower_s[k], lower[k]);
    if (k < a.n_ps && first[k] != 0xffffffffu) atomicMin(&first_s[k], first[k]);
  }
  atomicMax(&max_s, mx);
  __syncthreads();
  if (threadIdx.x < a.n_ps) {
    const int k = threadIdx.x;
    if (lower_s[k]) atomicMax(&s->lower[k], lower_s[k]);
    if (first_s[k] != 0xffffffffu) atomicMin(&s->first[k], first_s[k]);
  }
  if (threadIdx.x == 0) atomicMax(&s->max_key, max_s);
}

// np.interp between (B, v0) and (B + w_f, v1), in its order of operations
__global__ void __launch_bounds__(kThreads) k_vis_select_finish(RcVisSelectArgs a) {
  const RcVisState* s = a.state;
  const int k = threadIdx.x;
  if (k >= a.n_ps) return;
  double r;
  if (s->bad) {
    r = nan_d();
  } else if (!s->found[k]) {
    r = (double)key_float(s->max_key);
  } else {
    const double v1 = (double)key_float(s->prefix[k]), B = s->below[k], t = s->t[k];
    const uint32_t at = s->first[k];
    const double w_f = at < (uint32_t)a.n ? (double)weight_of(a, (int64_t)at) : 0.0;
    const double top = B + w_f;
    if (top <= t || s->lower[k] == 0u) {
      r = v1;
    } else {
      const double v0 = (double)key_float(s->lower[k] - 1u);
      r = (v1 - v0) / (top - B) * (t - B) + v0;
    }
  }
  a.out[k] = r;
}

// ---- np.max ---------------------------------------------------------------------------------------------------------------

struct MaxNan { float m; bool nan; };
__device__ __forceinline__ void take(MaxNan& r, float x) {
  r.nan = r.nan || x != x;
  r.m = fmaxf(r.m, x);
}
// the maximum over a workgroup; thread 0 holds it
__device__ __forceinline__ float block_max(MaxNan r, float* lds /* [4] */, int* lds_nan /* [4] */) {
  int nan = r.nan ? 1 : 0;
  for (int o = 32; o > 0; o >>= 1) {
    r.m = fmaxf(r.m, __shfl_down(r.m, o, 64));
    nan |= __shfl_down(nan, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    lds[threadIdx.x >> 6] = r.m;
    lds_nan[threadIdx.x >> 6] = nan;
  }
  __syncthreads();
  const float m = fmaxf(fmaxf(lds[0], lds[1]), fmaxf(lds[2], lds[3]));
  return (lds_nan[0] | lds_nan[1] | lds_nan[2] | lds_nan[3]) ? nan_f() : m;
}

__global__ void __launch_bounds__(kThreads) k_vis_max(RcVisMaxArgs a) {
  __shared__ float lds[4];
  __shared__ int lds_nan[4];
  MaxNan r{-INFINITY, false};
  const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x, step = (int64_t)gridDim.x * kThreads;
  const int64_t nvec = ((uintptr_t)a.src & 15u) == 0 ? a.n / 4 : 0;      // 16-byte loads where the array allows them
  for (int64_t v = tid; v < nvec; v += step) {
    const float4 x = reinterpret_cast<const float4*>(a.src)[v];
    take(r, x.x);
    take(r, x.y);
    take(r, x.z);
    take(r, x.w);
  }
  for (int64_t i = 4 * nvec + tid; i < a.n; i += step) take(r, a.src[i]);
  const float m = block_max(r, lds, lds_nan);
  if (threadIdx.x == 0) a.part[blockIdx.x] = m;
}

__global__ void __launch_bounds__(kThreads) k_vis_max_finish(RcVisMaxArgs a, int blocks) {
  __shared__ float lds[4];
  __shared__ int lds_nan[4];
  MaxNan r{-INFINITY, false};
  for (int b = threadIdx.x; b < blocks; b += kThreads) take(r, a.part[b]);
  const float m = block_max(r, lds, lds_nan);
  if (threadIdx.x == 0) *a.out = m;
}

// ---- pictures -------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ float wave_sum_f(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// One wave per pixel (grid-stride): the pixel's row of channels n_bins floats is read once, lane after lane; element e of
// a row belongs to channel e % channels.
__global__ void __launch_bounds__(kThreads) k_vis_bins(RcVisBinsArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
  const int row = a.channels * a.n_bins;
  for (int64_t pix = wave; pix < a.n_pix; pix += nwaves) {
    const float* p = a.src + pix * row;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int e = lane; e < row; e += 64) {
      const float x = p[e];
      const int c = a.channels == 1 ? 0 : e % 3;
      s0 += c == 0 ? x : 0.0f;
      s1 += c == 1 ? x : 0.0f;
      s2 += c == 2 ? x : 0.0f;
    }
    s0 = wave_sum_f(s0);
    if (a.channels == 3) {
      s1 = wave_sum_f(s1);
      s2 = wave_sum_f(s2);
    }
    if (lane == 0) {
      a.dst[a.channels * pix] = s0;
      if (a.channels == 3) {
        a.dst[3 * pix + 1] = s1;
        a.dst[3 * pix + 2] = s2;
      }
    }
  }
}

// clip, linear_to_srgb, nan_to_num and save_u8 (utils.save_img_u8) are rc_dev_vis.h's

// the depth curve of the suites: -log(x + eps)
__device__ __forceinline__ float depth_curve(float x) { return -logf(x + kF32Eps); }

// one value of a colour item: scaled, then the operation
__device__ __forceinline__ float colour_value(const RcVisDevItem& it, float x, float divisor, float matte) {
  if (it.op == RC_VIS_ABS) x = fabsf(x);
  x = x * it.scale;
  x = x / it.divide;
  if (it.divisor) x = x / divisor;
  switch (it.op) {
    case RC_VIS_SRGB:
    case RC_VIS_BINSUM_SRGB: return linear_to_srgb(x);
    case RC_VIS_BINSUM_CLIP_SRGB: return linear_to_srgb(clip(x, 0.0f, 1.0f));
    case RC_VIS_MATTE: {
      float y = it.exponent != 1.0f ? powf(x, it.exponent) : x;
      if (it.offset != 0.0f) y = y + it.offset;
      return it.acc ? y + matte : y;
    }
    default: return x;                                     // RC_VIS_ABS
  }
}

__global__ void __launch_bounds__(kThreads) k_vis_items(RcVisItemsArgs a) {
  const RcVisDevItem& it = a.item[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.n_pix) return;
  float y0, y1, y2;
  if (it.op == RC_VIS_TURBO) {
    double lo = it.bounds[0], hi = it.bounds[1];
    if (it.auto_bounds) {                                  // `lo or (lo_auto - eps)`: a bound of exactly 0 is falsy
      if (lo == 0.0) lo = it.auto_bounds[0] - (double)kF32Eps;
      if (hi == 0.0) hi = it.auto_bounds[1] + (double)kF32Eps;
    }
    const float c_lo = depth_curve((float)lo), c_hi = depth_curve((float)hi), c_x = depth_curve(it.src[i]);
    const float least = (c_lo != c_lo || c_hi != c_hi) ? nan_f() : fminf(c_lo, c_hi);
    float v = clip((c_x - least) / fabsf(c_hi - c_lo), 0.0f, 1.0f);
    v = v != v ? 0.0f : v;                                 // nan_to_num: nothing infinite is left after the clip
    const int at = min((int)(v * 256.0f), 255);
    y0 = kTurbo[3 * at];
    y1 = kTurbo[3 * at + 1];
    y2 = kTurbo[3 * at + 2];
  } else {
    const float divisor = it.divisor ? *it.divisor : 1.0f;
    const float matte = it.acc ? 1.0f - it.acc[i] : 0.0f;
    if (it.channels == 3) {
      y0 = colour_value(it, it.src[3 * i], divisor, matte);
      y1 = colour_value(it, it.src[3 * i + 1], divisor, matte);
      y2 = colour_value(it, it.src[3 * i + 2], divisor, matte);
    } else {
      y0 = y1 = y2 = colour_value(it, it.src[i], divisor, matte);
    }
  }
  if (it.nan_to_num) {
    y0 = nan_to_num(y0);
    y1 = nan_to_num(y1);
    y2 = nan_to_num(y2);
  }
  if (it.mask && !(it.mask[i] > 0.0f)) y0 = y1 = y2 = 1.0f;
  if (it.out_f32) {
    it.out_f32[3 * i] = y0;
    it.out_f32[3 * i + 1] = y1;
    it.out_f32[3 * i + 2] = y2;
  }
  if (it.out_u8) {                                         // save_img_u8: round half to even
    it.out_u8[3 * i] = save_u8(y0);
    it.out_u8[3 * i + 1] = save_u8(y1);
    it.out_u8[3 * i + 2] = save_u8(y2);
  }
}

}  // namespace

int rc_vis_select_blocks(int64_t n) {
  const int64_t b = (n + kThreads - 1) / kThreads;
  return (int)(b < 1 ? 1 : (b < kRcVisMaxBlocks ? b : kRcVisMaxBlocks));
}
int rc_vis_max_blocks(int64_t n) {
  const int64_t b = (n + 4 * kThreads - 1) / (4 * kThreads);
  return (int)(b < 1 ? 1 : (b < 1024 ? b : 1024));
}
const float* rc_vis_turbo_host() { return kTurboHost; }

void rc_launch_vis_select(const RcVisSelectArgs& a, hipStream_t stream) {
  const int blocks = rc_vis_select_blocks(a.n);
  hipLaunchKernelGGL(k_vis_select_begin, dim3(1), dim3(kThreads), 0, stream, a);
  for (int pass = 0; pass < kPasses; ++pass) {
    hipLaunchKernelGGL(k_vis_select_hist, dim3(blocks), dim3(kThreads), 0, stream, a, pass);
    hipLaunchKernelGGL(k_vis_select_narrow, dim3(a.n_ps), dim3(kThreads), 0, stream, a, pass, blocks);
  }
  hipLaunchKernelGGL(k_vis_select_neighbours, dim3(blocks), dim3(kThreads), 0, stream, a);
  hipLaunchKernelGGL(k_vis_select_finish, dim3(1), dim3(kThreads), 0, stream, a);
}
void rc_launch_vis_max(const RcVisMaxArgs& a, hipStream_t stream) {
  const int blocks = rc_vis_max_blocks(a.n);
  hipLaunchKernelGGL(k_vis_max, dim3(blocks), dim3(kThreads), 0, stream, a);
  hipLaunchKernelGGL(k_vis_max_finish, dim3(1), dim3(kThreads), 0, stream, a, blocks);
}
void rc_launch_vis_bins(const RcVisBinsArgs& a, hipStream_t stream) {
  const int64_t b = (a.n_pix + 3) / 4;
  hipLaunchKernelGGL(k_vis_bins, dim3((int)(b < 8192 ? b : 8192)), dim3(kThreads), 0, stream, a);
}
void rc_launch_vis_items(const RcVisItemsArgs& a, int n_items, hipStream_t stream) {
  const int64_t blocks = (a.n_pix + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(k_vis_items, dim3((unsigned)blocks, (unsigned)n_items), dim3(kThreads), 0, stream, a);
}
