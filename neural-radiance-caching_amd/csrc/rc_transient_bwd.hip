// The time-resolved cache's data loss and the adjoint of the TransientVolumeIntegrator with the two per-bin head layers
// (DESIGN.md §4.15): the kernels behind rc_transient_data_backward (rc_transient_bwd_host.inc).
//
//   k_transient_loss      train_utils.compute_transient_data_loss (internal/train_utils.py:531-640) with loss type
//                         'rawnerf_transient_unbiased' (:725-732): one wavefront per ray turns rgb [700][3], gt, the optional
//                         nocorr pair and lossmult into G = d loss / d rgb, the ray's loss and mse sums, and Gt = the temporal
//                         filter's transpose applied to G (the forward's filter is a true 'same' convolution of the direct
//                         part, render.py:406-417: its transpose is the correlation with the same taps).  The per-ray and
//                         per-channel sums over the bins are wave reductions; the scalars are added up by
//                         k_interlevel_reduce in a fixed order.
//   k_transient_loss_kinds  the same plan and outputs under every rc_transient_loss_type (_select_transient_data_loss_function,
//                         :686-750: mse, mse_unbiased, rawnerf_transient, the four iToF types) and under Config.use_itof
//                         (:595-597, :622-623).  The modulation table W [2 P + 1][700] of render_utils.dtof_to_itof
//                         (rc_itof_host.h) is staged in LDS once per workgroup; the 2 x 3 row sums I_r(d), I_r(dn) of a row
//                         are wave reductions, one row at a time, and sum_r 2 I_r W_r[b] is accumulated per entry in
//                         registers.  No atomics: two calls on the same inputs are bitwise equal.
//   k_dtof_to_itof        render_utils.dtof_to_itof itself on [n][700][3], with the same table and row reduction.
//   k_transient_bins_bwd  the adjoint of k_transient_bins (rc_transient.hip), one wavefront per ray with the ray's G row in
//                         LDS: the gather that transposes shift_direct (render.py:436-477; a sample that spilled into the next
//                         ray of the batch reads that ray's Gt), the two-tap gather that transposes shift_map_coordinates
//                         (render.py:480-496), the clamp / zero_invalid_bins masks, indirect_scale, softplus' and tint * ibrdf.
//                         The heads' pre-activations are recomputed tile by tile as X W on v_mfma_f32_32x32x2_f32 (samples in
//                         the rows, 32 histogram entries in the columns, as the forward; the weights come row-major from L2),
//                         fp32 whatever the forward's arithmetic.  dZ of both heads goes to the chunk's buffers, where
//                         k_gemm_tile picks it up for dW += X^T dZ and dX = dZ W^T.
#include <hip/hip_runtime.h>

#include "rc_internal.h"
#include "rc_dev_transient.h"

using namespace rcdev;

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kB = kBins, kH = kHist;
constexpr int kPerLane = (kH + 63) / 64;       // histogram entries of a lane
constexpr int kTiles = (kH + 31) / 32;         // 66 column tiles of 32 entries
constexpr int kWavesPerBlock = 4;
constexpr int kBinsWaves = 1;          // rays (waves) of a k_transient_bins_bwd workgroup

__device__ __forceinline__ float half_sum(float v) {      // over the 32 lanes of a half-wave, every lane gets the sum
#pragma unroll
  for (int d = 16; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ float wave_total(float v) { return half_sum(v) + __shfl_xor(half_sum(v), 32, 64); }

__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }
// d jnp.clip(x, 0, hi) / dx = d minimum(maximum(x, 0), hi): each tie passes half
__device__ __forceinline__ float clip_grad(float x, float hi) {
  const float lo_g = x > 0.0f ? 1.0f : (x == 0.0f ? 0.5f : 0.0f);
  const float y = fmaxf(x, 0.0f);
  const float hi_g = y < hi ? 1.0f : (y == hi ? 0.5f : 0.0f);
  return lo_g * hi_g;
}

__global__ __launch_bounds__(kWavesPerBlock * 64) void k_transient_loss(RcTransLossArgs a) {
  __shared__ float sG[kWavesPerBlock][kH];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int64_t ray = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  const bool ray_ok = ray < a.n;
  if (!ray_ok) ray = a.n - 1;
  const float* rgb = a.rgb + ray * kH;
  const float* gt = a.gt + ray * kH;
  const float* rgbn = a.rgb_nocorr ? a.rgb_nocorr + ray * kH : rgb;      // train_utils.py:604-610
  const float* gtn = a.gt_nocorr ? a.gt_nocorr + ray * kH : gt;
  float dn[kPerLane];
  // per channel: sum of the clipped colour, of d, of dn, of d dn, of d^2, count of gt > thresh
  float acc[3][6];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int q = 0; q < 6; ++q) acc[c][q] = 0.0f;
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const int e = lane + 64 * k;
    const bool ok = e < kH;
    const int ec = ok ? e : 0;
    const float r = rgb[ec], g = gt[ec];
    const float d = r - g, dnv = rgbn[ec] - gtn[ec];
    dn[k] = dnv;
    const float cl = td_rawnerf_clip(a, r, g);
    const int ch = e % 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const bool m = ok && ch == c;
      acc[c][0] += m ? cl : 0.0f;
      acc[c][1] += m ? d : 0.0f;
      acc[c][2] += m ? dnv : 0.0f;
      acc[c][3] += m ? d * dnv : 0.0f;
      acc[c][4] += m ? d * d : 0.0f;
      acc[c][5] += (m && g > a.thresh) ? 1.0f : 0.0f;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int q = 0; q < 6; ++q) acc[c][q] = wave_total(acc[c][q]);
  const float lm0 = a.lossmult ? a.lossmult[ray] : 1.0f;
  float gmul[3], gadd[3], loss = 0.0f, mse = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float lm = acc[c][5] > 0.0f ? 0.0f : lm0;                       // train_utils.py:586-590
    const float p = a.exponent == 1.0f ? acc[c][0] : powf(acc[c][0], a.exponent);
    const float s = 1.0f / (p + a.eps);                                   // train_utils.py:217
    // 2 d sg(dn) s per bin, and the gauss constant row (0.5 sum d)(0.5 sum dn) 2 s gauss_mult / n_bins on every bin
    loss += lm * (s * (2.0f * acc[c][3] + a.gauss * (acc[c][1] * acc[c][2])));
    mse += lm * acc[c][4];
    gmul[c] = a.coef * (lm * s);
    gadd[c] = a.gauss * acc[c][2];                // the row is divided by n_bins, then added to all n_bins bins: once
  }
  if (ray_ok && lane == 0) { a.loss_ray[ray] = loss; a.loss_ray[a.n + ray] = mse; }
  float* sg = sG[wave];
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const int e = lane + 64 * k;
    if (e < kH) {
      const int ch = e % 3;
      const float gm = ch == 0 ? gmul[0] : (ch == 1 ? gmul[1] : gmul[2]);
      const float ga = ch == 0 ? gadd[0] : (ch == 1 ? gadd[1] : gadd[2]);
      const float v = gm * (2.0f * dn[k] + ga);
      sg[e] = v;
      if (ray_ok) a.G[ray * kH + e] = v;
    }
  }
  __syncthreads();
  td_filter_transpose_row(a, sg, lane, ray_ok ? a.Gt + ray * kH : nullptr);
}

// per-sample parameters of a ray in LDS
enum { P_W = 0, P_DIND, P_LO, P_HI, P_TIB0, P_TIB1, P_TIB2, P_DW, P_DT0, P_DT1, P_DT2, P_COUNT };

__global__ __launch_bounds__(kBinsWaves * 64) void k_transient_bins_bwd(RcTransBinsBwdArgs a) {
  __shared__ float sG[kBinsWaves][kH];
  __shared__ float sP[kBinsWaves][P_COUNT][32];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int fl = lane & 31, h = lane >> 5;
  int64_t rl = (int64_t)blockIdx.x * kBinsWaves + wave;      // ray of the chunk
  const bool ray_ok = rl < a.C;
  if (!ray_ok) rl = a.C - 1;
  const int64_t ray = a.r0 + rl;
  const int64_t n = a.n_rays * 32;
  float* sg = sG[wave];
  float (*sp)[32] = sP[wave];
  for (int e = lane; e < kH; e += 64) sg[e] = a.G[ray * kH + e];
  int win_lo = kB, win_hi = -1;
  float dir_dw = 0.0f;
  if (lane < 32) {
    const int64_t p = ray * 32 + lane;
    const TdSample in = td_sample(a, n, p);
    sp[P_W][lane] = in.w;
    sp[P_DIND][lane] = in.d_ind;
    sp[P_TIB0][lane] = in.tib[0];
    sp[P_TIB1][lane] = in.tib[1];
    sp[P_TIB2][lane] = in.tib[2];
    const TdWindow win = td_window(a, in.ld, in.cdist);
    sp[P_LO][lane] = __int_as_float(win.lo);
    sp[P_HI][lane] = __int_as_float(win.hi);
    if (win.lo <= win.hi) { win_lo = win.lo; win_hi = win.hi; }
    // ---- the direct scatter's adjoint (shift_direct, render.py:436-477): a gather of Gt at the sample's two bins, in this
    //      ray's row or the next ray's (the flattened [n 700] histogram), dropped behind the last ray as in the forward
    const TdDirect own = td_direct(a, in.ld, in.rd, 0), next = td_direct(a, in.ld, in.rd, kB);
    auto gt3 = [&](int b_own, int b_next, float (&o)[3]) {
      o[0] = o[1] = o[2] = 0.0f;
      const int b = b_own >= 0 ? b_own : b_next;
      const int64_t r = b_own >= 0 ? ray : ray + 1;
      if (b < 0 || r >= a.n_rays) return;
      const float* g = a.Gt + r * kH + 3 * b;
      o[0] = g[0]; o[1] = g[1]; o[2] = g[2];
    };
    float gl[3], gh[3];
    gt3(own.il, next.il, gl);
    gt3(own.ih, next.ih, gh);
    float dd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float gat = own.w_low * gl[c] + own.w_high * gh[c];
      const float direct = a.tshade[(RC_TS_DD + c) * n + p] + a.tshade[(RC_TS_DS + c) * n + p];
      dd[c] = in.w * gat;
      dir_dw += direct * gat;
    }
    if (ray_ok) {
      a.d_direct[3 * p] = dd[0]; a.d_direct[3 * p + 1] = dd[1]; a.d_direct[3 * p + 2] = dd[2];
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    win_lo = min(win_lo, __shfl_xor(win_lo, d, 64));
    win_hi = max(win_hi, __shfl_xor(win_hi, d, 64));
  }
  // tiles outside the bins any sample of the ray keeps: dZ is exactly zero there (the forward's tile-range skip)
  const int T_lo = win_lo <= win_hi ? (3 * win_lo) / 32 : kTiles;
  const int T_hi = win_lo <= win_hi ? (3 * win_hi + 2) / 32 : -1;
  // the heads' inputs of this ray's 32 samples: MFMA A operands (k_transient_shader's accumulator order)
  float xs[64], xi[32];
#pragma unroll
  for (int s = 0; s < 64; ++s) xs[s] = a.slf_feat[(ray * 64 + s) * 64 + lane];
#pragma unroll
  for (int s = 0; s < 32; ++s) xi[s] = a.irr_feat[(ray * 32 + s) * 64 + lane];
  // ... and row-major in the reference's column order for the GEMMs: step s, half h holds column feat(s) + 4 h
  if (ray_ok) {
    float* xo = a.x_slf + (rl * 32 + fl) * 128 + 4 * h;
#pragma unroll
    for (int s = 0; s < 64; ++s) xo[32 * (s >> 4) + (s & 3) + 8 * ((s & 15) >> 2)] = xs[s];
    float* io = a.x_irr + (rl * 32 + fl) * 64 + 4 * h;
#pragma unroll
    for (int s = 0; s < 32; ++s) io[32 * (s >> 4) + (s & 3) + 8 * ((s & 15) >> 2)] = xi[s];
  }
  __syncthreads();
  float dws[16], dtib[3][16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { dws[r] = 0.0f; dtib[0][r] = 0.0f; dtib[1][r] = 0.0f; dtib[2][r] = 0.0f; }
  float* const zi = a.dz_irr + (rl * 32 + 4 * h) * (int64_t)kH;
  float* const zs = a.dz_slf + (rl * 32 + 4 * h) * (int64_t)kRcTdLdSlf;
  for (int T = 0; T < kTiles; ++T) {
    const int f = T * 32 + fl;
    const bool fok = f < kH;
    if (T < T_lo || T > T_hi) {
      if (ray_ok) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = (r & 3) + 8 * (r >> 2);
          if (fok) zi[(int64_t)i * kH + f] = 0.0f;
          if (f < kRcTdLdSlf) zs[(int64_t)i * kRcTdLdSlf + f] = 0.0f;
        }
      }
      continue;
    }
    const int fc = fok ? f : kH - 1;
    // ---- X W of the tile for both heads, two accumulation chains side by side
    f32x16 as, ai;
#pragma unroll
    for (int r = 0; r < 16; ++r) { as[r] = 0.0f; ai[r] = 0.0f; }
    const float* ps = a.w_slf + (int64_t)(4 * h) * (kH + 1) + fc;
    const float* pi = a.w_irr + (int64_t)(4 * h) * kH + fc;
#pragma unroll
    for (int g = 0; g < 32; ++g) {
      const int s0 = 2 * g, s1 = 2 * g + 1;
      const int k0 = 32 * (s0 >> 4) + (s0 & 3) + 8 * ((s0 & 15) >> 2), k1 = 32 * (s1 >> 4) + (s1 & 3) + 8 * ((s1 & 15) >> 2);
      const int kg = 32 * (g >> 4) + (g & 3) + 8 * ((g & 15) >> 2);
      as = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[s0], ps[(int64_t)k0 * (kH + 1)], as, 0, 0, 0);
      ai = __builtin_amdgcn_mfma_f32_32x32x2f32(xi[g], pi[(int64_t)kg * kH], ai, 0, 0, 0);
      as = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[s1], ps[(int64_t)k1 * (kH + 1)], as, 0, 0, 0);
    }
    const float bs = a.b_slf[fc] + a.slf_rgb_bias, bi = a.b_irr[fc] + a.irradiance_bias;
    const int b = f / 3, c = f - 3 * b;
    const float b_f = (float)b;
    const int b_live = fok ? b : -(1 << 29);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = (r & 3) + 8 * (r >> 2) + 4 * h;
      const int lo = __float_as_int(sp[P_LO][i]), hi = __float_as_int(sp[P_HI][i]);
      const bool live = b_live >= lo && b_live <= hi;
      float dzi = 0.0f, dzs = 0.0f;
      if (__builtin_amdgcn_ballot_w64(live) != 0ull) {
        const float w = sp[P_W][i], dmove = sp[P_DIND][i];
        const float tib = sp[P_TIB0 + c][i];
        // the time shift's transpose (shift_map_coordinates): entry b reaches the targets y0 = b + floor(d) and y0 + 1
        // with the weights the targets compute (k_transient_bins' wa, and its wb as seen from the source)
        const float fd = floorf(dmove);
        const int e0 = f + 3 * (int)fminf(fmaxf(fd, -1.0e6f), 1.0e6f);
        const float t = (b_f + fd) - dmove;
        const bool at_b = t == b_f;
        const float wa = at_b ? 1.0f : t - (b_f - 1.0f);
        const float t2 = ((b_f + fd) + 1.0f) - dmove;
        const float wb = 1.0f - (t2 - b_f);
        const float g0 = (unsigned)e0 < (unsigned)kH ? sg[e0] : 0.0f;
        const float g1 = (unsigned)(e0 + 3) < (unsigned)kH ? sg[e0 + 3] : 0.0f;
        const float gsum = wa * g0 + wb * g1;
        const float zi_ = ai[r] + bi, zs_ = as[r] + bs;
        const float spi = softplus_f(zi_), sps = softplus_f(zs_);
        const float ref = fmaxf(sps, 0.0f);
        const float diff_pre = spi * a.indirect_scale, spec_pre = (tib * ref) * a.indirect_scale;
        const float diff = live ? clip0(diff_pre, a.rgb_max) : 0.0f, spec = live ? clip0(spec_pre, a.rgb_max) : 0.0f;
        const float g = w * gsum;
        const float gd = live ? (g * clip_grad(diff_pre, a.rgb_max)) * a.indirect_scale : 0.0f;
        const float gs = live ? (g * clip_grad(spec_pre, a.rgb_max)) * a.indirect_scale : 0.0f;
        const float ref_g = sps > 0.0f ? 1.0f : (sps == 0.0f ? 0.5f : 0.0f);      // clip(softplus, 0, inf)
        dzi = gd * sigmoid_f(zi_);
        dzs = ((gs * tib) * ref_g) * sigmoid_f(zs_);
        dws[r] += gsum * (diff + spec);
        const float dt = gs * ref;
        dtib[0][r] += c == 0 ? dt : 0.0f;
        dtib[1][r] += c == 1 ? dt : 0.0f;
        dtib[2][r] += c == 2 ? dt : 0.0f;
      }
      if (ray_ok) {
        const int ir = (r & 3) + 8 * (r >> 2);
        if (fok) zi[(int64_t)ir * kH + f] = dzi;
        if (f < kRcTdLdSlf) zs[(int64_t)ir * kRcTdLdSlf + f] = fok ? dzs : 0.0f;
      }
    }
  }
  // ---- per-sample sums over the ray's entries (the 32 lanes of a half-wave), in a fixed order
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = (r & 3) + 8 * (r >> 2) + 4 * h;
    const float v0 = half_sum(dws[r]), v1 = half_sum(dtib[0][r]), v2 = half_sum(dtib[1][r]), v3 = half_sum(dtib[2][r]);
    if (fl == 0) { sp[P_DW][i] = v0; sp[P_DT0][i] = v1; sp[P_DT1][i] = v2; sp[P_DT2][i] = v3; }
  }
  __syncthreads();
  if (lane < 32 && ray_ok) {
    const int64_t p = ray * 32 + lane;
    a.d_weights[p] = dir_dw + sp[P_DW][lane];
    a.d_tib[3 * p] = sp[P_DT0][lane]; a.d_tib[3 * p + 1] = sp[P_DT1][lane]; a.d_tib[3 * p + 2] = sp[P_DT2][lane];
  }
}

// ---- the loss family (rc_transient_loss_type) and render_utils.dtof_to_itof ------------------------------------------
// A lane holds the entries e = lane + 64 k of its ray, k < kPerLane.  With lane = 3 b0 + l3 and slot j = k % 3 (known at
// compile time once the k loop is unrolled), entry k is channel (l3 + j) % 3 of bin a[j] + 21 k + k / 3: three per-lane
// values a[j] = b0 + carry(l3 + j) and an immediate.  Sums over the entries are kept per slot and turned by l3 at the end.
struct LaneMap { int l3, a[3]; };

__device__ __forceinline__ LaneMap lane_map(int lane) {
  LaneMap m;
  m.l3 = lane % 3;
  const int b0 = lane / 3;
  m.a[0] = b0; m.a[1] = b0 + (m.l3 == 2 ? 1 : 0); m.a[2] = b0 + (m.l3 >= 1 ? 1 : 0);
  return m;
}
// the bin of entry k; the last k runs past the histogram in the lanes >= kH - 64 (kPerLane - 1): clamped, its value is 0
__device__ __forceinline__ int lane_bin(const LaneMap& m, int k) {
  const int b = m.a[k % 3] + 21 * k + k / 3;
  return k == kPerLane - 1 ? min(b, kB - 1) : b;
}
__device__ __forceinline__ bool lane_entry_ok(int lane, int k) { return lane + 64 * k < kH; }
// per-slot values -> the value of channel c, and per-channel values -> the value of slot j (the three candidates are read
// into values first: a conditional between array elements would index the array by a run-time value and put it in scratch)
__device__ __forceinline__ float pick3(int l3, float v0, float v1, float v2) { return l3 == 0 ? v0 : (l3 == 1 ? v1 : v2); }
__device__ __forceinline__ float slot_to_channel(const float (&t)[3], int l3, int c) {
  return pick3(l3, t[c], t[(c + 2) % 3], t[(c + 1) % 3]);
}
__device__ __forceinline__ float channel_to_slot(const float (&v)[3], int l3, int j) {
  return pick3(l3, v[j], v[(j + 1) % 3], v[(j + 2) % 3]);
}

// I_r(x) of the wave's ray, per channel: sum_b W_r[b] x_b.  w: the row in LDS; x: the lane's entries, 0 past the histogram.
// Per lane the entries of a slot are added in the order of k, then the lanes by wave_total: a fixed order.
__device__ __forceinline__ void itof_row(const float* w, const LaneMap& m, const float (&x)[kPerLane], float (&I)[3]) {
  float t[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) t[k % 3] += w[lane_bin(m, k)] * x[k];
#pragma unroll
  for (int c = 0; c < 3; ++c) I[c] = wave_total(slot_to_channel(t, m.l3, c));
}

// the table to LDS, once per workgroup
__device__ __forceinline__ void stage_itof_table(float* sW, const float* W, int n_rows) {
  for (int i = threadIdx.x; i < n_rows * kB; i += blockDim.x) sW[i] = W[i];
  __syncthreads();
}

// k_transient_loss under every rc_transient_loss_type, with or without use_itof: the same plan and the same outputs.
__global__ __launch_bounds__(kWavesPerBlock * 64) void k_transient_loss_kinds(RcTransLossKindArgs ka) {
  extern __shared__ __attribute__((aligned(16))) float sW[];      // [n_rows][kB]
  __shared__ float sG[kWavesPerBlock][kH];
  const RcTransLossArgs& a = ka.base;
  const int kind = ka.kind;
  const bool itof_kind = kind >= RC_TLOSS_MSE_ITOF;
  const bool unbiased = kind == RC_TLOSS_RAWNERF_TRANSIENT_UNBIASED || kind == RC_TLOSS_MSE_UNBIASED ||
                        kind == RC_TLOSS_MSE_ITOF_UNBIASED || kind == RC_TLOSS_RAWNERF_TRANSIENT_ITOF_UNBIASED;
  const bool rawnerf = kind == RC_TLOSS_RAWNERF_TRANSIENT_UNBIASED || kind == RC_TLOSS_RAWNERF_TRANSIENT ||
                       kind == RC_TLOSS_RAWNERF_TRANSIENT_ITOF || kind == RC_TLOSS_RAWNERF_TRANSIENT_ITOF_UNBIASED;
  const bool gauss_row = kind == RC_TLOSS_RAWNERF_TRANSIENT_UNBIASED || kind == RC_TLOSS_RAWNERF_TRANSIENT;
  const bool rows_used = itof_kind || ka.use_itof != 0;
  if (rows_used) stage_itof_table(sW, ka.W, ka.n_rows);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const LaneMap m = lane_map(lane);
  int64_t ray = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  const bool ray_ok = ray < a.n;
  if (!ray_ok) ray = a.n - 1;
  const float* rgb = a.rgb + ray * kH;
  const float* gt = a.gt + ray * kH;
  const float* rgbn = a.rgb_nocorr ? a.rgb_nocorr + ray * kH : rgb;      // train_utils.py:604-610
  const float* gtn = a.gt_nocorr ? a.gt_nocorr + ray * kH : gt;
  float d[kPerLane], dn[kPerLane];
  // per slot: sum of the clipped colour, of d, of dn, of d dn, of d^2, count of gt > thresh
  float acc[6][3];
#pragma unroll
  for (int q = 0; q < 6; ++q) acc[q][0] = acc[q][1] = acc[q][2] = 0.0f;
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const bool ok = lane_entry_ok(lane, k);
    const int ec = ok ? lane + 64 * k : 0;
    const float r = rgb[ec], g = gt[ec];
    const float dv = ok ? r - g : 0.0f, dnv = ok ? rgbn[ec] - gtn[ec] : 0.0f;
    d[k] = dv; dn[k] = dnv;
    const float cl = td_rawnerf_clip(a, r, g);
    const int j = k % 3;
    acc[0][j] += ok ? cl : 0.0f;
    acc[1][j] += dv;
    acc[2][j] += dnv;
    acc[3][j] += dv * dnv;
    acc[4][j] += dv * dv;
    acc[5][j] += (ok && g > a.thresh) ? 1.0f : 0.0f;
  }
  float tot[6][3];
#pragma unroll
  for (int q = 0; q < 6; ++q)
#pragma unroll
    for (int c = 0; c < 3; ++c) tot[q][c] = wave_total(slot_to_channel(acc[q], m.l3, c));
  // ---- the rows: I_r(d) for the mse stat under use_itof; for the iToF types the loss and sum_r 2 I_r(x) W_r[b]
  float g[kPerLane];
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) g[k] = 0.0f;
  float rows_loss[3] = {0.0f, 0.0f, 0.0f}, rows_mse[3] = {0.0f, 0.0f, 0.0f};
  if (rows_used) {
#pragma unroll 1
    for (int r = 0; r < ka.n_rows; ++r) {
      const float* w = sW + r * kB;
      float Id[3], Ix[3];
      itof_row(w, m, d, Id);
#pragma unroll
      for (int c = 0; c < 3; ++c) rows_mse[c] += Id[c] * Id[c];
      if (itof_kind) {
        if (unbiased) {
          itof_row(w, m, dn, Ix);
#pragma unroll
          for (int c = 0; c < 3; ++c) rows_loss[c] += 2.0f * (Id[c] * Ix[c]);
        } else {
#pragma unroll
          for (int c = 0; c < 3; ++c) { Ix[c] = Id[c]; rows_loss[c] += Id[c] * Id[c]; }
        }
        float A[3], As[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) A[c] = 2.0f * Ix[c];
#pragma unroll
        for (int j = 0; j < 3; ++j) As[j] = channel_to_slot(A, m.l3, j);
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) g[k] += As[k % 3] * w[lane_bin(m, k)];
      }
    }
  }
  const float lm0 = a.lossmult ? a.lossmult[ray] : 1.0f;
  float gmul[3], gadd[3], loss = 0.0f, mse = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float lm = tot[5][c] > 0.0f ? 0.0f : lm0;                       // train_utils.py:586-590
    float s = 1.0f;
    if (rawnerf) {
      const float p = a.exponent == 1.0f ? tot[0][c] : powf(tot[0][c], a.exponent);
      s = 1.0f / (p + a.eps);                                             // train_utils.py:217
    }
    // the gauss constant row of the two per-bin rawnerf types: on every bin gauss sum x (x = dn or d), counted once
    const float sum_x = unbiased ? tot[2][c] : tot[1][c];
    gadd[c] = gauss_row ? a.gauss * sum_x : 0.0f;
    float L;
    if (itof_kind) L = rows_loss[c];
    else if (unbiased) L = 2.0f * tot[3][c] + gadd[c] * tot[1][c];
    else L = tot[4][c] + 0.5f * (gadd[c] * tot[1][c]);
    loss += (lm * (s * L)) * ka.q;
    mse += lm * (ka.use_itof ? rows_mse[c] / (float)ka.n_rows : tot[4][c]);
    gmul[c] = (a.coef * (lm * s)) * ka.q;
  }
  if (ray_ok && lane == 0) { a.loss_ray[ray] = loss; a.loss_ray[a.n + ray] = mse; }
  float gms[3], gas[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) { gms[j] = channel_to_slot(gmul, m.l3, j); gas[j] = channel_to_slot(gadd, m.l3, j); }
  float* sg = sG[wave];
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const int e = lane + 64 * k;
    if (e < kH) {
      const float x = unbiased ? dn[k] : d[k];
      const float v = gms[k % 3] * (itof_kind ? g[k] : 2.0f * x + gas[k % 3]);
      sg[e] = v;
      if (ray_ok) a.G[ray * kH + e] = v;
    }
  }
  __syncthreads();
  td_filter_transpose_row(a, sg, lane, ray_ok ? a.Gt + ray * kH : nullptr);
}

// render_utils.dtof_to_itof: x [n][kB][3] -> out [n][n_rows][3], one wavefront per ray
__global__ __launch_bounds__(kWavesPerBlock * 64) void k_dtof_to_itof(RcDtofToItofArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sW[];      // [n_rows][kB]
  stage_itof_table(sW, a.W, a.n_rows);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const LaneMap m = lane_map(lane);
  int64_t ray = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  const bool ray_ok = ray < a.n;
  if (!ray_ok) ray = a.n - 1;
  const float* x = a.x + ray * kH;
  float v[kPerLane];
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const bool ok = lane_entry_ok(lane, k);
    const float t = x[ok ? lane + 64 * k : 0];
    v[k] = ok ? t : 0.0f;
  }
#pragma unroll 1
  for (int r = 0; r < a.n_rows; ++r) {
    float I[3];
    itof_row(sW + r * kB, m, v, I);
    if (ray_ok && lane == 0) {
      float* o = a.out + (ray * a.n_rows + r) * 3;
      o[0] = I[0]; o[1] = I[1]; o[2] = I[2];
    }
  }
}

constexpr int kItofLdsBytes = (2 * RC_ITOF_MAX_PAIRS + 1) * kB * (int)sizeof(float);

}  // namespace

void rc_launch_transient_loss_kinds(const RcTransLossKindArgs& a, hipStream_t st) {
  if (a.base.n <= 0) return;
  static std::atomic<uint64_t> prepared{0};
  if (rc_first_use_on_device(prepared))
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_transient_loss_kinds), hipFuncAttributeMaxDynamicSharedMemorySize,
                              kItofLdsBytes);
  const bool rows_used = a.kind >= RC_TLOSS_MSE_ITOF || a.use_itof != 0;
  const int lds = rows_used ? a.n_rows * kB * (int)sizeof(float) : 0;
  hipLaunchKernelGGL(k_transient_loss_kinds, dim3((unsigned)((a.base.n + kWavesPerBlock - 1) / kWavesPerBlock)),
                     dim3(kWavesPerBlock * 64), lds, st, a);
}

void rc_launch_dtof_to_itof(const RcDtofToItofArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  static std::atomic<uint64_t> prepared{0};
  if (rc_first_use_on_device(prepared))
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dtof_to_itof), hipFuncAttributeMaxDynamicSharedMemorySize,
                              kItofLdsBytes);
  hipLaunchKernelGGL(k_dtof_to_itof, dim3((unsigned)((a.n + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kWavesPerBlock * 64),
                     a.n_rows * kB * (int)sizeof(float), st, a);
}

void rc_launch_transient_loss(const RcTransLossArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_transient_loss, dim3((unsigned)((a.n + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kWavesPerBlock * 64), 0,
                     st, a);
}

void rc_launch_transient_bins_bwd(const RcTransBinsBwdArgs& a, hipStream_t st) {
  if (a.C <= 0) return;
  hipLaunchKernelGGL(k_transient_bins_bwd, dim3((unsigned)((a.C + kBinsWaves - 1) / kBinsWaves)),
                     dim3(kBinsWaves * 64), 0, st, a);
}
