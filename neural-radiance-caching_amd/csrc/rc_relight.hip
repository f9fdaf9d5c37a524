// Relighting under an explicit HDR environment image: the image lookup, the image's sampling tables,
// the categorical draw over its texels, the environment sampler of the material stage and the albedo ratio.  Host side:
// rc_relight_host.inc.  No MFMA, no scratch, no float atomics; -ffp-contract=off like the rest of the library.
//
//   k_env_pad      rgb [H][W][3] -> the handle's padded copy [(H+2)][(W+2)][4], border and 4th channel zero
//   k_env_lookup   get_environment_color for n directions (rc_dev_relight.h)
//   k_env_tables_sum / k_env_tables   pmf, pdf, dirs of an image (datasets.py:2113-2154); the normaliser is summed in
//                  double in a fixed order (per-workgroup slots, then every workgroup adds the slots in the same order)
//   k_env_logp     safe_log(pmf) once per bound image: the logits of every later draw
//   k_env_pick     jax.random.categorical over the texels without its noise in memory: the threefry block i yields the
//                  Gumbel values of the flat elements i and i + half, both are used; a wave reduces (score, lowest texel)
//                  and hands ONE 64-bit integer max per pick to memory (order-free, so two runs are bitwise equal)
//   k_env_pick_finish   the integer maxima -> texel indices
//   k_env_sample   EnvironmentSampler.sample_directions + importance_sample_rays as a drop-in for k_brdf_sample
//   k_albedo_ratio albedo <- clip(albedo * ratio, 0, 1) on rows of RC_MAT_CH
#include <hip/hip_runtime.h>

#include "rc_internal.h"
#include "rc_dev_prng.h"
#include "rc_dev_material.h"
#include "rc_dev_relight.h"
#include "rc_dev_reduce.h"

namespace {

__global__ __launch_bounds__(256) void k_env_pad(const float* rgb, int H, int W, float* padded) {
  const int64_t PW = (int64_t)W + 2, total = ((int64_t)H + 2) * PW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / PW, c = i - r * PW;
    float4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (r >= 1 && r <= H && c >= 1 && c <= W) {
      const float* s = rgb + ((r - 1) * W + (c - 1)) * 3;
      v.x = s[0]; v.y = s[1]; v.z = s[2];
    }
    reinterpret_cast<float4*>(padded)[i] = v;
  }
}

__global__ __launch_bounds__(256) void k_env_lookup(RcEnvLookupArgs a) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
    float o[3];
    env_lookup(a.im, a.viewdirs[3 * i], a.viewdirs[3 * i + 1], a.viewdirs[3 * i + 2], o);
    a.out[3 * i] = o[0]; a.out[3 * i + 1] = o[1]; a.out[3 * i + 2] = o[2];
  }
}

// jnp.linspace(lo, hi, n)[i] in fp32: lo (1 - s) + hi s with s = i / (n - 1), the last element hi itself
__device__ __forceinline__ float linspace_at(float lo, float hi, int n, int i) {
  if (n == 1) return lo;
  if (i == n - 1) return hi;
  const float s = (float)i / (float)(n - 1);
  return lo * (1.0f - s) + hi * s;
}
// sin(theta_row): the reference's h_interval is 1 / H, not pi / H (kept; DESIGN.md "Oddities")
__device__ __forceinline__ float env_row_sin(int H, int i) {
  const float hi = 1.0f / (float)H;
  return sinf(linspace_at(0.0f + 0.5f * hi, kEnvPi - 0.5f * hi, H, i));
}
__device__ __forceinline__ float env_intensity(const RcEnvTablesArgs& a, int64_t t) {
  const float* s = a.rgb + 3 * t;
  return (s[0] * a.scale + s[1] * a.scale) + s[2] * a.scale;
}

__global__ __launch_bounds__(256) void k_env_tables_sum(RcEnvTablesArgs a) {
  __shared__ double lds[4];
  const int64_t hw = (int64_t)a.H * a.W;
  double s[1] = {0.0};
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < hw; t += (int64_t)gridDim.x * 256)
    s[0] += (double)(env_intensity(a, t) * env_row_sin(a.H, (int)(t / a.W)));
  block_sums<1>(s, lds, a.part + blockIdx.x);
}

__global__ __launch_bounds__(256) void k_env_tables(RcEnvTablesArgs a, int n_part) {
  __shared__ double lds[kReduceThreads];
  const float total = (float)ordered_sum(a.part, n_part, 1, lds);
  const int64_t hw = (int64_t)a.H * a.W;
  const float lat = kEnvPi / (float)a.H, lng = kEnvTwoPi / (float)a.W;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < hw; t += (int64_t)gridDim.x * 256) {
    const int i = (int)(t / a.W), j = (int)(t - (int64_t)i * a.W);
    const float st = env_row_sin(a.H, i);
    const float pmf = (env_intensity(a, t) * st) / total;
    a.pmf[t] = pmf;
    a.pdf[t] = ((pmf * (float)a.H) * (float)a.W) / (19.7392082f * st);           // 2 pi^2
    const float phi = linspace_at(kEnvPi / 2.0f - 0.5f * lat, -kEnvPi / 2.0f + 0.5f * lat, a.H, i);
    const float th = linspace_at(kEnvPi - 0.5f * lng, -kEnvPi + 0.5f * lng, a.W, j);
    a.dirs[3 * t] = cosf(th) * cosf(phi); a.dirs[3 * t + 1] = sinf(th) * cosf(phi); a.dirs[3 * t + 2] = sinf(phi);
  }
}

// math.safe_log (internal/math.py:177): log(clip(x, tiny, max)); a NaN is handed on
__global__ __launch_bounds__(256) void k_env_logp(const float* pmf, int64_t hw, float* logp) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < hw; t += (int64_t)gridDim.x * 256) {
    const float p = pmf[t];
    logp[t] = logf(p != p ? p : fminf(fmaxf(p, kPrngTiny), RC_FMAX));
  }
}

// (score, texel) as one unsigned 64-bit key whose integer order is "higher score first, then lower texel": the score's
// bits made monotone (a NaN above everything, as argmax takes the first NaN), the texel complemented.  0 = nothing.
__device__ __forceinline__ unsigned long long pick_key(float score, uint32_t texel) {
  uint32_t b = __float_as_uint(score);
  b = score != score ? 0xFFFFFFFFu : ((b & 0x80000000u) ? ~b : (b | 0x80000000u));
  return ((unsigned long long)b << 32) | (unsigned long long)(0xFFFFFFFFu - texel);
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

constexpr int kPickPerThread = 16;                    // texels per thread: a workgroup covers 4096 texels of one pick

// Grid: x = texel tile, y = k1, the pick of a counter block's FIRST word.  Flat element e = k * hw + t of the noise
// [1, T, hw, 1]; n = T hw elements, half = ceil(n / 2) counter blocks.  Block i = k1 hw + t holds the elements i and
// i + half = (k1 + q + carry) hw + (t + r - carry hw) with half = q hw + r: the second word belongs to pick k1 + q or
// k1 + q + 1, the same for a whole wave except around one texel.
__global__ __launch_bounds__(256) void k_env_pick(RcEnvPickArgs a) {
  const uint32_t hw = (uint32_t)a.hw, n = (uint32_t)a.T * hw, half = (n + 1u) >> 1;
  const uint32_t q = half / hw, r = half - q * hw;
  const uint32_t k1 = blockIdx.y;
  unsigned long long best1 = 0, best2 = 0, best3 = 0;    // picks k1, k1 + q, k1 + q + 1
  const uint32_t t0 = blockIdx.x * (256u * kPickPerThread) + threadIdx.x;
#pragma unroll 4
  for (int m = 0; m < kPickPerThread; ++m) {
    const uint32_t t = t0 + 256u * m;
    const uint32_t i = k1 * hw + t;
    if (t >= hw || i >= half) break;
    uint32_t x0 = i, x1 = i + half < n ? i + half : 0u;
    threefry2x32(a.key0, a.key1, x0, x1);
    const float lp = a.logp[t];
    const unsigned long long c1 = pick_key(lp + prng_gumbel(x0), t);
    best1 = c1 > best1 ? c1 : best1;
    if (i + half < n) {
      const bool carry = t + r >= hw;                    // no overflow: t, r < hw <= 2^31 (T = 1: r = half and t < half, so t + r < n)
      const uint32_t t2 = carry ? t + r - hw : t + r;
      const unsigned long long c2 = pick_key(a.logp[t2] + prng_gumbel(x1), t2);
      if (carry) best3 = c2 > best3 ? c2 : best3; else best2 = c2 > best2 ? c2 : best2;
    }
  }
  best1 = wave_max_u64(best1); best2 = wave_max_u64(best2); best3 = wave_max_u64(best3);
  if ((threadIdx.x & 63) == 0) {
    if (best1) atomicMax(a.best + k1, best1);
    if (best2) atomicMax(a.best + k1 + q, best2);
    if (best3) atomicMax(a.best + k1 + q + 1, best3);
  }
}

__global__ __launch_bounds__(256) void k_env_pick_finish(const unsigned long long* best, int T, int32_t* picks) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < T) picks[k] = (int32_t)(0xFFFFFFFFu - (uint32_t)(best[k] & 0xFFFFFFFFull));
}

// One thread per secondary sample, in the order of the trace's batch: [specular block n Ks | diffuse block n Kd].
__global__ __launch_bounds__(256) void k_env_sample(RcEnvSampleArgs a) {
  const int64_t K = a.Ks + a.Kd, nspec = a.n * a.Ks, total = a.n * K;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const bool spec = idx < nspec;
  const int64_t j = spec ? idx : idx - nspec;            // b * Kleg + k: the index the reference's repeat / reshape leaves
  const int Kleg = spec ? a.Ks : a.Kd;
  const int64_t r = j / Kleg;
  const int k = (int)(j - r * Kleg);
  const int32_t* picks = spec ? a.picks_spec : a.picks_diff;
  const int T = spec ? a.T_spec : a.T_diff;
  int64_t p = picks[j % T];
  p = p < 0 ? 0 : (p >= a.hw ? a.hw - 1 : p);
  const V3 nrm = {a.nrm[3 * r], a.nrm[3 * r + 1], a.nrm[3 * r + 2]};
  const Frame f = make_frame(nrm);
  // global_dirs: global_to_local of the texel's direction; the direction traced is local_to_global of that
  const V3 ld = to_local(V3{a.dirs[3 * p], a.dirs[3 * p + 1], a.dirs[3 * p + 2]}, f);
  const V3 g = to_global(ld, f);
  const float pdf = fmaxf(a.pdf[p], 0.0f);               // one sampler in the set: weight 1
  const float weight = ld.z > 0.0f ? 1.0f : 0.0f;        // material.py:1757-1761
  a.sec_origins[3 * idx] = a.pts[3 * r] + nrm.x * a.normal_eps;
  a.sec_origins[3 * idx + 1] = a.pts[3 * r + 1] + nrm.y * a.normal_eps;
  a.sec_origins[3 * idx + 2] = a.pts[3 * r + 2] + nrm.z * a.normal_eps;
  a.sec_dirs[3 * idx] = g.x; a.sec_dirs[3 * idx + 1] = g.y; a.sec_dirs[3 * idx + 2] = g.z;
  a.sec_near[idx] = a.near; a.sec_far[idx] = a.far;
  a.sec_lights[3 * idx] = a.lights ? a.lights[3 * r] : 0.0f;
  a.sec_lights[3 * idx + 1] = a.lights ? a.lights[3 * r + 1] : 0.0f;
  a.sec_lights[3 * idx + 2] = a.lights ? a.lights[3 * r + 2] : 0.0f;
  float* sm = a.samples + (r * K + (spec ? k : a.Ks + k)) * RC_SMP_CH;
  sm[0] = ld.x; sm[1] = ld.y; sm[2] = ld.z; sm[3] = pdf; sm[4] = weight;
  if (spec && k == 0) {
    const V3 lv = to_local(V3{-a.viewdirs[3 * r], -a.viewdirs[3 * r + 1], -a.viewdirs[3 * r + 2]}, f);
    a.local_view[3 * r] = lv.x; a.local_view[3 * r + 1] = lv.y; a.local_view[3 * r + 2] = lv.z;
  }
}

// material.py:2106-2116: albedo <- clip(albedo * ratio, 0, 1) (jnp.clip: a NaN is handed on)
__global__ __launch_bounds__(256) void k_albedo_ratio(float* mat, int64_t n, const float* ratio) {
  const float r[3] = {ratio[0], ratio[1], ratio[2]};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = mat[i * RC_MAT_CH + c] * r[c];
      mat[i * RC_MAT_CH + c] = v != v ? v : fminf(fmaxf(v, 0.0f), 1.0f);
    }
  }
}

unsigned stream_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 2048)); }

}  // namespace

void rc_launch_env_pad(const float* rgb, int H, int W, float* padded, hipStream_t st) {
  hipLaunchKernelGGL(k_env_pad, dim3(stream_blocks(((int64_t)H + 2) * (W + 2))), dim3(256), 0, st, rgb, H, W, padded);
}
void rc_launch_env_lookup(const RcEnvLookupArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_env_lookup, dim3(stream_blocks(a.n)), dim3(256), 0, st, a);
}
int rc_env_tables_blocks(int64_t hw) { return (int)std::max<int64_t>(1, std::min<int64_t>((hw + 255) / 256, 1024)); }
void rc_launch_env_tables(const RcEnvTablesArgs& a, hipStream_t st) {
  const int64_t hw = (int64_t)a.H * a.W;
  const int nb = rc_env_tables_blocks(hw);
  hipLaunchKernelGGL(k_env_tables_sum, dim3((unsigned)nb), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_env_tables, dim3(stream_blocks(hw)), dim3(256), 0, st, a, nb);
}
void rc_launch_env_logp(const float* pmf, int64_t hw, float* logp, hipStream_t st) {
  hipLaunchKernelGGL(k_env_logp, dim3(stream_blocks(hw)), dim3(256), 0, st, pmf, hw, logp);
}
void rc_launch_env_pick(const RcEnvPickArgs& a, hipStream_t st) {
  const int64_t n = (int64_t)a.T * a.hw, half = (n + 1) >> 1;
  const int64_t tile = 256 * kPickPerThread;
  (void)hipMemsetAsync(a.best, 0, sizeof(unsigned long long) * (size_t)a.T, st);
  // the picks whose texels hold a first word: ceil(half / hw) (<= T <= 65535 = the grid's y limit, checked by the caller)
  hipLaunchKernelGGL(k_env_pick, dim3((unsigned)((std::min<int64_t>(a.hw, half) + tile - 1) / tile), (unsigned)((half + a.hw - 1) / a.hw)),
                     dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_env_pick_finish, dim3((unsigned)((a.T + 255) / 256)), dim3(256), 0, st, a.best, a.T, a.picks);
}
void rc_launch_env_sample(const RcEnvSampleArgs& a, hipStream_t st) {
  const int64_t total = a.n * (a.Ks + a.Kd);
  if (total <= 0) return;
  hipLaunchKernelGGL(k_env_sample, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
}
void rc_launch_albedo_ratio(float* mat, int64_t n, const float* ratio, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_albedo_ratio, dim3(stream_blocks(n)), dim3(256), 0, st, mat, n, ratio);
}
