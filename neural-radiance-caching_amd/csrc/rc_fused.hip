// Fused cache forward for primary rays: ONE launch per ray batch, one wavefront per ray.
//
//   3 x [ resample intervals -> cast -> contract -> grid lookup -> density MLP -> alpha weights ]
//   -> appearance grid -> cache shader -> volume compositing
//
// Everything between the ray record and the rendered pixel stays on chip: the step functions and
// sample distances live in a per-wave LDS slice, grid features are written straight into the MFMA
// B-operand slots of the density MLP / shader, the 64-wide hidden feature of the last density MLP is
// already parked where the shader reads it, per-sample colours are composited out of registers.
// The four waves of a workgroup (four rays) march in lockstep through ONE weight stream
// [density MLP 0 | density MLP 1 | density MLP 2 (+ backward fragments) | shader] pulled through the
// LDS ring by LDS-DMA.  Levels 0/1 have 64 samples per ray = two 32-point MFMA tiles per wave, so every
// weight fragment feeds two MFMAs there.
//
// Same arithmetic, in the same order, as the stand-alone kernels (rc_sample.hip, rc_hashgrid.hip,
// rc_mlp.hip), whose reference citations apply; this file only changes where the data lives.  Proposal levels 0 and 1
// are two calls of proposal_level; resample, mean_of, density_of, level2_combine, export_samples and the phases shared
// with the two-wave kernel (analytic_normal, the distance statistics, store3 / store1) are rc_fused_common.h's.
//
// Scalar batches.  One wave per SIMD issues in order, so a scalar load that is waited for right behind its issue is a
// scalar-cache round trip on the ray's chain.  The arguments are therefore laid out by phase (rc_fused_common.h:
// RcResampleRec, RcLookupRec, RcShadeRec -- what ONE phase reads, side by side) and every record is read as a few wide
// s_loads one phase ahead of its use, then named by one empty asm behind the work that covers the loads; the phase uses
// those registers and reads no argument itself:
//   resampling 0 + lookup 0         read at kernel entry, named behind ws_begin's wait and barrier
//   resampling 1 + lookup 1         read behind the last table load of lookup 0, named behind the level-0 density MLP
//   resampling 2 + lookup 2         read behind the last table load of lookup 1, named behind the level-1 density MLP
//   shader and compositing scalars  read in front of lookup 2, named behind the level-2 density MLP's output layer
//   output pointers                 read in front of the compositing's butterfly, named behind it (RC_OUT_PINS)
// (behind the table loads and not in front of the MLP: the first LDS wait of the MLP would close the scalar loads too, the
// two share a counter.)  No scalar load lies between the table loads of a lookup
// (tests/test_fused_scalar_batches_code_objects.py).
//
// Used for the cache pass on primary rays without resampling (BASELINE configs 1, 2, 4); secondary
// rays, resampling and the material stage use the stand-alone kernels.
#include "rc_fused_common.h"
#include <type_traits>

using namespace rcdev;
using namespace rcfused;

namespace {

// act steps [32, 48) of the one-wave kernel: the appearance features, where shader_tile reads them (the two-wave kernel
// still parks them at kAppTmp: its density MLP runs on another layout)
constexpr int kAppSteps = 32;

// Operands of the empty asm statements that pin pointers in scalar registers (one asm statement holding all operands of
// a pin: that is what makes all of them live together): the compositing tail's copies op[] of a.out.ptr[0 .. 18], and the workspace pointers of
// export_samples with the ray count
#define RC_OUT_PINS "s"(op[0]), "s"(op[1]), "s"(op[2]), "s"(op[3]), "s"(op[4]), "s"(op[5]), "s"(op[6]), "s"(op[7]), "s"(op[8]), "s"(op[9]), \
                    "s"(op[10]), "s"(op[11]), "s"(op[12]), "s"(op[13]), "s"(op[14]), "s"(op[15]), "s"(op[16]), "s"(op[17]), "s"(op[18])
#define RC_EXPORT_PINS "s"(a.f_tdist), "s"(a.f_density), "s"(a.f_means), "s"(a.f_normals_pred), "s"(a.n)

// A lookup's record (RcLookupRec) in registers: the K levels' tables and sizes, the hashed levels' masks (a dense level's
// stays the constant 0: its lookup takes none) and the scalars of the proposal level around the lookup.  fetch_lookup
// reads, pin_lookup is the one empty asm that names every value read (K is 6, 7 or 8).
template <int K> struct LookupRegs { const float* table[K]; int32_t size[K]; uint32_t mask[K]; float bbox, precondition, contract_radius, density_bias; };
template <int K>
__device__ __forceinline__ LookupRegs<K> fetch_lookup(const RcLookupRec& q) {
  LookupRegs<K> g;
#pragma unroll
  for (int l = 0; l < K; ++l) { g.table[l] = q.table[l]; g.size[l] = q.size[l]; g.mask[l] = l < kFusedDense ? 0u : q.mask[l]; }
  g.bbox = q.bbox; g.precondition = q.precondition; g.contract_radius = q.contract_radius; g.density_bias = q.density_bias;
  return g;
}
#define RC_LOOKUP_PINS6(g) "s"(g.table[0]), "s"(g.table[1]), "s"(g.table[2]), "s"(g.table[3]), "s"(g.table[4]), "s"(g.table[5]),      \
                           "s"(g.size[0]), "s"(g.size[1]), "s"(g.size[2]), "s"(g.size[3]), "s"(g.size[4]), "s"(g.size[5]),              \
                           "s"(g.mask[3]), "s"(g.mask[4]), "s"(g.mask[5]), "s"(g.bbox), "s"(g.precondition), "s"(g.contract_radius), \
                           "s"(g.density_bias)
static_assert(kFusedDense == 3, "the pins name the masks of levels 3 and up");
template <int K>
__device__ __forceinline__ void pin_lookup(const LookupRegs<K>& g) {
  static_assert(K >= 6 && K <= 8, "RC_LOOKUP_PINS6 and the levels behind it");
  if constexpr (K == 6) asm volatile("" :: RC_LOOKUP_PINS6(g));
  else if constexpr (K == 7) asm volatile("" :: RC_LOOKUP_PINS6(g), "s"(g.table[6]), "s"(g.size[6]), "s"(g.mask[6]));
  else asm volatile("" :: RC_LOOKUP_PINS6(g), "s"(g.table[6]), "s"(g.size[6]), "s"(g.mask[6]), "s"(g.table[7]), "s"(g.size[7]), "s"(g.mask[7]));
}
// the shader's and the tail's record (RcShadeRec) in registers
struct ShadeRegs { ShaderConsts sh; float bg; const float* lights; const float* viewdirs; float pct0, pct1, pct2; };
__device__ __forceinline__ ShadeRegs fetch_shade(const RcShadeRec& q) {
  return ShadeRegs{q.sh, q.bg, q.lights, q.viewdirs, q.pct[0], q.pct[1], q.pct[2]};
}
#define RC_SHADE_PINS(k) "s"(k.sh.roughness_bias), "s"(k.sh.irradiance_bias), "s"(k.sh.ambient_bias), "s"(k.sh.rgb_max), "s"(k.sh.slf_ambient_bias), \
                         "s"(k.bg), "s"(k.lights), "s"(k.viewdirs), "s"(k.pct0), "s"(k.pct1), "s"(k.pct2)

// Density MLP of a proposal level on 64 samples (two point-tiles); returns the raw density of
// sample `lane`.  K grid features of this lane's sample are in f[].
template <int K, int FB, int NF, class WS>
__device__ __forceinline__ float density_level64(const WS& ws, float* act_wave, int lane, const float (&f)[K]) {
  constexpr int KS0 = (K + 1) / 2 + 1;
  using FR = FusedDens<KS0, FB>;
  const int tile = lane >> 5, j = lane & 31, h = lane >> 5;
  // scatter the features into B-operand slots: feature k of point (tile, j) -> step k/2, lane j + 32 (k & 1)
#pragma unroll
  for (int k = 0; k < 2 * (KS0 - 1); ++k)
    act_wave[tile * kTileStride + (k >> 1) * 64 + j + 32 * (k & 1)] = k < K ? f[k < K ? k : 0] : 0.0f;
#pragma unroll
  for (int p = 0; p < 2; ++p) act_wave[p * kTileStride + (KS0 - 1) * 64 + lane] = h == 0 ? 1.0f : 0.0f;
  lds_sync<false>();
  float* act = act_wave + lane;
  f32x16 acc[2][2];
#pragma unroll
  for (int p = 0; p < 2; ++p) { acc[p][0] = zero16(); acc[p][1] = zero16(); }
  mlp_layer_pt<2, 2, KS0, FB + FR::D0, NF>(ws, act, kTileStride, acc);
  // D0 -> D1 in registers (rc_dev_mlp.h BHand): relu(acc) and the bias step of both point-tiles
  BHandPt<2, 2, true> hd;
#pragma unroll
  for (int p = 0; p < 2; ++p) hand_off<2, true>(acc[p], lane, hd.hand[p]);
#pragma unroll
  for (int p = 0; p < 2; ++p) { acc[p][0] = zero16(); acc[p][1] = zero16(); }
  mlp_layer_pth<2, 2, 2, true, FB + FR::D1, NF>(ws, hd, acc);
  float out[2][1], nokeep[1];
  if constexpr (kRcFusedRows) dot_rows<2, 2, 1, FB + FR::DO, NF>(ws, acc, out, nokeep);
  else dot_out<2, 2, 1, FB + FR::DO, NF>(ws, acc, out, nokeep);       // output_density_layer on relu(acc), both point-tiles
  // the dot product is complete on both half-waves: sample `lane` = (tile = lane >> 5, point lane & 31)
  return tile == 0 ? out[0][0] : out[1][0];
}

// Proposal level LEVEL (0, 1) on the 64 intervals in s_td, K grid levels, density MLP at fragment FB: sample mean ->
// contract -> lookup -> density MLP -> the alpha weight of sample `lane`.  Every scalar it reads is in g (fetched one phase
// earlier); fetch_next() issues the scalar loads of the next phase's records behind the lookup's table loads, pin_next()
// names them behind the density MLP.
template <int LEVEL, int K, int FB, int NF, class WS, class FETCH, class PIN>
__device__ __forceinline__ float proposal_level(const LookupRegs<K>& g, const WS& ws, float* act_wave, const Ray& r, const float* s_td, int lane,
                                                unsigned long long* stamps, const FETCH& fetch_next, const PIN& pin_next) {
  float mx, my, mz, t0, t1;
  mean_of(r, s_td, lane, mx, my, mz, t0, t1);
  float cx = mx, cy = my, cz = mz;
  contract3(cx, cy, cz, g.contract_radius);
  float f[K];
  {
    const float ux = unit_box(g.bbox, cx), uy = unit_box(g.bbox, cy), uz = unit_box(g.bbox, cz);
#if defined(RC_ABL) && RC_ABL == 11
    for (int l = 0; l < K; ++l) f[l] = ux * (float)l + uy - uz;
    fetch_next();
#else
    // the cell-table loads of 16 bytes (dense levels) + the corner loads (hashed levels) in flight before the first
    // combine: 6 + 24 on level 0, 6 + 32 on level 1.
    // The kind of level l is the compile-time l < kFusedDense (fused_geometry_ok), never the run-time L.dense: as two arms
    // of a branch that fill the same C[l], the hashed arm is a fall-through successor of the dense one for the compiler's
    // wait-count pass and opened with s_waitcnt vmcnt(0) -- one memory round trip per hashed level instead of one in all
    Corners<1> C[K];
    if constexpr (LEVEL == 0) RC_FSTAMP(12);
#pragma unroll
    for (int l = 0; l < K; ++l) {
      if (l < kFusedDense) grid_fetch_cell(g.table[l], g.size[l], ux, uy, uz, C[l]);
      else grid_fetch<1, true>(g.table[l], g.size[l], g.mask[l], 0u, false, ux, uy, uz, C[l]);
    }
    if constexpr (LEVEL == 0) RC_FSTAMP_NOWAIT(13);
    // the next phase's records behind the last table load: their round trip runs beside the tables' (a wait on LDS in
    // front of the MLP closes scalar loads too -- the two share a counter -- so in front of the MLP they would wait there)
    fetch_next();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int l = 0; l < K; ++l) {
      float v[1], jd[1];
      grid_combine<1, false>(C[l], v, jd);
      f[l] = v[0] * g.precondition;
    }
#endif
  }
  RC_FSTAMP(LEVEL == 0 ? 2 : 5);
#if defined(RC_ABL) && RC_ABL == 13
  const float raw = f[0] + f[K - 1];
#else
  const float raw = density_level64<K, FB, NF>(ws, act_wave, lane, f);
#endif
  pin_next();
  return alpha_weight(density_of(g.density_bias, raw, cx, cy, cz, g.bbox), t0, t1, r.dnorm, true, lane);
}

// FRONT: stop behind the last proposal level (density MLP + appearance lookup) and hand the per-sample results to the
// stages of the time-resolved cache; the stream then ends at F_SH.
// EXPORT: the full kernel that also leaves the last level's per-sample results (fence posts, density, sample means,
// predicted normals) in the workspace buffers of the launch-per-stage plan, for a caller that goes on working per sample
// behind the cache pass (the material stage: its shading-point pick and the material-only composite).
template <bool GRAD, bool FRONT = false, bool EXPORT = false>
__global__ __launch_bounds__(kWaves * 64) void k_cache_fused(RcFusedArgs a) {
  split_exclusive_simd();
  constexpr int NF = FRONT ? F_SH : NF_FUSED;
  extern __shared__ __attribute__((aligned(16))) float lds_dyn[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int64_t ray = (int64_t)blockIdx.x * kWaves + wave;
  const bool ray_ok = ray < a.n;
  if (!ray_ok) ray = a.n - 1;                      // keep the wave in the workgroup's lockstep
  float* ring = lds_dyn;
  float* act_wave = lds_dyn + kRingFloats + wave * (kShActSteps * 64);
  const Scratch s = carve_scratch(lds_dyn + kRingFloats + kWaves * (kShActSteps * 64) + wave * kScratch);
  WStream ws(a.wstream, ring, lane, wave);
#ifdef RC_STAMPS
  unsigned long long stamps[16];
  const unsigned long long rt0 = __builtin_amdgcn_s_memrealtime();
#endif
  RC_FSTAMP(0);
  // the records of the first resampling and the first lookup: their scalar loads go out here, the wait and the barrier of
  // ws_begin cover them
  const ResampleRegs rs0 = fetch_resample(a.rs[0]);
  const LookupRegs<6> g0 = fetch_lookup<6>(a.look[0]);
  __builtin_amdgcn_sched_barrier(0);
  ws_begin<NF>(ws);
  asm volatile("" :: RC_RESAMPLE_PINS(rs0));
  pin_lookup(g0);

  const Ray r = load_ray(a, ray);

  // ------------------------------------------------------------------ level 0 (P = 1, S = 64)
  if (lane == 0) { s.sd[0][0] = 0.0f; s.sd[0][1] = 1.0f; }
  lds_sync<false>();
  resample<FRONT>(a, rs0, r, ray, s, lane, 1, 64, rs0.anneal * safe_log(1.0f + rs0.padding), s.sd[0]);
  RC_FSTAMP(1);
  // the records of level 1 behind the level-0 density MLP, those of level 2 behind the level-1 one
  ResampleRegs rs1, rs2;
  LookupRegs<7> g1;
  LookupRegs<8> g2;
  float w = proposal_level<0, 6, F_L0, NF>(g0, ws, act_wave, r, s.td, lane, RC_FSTAMP_BUF,
                                           [&] { rs1 = fetch_resample(a.rs[1]); g1 = fetch_lookup<7>(a.look[1]); },
                                           [&] { asm volatile("" :: RC_RESAMPLE_PINS(rs1)); pin_lookup(g1); });
  RC_FSTAMP(3);
  for (int e2 = lane; e2 <= 64; e2 += 64) s.sd[1][e2] = s.out[e2];
  lds_sync<false>();
  // ------------------------------------------------------------------ level 1 (P = 64, S = 64)
  resample<FRONT>(a, rs1, r, ray, s, lane, 64, 64, rs1.anneal * safe_log(w + rs1.padding), s.sd[1]);
  RC_FSTAMP(4);
  w = proposal_level<1, 7, F_L1, NF>(g1, ws, act_wave, r, s.td, lane, RC_FSTAMP_BUF,
                                     [&] { rs2 = fetch_resample(a.rs[2]); g2 = fetch_lookup<8>(a.look[2]); },
                                     [&] { asm volatile("" :: RC_RESAMPLE_PINS(rs2)); pin_lookup(g2); });
  RC_FSTAMP(6);
  for (int e2 = lane; e2 <= 64; e2 += 64) s.sd[0][e2] = s.out[e2];
  lds_sync<false>();
  // ------------------------------------------------------------------ level 2 (P = 64, S = 32)
  resample<FRONT>(a, rs2, r, ray, s, lane, 64, 32, rs2.anneal * safe_log(w + rs2.padding), s.sd[0]);
  RC_FSTAMP(7);
  const int j = lane & 31, h = lane >> 5;
  float mx, my, mz, t0, t1;
  mean_of(r, s.td, j, mx, my, mz, t0, t1);
  float cx = mx, cy = my, cz = mz;
  const float zx = rc_div(mx, g2.contract_radius), zy = rc_div(my, g2.contract_radius), zz = rc_div(mz, g2.contract_radius);
  contract3(cx, cy, cz, g2.contract_radius);
  float* act = act_wave + lane;
  // the shader's and the tail's record: in front of the level-2 lookup, whose memory time and the density MLP behind it
  // cover its loads
  ShadeRegs k{};
  if constexpr (!FRONT) k = fetch_shade(a.shade);
  __builtin_amdgcn_sched_barrier(0);
  {
    // half-wave 0 looks up the level-2 density grid, half-wave 1 the appearance grid (same level sizes; bbox /
    // precondition: same for both grids, checked on the host)
    float f[32];
    const float ux = unit_box(g2.bbox, cx), uy = unit_box(g2.bbox, cy), uz = unit_box(g2.bbox, cz);
    // two rounds of four levels: 32 corner loads of 16 bytes in flight per lane
#if defined(RC_ABL) && RC_ABL == 11
    for (int k = 0; k < 32; ++k) f[k] = ux * (float)k + uy - uz;
    if (false)
#endif
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      Corners<4> C[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int l = half * 4 + q;
        // level geometry is identical for the two grids (checked on the host) and so is the entry index: the host keeps
        // a copy of the two tables interleaved entry by entry ([density 16 B | appearance 16 B]), so the two half-waves
        // of a point read the two halves of ONE 32-byte pair -- half the cache-line requests and sector traffic
        grid_fetch<4, true, 2, true>(g2.table[l] + 4 * h, g2.size[l], g2.mask[l], 0u, l < kFusedDense, ux, uy, uz, C[q]);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int l = half * 4 + q;
        float v[4], jd[GRAD ? 12 : 1];
        level2_combine<GRAD>(g2.precondition, C[q], v, jd);
#pragma unroll
        for (int c = 0; c < 4; ++c) f[4 * l + c] = v[c];
        if constexpr (GRAD) level2_jacobian(g2.precondition, g2.size[l], g2.bbox, l, jd, act_wave, j, h);
      }
    }
    // feature k of point j -> step base + k/2, lane j + 32 (k & 1): density features feed D0 at [0,16), appearance
    // features go straight to the shader's steps [kAppSteps, kAppSteps + 16): the level-2 density MLP reads [0, 17),
    // hands D0 -> D1 over in registers and parks its hidden feature at [0, 32) (the fp32 chain in both arithmetics), the
    // backward pass reads the Jacobian at kJac and up -- nothing touches [32, 48) before the shader does
    const int base = h == 0 ? 0 : kAppSteps;
#pragma unroll
    for (int k = 0; k < 32; ++k) act_wave[(base + (k >> 1)) * 64 + j + 32 * (k & 1)] = f[k];
    act[16 * 64] = h == 0 ? 1.0f : 0.0f;
    lds_sync<false>();
  }
  RC_FSTAMP(8);
  // density MLP of the last level on one tile (same code as k_density_mlp<17, GRAD>)
  using FR = FusedDens<17, F_L2>;
  float density, npx, npy, npz, ngx = 0.0f, ngy = 0.0f, ngz = 0.0f;
  {
    f32x16 acc[2];
    acc[0] = zero16(); acc[1] = zero16();
    mlp_layer_d<2, 17, F_L2 + FR::D0, NF>(ws, act, acc);
    uint32_t m0 = 0, m1 = 0;
    if constexpr (GRAD) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) m0 |= (acc[t][r] > 0.0f ? 1u : 0u) << (t * 16 + r);
    }
    {
      BHand<2, true> hd;                        // D0 -> D1 in registers
      hand_off<2, true>(acc, lane, hd);
      acc[0] = zero16(); acc[1] = zero16();
      mlp_layer_dh<2, 2, true, F_L2 + FR::D1, NF>(ws, hd, acc);
    }
    if constexpr (GRAD) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) m1 |= (acc[t][r] > 0.0f ? 1u : 0u) << (t * 16 + r);
    }
    park<2, true>(acc, act, 0);               // hidden feature: stays at [0,32) for the shader
    float out[4], wout[GRAD ? 32 : 1];
    if constexpr (kRcFusedRows) dot_rows1<2, 4, F_L2 + FR::DO, NF, GRAD>(ws, acc, out, wout);
    else dot_out1<2, 4, F_L2 + FR::DO, NF, GRAD>(ws, acc, out, wout);      // density + predicted normals on relu(acc)
    if constexpr (!FRONT) asm volatile("" :: RC_SHADE_PINS(k));
    density = density_of(g2.density_bias, out[0], cx, cy, cz, g2.bbox);
    npx = out[1]; npy = out[2]; npz = out[3];
    neg_normalize(npx, npy, npz);
    if constexpr (GRAD) {
      // the backward pass's B operands are the lane's own registers (masked output weights, masked gradient): the
      // hidden feature at [0, 32) is never displaced
      BHand<2, false> bw;
      bw.one = 0.0f;
#pragma unroll
      for (int s = 0; s < 32; ++s) bw.v[s] = ((m1 >> s) & 1u) ? wout[s] : 0.0f;
      f32x16 g[2];
      g[0] = zero16(); g[1] = zero16();
      mlp_layer_dh<2, 2, false, F_L2 + FR::B1, NF>(ws, bw, g);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) bw.v[t * 16 + r] = ((m0 >> (t * 16 + r)) & 1u) ? g[t][r] : 0.0f;
      f32x16 gf[1];
      gf[0] = zero16();
      mlp_layer_dh<1, 2, false, F_L2 + FR::B0, NF>(ws, bw, gf);
      analytic_normal(gf[0], act_wave, j, h, zx, zy, zz, g2.contract_radius, ngx, ngy, ngz);
    } else if constexpr (!FRONT) {
      // the stream is consumed strictly in order: step the ring over the unused backward fragments
#pragma unroll
      for (int f = F_L2 + FR::B1; f < F_SH; ++f)
        if (f % kChunk == 0) ws_advance<NF>(ws, f / kChunk);
    }
  }
  RC_FSTAMP(9);
  if constexpr (FRONT) {
    // hand-over to the stages behind the sampler, in the layouts of the launch-per-stage front end
    // (the buffer pointers as one batch of scalar loads in front of the first store, as in the compositing tail below)
    asm volatile("" :: RC_EXPORT_PINS, "s"(a.f_normals_grad), "s"(a.f_hbuf), "s"(a.f_app));
    if (ray_ok) {
      const int64_t np = a.n * 32, p = ray * 32 + j;
      export_samples<GRAD>(a, ray, lane, s.td, density, mx, my, mz, npx, npy, npz, ngx, ngy, ngz);
      float* hb = a.f_hbuf + ray * (32 * 64) + lane;
#pragma unroll
      for (int k = 0; k < 32; ++k) hb[k * 64] = act[k * 64];                 // hidden feature, accumulator layout
#pragma unroll
      for (int k = 0; k < 16; ++k) a.f_app[(int64_t)(2 * k + h) * np + p] = act[(kAppSteps + k) * 64];   // feature 2 k + h of point j
    }
    return;
  }
  // ------------------------------------------------------------------ shader on the 32 samples
  act[48 * 64] = h == 0 ? 1.0f : 0.0f;      // the appearance features are at [32, 48) since the level-2 scatter
#if defined(RC_ABL) && RC_ABL == 12
  ShadeOut so;
  for (int c = 0; c < 3; ++c) { so.rgb[c] = act[c * 64]; so.ad[c] = npx; so.idf[c] = npy; so.is[c] = npz; so.tint[c] = density; }
#else
  // (NF_FUSED, which is NF here: FRONT has returned above, and its instantiation of what follows -- never reached -- must not
  // name a stream that ends in front of the shader's row tables, whose reader asserts that its block lies inside the stream)
  const ShadeOut so = shader_tile<F_SH, NF_FUSED, WStream, FusedShader>(ws, act, lane, h, npx, npy, npz, k.viewdirs[3 * ray], k.viewdirs[3 * ray + 1],
                                            k.viewdirs[3 * ray + 2], k.sh);
#endif

  RC_FSTAMP(10);
  // ------------------------------------------------------------------ volume compositing (k_composite)
  const bool act_s = lane < 32;
  const float wnf = alpha_weight(density, t0, t1, r.dnorm, act_s, lane);
  // The output pointers the tail stores through, fetched as ONE batch of scalar loads in front of the sums: read where
  // they are used, each store opened with its own s_load, a wait for it and a branch -- a scalar-cache round trip per
  // output on the ray's chain.  The loads go out here (fence below), the values are pinned in scalar registers by the
  // empty asm behind the butterfly, whose vector work covers their latency; the stores then find them there.
  constexpr int kOutPtrs = RC_OUT_LIGHT_DISTS + 1;     // every output of the primary-ray pass: ids [0, kOutPtrs)
  float* op[kOutPtrs];
#pragma unroll
  for (int i = 0; i < kOutPtrs; ++i) op[i] = a.out.ptr[i];
  if constexpr (EXPORT) {
    // its stores open a block of their own, behind which the loads above would sink: pinned in front of it, with the
    // workspace pointers
    asm volatile("" :: RC_EXPORT_PINS, RC_OUT_PINS);
  }
  __builtin_amdgcn_sched_barrier(0);
  // (EXPORT) the last level's per-sample results, behind the shader: every value is still live for the compositing, and
  // no scalar load of the shader then falls between the kernel's first and last store
  if constexpr (EXPORT) {
    if (ray_ok) export_samples<false>(a, ray, lane, s.td, density, mx, my, mz, npx, npy, npz, ngx, ngy, ngz);
  }
  const bool st = lane == 0 && ray_ok;      // store3 / store1 of the ray's outputs
  // every weighted sum of the ray in one batched butterfly
  enum { V_ACC = 0, V_RGB = 1, V_AD = 4, V_IDF = 7, V_IS = 10, V_TINT = 13, V_DIF = 16, V_IND = 19, V_MEAN = 22, V_RD = 25,
         V_LD = 26, V_NP = 27, V_NG = 30, V_LOGT = 33, V_COUNT = 34 };
  // The 32 samples sit on lanes 0-31 and every factor below is the same on lanes j and j + 32, so two channels share a
  // register: channel 2 k on the lower half-wave, 2 k + 1 on the upper one, both weighted with the lower half's wnf
  // (wave_sum32_pairs: 17 registers and 5 steps instead of 34 and 6, each sum in k_composite's order).
  static_assert(V_COUNT % 2 == 0, "channels are reduced in pairs");
  float x[V_COUNT];
  x[V_ACC] = 1.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    x[V_RGB + c] = so.rgb[c];
    x[V_AD + c] = so.ad[c];
    x[V_IDF + c] = so.idf[c];
    x[V_IS + c] = so.is[c];
    x[V_TINT + c] = so.tint[c];
    x[V_DIF + c] = so.ad[c] + so.idf[c];
    x[V_IND + c] = so.idf[c] + so.is[c];
  }
  x[V_MEAN] = mx; x[V_MEAN + 1] = my; x[V_MEAN + 2] = mz;
  x[V_RD] = sqrtf((r.ox - mx) * (r.ox - mx) + (r.oy - my) * (r.oy - my) + (r.oz - mz) * (r.oz - mz));
  x[V_LD] = 0.0f;
  if (k.lights) {
    const float lx = k.lights[3 * ray], ly = k.lights[3 * ray + 1], lz = k.lights[3 * ray + 2];
    x[V_LD] = sqrtf((lx - mx) * (lx - mx) + (ly - my) * (ly - my) + (lz - mz) * (lz - mz));
  }
  x[V_NP] = npx; x[V_NP + 1] = npy; x[V_NP + 2] = npz;
  x[V_NG] = ngx; x[V_NG + 1] = ngy; x[V_NG + 2] = ngz;
  x[V_LOGT] = logf(0.5f * (t0 + t1));
  float wnf2 = wnf, wnf_hi = wnf;
  swap_halves(wnf2, wnf_hi);                    // wnf2: lanes 32-63 take the weights of lanes 0-31
  float vp[V_COUNT / 2], v[V_COUNT];
#pragma unroll
  for (int k = 0; k < V_COUNT / 2; ++k) vp[k] = wnf2 * (h ? x[2 * k + 1] : x[2 * k]);
  wave_sum32_pairs<V_COUNT / 2>(vp, v);
  // all pointers are in scalar registers here: one wait for the batch, and the stores below use these values
  static_assert(kOutPtrs == 19, "RC_OUT_PINS names every pointer");
  asm volatile("" :: RC_OUT_PINS);
  __builtin_amdgcn_sched_barrier(0);
  const float accw = v[V_ACC];
  const float bgw = fmaxf(0.0f, 1.0f - accw) * k.bg;
  store3(op[RC_OUT_RGB], st, ray, v[V_RGB] + bgw, v[V_RGB + 1] + bgw, v[V_RGB + 2] + bgw);
  store3(op[RC_OUT_DIRECT_RGB], st, ray, v[V_AD], v[V_AD + 1], v[V_AD + 2]);
  store3(op[RC_OUT_INDIRECT_DIFFUSE_RGB], st, ray, v[V_IDF], v[V_IDF + 1], v[V_IDF + 2]);
  store3(op[RC_OUT_INDIRECT_SPECULAR_RGB], st, ray, v[V_IS], v[V_IS + 1], v[V_IS + 2]);
  store3(op[RC_OUT_SPECULAR_RGB], st, ray, v[V_IS], v[V_IS + 1], v[V_IS + 2]);
  store3(op[RC_OUT_ALBEDO_RGB], st, ray, v[V_TINT], v[V_TINT + 1], v[V_TINT + 2]);
  store3(op[RC_OUT_DIFFUSE_RGB], st, ray, v[V_DIF], v[V_DIF + 1], v[V_DIF + 2]);
  store3(op[RC_OUT_INDIRECT_RGB], st, ray, v[V_IND], v[V_IND + 1], v[V_IND + 2]);
  store3(op[RC_OUT_INDIRECT_OCC], st, ray, accw, accw, accw);
  store1(op[RC_OUT_ACC], st, ray, accw);
  store3(op[RC_OUT_MEANS], st, ray, v[V_MEAN], v[V_MEAN + 1], v[V_MEAN + 2]);
  store1(op[RC_OUT_RAY_DISTS], st, ray, v[V_RD]);
  if (k.lights) store1(op[RC_OUT_LIGHT_DISTS], st, ray, v[V_LD]);
  store3(op[RC_OUT_NORMALS_PRED], st, ray, v[V_NP], v[V_NP + 1], v[V_NP + 2]);
  if constexpr (GRAD) store3(op[RC_OUT_NORMALS], st, ray, v[V_NG], v[V_NG + 1], v[V_NG + 2]);
  store1(op[RC_OUT_DISTANCE_MEAN], st, ray, distance_mean(v[V_LOGT], accw, s.td));
  // (by value: a conditional on the members themselves selects their address and loads per lane, rc_dev_grid.h pick_half)
  const float pct0 = k.pct0, pct1 = k.pct1, pct2 = k.pct2;
  distance_percentiles([=](int i) { return pick_half(i, pct0, pick_half(i - 1, pct1, pct2)); }, ray, ray_ok, lane, wnf, accw, s.td, s.cw, op[RC_OUT_DISTANCE_PERCENTILE_5], op[RC_OUT_DISTANCE_MEDIAN],
                       op[RC_OUT_DISTANCE_PERCENTILE_95]);
  RC_FSTAMP(11);
#ifdef RC_STAMPS
  if (lane == 0 && a.stamps && ray_ok) {
    unsigned long long* d = a.stamps + ray * 16;
    for (int i = 0; i < 12; ++i) d[i] = stamps[i];
    d[14] = rt0; d[15] = __builtin_amdgcn_s_memrealtime();
    d[12] = stamps[12]; d[13] = stamps[13];
  }
#endif
}

}  // namespace

#ifdef RC_STAMPS
static unsigned long long* g_fused_stamps = nullptr;
extern "C" void* rc_debug_fused_stamps() { return g_fused_stamps; }
#endif

__global__ void k_build_cells(const float* __restrict__ src, int N, int F, float* __restrict__ dst, int dst_stride, int dst_off) {
  const int M = N + 3;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (int64_t)M * M * M * 8;
  if (i >= total) return;
  int64_t e;
  const bool inside = rc_cell_corner(N, i, &e);      // rc_pack_host.h (the same rule runs under the CPU sanitizers)
  for (int f = 0; f < F; ++f) dst[i * dst_stride + dst_off + f] = inside ? src[e * F + f] : 0.0f;
}

void rc_launch_build_cells(const float* src, int N, int F, float* dst, int dst_stride, int dst_off, hipStream_t stream) {
  const int64_t total = (int64_t)(N + 3) * (N + 3) * (N + 3) * 8;
  hipLaunchKernelGGL(k_build_cells, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, src, N, F, dst, dst_stride, dst_off);
}

int rc_fused_stream_offsets(int* l0, int* l1, int* l2, int* sh) {
  *l0 = F_L0; *l1 = F_L1; *l2 = F_L2; *sh = F_SH;
  return NF_FUSED;
}

void rc_launch_fused(const RcFusedLaunch& L, hipStream_t stream) {
  if (L.n <= 0) return;
  static std::atomic<uint64_t> prepared{0};
  const int lds = (kRingFloats + kWaves * (kShActSteps * 64 + kScratch)) * (int)sizeof(float);
  // the six instantiations, by [GRAD][form]
  enum { kPlain = 0, kFront = 1, kExport = 2 };
  using Kernel = void (*)(RcFusedArgs);
  static const Kernel kernels[2][3] = {
      {k_cache_fused<false>, k_cache_fused<false, true>, k_cache_fused<false, false, true>},
      {k_cache_fused<true>, k_cache_fused<true, true>, k_cache_fused<true, false, true>}};
  if (rc_first_use_on_device(prepared)) {
    for (int g = 0; g < 2; ++g)
      for (int f = 0; f < 3; ++f)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernels[g][f]), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  }
  RcFusedArgs a{};
  a.origins = L.rays.origins; a.directions = L.rays.directions; a.near = L.rays.near; a.far = L.rays.far; a.n = L.n;
  // the per-phase records (rc_fused_common.h), from the same fields as the arrays behind them
  for (int l = 0; l < 3; ++l) a.rs[l] = RcResampleRec{L.jitter[l], make_uspec(L.num_samples[l], L.jitter[l] != nullptr), L.anneal, L.padding};
  for (int g = 0; g < 3; ++g) {
    RcLookupRec& q = a.look[g];
    for (int l = 0; l < RC_MAX_GRID_LEVELS; ++l) {
      const RcGridLevel& lv = L.grid[g]->lvl[l];
      q.table[l] = g == 2 ? L.pair_table[l] : (l < kFusedDense ? L.cell_table[g][l] : lv.table);
      q.size[l] = lv.size; q.mask[l] = lv.mask;
    }
    q.bbox = L.grid[g]->bbox; q.precondition = L.grid[g]->precondition; q.contract_radius = L.contract_radius; q.density_bias = L.density_bias;
  }
  a.shade.sh = ShaderConsts{L.roughness_bias, L.irradiance_bias, L.ambient_bias, L.rgb_max, L.slf_ambient_bias};
  a.shade.bg = L.bg; a.shade.density_bias = L.density_bias; a.shade.contract_radius = L.contract_radius;
  a.shade.lights = L.rays.lights; a.shade.viewdirs = L.rays.viewdirs;
  for (int i = 0; i < 3; ++i) a.shade.pct[i] = L.pct[i];
  for (int g = 0; g < 4; ++g) a.grid[g] = *L.grid[g];
  for (int l = 0; l < RC_MAX_GRID_LEVELS; ++l) {
    a.pair_table[l] = L.pair_table[l];
    a.cell_table[0][l] = L.cell_table[0][l]; a.cell_table[1][l] = L.cell_table[1][l];
  }
  a.wstream = L.wstream; a.ide_coef = L.ide_coef;
  a.out = L.out;
#ifdef RC_STAMPS
  {
    static unsigned long long* buf = nullptr; static int64_t cap = 0;
    // 2 x: the two-wave kernel keeps the stamps of a ray's second wave at [n + ray]
    if (cap < L.n) { if (buf) (void)hipFree(buf); (void)hipMalloc((void**)&buf, (size_t)L.n * 2 * 16 * 8); cap = L.n; }
    a.stamps = buf; g_fused_stamps = buf;
  }
#endif
  dim3 grid((unsigned)((L.n + kWaves - 1) / kWaves)), block(kWaves * 64);
  if (L.front || L.export_samples) {
    a.f_tdist = L.f_tdist; a.f_density = L.f_density; a.f_means = L.f_means; a.f_normals_pred = L.f_normals_pred;
  }
  if (L.front) {
    a.use_raydist = L.use_raydist; a.raydist_p = L.raydist_p; a.raydist_premult = L.raydist_premult;
    a.y_max = L.raydist_p < 0.0f ? nextafterf((L.raydist_p - 1.0f) / L.raydist_p, -INFINITY) : 0.0f;       // as rc_launch_sample
    a.f_normals_grad = L.want_grad ? L.f_normals_grad : nullptr; a.f_hbuf = L.f_hbuf; a.f_app = L.f_app;
  }
  const bool grad = L.front ? L.want_grad != 0 : L.out.ptr[RC_OUT_NORMALS] != nullptr;
#if RC_TEAM_KERNEL
  if (!L.front && L.team) {        // the two-wave kernel exports by itself where a.f_density is set
    a.prio_mode = L.prio_mode;
    rc_launch_fused_team(a, grad, stream);
    return;
  }
#endif
  const int form = L.front ? kFront : (L.export_samples && !L.team ? kExport : kPlain);
  hipLaunchKernelGGL(kernels[grad][form], grid, block, lds, stream, a);
}
