// Driver of tests/test_gpu_transient_bins.py: the time-resolved cache's per-bin kernels through their launchers on the
// argument structs of a case file, every output buffer written back whole (kernel table and slot order:
// tests/transient_bins_ref.py; formats: tests/sample_ref.py).  It calls rc_launch_shadow_rays, rc_launch_transient_bins,
// rc_launch_transient_slice and rc_launch_transient_bins_bwd only, and links the product's own rc_transient.o,
// rc_transient_slice.o and rc_transient_bwd.o (`make transientcheck` in csrc/: build/transientcheck from the split-form
// objects, build/f32/transientcheck from the RC_SPLIT_MFMA=0 ones), so the kernels under test are the library's objects.
//   transientcheck <cases> <results>   runs every launch in order (null stream, synchronised, hipGetLastError after each);
//                                      the first HIP error ends the run with a non-zero exit and nothing more is launched
// The case file carries the two head layers plain (output_rgba_layer [128][2101] + bias, transient_indirect_layer [64][2100]
// + bias).  k_transient_bins_bwd takes them as they are; for k_transient_bins and k_transient_slice the driver packs them
// with the functions the library packs its own weights with (rc_pack_host.h pack_bins_stream, pack_slice_columns), once per
// distinct set of weight buffers.  The temporal taps and the slice times are case-file buffers.
// Every buffer is device memory of its own with guard zones, canaries where the case file stores nothing.  A launch's
// pointers are checked against the sizes its counts imply before it runs.  (The case file, the checked view of a launch
// and the main loop: csrc/check_driver.h.)
#define DRIVER_NAME "transientcheck"
#include "../neural-radiance-caching_amd/csrc/check_driver.h"

#include "../neural-radiance-caching_amd/csrc/rc_internal.h"
#include "../neural-radiance-caching_amd/csrc/rc_pack_host.h"

namespace {

constexpr int64_t kMagicCases = 0x54524E5343415345, kMagicResults = 0x54524E5352534C54;
constexpr int kBins = kRcTdBins, kHist = kRcTdHist, kTiles = (kHist + 31) / 32;
constexpr int64_t kMaxRays = 64;

enum Kernel { K_SHADOW, K_BINS, K_SLICE, K_BINS_BWD, K_COUNT };
// slots shared by the three per-bin kernels
enum { S_WSLF = 0, S_BSLF, S_WIRR, S_BIRR, S_SLF, S_IRR, S_TSHADE, S_WEIGHTS, S_NEXT };

struct Packed {
  int64_t key[4];
  float* stream; float* col_slf; float* col_irr;
};
std::vector<Packed> g_packs;

float* to_device(const std::vector<float>& v) {
  float* d = nullptr;
  CHECK(hipMalloc((void**)&d, v.size() * sizeof(float)));
  CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  return d;
}

// the packed forms of the head layers in slots [S_WSLF, S_BIRR], built on first use
const Packed& packed(const Launch& L) {
  const float* ws = L.H(S_WSLF, 128 * (kHist + 1), true);
  const float* bs = L.H(S_BSLF, kHist + 1, true);
  const float* wi = L.H(S_WIRR, 64 * kHist, true);
  const float* bi = L.H(S_BIRR, kHist, true);
  const int64_t key[4] = {L.B(S_WSLF), L.B(S_BSLF), L.B(S_WIRR), L.B(S_BIRR)};
  for (const Packed& p : g_packs)
    if (!memcmp(p.key, key, sizeof(key))) return p;
  rcpack::HostLayer slf, irr;
  slf.in = 128; slf.out = kHist + 1; slf.kernel.assign(ws, ws + 128 * (kHist + 1)); slf.bias.assign(bs, bs + kHist + 1);
  irr.in = 64; irr.out = kHist; irr.kernel.assign(wi, wi + 64 * kHist); irr.bias.assign(bi, bi + kHist);
  slf.have_kernel = slf.have_bias = irr.have_kernel = irr.have_bias = true;
  const int frags = rc_transient_bins_frags();
  if (frags % kTiles) die("the bins stream is not a whole number of fragments per tile");
  const std::vector<float> stream = rcpack::pack_bins_stream(slf, irr, kHist, frags / kTiles);
  if ((int64_t)stream.size() != (int64_t)frags * 64) die("bins stream length mismatch");
  Packed p;
  memcpy(p.key, key, sizeof(key));
  p.stream = to_device(stream);
  p.col_slf = to_device(rcpack::pack_slice_columns(slf, 4, kHist, kRcSliceStrideSlf));
  p.col_irr = to_device(rcpack::pack_slice_columns(irr, 2, kHist, kRcSliceStrideIrr));
  g_packs.push_back(p);
  return g_packs.back();
}

// the block RcTransBinsArgs, RcTransSliceArgs and RcTransBinsBwdArgs share: floats 0-7 in the struct's order
void shared_fields(const Launch& L, RcTransIn& a, int64_t n, int64_t thr, int64_t light_zero) {
  if (thr < -(1 << 20) || thr > (1 << 20)) die("bad bin threshold");
  a.n_rays = n;
  a.slf_feat = L.P(S_SLF, n * 64 * 64, true); a.irr_feat = L.P(S_IRR, n * 32 * 64, true);
  a.tshade = L.P(S_TSHADE, RC_TS_COUNT * n * 32, true); a.weights = L.P(S_WEIGHTS, n * 32, true);
  a.exposure = L.F(0); a.shift = L.F(1); a.max_dists = L.F(2); a.irradiance_bias = L.F(3); a.slf_rgb_bias = L.F(4);
  a.indirect_scale = L.F(5); a.rgb_max = L.F(6); a.light_near = L.F(7);
  a.bin_zero_threshold_light = (int32_t)thr; a.light_zero = light_zero != 0;
  if (!(a.exposure > 0.0f)) die("bad exposure");
}

void run(const Launch& L) {
  const int64_t kind = L.rec[0];
  const int64_t n = L.I(0);
  if (kind == K_SHADOW) {
    const int64_t S = L.I(1);
    if (n < 1 || n > 65536 || S < 1 || S > 64) die("bad sample counts");
    RcShadowRayArgs a{};
    a.n = n; a.samples_per_ray = (int32_t)S;
    a.normal_eps = L.F(0); a.shadow_near = L.F(1); a.shadow_far = L.F(2); a.light_near = L.F(3);
    a.means = L.P(0, 3 * n, true); a.normals = L.P(1, 3 * n, true); a.lights = L.P(2, 3 * ((n + S - 1) / S), true);
    a.origins = L.P(3, 3 * n, true); a.dirs = L.P(4, 3 * n, true); a.near = L.P(5, n, true); a.far = L.P(6, n, true);
    a.out_normals = L.P(7, 3 * n, true); a.out_lights = L.P(8, 3 * n, true);
    rc_launch_shadow_rays(a, nullptr);
    return;
  }
  if (n < 1 || n > kMaxRays) die("bad ray count");
  if (kind == K_BINS_BWD) {
    const int64_t r0 = L.I(1), C = L.I(2);
    if (r0 < 0 || C < 1 || r0 + C > n) die("bad chunk");
    RcTransBinsBwdArgs a{};
    shared_fields(L, a, n, L.I(3), L.I(4));
    a.r0 = r0; a.C = C;
    a.w_slf = L.P(S_WSLF, 128 * (kHist + 1), true); a.b_slf = L.P(S_BSLF, kHist + 1, true);
    a.w_irr = L.P(S_WIRR, 64 * kHist, true); a.b_irr = L.P(S_BIRR, kHist, true);
    a.G = L.P(S_NEXT, n * kHist, true); a.Gt = L.P(S_NEXT + 1, n * kHist, true);
    a.dz_irr = L.P(S_NEXT + 2, C * 32 * kHist, true); a.dz_slf = L.P(S_NEXT + 3, C * 32 * kRcTdLdSlf, true);
    a.x_irr = L.P(S_NEXT + 4, C * 32 * 64, true); a.x_slf = L.P(S_NEXT + 5, C * 32 * 128, true);
    a.d_tib = L.P(S_NEXT + 6, n * 32 * 3, true); a.d_direct = L.P(S_NEXT + 7, n * 32 * 3, true);
    a.d_weights = L.P(S_NEXT + 8, n * 32, true);
    rc_launch_transient_bins_bwd(a, nullptr);
    return;
  }
  const int64_t n_taps = L.I(3);
  if (n_taps < 0 || n_taps > 64) die("bad tap count");
  const Packed& pk = packed(L);
  if (kind == K_BINS) {
    RcTransBinsArgs a{};
    shared_fields(L, a, n, L.I(1), L.I(2));
    a.wstream = pk.stream;
    a.n_taps = (int32_t)n_taps; a.taps = L.P(S_NEXT, n_taps, n_taps > 0);
    float** hist[5] = {&a.out_rgb, &a.out_direct, &a.out_indirect, &a.out_ti_diffuse, &a.out_ti_specular};
    float** per_ray[16] = {&a.out_direct_rgb, &a.out_indirect_rgb, &a.out_integrated_rgb, &a.out_diffuse_rgb, &a.out_specular_rgb,
                           &a.out_albedo_rgb, &a.out_occ, &a.out_indirect_occ, &a.out_irradiance_rgb, &a.out_light_radiance_rgb,
                           &a.out_n_dot_l_rgb, &a.out_direct_diffuse_rgb, &a.out_direct_specular_rgb, &a.out_indirect_diffuse_rgb,
                           &a.out_indirect_specular_rgb, &a.out_direct_rgb_viz};
    static_assert(S_NEXT + 1 + 5 + 16 <= kBufs, "the launch record holds every output pointer");
    for (int o = 0; o < 5; ++o) *hist[o] = L.P(S_NEXT + 1 + o, n * kHist);
    for (int o = 0; o < 16; ++o) *per_ray[o] = L.P(S_NEXT + 6 + o, 3 * n);
    rc_launch_transient_bins(a, nullptr);
    return;
  }
  if (kind != K_SLICE) die("unknown kernel");
  const int64_t count = L.I(4);
  if (count < 1 || count > kRcSliceMax) die("bad slice count");
  RcTransSliceArgs a{};
  shared_fields(L, a, n, L.I(1), L.I(2));
  a.w_slf = pk.col_slf; a.w_irr = pk.col_irr;
  a.n_taps = (int32_t)n_taps; a.taps = L.P(S_NEXT, n_taps, n_taps > 0);
  a.count = (int32_t)count;
  const float* t = L.H(S_NEXT + 1, count, true);
  for (int k = 0; k < kRcSliceMax; ++k) {
    a.t[k] = k < count ? t[k] : 0.0f;
    if (!(a.t[k] >= 0.0f && a.t[k] <= (float)(kBins - 1))) die("a slice time outside [0, 699]");
  }
  a.out_rgb = L.P(S_NEXT + 2, n * count * 3); a.out_direct = L.P(S_NEXT + 3, n * count * 3);
  a.out_indirect = L.P(S_NEXT + 4, n * count * 3);
  rc_launch_transient_slice(a, nullptr);
}

}  // namespace

int main(int argc, char** argv) {
  const int rc = driver_main(argc, argv, kMagicCases, kMagicResults, K_COUNT, run);
  for (const Packed& p : g_packs) {
    (void)hipFree(p.stream); (void)hipFree(p.col_slf); (void)hipFree(p.col_irr);
  }
  return rc;
}
