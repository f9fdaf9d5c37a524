// Driver of tests/test_gpu_sample.py: the per-ray kernels of csrc/rc_sample.hip through their launchers on the argument
// structs of a case file, every output buffer written back whole (formats: tests/sample_ref.py).  It calls
// rc_launch_sample_intervals, rc_launch_sample, rc_launch_resample, rc_launch_composite, rc_launch_composite_pick and
// rc_launch_ladder_bounds only, and links the product's own rc_sample.o (`make samplecheck` in csrc/), so the kernels under
// test are the library's objects.
//   samplecheck <cases> <results>     runs every launch in order (null stream, synchronised, hipGetLastError after each);
//                                     the first HIP error ends the run with a non-zero exit and nothing more is launched
// Every buffer is device memory of its own with guard zones, canaries where the case file stores nothing.  A launch's
// pointers are checked against the sizes its counts imply before it runs.  (The case file, the checked view of a launch
// and the main loop: csrc/check_driver.h.)
#define DRIVER_NAME "samplecheck"
#include "../neural-radiance-caching_amd/csrc/check_driver.h"

#include "../neural-radiance-caching_amd/csrc/rc_internal.h"

namespace {

constexpr int64_t kMagicCases = 0x53414D5043415345, kMagicResults = 0x53414D5052534C54;

enum Kernel { K_INTERVALS, K_LEVEL, K_RESAMPLE, K_COMPOSITE, K_PICK, K_LADDER, K_COUNT };

void run(const Launch& L) {
  const int64_t kind = L.rec[0];
  if (kind == K_LADDER) {
    rc_launch_ladder_bounds(L.F(0), L.F(1), L.F(2), L.F(3), L.F(4), L.P(0, 2, true), nullptr);
    return;
  }
  const int64_t n = L.I(0);
  if (n < 1 || n > 4096) die("bad ray count");
  if (kind == K_PICK) {
    rc_launch_composite_pick(n, L.P(0, 3 * n, true), L.P(1, n, true), L.P(2, n, true), L.F(0), L.P(3, 3 * n), L.P(4, n), nullptr);
    return;
  }
  if (kind == K_INTERVALS || kind == K_LEVEL) {
    const int64_t P = L.I(1), S = L.I(2);
    if (P < 1 || P > 64 || S < 2 || S > 64) die("bad bin or sample count");
    if (kind == K_INTERVALS) {
      rc_launch_sample_intervals(L.P(0, n * (P + 1), true), L.P(1, n * P, true), n, (int)P, (int)S, L.P(2, n),
                                 L.P(3, n * (S + 1), true), nullptr);
      return;
    }
    RcSampleArgs a{};
    a.n_rays = n; a.P = (int32_t)P; a.S = (int32_t)S;
    a.secondary = (int32_t)L.I(3); a.use_raydist = (int32_t)L.I(4);
    a.anneal = L.F(0); a.padding = L.F(1); a.raydist_p = L.F(2); a.raydist_premult = L.F(3); a.eps_dot_min = L.F(4);
    a.far_clamp = L.F(5);
    a.origins = L.P(0, 3 * n, true); a.directions = L.P(1, 3 * n, true);
    a.normals = L.P(5, 3 * n);
    a.viewdirs = L.P(2, 3 * n, a.normals != nullptr);
    a.near = L.P(3, n, true); a.far = L.P(4, n, true);
    a.prev_sdist = L.P(6, n * (P + 1));
    if (!a.prev_sdist && P != 1) die("level 0 has one bin");
    a.prev_tdist = L.P(7, n * (P + 1), a.prev_sdist != nullptr);
    a.prev_density = L.P(8, n * P, a.prev_sdist != nullptr);
    a.prev_weights = L.P(9, n * P);
    if (a.prev_weights && !a.prev_sdist) die("no previous level to write weights for");
    a.jitter = L.P(10, n);
    a.sdist = L.P(11, n * (S + 1), true); a.tdist = L.P(12, n * (S + 1), true);
    a.means = L.P(13, 3 * n * S);
    a.s_bounds = L.P(14, 2);
    rc_launch_sample(a, nullptr);
    return;
  }
  const int64_t S = L.I(1);
  if (S < 2 || S > 64) die("bad sample count");
  if (kind == K_RESAMPLE) {
    RcResampleArgs a{};
    a.n_rays = n; a.S = (int32_t)S;
    a.tdist = L.P(0, n * (S + 1), true); a.density = L.P(1, n * S, true); a.directions = L.P(2, 3 * n, true);
    a.gumbel = L.P(3, n * S);
    a.inds_in = L.Pi(4, n, a.gumbel == nullptr);
    a.inds_out = const_cast<int32_t*>(L.Pi(5, n, true));
    a.filt_weight = L.P(6, n, true); a.weights = L.P(7, n * S, true);
    a.acc_out = L.P(8, n);
    a.src_out = const_cast<int32_t*>(L.Pi(9, n));
    a.pts_out = L.P(12, 3 * n);
    a.means = L.P(10, 3 * n * S, a.pts_out != nullptr);
    a.normals = L.P(11, 3 * n * S, a.pts_out != nullptr);
    a.nrm_out = L.P(13, 3 * n, a.pts_out != nullptr);
    if (a.nrm_out && !a.pts_out) die("the gathers come all four or none");
    rc_launch_resample(a, nullptr);
    return;
  }
  if (kind != K_COMPOSITE) die("unknown kernel");
  const int64_t Sf = L.I(2);
  RcCompositeArgs a{};
  a.n_rays = n; a.S = (int32_t)S; a.Sf = (int32_t)Sf;
  a.bg = L.F(0); a.pct[0] = L.F(1); a.pct[1] = L.F(2); a.pct[2] = L.F(3);
  constexpr int kOut0 = 12;
  static const bool scalar[RC_OUT_COUNT] = {false, true, true, true, true, true, false, false, false, false, false,
                                            false, false, false, false, false, false, true, true, false, false};
  for (int o = 0; o < RC_OUT_COUNT; ++o) a.out.ptr[o] = L.P(kOut0 + o, scalar[o] ? n : 3 * n);
  auto want = [&](int id) { return a.out.ptr[id] != nullptr; };
  const bool components = want(RC_OUT_DIRECT_RGB) || want(RC_OUT_INDIRECT_DIFFUSE_RGB) || want(RC_OUT_INDIRECT_SPECULAR_RGB) ||
                          want(RC_OUT_SPECULAR_RGB) || want(RC_OUT_ALBEDO_RGB) || want(RC_OUT_DIFFUSE_RGB) || want(RC_OUT_INDIRECT_RGB);
  const bool positions = components || want(RC_OUT_MEANS) || want(RC_OUT_RAY_DISTS) || want(RC_OUT_LIGHT_DISTS);
  a.inds = L.Pi(9, n, Sf != S);
  a.filt_weight = L.P(10, n, a.inds != nullptr);
  if (!(Sf == S && !a.inds) && !(Sf == 1 && a.inds)) die("Sf is S without a pick, or 1 with one");
  a.directions = L.P(0, 3 * n, true);
  a.origins = L.P(1, 3 * n, components || want(RC_OUT_RAY_DISTS));
  a.lights = L.P(2, 3 * n);
  a.tdist = L.P(3, n * (S + 1), true); a.density = L.P(4, n * S, true);
  a.means = L.P(5, 3 * n * S, positions);
  a.normals_pred = L.P(6, 3 * n * S);
  a.normals_grad = L.P(7, 3 * n * S);
  a.shade = L.P(8, (int64_t)RC_SHADE_CH * n * Sf, components || want(RC_OUT_RGB));
  a.weights = L.P(11, n * S);
  rc_launch_composite(a, nullptr);
}

}  // namespace

int main(int argc, char** argv) { return driver_main(argc, argv, kMagicCases, kMagicResults, K_COUNT, run); }
