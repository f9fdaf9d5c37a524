// Driver of tests/test_gpu_sample.py: the per-ray kernels of csrc/rc_sample.hip through their launchers on the argument
// structs of a case file, every output buffer written back whole (formats: tests/sample_ref.py).  It calls
// rc_launch_sample_intervals, rc_launch_sample, rc_launch_resample, rc_launch_composite, rc_launch_composite_pick and
// rc_launch_ladder_bounds only, and links the product's own rc_sample.o (`make samplecheck` in csrc/), so the kernels under
// test are the library's objects.
//   samplecheck <cases> <results>     runs every launch in order (null stream, synchronised, hipGetLastError after each);
//                                     the first HIP error ends the run with a non-zero exit and nothing more is launched
// Every buffer is device memory of its own with guard zones, canaries where the case file stores nothing.  A launch's
// pointers are checked against the sizes its counts imply before it runs.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "../neural-radiance-caching_amd/csrc/rc_internal.h"

#define CHECK(x)                                                                                            \
  do {                                                                                                      \
    hipError_t e_ = (x);                                                                                    \
    if (e_ != hipSuccess) {                                                                                 \
      fprintf(stderr, "samplecheck: %s: %s (launch %lld)\n", #x, hipGetErrorString(e_), (long long)g_launch); \
      exit(2);                                                                                              \
    }                                                                                                       \
  } while (0)

namespace {

constexpr int64_t kMagicCases = 0x53414D5043415345, kMagicResults = 0x53414D5052534C54;
constexpr int64_t kGuard = 256;
constexpr uint32_t kCanary = 0x7FC0BEEF;
constexpr int kInts = 8, kFlts = 8, kBufs = 40, kFields = 1 + kInts + kFlts + kBufs;
int64_t g_launch = -1;

enum Kernel { K_INTERVALS, K_LEVEL, K_RESAMPLE, K_COMPOSITE, K_PICK, K_LADDER, K_COUNT };

[[noreturn]] void die(const char* what) {
  fprintf(stderr, "samplecheck: %s (launch %lld)\n", what, (long long)g_launch);
  exit(3);
}

struct File {
  std::vector<int64_t> head;               // buffer table, launch table
  std::vector<float> data;
  int64_t n_buf = 0, n_launch = 0;
  const int64_t* buf(int64_t b) const { return &head[2 * b]; }
  const int64_t* fields(int64_t c) const { return &head[2 * n_buf + kFields * c]; }
};

File read_cases(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) die("cannot open the case file");
  int64_t h[4];
  if (fread(h, 8, 4, f) != 4 || h[0] != kMagicCases || h[3] != kFields || h[1] < 0 || h[2] < 0) die("bad case file header");
  File r;
  r.n_buf = h[1]; r.n_launch = h[2];
  r.head.resize(2 * r.n_buf + kFields * r.n_launch);
  if (fread(r.head.data(), 8, r.head.size(), f) != r.head.size()) die("short case file");
  int64_t total = 0;
  for (int64_t b = 0; b < r.n_buf; ++b) {
    if ((r.buf(b)[0] != total && r.buf(b)[0] != -1) || r.buf(b)[1] < 2 * kGuard) die("bad buffer table");
    if (r.buf(b)[0] >= 0) total += r.buf(b)[1];
  }
  r.data.resize(total);
  if (fread(r.data.data(), 4, total, f) != (size_t)total) die("short case file");
  fclose(f);
  return r;
}

// One launch's view of the case file: integer and float fields, and pointers checked against the size the counts imply.
struct Launch {
  const File& fl;
  const std::vector<float*>& dev;
  const int64_t* rec;
  int64_t I(int j) const { return rec[1 + j]; }
  float F(int j) const {
    const uint32_t bits = (uint32_t)rec[1 + kInts + j];
    float v;
    memcpy(&v, &bits, 4);
    return v;
  }
  bool has(int j) const { return rec[1 + kInts + kFlts + j] >= 0; }
  // the logical floats of slot j (nullptr when the case leaves it out): exactly `need` of them between the guards
  float* P(int j, int64_t need, bool required = false) const {
    const int64_t b = rec[1 + kInts + kFlts + j];
    if (b < 0) {
      if (required) die("a required pointer is missing");
      return nullptr;
    }
    if (b >= fl.n_buf || fl.buf(b)[1] != need + 2 * kGuard) die("a buffer does not have the size its launch implies");
    return dev[b] + kGuard;
  }
  const int32_t* Pi(int j, int64_t need, bool required = false) const { return reinterpret_cast<const int32_t*>(P(j, need, required)); }
};

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

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: samplecheck <cases> <results>\n");
    return 1;
  }
  const File fl = read_cases(argv[1]);
  FILE* out = fopen(argv[2], "wb");
  if (!out) die("cannot open the result file");
  std::vector<float*> dev(fl.n_buf, nullptr);
  int64_t n_out = 0;
  for (int64_t b = 0; b < fl.n_buf; ++b) {
    const int64_t at = fl.buf(b)[0], len = fl.buf(b)[1];
    CHECK(hipMalloc((void**)&dev[b], len * sizeof(float)));
    if (at >= 0) {
      CHECK(hipMemcpy(dev[b], fl.data.data() + at, len * sizeof(float), hipMemcpyHostToDevice));
    } else {                               // an output: canaries alone
      CHECK(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(dev[b]), (int)kCanary, len));
      ++n_out;
    }
  }
  CHECK(hipDeviceSynchronize());
  const auto t0 = std::chrono::steady_clock::now();
  for (int64_t n = 0; n < fl.n_launch; ++n) {
    g_launch = n;
    const Launch L{fl, dev, fl.fields(n)};
    if (L.rec[0] < 0 || L.rec[0] >= K_COUNT) die("unknown kernel");
    run(L);
    CHECK(hipDeviceSynchronize());
    CHECK(hipGetLastError());
  }
  const auto t1 = std::chrono::steady_clock::now();
  const int64_t us = std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count();
  const int64_t head[4] = {kMagicResults, n_out, fl.n_launch, us};
  if (fwrite(head, 8, 4, out) != 4) die("short write");
  std::vector<float> host;
  for (int64_t b = 0; b < fl.n_buf; ++b) {
    if (fl.buf(b)[0] >= 0) continue;
    const int64_t len = fl.buf(b)[1];
    host.resize(len);
    CHECK(hipMemcpy(host.data(), dev[b], len * sizeof(float), hipMemcpyDeviceToHost));
    if (fwrite(host.data(), 4, len, out) != (size_t)len) die("short write");
  }
  if (fclose(out)) die("short write");
  for (float* d : dev) CHECK(hipFree(d));
  printf("samplecheck ok: %lld launches, %lld output buffers, %.3f s\n", (long long)fl.n_launch, (long long)n_out, us * 1e-6);
  return 0;
}
