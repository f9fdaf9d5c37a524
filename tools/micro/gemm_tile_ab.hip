// k_gemm (rc_data.hip: one wave per 32 x 32 tile, operands straight from global memory) against k_gemm_tile
// (rc_envmap_bwd.hip: 128 x 128 tile per workgroup, operand panels through LDS) on the dense shapes of the EnvMap's
// backward at `rows` rows: the recompute (X W + b, ReLU), the input gradients (dY W^T, masked) and the
// weight gradients (X^T dY over 1024-row K slices + k_sum_parts).  Both kernels run in one process, alternating, each
// launch between its own pair of events; per shape one JSON line: the medians, TFLOP/s and share of the 157 TFLOP/s
// fp32-MFMA peak of both, k_gemm's run-to-run spread (max - min) / median and the largest difference of the results.
// Build (from the repository root):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off tools/micro/gemm_tile_ab.hip \
//     neural-radiance-caching_amd/csrc/rc_data.hip neural-radiance-caching_amd/csrc/rc_envmap_bwd.hip -o tools/micro/gemm_tile_ab
// Run: tools/micro/gemm_tile_ab [rows = 32768] [reps = 20]
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../neural-radiance-caching_amd/csrc/rc_internal.h"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

namespace {

constexpr double kPeak = 157e12;
constexpr int64_t kSlice = 1024;

struct Shape { const char* name; int kind; int in, out; int64_t ldx, ldy; };   // kind 0 fwd, 1 dx, 2 wgrad

float* dev_random(size_t n, unsigned seed) {
  std::vector<float> h(n);
  unsigned s = seed * 2654435761u + 12345u;
  for (size_t i = 0; i < n; ++i) { s = s * 1664525u + 1013904223u; h[i] = ((s >> 8) & 0xffff) / 65536.0f - 0.5f; }
  float* d = nullptr;
  CHECK(hipMalloc((void**)&d, n * sizeof(float)));
  CHECK(hipMemcpy(d, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
  return d;
}

}  // namespace

int main(int argc, char** argv) {
  const int64_t rows = argc > 1 ? atoll(argv[1]) : 32768;
  const int reps = argc > 2 ? atoi(argv[2]) : 20;
  const Shape shapes[] = {
      {"fwd 27->256", 0, 27, 256, 288, 256},   {"fwd 256->256", 0, 256, 256, 256, 256}, {"fwd 283->128", 0, 283, 128, 288, 128},
      {"fwd 128->4", 0, 128, 4, 128, 4},       {"dX 4->128", 1, 128, 4, 128, 4},        {"dX 128->256", 1, 283, 128, 256, 128},
      {"dX 256->256", 1, 256, 256, 256, 256},  {"dW 27x256", 2, 27, 256, 288, 256},     {"dW 256x256", 2, 256, 256, 256, 256},
      {"dW 283x128", 2, 283, 128, 288, 128},   {"dW 128x4", 2, 128, 4, 128, 4}};
  const int64_t Z = (rows + kSlice - 1) / kSlice;
  float* X = dev_random((size_t)rows * 288, 1);
  float* dY = dev_random((size_t)rows * 256, 2);
  float* W = dev_random(283 * 256, 3);
  float* bias = dev_random(256, 4);
  float* out[2];
  const size_t out_n = std::max((size_t)rows * 288, (size_t)Z * 283 * 256);
  for (float*& o : out) { CHECK(hipMalloc((void**)&o, out_n * sizeof(float))); CHECK(hipMemset(o, 0, out_n * sizeof(float))); }
  float* grads[2];
  for (float*& g : grads) { CHECK(hipMalloc((void**)&g, 283 * 256 * sizeof(float))); }
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  std::vector<float> h0, h1;
  for (const Shape& s : shapes) {
    RcGemmArgs g{};
    int parts = 1;
    int64_t count = 0;
    double flop = 0;
    if (s.kind == 0) {
      g.M = (int)rows; g.N = s.out; g.K = s.in; g.a = X; g.sai = s.ldx; g.sak = 1; g.b = W; g.sbk = s.out; g.sbj = 1;
      g.sci = s.ldy; g.scj = 1; g.bias = bias; g.relu = 1; g.kslice = g.K;
      count = rows * s.ldy;
    } else if (s.kind == 1) {
      const int nj = std::min(s.in, 256);
      g.M = (int)rows; g.N = nj; g.K = s.out; g.a = dY; g.sai = s.ldy; g.sak = 1; g.b = W; g.sbk = 1; g.sbj = s.out;
      g.sci = s.ldx; g.scj = 1; g.mask = X; g.smi = 288; g.smj = 1; g.kslice = g.K;
      count = rows * s.ldx;
    } else {
      g.M = s.in; g.N = s.out; g.K = rows; g.a = X; g.sai = 1; g.sak = s.ldx; g.b = dY; g.sbk = s.ldy; g.sbj = 1;
      g.sci = s.out; g.scj = 1; g.kslice = kSlice; g.spart = (int64_t)s.in * s.out;
      parts = (int)Z;
      count = g.spart;
    }
    flop = 2.0 * g.M * g.N * (double)g.K;
    std::vector<float> t[2];
    for (int r = 0; r < reps + 3; ++r)
      for (int which = 0; which < 2; ++which) {
        g.c = out[which];
        if (s.kind == 2) CHECK(hipMemsetAsync(grads[which], 0, count * sizeof(float), nullptr));
        CHECK(hipEventRecord(e0, nullptr));
        if (which == 0) rc_launch_gemm(g, parts, nullptr); else rc_launch_gemm_tile(g, parts, nullptr);
        if (s.kind == 2) rc_launch_sum_parts(out[which], parts, g.spart, grads[which], nullptr);
        CHECK(hipEventRecord(e1, nullptr));
        CHECK(hipEventSynchronize(e1));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 3) t[which].push_back(ms);
      }
    CHECK(hipGetLastError());
    // results: the written C (fwd / dX: every row's N columns), or the summed weight gradient
    const size_t n = s.kind == 2 ? (size_t)count : (size_t)count;
    h0.resize(n); h1.resize(n);
    CHECK(hipMemcpy(h0.data(), s.kind == 2 ? grads[0] : out[0], n * sizeof(float), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h1.data(), s.kind == 2 ? grads[1] : out[1], n * sizeof(float), hipMemcpyDeviceToHost));
    double maxdiff = 0, maxabs = 0;
    for (size_t i = 0; i < n; ++i) { maxdiff = std::max(maxdiff, (double)std::fabs(h0[i] - h1[i])); maxabs = std::max(maxabs, (double)std::fabs(h0[i])); }
    for (auto& v : t) std::sort(v.begin(), v.end());
    const double m0 = t[0][t[0].size() / 2], m1 = t[1][t[1].size() / 2];
    printf("{\"shape\": \"%s\", \"rows\": %lld, \"M\": %d, \"N\": %d, \"K\": %lld, \"gflop\": %.3f, \"k_gemm_ms\": %.4f, "
           "\"k_gemm_tile_ms\": %.4f, \"k_gemm_tflops\": %.2f, \"k_gemm_tile_tflops\": %.2f, \"k_gemm_peak_share\": %.4f, "
           "\"k_gemm_tile_peak_share\": %.4f, \"k_gemm_spread\": %.4f, \"k_gemm_tile_spread\": %.4f, \"flop_floor_ms\": %.5f, "
           "\"max_abs_diff\": %.3e, \"max_abs\": %.3e}\n",
           s.name, (long long)rows, g.M, g.N, (long long)g.K, flop / 1e9, m0, m1, flop / m0 / 1e9, flop / m1 / 1e9,
           flop / m0 / 1e9 / (kPeak / 1e12), flop / m1 / 1e9 / (kPeak / 1e12), (t[0].back() - t[0].front()) / m0,
           (t[1].back() - t[1].front()) / m1, flop / kPeak * 1e3, maxdiff, maxabs);
    fflush(stdout);
  }
  return 0;
}
