// Driver of tests/test_gpu_halfwave_pairs.py: the half-wave helpers of csrc/rc_dev_sample.h and csrc/rc_dev_mlp.h on one
// wave, beside the functions they stand in for (`make halfwavecheck` in csrc/ -> build/halfwavecheck).
//   halfwavecheck <in> <out>
// <in>, float32:  kChan x 32 channel values (channel c, lane j)  |  kRounds x 2 x 32 arguments (round r: xa[j], then xb[j])
// <out>, float32: kChan sums of wave_sum_n<kChan> on registers whose lanes 32-63 are zeros  |  kChan sums of
//                 wave_sum32_pairs<kChan / 2>  |  per round and lane (64) eight values: softplus_pair's ya, yb, softplus(xa),
//                 softplus(xb), sigmoid_pair's ya, yb, sigmoidf(xa), sigmoidf(xb)
// Both kernels run as one wave of 64 lanes; every index is a compile-time bound of the buffers allocated below.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../neural-radiance-caching_amd/csrc/rc_dev_mlp.h"
#include "../neural-radiance-caching_amd/csrc/rc_dev_sample.h"

namespace {

constexpr int kChan = 34, kRounds = 4, kPerLane = 8;
constexpr size_t kIn = kChan * 32 + kRounds * 2 * 32, kOut = 2 * kChan + kRounds * 64 * kPerLane;

#define CHECK(x)                                                                  \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) {                                                       \
      fprintf(stderr, "halfwavecheck: %s: %s\n", #x, hipGetErrorString(e_));      \
      exit(2);                                                                    \
    }                                                                             \
  } while (0)

__global__ void __launch_bounds__(64) k_sums(const float* __restrict__ in, float* __restrict__ out) {
  const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
  float v[kChan], vp[kChan / 2], tot[kChan];
#pragma unroll
  for (int c = 0; c < kChan; ++c) v[c] = lane < 32 ? in[c * 32 + j] : 0.0f;
#pragma unroll
  for (int k = 0; k < kChan / 2; ++k) vp[k] = in[(2 * k + h) * 32 + j];
  rcdev::wave_sum_n<kChan>(v);
  rcdev::wave_sum32_pairs<kChan / 2>(vp, tot);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < kChan; ++c) { out[c] = v[c]; out[kChan + c] = tot[c]; }
  }
}

__global__ void __launch_bounds__(64) k_pairs(const float* __restrict__ in, float* __restrict__ out) {
  const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
  for (int r = 0; r < kRounds; ++r) {
    const float xa = in[(2 * r) * 32 + j], xb = in[(2 * r + 1) * 32 + j];
    float* o = out + (r * 64 + lane) * kPerLane;
    float ya, yb;
    rcdev::softplus_pair(h, xa, xb, ya, yb);
    o[0] = ya; o[1] = yb; o[2] = rcdev::softplus(xa); o[3] = rcdev::softplus(xb);
    rcdev::sigmoid_pair(h, xa, xb, ya, yb);
    o[4] = ya; o[5] = yb; o[6] = rcdev::sigmoidf(xa); o[7] = rcdev::sigmoidf(xb);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: halfwavecheck <in> <out>\n");
    return 1;
  }
  std::vector<float> in(kIn), out(kOut);
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(in.data(), 4, kIn, f) != kIn || fgetc(f) != EOF) {
    fprintf(stderr, "halfwavecheck: %s does not hold exactly %zu floats\n", argv[1], kIn);
    return 3;
  }
  fclose(f);
  float *d_in = nullptr, *d_out = nullptr;
  CHECK(hipMalloc((void**)&d_in, kIn * sizeof(float)));
  CHECK(hipMalloc((void**)&d_out, kOut * sizeof(float)));
  CHECK(hipMemcpy(d_in, in.data(), kIn * sizeof(float), hipMemcpyHostToDevice));
  CHECK(hipMemset(d_out, 0xff, kOut * sizeof(float)));
  hipLaunchKernelGGL(k_sums, dim3(1), dim3(64), 0, nullptr, d_in, d_out);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  hipLaunchKernelGGL(k_pairs, dim3(1), dim3(64), 0, nullptr, d_in + kChan * 32, d_out + 2 * kChan);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(out.data(), d_out, kOut * sizeof(float), hipMemcpyDeviceToHost));
  CHECK(hipFree(d_in));
  CHECK(hipFree(d_out));
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 4, kOut, f) != kOut || fclose(f)) {
    fprintf(stderr, "halfwavecheck: cannot write %s\n", argv[2]);
    return 3;
  }
  printf("halfwavecheck ok: %d channels, %d rounds\n", kChan, kRounds);
  return 0;
}
