// Driver of tests/test_gpu_gemm.py: k_gemm (csrc/rc_data.hip) and k_gemm_tile (csrc/rc_envmap_bwd.hip) through their
// launchers on the descriptors of a case file, every result written back whole (formats: tests/gemm_ref.py).  It calls
// rc_launch_gemm, rc_launch_gemm_tile and rc_launch_sum_parts only, and links the product's own rc_data.o and
// rc_envmap_bwd.o (`make gemmcheck` in csrc/), so the kernels under test are the library's objects.
//   gemmcheck --info                  prints the device's CU count
//   gemmcheck <cases> <results>       runs every case on both launchers (null stream, synchronised, hipGetLastError after
//                                     each); the first HIP error ends the run with a non-zero exit
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "../neural-radiance-caching_amd/csrc/rc_internal.h"

#define CHECK(x)                                                                                   \
  do {                                                                                             \
    hipError_t e_ = (x);                                                                           \
    if (e_ != hipSuccess) {                                                                        \
      fprintf(stderr, "gemmcheck: %s: %s (case %lld)\n", #x, hipGetErrorString(e_), (long long)g_case); \
      exit(2);                                                                                     \
    }                                                                                              \
  } while (0)

namespace {

constexpr int64_t kMagicCases = 0x47454D4D43415345, kMagicResults = 0x47454D4D52534C54;
constexpr int64_t kGuard = 64;
constexpr uint32_t kCanary = 0x7FC0BEEF;
int64_t g_case = -1;

enum Field { F_M, F_N, F_K, F_A_BUF, F_A_OFF, F_SAI, F_SAK, F_B_BUF, F_B_OFF, F_SBK, F_SBJ, F_C_BUF, F_C_OFF, F_SCI, F_SCJ,
             F_BIAS_BUF, F_BIAS_OFF, F_MASK_BUF, F_MASK_OFF, F_SMI, F_SMJ, F_RELU, F_ACC, F_KSLICE, F_SPART, F_KPARTS,
             F_G_BUF, F_G_OFF, F_COUNT };

[[noreturn]] void die(const char* what) {
  fprintf(stderr, "gemmcheck: %s (case %lld)\n", what, (long long)g_case);
  exit(3);
}

struct File {
  std::vector<int64_t> head;               // buffer table, case table
  std::vector<float> data;
  int64_t n_buf = 0, n_case = 0;
  const int64_t* buf(int64_t b) const { return &head[2 * b]; }
  const int64_t* fields(int64_t c) const { return &head[2 * n_buf + F_COUNT * c]; }
};

File read_cases(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) die("cannot open the case file");
  int64_t h[4];
  if (fread(h, 8, 4, f) != 4 || h[0] != kMagicCases || h[3] != F_COUNT || h[1] < 0 || h[2] < 0) die("bad case file header");
  File r;
  r.n_buf = h[1]; r.n_case = h[2];
  r.head.resize(2 * r.n_buf + F_COUNT * r.n_case);
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

// every logical element of an operand lies inside its buffer, guards excluded (strides are not negative)
void inside(const File& fl, int64_t b, int64_t off, int64_t n0, int64_t s0, int64_t n1, int64_t s1) {
  if (b < 0 || b >= fl.n_buf || s0 < 0 || s1 < 0 || off < kGuard) die("descriptor outside its buffer");
  const int64_t ext = (n0 <= 0 || n1 <= 0) ? 0 : (n0 - 1) * s0 + (n1 - 1) * s1 + 1;
  if (off + ext > fl.buf(b)[1] - kGuard) die("descriptor outside its buffer");
}

float* upload(const File& fl, int64_t b) {
  float* d = nullptr;
  const int64_t at = fl.buf(b)[0], len = fl.buf(b)[1];
  CHECK(hipMalloc((void**)&d, len * sizeof(float)));
  if (at >= 0) {
    CHECK(hipMemcpy(d, fl.data.data() + at, len * sizeof(float), hipMemcpyHostToDevice));
  } else {                                 // not stored: canaries alone
    CHECK(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(d), (int)kCanary, len));
  }
  return d;
}

int64_t low4(const void* p) { return p ? (int64_t)(reinterpret_cast<uintptr_t>(p) & 15) : -1; }

}  // namespace

int main(int argc, char** argv) {
  int dev = 0, cus = 0;
  CHECK(hipGetDevice(&dev));
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, dev));
  cus = prop.multiProcessorCount;
  if (argc == 2 && !strcmp(argv[1], "--info")) {
    printf("cus %d\n", cus);
    return 0;
  }
  if (argc != 3) {
    fprintf(stderr, "usage: gemmcheck --info | gemmcheck <cases> <results>\n");
    return 1;
  }
  const File fl = read_cases(argv[1]);
  FILE* out = fopen(argv[2], "wb");
  if (!out) die("cannot open the result file");
  std::vector<int64_t> head(4 + 10 * fl.n_case, -1);
  if (fwrite(head.data(), 8, head.size(), out) != head.size()) die("short write");
  std::vector<float> host;
  const auto t0 = std::chrono::steady_clock::now();
  for (int64_t n = 0; n < fl.n_case; ++n) {
    g_case = n;
    const int64_t* c = fl.fields(n);
    const int64_t M = c[F_M], N = c[F_N], K = c[F_K], kparts = c[F_KPARTS];
    if (M < 0 || N < 0 || K < 0 || kparts < 1 || c[F_SPART] < 0 || c[F_KSLICE] < 0) die("bad sizes");
    inside(fl, c[F_A_BUF], c[F_A_OFF], M, c[F_SAI], K, c[F_SAK]);
    inside(fl, c[F_B_BUF], c[F_B_OFF], K, c[F_SBK], N, c[F_SBJ]);
    inside(fl, c[F_C_BUF], c[F_C_OFF] + (kparts - 1) * c[F_SPART], M, c[F_SCI], N, c[F_SCJ]);
    if (c[F_BIAS_BUF] >= 0) inside(fl, c[F_BIAS_BUF], c[F_BIAS_OFF], N, 1, 1, 0);
    if (c[F_MASK_BUF] >= 0) inside(fl, c[F_MASK_BUF], c[F_MASK_OFF], M, c[F_SMI], N, c[F_SMJ]);
    if (c[F_G_BUF] >= 0) inside(fl, c[F_G_BUF], c[F_G_OFF], c[F_SPART], 1, 1, 0);
    float* da = upload(fl, c[F_A_BUF]);
    float* db = upload(fl, c[F_B_BUF]);
    float* dbias = c[F_BIAS_BUF] >= 0 ? upload(fl, c[F_BIAS_BUF]) : nullptr;
    float* dmask = c[F_MASK_BUF] >= 0 ? upload(fl, c[F_MASK_BUF]) : nullptr;
    for (int which = 0; which < 2; ++which) {
      float* dc = upload(fl, c[F_C_BUF]);                   // a fresh copy of the old C and of the sums per launcher
      float* dg = c[F_G_BUF] >= 0 ? upload(fl, c[F_G_BUF]) : nullptr;
      RcGemmArgs g{};
      g.M = (int)M; g.N = (int)N; g.K = K;
      g.a = da + c[F_A_OFF]; g.sai = c[F_SAI]; g.sak = c[F_SAK];
      g.b = db + c[F_B_OFF]; g.sbk = c[F_SBK]; g.sbj = c[F_SBJ];
      g.c = dc + c[F_C_OFF]; g.sci = c[F_SCI]; g.scj = c[F_SCJ];
      g.bias = dbias ? dbias + c[F_BIAS_OFF] : nullptr;
      g.mask = dmask ? dmask + c[F_MASK_OFF] : nullptr; g.smi = c[F_SMI]; g.smj = c[F_SMJ];
      g.relu = (int)c[F_RELU]; g.accumulate = (int)c[F_ACC];
      g.kslice = c[F_KSLICE]; g.spart = c[F_SPART];
      if (which == 0) rc_launch_gemm(g, (int)kparts, nullptr); else rc_launch_gemm_tile(g, (int)kparts, nullptr);
      CHECK(hipDeviceSynchronize());
      CHECK(hipGetLastError());
      if (dg) {
        rc_launch_sum_parts(g.c, (int)kparts, g.spart, dg + c[F_G_OFF], nullptr);
        CHECK(hipDeviceSynchronize());
        CHECK(hipGetLastError());
      }
      int64_t* al = &head[4 + 10 * n + 5 * which];
      al[0] = low4(g.a); al[1] = low4(g.b); al[2] = low4(g.c); al[3] = low4(g.bias); al[4] = low4(g.mask);
      for (float* d : {dc, dg}) {
        if (!d) continue;
        const int64_t len = fl.buf(d == dc ? c[F_C_BUF] : c[F_G_BUF])[1];
        host.resize(len);
        CHECK(hipMemcpy(host.data(), d, len * sizeof(float), hipMemcpyDeviceToHost));
        if (fwrite(host.data(), 4, len, out) != (size_t)len) die("short write");
        CHECK(hipFree(d));
      }
    }
    for (float* d : {da, db, dbias, dmask})
      if (d) CHECK(hipFree(d));
  }
  const auto t1 = std::chrono::steady_clock::now();
  head[0] = kMagicResults; head[1] = cus; head[2] = fl.n_case;
  head[3] = std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count();
  if (fseek(out, 0, SEEK_SET) || fwrite(head.data(), 8, head.size(), out) != head.size() || fclose(out)) die("short write");
  printf("gemmcheck ok: %lld cases, %d CUs, %.3f s\n", (long long)fl.n_case, cus, head[3] * 1e-6);
  return 0;
}
