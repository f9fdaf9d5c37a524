// What the case-file drivers of the GPU tests share (tests/sample_check.hip, tests/matstage_check.hip, tests/transient_check.hip; formats:
// tests/sample_ref.py).  It lives beside the Makefile so that a driver's target depends on nothing under tests/ but the
// driver's own file.  The case file, one launch's checked view of it, and the main loop.  Every buffer is device memory of
// its own with guard zones, canaries where the case file stores nothing.  The launches run in order on the null stream,
// synchronised, with hipGetLastError after each; the first HIP error ends the run with a non-zero exit and nothing more is
// launched.  Every output buffer is written back whole.
// The including file defines DRIVER_NAME (a string literal) first.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#define CHECK(x)                                                                                             \
  do {                                                                                                       \
    hipError_t e_ = (x);                                                                                     \
    if (e_ != hipSuccess) {                                                                                  \
      fprintf(stderr, DRIVER_NAME ": %s: %s (launch %lld)\n", #x, hipGetErrorString(e_), (long long)g_launch); \
      exit(2);                                                                                               \
    }                                                                                                        \
  } while (0)

namespace {

constexpr int64_t kGuard = 256;
constexpr uint32_t kCanary = 0x7FC0BEEF;
constexpr int kInts = 8, kFlts = 8, kBufs = 40, kFields = 1 + kInts + kFlts + kBufs;
int64_t g_launch = -1;

[[noreturn]] void die(const char* what) {
  fprintf(stderr, DRIVER_NAME ": %s (launch %lld)\n", what, (long long)g_launch);
  exit(3);
}

struct File {
  std::vector<int64_t> head;               // buffer table, launch table
  std::vector<float> data;
  int64_t n_buf = 0, n_launch = 0;
  const int64_t* buf(int64_t b) const { return &head[2 * b]; }
  const int64_t* fields(int64_t c) const { return &head[2 * n_buf + kFields * c]; }
};

File read_cases(const char* path, int64_t magic) {
  FILE* f = fopen(path, "rb");
  if (!f) die("cannot open the case file");
  int64_t h[4];
  if (fread(h, 8, 4, f) != 4 || h[0] != magic || h[3] != kFields || h[1] < 0 || h[2] < 0) die("bad case file header");
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
  // the same floats of slot j as the case file stores them, on the host (what a driver packs or copies into an argument
  // struct before the launch); the slot has to be a stored buffer
  const float* H(int j, int64_t need, bool required = false) const {
    if (!P(j, need, required)) return nullptr;
    const int64_t b = rec[1 + kInts + kFlts + j];
    if (fl.buf(b)[0] < 0) die("a buffer read on the host is not stored in the case file");
    return fl.data.data() + fl.buf(b)[0] + kGuard;
  }
  int64_t B(int j) const { return rec[1 + kInts + kFlts + j]; }
};

int driver_main(int argc, char** argv, int64_t magic_cases, int64_t magic_results, int64_t n_kernels, void (*run)(const Launch&)) {
  if (argc != 3) {
    fprintf(stderr, "usage: " DRIVER_NAME " <cases> <results>\n");
    return 1;
  }
  const File fl = read_cases(argv[1], magic_cases);
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
    if (L.rec[0] < 0 || L.rec[0] >= n_kernels) die("unknown kernel");
    run(L);
    CHECK(hipDeviceSynchronize());
    CHECK(hipGetLastError());
  }
  const auto t1 = std::chrono::steady_clock::now();
  const int64_t us = std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count();
  const int64_t head[4] = {magic_results, n_out, fl.n_launch, us};
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
  printf(DRIVER_NAME " ok: %lld launches, %lld output buffers, %.3f s\n", (long long)fl.n_launch, (long long)n_out, us * 1e-6);
  return 0;
}

}  // namespace
