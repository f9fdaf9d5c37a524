// `make prngcheck`: the material stage's random_split tree (rc_prng_host.h) compiled for the CPU under AddressSanitizer +
// UBSan, without the HIP runtime.  Prints the segment table of every case of tests/test_material_randoms_plan.py:
//   case <n> <K> <train> <env> <loss> <vmf> rc <code> count <rows> words <arena words>
//   seg <id> <mode> <n> <key0> <key1> <offset> <offset2>
// tests/test_prngcheck.py compares them with prng.material_stage_plan.  A sanitizer report makes the program exit non-zero.
#include <stdio.h>

#include <vector>

#include "rc_prng_host.h"

int main() {
  const int64_t ns[4] = {1, 3, 257, 1000};
  const int32_t Ks[4] = {2, 6, 8, 32};
  const int32_t levels[3] = {64, 64, 32};
  const uint32_t loss_key[2] = {0u, 99u};
  for (int c = 0; c < 4; ++c)
    for (uint32_t bits = 0; bits < 16; ++bits) {
      const uint32_t train = bits & 1u, env = (bits >> 1) & 1u, loss = (bits >> 2) & 1u, vmf = (bits >> 3) & 1u;
      const uint32_t key[2] = {0u, (uint32_t)(7 + ns[c])};
      // exactly as many rows as the plan needs (one short first: the call must refuse it and still report the count)
      int32_t count = 0;
      int64_t words = 0;
      std::vector<rc_prng_segment> none(1);
      const uint32_t flags = train * RC_PRNG_PLAN_TRAIN | env * RC_PRNG_PLAN_ENV_SAMPLER | vmf * RC_PRNG_PLAN_VMF_NOISE;
      int rc = rc_material_randoms_plan_host(key, loss ? loss_key : nullptr, ns[c], Ks[c], 0.5f, 128, levels, 3, flags,
                                             none.data(), 0, &count, &words);
      if (rc != RC_ERR_INVALID_ARG || count < 1) { printf("capacity 0 was not refused\n"); return 1; }
      std::vector<rc_prng_segment> segs((size_t)count);
      rc = rc_material_randoms_plan_host(key, loss ? loss_key : nullptr, ns[c], Ks[c], 0.5f, 128, levels, 3, flags, segs.data(),
                                         count - 1, &count, &words);
      if (rc != RC_ERR_INVALID_ARG) { printf("capacity count - 1 was not refused\n"); return 1; }
      rc = rc_material_randoms_plan_host(key, loss ? loss_key : nullptr, ns[c], Ks[c], 0.5f, 128, levels, 3, flags, segs.data(),
                                         (int32_t)segs.size(), &count, &words);
      printf("case %lld %d %u %u %u %u rc %d count %d words %lld\n", (long long)ns[c], Ks[c], train, env, loss, vmf, rc, count,
             (long long)words);
      for (int32_t s = 0; s < count; ++s)
        printf("seg %d %d %lld %u %u %lld %lld\n", segs[s].id, segs[s].mode, (long long)segs[s].n, segs[s].key[0],
               segs[s].key[1], (long long)segs[s].offset, (long long)segs[s].offset2);
    }
  // refusals: K = 5 (Ks + Kd = 2 + 2 with Python's round), null pointers
  const uint32_t key[2] = {1u, 2u};
  rc_prng_segment segs[RC_PRNG_MAX_SEGMENTS];
  int32_t count = 0;
  int64_t words = 0;
  printf("refuse K5 %d\n", rc_material_randoms_plan_host(key, nullptr, 4, 5, 0.5f, 128, levels, 3, 0u, segs, 32, &count, &words));
  printf("refuse null_key %d\n", rc_material_randoms_plan_host(nullptr, nullptr, 4, 8, 0.5f, 128, levels, 3, 0u, segs, 32, &count, &words));
  printf("refuse null_segs %d\n", rc_material_randoms_plan_host(key, nullptr, 4, 8, 0.5f, 128, levels, 3, 0u, nullptr, 32, &count, &words));
  printf("refuse null_count %d\n", rc_material_randoms_plan_host(key, nullptr, 4, 8, 0.5f, 128, levels, 3, 0u, segs, 32, nullptr, &words));
  printf("refuse null_levels %d\n", rc_material_randoms_plan_host(key, nullptr, 4, 8, 0.5f, 128, nullptr, 3, 0u, segs, 32, &count, &words));
  return 0;
}
