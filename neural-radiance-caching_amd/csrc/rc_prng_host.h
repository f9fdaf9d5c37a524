// Host-only part of the random numbers (no HIP in this header): Threefry-2x32, jax 0.4.16's split / random_split, and the
// random_split tree of one material-stage forward as a table of rc_prng_segment rows (rc_material_randoms_plan,
// include/rc_abi.h).  The tree is the one ../prng.py material_stage_plan holds, site for site and in the same order; the
// sites are cited there.  rc_api.hip exports it; csrc/prngcheck.cpp compiles the same code for the CPU with
// -fsanitize=address,undefined and tests/test_prngcheck.py compares its tables with the Python plan (`make prngcheck`).
// Like every key path of the package the order of the splits is restated from the source, not pinned against a jax run.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/rc_abi.h"

struct RcKey { uint32_t k0, k1; };

inline uint32_t rc_rotl32_host(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

inline void rc_threefry2x32_host(RcKey key, uint32_t& x0, uint32_t& x1) {
  const uint32_t ks[3] = {key.k0, key.k1, key.k0 ^ key.k1 ^ 0x1BD11BDAu};
  static const int R[2][4] = {{13, 15, 26, 6}, {17, 29, 16, 24}};
  x0 += ks[0];
  x1 += ks[1];
  for (int i = 0; i < 5; ++i) {
    for (int j = 0; j < 4; ++j) {
      x0 += x1;
      x1 = rc_rotl32_host(x1, R[i & 1][j]) ^ x0;
    }
    x0 += ks[(i + 1) % 3];
    x1 += ks[(i + 2) % 3] + (uint32_t)(i + 1);
  }
}

// jax.random.split(key, 2): the counters iota(4) cut in two halves -> blocks (0, 2) and (1, 3); the result
// concat(word0s, word1s) reshaped [2, 2]: first = (a0, b0), second = (a1, b1) with (a, a1) / (b, b1) the blocks' outputs
inline void rc_split_host(RcKey key, RcKey& first, RcKey& second) {
  uint32_t a0 = 0, a1 = 2, b0 = 1, b1 = 3;
  rc_threefry2x32_host(key, a0, a1);
  rc_threefry2x32_host(key, b0, b1);
  first = {a0, b0};
  second = {a1, b1};
}

// internal/utils.py:118-123
inline RcKey rc_first_host(RcKey key) { RcKey a, b; rc_split_host(key, a, b); return a; }
inline RcKey rc_second_host(RcKey key) { RcKey a, b; rc_split_host(key, a, b); return b; }

// Python's round() of a double: half to even (the default rounding mode's nearbyint)
inline int rc_round_half_even(double x) { return (int)nearbyint(x); }

constexpr int64_t RC_PRNG_ALIGN_WORDS = 64;

struct RcPlanBuilder {
  rc_prng_segment* segs;
  int32_t capacity, count = 0;
  bool overflow = false, too_large = false;
  void add(RcKey key, int32_t mode, int32_t id, int64_t n) {
    if (n >= 0xFFFFFFFFll) too_large = true;
    if (count >= capacity) { overflow = true; ++count; return; }
    rc_prng_segment& s = segs[count++];
    s.key[0] = key.k0; s.key[1] = key.k1;
    s.mode = mode; s.id = id;
    s.lo = 0.0f; s.hi = 1.0f;
    s.n = n; s.offset = 0; s.offset2 = -1;
  }
  rc_prng_segment* find(int32_t id) {
    for (int32_t i = 0; i < count && i < capacity; ++i)
      if (segs[i].id == id) return &segs[i];
    return nullptr;
  }
};

// sampler_randoms of ../prng.py: per level one random_split for the jitter, one more for the density MLP
inline void rc_plan_sampler(RcPlanBuilder& b, RcKey rng, int32_t id0, int64_t rays, int32_t n_levels) {
  for (int32_t l = 0; l < n_levels; ++l) {
    RcKey key;
    rc_split_host(rng, key, rng);
    b.add(key, RC_PRNG_MODE_UNIFORM, id0 + l, rays);
    rng = rc_second_host(rng);
  }
}

inline int rc_material_randoms_plan_host(const uint32_t model_key[2], const uint32_t* loss_key, int64_t n, int32_t K,
                                         float diffuse_fraction, int32_t num_vmf, const int32_t* level_samples,
                                         int32_t n_levels, uint32_t flags, rc_prng_segment* segs, int32_t capacity,
                                         int32_t* count, int64_t* arena_words) {
  if (!model_key || !level_samples || !segs || !count || !arena_words) return RC_ERR_INVALID_ARG;
  if (n < 1 || K < 2 || capacity < 0 || n_levels < 1 || n_levels > RC_MAX_LEVELS || num_vmf < 1) return RC_ERR_INVALID_ARG;
  if (flags & ~(RC_PRNG_PLAN_TRAIN | RC_PRNG_PLAN_ENV_SAMPLER | RC_PRNG_PLAN_VMF_NOISE)) return RC_ERR_INVALID_ARG;
  for (int32_t l = 0; l < n_levels; ++l)
    if (level_samples[l] < 1) return RC_ERR_INVALID_ARG;
  const int Kd = rc_round_half_even(K * (double)diffuse_fraction);
  const int Ks = rc_round_half_even(K * (1.0 - (double)diffuse_fraction));
  const int Kc = rc_round_half_even(0.5 * Kd), Kl = Kd - Kc;
  if (Ks + Kd != K || Ks < 0 || Kd < 0) return RC_ERR_UNSUPPORTED;
  if (n > (int64_t)0xFFFFFFFFll / K / level_samples[n_levels - 1] || n > (int64_t)0xFFFFFFFFll / 3 / num_vmf)
    return RC_ERR_INVALID_ARG;                                         // the largest tensors: sec_gumbel, vmf_noise
  const int64_t S = level_samples[n_levels - 1];
  const bool train = flags & RC_PRNG_PLAN_TRAIN, env = flags & RC_PRNG_PLAN_ENV_SAMPLER;
  RcPlanBuilder b{segs, capacity};
  RcKey rng{model_key[0], model_key[1]}, t;

  // -- primary rays' jitter: model_cache_rng (models.py:1156, 1176, 1375), cache_keys()["sampler"] (:710-712)
  t = rc_first_host(rc_first_host(rc_second_host(rng)));
  rc_plan_sampler(b, rc_first_host(t), RC_PRNG_MEMBER_JITTER, n, n_levels);
  rng = rc_second_host(rng);                      // :1156
  rng = rc_second_host(rng);                      // :1177
  RcKey k_samples, k_mat;
  rc_split_host(rng, k_samples, rng);             // :1195
  rng = rc_second_host(rng);                      // :1208
  k_mat = rc_first_host(rng);                     // :1220
  // -- categorical pick of the shading sample: :1417, :1431, :241
  b.add(rc_first_host(rc_first_host(rc_second_host(k_samples))), RC_PRNG_MODE_GUMBEL, RC_PRNG_MEMBER_GUMBEL, n * S);
  if ((flags & RC_PRNG_PLAN_VMF_NOISE) && !env)   // light_sampler.py:135-144: random_split(PRNGKey(1))[0]
    b.add(rc_first_host(RcKey{0u, 1u}), RC_PRNG_MODE_NORMAL, RC_PRNG_MEMBER_VMF_NOISE, n * num_vmf * 3);
  // -- material shader: models.py:1548, shading.py:289, material.py:1971, 1988, 2030, 2535
  t = rc_first_host(rc_first_host(k_mat));
  t = rc_second_host(rc_second_host(t));
  const RcKey k_out = rc_first_host(rc_first_host(t));
  RcKey k_spec, k_diff;
  rc_split_host(k_out, k_spec, t);                // :1383 indirect specular
  k_diff = rc_first_host(t);                      // :1416 indirect diffuse

  // one pass of get_outgoing_radiance: :1642, :1721 get_secondary_rays, :1780 radiance_cache_fn, render_utils.py:962
  struct Pass { RcKey ki, kc; };
  auto one_pass = [](RcKey k_pass) {
    RcKey kh = rc_first_host(k_pass), kh1, r2;
    rc_split_host(kh, kh1, r2);
    return Pass{rc_first_host(kh1), rc_first_host(rc_first_host(r2))};     // kc: material.py:2190
  };
  // the secondary trace of one leg: cache_keys (models.py:712 sampler, 727 resample); the sampler runs on PRNGKey(0)
  // unless train (sampling.py:170-179)
  auto trace = [&](RcKey kc, int Kp, int32_t id_jitter, int32_t id_gumbel) {
    RcKey k_sampler, r, k_resample;
    rc_split_host(kc, k_sampler, r);
    k_resample = rc_first_host(r);
    rc_plan_sampler(b, train ? k_sampler : RcKey{0u, 0u}, id_jitter, n * Kp, n_levels);
    b.add(rc_first_host(k_resample), RC_PRNG_MODE_GUMBEL, id_gumbel, n * Kp * S);      // :241
  };

  const Pass ps = one_pass(k_spec), pd = one_pass(k_diff);
  // importance_sample_rays: per sampler :767 (ka), :324 (the [m, 2] uniform), :784 (the sampler's rng)
  RcKey ka, r3, kb;
  rc_split_host(ps.ki, ka, r3);
  kb = rc_first_host(r3);
  if (env) b.add(rc_first_host(kb), RC_PRNG_MODE_BITS, RC_PRNG_MEMBER_PICKS_KEY_SPEC, 0);          // render_utils.py:215
  else b.add(rc_first_host(ka), RC_PRNG_MODE_UNIFORM, RC_PRNG_MEMBER_SPEC_U, n * Ks * 2);
  trace(ps.kc, Ks, RC_PRNG_MEMBER_SPEC_JITTER, RC_PRNG_MEMBER_SPEC_GUMBEL);
  rc_split_host(pd.ki, ka, r3);
  rc_split_host(r3, kb, r3);
  if (env) {
    b.add(rc_first_host(kb), RC_PRNG_MODE_BITS, RC_PRNG_MEMBER_PICKS_KEY_DIFF, 0);
  } else {
    b.add(rc_first_host(ka), RC_PRNG_MODE_UNIFORM, RC_PRNG_MEMBER_COS_U, n * Kc * 2);
    const RcKey k_light = rc_first_host(rc_second_host(r3));       // second sampler: :767 (skipped), :784
    RcKey kv1, r5, kn;
    rc_split_host(rc_first_host(k_light), kv1, r5);                // render_utils.py:1450, sample_vmf :1407
    b.add(rc_first_host(kv1), RC_PRNG_MODE_GUMBEL, RC_PRNG_MEMBER_VMF_LOBE_GUMBEL, n * num_vmf);   // :1358
    rc_split_host(r5, kn, r5);                                     // :1409
    b.add(kn, RC_PRNG_MODE_NORMAL, RC_PRNG_MEMBER_VMF_V, n * Kl * 2);
    b.add(rc_first_host(r5), RC_PRNG_MODE_UNIFORM, RC_PRNG_MEMBER_VMF_TMP, n * Kl);                // :1413
  }
  trace(pd.kc, Kd, RC_PRNG_MEMBER_DIFF_JITTER, RC_PRNG_MEMBER_DIFF_GUMBEL);
  if (loss_key) {                                 // material_smoothness_noise: train_utils.py:2530, 2541, 2566
    t = rc_second_host(rc_second_host(RcKey{loss_key[0], loss_key[1]}));
    b.add(rc_first_host(t), RC_PRNG_MODE_NORMAL, RC_PRNG_MEMBER_NOISE, n * 3);
  }
  *count = b.count;
  if (b.overflow || b.too_large) return RC_ERR_INVALID_ARG;

  // -- offsets: the members in the order of the structs, each at a multiple of RC_PRNG_ALIGN_WORDS
  int64_t at = 0;
  auto place = [&](int32_t id, bool planes) {
    rc_prng_segment* s = b.find(id);
    if (!s) return;
    s->offset = at;
    if (planes) {
      at = (at + (s->n + 1) / 2 + RC_PRNG_ALIGN_WORDS - 1) / RC_PRNG_ALIGN_WORDS * RC_PRNG_ALIGN_WORDS;
      s->offset2 = at;
      at += s->n / 2;
    } else {
      at += s->n;
    }
    at = (at + RC_PRNG_ALIGN_WORDS - 1) / RC_PRNG_ALIGN_WORDS * RC_PRNG_ALIGN_WORDS;
  };
  // two adjacent segments of one member: [spec | diff]
  auto place_pair = [&](int32_t id_spec, int32_t id_diff) {
    rc_prng_segment *s = b.find(id_spec), *d = b.find(id_diff);
    s->offset = at;
    d->offset = at + s->n;
    at = (d->offset + d->n + RC_PRNG_ALIGN_WORDS - 1) / RC_PRNG_ALIGN_WORDS * RC_PRNG_ALIGN_WORDS;
  };
  for (int32_t l = 0; l < n_levels; ++l) place(RC_PRNG_MEMBER_JITTER + l, false);
  place(RC_PRNG_MEMBER_GUMBEL, false);
  place(RC_PRNG_MEMBER_VMF_NOISE, false);
  place(RC_PRNG_MEMBER_SPEC_U, true);
  place(RC_PRNG_MEMBER_COS_U, true);
  place(RC_PRNG_MEMBER_VMF_LOBE_GUMBEL, false);
  place(RC_PRNG_MEMBER_VMF_V, false);
  place(RC_PRNG_MEMBER_VMF_TMP, false);
  for (int32_t l = 0; l < n_levels; ++l) place_pair(RC_PRNG_MEMBER_SPEC_JITTER + l, RC_PRNG_MEMBER_DIFF_JITTER + l);
  place_pair(RC_PRNG_MEMBER_SPEC_GUMBEL, RC_PRNG_MEMBER_DIFF_GUMBEL);
  place(RC_PRNG_MEMBER_NOISE, false);
  *arena_words = at;
  return RC_OK;
}
