"""Counter-based random numbers with the stream layout of the reference's `jax.random`.

The reference pins jax==0.4.16 (requirements.txt:2), whose default PRNG is threefry2x32 with raw uint32[2] keys
and the *non-partitionable* counter layout.  jax is not part of /root/reference, so this module restates the
published algorithm (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11: Threefry-2x32, 20 rounds)
and jax 0.4.16's conventions on top of it:

  PRNGKey(seed)          key = [seed >> 32, seed & 0xffffffff]
  threefry over counts   counts.ravel() is cut in two halves; element i of the first half and element i of the
                         second half are the two words of block i (an odd count is padded with one 0 and the last
                         output dropped); the result is concat(out_word0, out_word1)
  split(key, n)          counts = iota(2 n), result reshaped [n, 2]
  fold_in(key, d)        one block with counter PRNGKey(d)
  random_bits(key, shp)  counts = iota(prod(shp))
  uniform                mantissa trick: (bits >> 9 | 0x3f800000) as float - 1, then *(max-min)+min, max(min, .)
  normal                 sqrt(2) * erfinv(uniform(nextafter(-1, 0), 1)), erfinv = XLA's single-precision
                         polynomial (Giles, "Approximating the erfinv function")
  gumbel / categorical   -log(-log(uniform(tiny, 1))); argmax(gumbel + logits)

Pinned by the published known-answer values of Random123 and of the jax documentation (tests/golden/prng_kat.json,
tests/test_prng.py).  What CANNOT be checked in this container is the reference's *call order* end to end (no jax
here): `cache_pass_randoms` follows the `utils.random_split` sites cited in its docstring, read from the source.

Bits, keys and uniforms are integer / exactly-rounded float arithmetic and therefore bit-exact with jax; `normal` and
`gumbel` go through log/log1p/sqrt, which differ between XLA back ends by an ulp as well.

The device twin is rc_prng_fill (csrc/rc_prng.hip, include/rc_abi.h): same counter layout, filled in HBM.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np

_ROT = ((13, 15, 26, 6), (17, 29, 16, 24))
_PARITY = np.uint32(0x1BD11BDA)

MODE_BITS, MODE_UNIFORM, MODE_NORMAL, MODE_GUMBEL = 0, 1, 2, 3


def _rotl(x, r):
    return (x << np.uint32(r)) | (x >> np.uint32(32 - r))


def threefry2x32(key, x0, x1) -> Tuple[np.ndarray, np.ndarray]:
    """Threefry-2x32, 20 rounds, on arrays of counter words (x0, x1) under one key (k0, k1)."""
    k0, k1 = np.uint32(key[0]), np.uint32(key[1])
    ks = (k0, k1, np.uint32(k0 ^ k1 ^ _PARITY))
    x0 = np.array(x0, dtype=np.uint32, copy=True)
    x1 = np.array(x1, dtype=np.uint32, copy=True)
    with np.errstate(over="ignore"):
        x0 += ks[0]
        x1 += ks[1]
        for i in range(5):
            for r in _ROT[i % 2]:
                x0 += x1
                x1 = _rotl(x1, r) ^ x0
            x0 += ks[(i + 1) % 3]
            x1 += ks[(i + 2) % 3] + np.uint32(i + 1)
    return x0, x1


def _threefry_counts(key, counts) -> np.ndarray:
    c = np.asarray(counts, dtype=np.uint32).ravel()
    odd = c.size & 1
    if odd:
        c = np.concatenate([c, np.zeros(1, np.uint32)])
    half = c.size // 2
    a, b = threefry2x32(key, c[:half], c[half:])
    out = np.concatenate([a, b])
    return out[:-1] if odd else out


def PRNGKey(seed: int) -> np.ndarray:
    seed = int(seed)
    return np.array([(seed >> 32) & 0xFFFFFFFF, seed & 0xFFFFFFFF], dtype=np.uint32)


def as_key(key) -> np.ndarray:
    k = np.asarray(key)
    if k.shape != (2,) or k.dtype != np.uint32:
        raise ValueError("a PRNG key is a uint32 array of shape (2,)")
    return k


def is_key(x) -> bool:
    return isinstance(x, np.ndarray) and x.shape == (2,) and x.dtype == np.uint32


def split(key, num: int = 2) -> np.ndarray:
    return _threefry_counts(as_key(key), np.arange(2 * num, dtype=np.uint32)).reshape(num, 2)


def fold_in(key, data: int) -> np.ndarray:
    return _threefry_counts(as_key(key), PRNGKey(data))


def random_split(rng):
    """internal/utils.py:118-123."""
    if rng is None:
        return None, None
    k = split(rng)
    return k[0], k[1]


def chunk_keys(key):
    """Key schedule of one render_image chunk (internal/models.py:2445 -> train_utils.py:3794, 3817-3818): one split
    for model.apply, one more for the key handed on to the next chunk.  Returns (apply_key, next_key)."""
    apply_key, key = random_split(key)
    next_key, _ = random_split(key)
    return apply_key, next_key


def random_bits(key, shape) -> np.ndarray:
    shape = tuple(int(s) for s in np.atleast_1d(shape)) if not isinstance(shape, tuple) else shape
    n = int(np.prod(shape)) if len(shape) else 1
    if n >= 2 ** 32 - 1:
        raise ValueError("more than 2^32 - 2 values per call are not supported")
    return _threefry_counts(as_key(key), np.arange(n, dtype=np.uint32)).reshape(shape)


def uniform(key, shape=(), minval=0.0, maxval=1.0) -> np.ndarray:
    bits = random_bits(key, tuple(shape))
    f = ((bits >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
    lo, hi = np.float32(minval), np.float32(maxval)
    return np.maximum(lo, (f * (hi - lo)).astype(np.float32) + lo).astype(np.float32)


_ERFINV_CENTRAL = (2.81022636e-08, 3.43273939e-07, -3.5233877e-06, -4.39150654e-06, 0.00021858087,
                   -0.00125372503, -0.00417768164, 0.246640727, 1.50140941)
_ERFINV_TAIL = (-0.000200214257, 0.000100950558, 0.00134934322, -0.00367342844, 0.00573950773,
                -0.0076224613, 0.00943887047, 1.00167406, 2.83297682)


def erfinv32(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    w = (-np.log1p(-x * x)).astype(np.float32)
    central = w < np.float32(5.0)
    with np.errstate(invalid="ignore"):
        ww = np.where(central, w - np.float32(2.5), np.sqrt(w) - np.float32(3.0)).astype(np.float32)
    p = np.where(central, np.float32(_ERFINV_CENTRAL[0]), np.float32(_ERFINV_TAIL[0])).astype(np.float32)
    for a, b in zip(_ERFINV_CENTRAL[1:], _ERFINV_TAIL[1:]):
        p = (np.where(central, np.float32(a), np.float32(b)) + p * ww).astype(np.float32)
    return (p * x).astype(np.float32)


def normal(key, shape=()) -> np.ndarray:
    lo = np.nextafter(np.float32(-1.0), np.float32(0.0))
    u = uniform(key, shape, lo, 1.0)
    return (np.float32(np.sqrt(2.0)) * erfinv32(u)).astype(np.float32)


def gumbel(key, shape=()) -> np.ndarray:
    u = uniform(key, shape, np.finfo(np.float32).tiny, 1.0)
    return (-np.log(-np.log(u))).astype(np.float32)


def categorical(key, logits, axis: int = -1, shape: Optional[Sequence[int]] = None) -> np.ndarray:
    """jax.random.categorical of jax 0.4.16: argmax over `axis` of gumbel noise + logits, the noise drawn with
    `logits.shape[axis]` re-inserted at `axis` of the requested batch shape."""
    logits = np.asarray(logits, dtype=np.float32)
    axis = axis % logits.ndim
    batch = tuple(np.delete(logits.shape, axis))
    shape = batch if shape is None else tuple(shape)
    prefix = shape[: len(shape) - len(batch)]
    lshape = list(shape[len(shape) - len(batch):])
    lshape.insert(axis, logits.shape[axis])
    g = gumbel(key, prefix + tuple(lshape))
    return np.argmax(g + logits.reshape((1,) * len(prefix) + logits.shape), axis=axis + len(prefix))


# ---------------------------------------------------------------------------------------------------------
# the reference's call order on the cache path
# ---------------------------------------------------------------------------------------------------------

def max_jitter(num_samples: int, eps: float = float(np.finfo(np.float32).eps)) -> float:
    """stepfun.py:197-198."""
    u_max = eps + (1 - eps) / num_samples
    return (1 - u_max) / (num_samples - 1) - eps


def sampler_randoms(sampler_rng, n_rays: int, num_samples: Sequence[int]):
    """Per-level jitter of ProposalVolumeSampler.__call__ given the rng it is called with (sampling.py:341-346:
    one random_split for sample_intervals, :408-409 one more for the density MLP, per level).  single_jitter=True:
    one uniform [n_rays, 1] per level (stepfun.py:196-202).  Returned as the UNIT uniform the C ABI takes
    (rc_randoms.jitter): jax's uniform(maxval=max_jitter) is float32(unit * max_jitter), the product the sampling
    kernel forms itself."""
    return [uniform(d.key, d.shape) for d in _sampler_plan(sampler_rng, "jitter", n_rays, len(num_samples))]


def cache_keys(cache_rng) -> Dict[str, np.ndarray]:
    """Keys of the radiance cache's __call__ given its rng (models.py:710-712 sampler, :727 resample, :748 shader;
    the use_slf / env_map_only branches are not taken on this path)."""
    k_sampler, rng = random_split(as_key(cache_rng))
    k_resample, rng = random_split(rng)
    k_shader, rng = random_split(rng)
    return {"sampler": k_sampler, "resample": k_resample, "shader": k_shader}


def model_cache_rng(model_rng) -> np.ndarray:
    """rng the cache is called with, from the rng of BaseMaterialModel.__call__ (models.py:1156 bypass split,
    :1176 cache-pass split, :1375 split inside _handle_cache_pass)."""
    _, rng = random_split(as_key(model_rng))
    k_pass, rng = random_split(rng)
    k_cache, _ = random_split(k_pass)
    return k_cache


def cache_pass_randoms(model_rng, n_rays: int, num_samples: Sequence[int], resample: bool = False):
    """Explicit random tensors of one primary cache pass (the dict the C ABI's rc_randoms takes) derived from the
    model's rng like the reference would.  Gumbel noise [n_rays, S] of the num_resample = 1 categorical draw
    (models.py:240-247: one more random_split inside maybe_resample) only when `resample`."""
    ck = cache_keys(model_cache_rng(model_rng))
    rnd = {"jitter": sampler_randoms(ck["sampler"], n_rays, num_samples)}
    if resample:
        key, _ = random_split(ck["resample"])
        rnd["gumbel"] = gumbel(key, (n_rays, int(num_samples[-1]), 1))[..., 0]
    return rnd


def pixel_jitter(rng, shape, jitter: int = 1, jitter_scale: float = 1.0):
    """The sub-pixel offsets camera_utils.pixels_to_rays draws when jitter > 0 (internal/camera_utils.py:943-957):
    key, rng = split(rng); k1, k2 = split(key); jitter == 1: U(0, 1) - 0.5 each, otherwise N(0, 1) * 0.5; with
    jitter_scale > 1 a second uniform pair from split(k1) is added.  Returns (dx, dy) float32 arrays of `shape` --
    what rc_camera.pix_dx / pix_dy (cast_ray_batch(..., pix_jitter=...)) take.  As with the other key paths of this
    module the call ORDER is restated from the source and cannot be checked against a JAX run here."""
    key, _ = split(as_key(rng))
    k1, k2 = split(key)
    if jitter == 1:
        dx = uniform(k1, shape) - np.float32(0.5)
        dy = uniform(k2, shape) - np.float32(0.5)
    else:
        dx = normal(k1, shape) * np.float32(0.5)
        dy = normal(k2, shape) * np.float32(0.5)
    if jitter_scale > 1.0:
        k1, k2 = split(k1)
        dx = dx + (uniform(k1, shape) - np.float32(0.5))
        dy = dy + (uniform(k2, shape) - np.float32(0.5))
    return dx.astype(np.float32), dy.astype(np.float32)


def light_vmf_noise(shape, seed: int = 1) -> np.ndarray:
    """Constant mean noise of LightMLP.get_vmfs (light_sampler.py:135-144): normal(random_split(PRNGKey(seed))[0],
    vmf_params.shape[:-1] + (3,)); the caller scales it by vmf_scale / 2."""
    key, _ = random_split(PRNGKey(seed))
    return normal(key, tuple(shape))


def material_pass_randoms(model_rng, n_rays: int, cfg, rc=None, train: bool = False) -> Dict[str, object]:
    """Explicit random tensors of ONE material-stage forward (the dict rc_material_randoms / Model.apply(passes=
    ("cache", "light", "material")) take) derived from the model's rng at the reference's split sites:

      BaseMaterialModel.__call__            models.py:1156 (bypass), 1177 (cache pass), 1195 (_get_material_samples),
                                            1208 (light sampler), 1220 (_handle_material_pass)
      _get_material_samples                 models.py:1417 (first maybe_resample, no draw), 1431 (MaterialModel's resample)
        maybe_resample                      models.py:241 -> jax.random.categorical == argmax(logits + gumbel[R, S, 1])
      _handle_material_pass -> shader       models.py:1548; shading.py:289; material.py:1971, 1988, 2030, 2535
      get_outgoing_radiance                 material.py:1383 (indirect specular), 1416 (indirect diffuse); 1642, 1721, 1780
      get_secondary_rays / importance_...   render_utils.py:962, 767 + 324 (uh, uw = uniform(key, [N K, 2])), 784
      LightSampler.sample_directions        render_utils.py:1450, 1407, 1358 (lobe: categorical over 128 logits),
                                            1409 (normal [N, K, 2]), 1413 (uniform [N, K])
      secondary cache calls                 material.py:2190; models.py:712 / 727 (resample gumbel [R, K, S, 1]);
                                            their sampler runs on the constant PRNGKey(0) at render time
                                            (sampling.py:170-179) -- the specular and the diffuse trace therefore draw the
                                            SAME per-level jitter
    The call order is restated from the source and cannot be checked against a jax run here (no jax in the image).
    With `rc` (a RadianceCache) the same tensors are drawn in HBM by one launch (rc.material_randoms: cuda views of one
    arena, sec_jitter / sec_gumbel in the ABI's layout instead of the spec_* / diff_* pairs); train: material_stage_plan."""
    if rc is not None:
        return rc.material_randoms(model_rng, n_rays, cfg.num_secondary_samples, train=train)
    if train:
        return plan_randoms(material_stage_plan(model_rng, n_rays, cfg, train=True, vmf_noise=True))
    return _material_stage_randoms(model_rng, n_rays, cfg, env_sampler=False)


def relight_pass_randoms(model_rng, n_rays: int, cfg) -> Dict[str, object]:
    """The random inputs of ONE relit material-stage forward under Config.compute_relight_metrics (EnvironmentSampler in
    both sampler sets; relight.relight(mode="env")): the tensors material_pass_randoms gives for the parts both modes
    share (the primary rays' jitter, the shading sample's gumbel, the secondary traces' jitter and gumbel) and the two
    categorical keys of the texel draws, "picks_key_spec" and "picks_key_diff", at their split sites:

      get_outgoing_radiance                 material.py:1383 (indirect specular), 1416 (indirect diffuse); 1513, 1540 reuse
                                            the rays of these two legs for the direct (env-map) passes
      importance_sample_rays                render_utils.py:767 (uh, uw: drawn, not used by this sampler), 784 (the
                                            sampler's rng); ONE sampler per set, with the leg's whole count
      EnvironmentSampler.sample_directions  render_utils.py:215 (key, rng = split(rng); categorical(key, ...))
    The secondary cache calls' keys do not depend on the sampler set, so the traces draw what material_pass_randoms
    draws.  Like that function the call order is restated from the source and not pinned to a jax run."""
    return _material_stage_randoms(model_rng, n_rays, cfg, env_sampler=True)


def _material_stage_randoms(model_rng, n_rays: int, cfg, env_sampler: bool) -> Dict[str, object]:
    return plan_randoms(material_stage_plan(model_rng, n_rays, cfg, env_sampler=env_sampler, vmf_noise=True))


class Draw(NamedTuple):
    """One jax.random draw of a plan.  name: the member of the randoms dict ("jitter[1]": element 1 of the list "jitter");
    key: uint32[2]; mode: MODE_*; shape: the shape jax draws (its element count fixes the counter layout); layout: "flat"
    (the member is the tensor), "planes" (the last axis of 2 is split: <name>1 = [..., 0], <name>2 = [..., 1]) or "key" (no
    tensor: the member is the key itself)."""
    name: str
    key: np.ndarray
    mode: int
    shape: Tuple[int, ...]
    layout: str


# member ids of the C twin (include/rc_abi.h rc_prng_member); "<name>[l]" is id + l
MEMBER_IDS = {"jitter": 0, "gumbel": 8, "vmf_noise": 9, "spec_u": 10, "cos_u": 11, "vmf_lobe_gumbel": 12, "vmf_v": 13,
              "vmf_tmp": 14, "spec_gumbel": 15, "diff_gumbel": 16, "noise": 17, "picks_key_spec": 18, "picks_key_diff": 19,
              "spec_jitter": 24, "diff_jitter": 32}


def member_id(name: str) -> int:
    base, _, idx = name.partition("[")
    return MEMBER_IDS[base] + (int(idx[:-1]) if idx else 0)


def material_split(cfg, K: Optional[int] = None) -> Tuple[int, int, int, int]:
    """(Ks, Kd, Kc, Kl) of K secondary samples: GGX, diffuse = cosine + light sampler (Python's round: half to even)."""
    K = int(cfg.num_secondary_samples if K is None else K)
    Kd = int(round(K * cfg.diffuse_sample_fraction))
    Ks = int(round(K * (1.0 - cfg.diffuse_sample_fraction)))
    Kc = int(round(0.5 * Kd))
    return Ks, Kd, Kc, Kd - Kc


def _sampler_plan(sampler_rng, name: str, n_rays: int, num_levels: int):
    """sampler_randoms as draws: per level one random_split for the jitter, one more for the density MLP."""
    rng, out = as_key(sampler_rng), []
    for l in range(num_levels):
        key, rng = random_split(rng)
        out.append(Draw(f"{name}[{l}]", key, MODE_UNIFORM, (n_rays, 1), "flat"))
        _, rng = random_split(rng)
    return out


def material_stage_plan(model_rng, n_rays: int, cfg, train: bool = False, env_sampler: bool = False, loss_key=None,
                        vmf_noise: bool = False) -> list:
    """The random_split tree of ONE material-stage forward as an ordered list of Draw rows: the split sites that
    material_pass_randoms / relight_pass_randoms cite, and no tensor.  plan_randoms realises it on the host;
    rc_material_randoms_plan (csrc/rc_prng_host.h) is the same tree in C, row for row, and rc_prng_fill_segments fills it
    in HBM in one launch (RadianceCache.material_randoms).

      train        True: the sampler of each secondary trace runs on its own key, cache_keys(kc)["sampler"] with kc the key
                   of material.py:2190 -- internal/sampling.py:170-179 replaces the rng by PRNGKey(0) only when
                   `deterministic or (not train and is_secondary)`.  False: PRNGKey(0) for both traces (render time).
      env_sampler  EnvironmentSampler in both sampler sets (relight_pass_randoms): the two texel-draw keys as "key" rows.
      loss_key     the key material_smoothness receives (extra_loss_keys): the plan ends with its noise [n, 3]
                   (material_smoothness_noise).
      vmf_noise    add light_vmf_noise's PRNGKey(1) constant [n, num_vmf, 3]; it depends on n alone, so callers cache it.

    Like every key path of this module the call order is restated from the source and is NOT pinned against a jax run (no
    jax here); that holds for the train=True reading and for the place of the noise as well."""
    n = int(n_rays)
    Ks, Kd, Kc, Kl = material_split(cfg)
    levels = [int(lvl[2]) for lvl in cfg.sampling_strategy]
    S, NL, V = levels[-1], len(levels), int(cfg.num_vmf)
    rng = as_key(model_rng)
    plan = _sampler_plan(cache_keys(model_cache_rng(rng))["sampler"], "jitter", n, NL)      # primary rays' jitter
    _, rng = random_split(rng)                # :1156
    _, rng = random_split(rng)                # :1177
    k_samples, rng = random_split(rng)        # :1195
    _, rng = random_split(rng)                # :1208 (LightMLP draws nothing from it: its noise is the PRNGKey(1) constant)
    k_mat, rng = random_split(rng)            # :1220
    # -- categorical pick of the shading sample
    _, r = random_split(k_samples)            # :1417
    k2, r = random_split(r)                   # :1431
    kg, _ = random_split(k2)                  # :241
    plan.append(Draw("gumbel", kg, MODE_GUMBEL, (n, S), "flat"))
    if vmf_noise and not env_sampler:         # (the LightSampler is not evaluated under the EnvironmentSampler)
        plan.append(Draw("vmf_noise", random_split(PRNGKey(1))[0], MODE_NORMAL, (n, V, 3), "flat"))
    # -- material shader
    k_sh, _ = random_split(k_mat)             # models.py:1548
    k_pa, _ = random_split(k_sh)              # shading.py:289
    _, r = random_split(k_pa)                 # material.py:1971
    _, r = random_split(r)                    # :1988
    k_int, _ = random_split(r)                # :2030
    k_out, _ = random_split(k_int)            # :2535
    k_spec, r = random_split(k_out)           # :1383 indirect specular
    k_diff, r = random_split(r)               # :1416 indirect diffuse (the env-map passes reuse these rays)

    def one_pass(k_pass, n_samplers):
        """-> ([(key of the [m, 2] uniform, sampler rng)] per sampler, key of the cache call)."""
        kh, _ = random_split(k_pass)          # :1642
        kh1, r2 = random_split(kh)            # :1721 get_secondary_rays
        kh2, _ = random_split(r2)             # :1780 radiance_cache_fn
        ki, _ = random_split(kh1)             # render_utils.py:962
        keys, r3 = [], ki
        for _ in range(n_samplers):
            ka, r3 = random_split(r3)         # :767
            ku, _ = random_split(ka)          # :324
            kb, r3 = random_split(r3)         # :784
            keys.append((ku, kb))
        kc, _ = random_split(kh2)             # material.py:2190
        return keys, kc

    def trace_plan(kc, Kp, name):
        ck = cache_keys(kc)                   # models.py:712 (sampler: PRNGKey(0) unless train), 727, 748
        kg2, _ = random_split(ck["resample"])  # :241
        return (_sampler_plan(ck["sampler"] if train else PRNGKey(0), f"{name}_jitter", n * Kp, NL)
                + [Draw(f"{name}_gumbel", kg2, MODE_GUMBEL, (n * Kp, S), "flat")])

    keys_s, kc_spec = one_pass(k_spec, 1)
    keys_d, kc_diff = one_pass(k_diff, 1 if env_sampler else 2)
    if env_sampler:
        plan.append(Draw("picks_key_spec", random_split(keys_s[0][1])[0], MODE_BITS, (0,), "key"))    # render_utils.py:215
    else:
        plan.append(Draw("spec_u", keys_s[0][0], MODE_UNIFORM, (n, Ks, 2), "planes"))
    plan += trace_plan(kc_spec, Ks, "spec")
    if env_sampler:
        plan.append(Draw("picks_key_diff", random_split(keys_d[0][1])[0], MODE_BITS, (0,), "key"))
    else:
        plan.append(Draw("cos_u", keys_d[0][0], MODE_UNIFORM, (n, Kc, 2), "planes"))
        ks, _ = random_split(keys_d[1][1])    # LightSampler.sample_directions (render_utils.py:1450)
        kv1, r5 = random_split(ks)            # sample_vmf :1407
        kl, _ = random_split(kv1)             # sample_vmf_vars :1358
        plan.append(Draw("vmf_lobe_gumbel", kl, MODE_GUMBEL, (n, V), "flat"))
        kn, r5 = random_split(r5)             # :1409
        plan.append(Draw("vmf_v", kn, MODE_NORMAL, (n, Kl, 2), "flat"))
        kt, _ = random_split(r5)              # :1413
        plan.append(Draw("vmf_tmp", kt, MODE_UNIFORM, (n, Kl), "flat"))
    plan += trace_plan(kc_diff, Kd, "diff")
    if loss_key is not None:
        key = as_key(loss_key)
        _, key = random_split(key)            # train_utils.py:2530
        _, key = random_split(key)            # :2541
        kn2, _ = random_split(key)            # :2566
        plan.append(Draw("noise", kn2, MODE_NORMAL, (n, 3), "flat"))
    return plan


_DRAW_FN = {MODE_BITS: lambda k, s: random_bits(k, s), MODE_UNIFORM: lambda k, s: uniform(k, s),
            MODE_NORMAL: lambda k, s: normal(k, s), MODE_GUMBEL: lambda k, s: gumbel(k, s)}


def put_member(out: Dict[str, object], name: str, value) -> None:
    """Store one plan member under its name; "<base>[l]" appends to the list out[base] (levels come in order)."""
    base, _, idx = name.partition("[")
    if idx:
        out.setdefault(base, []).append(value)
    else:
        out[name] = value


def plan_randoms(plan) -> Dict[str, object]:
    """Host realisation of a material_stage_plan: the randoms dict with numpy arrays."""
    out: Dict[str, object] = {}
    for d in plan:
        if d.layout == "key":
            out[d.name] = d.key
            continue
        x = _DRAW_FN[d.mode](d.key, tuple(d.shape))
        if d.layout == "planes":
            out[d.name + "1"], out[d.name + "2"] = x[..., 0], x[..., 1]
        else:
            put_member(out, d.name, x)
    return out


# the extra losses of the material stage in _compute_extra_losses' dict order (internal/train_utils.py:3620-3632); each
# enabled one takes one split of the key (:3648)
EXTRA_LOSS_ORDER = ("emission", "residual_albedo", "direct_indirect_consistency", "light_sampling",
                    "material_surface_light_field", "material_smoothness", "geometry_smoothness", "material_correlation",
                    "material_ray_sampler", "maximum_radiance", "normalize_weight")
# material_light_from_scratch's extra losses (configs/trainer.gin:333-350)
MATERIAL_STAGE_EXTRA_LOSSES = ("material_ray_sampler", "material_smoothness", "light_sampling")


def extra_loss_keys(cur_key, enabled: Sequence[str] = MATERIAL_STAGE_EXTRA_LOSSES) -> Dict[str, np.ndarray]:
    """The key each enabled extra loss receives from _compute_extra_losses (train_utils.py:3648: rng, cur_key =
    random.split(cur_key), in EXTRA_LOSS_ORDER)."""
    out = {}
    key = as_key(cur_key)
    for name in EXTRA_LOSS_ORDER:
        if name in enabled:
            k = split(key)
            out[name], key = k[0], k[1]
    return out


def material_smoothness_noise(loss_key, n_points: int) -> np.ndarray:
    """nu of material_smoothness_loss (train_utils.py:2530-2574) from the key the loss receives: three splits (:2530 the
    resample pick, :2541 the cache_shader pick, :2566 the noise), then normal(rng, [n, 3]) (:2568).  The perturbed
    shading pass's key (:2574) is not drawn from here (material_only, shading_only: the material head draws nothing).
    The order against a jax run is unverified (no jax here)."""
    key = as_key(loss_key)
    _, key = random_split(key)      # :2530
    _, key = random_split(key)      # :2541
    rng, _ = random_split(key)      # :2566
    return normal(rng, (int(n_points), 3))


def geometry_smoothness_noise(loss_key, n_rays: int, S: int, rc=None):
    """The noise of geometry_smoothness_loss (train_utils.py:2728-2743) from the key the loss receives: two
    jax.random.split (:2728, :2741; plain splits, not utils.random_split), the second `rng` being the normal's key, then
    normal(rng, [n, S, 3]) (:2743; the shape of the last level's means).  With `rc` it is drawn on the device by one
    rc_prng_fill in normal mode (the same bits and counters; the values an ulp or two from the host twin's, as every
    normal of rc_prng_fill); otherwise on the host.  The order against a jax run is unverified (no jax here)."""
    key = split(as_key(loss_key))[1]      # :2728  rng, cur_key = random.split(cur_key)
    rng = split(key)[0]                   # :2741  rng, cur_key = random.split(cur_key)
    shape = (int(n_rays), int(S), 3)
    return rc.prng_fill(rng, shape, mode="normal") if rc is not None else normal(rng, shape)


def backward_mask_keys(cur_key):
    """The two keys _compute_backward_mask_loss (internal/train_utils.py:3348-3401) takes from the key per_output_loss_fn
    hands it: (key of the uniform pair, rng of the weights-only model.apply on the backward rays).  :3363 random.split ->
    get_secondary_rays' random_split (render_utils.py:965) -> importance_sample_rays' split for its one sampler (:767)
    -> RandomGenerator2D.sample's split (:324); then :3385 random.split for model.apply.  Like every key path of this
    module the call order is restated from the source and is not pinned against a jax run (no jax here)."""
    k = split(as_key(cur_key))            # train_utils.py:3363
    rng, cur = k[0], k[1]
    key, _ = random_split(rng)            # render_utils.py:965
    ka, _ = random_split(key)             # :767
    ku, _ = random_split(ka)              # :324
    k_apply = split(cur)[0]               # train_utils.py:3385
    return ku, k_apply


def backward_mask_randoms(cur_key, n_rays: int, num_samples: Sequence[int], rc=None) -> Dict[str, object]:
    """The draws of the backward mask term for n_rays batch rays: "u1", "u2" = the two columns of uniform(key, (n, 2))
    (RandomGenerator2D(1, 1, False) is not stratified: uh, uw of render_utils.py:325-327) and "jitter" = the per-level
    sampler jitter of the weights-only pass on the backward rays (cache_pass_randoms of its model rng).  With `rc` the
    pair is generated on the device by one rc_prng_fill (bit-equal to the host's); otherwise on the host.  Unpinned
    against jax, as backward_mask_keys says."""
    ku, k_apply = backward_mask_keys(cur_key)
    u = rc.prng_fill(ku, (int(n_rays), 2)) if rc is not None else uniform(ku, (int(n_rays), 2))
    u1, u2 = (u[:, 0].contiguous(), u[:, 1].contiguous()) if rc is not None else (np.ascontiguousarray(u[:, 0]), np.ascontiguousarray(u[:, 1]))
    return {"u1": u1, "u2": u2, "jitter": cache_pass_randoms(k_apply, n_rays, num_samples)["jitter"]}
