"""The cache pass at non-default render settings: the case table, the configs, the seeded batches, the oracle
runs and the conditions that rest on the oracle alone.  Shared by test_render_settings.py (CPU: the conditions) and
test_gpu_render_settings.py (GPU: the kernels under the same configs), so the two cannot drift apart.  Test helper, not a
test module.

rc_config is public ABI and RenderConfig maps onto it field by field, but the defaults coincide: density_bias,
roughness_bias, slf_ambient_bias and env_rgb_bias are all -1, irradiance_bias and ambient_irradiance_bias both -2,
env_map_distance equals the far of every secondary-ray test and rgb_max (1e4) never clips.  Two fields exchanged anywhere
between the ctypes struct and a kernel argument would pass every test that runs at the defaults.  Each case here moves one
field to a value distinct from every other value and every default; `combined` moves all of them at once."""
import dataclasses
import functools

import numpy as np
import torch

import common
import nrc_amd
from loss_cases import GUARD_FACTOR
from oracle import cache_ref

DEFAULT = nrc_amd.hotdog_config()
N_LEVELS = DEFAULT.num_levels
SAMPLES = tuple(s for _, _, s in DEFAULT.sampling_strategy)

# field -> case value.  rc_create accepts every one of them (it checks the sampling strategy and the grids only), so no
# value had to be replaced by a neighbour.
# ambient_irradiance_bias moves up, next to irradiance_bias, not down: at -3.0 with irradiance_bias -0.75 and
# slf_ambient_bias 0.25, `combined` has no rgb_max that clips 10-90 % of all three clamped channels (fp64 oracle, 64 rays:
# the ambient diffuse's 90 % quantile is 0.066-0.081, the 10 % quantiles of the two indirect channels are 0.26-0.30; at
# their pooled median, 0.324, no ambient entry clips).  The clipped share is a condition of test_render_settings.py, so the
# value gives way: at -0.6 the pooled median (0.393) clips 29-82 % of each channel.
# resample_padding stays clear of 1e-2, the default of shadow_normal_eps_dot_min.
VALUES = {
    "density_bias": -0.25,                  # default -1.0
    "roughness_bias": 0.5,                  # -1.0
    "irradiance_bias": -0.75,               # -2.0
    "ambient_irradiance_bias": -0.6,        # -2.0 (the note above)
    "slf_ambient_bias": 0.25,               # -1.0
    "rgb_max": 0.13,                        # 1e4: clips about half of each clamped channel (test_render_settings.py)
    "env_rgb_bias": -2.5,                   # -1.0
    "bg_intensity": 0.35,                   # 1.0
    "percentiles": (20.0, 60.0, 90.0),      # (5, 50, 95)
    "anneal": 0.7,                          # 0.4
    "resample_padding": 2e-2,               # 1e-5 (not 1e-2, the default of shadow_normal_eps_dot_min)
    "raydist_p": -0.5,                      # -1.5
    "raydist_premult": 1.25,                # 2.0
    "shadow_normal_eps_dot_min": 0.08,      # 1e-2
    "env_map_distance": 1.5,                # 2.0, the far of common.secondary_case: the clamp binds
}
FIELDS = tuple(VALUES)
CASES = FIELDS + ("combined",)
# the fields whose defaults coincide: exchanged on the way to a kernel they pass every test at the defaults
COINCIDING = (("density_bias", "roughness_bias", "slf_ambient_bias", "env_rgb_bias"), ("irradiance_bias", "ambient_irradiance_bias"))
SWAP_PAIRS = tuple((a, b) for group in COINCIDING for i, a in enumerate(group) for b in group[i + 1:])

SHADER_CASES = ("roughness_bias", "irradiance_bias", "ambient_irradiance_bias", "slf_ambient_bias", "rgb_max", "combined")
DENSITY_CASES = ("density_bias", "combined")
ENVMAP_CASES = ("env_rgb_bias", "combined")
PRIMARY_PASS_CASES = ("anneal", "resample_padding", "bg_intensity", "percentiles", "combined")
SECONDARY_PASS_CASES = ("raydist_p", "raydist_premult", "shadow_normal_eps_dot_min", "env_map_distance", "combined")
CLIPPED_CASES = ("rgb_max", "combined")
CLAMPED = ("direct_diffuse_rgb", "indirect_diffuse_rgb", "indirect_specular_rgb")      # ambient diffuse is the direct diffuse

SHADE_KEYS = (("rgb", 0), ("direct_diffuse_rgb", 3), ("indirect_diffuse_rgb", 6), ("indirect_specular_rgb", 9),
              ("albedo_rgb", 12))       # rc_internal.h RC_SH_*; tests/test_gpu_mlp_floor.py
# the device names its three distance outputs after the default percentiles; they follow cfg.percentiles by position
PCT_KEYS = ("distance_percentile_5", "distance_median", "distance_percentile_95")
LEVEL_KEYS = tuple(f"{w}{l}" for l in range(N_LEVELS) for w in ("sdist", "tdist", "weights", "density"))
PASS_KEYS = ("rgb", "acc", "distance_mean") + PCT_KEYS + LEVEL_KEYS
SHADE_OUT = tuple("shade:" + k for k, _ in SHADE_KEYS)

# field -> the outputs (of `flatten`) it must move; (primary outputs, secondary outputs)
_LEVELS = lambda *ws: tuple(f"{w}{l}" for l in range(N_LEVELS) for w in ws)
MOVES = {
    "density_bias": (_LEVELS("density", "weights"), ()),
    "roughness_bias": (("shade:indirect_specular_rgb",), ()),
    "irradiance_bias": (("shade:indirect_diffuse_rgb",), ()),
    "ambient_irradiance_bias": (("shade:direct_diffuse_rgb",), ()),
    "slf_ambient_bias": (("shade:indirect_specular_rgb",), ()),
    "rgb_max": (("shade:direct_diffuse_rgb", "shade:indirect_diffuse_rgb", "shade:indirect_specular_rgb"), ()),
    "env_rgb_bias": ((), ("env_map_rgb",)),
    "bg_intensity": (("rgb",), ()),
    "percentiles": (PCT_KEYS, ()),
    "anneal": (("sdist1", "sdist2"), ()),
    "resample_padding": (("sdist1", "sdist2"), ()),
    "raydist_p": ((), _LEVELS("tdist")),
    "raydist_premult": ((), _LEVELS("tdist")),
    "shadow_normal_eps_dot_min": ((), _LEVELS("tdist")),
    "env_map_distance": ((), _LEVELS("tdist")),
}

EPS_SHADE, EPS_ENV, K = 2e-7, 5e-7, 3.0          # tests/test_gpu_mlp_floor.py


def weights(smooth):
    """White-noise tables, or the smooth ones (table amplitude 0.2 * 0.5 ** level) the whole-pass floor checks need."""
    return common.weights_material_np(True) if smooth else common.weights_np()


def primary_batch(n):
    return nrc_amd.synthetic_rays(n, seed=31), common.jitters(n, seed=5)


def secondary_batch(n):
    return common.secondary_case(n, seed=11)


def flatten(out, secondary=False):
    """{name: float64 array} of a cache_ref.cache_forward result: PASS_KEYS, the per-sample shade channels and, on
    secondary rays with the EnvMap, env_map_rgb.  The distance outputs go by the position of their percentile."""
    r = out["render"]
    f = {k: r[k] for k in ("rgb", "acc", "distance_mean")}
    names = ["median" if p == 50 else "percentile_" + str(int(p)) for p in out["cfg"].percentiles]
    f.update({k: r["distance_" + nm] for k, nm in zip(PCT_KEYS, names)})
    for l in range(N_LEVELS):
        f.update({f"{w}{l}": out["sampler"][l][w] for w in ("sdist", "tdist", "weights", "density")})
    f.update({"shade:" + k: out["shader"][k] for k, _ in SHADE_KEYS})
    if secondary and "env_map_rgb" in r:
        f["env_map_rgb"] = r["env_map_rgb"]
    return {k: v.double().numpy() for k, v in f.items()}


def oracle_primary(cfg, n, dtype, smooth=True):
    rays, jit = primary_batch(n)
    with torch.no_grad():
        out = cache_ref.cache_forward(common.to_torch(weights(smooth), dtype), cfg, common.rays_torch(rays, dtype),
                                      [torch.from_numpy(j).to(dtype) for j in jit], want_grad_normals=False)
    out["cfg"] = cfg
    return out


def oracle_secondary(cfg, n, dtype, smooth=True, inds=None, use_env_map=True):
    """Secondary rays (tests/test_gpu_parity.py _oracle_secondary); `inds` [n] hands the categorical picks over."""
    rays, rnd = secondary_batch(n)
    jit = [torch.from_numpy(j)[:, None].to(dtype) for j in rnd["jitter"]]
    inds = None if inds is None else torch.from_numpy(np.asarray(inds, np.int64))[:, None]
    with torch.no_grad():
        out = cache_ref.cache_forward(common.to_torch(weights(smooth), dtype), cfg, common.rays_dict_torch(rays, dtype), jit,
                                      is_secondary=True, gumbel=torch.from_numpy(rnd["gumbel"]).to(dtype), inds=inds,
                                      use_env_map=use_env_map, want_grad_normals=False)
    out["cfg"] = cfg
    return out


def secondary_refs(cfg, n, smooth=True, use_env_map=True):
    """(fp64, fp32, picks): the fp64 oracle draws the picks, the fp32 one is handed them, as the device is."""
    r64 = oracle_secondary(cfg, n, torch.float64, smooth, use_env_map=use_env_map)
    picks = r64["filtered_sampler_inds"][:, 0].numpy().astype(np.int32)
    return r64, oracle_secondary(cfg, n, torch.float32, smooth, inds=picks, use_env_map=use_env_map), picks


def shader_stage(cfg, out, dtype, smooth=True):
    """{"shade:<key>": float64 array} of cache_ref.cache_shader alone under cfg, in `dtype`, on the shader inputs of the
    cache_forward result `out` (its samples' means, hidden features, normals; the appearance features looked up in
    out's own precision): the oracle's counterpart of the GPU shader check, which feeds the stage the device's inputs."""
    from oracle import hashgrid_ref, mathx
    sh = out["shader"]
    src = sh["means"].dtype
    rays = primary_batch(len(sh["means"]))[0]
    with torch.no_grad():
        app = hashgrid_ref.hash_encoding(common.to_torch(weights(smooth), src), f"{cache_ref.P}Cache/Shader/appearance_grid",
                                         cfg.appearance_grid, mathx.contract_radius(sh["means"], cfg.contract_radius))
        sres = {k: sh[k].to(dtype) for k in ("means", "feature", "normals_to_use")}
        o = cache_ref.cache_shader(common.to_torch(weights(smooth), dtype), cfg, common.rays_torch(rays, dtype), sres,
                                   app=app.to(dtype))
    return {"shade:" + k: o[k].double().numpy() for k, _ in SHADE_KEYS}


def granted(key, c64, c32):
    """The tolerance the GPU test grants output `key`, from the fp32 oracle's own distance from fp64 under the same config
    (scalar, or per channel for the shade channels and the EnvMap): the whole-pass floor check's 3 x floor + 1e-7
    (test_gpu_parity.py), mlp_floor.floor_check's K x floor + EPS x max|fp64| per channel."""
    if key.startswith("shade:") or key == "env_map_rgb":
        eps = EPS_ENV if key == "env_map_rgb" else EPS_SHADE
        c = c64.shape[-1]
        a, b = c64.reshape(-1, c), c32.reshape(-1, c)
        return K * np.abs(b - a).max(0) + eps * np.abs(a).max(0)
    return 3.0 * float(np.abs(c32 - c64).max()) + 1e-7


def effect(key, c64, d64):
    """max|case fp64 - default fp64|, per channel where `granted` is."""
    d = np.abs(c64 - d64)
    return d.reshape(-1, d.shape[-1]).max(0) if key.startswith("shade:") or key == "env_map_rgb" else float(d.max())


def guard(what, keys, c64, c32, d64, every=True):
    """A settings case must be able to fail (loss_cases.guard): its fp64 result differs from the fp64 result at `d64`'s
    settings by more than GUARD_FACTOR x the granted tolerance -- in every output of `keys` (every channel of it), or with
    every=False in at least one.  Rests on the reference alone."""
    ratios = effect_ratios(keys, c64, c32, d64)
    print(what, "effect of the setting / granted tolerance:", {k: f"{r:.3g}" for k, r in ratios.items()})
    moved = [r > GUARD_FACTOR for r in ratios.values()]
    assert moved and (all(moved) if every else any(moved)), (what, ratios)


def effect_ratios(keys, c64, c32, d64):
    """{key: effect / granted tolerance}, the smallest over a key's channels."""
    return {k: float(np.min(np.asarray(effect(k, c64[k], d64[k])) / np.asarray(granted(k, c64[k], c32[k])))) for k in keys}


def preclamp_pool(cfg, n=64, smooth=False):
    """The fp64 values of the three clamped channels before the clamp, pooled: the oracle under cfg with rgb_max out of reach."""
    out = oracle_primary(dataclasses.replace(cfg, rgb_max=DEFAULT.rgb_max), n, torch.float64, smooth)
    v = np.concatenate([out["shader"][k].numpy().reshape(-1) for k in CLAMPED])
    assert v.max() < DEFAULT.rgb_max
    return v


@functools.lru_cache(maxsize=1)
def combined_rgb_max():
    """rgb_max of `combined`: the biases shift the three channels, so the clamp goes to the fp64 median of their pooled
    pre-clamp values under the combined biases (64 rays, white-noise weights; the oracle, never the device), as the
    float32 the device receives."""
    cfg = dataclasses.replace(DEFAULT, **{k: v for k, v in VALUES.items() if k != "rgb_max"})
    return float(np.float32(np.median(preclamp_pool(cfg))))


def config(name):
    """RenderConfig of one entry of CASES."""
    if name == "combined":
        return dataclasses.replace(DEFAULT, **dict(VALUES, rgb_max=combined_rgb_max()))
    return dataclasses.replace(DEFAULT, **{name: VALUES[name]})


def swapped(cfg, a, b):
    return dataclasses.replace(cfg, **{a: getattr(cfg, b), b: getattr(cfg, a)})


def clipped_share(out, cfg):
    """{channel: share of its entries that sit at rgb_max} of a cache_forward result."""
    return {k: float((out["shader"][k].numpy() >= cfg.rgb_max).mean()) for k in CLAMPED}


def replaced_near(cfg, rays):
    """(near as the rays give it, near after sampling.py:182-205, far after the env_map_distance clamp), float64 [n]."""
    r = common.rays_dict_torch(rays, torch.float64)
    r["far"] = torch.clamp(r["far"], max=cfg.env_map_distance)
    return r["near"][:, 0].numpy(), cache_ref.secondary_near(cfg, r)[:, 0].numpy(), r["far"][:, 0].numpy()
