"""Every split-form MLP stage against fp64, at the fp32 noise floor of the oracle, on the HIP path's own inputs.

The shader-class layers multiply on the bf16 pipe (rc_dev_mlp.h: each fp32 operand cut into three bf16 pieces, six
products summed by v_mfma_f32_32x32x16_bf16) and claim fp32-grade results.  Whole-render bounds cannot hold them to
that: the render's floor comes from upstream sample positions that random hash tables amplify.  So each stage is fed
the inputs the HIP path itself computed (read back from the workspace), the fp64 oracle stage on those inputs is the
exact value, and the fp32 oracle stage on the same inputs is the floor.  Per output channel c:

    max|HIP_c - fp64_c| <= K * max|fp32_c - fp64_c| + EPS * max|fp64_c|

EPS absorbs the device transcendentals (v_exp_f32 / v_log_f32 in softplus and sigmoid, sin in the encodings).  Each
test also shows its own power: numpy's emulation of the nearest plausible wrong arithmetic -- the bf16 split with only
the three leading products (hi.hi, mid.hi, hi.mid, accumulated in fp32) -- must exceed the bound by POWER x.
"""
import contextlib
import dataclasses

import numpy as np
import pytest
import torch

import common
import nrc_amd

pytestmark = pytest.mark.gpu
K = 3.0
EPS = 2e-7          # the shaders' softplus / sigmoid; the EnvMap's sin(2^3 d) encodings take EPS_ENV
EPS_ENV = 5e-7
POWER = 10.0


# ---------------------------------------------------------------------------------------------
# the wrong arithmetic the bounds must reject
# ---------------------------------------------------------------------------------------------
def _top16(x):
    """bf16 truncation of an fp32 tensor (the split's pieces, rc_dev_mlp.h split8)."""
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def dense_split3(weights, path, x):
    """flax Dense in the split form with the three smallest products dropped: of a = hi + mid + lo (exact) keep only
    hi.hi + mid.hi + hi.mid, in fp32.  The bias is the weight of an input that is exactly 1 (hi = 1, mid = 0).
    The density MLPs (Sampler) stay exact: they are fp32 MFMA chains in every build."""
    from oracle.cache_ref import P
    if "/Sampler/" in path:
        return _DENSE(weights, path, x)
    k = weights[f"{P}{path}/kernel"].to(torch.float32)
    b = weights[f"{P}{path}/bias"].to(torch.float32)
    x = x.to(torch.float32)
    xh, kh = _top16(x), _top16(k)
    xm, km = _top16(x - xh), _top16(k - kh)
    bh = _top16(b)
    return xh @ kh + xm @ kh + xh @ km + (bh + _top16(b - bh))


from oracle.cache_ref import dense as _DENSE  # noqa: E402


@contextlib.contextmanager
def split3(*modules):
    saved = [m.dense for m in modules]
    try:
        for m in modules:
            m.dense = dense_split3
        yield
    finally:
        for m, d in zip(modules, saved):
            m.dense = d


def floor_stats(hip, b32, b64, emu):
    """Per channel (last axis): max|HIP - fp64|, the floor max|fp32 - fp64|, max|emulation - fp64|, max|fp64|."""
    c = hip.shape[-1]
    hip, b32, b64, emu = (np.asarray(a, np.float64).reshape(-1, c) for a in (hip, b32, b64, emu))
    assert np.isfinite(hip).all()
    return (np.abs(hip - b64).max(0), np.abs(b32 - b64).max(0), np.abs(emu - b64).max(0), np.abs(b64).max(0))


def floor_check(name, hip, b32, b64, emu, power=True, eps=EPS, cfg=None):
    """The bound above per channel, and (power) the emulation POWER x beyond it.  cfg: the config of a case that is not at
    the hotdog defaults; its figures are printed (HIP / floor, HIP / bound, emulation / bound per channel) and a failure
    names the fields that are off their defaults."""
    err, floor, wrong, scale = floor_stats(hip, b32, b64, emu)
    bound = K * floor + eps * scale
    if cfg is not None:
        base = nrc_amd.hotdog_config()
        name = (name, {f.name: getattr(cfg, f.name) for f in dataclasses.fields(cfg) if getattr(cfg, f.name) != getattr(base, f.name)})
        with np.errstate(divide="ignore", invalid="ignore"):
            print(name[0], "HIP / floor", np.round(err / floor, 2), "HIP / bound", np.round(err / bound, 2),
                  "emulation / bound", np.round(wrong / bound, 1))
    assert (err <= bound).all(), (name, "HIP", err, "floor", floor, "bound", bound)
    if power:
        assert (wrong >= POWER * bound).all(), (name, "3-product emulation", wrong, "bound", bound)


# ---------------------------------------------------------------------------------------------
# k_envmap: the model EnvMap of secondary rays, a function of the view direction alone
# ---------------------------------------------------------------------------------------------
def adversarial_dirs(n, seed=0):
    """The six axes, directions with +-0 components, near-grazing ones (components of 1e-7 .. 2^-24 and subnormal),
    then random unit vectors."""
    z = -0.0
    adv = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),
           (z, 1, 0), (0, z, -1), (1, z, z), (z, z, -1), (0.6, z, 0.8), (z, -0.8, 0.6), (-0.6, 0.8, z),
           (1, 1e-7, 0), (1e-7, -1, -1e-7), (1, -2.0 ** -24, 2.0 ** -24), (2.0 ** -24, 2.0 ** -24, 1), (1, 1e-40, -1e-40),
           (0.7071067811865476, 0.7071067811865476, 1e-7), (-0.5773502691896258, 0.5773502691896258, -0.5773502691896258)]
    rng = np.random.default_rng(seed)
    rnd = rng.normal(size=(max(n - len(adv), 0), 3))
    d = np.concatenate([np.asarray(adv, np.float64), rnd])[:n]
    nrm = np.linalg.norm(d, axis=-1, keepdims=True)
    return np.where(d == 0, d, d / nrm).astype(np.float32)      # keeps the sign of every zero


@pytest.fixture(scope="module")
def rc_noise():
    from nrc_amd import rc_ext
    h = rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)
    h.load_weights(common.weights_np())
    return h


@pytest.fixture(scope="module")
def rc_smooth():
    from nrc_amd import rc_ext
    h = rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)
    h.load_weights(common.weights_material_np(True))
    return h


def envmap_case(rc, n, cfg=None, weights_np=None):
    """cfg, weights_np: the config the handle was made with and the weights it holds (None: the hotdog defaults,
    common.weights_np())."""
    from nrc_amd import rc_ext
    from oracle import cache_ref
    cfg = nrc_amd.hotdog_config() if cfg is None else cfg
    rays, rnd = common.secondary_case(n, seed=11)
    d = adversarial_dirs(n, seed=n)
    rays["directions"] = rays["viewdirs"] = d
    out = rc.render_rays(rays, rnd, rc_ext.RC_PASS_CACHE | rc_ext.RC_PASS_SECONDARY, outputs=["env_map_rgb"])
    torch.cuda.synchronize()
    hip = out["env_map_rgb"].cpu().numpy()
    w = common.weights_np() if weights_np is None else weights_np
    vd = torch.from_numpy(d)
    with torch.no_grad():
        b64 = cache_ref.model_env_map_rgb(common.to_torch(w, torch.float64), cfg, vd.double()).numpy()
        b32 = cache_ref.model_env_map_rgb(common.to_torch(w), cfg, vd).numpy()
        with split3(cache_ref):
            emu = cache_ref.model_env_map_rgb(common.to_torch(w), cfg, vd).numpy()
    return hip, b32, b64, emu


@pytest.mark.parametrize("n", [1, 3, 255, 257, 4097])
def test_envmap_at_the_fp32_floor(rc_noise, n):
    """k_envmap (pos_enc(dir, 0, 4) -> 3 x 256 -> skip -> 128 -> rgb) on adversarial view directions; batch sizes
    around the 32-ray tiles and the 128-ray workgroups.  Measured HIP / floor: split build 0.6-2.5, fp32 build 0.1-1.9
    (n = 1, a single axis, has a floor of 3e-10 on one channel: there the device sin / exp, ~3e-7 of the value, is
    the error, 0.74-1.45 of the old EPS = 2e-7 bound, hence EPS_ENV); the 3-product emulation lands 20-500 x the bound."""
    floor_check(f"env_map_rgb n={n}", *envmap_case(rc_noise, n), eps=EPS_ENV)


# ---------------------------------------------------------------------------------------------
# k_cache_shader (launch-per-stage plan): the cache shader on the last level's samples
# ---------------------------------------------------------------------------------------------
def acc_order():
    """Feature index of hidden-feature slot (step s, half h) in the accumulator layout of hbuf (rc_pack_host.h acc_feat)."""
    s, h = np.meshgrid(np.arange(32), np.arange(2), indexing="ij")
    return 32 * (s // 16) + (s % 4) + 8 * ((s % 16) // 4) + 4 * h           # [32, 2]


def shader_inputs(rc, n, S=None, cfg=None):
    """The shader's inputs as the HIP path computed them: hidden density feature [n, S, 64] (hbuf: [tile][step][half,
    point]), appearance features [n, S, 32] (app: feature-major), normals_pred [n, S, 3] (SoA), means [n, S, 3].
    S: the last level's sample count, taken from cfg (None: the hotdog defaults) where it is not given."""
    S = (nrc_amd.hotdog_config() if cfg is None else cfg).sampling_strategy[-1][2] if S is None else S
    np_ = n * S
    tiles = (np_ + 31) // 32
    hb = rc.workspace("hbuf")[: tiles * 32 * 64].reshape(tiles, 32, 2, 32)          # [tile, step, half, point]
    hidden = np.empty((tiles * 32, 64), np.float32)
    hidden[:, acc_order()] = hb.transpose(0, 3, 1, 2).reshape(tiles * 32, 32, 2)
    app = rc.workspace("app")[: 32 * np_].reshape(32, np_).T
    nrm = rc.workspace("normals_pred")[: 3 * np_].reshape(3, np_).T
    means = rc.workspace("means2")[: 3 * np_].reshape(3, np_).T
    shade = rc.workspace("shade")[: 15 * np_].reshape(15, np_).T
    r = lambda a: np.ascontiguousarray(a[:np_].reshape(n, S, -1))
    return r(hidden), r(app), r(nrm), r(means), r(shade)


SHADE_KEYS = (("rgb", 0), ("direct_diffuse_rgb", 3), ("indirect_diffuse_rgb", 6), ("indirect_specular_rgb", 9),
              ("albedo_rgb", 12))       # rc_internal.h RC_SH_RGB / AD / ID / IS / TINT


def cache_shader_case(rc, weights_np, n=64, cfg=None):
    """cfg: the config the handle was made with (None: the hotdog defaults)."""
    from oracle import cache_ref
    cfg = nrc_amd.hotdog_config() if cfg is None else cfg
    rays = nrc_amd.synthetic_rays(n, seed=31)
    rc.set_fused(False)
    try:
        rc.render_rays(rays.hot_fields(), {"jitter": common.jitters(n, seed=5)})
        torch.cuda.synchronize()
    finally:
        rc.set_fused(True)
    hidden, app, nrm, means, shade = shader_inputs(rc, n, cfg=cfg)
    rt = common.rays_torch(rays)

    def run(dtype, patched=False):
        w = common.to_torch(weights_np, dtype)
        t = lambda a: torch.from_numpy(a).to(dtype)
        sres = {"means": t(means), "feature": t(hidden), "normals_to_use": t(nrm)}
        rr = {"viewdirs": rt["viewdirs"].to(dtype), "origins": rt["origins"].to(dtype)}
        with torch.no_grad(), (split3(cache_ref) if patched else contextlib.nullcontext()):
            o = cache_ref.cache_shader(w, cfg, rr, sres, app=t(app))
        return np.concatenate([o[k].numpy() for k, _ in SHADE_KEYS], axis=-1)

    hip = np.concatenate([shade[..., c:c + 3] for _, c in SHADE_KEYS], axis=-1)
    return hip, run(torch.float32), run(torch.float64), run(torch.float32, patched=True)


@pytest.mark.parametrize("smooth", [False, True])
def test_cache_shader_at_the_fp32_floor(rc_noise, rc_smooth, smooth):
    """k_cache_shader on its own inputs, every shade channel (rgb, ambient diffuse, indirect diffuse, indirect
    specular, tint); the white-noise and the smooth weights.  k_cache_fused runs the same shader_tile and equals this
    plan bitwise (test_gpu_parity.py test_fused_plan_equals_staged_plan), so the bound holds for it too.
    Measured HIP / floor per channel: 0.6-1.2 in the split build, 0.7-1.3 in the fp32 build (white noise; at most
    0.31 of the bound); the 3-product emulation lands 10.9-89 x the bound."""
    rc = rc_smooth if smooth else rc_noise
    w = common.weights_material_np(True) if smooth else common.weights_np()
    floor_check(f"cache shader smooth={smooth}", *cache_shader_case(rc, w))


# ---------------------------------------------------------------------------------------------
# k_transient_shader: the transient shader on the last level's samples of the primary rays
# ---------------------------------------------------------------------------------------------
# tshade channels (rc_internal.h RC_TS_*) -> the oracle stage's key (channels of width 1 come from [.., 1] keys)
TSHADE_KEYS = (("direct_diffuse_rgb", 0, 3), ("direct_specular_rgb", 3, 3), ("albedo_rgb", 6, 3), ("tint_ibrdf", 9, 3),
               ("roughness", 12, 1), ("n_dot_l_rgb", 13, 1), ("irradiance_rgb", 14, 1), ("occ", 15, 1),
               ("light_dists", 16, 1), ("ray_dists", 17, 1))
# carried by split layers (the heads, the BRDF and integrated-BRDF chains): the emulation must land POWER x beyond
# (measured on the oracle's own inputs: 15.7-44 x).  n.l, irradiance, occlusion and the distances are geometry of the
# inputs, no MLP between them and the workspace.  Direct diffuse = albedo n.l L / pi carries the floor of the light's
# 1 / d^2 falloff (2.6e-6 against the albedo head's 8e-8), so the emulation reaches only 6.9-9.7 x there: its split
# layer, the albedo head, is held with power on its own channel (on the GPU: 9.0-9.3 x on direct diffuse)
TSHADE_MLP = ("direct_specular_rgb", "albedo_rgb", "tint_ibrdf", "roughness")


def transient_shader_case(rc, weights_np, n=48):
    """k_transient_shader's inputs (the same workspace buffers as k_cache_shader's) fed to transient_ref.transient_shader
    in fp64, fp32 and the 3-product emulation.  Returns {key: (hip, b32, b64, emu)}: every tshade channel but the camera
    distance, and the irradiance trunk's 64 features (t_irr, accumulator layout like hbuf)."""
    from oracle import cache_ref, transient_ref
    cfg = nrc_amd.cornell_transient_config()
    rays = nrc_amd.synthetic_transient_rays(n)
    rc.render_transient(rays.hot_fields(), {"jitter": common.jitters(n, seed=5)})
    torch.cuda.synchronize()
    hidden, app, nrm, means, _ = shader_inputs(rc, n)
    np_ = n * 32
    ts = rc.workspace("tshade")[: 19 * np_].reshape(19, np_).T.reshape(n, 32, 19)
    tiles = np_ // 32
    ib = rc.workspace("t_irr")[: tiles * 32 * 64].reshape(tiles, 32, 2, 32)
    irr = np.empty((np_, 64), np.float32)
    irr[:, acc_order()] = ib.transpose(0, 3, 1, 2).reshape(np_, 32, 2)
    rt = common.rays_torch(rays)

    def run(dtype, patched=False):
        w = common.to_torch(weights_np, dtype)
        t = lambda a: torch.from_numpy(a).to(dtype)
        sres = {"means": t(means), "feature": t(hidden), "normals_to_use": t(nrm)}
        rr = {k: v.to(dtype) for k, v in rt.items()}
        with torch.no_grad(), (split3(transient_ref, cache_ref) if patched else contextlib.nullcontext()):
            o = transient_ref.transient_shader(w, cfg, rr, sres, app=t(app))
            # the irradiance trunk (transient_ref.transient_indirect_diffuse's first two layers)
            lights = rr["lights"][:, None, :] * torch.ones_like(sres["means"])
            x = torch.cat([sres["feature"], t(app), transient_ref.light_enc(lights, cfg.transient.deg_lights)], dim=-1)
            x = torch.relu(transient_ref.dense(w, f"{transient_ref.SH}/irradiance_layers_0", x))
            x = torch.relu(transient_ref.dense(w, f"{transient_ref.SH}/irradiance_layers_1", x))
        res = {k: o[k][..., :c].numpy() for k, _, c in TSHADE_KEYS}
        res["t_irr"] = x.numpy()
        return res

    hip = {k: ts[..., ch:ch + c] for k, ch, c in TSHADE_KEYS}
    hip["t_irr"] = irr.reshape(n, 32, 64)
    b32, b64, emu = run(torch.float32), run(torch.float64), run(torch.float32, patched=True)
    return {k: (hip[k], b32[k], b64[k], emu[k]) for k in hip}


@pytest.mark.parametrize("smooth", [False, True])
def test_transient_shader_at_the_fp32_floor(smooth):
    """k_transient_shader on its own inputs: every tshade channel (direct diffuse / specular, albedo, tint x
    integrated BRDF, roughness, n.l, irradiance, occlusion, light and ray distance; the camera distance has no oracle
    key) and the irradiance trunk's features that k_transient_bins' per-bin heads read (t_irr).  The emulation power
    is asserted on the channels split layers carry (TSHADE_MLP, t_irr).  Measured HIP / floor, split build and fp32
    build: 0.5-2.1 and 0.7-2.3 on every channel; the emulation lands 18.5-42 x the bound on TSHADE_MLP and >= 25 x on
    every live t_irr feature (a unit that is zero on every sample has bound and emulation error 0)."""
    from nrc_amd import rc_ext
    w = common.weights_transient_np(smooth=smooth)
    rc = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    rc.load_weights(w)
    for k, case in transient_shader_case(rc, w).items():
        floor_check(f"tshade {k} smooth={smooth}", *case, power=k in TSHADE_MLP or k == "t_irr")


# ---------------------------------------------------------------------------------------------
# k_transient_shader + k_transient_bins: the floor form of the whole transient render on the smooth field
# ---------------------------------------------------------------------------------------------
TRANSIENT_BINS = ("rgb", "transient_direct_viz", "transient_indirect_viz", "transient_indirect_diffuse",
                  "transient_indirect_specular")
TRANSIENT_3 = ("integrated_rgb", "direct_rgb", "indirect_rgb", "diffuse_rgb", "specular_rgb", "albedo_rgb", "occ", "indirect_occ",
               "irradiance_rgb", "light_radiance_rgb", "n_dot_l_rgb", "direct_diffuse_rgb", "direct_specular_rgb",
               "indirect_diffuse_rgb", "indirect_specular_rgb")


# the per-bin heads' own keys (k_transient_bins, tile_xw2_split): there the 3-product emulation lands 22-41 x the bound.
# Every other key is held to the bound alone: the per-bin totals (rgb, *_viz) carry the floor of the direct term's
# binning, the occlusion / light keys no MLP at all, and on the integrated keys the emulation lands only 7-19 x the
# bound (whole-render floors of 1e-6 on values of 2)
TRANSIENT_POWER = ("transient_indirect_diffuse", "transient_indirect_specular")


@pytest.fixture(scope="module")
def rc_transient_smooth():
    from nrc_amd import rc_ext
    h = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    h.load_weights(common.weights_transient_np(smooth=True))
    return h


def transient_case(rc, n=48, jitter_seed=None):
    from oracle import cache_ref, transient_ref
    rays = nrc_amd.synthetic_transient_rays(n)
    rnd = None if jitter_seed is None else {"jitter": common.jitters(n, seed=jitter_seed)}
    out = rc.render_transient(rays.hot_fields(), rnd)
    torch.cuda.synchronize()
    hip = {k: v.cpu().numpy() for k, v in out.items()}
    with torch.no_grad():
        r32 = common.oracle_transient(n, jitter_seed, smooth=True)["render"]
        r64 = common.oracle_transient(n, jitter_seed, smooth=True, dtype=torch.float64)["render"]
        with split3(transient_ref, cache_ref):
            emu = common.oracle_transient(n, jitter_seed, smooth=True)["render"]
    return hip, r32, r64, emu


@pytest.mark.parametrize("jitter_seed", [None, 9])
def test_transient_render_at_the_fp32_floor(rc_transient_smooth, jitter_seed):
    """Smooth transient weights: every per-bin key ([n, 700, 3]; the per-bin heads of k_transient_bins,
    tile_xw2_split) and every integrated key against fp64, K x the fp32 oracle's floor.  The 3-product emulation
    applies to every layer but the density MLPs'.  Measured HIP / floor: 0.6-1.9 on every key in both builds (at most
    0.59 of the bound); the per-bin heads 0.6-1.3."""
    hip, r32, r64, emu = transient_case(rc_transient_smooth, jitter_seed=jitter_seed)
    for k in TRANSIENT_BINS + TRANSIENT_3:
        floor_check(k, hip[k], r32[k].numpy(), r64[k].numpy(), emu[k].numpy(), power=k in TRANSIENT_POWER)
