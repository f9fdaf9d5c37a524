"""The forward cache pass at non-default render settings, stage by stage (the cases, their configs and the
conditions on the reference are render_settings_cases.py, held on the CPU by test_render_settings.py).

The cache pass reads sixteen float settings from rc_config and the rest of the GPU suite runs it at one value of each, where
four biases are -1, two are -2, the far clamp equals the rays' far and rgb_max never clips.  Each setting reaches the
device by several hand-written routes (the launch-per-stage plan, the fused template, the level kernels, the material
stage's secondary EnvMap).  Here every case has one field off its default -- `combined` all of them -- and

  * each stage is held on the inputs the device itself computed (rc_set_fused(0) fills the workspace), the fp64 oracle stage
    being the exact value and the fp32 oracle stage the floor, with the bounds of tests/test_gpu_mlp_floor.py and of
    test_gpu_parity.py test_intermediates_sit_at_the_fp32_noise_floor_of_the_oracle unchanged: k_density_mlp / k_level
    under density_bias, k_cache_shader under the four shader biases and a binding rgb_max (the 3-product emulation 10 x
    beyond the bound there too), k_envmap under env_rgb_bias, and the sampler and compositor through the whole-pass
    floor check on the smooth weights, secondary rays with the fp64 oracle's picks handed over;
  * the launch plans stay one function: every output bitwise equal across rc_set_fused 0, 2, 1 and 3 under a binding
    clamp, moved percentiles and `combined`; the forced-resampling and secondary passes across 0, 2 and 1.

Measured HIP / floor over all cases and both weight sets (MI355X; split build | fp32-MFMA build):
  density stage            0.83-1.04 | 0.83-1.04   (an fp32 MFMA chain in both builds)
  shader stage             0.43-1.63 | 0.56-1.47   per channel, at most 0.43 | 0.37 of the bound; the 3-product emulation
                                                   lands 10.9-94.2 x the bound (rgb_max: 10.9-80.7, combined: 11.6-88.7)
  EnvMap stage             1.49-2.45 | 0.80-1.41   at most 0.60 | 0.33 of the bound; emulation 59.6-100.9 x
  primary whole pass       0.49-2.09 | 0.49-2.09   (at the defaults, same rays: 0.49-2.09; the 2.09 is tdist1, 0.69 of the bound)
  secondary whole pass     0.39-2.75 | 0.39-2.75   (at the defaults: 0.46-1.48)
The worst whole-pass figure is raydist_p = -0.5: weights1 2.75 and tdist1 2.13 x the floor (0.83 of the bound); under every
other setting the worst key is at or below 1.6 x, or is the defaults' own tdist1.  Every setting moves its outputs by
5e3-5e5 x the granted tolerance (the guards), so a dropped or exchanged field is out of reach of every bound here.
"""
import numpy as np
import pytest
import torch

import common
import nrc_amd
import render_settings_cases as rs
import test_gpu_mlp_floor as mf
from nrc_amd import rc_ext
from nrc_amd.model import _CACHE_DEVICE_KEYS
from oracle import cache_ref

pytestmark = pytest.mark.gpu
N = 64
WEIGHTS = pytest.mark.parametrize("smooth", [False, True], ids=["noise", "smooth"])
SECONDARY = rc_ext.RC_PASS_CACHE | rc_ext.RC_PASS_SECONDARY


def case_config(name):
    return rs.DEFAULT if name == "default" else rs.config(name)


@pytest.fixture(scope="module")
def handle():
    """handle(name, smooth): the handle of a case on one of the two weight sets, made once per module."""
    made = {}

    def get(name, smooth):
        if (name, smooth) not in made:
            made[name, smooth] = common.make_rc(cfg=case_config(name), weights=rs.weights(smooth))
        return made[name, smooth]

    yield get
    made.clear()


@pytest.fixture(scope="module")
def defaults():
    """The fp64 and fp32 oracle at the defaults on the module's two batches (smooth weights): the whole-pass checks run at
    the defaults too, and the guards measure each setting's effect against the fp64 one."""
    p64, p32 = (rs.flatten(rs.oracle_primary(rs.DEFAULT, N, dt)) for dt in (torch.float64, torch.float32))
    s64, s32, picks = rs.secondary_refs(rs.DEFAULT, N, use_env_map=False)
    return {"primary": (p64, p32), "secondary": (rs.flatten(s64, True), rs.flatten(s32, True), picks)}


def staged(rc, call):
    """call() on the launch-per-stage plan, which leaves every intermediate in the workspace."""
    rc.set_fused(0)
    try:
        out = call()
        torch.cuda.synchronize()
    finally:
        rc.set_fused(1)
    return {k: v.cpu().numpy() for k, v in out.items()}


def level_buffers(rc, n):
    """sdist / tdist / weights / density of every level as the last call left them."""
    b = {}
    for l, S in enumerate(rs.SAMPLES):
        for w, cols in (("sdist", S + 1), ("tdist", S + 1), ("weights", S), ("density", S)):
            b[f"{w}{l}"] = rc.workspace(f"{w}{l}")[: n * cols].reshape(n, cols)
    return b


def pass_check(what, hip, c64, c32, keys=rs.PASS_KEYS):
    """test_intermediates_sit_at_the_fp32_noise_floor_of_the_oracle's bound on every key: max|HIP - fp64| <= 3 x
    max|fp32 - fp64| + 1e-7, every entry."""
    ratios, of_bound, bad = {}, {}, []
    for k in keys:
        a = np.asarray(hip[k], np.float64).reshape(c64[k].shape)
        assert np.isfinite(a).all(), k
        floor, err = float(np.abs(c32[k] - c64[k]).max()), float(np.abs(a - c64[k]).max())
        ratios[k] = round(err / floor, 2) if floor > 0 else (0.0 if err == 0 else float("inf"))
        of_bound[k] = round(err / (3.0 * floor + 1e-7), 2)
        if not err <= 3.0 * floor + 1e-7:
            bad.append((k, err, floor))
    top = max(of_bound, key=of_bound.get)
    print(what, "HIP / floor:", ratios, "worst", max(ratios.values()), "| largest share of the bound:", top, of_bound[top])
    assert not bad, (what, bad)


def moved(name, which):
    fields = rs.FIELDS if name == "combined" else (name,)
    return tuple(sorted({k for f in fields for k in rs.MOVES[f][which] if k in rs.PASS_KEYS}))


# ---------------------------------------------------------------------------------------------
# each stage on the device's own inputs
# ---------------------------------------------------------------------------------------------
@WEIGHTS
@pytest.mark.parametrize("name", rs.DENSITY_CASES)
def test_density_stage(handle, name, smooth):
    """k_density_mlp / k_level under density_bias: density{l} of all three levels against cache_ref.density_mlp at the
    device's own means{l}, every entry, 3 x the fp32 oracle stage's distance from fp64 + 1e-7."""
    cfg, rc = rs.config(name), handle(name, smooth)
    rays, jit = rs.primary_batch(N)
    staged(rc, lambda: rc.render_rays(rays.hot_fields(), {"jitter": jit}, outputs=["rgb"]))
    hip, c64, c32, d64 = {}, {}, {}, {}
    for l, S in enumerate(rs.SAMPLES):
        np_ = N * S
        means = rc.workspace(f"means{l}")[: 3 * np_].reshape(3, np_).T.reshape(N, S, 3)
        hip[f"density{l}"] = rc.workspace(f"density{l}")[:np_].reshape(N, S)
        for dt, into, c in ((torch.float64, c64, cfg), (torch.float32, c32, cfg), (torch.float64, d64, rs.DEFAULT)):
            with torch.no_grad():
                o = cache_ref.density_mlp(common.to_torch(rs.weights(smooth), dt), c, l, common.rays_torch(rays, dt),
                                          torch.from_numpy(means).to(dt), want_grad_normals=False)
            into[f"density{l}"] = o["density"].double().numpy()
    keys = tuple(hip)
    rs.guard(f"density stage {name}", keys, c64, c32, d64)
    pass_check(f"density stage {name} smooth={smooth}", hip, c64, c32, keys)


@WEIGHTS
@pytest.mark.parametrize("name", rs.SHADER_CASES)
def test_shader_stage(handle, name, smooth):
    """k_cache_shader under the four shader biases, a clamp that binds on about half of each clamped channel, and all of
    them: the fifteen shade channels on the device's own inputs, mlp_floor.floor_check as it stands, its power arm
    included.  The clamp is Lipschitz: a clipped entry needs no exclusion and none is made."""
    cfg = rs.config(name)
    case = mf.cache_shader_case(handle(name, smooth), rs.weights(smooth), N, cfg=cfg)
    if name in rs.CLIPPED_CASES:
        hip = case[0].reshape(-1, 15)
        share = [float((hip[:, c:c + 3] >= np.float32(cfg.rgb_max)).mean()) for _, c in rs.SHADE_KEYS[1:4]]
        print(f"shader stage {name} smooth={smooth}: clipped share on the device", np.round(share, 3))
        assert all(0.1 <= s <= 0.9 for s in share), share
        assert float(hip[:, 3:12].max()) == np.float32(cfg.rgb_max)
    mf.floor_check(f"shader stage {name} smooth={smooth}", *case, cfg=cfg)


@WEIGHTS
@pytest.mark.parametrize("name", rs.ENVMAP_CASES)
def test_envmap_stage(handle, name, smooth):
    """k_envmap under env_rgb_bias on mlp_floor's adversarial view directions, 257 rays."""
    cfg = rs.config(name)
    case = mf.envmap_case(handle(name, smooth), 257, cfg=cfg, weights_np=rs.weights(smooth))
    mf.floor_check(f"envmap stage {name} smooth={smooth}", *case, eps=mf.EPS_ENV, cfg=cfg)


@pytest.mark.parametrize("name", ("default",) + rs.PRIMARY_PASS_CASES)
def test_primary_pass_at_the_fp32_floor(handle, defaults, name):
    """The sampler and the compositor on primary rays (smooth weights): sdist / tdist / weights / density of every level,
    rgb, acc and the four distance outputs -- the three percentile outputs by position -- within 3 x the fp32 oracle's
    own distance from fp64 under the same config."""
    cfg, rc = case_config(name), handle(name, True)
    rays, jit = rs.primary_batch(N)
    hip = staged(rc, lambda: rc.render_rays(rays.hot_fields(), {"jitter": jit}))
    hip.update(level_buffers(rc, N))
    if name == "default":
        c64, c32 = defaults["primary"]
    else:
        c64, c32 = (rs.flatten(rs.oracle_primary(cfg, N, dt)) for dt in (torch.float64, torch.float32))
        rs.guard(f"primary pass {name}", moved(name, 0), c64, c32, defaults["primary"][0])
    pass_check(f"primary pass {name}", hip, c64, c32)


@pytest.mark.parametrize("name", ("default",) + rs.SECONDARY_PASS_CASES)
def test_secondary_pass_at_the_fp32_floor(handle, defaults, name):
    """The same on secondary rays: the far clamp, the near replacement and the power-ladder distances.  The fp64 oracle's
    picks go to the device (and to the fp32 oracle) through resample_inds, which removes the one discontinuous step; no
    ray is left out."""
    cfg, rc = case_config(name), handle(name, True)
    rays, rnd = rs.secondary_batch(N)
    if name == "default":
        c64, c32, picks = defaults["secondary"]
    else:
        r64, r32, picks = rs.secondary_refs(cfg, N, use_env_map=False)
        c64, c32 = rs.flatten(r64, True), rs.flatten(r32, True)
        rs.guard(f"secondary pass {name}", moved(name, 1), c64, c32, defaults["secondary"][0])
    rnd = dict(jitter=rnd["jitter"], resample_inds=picks)
    hip = staged(rc, lambda: rc.render_rays(rays, rnd, SECONDARY | rc_ext.RC_PASS_NO_ENVMAP))
    assert np.array_equal(rc.workspace("inds", np.int32)[:N], picks)
    hip.update(level_buffers(rc, N))
    pass_check(f"secondary pass {name}", hip, c64, c32)


# ---------------------------------------------------------------------------------------------
# the launch plans stay one function
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jitter", [False, True], ids=["det", "jit"])
@pytest.mark.parametrize("n", [1, 130])
@pytest.mark.parametrize("name", ["rgb_max", "combined", "percentiles"])
def test_plans_stay_bitwise_equal(handle, name, n, jitter):
    """test_gpu_shader_fill.test_plans_stay_bitwise_equal under a binding clamp, moved percentiles and `combined`: every
    output key equal across rc_set_fused 0, 2, 1 and 3 (on the fp32-MFMA build mode 1 is k_cache_fused_team with its own
    copy of the shader glue)."""
    rc = handle(name, False)
    rays = nrc_amd.synthetic_rays(n, seed=4100 + n)
    rnd = {"jitter": common.jitters(n, seed=6)} if jitter else None
    res = {}
    try:
        for mode in (0, 2, 1, 3):
            rc.set_fused(mode)
            out = rc.render_rays(rays.hot_fields(), rnd, outputs=list(_CACHE_DEVICE_KEYS))
            torch.cuda.synchronize()
            res[mode] = {k: v.cpu().numpy() for k, v in out.items()}
    finally:
        rc.set_fused(1)
    for k in _CACHE_DEVICE_KEYS:
        assert res[0][k].shape[0] == n and np.isfinite(res[0][k]).all(), k
        for mode in (2, 1, 3):
            assert np.array_equal(res[0][k], res[mode][k]), (k, f"plan 0 vs plan {mode}")
    if name in rs.CLIPPED_CASES:          # composited from clamped samples with weights that sum to acc <= 1
        assert float(res[0]["indirect_diffuse_rgb"].max()) <= np.float32(rs.config(name).rgb_max) * (1 + 1e-6)


@pytest.mark.parametrize("n", [257, 24577])
def test_resampling_and_secondary_passes_equal_across_plans(handle, n):
    """test_gpu_grid_geometries.test_level_kernels_equal_the_separate_kernels under `combined`: the forced-resampling pass
    and the secondary pass with and without its EnvMap on plans 0, 2 and 1 -- densities, fence posts and outputs bitwise
    equal.  From 24 576 rays plan 1 runs a proposal level with its sampling in front (k_level_ray)."""
    rc = handle("combined", False)
    rc.set_graph_mode(0)
    rays = nrc_amd.synthetic_rays(n, seed=31).hot_fields()
    srays, srnd = common.secondary_case(n, seed=12)
    g = np.random.default_rng(4).gumbel(size=(n, 32)).astype(np.float32)
    cases = [(rays, {"jitter": common.jitters(n, seed=9), "gumbel": g}, rc_ext.RC_PASS_CACHE | rc_ext.RC_PASS_RESAMPLE,
              ["rgb", "acc", "distance_median", "distance_percentile_95", "means"]),
             (srays, srnd, SECONDARY | rc_ext.RC_PASS_NO_ENVMAP, ["rgb", "acc", "distance_mean", "distance_percentile_5"]),
             (srays, srnd, SECONDARY, ["rgb", "acc", "env_map_rgb", "rgb_no_env", "indirect_specular_rgb"])]
    try:
        for fields, rnd, mask, outs in cases:
            res = {}
            for mode in (0, 2, 1):
                rc.set_fused(mode)
                o = rc.render_rays(fields, rnd, mask, outputs=outs)
                torch.cuda.synchronize()
                res[mode] = {k: v.cpu() for k, v in o.items()}
                for nm, cnt in (("density0", n * 64), ("density1", n * 64), ("density2", n * 32), ("tdist1", n * 65), ("tdist2", n * 33)):
                    res[mode][nm] = torch.from_numpy(rc.workspace(nm)[:cnt].copy())
            for mode in (2, 1):
                for k in res[0]:
                    assert torch.equal(res[0][k], res[mode][k]), (mask, mode, k)
            assert float(res[0]["density1"].abs().sum()) > 0.0 and bool(torch.isfinite(res[0]["rgb"]).all())
            if mask & rc_ext.RC_PASS_SECONDARY:          # the far clamp of `combined` binds
                assert float(res[0]["tdist2"].max()) <= 1.5 + 1e-5
    finally:
        rc.set_fused(1)
        rc.set_graph_mode(1)
