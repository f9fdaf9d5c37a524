"""The conditions on the reference that tests/test_gpu_render_settings.py rests on (render_settings_cases.py), on the CPU
oracle alone: 16 rays through cache_ref.cache_forward in fp64 and fp32, white-noise and smooth weights.

  * guard: under every case the fp64 result differs from the fp64 result at the defaults, in each output the table names, by
    more than GUARD_FACTOR (100) x the tolerance the GPU test grants that output -- a call that dropped the setting on its
    way to a kernel could not pass.  The sampler's and the compositor's outputs take the whole-pass tolerance (3 x the fp32
    pass's distance from the fp64 pass + 1e-7); the shade channels the stage tolerance (K x the fp32 shader's distance from
    the fp64 shader on the same inputs + EPS x max|value|, per channel), which is what the GPU shader check grants;
  * swap guard: `combined` with the two values of any pair of fields whose defaults coincide exchanged differs from
    `combined` itself by the same margin in at least one output -- an exchange of two such fields could not pass;
  * the clamp binds on 10-90 % of each clamped channel, the far clamp on every secondary ray, and the replaced near lies
    strictly inside (near, far) on at least half of them."""
import functools

import numpy as np
import pytest
import torch

import render_settings_cases as rs

N = 16
WEIGHTS = pytest.mark.parametrize("smooth", [False, True], ids=["noise", "smooth"])


def moved_keys(name):
    fields = rs.FIELDS if name == "combined" else (name,)
    return tuple(sorted({k for f in fields for k in rs.MOVES[f][s]}) for s in (0, 1))


@functools.lru_cache(maxsize=None)
def primary(name, smooth):
    """(fp64, fp32, the fp64 pass itself) of the primary rays under case `name` ("default": the defaults), flattened; the
    shade channels are the shader stage's on the fp64 pass's inputs."""
    cfg = rs.DEFAULT if name == "default" else rs.config(name)
    o64 = rs.oracle_primary(cfg, N, torch.float64, smooth)
    c64, c32 = rs.flatten(o64), rs.flatten(rs.oracle_primary(cfg, N, torch.float32, smooth))
    c64.update(rs.shader_stage(cfg, o64, torch.float64, smooth))
    c32.update(rs.shader_stage(cfg, o64, torch.float32, smooth))
    return c64, c32, o64


@functools.lru_cache(maxsize=None)
def secondary(name, smooth):
    cfg = rs.DEFAULT if name == "default" else rs.config(name)
    r64, r32, _ = rs.secondary_refs(cfg, N, smooth)
    return rs.flatten(r64, True), rs.flatten(r32, True)


def test_every_value_is_distinct():
    """No two case values are equal and none equals any default of the table's fields: an exchange of two fields, or a
    field dropped for its default, changes the config the kernels see."""
    flat = lambda v: tuple(v) if isinstance(v, tuple) else (v,)
    values = [float(x) for f in rs.FIELDS for x in flat(rs.VALUES[f])] + [rs.combined_rgb_max()]
    defaults = {float(x) for f in rs.FIELDS for x in flat(getattr(rs.DEFAULT, f))}
    assert len(set(values)) == len(values), sorted(values)
    assert not set(values) & defaults, sorted(set(values) & defaults)
    for f in rs.FIELDS:
        assert getattr(rs.config(f), f) == rs.VALUES[f] and getattr(rs.config("combined"), f) == (
            rs.combined_rgb_max() if f == "rgb_max" else rs.VALUES[f])
    assert len(rs.SWAP_PAIRS) == 7
    for a, b in rs.SWAP_PAIRS:
        assert getattr(rs.DEFAULT, a) == getattr(rs.DEFAULT, b), (a, b)


@WEIGHTS
@pytest.mark.parametrize("name", rs.CASES)
def test_guard(name, smooth):
    pk, sk = moved_keys(name)
    assert pk or sk
    if pk:
        c64, c32, o64 = primary(name, smooth)
        d64 = dict(primary("default", smooth)[0])
        d64.update(rs.shader_stage(rs.DEFAULT, o64, torch.float64, smooth))       # the default shader on the case's inputs
        rs.guard(f"{name} primary", pk, c64, c32, d64)
    if sk:
        c64, c32 = secondary(name, smooth)
        rs.guard(f"{name} secondary", sk, c64, c32, secondary("default", smooth)[0])


@WEIGHTS
@pytest.mark.parametrize("pair", rs.SWAP_PAIRS, ids=["-".join(p) for p in rs.SWAP_PAIRS])
def test_swap_guard(pair, smooth):
    cfg = rs.swapped(rs.config("combined"), *pair)
    c64, c32, o64 = primary("combined", smooth)
    s64, s32 = secondary("combined", smooth)
    w64 = rs.flatten(rs.oracle_primary(cfg, N, torch.float64, smooth))
    w64.update(rs.shader_stage(cfg, o64, torch.float64, smooth))                   # the swapped shader on combined's inputs
    ws64 = rs.flatten(rs.oracle_secondary(cfg, N, torch.float64, smooth), True)
    ratios = rs.effect_ratios(rs.PASS_KEYS + rs.SHADE_OUT, c64, c32, w64)
    ratios.update({"secondary " + k: r for k, r in rs.effect_ratios(rs.PASS_KEYS + ("env_map_rgb",), s64, s32, ws64).items()})
    top = max(ratios, key=ratios.get)
    print("swap", pair, "largest effect / granted tolerance:", top, f"{ratios[top]:.3g}")
    assert ratios[top] > rs.GUARD_FACTOR, (pair, ratios)


@WEIGHTS
@pytest.mark.parametrize("name", rs.CLIPPED_CASES)
@pytest.mark.parametrize("n", [N, 64])
def test_clipped_share(name, smooth, n):
    """A condition, not a measurement: a channel outside 10-90 % asks for another value in the table."""
    cfg = rs.config(name)
    o64 = primary(name, smooth)[2] if n == N else rs.oracle_primary(cfg, n, torch.float64, smooth)
    share = rs.clipped_share(o64, cfg)
    print(name, "smooth" if smooth else "noise", n, "rgb_max", cfg.rgb_max, share)
    for k, s in share.items():
        assert 0.1 <= s <= 0.9, (name, k, s)


@pytest.mark.parametrize("n", [N, 64])
def test_far_clamp_binds_and_the_near_is_replaced(n):
    rays, _ = rs.secondary_batch(n)
    for name in ("env_map_distance", "combined"):
        assert float(np.asarray(rays["far"]).min()) > rs.config(name).env_map_distance == 1.5
    for name in ("shadow_normal_eps_dot_min", "combined"):
        near, new, far = rs.replaced_near(rs.config(name), rays)
        inside = (new > near) & (new < far)
        print(name, n, "replaced near strictly inside (near, far):", float(inside.mean()))
        assert inside.mean() >= 0.5, (name, inside.mean())
