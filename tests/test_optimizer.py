"""The cache stage's optimizer on the CPU: the learning-rate schedule against closed forms, the group of every tensor
against a simulation of optax.chain / optax.masked, the float32 Adam restatement against fp64, and the new ABI entry
points in the binding."""
import math
import re

import numpy as np
import pytest

import nrc_amd
import optimizer_ref as ref
from nrc_amd import rc_ext, train
from nrc_amd.config import OptimizerConfig

CFG = OptimizerConfig()
PREFIXES = [e.prefix for e in CFG.extra_opt_params]


def _cache_stage_names():
    """Every tensor name of the four cache-stage gradient layouts (density levels 0-2 and the shader layout)."""
    shapes = nrc_amd.param_shapes(nrc_amd.hotdog_config())
    dens = [k for k in shapes if k.startswith("params/Cache/Sampler/") and "pred_normals_layer" not in k]
    app = [(k, shapes[k]) for k in shapes if k.startswith("params/Cache/Shader/appearance_grid/")]
    shader, _ = train.shader_grad_layout(nrc_amd.hotdog_config(), app)
    return dens + [n for n, _, _ in shader]


# ---- learning-rate schedule ---------------------------------------------------------------------------------------

def test_schedule_closed_forms():
    cache = dict(CFG.groups())["Cache"]
    lr = lambda s: float(train.learning_rate_decay(s, **cache))
    assert lr(0) == pytest.approx(1e-8 * 0.01, rel=1e-6)
    assert lr(2500) == pytest.approx(0.01 * 10 ** -0.2, rel=1e-6)
    assert lr(25000) == pytest.approx(1e-4, rel=1e-6)
    assert lr(40000) == pytest.approx(1e-4, rel=1e-6)
    # halfway through the delay: mult + (1 - mult) sin(pi/4), times the log-linear value at t = 0.05
    want = (1e-8 + (1 - 1e-8) * math.sin(math.pi / 4)) * 0.01 * 10 ** (-2 * 0.05)
    assert lr(1250) == pytest.approx(want, rel=1e-6)
    main = dict(CFG.groups())["main"]
    assert float(train.learning_rate_decay(25000, **main)) == pytest.approx(1e-3, rel=1e-6)
    assert float(train.learning_rate_decay(0, 0.0, 0.0, 10)) == 0.0
    assert float(train.learning_rate_decay(5, 1.0, 0.5, 10)) == pytest.approx(0.5 ** 0.5, rel=1e-6)   # no delay


def test_schedule_matches_fp64_everywhere():
    for name, sched in CFG.groups():
        for s in (0, 1, 7, 100, 1249, 2499, 2500, 2501, 12345, 24999, 25000, 60000):
            got = float(train.learning_rate_decay(s, **sched))
            assert got == pytest.approx(ref.lr_decay_f64(s, **sched), rel=2e-6), (name, s)


def test_material_variant_and_trainer_scaling():
    mat = dict(OptimizerConfig(material=True).groups())
    assert mat["Cache"]["lr_init"] == 0.002 and mat["Cache"]["lr_final"] == 2e-5 and mat["Cache"]["lr_delay_steps"] == 0
    assert float(train.learning_rate_decay(0, **mat["Cache"])) == pytest.approx(0.002, rel=1e-6)   # no delay
    assert mat["SurfaceLightFieldMem"]["lr_init"] == 0.01
    assert mat["main"]["lr_init"] == 0.01            # the main Adam has no _material variant
    # batch 16384 of base 65536: scale_factor 4 -> lr / 4 * lr_factor, steps * 4 // train_length_mult
    sc = OptimizerConfig(batch_size=16384, lr_factor=2.0, train_length_mult=2)
    assert sc.scale_factor == 4
    g = dict(sc.groups())
    assert g["Cache"]["lr_init"] == pytest.approx(0.01 / 4 * 2.0) and g["Cache"]["lr_final"] == pytest.approx(1e-4 / 4 * 2.0)
    assert g["Cache"]["lr_delay_steps"] == 2500 * 4 // 2 and g["Cache"]["max_steps"] == 25000 * 4 // 2
    assert g["main"]["max_steps"] == 50000 and g["main"]["lr_init"] == pytest.approx(0.005)
    hot = dict(CFG.groups())
    assert CFG.scale_factor == 1 and hot["Cache"]["max_steps"] == 25000 and hot["EnvMap"]["lr_init"] == 5e-4


def test_train_frac():
    assert train.train_frac_at(0, 25000) == 0.0
    assert train.train_frac_at(24999, 25000) == 1.0
    assert train.train_frac_at(30000, 25000) == 1.0
    assert train.train_frac_at(12499.5, 25000) == pytest.approx(0.5)


# ---- groups -------------------------------------------------------------------------------------------------------

def test_param_group_matches_chain_masked_simulation():
    names = _cache_stage_names()
    assert len(names) > 70
    extra = ["params/Cache/EnvMap/layer_0/kernel", "params/Cache/Shader/EnvMap/layer_0/bias",
             "params/MaterialShader/bottleneck_layer/kernel", "params/LightSampler/layers_0/kernel",
             "params/Vignette/kernel", "params/Cache/Shader/SurfaceLightFieldMem/layer_0/kernel",
             "params/CacheX/SurfaceLightFieldY/kernel"]
    sim = ref.simulate_groups(names + extra, PREFIXES)
    for n in names + extra:
        assert len(sim[n]) == 1, (n, sim[n])                 # every tensor receives exactly one Adam
        assert train.param_group(n) == sim[n][0], (n, sim[n])
    groups = {n: train.param_group(n) for n in names}
    assert {g for g in groups.values()} == {"Cache", "SurfaceLightField"}
    assert all((g == "SurfaceLightField") == ("/SurfaceLightField/" in n) for n, g in groups.items())
    assert train.param_group("params/Cache/EnvMap/layer_0/kernel") == "EnvMap"
    assert train.param_group("params/Cache/Shader/EnvMap/layer_0/bias") == "EnvMap"
    assert train.param_group("params/Vignette/kernel") == "main"
    assert train.param_group("params/CacheX/SurfaceLightFieldY/kernel") == "main"     # whole path elements only


# ---- the Adam restatement -----------------------------------------------------------------------------------------

def _grads(rng, n, step, infs=True):
    g = rng.standard_normal(n).astype(np.float32) * np.float32(10.0 ** rng.uniform(-4, 1))
    g[rng.random(n) < 0.05] = 0.0
    if step % 5 == 3:
        g[:] = 0.0                                           # a zero gradient with non-zero moments still moves p
    g[7] = np.nan
    if infs:
        g[8] = np.inf
        g[9] = -np.inf
    g[10:20] = np.float32(1e-40) * rng.standard_normal(10).astype(np.float32)      # subnormal
    return g


@pytest.mark.parametrize("clip", [(0.0, 0.0), (0.5, 0.0), (0.0, 3.0), (0.2, 1.5)])
def test_adam_f32_restatement_against_fp64(clip):
    max_val, max_norm = clip
    cfg = OptimizerConfig(grad_max_val=max_val, grad_max_norm=max_norm)
    rng = np.random.default_rng(3)
    n = 4000
    grp = np.zeros(n, np.int64)
    grp[2500:] = 2                                           # two groups with their own schedule
    groups = [s for _, s in cfg.groups()]
    p32 = rng.standard_normal(n).astype(np.float32) * np.float32(0.1)
    p64, mu32, nu32 = p32.astype(np.float64), np.zeros(n, np.float32), np.zeros(n, np.float32)
    mu64, nu64, mabs = np.zeros(n), np.zeros(n), np.zeros(n)
    start = 2600                                             # past the delay: steps of a visible size
    for t in range(start, start + 50):
        g = _grads(rng, n, t, infs=max_norm == 0)      # an inf makes the float32 norm inf and the multiplier 0
        sc = train.adam_scalars(t, cfg)
        m32 = ref.norm_mult([g], max_val, max_norm, np.float32)[1] if max_norm > 0 else None
        m64 = ref.norm_mult([g], max_val, max_norm)[1] if max_norm > 0 else None
        p32, mu32, nu32 = ref.adam_f32(p32, g, mu32, nu32, grp, sc, m32)
        p64, mu64, nu64 = ref.adam_f64(p64, g, mu64, nu64, grp, t, groups, cfg.b1, cfg.b2, cfg.eps, max_val, m64)
        assert p32.dtype == np.float32 and np.all(np.isfinite(p32))
        # the moments follow fp64 to float32 rounding; FLT_MAX-sized entries are huge and still finite
        # float32 rounding of mu is relative to the sum of the magnitudes that entered it (cancellation aside)
        mabs = (1 - cfg.b1) * np.abs(ref.sanitize(g, max_val, np.float64)) * (1.0 if m64 is None else m64) + cfg.b1 * mabs
        assert np.all(np.abs(mu32 - mu64) <= 1e-5 * mabs + 1e-37), t
    # +-FLT_MAX (from +-inf) squares to inf in float32: nu = inf and the entry stops moving, where fp64 keeps a finite nu;
    # the reference computes in float32, so those two entries are checked for that and left out of the fp64 comparison
    ok = np.ones(n, bool)
    if max_val == 0 and max_norm == 0:
        assert np.all(np.isinf(nu32[8:10])) and np.all(np.isfinite(nu64[8:10]))
        ok[8:10] = False
    # each step moves an entry by at most ~lr; 50 steps of float32 rounding stay far below that
    lr = max(float(train.learning_rate_decay(start, **s)) for s in groups)
    assert np.max(np.abs(p32 - p64)[ok]) < 1e-3 * lr * 50
    if max_val > 0:
        assert np.max(np.abs(mu32)) <= max_val * (1 + 1e-6)


def test_adam_semantics():
    """nan_to_num, the dense update of zero gradients, the value clip and the norm clip, on hand-checked values."""
    sc = train.adam_scalars(0, OptimizerConfig(grad_max_val=1.0))
    grp = np.full(4, 1)
    p, mu, nu = ref.adam_f32(np.zeros(4, np.float32), np.array([np.nan, np.inf, -np.inf, 0.5], np.float32),
                             np.zeros(4, np.float32), np.zeros(4, np.float32), grp, sc)
    np.testing.assert_array_equal(mu, np.float32(0.1) * np.array([0, 1, -1, 0.5], np.float32))
    assert p[0] == 0 and p[1] < 0 < p[2]
    # a zero gradient with non-zero moments moves the parameter
    p2, _, _ = ref.adam_f32(p, np.zeros(4, np.float32), mu, nu, grp, train.adam_scalars(1))
    assert np.all((p2 != p)[1:])
    norm, mult = ref.norm_mult([np.array([3.0, 4.0], np.float32)], 0.0, 1.0)
    assert norm == 5.0 and mult == pytest.approx(0.2)
    assert ref.norm_mult([np.array([3.0, 4.0], np.float32)], 0.0, 10.0)[1] == 1.0


def test_bias_corrections_and_rounded_decays():
    sc = train.adam_scalars(0)
    assert sc["one_minus_b1"][0] == np.float32(0.1) and sc["one_minus_b2"][0] == np.float32(0.01)
    assert sc["bias_correction1"][0] == np.float32(1) - np.float32(0.9)
    late = train.adam_scalars(10000)
    assert late["bias_correction1"][0] == 1.0 and late["bias_correction2"][0] == 1.0
    assert len(sc["lr"]) == len(CFG.groups()) <= rc_ext.RC_ADAM_MAX_GROUPS


# ---- ABI ----------------------------------------------------------------------------------------------------------

def test_binding_lists_the_optimizer_entry_points():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rc_abi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("rc_adam_update", "rc_load_params_flat"):
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in rc_ext.EXPORTS
    assert re.search(r"#define RC_ADAM_MAX_GROUPS (\d+)", hdr).group(1) == str(rc_ext.RC_ADAM_MAX_GROUPS)
    assert re.search(r"#define RC_LAYOUT_SHADER \((-?\d+)\)", hdr).group(1) == str(rc_ext.RC_LAYOUT_SHADER)


def test_struct_layouts_match_c(tmp_path):
    import ctypes
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "rc_abi.h"\nint main(void) {\n'
            '  printf("%zu %zu %zu %zu %zu\\n", sizeof(rc_adam_buffer), sizeof(rc_adam_step), offsetof(rc_adam_step, grad_max_val),'
            ' offsetof(rc_adam_step, zero_grads), offsetof(rc_adam_buffer, seg_group));\n  return 0;\n}\n')
    (tmp_path / "t.c").write_text(prog)
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [ctypes.sizeof(rc_ext.rc_adam_buffer), ctypes.sizeof(rc_ext.rc_adam_step),
                   rc_ext.rc_adam_step.grad_max_val.offset, rc_ext.rc_adam_step.zero_grads.offset,
                   rc_ext.rc_adam_buffer.seg_group.offset]
