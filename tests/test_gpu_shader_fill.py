"""The shader tile with the feature split once for its three readers and the bias blocks' zero products dropped.

Three properties:
  * the fused kernel, its rc_set_fused(3) twin and the launch-per-stage plan stay bitwise equal at ray counts that leave a
    workgroup partly empty (1, 5) and that end on a partial workgroup behind many full ones (130 = 32 x 4 + 2), with and
    without the analytic normals (the two GRAD instantiations of the fused kernel);
  * the split build's arithmetic is pinned: tests/golden/shader_pin_split_64.npz holds every output of 64 rays as the
    library BEFORE this change rendered them (its source hash is inside the file), and the outputs are array_equal to it;
  * the IDE is read by block 6 of the 85-step layer, the first block behind the six whose pieces come ready (the seam
    of the layer's operand pipeline), and feeds indirect_specular_rgb: that key and rgb against the oracle at the
    1e-4 of tests/test_gpu_parity.py, on rays whose view directions run from straight down (z < -0.9) to grazing
    (|z| < 0.5), so that the reflections about the samples' normals reach both ends of the IDE polynomials' range; the bound does not rest on the code under test: the oracle's
    own fp32-to-fp64 distance on these rays is checked to be below it.
"""
import os

import numpy as np
import pytest
import torch

import common
import nrc_amd
from nrc_amd.model import _CACHE_DEVICE_KEYS

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PIN = os.path.join(GOLD, "shader_pin_split_64.npz")
RGB_TOL = 1e-4          # tests/test_gpu_parity.py
N_PIN, SEED_PIN = 64, 20200823


@pytest.fixture(scope="module")
def rc():
    return common.make_rc()


@pytest.fixture(scope="module")
def pin_render(rc):
    """The 64 pin rays through the fused plan, every output key; shared by the pin and the oracle test."""
    rays = nrc_amd.synthetic_rays(N_PIN, seed=SEED_PIN)
    rc.set_fused(True)
    out = rc.render_rays(rays.hot_fields(), None)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("normals", [True, False])
@pytest.mark.parametrize("n", [1, 5, 130])
def test_plans_stay_bitwise_equal(rc, n, normals):
    keys = [k for k in _CACHE_DEVICE_KEYS if normals or k != "normals"]
    assert ("normals" in keys) == normals
    rays = nrc_amd.synthetic_rays(n, seed=4100 + n)
    res = {}
    for mode in (1, 3, 0):
        rc.set_fused(mode)
        try:
            out = rc.render_rays(rays.hot_fields(), None, outputs=keys)
            torch.cuda.synchronize()
        finally:
            rc.set_fused(True)
        res[mode] = {k: v.cpu().numpy() for k, v in out.items()}
    for k in keys:
        assert res[1][k].shape[0] == n and np.isfinite(res[1][k]).all(), k
        assert np.array_equal(res[1][k], res[3][k]), (k, "fused 1 vs fused 3")
        assert np.array_equal(res[1][k], res[0][k]), (k, "fused vs launch-per-stage")


def test_split_arithmetic_is_pinned_to_the_parent(pin_render):
    from nrc_amd import rc_ext
    if rc_ext.mlp_arithmetic() != "bf16x3-split":
        pytest.skip(f"the pin holds the split build's arithmetic; this library runs {rc_ext.mlp_arithmetic()}")
    g = dict(np.load(PIN))
    assert str(g.pop("mlp_arithmetic")) == "bf16x3-split"
    parent = str(g.pop("source_hash"))
    assert len(parent) == 16
    assert set(_CACHE_DEVICE_KEYS) <= set(g), sorted(set(_CACHE_DEVICE_KEYS) - set(g))
    for k, v in g.items():
        assert v.dtype == np.float32 and pin_render[k].dtype == np.float32, k
        assert np.array_equal(pin_render[k], v), (k, float(np.abs(pin_render[k] - v).max()), "parent source " + parent)


def test_ide_blocks_behind_the_ready_feature_vs_oracle(pin_render):
    rays = nrc_amd.synthetic_rays(N_PIN, seed=SEED_PIN)
    vz = np.asarray(rays.hot_fields()["viewdirs"])[:, 2]
    assert vz.min() < -0.9 and (np.abs(vz) < 0.5).any(), (vz.min(), vz.max())      # the shell is the upper one: v points down
    r32 = common.oracle_cache(N_PIN, seed=SEED_PIN, want_grad_normals=False)["render"]
    r64 = common.oracle_cache(N_PIN, seed=SEED_PIN, want_grad_normals=False, dtype=torch.float64)["render"]
    for k in ("rgb", "indirect_specular_rgb"):
        floor = float(np.abs(r32[k].numpy().astype(np.float64) - r64[k].numpy()).max())
        err = float(np.abs(pin_render[k] - r32[k].numpy()).max())
        print(f"{k}: max|hip - oracle fp32| = {err:.3e}, oracle fp32 vs fp64 = {floor:.3e}")
        assert floor < RGB_TOL, (k, floor)
        assert err <= RGB_TOL, (k, err)
