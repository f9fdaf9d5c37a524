"""The fused kernel and the shader tile hand activations from layer to layer in registers (rc_dev_mlp.h BHand): the same
values, pieces and MFMAs in the same order, so every result is bitwise what the library rendered before.

  * tests/golden/handoff_pin.npz (tools/make_handoff_pin.py, run on the parent commit; its source hash is inside) holds
    the renders of tests/handoff_cases.py for BOTH arithmetics: every cache output of 33 jittered rays (eight full
    workgroups and one lane of a ninth), a 9-ray time-resolved render through the fused front end (FRONT instantiation)
    and a 9-ray material render on the fused plan (EXPORT instantiation).  The loaded library is held to the part of
    its own arithmetic, the other part is skipped; the fp32-MFMA build, which nothing else pins bitwise, renders in a
    fresh child process (RC_HIP_LIBRARY) as in tests/test_gpu_f32_build.py.  Outputs the pin keeps as a digest (the
    700-bin histograms) are compared by digest.
  * the GRAD = false instantiation (no `normals` asked for: the ring steps over the unused backward fragments) gives
    the pinned values of every other key on the same 33 rays;
  * 4 rays (exactly one full workgroup) and 6 (one full, one half empty) on plans 1, 3 and 0, bitwise: the neighbours
    1, 5 and 130 are in tests/test_gpu_shader_fill.py.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import common
import handoff_cases
import nrc_amd
from nrc_amd.model import _CACHE_DEVICE_KEYS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
CSRC = os.path.join(ROOT, "neural-radiance-caching_amd", "csrc")
PIN = os.path.join(TESTS, "golden", "handoff_pin.npz")
VARIANT = os.path.join(ROOT, "build", "f32", "librc_hip.so")
ARITHMETICS = ("bf16x3-split", "f32-mfma")


def _pin(arith):
    """{"<render>/<output>": array or digest string} of one arithmetic, and the parent's source hash"""
    g = dict(np.load(PIN))
    part = {k[len(arith) + 1:]: v for k, v in g.items() if k.startswith(arith + "/")}
    parent = str(part.pop("source_hash"))
    assert len(parent) == 16
    return part, parent


def _assert_equals_pin(got, part, parent, only=None):
    seen = 0
    for k, v in part.items():
        name = k[:-len("#sha256")] if k.endswith("#sha256") else k
        if only is not None and not only(name):
            continue
        seen += 1
        assert name in got, (name, "parent source " + parent)
        assert got[name].dtype == np.float32, name
        if k.endswith("#sha256"):
            assert hashlib.sha256(np.ascontiguousarray(got[name]).tobytes()).hexdigest() == str(v), (name, "parent source " + parent)
        else:
            assert v.dtype == np.float32 and got[name].shape == v.shape, (name, got[name].shape, v.shape)
            assert np.array_equal(got[name], v), (name, float(np.abs(got[name] - v).max()), "parent source " + parent)
    return seen


@pytest.fixture(scope="module")
def loaded_render():
    return handoff_cases.render_all()


def test_the_pin_holds_all_three_renders_for_both_arithmetics():
    for arith in ARITHMETICS:
        part, _ = _pin(arith)
        names = {k[:-len("#sha256")] if k.endswith("#sha256") else k for k in part}
        assert {"cache/" + k for k in _CACHE_DEVICE_KEYS} <= names, arith
        assert any(k.startswith("transient/") for k in names) and any(k.startswith("material/m:") for k in names), arith
        assert part["cache/rgb"].shape == (handoff_cases.N_CACHE, 3)
    assert os.path.getsize(PIN) < 100 * 1024


@pytest.mark.parametrize("arith", ARITHMETICS)
def test_loaded_library_renders_what_the_parent_rendered(loaded_render, arith):
    from nrc_amd import rc_ext
    if rc_ext.mlp_arithmetic() != arith:
        pytest.skip(f"this part of the pin holds {arith}; the loaded library runs {rc_ext.mlp_arithmetic()}")
    part, parent = _pin(arith)
    assert _assert_equals_pin(loaded_render, part, parent) == len(part)
    assert set(loaded_render) == {k[:-len("#sha256")] if k.endswith("#sha256") else k for k in part}


def test_fp32_build_renders_what_the_parent_rendered(tmp_path):
    r = subprocess.run(["make", "-C", CSRC, "-j16", "variant-f32"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    path = str(tmp_path / "f32.npz")
    env = {**os.environ, "RC_HIP_LIBRARY": VARIANT,
           "PYTHONPATH": os.pathsep.join([ROOT, TESTS, os.environ.get("PYTHONPATH", "")])}
    r = subprocess.run([sys.executable, os.path.join(TESTS, "handoff_cases.py"), path], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    got = dict(np.load(path))
    assert str(got.pop("mlp_arithmetic")) == "f32-mfma"
    got.pop("source_hash")
    part, parent = _pin("f32-mfma")
    assert _assert_equals_pin(got, part, parent) == len(part)


def test_kernel_without_the_backward_renders_the_pinned_values():
    from nrc_amd import rc_ext
    part, parent = _pin(rc_ext.mlp_arithmetic())
    keys = [k for k in _CACHE_DEVICE_KEYS if k != "normals"]
    rc = common.make_rc()
    rc.set_fused(True)
    out = rc.render_rays(handoff_cases.cache_rays().hot_fields(), handoff_cases.cache_randoms(), outputs=keys)
    torch.cuda.synchronize()
    got = {"cache/" + k: v.cpu().numpy() for k, v in out.items()}
    assert "cache/normals" not in got
    seen = _assert_equals_pin(got, part, parent, only=lambda name: name.startswith("cache/") and name != "cache/normals")
    assert seen == len(keys)


@pytest.mark.parametrize("normals", [True, False])
@pytest.mark.parametrize("n", [4, 6])
def test_plans_stay_bitwise_equal_at_whole_workgroups(n, normals):
    keys = [k for k in _CACHE_DEVICE_KEYS if normals or k != "normals"]
    rc = common.make_rc()
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
