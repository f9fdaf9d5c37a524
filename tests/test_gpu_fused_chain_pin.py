"""The one-wave fused kernel fetches the output pointers of its compositing tail (and the workspace pointers of its FRONT
and EXPORT forms) as one batch of scalar loads, stores the EXPORT results behind the shader, and writes the appearance
features straight to the shader's LDS steps.  That changes when a pointer is read and where a value waits, never a value:

  * tests/golden/chain_pin.npz (tools/make_chain_pin.py, run on the parent commit; its source hash is inside) holds the
    renders of tests/chain_cases.py for BOTH arithmetics: rc_set_fused(3) on 1, 5 and 260 rays with every cache output,
    without `normals` (GRAD = false), `rgb` alone and the three distance percentiles alone (null pointers in the batched
    tail), with and without lights and jitter, 260 rays that leave the bounding box and the contraction radius, two
    render_transient front ends (FRONT) and one render_material pass (EXPORT).  The loaded library is held to the part of
    its own arithmetic with np.array_equal; the fp32-MFMA build renders in a fresh child process (RC_HIP_LIBRARY) as in
    tests/test_gpu_f32_build.py.
  * the same cases on the launch-per-stage plan (rc_set_fused(0)) equal the fused renders array for array.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_cases
import nrc_amd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
CSRC = os.path.join(ROOT, "neural-radiance-caching_amd", "csrc")
PIN = os.path.join(TESTS, "golden", "chain_pin.npz")
VARIANT = os.path.join(ROOT, "build", "f32", "librc_hip.so")
ARITHMETICS = ("bf16x3-split", "f32-mfma")


def _pin(arith):
    g = dict(np.load(PIN))
    part = {k[len(arith) + 1:]: v for k, v in g.items() if k.startswith(arith + "/")}
    parent = str(part.pop("source_hash"))
    assert len(parent) == 16
    return part, parent


def _assert_equal(got, want, what):
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    for k, v in want.items():
        assert v.dtype == np.float32 and got[k].dtype == np.float32 and got[k].shape == v.shape, (k, got[k].shape, v.shape)
        assert np.array_equal(got[k], v), (k, float(np.abs(got[k] - v).max()), what)


@pytest.fixture(scope="module")
def fused():
    return chain_cases.render_all(chain_cases.FUSED)


def test_the_pin_holds_every_case_for_both_arithmetics():
    from nrc_amd.model import _CACHE_DEVICE_KEYS
    names = {c[0]: c[3] for c in chain_cases.plain_cases()}
    assert {"all/n1", "nonorm/n5", "rgb/n260", "pct/n1", "all_nolights", "all_nojit", "pct_nolights_nojit", "wide/n260"} <= set(names)
    want = {f"{name}/{k}" for name, keys in names.items() for k in keys}
    for arith in ARITHMETICS:
        part, _ = _pin(arith)
        plain = {k for k in part if not k.startswith(("front/", "export/"))}
        assert plain == want, (arith, sorted(plain ^ want))
        assert part["all/n1/rgb"].shape == (1, 3) and part["all/n260/normals"].shape == (260, 3) and part["pct/n5/distance_median"].shape == (5,)
        assert set(k.rsplit("/", 1)[1] for k in part if k.startswith("all/n5/")) == set(_CACHE_DEVICE_KEYS)
        assert any(k.startswith("front/n5/") for k in part) and any(k.startswith("front/n9/") for k in part)
        assert any(k.startswith("export/n5/c:") for k in part) and any(k.startswith("export/n5/m:") for k in part)
        assert all(np.isfinite(v).all() for v in part.values())
    assert os.path.getsize(PIN) < 1024 * 1024


def test_the_wide_rays_leave_the_box_and_the_contraction_radius():
    cfg = nrc_amd.hotdog_config()
    r = chain_cases.wide_rays(260)
    t = np.linspace(r["near"].reshape(-1, 1), r["far"].reshape(-1, 1), 64, axis=-1).reshape(260, 64, 1)
    p = r["origins"][:, None, :] + t * r["directions"][:, None, :]
    rad = np.linalg.norm(p, axis=-1)
    beyond = rad > cfg.contract_radius
    z = p / cfg.contract_radius
    m = np.maximum(1.0, (z * z).sum(-1, keepdims=True))
    c = z * (2.0 * np.sqrt(m) - 1.0) / m
    outside = (np.abs(c) >= 1.0).any(-1)          # bounding box of the hotdog grids: [-1, 1]^3 of the contracted position
    print("beyond the contraction radius", beyond.mean(), "outside the box", outside.mean())
    assert 0.25 <= beyond.mean() <= 0.99 and 0.25 <= outside.mean() <= 0.99
    assert (~outside).mean() >= 0.01              # ... and some samples inside, on every kind of level


def test_loaded_library_renders_what_the_parent_rendered(fused):
    from nrc_amd import rc_ext
    part, parent = _pin(rc_ext.mlp_arithmetic())
    _assert_equal(fused, part, "parent source " + parent)


def test_fused_and_launch_per_stage_plans_agree(fused):
    staged = chain_cases.render_all(chain_cases.STAGED)
    _assert_equal(staged, fused, "launch-per-stage against fused")


def test_fp32_build_renders_what_the_parent_rendered(tmp_path):
    r = subprocess.run(["make", "-C", CSRC, "-j16", "variant-f32"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    path = str(tmp_path / "f32.npz")
    env = {**os.environ, "RC_HIP_LIBRARY": VARIANT,
           "PYTHONPATH": os.pathsep.join([ROOT, TESTS, os.environ.get("PYTHONPATH", "")])}
    r = subprocess.run([sys.executable, os.path.join(TESTS, "chain_cases.py"), path], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    got = dict(np.load(path))
    assert str(got.pop("mlp_arithmetic")) == "f32-mfma"
    got.pop("source_hash")
    part, parent = _pin("f32-mfma")
    _assert_equal(got, part, "parent source " + parent)
