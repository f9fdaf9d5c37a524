"""The one-wave fused kernel reads the scalars of each phase from a per-phase argument record (RcLookupRec, RcResampleRec,
RcShadeRec of rc_fused_common.h), fetched as one batch of scalar loads one phase ahead of use.  That moves where an
argument lives and when it is read, never a value:

  * every case of tests/scalar_batch_cases.py -- 1, 3, 4, 5 and 257 rays; with `normals` (GRAD) or without; jitter on all
    three levels or none; `lights` given or null; the percentile triple (10, 40, 90) -- renders the same arrays on the fused
    plan (rc_set_fused(3)) as on the launch-per-stage plan (rc_set_fused(0)), np.array_equal on every output key, and so do
    the transient front end (FRONT) and the material stage's export (EXPORT) at 5 and 257 rays;
  * the same comparison on the fp32-MFMA build, rendered in a fresh child process (RC_HIP_LIBRARY) as in
    tests/test_gpu_f32_build.py;
  * tests/golden/scalar_batch_pin.npz (tools/make_scalar_batch_pin.py, run on the parent commit; its source hash is inside)
    holds `all/n257` of both arithmetics as the parent rendered it; both builds are held to it with np.array_equal.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import scalar_batch_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
CSRC = os.path.join(ROOT, "neural-radiance-caching_amd", "csrc")
PIN = os.path.join(TESTS, "golden", "scalar_batch_pin.npz")
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
def fused_plain():
    return cases.render_plain(cases.FUSED)


@pytest.fixture(scope="module")
def f32_child(tmp_path_factory):
    """{"f:<key>": fused, "s:<key>": staged} of every case on the fp32-MFMA build"""
    r = subprocess.run(["make", "-C", CSRC, "-j16", "variant-f32"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    path = str(tmp_path_factory.mktemp("scalar_batches") / "f32.npz")
    env = {**os.environ, "RC_HIP_LIBRARY": VARIANT,
           "PYTHONPATH": os.pathsep.join([ROOT, TESTS, os.environ.get("PYTHONPATH", "")])}
    r = subprocess.run([sys.executable, os.path.join(TESTS, "scalar_batch_cases.py"), path, "compare"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    got = dict(np.load(path))
    assert str(got.pop("mlp_arithmetic")) == "f32-mfma"
    got.pop("source_hash")
    return got


def test_the_cases_cover_every_moved_scalar():
    from nrc_amd.model import _CACHE_DEVICE_KEYS
    names = {c[0]: c for c in cases.plain_cases()}
    assert set(names) == {f"{s}/n{n}" for n in (1, 3, 4, 5, 257) for s in ("all", "nonorm_nojit", "nolights", "pct")}
    for n in cases.SIZES:
        assert "normals" in names[f"all/n{n}"][4] and "normals" not in names[f"nonorm_nojit/n{n}"][4]
        assert len(names[f"all/n{n}"][3]["jitter"]) == 3 and names[f"nonorm_nojit/n{n}"][3] is None
        assert "lights" in names[f"all/n{n}"][2] and "lights" not in names[f"nolights/n{n}"][2]
        assert names[f"pct/n{n}"][1] == "pct" and set(names[f"all/n{n}"][4]) == set(_CACHE_DEVICE_KEYS)
    for arith in ARITHMETICS:
        part, _ = _pin(arith)
        assert set(part) == {f"all/n257/{k}" for k in _CACHE_DEVICE_KEYS}, arith
        assert part["all/n257/rgb"].shape == (257, 3) and all(np.isfinite(v).all() for v in part.values())
    assert os.path.getsize(PIN) < 1024 * 1024


def test_fused_and_launch_per_stage_plans_agree(fused_plain):
    staged = cases.render_plain(cases.STAGED)
    _assert_equal(fused_plain, staged, "fused against launch-per-stage")
    # the non-default percentiles reach the kernel: the three distances differ from the default handle's
    assert not np.array_equal(fused_plain["pct/n257/distance_percentile_5"], fused_plain["all/n257/distance_percentile_5"])
    assert not np.array_equal(fused_plain["nolights/n257/rgb"], np.zeros_like(fused_plain["nolights/n257/rgb"]))


def test_front_and_export_agree_with_their_launch_per_stage_counterparts():
    fused, staged = cases.render_forms(cases.FUSED), cases.render_forms(cases.STAGED)
    assert any(k.startswith("front/n257/") for k in fused) and any(k.startswith("export/n257/m:") for k in fused)
    _assert_equal(fused, staged, "FRONT / EXPORT against launch-per-stage")


def test_loaded_library_renders_what_the_parent_rendered(fused_plain):
    from nrc_amd import rc_ext
    part, parent = _pin(rc_ext.mlp_arithmetic())
    _assert_equal({k: v for k, v in fused_plain.items() if k.startswith("all/n257/")}, part, "parent source " + parent)


def test_fp32_build_fused_and_launch_per_stage_plans_agree(f32_child):
    fused = {k[2:]: v for k, v in f32_child.items() if k.startswith("f:")}
    staged = {k[2:]: v for k, v in f32_child.items() if k.startswith("s:")}
    assert any(k.startswith("pct/n1/") for k in fused) and any(k.startswith("front/n5/") for k in fused)
    assert any(k.startswith("export/n257/") for k in fused)
    _assert_equal(fused, staged, "fp32 build: fused against launch-per-stage")


def test_fp32_build_renders_what_the_parent_rendered(f32_child):
    part, parent = _pin("f32-mfma")
    _assert_equal({k[2:]: v for k, v in f32_child.items() if k.startswith("f:all/n257/")}, part, "parent source " + parent)
