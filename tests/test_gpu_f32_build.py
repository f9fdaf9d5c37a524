"""The fp32-MFMA build (RC_SPLIT_MFMA=0: the exact fp32 MFMA chain in every layer, the reference's own arithmetic and
the fallback of the split form) under the GPU suite.

`make variant-f32` builds it into build/f32/librc_hip.so with objects of its own.  It is only ever loaded by fresh child
processes (RC_HIP_LIBRARY), never by this one, which has the product library loaded: the child runs the GPU parity
modules against it -- there rc_set_fused(1) is the two-wave kernel k_cache_fused_team, so
test_two_wave_fused_kernel_equals_the_one_wave_kernel compares two kernels -- and a second child renders the
256-ray cache pass and the 128-ray material stage into a temporary .npz that this process holds, next to its own
renders, to the fp64 oracle.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import common
import nrc_amd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-radiance-caching_amd", "csrc")
VARIANT = os.path.join(ROOT, "build", "f32", "librc_hip.so")
CHILD_MODULES = ("tests/test_gpu_parity.py", "tests/test_gpu_abi_robustness.py", "tests/test_gpu_large_plan.py",
                 "tests/test_gpu_boundary.py", "tests/test_gpu_mlp_floor.py", "tests/test_gpu_render_settings.py")
MIN_PASSED = 154     # 108 + the 46 tests of test_gpu_render_settings.py; 162 GPU tests in the child's modules
K = 3.0
_SUITE = {}          # how the suite child ended: a fault there starts no further child on that library

# the child that renders for the cross-build check on one library: the 256-ray cache pass of test_gpu_parity.py, and
# the 128-ray material stage on the smooth weights with the fp32 oracle's picks handed over (test_gpu_parity.py
# _material_with_picks), the picks read from the parent's .npz
RENDER = r"""
import sys
import numpy as np, torch
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import common, nrc_amd
from nrc_amd import rc_ext
from oracle import material_ref
rc = common.make_rc()
rays = nrc_amd.synthetic_rays(256, seed=20200823)
out = {{"cache:" + k: v.cpu().numpy() for k, v in rc.render_rays(rays.hot_fields(), {{"jitter": common.jitters(256, seed=7)}}).items()}}
cfg = nrc_amd.hotdog_config()
picks = dict(np.load({picks!r}))
rm = rc_ext.RadianceCache(cfg, 0)
rm.load_weights(common.weights_material_np(True))
rnd = material_ref.draw_randoms(cfg, 128, seed=3)
rnd = dict(rnd, gumbel=None, spec_gumbel=None, diff_gumbel=None, **{{k: v.astype(np.int32) for k, v in picks.items()}})
_, mres = rm.render_material(nrc_amd.synthetic_rays(128, seed=77).hot_fields(), rnd)
torch.cuda.synchronize()
out.update({{"material:" + k: v.cpu().numpy() for k, v in mres.items()}})
np.savez({path!r}, arithmetic=rc_ext.mlp_arithmetic(), **out)
"""
MAT_KEYS = ("rgb", "direct_rgb", "indirect_rgb", "diffuse_rgb", "specular_rgb", "material_albedo", "material_roughness",
            "lighting_irradiance", "acc")


@pytest.fixture(scope="module")
def variant():
    r = subprocess.run(["make", "-C", CSRC, "-j16", "variant-f32"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert os.path.exists(VARIANT)
    return VARIANT


def _child_env(lib):
    return {**os.environ, "RC_HIP_LIBRARY": lib}


def test_gpu_suite_passes_on_the_fp32_build(variant):
    _SUITE["status"] = "timeout"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", *CHILD_MODULES],
                       cwd=ROOT, env=_child_env(variant), capture_output=True, text=True, timeout=1200)
    _SUITE["status"] = r.returncode
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    summary = [l for l in r.stdout.splitlines() if " passed" in l or " failed" in l or " error" in l]
    passed = 0
    if summary:
        for tok, nxt in zip(summary[-1].split(), summary[-1].split()[1:]):
            if nxt.startswith("passed"):
                passed = int(tok)
    assert r.returncode == 0 and passed >= MIN_PASSED, (f"fp32 build: exit {r.returncode}, {passed} passed "
                                                        f"(minimum {MIN_PASSED})", tail)
    print(f"fp32 build: {summary[-1] if summary else ''}")


def _oracle_material(dtype, picks):
    from oracle import material_ref
    cfg = nrc_amd.hotdog_config()
    rnd = material_ref.draw_randoms(cfg, 128, seed=3)
    if picks is not None:
        rnd = dict(rnd, **picks)
    return material_ref.material_forward(common.to_torch(common.weights_material_np(True), dtype), cfg,
                                         common.rays_torch(nrc_amd.synthetic_rays(128, seed=77), dtype), rnd)


def test_both_builds_sit_at_the_fp32_floor(variant, tmp_path):
    """The 256-ray cache pass and the 128-ray material stage (smooth weights, the fp32 oracle's picks handed over) of
    the fp32 build (child, .npz) and of the split build (this process) against the fp64 oracle: neither more than K x
    the fp32 oracle's distance from it.  Not started when the suite child above ended on a signal or its time limit.
    Measured HIP / floor, equal in the two builds to two digits: cache pass 0.58-1.15, material stage 1.02-1.29
    (lighting_irradiance 2.48-2.49)."""
    from nrc_amd import rc_ext
    st = _SUITE.get("status", 0)
    assert st == "timeout" or st >= 0, f"the suite child on the fp32 build ended on signal {-st}: nothing more is run on it"
    assert st != "timeout", "the suite child on the fp32 build hit its time limit: nothing more is run on it"
    ref = _oracle_material(torch.float32, None)
    picks = {"resample_inds": ref["inds"][:, 0].numpy().astype(np.int32),
             "spec_resample_inds": ref["debug"]["specular"]["inds"].numpy().astype(np.int32),
             "diff_resample_inds": ref["debug"]["diffuse"]["inds"].numpy().astype(np.int32)}
    ppath, path = str(tmp_path / "picks.npz"), str(tmp_path / "f32.npz")
    np.savez(ppath, **picks)
    src = RENDER.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path, picks=ppath)
    r = subprocess.run([sys.executable, "-c", src], cwd=ROOT, env=_child_env(variant), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    f32 = dict(np.load(path))
    assert str(f32.pop("arithmetic")) == "f32-mfma"
    assert rc_ext.mlp_arithmetic() == "bf16x3-split"
    # the same two renders on the product library, in this process
    rc = common.make_rc()
    rays = nrc_amd.synthetic_rays(256, seed=20200823)
    split = {"cache:" + k: v.cpu().numpy() for k, v in rc.render_rays(rays.hot_fields(), {"jitter": common.jitters(256, seed=7)}).items()}
    from oracle import material_ref
    cfg = nrc_amd.hotdog_config()
    rm = rc_ext.RadianceCache(cfg, 0)
    rm.load_weights(common.weights_material_np(True))
    rnd = dict(material_ref.draw_randoms(cfg, 128, seed=3), gumbel=None, spec_gumbel=None, diff_gumbel=None, **picks)
    _, mres = rm.render_material(nrc_amd.synthetic_rays(128, seed=77).hot_fields(), rnd)
    torch.cuda.synchronize()
    split.update({"material:" + k: v.cpu().numpy() for k, v in mres.items()})
    # the floors: fp32 and fp64 oracles, the material stage on the same picks
    c32 = common.oracle_cache(256, jitter_seed=7, want_grad_normals=False)["render"]
    c64 = common.oracle_cache(256, jitter_seed=7, want_grad_normals=False, dtype=torch.float64)["render"]
    m32 = _oracle_material(torch.float32, picks)["render"]
    m64 = _oracle_material(torch.float64, picks)["render"]
    pairs = [("cache:" + k, c32[k], c64[k]) for k in ("rgb", "acc", "diffuse_rgb", "specular_rgb", "indirect_rgb",
                                                      "albedo_rgb", "means", "normals_pred", "distance_median")]
    pairs += [("material:" + k, m32[k], m64[k]) for k in MAT_KEYS]
    ratios, bad = {}, []
    for k, b32, b64 in pairs:
        b32, b64 = b32.numpy().astype(np.float64), b64.numpy()
        floor = np.abs(b32 - b64).max()
        for name, res in (("f32-mfma", f32), ("bf16x3-split", split)):
            err = np.abs(res[k].astype(np.float64).reshape(b64.shape) - b64).max()
            ratios[f"{name} {k}"] = round(float(err / floor), 2)
            if not err <= K * floor + 1e-7:
                bad.append((name, k, err, floor))
    print("HIP / floor:", ratios)
    assert not bad, (bad, ratios)
