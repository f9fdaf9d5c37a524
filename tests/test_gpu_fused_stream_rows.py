"""The fused kernels on their own weight streams (rc_api.hip build_fused_stream: output rows as tables in the split
build, rc_pack_host.h pack_dot_rows, read by rc_dev_mlp.h dot_rows) against the launch-per-stage plan, bitwise on every
output key.  The staged plan's kernels keep the fragment-form streams (pack_dot, dot_out), so it is an independent
reference: a table packed or read at a wrong offset, a wrong half-wave row or a bias out of place shows in the density,
the predicted or the analytic normals (level 2's table, whose first row is also the backward pass's output weight), the
integrated BRDF or the ambient colour of some ray.

Sizes: n = 1 and 3 leave the only workgroup partly idle (the idle waves are clamped to the last ray), 5 adds a second
workgroup, 257 more than one round per XCD.  With and without the analytic normals (the GRAD instantiation reads the
backward fragments behind level 2's table, the other one steps over them), with a subset of the outputs (null
pointers), and one case each through the FRONT path (the transient front end) and the EXPORT path (the material stage)
at 8 rays.  On the fp32-MFMA build the streams keep the fragment form and the same tests pass unchanged.
"""
import numpy as np
import pytest
import torch

import common
import nrc_amd
from nrc_amd.model import _CACHE_DEVICE_KEYS

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 5, 257]
ALL = tuple(_CACHE_DEVICE_KEYS)
NO_NORMALS = tuple(k for k in ALL if k != "normals")
SUBSET = ("rgb", "acc", "normals_pred")
_RC = []


def _rc():
    if not _RC:
        _RC.append(common.make_rc())
    return _RC[0]


@pytest.mark.parametrize("keys", [ALL, NO_NORMALS, SUBSET], ids=["normals", "no-normals", "subset"])
@pytest.mark.parametrize("n", SIZES)
def test_fused_plans_equal_the_launch_per_stage_plan(n, keys):
    assert "normals" in ALL
    rc = _rc()
    fields = nrc_amd.synthetic_rays(n, seed=9300 + n).hot_fields()
    rnd = {"jitter": common.jitters(n, seed=41 + n)}
    res = {}
    for mode in (1, 3, 0):
        rc.set_fused(mode)
        try:
            out = rc.render_rays(fields, rnd, outputs=list(keys))
            torch.cuda.synchronize()
        finally:
            rc.set_fused(True)
        res[mode] = {k: v.cpu().numpy() for k, v in out.items()}
    assert set(res[0]) == set(keys)
    for k in keys:
        assert res[0][k].shape[0] == n and np.isfinite(res[0][k]).all(), k
        assert np.array_equal(res[3][k], res[0][k]), (k, "rc_set_fused 3 vs launch-per-stage")
        assert np.array_equal(res[1][k], res[0][k]), (k, "rc_set_fused 1 vs launch-per-stage")
    assert np.any(res[0]["rgb"])


def test_front_path_equals_the_staged_transient_front_end():
    from nrc_amd import rc_ext
    rc = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    rc.load_weights(common.weights_transient_np())
    fields = nrc_amd.synthetic_transient_rays(8).hot_fields()
    rnd = {"jitter": common.jitters(8, seed=6)}
    res = {}
    for mode in (1, 0):
        rc.set_fused(mode)
        out = rc.render_transient(fields, rnd)
        torch.cuda.synchronize()
        res[mode] = {k: v.cpu().numpy() for k, v in out.items()}
    assert res[0] and set(res[0]) == set(res[1])
    for k in res[0]:
        assert np.isfinite(res[0][k]).all(), k
        assert np.array_equal(res[1][k], res[0][k]), k
    assert any(np.any(v) for v in res[0].values())


def test_export_path_equals_the_staged_material_stage():
    from nrc_amd import rc_ext
    from oracle import material_ref
    cfg = nrc_amd.hotdog_config()
    rc = rc_ext.RadianceCache(cfg, 0)
    rc.load_weights(common.weights_material_np(False))
    fields = nrc_amd.synthetic_rays(8, seed=6).hot_fields()
    rnd = material_ref.draw_randoms(cfg, 8, seed=9)
    res = {}
    for mode in (1, 3, 0):
        rc.set_fused(mode)
        cres, mres = rc.render_material(fields, rnd)
        torch.cuda.synchronize()
        res[mode] = {"c:" + k: v.cpu().numpy() for k, v in cres.items()}
        res[mode].update({"m:" + k: v.cpu().numpy() for k, v in mres.items()})
        res[mode]["inds"] = rc.workspace("inds", np.int32)[:8].copy()
    assert len(res[0]) > 2
    for mode in (1, 3):
        for k in res[0]:
            assert np.array_equal(res[mode][k], res[0][k]), (mode, k)
