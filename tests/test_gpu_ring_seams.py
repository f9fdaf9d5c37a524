"""The weight ring of the fused cache kernel (rc_dev_mlp.h ws_issue_piece: which piece lands where, issued by which
wave) against the launch-per-stage plan, whose kernels pull other streams through rings of their own: bitwise, on every
output key.

A piece issued to the wrong slot, from the wrong offset or not at all shows as a wrong weight fragment in some layer of
some ray, so every instantiation of the kernel is run at ray counts that leave the only workgroup partly idle (n = 1, 3:
the idle waves are clamped to the last ray and keep issuing their quarter of every chunk), end in a partial workgroup
(5, 257) and fill several:
  * with the analytic normals (the GRAD instantiation: the backward fragments of level 2 are read),
  * without them (their fragments are stepped over, the seams inside them still retire and refill the ring),
  * with a subset of the outputs,
  * the FRONT instantiation (the stream ends in front of the shader) through render_transient, on one ray,
  * the EXPORT instantiation through render_material, on one ray,
  * the same batch launched on two streams, the two results compared with each other.
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
SUBSET = ("rgb", "distance_median")
_RC = []


def _rc():
    if not _RC:
        _RC.append(common.make_rc())
    return _RC[0]


def _plans(render, modes=(1, 3, 0)):
    rc, res = _rc(), {}
    for mode in modes:
        rc.set_fused(mode)
        try:
            out = render(rc)
            torch.cuda.synchronize()
        finally:
            rc.set_fused(True)
        res[mode] = {k: v.cpu().numpy() for k, v in out.items()}
    return res


@pytest.mark.parametrize("keys", [ALL, NO_NORMALS, SUBSET], ids=["normals", "no-normals", "subset"])
@pytest.mark.parametrize("n", SIZES)
def test_fused_plan_equals_the_launch_per_stage_plan_bitwise(n, keys):
    assert "normals" in ALL
    fields = nrc_amd.synthetic_rays(n, seed=8100 + n).hot_fields()
    rnd = {"jitter": common.jitters(n, seed=21 + n)}
    res = _plans(lambda rc: rc.render_rays(fields, rnd, outputs=list(keys)))
    assert set(res[0]) == set(keys)
    for k in keys:
        assert res[0][k].shape[0] == n and np.isfinite(res[0][k]).all(), k
        assert np.array_equal(res[3][k], res[0][k]), (k, "fused 3 vs launch-per-stage")
        assert np.array_equal(res[1][k], res[0][k]), (k, "fused 1 vs launch-per-stage")
    assert np.any(res[0]["rgb"])


def test_front_kernel_through_render_transient_on_one_ray():
    from nrc_amd import rc_ext
    rc = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    rc.load_weights(common.weights_transient_np())
    fields = nrc_amd.synthetic_transient_rays(1).hot_fields()
    rnd = {"jitter": common.jitters(1, seed=5)}
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


def test_export_kernel_through_render_material_on_one_ray():
    from nrc_amd import rc_ext
    from oracle import material_ref
    cfg = nrc_amd.hotdog_config()
    rc = rc_ext.RadianceCache(cfg, 0)
    rc.load_weights(common.weights_material_np(False))
    fields = nrc_amd.synthetic_rays(1, seed=5).hot_fields()
    rnd = material_ref.draw_randoms(cfg, 1, seed=8)
    res = {}
    for mode in (1, 3, 0):
        rc.set_fused(mode)
        cres, mres = rc.render_material(fields, rnd)
        torch.cuda.synchronize()
        res[mode] = {"c:" + k: v.cpu().numpy() for k, v in cres.items()}
        res[mode].update({"m:" + k: v.cpu().numpy() for k, v in mres.items()})
        res[mode]["inds"] = rc.workspace("inds", np.int32)[:1].copy()
    assert len(res[0]) > 2
    for mode in (1, 3):
        for k in res[0]:
            assert np.array_equal(res[mode][k], res[0][k]), (mode, k)


@pytest.mark.parametrize("n", SIZES)
def test_two_streams_render_the_same_batch_the_same(n):
    rc = _rc()
    rc.set_fused(3)                     # the one-wave kernel, whatever the batch size
    try:
        fields = {k: rc._dev(v) for k, v in nrc_amd.synthetic_rays(n, seed=8200 + n).hot_fields().items() if v is not None}
        got = []
        for s in (torch.cuda.Stream(), torch.cuda.Stream()):
            with torch.cuda.stream(s):
                got.append(rc.render_rays(fields, None, outputs=list(ALL)))
        torch.cuda.synchronize()
    finally:
        rc.set_fused(True)
    for k in ALL:
        assert torch.equal(got[0][k], got[1][k]), k
    assert float(got[0]["rgb"].abs().sum()) > 0.0
