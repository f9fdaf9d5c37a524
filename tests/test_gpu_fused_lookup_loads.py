"""The one-wave fused kernel with the kinds of its grid levels fixed at compile time (rc_fused.hip: level l is dense iff
l < kFusedDense, so that the table loads of a lookup go out in one batch): rc_render_rays on the fused plans (rc_set_fused 1
and 3) against the launch-per-stage plan (0), bitwise, over the kernel's optional inputs and the outputs its tail selects
per lane.

n = 1 and 3 leave idle waves of the only workgroup clamped to the last ray, 4 is one whole workgroup, 5 and 257 end in a
partial one.  For every n and for the default and a non-default percentile triple (10 / 50 / 90), every combination of
  * lights given (not the ray origins: light_dists must differ from ray_dists) | absent,
  * jitter given | absent,
  * all of _CACHE_DEVICE_KEYS | only one of the three percentile keys | only light_dists
is rendered on the three plans.
"""
import dataclasses
import itertools

import numpy as np
import pytest
import torch

import common
import nrc_amd
from nrc_amd.model import _CACHE_DEVICE_KEYS

pytestmark = pytest.mark.gpu

PERCENTILE_KEYS = ("distance_percentile_5", "distance_median", "distance_percentile_95")
OUTPUT_SETS = (tuple(_CACHE_DEVICE_KEYS),) + tuple((k,) for k in PERCENTILE_KEYS) + (("light_dists",),)
PERCENTILES = ((5.0, 50.0, 95.0), (10.0, 50.0, 90.0))
_RC = {}


def _rc(pct):
    if pct not in _RC:
        _RC[pct] = common.make_rc(cfg=dataclasses.replace(nrc_amd.hotdog_config(), percentiles=pct))
    return _RC[pct]


def _fields(n, lights):
    f = {k: np.asarray(v) for k, v in nrc_amd.synthetic_rays(n, seed=7100 + n).hot_fields().items()}
    rng = np.random.Generator(np.random.PCG64(n))
    f["lights"] = (f["origins"] + rng.normal(scale=0.3, size=f["origins"].shape)).astype(np.float32) if lights else None
    return f


def _render(rc, fields, randoms, keys):
    res = {}
    for mode in (1, 3, 0):
        rc.set_fused(mode)
        try:
            out = rc.render_rays(fields, randoms, outputs=list(keys))
            torch.cuda.synchronize()
        finally:
            rc.set_fused(True)
        res[mode] = {k: v.cpu().numpy() for k, v in out.items()}
    return res


def test_the_output_sets_cover_what_the_tail_selects():
    assert set(PERCENTILE_KEYS) | {"light_dists"} <= set(_CACHE_DEVICE_KEYS)
    assert len(OUTPUT_SETS) == 5


@pytest.mark.parametrize("pct", PERCENTILES, ids=lambda p: "pct" + "-".join(str(int(v)) for v in p))
@pytest.mark.parametrize("n", [1, 3, 4, 5, 257])
def test_fused_plans_equal_the_launch_per_stage_plan_bitwise(n, pct):
    rc = _rc(pct)
    full = {}
    for lights, jitter, keys in itertools.product((True, False), (True, False), OUTPUT_SETS):
        tag = (lights, jitter, keys if len(keys) == 1 else "all")
        res = _render(rc, _fields(n, lights), {"jitter": common.jitters(n, seed=11 + n)} if jitter else None, keys)
        for k in keys:
            assert res[0][k].shape[0] == n and np.isfinite(res[0][k]).all(), (tag, k)
            assert np.array_equal(res[3][k], res[0][k]), (tag, k, "fused 3 vs launch-per-stage")
            assert np.array_equal(res[1][k], res[0][k]), (tag, k, "fused 1 vs launch-per-stage")
        if len(keys) > 1:
            full[(lights, jitter)] = res[3]
        else:
            # a subset leaves the requested key what it is among all keys
            assert np.array_equal(res[3][keys[0]], full[(lights, jitter)][keys[0]]), (tag, "subset vs all keys")
    # the inputs are really read: lights move light_dists only, jitter moves the samples
    assert not np.array_equal(full[(True, True)]["light_dists"], full[(False, True)]["light_dists"])
    assert not np.any(full[(False, True)]["light_dists"])
    assert np.array_equal(full[(True, True)]["rgb"], full[(False, True)]["rgb"])
    assert not np.array_equal(full[(True, True)]["rgb"], full[(True, False)]["rgb"])
    assert not np.allclose(full[(True, True)]["light_dists"], full[(True, True)]["ray_dists"])


def test_the_percentile_triple_reaches_the_kernel():
    d = {p: _render(_rc(p), _fields(5, True), None, PERCENTILE_KEYS)[3] for p in PERCENTILES}
    a, b = d[PERCENTILES[0]], d[PERCENTILES[1]]
    assert np.array_equal(a["distance_median"], b["distance_median"])
    assert np.all(a["distance_percentile_5"] <= b["distance_percentile_5"]) and not np.array_equal(a["distance_percentile_5"], b["distance_percentile_5"])
    assert np.all(a["distance_percentile_95"] >= b["distance_percentile_95"]) and not np.array_equal(a["distance_percentile_95"], b["distance_percentile_95"])
