"""Oracle contact for the launch plans the LARGE batches run.

From 24 576 rays on, the launch-per-stage plan runs a proposal level with its sampling in front as ONE launch
(k_level_ray, csrc/rc_level.hip; the switch is in rc_render_host.inc stage_levels) -- the plan the material stage's 32 768-ray
secondary trace and its bench line run.  The other GPU tests reach that plan only transitively (bitwise equal to the
separate kernels, which equal the oracle at n <= 512).  Here the oracle itself is run on a strided subset of a batch
large enough to take that plan (rays are independent: the oracle of a subset with the subset's random inputs is the
subset of the oracle), with the oracle's categorical picks handed over, on the smooth field, at the north-star 1e-4:

  * secondary rays (is_secondary=True) and forced resampling of primary rays at n = 25 001;
  * rc_render_material at 1024 primary rays (BASELINE configs[2] at the bench's own size): a 64-ray subset of the
    primaries with their 2 048 secondary rays;
  * the 128-ray material test on a SECOND smooth weight set (another seed for weights, rays and random inputs).

Reference: internal/sampling.py:284-639 under internal/material.py:1684-1864, 2191-2217; internal/models.py:193-292.
"""
import numpy as np
import pytest
import torch

import common
import nrc_amd
from test_gpu_parity import MAT_ALL_KEYS, RGB_TOL, _material_with_picks

pytestmark = pytest.mark.gpu
N_BIG = 25001          # >= 24 576: k_level_ray


@pytest.fixture(scope="module")
def rc_smooth():
    from nrc_amd import rc_ext
    h = rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)
    h.load_weights(common.weights_material_np(smooth=True))
    return h


def _take(d, idx):
    return {k: np.ascontiguousarray(np.asarray(v)[idx]) for k, v in d.items()}


def test_secondary_rays_25001_vs_oracle_on_a_subset(rc_smooth):
    from nrc_amd import rc_ext
    from oracle import cache_ref
    rays, rnd = common.secondary_case(N_BIG, seed=31)
    idx = np.arange(0, N_BIG, 25)                                   # 1001 rays
    sub = _take(rays, idx)
    jit = [torch.from_numpy(j[idx])[:, None] for j in rnd["jitter"]]
    ref = cache_ref.cache_forward(common.to_torch(common.weights_material_np(True)), nrc_amd.hotdog_config(),
                                  common.rays_dict_torch(sub), jit, is_secondary=True,
                                  gumbel=torch.from_numpy(rnd["gumbel"][idx]), want_grad_normals=False)
    picks = np.zeros(N_BIG, np.int32)
    picks[idx] = ref["filtered_sampler_inds"][:, 0].numpy()
    mask = rc_ext.RC_PASS_CACHE | rc_ext.RC_PASS_SECONDARY
    # the Gumbel draw on the device first: nearly all picks of the subset equal
    rc_smooth.render_rays(rays, rnd, mask, outputs=["rgb"])
    torch.cuda.synchronize()
    assert (rc_smooth.workspace("inds", np.int32)[:N_BIG][idx] == picks[idx]).mean() >= 0.99
    out = rc_smooth.render_rays(rays, dict(jitter=rnd["jitter"], resample_inds=picks), mask)
    torch.cuda.synchronize()
    assert np.array_equal(rc_smooth.workspace("inds", np.int32)[:N_BIG], picks)
    r = ref["render"]
    for l in range(3):
        td = rc_smooth.workspace(f"tdist{l}").reshape(N_BIG, -1)[idx]
        assert np.abs(td - ref["sampler"][l]["tdist"].numpy()).max() <= 2e-4, l
    for k in ("rgb", "acc", "diffuse_rgb", "specular_rgb", "indirect_rgb", "direct_rgb", "env_map_rgb", "distance_median"):
        a = out[k].cpu().numpy()[idx]
        d = np.abs(a - r[k].numpy().reshape(a.shape)).max()
        assert d <= RGB_TOL, (k, d)


def test_forced_resampling_25001_vs_oracle_on_a_subset(rc_smooth):
    from nrc_amd import rc_ext
    from oracle import cache_ref
    rays = nrc_amd.synthetic_rays(N_BIG, seed=404)
    rng = np.random.Generator(np.random.PCG64(12))
    g = rng.gumbel(size=(N_BIG, 32)).astype(np.float32)
    jit = common.jitters(N_BIG, seed=6)
    idx = np.arange(3, N_BIG, 25)                                   # 1000 rays
    sub = {k: torch.from_numpy(np.asarray(v)[idx]) for k, v in rays.hot_fields().items()}
    ref = cache_ref.cache_forward(common.to_torch(common.weights_material_np(True)), nrc_amd.hotdog_config(), sub,
                                  [torch.from_numpy(j[idx]) for j in jit], resample=True, gumbel=torch.from_numpy(g[idx]),
                                  want_grad_normals=False)
    picks = np.zeros(N_BIG, np.int32)
    picks[idx] = ref["filtered_sampler_inds"][:, 0].numpy()
    mask = rc_ext.RC_PASS_CACHE | rc_ext.RC_PASS_RESAMPLE
    out = rc_smooth.render_rays(rays.hot_fields(), {"jitter": jit, "resample_inds": picks}, mask)
    torch.cuda.synchronize()
    r = ref["render"]
    for k in ("rgb", "acc", "diffuse_rgb", "specular_rgb", "direct_rgb", "indirect_rgb", "albedo_rgb", "means",
              "normals_pred", "distance_mean", "distance_median", "ray_dists"):
        a = out[k].cpu().numpy()[idx]
        d = np.abs(a - r[k].numpy().reshape(a.shape)).max()
        # colours at the north-star 1e-4.  normals_pred is ONE picked sample's normalised 3-vector of the MLP (no
        # average over samples here): the normalisation divides the vector's own fp32 error by its length -- the
        # 5e-4 this suite gives geometry extras (test_gpu_parity.py header); measured 1.5e-4 on the worst of 1000 rays
        assert d <= (5e-4 if k == "normals_pred" else RGB_TOL), (k, d)


def _subset_material_randoms(rnd, idx, cfg):
    """The random tensors of `idx`'s primary rays and of their secondary rays (ray-major blocks of Ks / Kd)."""
    Ks = int(round(cfg.num_secondary_samples * (1.0 - cfg.diffuse_sample_fraction)))
    Kd = int(round(cfg.num_secondary_samples * cfg.diffuse_sample_fraction))
    si = (idx[:, None] * Ks + np.arange(Ks)[None]).reshape(-1)
    di = (idx[:, None] * Kd + np.arange(Kd)[None]).reshape(-1)
    out = {}
    for k, v in rnd.items():
        if k == "jitter":
            out[k] = [j[idx] for j in v]
        elif k == "spec_jitter":
            out[k] = [j[si] for j in v]
        elif k == "diff_jitter":
            out[k] = [j[di] for j in v]
        elif k == "spec_gumbel":
            out[k] = v[si]
        elif k == "diff_gumbel":
            out[k] = v[di]
        else:
            out[k] = v[idx]
    return out, si, di


def test_material_stage_1024_primaries_vs_oracle_on_a_subset(rc_smooth):
    """configs[2] at the size bench.py times it (1024 primary rays, 32 768 secondary rays: the k_level_ray plan)."""
    from oracle import material_ref
    cfg = nrc_amd.hotdog_config()
    wn = common.weights_material_np(True)
    n = 1024
    rays = nrc_amd.synthetic_rays(n, seed=515)
    rnd = material_ref.draw_randoms(cfg, n, seed=21)
    idx = np.arange(5, n, 16)                                       # 64 primaries, 2 048 secondaries
    sub_rnd, si, di = _subset_material_randoms(rnd, idx, cfg)
    sub_rays = {k: torch.from_numpy(np.asarray(v)[idx]) for k, v in rays.hot_fields().items()}
    ref = material_ref.material_forward(common.to_torch(wn), cfg, sub_rays, sub_rnd)
    Ks, Kd = si.size // idx.size, di.size // idx.size
    picks = dict(inds=np.zeros(n, np.int32), spec_inds=np.zeros(n * Ks, np.int32), diff_inds=np.zeros(n * Kd, np.int32))
    picks["inds"][idx] = ref["inds"][:, 0].numpy()
    picks["spec_inds"][si] = ref["debug"]["specular"]["inds"].numpy().reshape(-1)
    picks["diff_inds"][di] = ref["debug"]["diffuse"]["inds"].numpy().reshape(-1)
    cres, mres = _material_with_picks(rc_smooth, rays, rnd, picks)
    assert np.array_equal(rc_smooth.workspace("inds", np.int32)[:n], picks["inds"])
    r = ref["render"]
    for k in MAT_ALL_KEYS:
        a = mres[k].cpu().numpy()[idx]
        d = np.abs(a - r[k].numpy().reshape(a.shape)).max()
        assert d <= RGB_TOL, (k, d)
    assert np.abs(cres["rgb"].cpu().numpy()[idx] - r["cache_rgb"].numpy()).max() <= 1e-5


def test_material_stage_second_smooth_seed_holds_1e4():
    """test_material_stage_smooth_field_holds_1e4 on another smooth weight set, other rays and other random inputs."""
    from nrc_amd import rc_ext
    from oracle import material_ref
    cfg = nrc_amd.hotdog_config()
    wn = common.weights_material_np(True, 2)
    rc = rc_ext.RadianceCache(cfg, 0)
    rc.load_weights(wn)
    n = 128
    rays = nrc_amd.synthetic_rays(n, seed=1201)
    rnd = material_ref.draw_randoms(cfg, n, seed=44)
    ref = material_ref.material_forward(common.to_torch(wn), cfg, common.rays_torch(rays), rnd)
    picks = dict(inds=ref["inds"][:, 0].numpy(), spec_inds=ref["debug"]["specular"]["inds"].numpy(),
                 diff_inds=ref["debug"]["diffuse"]["inds"].numpy())
    cres, mres = _material_with_picks(rc, rays, rnd, picks)
    r = ref["render"]
    for k in MAT_ALL_KEYS:
        a = mres[k].cpu().numpy()
        d = np.abs(a - r[k].numpy().reshape(a.shape)).max()
        assert d <= RGB_TOL, (k, d)
    assert np.abs(cres["rgb"].cpu().numpy() - r["cache_rgb"].numpy()).max() <= 1e-5
