"""The time-resolved cache's data loss as restated in tests/transient_data_loss_ref.py, on the CPU:
the restatement against central finite differences in fp64, a hand-computed known-answer case, and the adjoint identity of
the TransientVolumeIntegrator's two linear maps with their transposes written as explicit gathers."""
import dataclasses

import numpy as np
import pytest
import torch

import common
import loss_cases as lc
import nrc_amd
import transient_data_loss_ref as tref
from nrc_amd.config import TransientDataLossConfig
from oracle import transient_ref

CFG = TransientDataLossConfig()


def _case(n=3, B=5, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    rgb = rng.uniform(0.0, 0.3, size=(n, B, 3))
    gt = rng.uniform(0.0, 0.3, size=(n, B, 3))
    return rgb, gt, rng


def test_loss_equals_the_loops():
    rgb, gt, rng = _case()
    rn, gn = rgb + 0.01 * rng.standard_normal(rgb.shape), gt + 0.01 * rng.standard_normal(gt.shape)
    lm = np.array([1.0, 0.0, 1.7])
    gt[2, 1, 0] = 2e6                                      # over loss_thresh: channel 0 of ray 2 drops out
    # the defaults, then every non-default setting test_gpu_loss_settings runs on the device (clip_val and loss_thresh from
    # the finite part of this gt: the clip binds, the threshold drops whole channels)
    fin = np.where(gt < 1e6, gt, 0.0)
    cfgs = [CFG] + [lc.transient_setting(name, fin) for name in lc.TRANSIENT_SETTINGS]
    assert cfgs[4].clip_val < fin.max() and 0.1 <= lc.transient_loss_thresh(fin)[1] <= 0.5
    for cfg in cfgs:
        for kw in (dict(), dict(rgb_nocorr=rn, gt_nocorr=gn), dict(lossmult=lm), dict(rgb_nocorr=rn, gt_nocorr=gn, lossmult=lm)):
            t = {k: torch.from_numpy(v) for k, v in kw.items()}
            loss, mse = tref.data_loss(torch.from_numpy(rgb), torch.from_numpy(gt), cfg=cfg, **t)
            l2, m2 = tref.loop_loss(rgb, gt, cfg=cfg, **kw)
            assert abs(float(loss) - l2) <= 1e-12 * max(1.0, abs(l2)), (cfg, kw.keys(), float(loss), l2)
            assert abs(float(mse) - m2) <= 1e-9 * max(1.0, abs(m2))


@pytest.fixture(scope="module")
def settings_batch():
    """The batch of test_gpu_loss_settings' transient cases with the fp64 restatement's render in the device's place, and
    the restatement at the default settings."""
    rays, jit = lc.transient_batch(8, seed=31, jitter_seed=32)
    u = np.random.Generator(np.random.PCG64(33)).uniform(0.5, 1.5, size=(8, 700, 3))
    d64 = tref.chain(common.weights_transient_np(False), rays, jit, lambda rgb: (rgb * u).astype(np.float32))
    return rays, jit, (d64["rgb"] * u).astype(np.float32), d64


@pytest.mark.parametrize("name", lc.TRANSIENT_SETTINGS)
def test_settings_reach_the_result(settings_batch, name):
    """Every non-default setting moves the fp64 loss or the largest head gradient by more than 100 x the tolerance the GPU
    comparison grants (loss_cases.guard), so a device call that ignored the setting could not pass."""
    rays, jit, gt, d64 = settings_batch
    cfg = lc.transient_setting(name, gt)
    extra = {}
    if name == "combined":
        n = len(gt)
        rng = np.random.Generator(np.random.PCG64(34))
        extra = dict(lossmult=lc.lossmult(n), rgb_nocorr=(gt * rng.uniform(0.5, 1.5, size=gt.shape)).astype(np.float32),
                     gt_nocorr=(gt * rng.uniform(0.5, 1.5, size=gt.shape)).astype(np.float32))
        d64 = lc.transient_refs(False, rays, jit, gt, **extra)[0]      # the defaults on the same extras
    if name == "loss_thresh":
        share = lc.transient_loss_thresh(gt)[1]
        assert 0.1 <= share <= 0.5, share
    if name in ("clip_val", "combined"):
        assert cfg.clip_val < float(gt.max())
    r64, r32 = lc.transient_refs(False, rays, jit, gt, loss_cfg=cfg, **extra)
    lc.transient_guard(name, r64, r32, d64)
    if name == "loss_thresh":
        zeroed = gt.max(axis=1) > cfg.loss_thresh
        assert np.all(r64["G"].transpose(0, 2, 1)[zeroed] == 0.0)


def test_known_answer_two_rays_four_bins():
    """2 rays, 4 bins, by hand.  Ray 0: rgb = 0.1 everywhere, gt = 0.2 everywhere -> d = -0.1.  c = max(rgb, gt) = 0.2, the
    scale 1 / (4 * 0.2 + 1e-2) = 1 / 0.81.  Main term per channel: 4 bins * 2 * 0.01 = 0.08.  Gauss constant: (0.5 * -0.4)^2
    * 2 * 0.01 = 0.0008, counted ONCE (divided by 4, broadcast over 4 bins, summed).  Ray 1: gt has one bin over
    loss_thresh in channel 1 -> that channel drops out; the others as ray 0 with lossmult 2."""
    rgb = np.full((2, 4, 3), 0.1)
    gt = np.full((2, 4, 3), 0.2)
    gt[1, 2, 1] = 1e7
    lm = np.array([1.0, 2.0])
    s = 1.0 / 0.81
    per_channel = s * (0.08 + 0.0008)
    want = (3 * per_channel + 2 * 2.0 * per_channel) / 6.0
    loss, mse = tref.data_loss(torch.from_numpy(rgb), torch.from_numpy(gt), lossmult=torch.from_numpy(lm), cfg=CFG)
    assert abs(float(loss) - want) <= 1e-14, (float(loss), want)
    assert abs(float(mse) - (3 * 0.04 + 2 * 2.0 * 0.04) / 6.0) <= 1e-14
    # the gauss constant counted once: without it the loss drops by exactly its share
    no_gauss, _ = tref.data_loss(torch.from_numpy(rgb), torch.from_numpy(gt), lossmult=torch.from_numpy(lm),
                                 cfg=dataclasses.replace(CFG, data_loss_gauss_mult=0.0))
    assert abs((float(loss) - float(no_gauss)) - s * 0.0008 * 7 / 6.0) <= 1e-14
    # rgb_nocorr given: the second factor is the nocorr difference (here twice d), the value doubles; defaulted = given as rgb
    rn = np.full((2, 4, 3), 0.0)
    twice, _ = tref.data_loss(torch.from_numpy(rgb), torch.from_numpy(gt), torch.from_numpy(rn), torch.from_numpy(np.full((2, 4, 3), 0.2)),
                              torch.from_numpy(lm), CFG)
    assert abs(float(twice) - 2.0 * want) <= 1e-14
    same, _ = tref.data_loss(torch.from_numpy(rgb), torch.from_numpy(gt), torch.from_numpy(rgb), torch.from_numpy(gt),
                             torch.from_numpy(lm), CFG)
    assert float(same) == float(loss)
    # the gradient is 2 sg(dn) s (half the derivative of the value), plus the constant's share, zero in the dropped channel
    r = torch.from_numpy(rgb).requires_grad_(True)
    tref.data_loss(r, torch.from_numpy(gt), lossmult=torch.from_numpy(lm), cfg=CFG)[0].backward()
    g = r.grad.numpy()
    want_g = s * (2 * -0.1 + 2 * 0.25 * -0.4 * 0.01) / 6.0
    assert np.allclose(g[0], want_g, rtol=0, atol=1e-15) and np.allclose(g[1, :, [0, 2]], 2 * want_g, rtol=0, atol=1e-15)
    assert np.all(g[1, :, 1] == 0.0)


def test_restatement_against_finite_differences_fp64():
    """d loss / d (head tensors) of the whole chain against central differences along random directions.  Differences of
    the VALUE see every factor, the stopped ones too: the second factor is frozen by passing the base render as the nocorr
    pair, and the scale by use_gt_rawnerf (c = clip(gt), a constant; the stop on the rendered c is pinned by the known-answer
    test's gradient)."""
    lcfg = dataclasses.replace(CFG, use_gt_rawnerf=True)
    n = 4
    rays = nrc_amd.synthetic_transient_rays(n, seed=11).hot_fields()
    jit = [j.reshape(-1) for j in common.jitters(n, seed=12)]
    w = common.weights_transient_np()
    rng = np.random.Generator(np.random.PCG64(3))
    base = tref.chain(w, rays, jit, lambda rgb: rgb * rng.uniform(0.5, 1.5, size=rgb.shape), loss_cfg=lcfg)
    rng = np.random.Generator(np.random.PCG64(3))
    gt = base["rgb"] * rng.uniform(0.5, 1.5, size=base["rgb"].shape)
    rn, gn = base["rgb"].copy(), gt.copy()
    for name in tref.HEAD_TENSORS:
        u = np.random.Generator(np.random.PCG64(5)).standard_normal(w[name].shape)
        eps = 1e-4
        vals = []
        for sgn in (+1.0, -1.0):
            w2 = dict(w)
            w2[name] = w[name].astype(np.float64) + sgn * eps * u
            vals.append(tref.chain(w2, rays, jit, gt, rgb_nocorr=rn, gt_nocorr=gn, loss_cfg=lcfg)["loss"])
        fd = (vals[0] - vals[1]) / (2 * eps)
        an = float((base["grads"][name] * u).sum())
        assert abs(fd - an) <= 1e-6 * max(abs(an), 1e-12) + 1e-12, (name, fd, an)


def test_integrator_adjoint_identities():
    """<A x, y> = <x, A^T y> for shift_direct (next-ray spill and the dropped tail included) and shift_map_coordinates,
    the transposes written as gathers."""
    rng = np.random.Generator(np.random.PCG64(1))
    n, S, B = 5, 6, 40
    dists = torch.from_numpy(rng.uniform(0.0, 2.2 * B, size=(n, S)))
    dists[0, 0] = 7.0                                      # an integral distance: floor == ceil
    assert (dists >= B).any() and (dists[-1] >= B).any()   # spill into the next ray, and past the end of the batch
    w = torch.from_numpy(rng.uniform(0.1, 1.0, size=(n, S)))
    x = torch.from_numpy(rng.standard_normal((n, S, 3)))
    y = torch.from_numpy(rng.standard_normal((n, B, 3)))
    Ax = transient_ref.shift_direct(dists, x, w, B)
    ATy = w[..., None] * tref.shift_direct_T(dists, y, B)
    assert abs(float((Ax * y).sum()) - float((x * ATy).sum())) <= 1e-12
    N = 7
    d = torch.from_numpy(rng.uniform(-3.0, B + 3.0, size=N))
    d[0] = 4.0
    h = torch.from_numpy(rng.standard_normal((N, B, 3)))
    g = torch.from_numpy(rng.standard_normal((N, B, 3)))
    Ah = transient_ref.shift_map_coordinates(h, d, 1.0, B)
    ATg = tref.shift_map_coordinates_T(g, d, B)
    assert abs(float((Ah * g).sum()) - float((h * ATg).sum())) <= 1e-12
    # and against autograd, as a second witness
    h2 = h.clone().requires_grad_(True)
    (transient_ref.shift_map_coordinates(h2, d, 1.0, B) * g).sum().backward()
    assert torch.allclose(h2.grad, ATg, rtol=0, atol=1e-13)


def test_config_provenance():
    c = TransientDataLossConfig()
    assert (c.loss_type, c.rawnerf_exponent, c.rawnerf_eps, c.data_loss_mult) == ("rawnerf_transient_unbiased", 1.0, 1e-2, 1.0)
    assert (c.data_loss_gauss_mult, tuple(c.transient_gauss_sigma_scales), c.transient_gauss_constant_scale) == (0.01, (), 0.5)
    assert (c.loss_thresh, c.use_gt_rawnerf, c.use_combined_rawnerf, c.mask_lossmult, c.clip_eval, c.use_itof) == \
        (1e6, False, True, False, False, False)
