"""rc_transient_data_backward on the GPU against the fp64 restatement of tests/transient_data_loss_ref.py.
Every comparison is loss_cases.check: 3 x the fp32 restatement's own distance from fp64 plus 1e-6 of the tensor's scale."""
import numpy as np
import pytest
import torch

import common
import loss_cases as lc
import nrc_amd
import transient_data_loss_ref as tref
from nrc_amd import config, rc_ext, train

pytestmark = pytest.mark.gpu

CHUNK = 256                     # kRcTdChunkRays
ADJOINTS = lc.TRANSIENT_ADJOINTS
LOOP_STEPS = 20
# The Adam loop's rate.  The target's head weights are loss_cases.perturbed: each element 5 % of itself away, which is an rms
# of 0.006 - 0.009 for the two He-uniform kernels (U(+-sqrt(6/64)), U(+-sqrt(6/128))).  Adam with eps = 1e-15 moves every
# element by about its rate per step whatever the gradient's size, so 20 steps at 1e-4 travel at most 0.002 per element and
# stay short of the target, while either schedule of the reference is unusable for a 20-step loop from count 0: the cache
# stage's 2 500-step delay starts at 1e-8 of its rate and moves no float32 weight, and the material stage's 0.002 steps a
# third of the whole distance in every element at once and lands 70 x above the first loss (Adam on the fp64 restatement
# does the same, to three digits).
LOOP_LR = 1e-4
UNSUPPORTED = -5                # RC_ERR_UNSUPPORTED


def _rc(smooth=False, weights=None):
    h = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    h.load_weights(common.weights_transient_np(smooth) if weights is None else weights)
    return h


@pytest.fixture(scope="module")
def handles():
    return {False: _rc(False), True: _rc(True)}


# shared with test_gpu_loss_settings, which runs the same comparison under a loss_cfg off the defaults
_batch, _target, _compare = lc.transient_batch, lc.transient_target, lc.transient_compare


@pytest.mark.parametrize("smooth", [False, True])
def test_loss_grads_and_adjoints_vs_fp64(handles, smooth):
    rc = handles[smooth]
    rays, jit = _batch(8, seed=31, jitter_seed=32)
    gt = _target(rc, rays, jit, 33)
    _compare(rc, smooth, rays, jit, gt, what=f"smooth={smooth}")


def test_far_samples_tile_range_skip(handles):
    rays, jit = _batch(8, seed=77, near=2.6, far=3.9)
    gt = _target(handles[False], rays, jit, 34)
    _, _, r64 = _compare(handles[False], False, rays, jit, gt, what="far")
    # the skip is really taken: whole column tiles of the heads get no gradient
    k = r64["grads"][tref.HEAD_IRR + "/kernel"]
    assert (np.abs(k).sum(0).reshape(700, 3).sum(1) == 0).sum() >= 32


def test_direct_spill_into_next_ray(handles):
    """The batch of test_transient_direct_spill_into_next_ray: samples whose direct bin is >= 700 read the NEXT ray's Gt."""
    rc = handles[False]
    rays, jit = _batch(8, seed=20200823)
    gt = _target(rc, rays, jit, 35)
    _, _, r64 = _compare(rc, False, rays, jit, gt, what="spill")
    t = rc.cfg.transient
    sh_ld = rc.workspace("tshade")[: 19 * 8 * 32].reshape(19, -1)
    d = (sh_ld[16] + sh_ld[17]) / t.exposure_time + t.transient_shift / t.exposure_time
    assert (d >= 700).any(), d.max()
    assert np.abs(r64["d_direct"]).max() > 0


def test_single_ray_and_chunk_plus_one(handles):
    rc = handles[True]
    for n in (1, CHUNK + 1):
        rays, jit = _batch(n, seed=41, jitter_seed=42)
        gt = _target(rc, rays, jit, 43)
        _compare(rc, True, rays, jit, gt, what=f"n={n}")


def test_lossmult_with_zeros_and_nocorr_pair(handles):
    rc = handles[False]
    n = 8
    rays, jit = _batch(n, seed=51, jitter_seed=52)
    gt = _target(rc, rays, jit, 53)
    _compare(rc, False, rays, jit, gt, lossmult=lc.lossmult(n), what="lossmult")
    rn, gn = _target(rc, rays, jit, 54), _target(rc, rays, jit, 55)
    _compare(rc, False, rays, jit, gt, rgb_nocorr=rn, gt_nocorr=gn, what="nocorr")


def test_bitwise_repeat_and_accumulation(handles):
    rc = handles[False]
    rays, jit = _batch(CHUNK + 8, seed=61, jitter_seed=62)
    gt = _target(rc, rays, jit, 63)
    rnd = {"jitter": jit}
    a, la = rc.transient_data_backward(rays, rnd, gt)
    adj = {k: rc.workspace("td:" + k).copy() for k, _ in ADJOINTS}
    b, lb = rc.transient_data_backward(rays, rnd, gt)
    assert torch.equal(a, b) and torch.equal(la, lb)
    for k, _ in ADJOINTS:
        assert np.array_equal(adj[k], rc.workspace("td:" + k)), k
    # accumulated into: one chunk's gradient added to itself is exactly twice it
    rays1, jit1 = {k: np.asarray(v)[:8] for k, v in rays.items()}, [j[:8] for j in jit]
    one, _ = rc.transient_data_backward(rays1, {"jitter": jit1}, gt[:8])
    two, _ = rc.transient_data_backward(rays1, {"jitter": jit1}, gt[:8], grad=one.clone())
    assert torch.equal(two, 2.0 * one) and float(one.abs().max()) > 0
    # grad=False: the loss and the adjoints without the heads' gradient
    none, lc_ = rc.transient_data_backward(rays, rnd, gt, grad=False)
    assert none is None and torch.equal(lc_, la)


def test_refusals(handles):
    rays, jit = _batch(4, seed=71)
    gt = np.zeros((4, 700, 3), np.float32)
    hot = common.make_rc()
    with pytest.raises(rc_ext.RcError) as e:
        hot.transient_data_backward(rays, None, gt, grad=False)
    assert e.value.code == UNSUPPORTED
    with pytest.raises(rc_ext.RcError) as e:
        hot.transient_head_grad_layout()
    assert e.value.code == UNSUPPORTED
    rc = handles[False]
    lib, st = rc.lib, torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(16, device="cuda")
    assert lib.rc_load_params_flat(rc._h, rc_ext.RC_LAYOUT_SHADER, buf.data_ptr(), st) == UNSUPPORTED
    assert lib.rc_load_params_flat(rc._h, 0, buf.data_ptr(), st) == UNSUPPORTED
    occ = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(use_occlusions=True), 0)
    occ.load_weights(common.weights_transient_np())
    with pytest.raises(rc_ext.RcError) as e:
        occ.transient_data_backward(rays, None, gt)
    assert e.value.code == UNSUPPORTED


def test_load_params_flat_renders_like_load_weights():
    w2 = lc.perturbed(lc.perturbed(common.weights_transient_np(), "transient_indirect_layer", 5), "output_rgba_layer", 6)
    a, b = _rc(weights=w2), _rc()
    rays, jit = _batch(64, seed=81, jitter_seed=82)
    rnd = {"jitter": jit}
    before = b.render_transient(rays, rnd, outputs=["rgb"])["rgb"].clone()
    layout, total = b.transient_head_grad_layout()
    b.load_params_flat("transient_heads", lc.flat_from_layout(layout, total, w2))
    ra, rb = a.render_transient(rays, rnd), b.render_transient(rays, rnd)
    assert not torch.equal(before, rb["rgb"])
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k


def test_adam_loop_lowers_the_loss():
    """transient_head_step, 20 steps on a fixed batch against a target rendered from perturbed head weights, at the constant
    rate LOOP_LR from count 0 (see there)."""
    w = common.weights_transient_np()
    w2 = lc.perturbed(lc.perturbed(w, "transient_indirect_layer", 7), "output_rgba_layer", 8)
    rays, jit = _batch(128, seed=91, jitter_seed=92)
    gt = _rc(weights=w2).render_transient(rays, {"jitter": jit}, outputs=["rgb"])["rgb"].clone()
    rc = _rc()
    ocfg = config.OptimizerConfig(lr_init=LOOP_LR, lr_final=LOOP_LR, lr_delay_steps=0, extra_opt_params=tuple(
        config.ExtraOptParams(g, LOOP_LR, LOOP_LR, 0, LOOP_LR, LOOP_LR, 0) for g in ("Cache", "SurfaceLightField")))
    opt = train.TransientHeadOptimizer(rc, ocfg)
    opt.init_from(w)
    assert [train.param_group(k) for k in opt.names()] == ["Cache", "Cache", "SurfaceLightField", "SurfaceLightField"]
    hist = [float(train.transient_head_step(rc, opt, rays, None, jit, gt)["data"]) for _ in range(LOOP_STEPS)]
    print("transient_head_step loop (data):", [f"{t:.6e}" for t in hist])
    assert opt.count == LOOP_STEPS and all(np.isfinite(hist))
    assert hist[-1] < hist[0], ("first and last loss", hist[0], hist[-1])
