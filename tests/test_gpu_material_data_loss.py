"""rc_material_data_backward on the GPU: the forward against rc_render_material, the loss and every tensor of the material
layout against the fp64 torch restatement (tests/material_data_loss_ref.py) at the call's own shading points, call
semantics and a material-stage training loop."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import common
import loss_cases as lc
import material_data_loss_ref as md
import material_smoothness_ref as ms
import nrc_amd
from nrc_amd import config, rc_ext, train

CFG = nrc_amd.hotdog_config()
RC_ERR_INVALID_ARG, RC_ERR_UNSUPPORTED, RC_ERR_MISSING_WEIGHT = -1, -5, -3

pytestmark = pytest.mark.gpu


def _case(n, K=8, seed=3):
    return (*lc.material_case(n, K, seed), lc.uniform_gt(n, seed + 2))


def _fwd(rc, n, K):
    nsec = n * K
    sizes = dict(m_pts=3 * n, m_nrm=3 * n, filt_weight=n, m_feat=32 * n, m_mat=5 * n, m_local_view=3 * n,
                 sec_samples=5 * nsec, sec_dirs=3 * nsec, sec_rgb=3 * nsec, sec_acc=nsec, sec_env=3 * nsec)
    return {k: rc.workspace(k)[:v].copy() for k, v in sizes.items()}


@pytest.mark.parametrize("K", [8, 32])
def test_forward_is_bitwise_render_material(K):
    rc = lc.make_material_rc()
    n = 1500
    rays, rnd, gt = _case(n, K)
    cres, mres = rc.render_material(rays, rnd, num_secondary_samples=K)
    torch.cuda.synchronize()
    want = _fwd(rc, n, K)
    want_rgb = mres["rgb"].cpu().numpy().reshape(-1)
    want_crgb = cres["rgb"].cpu().numpy().reshape(-1)
    cfg = dataclasses.replace(config.MaterialDataLossConfig(), num_secondary_samples=K)
    rc.material_data_backward(rays, rnd, gt, K, lossmult=lc.lossmult(n), cfg=cfg)
    torch.cuda.synchronize()
    got = _fwd(rc, n, K)
    for k in want:
        assert np.array_equal(want[k].view(np.uint32), got[k].view(np.uint32)), k
    assert np.array_equal(rc.workspace("md:rgb")[: 3 * n].view(np.uint32), want_rgb.view(np.uint32))
    assert np.array_equal(rc.workspace("md:cache_rgb")[: 3 * n].view(np.uint32), want_crgb.view(np.uint32))


def _trace_tensors(rc, n, K, dt):
    Ks = Kd = K // 2
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    f = _fwd(rc, n, K)
    sm, rgb_in, acc_in, env_in = md.split_trace(n, Ks, Kd, t(f["sec_samples"]), t(f["sec_rgb"]), t(f["sec_acc"]),
                                                t(f["sec_env"]))
    return (Ks, Kd, t(f["m_local_view"]).reshape(n, 3), sm, rgb_in, acc_in, env_in), f


@pytest.mark.parametrize("n", [512, 3001])
def test_loss_and_every_tensor_against_fp64_autograd(n):
    """At the call's own shading points and trace: the loss and every tensor of the material layout within 3x the fp32
    restatement's distance from fp64 (plus a 1e-6 relative floor)."""
    K = 8
    rc = lc.make_material_rc()
    rays, rnd, gt = _case(n, K, seed=21)
    lm = lc.lossmult(n, seed=22)
    cres, mres = rc.render_material(rays, rnd, num_secondary_samples=K)
    S = CFG.sampling_strategy[-1][2]
    acc_p = rc.workspace("weights2")[: n * S].reshape(n, S).sum(-1)
    acc_p_dev = mres["acc"].cpu().numpy().reshape(-1) if "acc" in mres else acc_p
    flat, loss = rc.material_data_backward(rays, rnd, gt, K, lossmult=lm)
    torch.cuda.synchronize()
    layout, total = rc.material_grad_layout()
    assert [(nm, tuple(s)) for nm, _, s in layout] == ms.material_layout(CFG)
    got = flat.cpu().numpy()
    crgb = rc.workspace("md:cache_rgb")[: 3 * n].reshape(n, 3)
    fw = rc.workspace("filt_weight")[:n]
    wn = {k: v for k, v in common.weights_material_np().items() if "MaterialShader" in k}
    refs, losses = {}, {}
    for dt in (torch.float64, torch.float32):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
        trace, f = _trace_tensors(rc, n, K, dt)
        w = {k: t(v).requires_grad_(True) for k, v in wn.items()}
        ls, rgb = md.chain_loss(w, CFG, t(f["m_pts"]).reshape(n, 3), trace, t(gt), t(crgb), t(fw), t(acc_p_dev), t(lm),
                                bg=CFG.bg_intensity)
        gs = torch.autograd.grad(ls, list(w.values()), allow_unused=True)
        refs[dt] = {k: (np.zeros(v.shape) if g is None else g.detach().double().numpy()) for (k, v), g in zip(w.items(), gs)}
        losses[dt] = float(ls)
    assert losses[torch.float64] > 0
    lc.check(np.array([float(loss[0])]), np.array([losses[torch.float64]]), np.array([losses[torch.float32]]), "loss")
    for name, off, shape in layout:
        size = int(np.prod(shape))
        lc.check(got[off: off + size], refs[torch.float64][name].reshape(-1), refs[torch.float32][name].reshape(-1), name)
    assert float(np.abs(got).max()) > 0


def test_semantics():
    K = 8
    rc = lc.make_material_rc()
    n = 777
    rays, rnd, gt = _case(n, K, seed=31)
    lm = lc.lossmult(n, seed=32)
    layout, total = rc.material_grad_layout()
    dense0 = [off for name, off, _ in layout if name.endswith("bottleneck_layer/kernel")][0]
    f1, l1 = rc.material_data_backward(rays, rnd, gt, K, lossmult=lm)
    f1, l1 = f1.clone(), l1.clone()
    f2, l2 = rc.material_data_backward(rays, rnd, gt, K, lossmult=lm)
    assert torch.equal(l1, l2)                                    # bitwise stable loss and dense gradients
    assert torch.equal(f1[dense0:], f2[dense0:])
    assert float(f1[:dense0].abs().max()) > 0 and float(f1[dense0:].abs().max()) > 0
    acc = torch.ones_like(f1)                                     # accumulates
    rc.material_data_backward(rays, rnd, gt, K, lossmult=lm, grad=acc)
    assert torch.equal(acc[dense0:] - 1.0, (f1[dense0:] + 1.0) - 1.0)
    np.testing.assert_allclose(acc.cpu().numpy(), 1.0 + f1.cpu().numpy(), rtol=1e-5, atol=1e-6 * float(f1.abs().max()))
    fz, lz = rc.material_data_backward(rays, rnd, gt, K, lossmult=lm, grad=False)   # NULL grads: the loss only
    assert fz is None and torch.equal(lz, l1)
    s = torch.cuda.Stream()                                       # a non-default stream
    with torch.cuda.stream(s):
        fs, ls = rc.material_data_backward(rays, rnd, gt, K, lossmult=lm)
    s.synchronize()
    assert torch.equal(ls, l1) and torch.equal(fs[dense0:], f1[dense0:])
    # raw calls: n = 0 writes nothing; a loss-only call leaves a gradient buffer alone; null loss / gt are refused
    r, held, _ = rc._rays_struct(rays)
    rr, mrd = rc._material_randoms(rnd, n, K, held)
    g_t = torch.from_numpy(gt).cuda()
    cfg = rc_ext.rc_material_data_loss(mult=1.0, weight=0.1, exponent=1.0, eps=1e-2, clip_val=1e4, thresh=1e6,
                                       use_gt_rawnerf=0, use_combined_rawnerf=1, use_norm_rawnerf=0)
    g0 = torch.zeros(total, device="cuda")
    out = torch.zeros(1, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    fn = rc.lib.rc_material_data_backward
    assert fn(rc._h, C.byref(r), g_t.data_ptr(), None, 0, C.byref(rr), C.byref(mrd), K, C.byref(cfg), g0.data_ptr(),
              out.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert float(g0.abs().max()) == 0.0 and float(out.abs().max()) == 0.0
    assert fn(rc._h, C.byref(r), g_t.data_ptr(), None, n, C.byref(rr), C.byref(mrd), K, C.byref(cfg), None,
              out.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert float(g0.abs().max()) == 0.0 and float(out[0]) > 0.0
    assert fn(rc._h, C.byref(r), g_t.data_ptr(), None, n, C.byref(rr), C.byref(mrd), K, C.byref(cfg), g0.data_ptr(),
              None, stream) == RC_ERR_INVALID_ARG
    assert fn(rc._h, C.byref(r), None, None, n, C.byref(rr), C.byref(mrd), K, C.byref(cfg), g0.data_ptr(),
              out.data_ptr(), stream) == RC_ERR_INVALID_ARG
    # a handle without the material weights, and a time-resolved handle
    bare = rc_ext.RadianceCache(CFG, 0)
    bare.load_weights(common.weights_np())
    rb, heldb, _ = bare._rays_struct(rays)
    rrb, mrb = bare._material_randoms(rnd, n, K, heldb)
    assert bare.lib.rc_material_data_backward(bare._h, C.byref(rb), g_t.data_ptr(), None, n, C.byref(rrb), C.byref(mrb), K,
                                              C.byref(cfg), None, out.data_ptr(), stream) == RC_ERR_MISSING_WEIGHT
    tr = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    tr.load_weights(common.weights_transient_np())
    r3, held3, _ = tr._rays_struct(rays)
    rr3, mr3 = tr._material_randoms(rnd, n, K, held3)
    assert tr.lib.rc_material_data_backward(tr._h, C.byref(r3), g_t.data_ptr(), None, n, C.byref(rr3), C.byref(mr3), K,
                                            C.byref(cfg), None, out.data_ptr(), stream) == RC_ERR_UNSUPPORTED
    del held, heldb, held3
    torch.cuda.synchronize()


LOOP_STEPS = 40


def test_material_stage_loop_lowers_the_data_loss_and_resumes():
    """material_stage_step (data + smoothness + regularizer) on a fixed batch, at the material-stage schedule of the
    MaterialShader group (OptimizerConfig(material=True))."""
    rc = lc.make_material_rc()
    opt = train.MaterialOptimizer(rc, config.OptimizerConfig(material=True))
    opt.init_from(common.weights_material_np(), count=0)
    n = 2048
    rays, rnd, gt = _case(n, 8, seed=61)
    noise = lc.normal_noise(n, 62)

    def each(losses):
        assert set(losses) == {"data", "material_smoothness", "regularizer/material_grid", "material_ray_sampler"}

    step = lambda: train.material_stage_step(rc, opt, rays, rnd, gt, noise)
    lc.step_loop(step, lambda losses: float(losses["data"]), opt, 0, LOOP_STEPS,
                 lambda totals: min(totals[-3:]) < 0.9 * totals[0], "material_stage_step loop (data):",
                 lambda t: f"{t:.6e}", each=each, render=lambda: lc.material_render(rc, 8))
