"""rc_material_smoothness_backward and rc_material_regularizer on the GPU: the forward against rc_render_material, the loss
and every tensor of the material layout against the fp64 torch restatement (tests/material_smoothness_ref.py), call
semantics, the regularizer, the material-layout refresh and a training loop."""
import ctypes as C

import numpy as np
import pytest
import torch

import common
import loss_cases as lc
import material_smoothness_ref as mr
import nrc_amd
from nrc_amd import config, rc_ext, train

CFG = nrc_amd.hotdog_config()
RC_ERR_INVALID_ARG, RC_ERR_UNSUPPORTED, RC_ERR_MISSING_WEIGHT = -1, -5, -3

pytestmark = pytest.mark.gpu


def _case(n, seed=3):
    return (*lc.material_case(n, seed=seed), lc.normal_noise(n, seed + 2))


def _fwd(rc, n):
    sizes = dict(m_pts=3 * n, filt_weight=n, m_mat=5 * n)
    return {k: rc.workspace(k)[:v].copy() for k, v in sizes.items()}


def test_forward_is_bitwise_render_material():
    rc = lc.make_material_rc()
    n = 1500
    rays, rnd, noise = _case(n)
    rc.render_material(rays, rnd)
    want = _fwd(rc, n)
    rc.material_smoothness_backward(rays, rnd, noise, lossmult=lc.lossmult(n))
    got = _fwd(rc, n)
    for k in want:
        assert np.array_equal(want[k].view(np.uint32), got[k].view(np.uint32)), k
    pts = rc.workspace("ms:pts")[: 6 * n].reshape(2, n, 3)
    assert np.array_equal(pts[0], want["m_pts"].reshape(n, 3))
    assert np.array_equal(pts[1], want["m_pts"].reshape(n, 3) + noise * np.float32(0.01))


@pytest.mark.parametrize("n", [512, 3001])
def test_loss_and_every_tensor_against_fp64_autograd(n):
    """At the call's own shading points (m_pts, x' from "ms:pts", filt_weight): the loss and every tensor of the material
    layout within 3x the fp32 restatement's distance from fp64 (plus a 1e-6 relative floor)."""
    rc = lc.make_material_rc()
    rays, rnd, noise = _case(n, seed=21)
    lm = lc.lossmult(n, seed=22)
    flat, loss = rc.material_smoothness_backward(rays, rnd, noise, lossmult=lm)
    torch.cuda.synchronize()
    layout, total = rc.material_grad_layout()
    assert [(nm, tuple(s)) for nm, _, s in layout] == mr.material_layout(CFG)
    got = flat.cpu().numpy()
    pts = rc.workspace("ms:pts")[: 6 * n].reshape(2, n, 3)
    fw = rc.workspace("filt_weight")[:n]
    mats = (rc.workspace("m_mat")[: 5 * n].reshape(n, 5), rc.workspace("ms:mat_p")[: 5 * n].reshape(n, 5))
    wn = {k: v for k, v in common.weights_material_np().items() if "MaterialShader" in k}
    refs, losses = {}, {}
    for dt in (torch.float64, torch.float32):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
        w = {k: t(v).requires_grad_(True) for k, v in wn.items()}
        ls = mr.chain_loss(w, CFG, t(pts[0]), t(pts[1]), t(lm), t(fw))
        gs = torch.autograd.grad(ls, list(w.values()), allow_unused=True)
        refs[dt] = {k: (np.zeros(v.shape) if g is None else g.detach().double().numpy()) for (k, v), g in zip(w.items(), gs)}
        losses[dt] = float(ls)
        if dt == torch.float64:       # the loss terms on the kernel's own materials
            split = lambda m: (t(m[:, :3]), t(m[:, 3]), t(m[:, 4]))
            lk = float(mr.smoothness_loss(split(mats[0]), split(mats[1]), t(lm) * t(fw)))
    assert losses[torch.float64] > 0
    lc.check(np.array([float(loss[0])]), np.array([losses[torch.float64]]), np.array([losses[torch.float32]]), "loss")
    assert float(loss[0]) == pytest.approx(lk, rel=1e-5)
    for name, off, shape in layout:
        size = int(np.prod(shape))
        g64 = refs[torch.float64][name].reshape(-1)
        g32 = refs[torch.float32][name].reshape(-1)
        lc.check(got[off: off + size], g64, g32, name)
    assert float(np.abs(got).max()) > 0


def test_zero_noise_gives_zero_loss():
    rc = lc.make_material_rc()
    n = 999
    rays, rnd, _ = _case(n, seed=25)
    _, loss = rc.material_smoothness_backward(rays, rnd, np.zeros((n, 3), np.float32), lossmult=lc.lossmult(n))
    assert float(loss[0]) == 0.0
    assert np.array_equal(rc.workspace("m_mat")[: 5 * n], rc.workspace("ms:mat_p")[: 5 * n])


def test_semantics():
    rc = lc.make_material_rc()
    n = 777
    rays, rnd, noise = _case(n, seed=31)
    lm = lc.lossmult(n, seed=32)
    layout, total = rc.material_grad_layout()
    dense0 = [off for name, off, _ in layout if name.endswith("bottleneck_layer/kernel")][0]
    f1, l1 = rc.material_smoothness_backward(rays, rnd, noise, lossmult=lm)
    f1, l1 = f1.clone(), l1.clone()
    f2, l2 = rc.material_smoothness_backward(rays, rnd, noise, lossmult=lm)
    assert torch.equal(l1, l2)                                    # bitwise stable loss and dense gradients
    assert torch.equal(f1[dense0:], f2[dense0:])
    assert float(f1[:dense0].abs().max()) > 0 and float(f1[dense0:].abs().max()) > 0
    acc = torch.ones_like(f1)                                     # accumulates
    rc.material_smoothness_backward(rays, rnd, noise, lossmult=lm, grad=acc)
    assert torch.equal(acc[dense0:] - 1.0, (f1[dense0:] + 1.0) - 1.0)
    np.testing.assert_allclose(acc.cpu().numpy(), 1.0 + f1.cpu().numpy(), rtol=1e-5, atol=1e-6 * float(f1.abs().max()))
    fz, lz = rc.material_smoothness_backward(rays, rnd, noise, lossmult=lm, grad=False)   # NULL grads: the loss only
    assert fz is None and torch.equal(lz, l1)
    s = torch.cuda.Stream()                                       # a non-default stream
    with torch.cuda.stream(s):
        fs, ls = rc.material_smoothness_backward(rays, rnd, noise, lossmult=lm)
    s.synchronize()
    assert torch.equal(ls, l1) and torch.equal(fs[dense0:], f1[dense0:])
    # raw calls: n = 0 writes nothing; a loss-only call leaves a gradient buffer alone; null loss / noise are refused
    r, held, _ = rc._rays_struct(rays)
    rr, mrd = rc._shading_randoms(rnd, held)
    nz = torch.from_numpy(noise).cuda()
    cfg = rc_ext.rc_material_smoothness_loss(mult=1.0, weight_albedo=1e-4, weight_other=1e-4, noise=0.01, tensoir_albedo=1)
    g0 = torch.zeros(total, device="cuda")
    out = torch.zeros(1, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    fn = rc.lib.rc_material_smoothness_backward
    assert fn(rc._h, C.byref(r), None, 0, C.byref(rr), C.byref(mrd), nz.data_ptr(), C.byref(cfg), g0.data_ptr(),
              out.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert float(g0.abs().max()) == 0.0 and float(out.abs().max()) == 0.0
    assert fn(rc._h, C.byref(r), None, n, C.byref(rr), C.byref(mrd), nz.data_ptr(), C.byref(cfg), None, out.data_ptr(),
              stream) == 0
    torch.cuda.synchronize()
    assert float(g0.abs().max()) == 0.0 and float(out[0]) > 0.0
    assert fn(rc._h, C.byref(r), None, n, C.byref(rr), C.byref(mrd), nz.data_ptr(), C.byref(cfg), g0.data_ptr(), None,
              stream) == RC_ERR_INVALID_ARG
    assert fn(rc._h, C.byref(r), None, n, C.byref(rr), C.byref(mrd), None, C.byref(cfg), g0.data_ptr(), out.data_ptr(),
              stream) == RC_ERR_INVALID_ARG
    # a handle without the material weights, and a time-resolved handle
    bare = rc_ext.RadianceCache(CFG, 0)
    bare.load_weights(common.weights_np())
    rb, heldb, _ = bare._rays_struct(rays)
    rrb, mrb = bare._shading_randoms(rnd, heldb)
    assert bare.lib.rc_material_smoothness_backward(bare._h, C.byref(rb), None, n, C.byref(rrb), C.byref(mrb), nz.data_ptr(),
                                                    C.byref(cfg), None, out.data_ptr(), stream) == RC_ERR_MISSING_WEIGHT
    tr = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    tr.load_weights(common.weights_transient_np())
    r3, held3, _ = tr._rays_struct(rays)
    rr3, mr3 = tr._shading_randoms(rnd, held3)
    assert tr.lib.rc_material_smoothness_backward(tr._h, C.byref(r3), None, n, C.byref(rr3), C.byref(mr3), nz.data_ptr(),
                                                  C.byref(cfg), None, out.data_ptr(), stream) == RC_ERR_UNSUPPORTED
    assert tr.lib.rc_material_regularizer(tr._h, 1.0, None, out.data_ptr(), stream) == RC_ERR_UNSUPPORTED
    del held, heldb, held3
    torch.cuda.synchronize()


def test_regularizer_against_numpy():
    rc = lc.make_material_rc()
    w = common.weights_material_np()
    layout, total = rc.material_grad_layout()
    flat, loss = rc.material_regularizer(0.7)
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    want = 0.0
    for name, off, shape in layout:
        size = int(np.prod(shape))
        if "material_grid" in name:
            x = np.asarray(w[name], np.float64).reshape(-1)
            want += 0.5 * np.mean(x * x)
            np.testing.assert_allclose(got[off: off + size], 0.7 * x / size, rtol=1e-6, atol=1e-30)
        else:
            assert float(np.abs(got[off: off + size]).max()) == 0.0, name
    assert float(loss[0]) == pytest.approx(0.7 * want, rel=1e-6)


def test_load_params_flat_material_renders_as_load_weights():
    w2 = lc.perturbed(common.weights_material_np(), "MaterialShader", 5)
    a = lc.make_material_rc(w2)
    b = lc.make_material_rc()
    b.load_params_flat("material", lc.flat_from_layout(*b.material_grad_layout(), w2))
    ra, rb = lc.material_render(a), lc.material_render(b)
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k


LOOP_STEPS = 40


def test_training_loop_lowers_the_loss_and_resumes():
    """material_step on a fixed batch.  The learning rate is the test's choice: the material-stage schedule of the
    MaterialShader group (OptimizerConfig(material=True): 0.002, no delay), not the cache stage's 5e-4 behind a
    2 500-step delay, so that 40 steps move the loss."""
    rc = lc.make_material_rc()
    opt = train.MaterialOptimizer(rc, config.OptimizerConfig(material=True))
    opt.init_from(common.weights_material_np(), count=0)
    n = 2048
    rays, rnd, noise = _case(n, seed=61)
    cfg = config.MaterialSmoothnessConfig()

    def each(losses):
        assert set(losses) == {"material_smoothness", "regularizer/material_grid", "material_ray_sampler"}
        assert float(losses["material_ray_sampler"]) == 0.0

    step = lambda: train.material_step(rc, opt, rays, rnd, noise, cfg=cfg)
    # the state two steps back is resumed: the handle renders bitwise what it rendered then, and the run goes on
    lc.step_loop(step, lambda losses: float(losses["material_smoothness"]), opt, 0, LOOP_STEPS,
                 lambda totals: min(totals[-3:]) < totals[0], "material_step loop:", lambda t: f"{t:.6e}",
                 each=each, render=lambda: lc.material_render(rc))
    assert {train.param_group(k) for k in opt.names()} == {"MaterialShader"}
