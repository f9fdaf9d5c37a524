"""rc_light_sampling_backward and rc_light_regularizer on the GPU: the forward against rc_render_material, the loss kernel
and the whole chain against the fp64 torch restatement (tests/light_sampling_ref.py), call semantics, the regularizer, the
light-layout refresh and a training loop."""
import ctypes as C

import numpy as np
import pytest
import torch

import common
import light_sampling_ref as lr
import loss_cases as lc
import nrc_amd
from nrc_amd import config, rc_ext, train

CFG = nrc_amd.hotdog_config()
RC_ERR_UNSUPPORTED, RC_ERR_MISSING_WEIGHT = -5, -3
FWD = ("m_pts", "m_nrm", "l_vmf", "l_vmf_logit", "sec_dirs", "sec_samples", "sec_rgb")

pytestmark = pytest.mark.gpu


def _split(K):
    Kd = int(round(K * CFG.diffuse_sample_fraction))
    return K - Kd, Kd


def _fwd(rc, n, K):
    Ks, Kd = _split(K)
    nsec = n * K
    sizes = dict(m_pts=3 * n, m_nrm=3 * n, l_vmf=640 * n, l_vmf_logit=128 * n, sec_dirs=3 * nsec, sec_samples=5 * nsec,
                 sec_rgb=3 * nsec)
    return {k: rc.workspace(k)[:v].copy() for k, v in sizes.items()}


@pytest.mark.parametrize("K", [8, 32])
def test_forward_is_bitwise_render_material(K):
    rc = lc.make_material_rc()
    n = 1500
    rays, rnd = lc.material_case(n, K)
    rc.render_material(rays, rnd, K)
    want = _fwd(rc, n, K)
    rc.light_sampling_backward(rays, rnd, K, lossmult=lc.lossmult(n))
    got = _fwd(rc, n, K)
    for k in FWD:
        assert np.array_equal(want[k].view(np.uint32), got[k].view(np.uint32)), k


def _restated(rc, n, K, rnd, lm, dtype):
    Ks, Kd = _split(K)
    b = _fwd(rc, n, K)
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    vp = t(rc.workspace("ls:vp")[: 640 * n]).reshape(n, 128, 5).requires_grad_(True)
    spec, diff = lr.split_samples(b["sec_dirs"], b["sec_samples"], b["sec_rgb"], b["m_nrm"], n, Ks, Kd, dtype)
    vm, kap, lg = lr.get_vmfs(vp, t(rnd["vmf_noise"]), t(b["m_pts"]).reshape(n, 3), CFG.vmf_scale)
    loss = lr.light_sampling_loss(vm, kap, lg, spec, diff, t(lm))
    (g,) = torch.autograd.grad(loss, vp)
    return float(loss), g.reshape(n, 640).numpy()


def test_loss_kernel_against_restatement():
    """The loss and d loss / d vmf_params on the forward's own buffers, within 3x the fp32 restatement's distance from
    fp64 (plus a 1e-6 relative floor)."""
    rc = lc.make_material_rc()
    n, K = 1024, 8
    rays, rnd = lc.material_case(n, K, seed=11)
    lm = lc.lossmult(n)
    _, loss = rc.light_sampling_backward(rays, rnd, K, lossmult=lm)
    torch.cuda.synchronize()
    dvp = rc.workspace("ls:dvp")[: 640 * n].reshape(n, 640)
    l64, g64 = _restated(rc, n, K, rnd, lm, torch.float64)
    l32, g32 = _restated(rc, n, K, rnd, lm, torch.float32)
    assert l64 > 0 and float(np.abs(g64).max()) > 0
    lc.check(np.array([float(loss[0])]), np.array([l64]), np.array([l32]), "loss")
    lc.check(dvp, g64, g32, "d vmf_params")


def test_whole_chain_against_fp64_autograd():
    rc = lc.make_material_rc()
    n, K = 512, 8
    rays, rnd = lc.material_case(n, K, seed=21)
    lm = lc.lossmult(n, seed=22)
    flat, _ = rc.light_sampling_backward(rays, rnd, K, lossmult=lm)
    torch.cuda.synchronize()
    layout, total = rc.light_grad_layout()
    assert [(nm, tuple(s)) for nm, _, s in layout] == lr.light_layout(CFG)
    got = flat.cpu().numpy()
    Ks, Kd = _split(K)
    b = _fwd(rc, n, K)
    wn = {k: v for k, v in common.weights_material_np().items() if "LightSampler" in k}
    refs = {}
    for dt in (torch.float64, torch.float32):
        t = lambda a: torch.from_numpy(np.asarray(a)).to(dt)
        w = {k: t(v).requires_grad_(True) for k, v in wn.items()}
        pts = t(b["m_pts"]).reshape(n, 3)
        spec, diff = lr.split_samples(b["sec_dirs"], b["sec_samples"], b["sec_rgb"], b["m_nrm"], n, Ks, Kd, dt)
        vp = lr.vmf_params(w, CFG, pts)
        vm, kap, lg = lr.get_vmfs(vp, t(rnd["vmf_noise"]), pts, CFG.vmf_scale)
        loss = lr.light_sampling_loss(vm, kap, lg, spec, diff, t(lm))
        gs = torch.autograd.grad(loss, list(w.values()), allow_unused=True)
        refs[dt] = {k: (np.zeros(v.shape) if g is None else g.detach().double().numpy()) for (k, v), g in zip(w.items(), gs)}
    for name, off, shape in layout:
        size = int(np.prod(shape))
        g64 = refs[torch.float64][name].reshape(-1)
        g32 = refs[torch.float32][name].reshape(-1)
        lc.check(got[off: off + size], g64, g32, name)
    assert float(np.abs(got).max()) > 0


def test_semantics():
    rc = lc.make_material_rc()
    n, K = 777, 8
    rays, rnd = lc.material_case(n, K, seed=31)
    lm = lc.lossmult(n, seed=32)
    layout, total = rc.light_grad_layout()
    dense0 = [off for name, off, _ in layout if name.endswith("layers_0/kernel")][0]
    f1, l1 = rc.light_sampling_backward(rays, rnd, K, lossmult=lm)
    f1, l1 = f1.clone(), l1.clone()
    f2, l2 = rc.light_sampling_backward(rays, rnd, K, lossmult=lm)
    assert torch.equal(l1, l2)                                    # bitwise stable loss and dense gradients
    assert torch.equal(f1[dense0:], f2[dense0:])
    assert float(f1[:dense0].abs().max()) > 0 and float(f1[dense0:].abs().max()) > 0
    acc = torch.ones_like(f1)                                     # accumulates
    rc.light_sampling_backward(rays, rnd, K, lossmult=lm, grad=acc)
    assert torch.equal(acc[dense0:] - 1.0, (f1[dense0:] + 1.0) - 1.0)
    np.testing.assert_allclose(acc.cpu().numpy(), 1.0 + f1.cpu().numpy(), rtol=1e-5, atol=1e-6 * float(f1.abs().max()))
    fz, lz = rc.light_sampling_backward(rays, rnd, K, lossmult=lm, grad=False)   # NULL grads: the loss only
    assert fz is None and torch.equal(lz, l1)
    s = torch.cuda.Stream()                                       # a non-default stream
    with torch.cuda.stream(s):
        fs, ls = rc.light_sampling_backward(rays, rnd, K, lossmult=lm)
    s.synchronize()
    assert torch.equal(ls, l1) and torch.equal(fs[dense0:], f1[dense0:])
    # n = 0 writes nothing
    r, held, _ = rc._rays_struct(rays)
    rr, mr = rc._material_randoms(rnd, n, K, held)
    cfg = rc_ext.rc_light_sampling_loss(mult=1.0, linear_to_srgb=1)
    g0 = torch.zeros(total, device="cuda")
    out = torch.zeros(1, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    assert rc.lib.rc_light_sampling_backward(rc._h, C.byref(r), None, 0, C.byref(rr), C.byref(mr), K, C.byref(cfg),
                                             g0.data_ptr(), out.data_ptr(), stream) == 0
    assert rc.lib.rc_light_sampling_backward(rc._h, C.byref(r), None, n, C.byref(rr), C.byref(mr), K, C.byref(cfg),
                                             g0.data_ptr(), None, stream) == -1
    torch.cuda.synchronize()
    assert float(g0.abs().max()) == 0.0 and float(out.abs().max()) == 0.0
    # a handle without the light / material weights, and a time-resolved handle
    bare = rc_ext.RadianceCache(CFG, 0)
    bare.load_weights(common.weights_np())
    rb, heldb, _ = bare._rays_struct(rays)
    rrb, mrb = bare._material_randoms(rnd, n, K, heldb)
    assert bare.lib.rc_light_sampling_backward(bare._h, C.byref(rb), None, n, C.byref(rrb), C.byref(mrb), K, C.byref(cfg),
                                               None, out.data_ptr(), stream) == RC_ERR_MISSING_WEIGHT
    tr = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    tr.load_weights(common.weights_transient_np())
    r3, held3, _ = tr._rays_struct(rays)
    rr3, mr3 = tr._material_randoms(rnd, n, K, held3)
    assert tr.lib.rc_light_sampling_backward(tr._h, C.byref(r3), None, n, C.byref(rr3), C.byref(mr3), K, C.byref(cfg),
                                             None, out.data_ptr(), stream) == RC_ERR_UNSUPPORTED
    assert tr.lib.rc_light_regularizer(tr._h, 1.0, None, out.data_ptr(), stream) == RC_ERR_UNSUPPORTED
    del held, heldb, held3
    torch.cuda.synchronize()


def test_regularizer_against_numpy():
    rc = lc.make_material_rc()
    w = common.weights_material_np()
    layout, total = rc.light_grad_layout()
    flat, loss = rc.light_regularizer(0.7)
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    want = 0.0
    for name, off, shape in layout:
        size = int(np.prod(shape))
        if "light_grid" in name:
            x = np.asarray(w[name], np.float64).reshape(-1)
            want += 0.5 * np.mean(x * x)
            np.testing.assert_allclose(got[off: off + size], 0.7 * x / size, rtol=1e-6, atol=1e-30)
        else:
            assert float(np.abs(got[off: off + size]).max()) == 0.0, name
    assert float(loss[0]) == pytest.approx(0.7 * want, rel=1e-6)


def test_load_params_flat_light_renders_as_load_weights():
    w2 = lc.perturbed(common.weights_material_np(), "LightSampler", 5)
    a = lc.make_material_rc(w2)
    b = lc.make_material_rc()
    b.load_params_flat("light", lc.flat_from_layout(*b.light_grad_layout(), w2))
    ra, rb = lc.material_render(a, 8), lc.material_render(b, 8)
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k


START, LOOP_STEPS = 2500, 40


def test_training_loop_lowers_the_loss_and_resumes():
    rc = lc.make_material_rc()
    opt = train.LightSamplerOptimizer(rc)
    opt.init_from(common.weights_material_np(), count=START)
    n = 2048
    rays, rnd = lc.material_case(n, 8, seed=61)
    cfg = config.LightSamplingConfig()
    step = lambda: train.light_sampler_step(rc, opt, rays, rnd, cfg=cfg)
    # the state two steps back is resumed: the handle renders bitwise what it rendered then, and the run goes on
    lc.step_loop(step, lambda losses: float(losses["light_sampling"]), opt, START, LOOP_STEPS,
                 lambda totals: min(totals[-3:]) < totals[0], "light_sampler_step loop:", lambda t: round(t, 6),
                 render=lambda: lc.material_render(rc, 8))
    assert {train.param_group(k) for k in opt.names()} == {"LightSampler"}
