"""rc_light_sampling_backward and rc_light_regularizer on the GPU: the forward against rc_render_material, the loss kernel
and the whole chain against the fp64 torch restatement (tests/light_sampling_ref.py), call semantics, the regularizer, the
light-layout refresh and a training loop."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import common
import light_sampling_ref as lr
import nrc_amd
from nrc_amd import config, rc_ext, train
from oracle import material_ref

CFG = nrc_amd.hotdog_config()
RC_ERR_UNSUPPORTED, RC_ERR_MISSING_WEIGHT = -5, -3
FWD = ("m_pts", "m_nrm", "l_vmf", "l_vmf_logit", "sec_dirs", "sec_samples", "sec_rgb")

pytestmark = pytest.mark.gpu


def _rc(weights=None):
    return common.make_rc(weights=weights if weights is not None else common.weights_material_np())


def _case(n, K=8, seed=3):
    rays = nrc_amd.synthetic_rays(n, seed=seed).hot_fields()
    rnd = material_ref.draw_randoms(dataclasses.replace(CFG, num_secondary_samples=K), n, seed=seed + 1)
    return rays, rnd


def _split(K):
    Kd = int(round(K * CFG.diffuse_sample_fraction))
    return K - Kd, Kd


def _lossmult(n, seed=9):
    rng = np.random.Generator(np.random.PCG64(seed))
    lm = rng.uniform(0.5, 2.0, size=n).astype(np.float32)
    lm[::7] = 0.0
    return lm


def _fwd(rc, n, K):
    Ks, Kd = _split(K)
    nsec = n * K
    sizes = dict(m_pts=3 * n, m_nrm=3 * n, l_vmf=640 * n, l_vmf_logit=128 * n, sec_dirs=3 * nsec, sec_samples=5 * nsec,
                 sec_rgb=3 * nsec)
    return {k: rc.workspace(k)[:v].copy() for k, v in sizes.items()}


@pytest.mark.parametrize("K", [8, 32])
def test_forward_is_bitwise_render_material(K):
    rc = _rc()
    n = 1500
    rays, rnd = _case(n, K)
    rc.render_material(rays, rnd, K)
    want = _fwd(rc, n, K)
    rc.light_sampling_backward(rays, rnd, K, lossmult=_lossmult(n))
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


def _check(got, ref64, ref32, what, rel_floor=1e-6):
    err, err32 = float(np.abs(got - ref64).max()), float(np.abs(ref32 - ref64).max())
    bound = 3.0 * err32 + rel_floor * float(np.abs(ref64).max()) + 1e-12
    assert err <= bound, (what, err, err32, bound)


def test_loss_kernel_against_restatement():
    """The loss and d loss / d vmf_params on the forward's own buffers, within 3x the fp32 restatement's distance from
    fp64 (plus a 1e-6 relative floor)."""
    rc = _rc()
    n, K = 1024, 8
    rays, rnd = _case(n, K, seed=11)
    lm = _lossmult(n)
    _, loss = rc.light_sampling_backward(rays, rnd, K, lossmult=lm)
    torch.cuda.synchronize()
    dvp = rc.workspace("ls:dvp")[: 640 * n].reshape(n, 640)
    l64, g64 = _restated(rc, n, K, rnd, lm, torch.float64)
    l32, g32 = _restated(rc, n, K, rnd, lm, torch.float32)
    assert l64 > 0 and float(np.abs(g64).max()) > 0
    _check(np.array([float(loss[0])]), np.array([l64]), np.array([l32]), "loss")
    _check(dvp, g64, g32, "d vmf_params")


def test_whole_chain_against_fp64_autograd():
    rc = _rc()
    n, K = 512, 8
    rays, rnd = _case(n, K, seed=21)
    lm = _lossmult(n, seed=22)
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
        _check(got[off: off + size], g64, g32, name)
    assert float(np.abs(got).max()) > 0


def test_semantics():
    rc = _rc()
    n, K = 777, 8
    rays, rnd = _case(n, K, seed=31)
    lm = _lossmult(n, seed=32)
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
    rc = _rc()
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


def _perturbed_light(seed=5):
    w = dict(common.weights_material_np())
    rng = np.random.Generator(np.random.PCG64(seed))
    for k in list(w):
        if "LightSampler" in k:
            w[k] = (np.asarray(w[k]) * (1.0 + 0.05 * rng.standard_normal(np.shape(w[k])))).astype(np.float32)
    return w


def _material_render(rc, n=1024, K=8):
    rays, rnd = _case(n, K, seed=51)
    cres, mres = rc.render_material(rays, rnd, K)
    return {**{"c_" + k: v.clone() for k, v in cres.items()}, **{"m_" + k: v.clone() for k, v in mres.items()}}


def test_load_params_flat_light_renders_as_load_weights():
    w2 = _perturbed_light()
    a = _rc(w2)
    b = _rc()
    layout, total = b.light_grad_layout()
    flat = torch.empty(total, dtype=torch.float32, device="cuda")
    for name, off, shape in layout:
        flat[off: off + int(np.prod(shape))] = torch.from_numpy(np.ascontiguousarray(w2[name], np.float32)).reshape(-1)
    b.load_params_flat("light", flat)
    ra, rb = _material_render(a), _material_render(b)
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k


START, LOOP_STEPS = 2500, 40


def test_training_loop_lowers_the_loss_and_resumes():
    rc = _rc()
    opt = train.LightSamplerOptimizer(rc)
    opt.init_from(common.weights_material_np(), count=START)
    n = 2048
    rays, rnd = _case(n, 8, seed=61)
    cfg = config.LightSamplingConfig()
    totals = []
    for i in range(LOOP_STEPS):
        if i == LOOP_STEPS - 2:
            sd, r_sd = opt.state_dict(), _material_render(rc)
        losses = train.light_sampler_step(rc, opt, rays, rnd, cfg=cfg)
        totals.append(float(losses["light_sampling"]))
    print("light_sampler_step loop:", [round(t, 6) for t in totals])
    assert opt.count == START + LOOP_STEPS
    assert all(np.isfinite(totals))
    assert min(totals[-3:]) < totals[0], totals
    assert {train.param_group(k) for k in opt.names()} == {"LightSampler"}
    # resume from the state two steps back: the handle renders bitwise what it rendered then, and the run goes on
    opt.load_state_dict(sd)
    assert opt.count == START + LOOP_STEPS - 2
    r_again = _material_render(rc)
    for k in r_sd:
        assert torch.equal(r_sd[k], r_again[k]), k
    for _ in range(2):
        losses = train.light_sampler_step(rc, opt, rays, rnd, cfg=cfg)
    assert opt.count == START + LOOP_STEPS
    assert float(losses["light_sampling"]) == pytest.approx(totals[-1], rel=1e-3)
