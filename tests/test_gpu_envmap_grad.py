"""rc_material_data_backward_env on the GPU: everything rc_material_data_backward computes stays
bitwise, every tensor of the EnvMap layout against the fp64 torch restatement (tests/envmap_grad_ref.py) at the call's own
trace, call semantics, rc_load_params_flat of the EnvMap layout, and material-stage training loops with the EnvMap."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import common
import envmap_grad_ref as eg
import loss_cases as lc
import material_data_loss_ref as md
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
def test_everything_of_the_old_call_is_bitwise(K):
    rc = lc.make_material_rc()
    n = 1500
    rays, rnd, gt = _case(n, K)
    lm = lc.lossmult(n)
    cfg = dataclasses.replace(config.MaterialDataLossConfig(), num_secondary_samples=K)
    f0, l0 = rc.material_data_backward(rays, rnd, gt, K, lossmult=lm, cfg=cfg)
    torch.cuda.synchronize()
    want = _fwd(rc, n, K)
    want.update({k: rc.workspace(k)[: 3 * n].copy() for k in ("md:rgb", "md:cache_rgb")})
    f0, l0 = f0.clone(), l0.clone()
    f1, e1, l1 = rc.material_data_backward(rays, rnd, gt, K, lossmult=lm, cfg=cfg, env_grad=True)
    torch.cuda.synchronize()
    got = _fwd(rc, n, K)
    got.update({k: rc.workspace(k)[: 3 * n].copy() for k in ("md:rgb", "md:cache_rgb")})
    for k in want:
        assert np.array_equal(want[k].view(np.uint32), got[k].view(np.uint32)), k
    assert torch.equal(l0, l1)
    layout, _ = rc.material_grad_layout()
    dense0 = [off for name, off, _ in layout if name.endswith("bottleneck_layer/kernel")][0]
    assert torch.equal(f0[dense0:], f1[dense0:])                  # the tables are scattered with atomics
    np.testing.assert_allclose(f1.cpu().numpy(), f0.cpu().numpy(), rtol=1e-5, atol=1e-6 * float(f0.abs().max()))
    assert float(e1.abs().max()) > 0


@pytest.mark.parametrize("n", [512, 3001, 4200])
def test_every_envmap_tensor_against_fp64_autograd(n):
    """At the call's own trace: every tensor of the EnvMap layout within 3x the fp32 restatement's distance from fp64
    (plus a 1e-6 relative floor).  3001 x 8 = 24 008 rows end inside a 128-row tile and inside a 1024-row K slice;
    4200 x 8 = 33 600 rows are two chunks (32 768 + 832).  Each case must have a gradient to find: the fp64 reference is
    non-zero on every tensor but the alpha column, and at least a quarter of the secondary rays have
    (1 - acc) * weight > 0; both are asserted here on the call's own trace buffers (sec_acc, sec_samples), not only on an
    oracle run beforehand.  Shares measured with these seeds on an MI355X: 0.5962 (n = 512), 0.5878 (3001), 0.5880 (4200);
    the smallest max|fp64 reference| of a tensor was 3.5e-05 (layer_0/kernel), the errors 1e-10 .. 2e-08."""
    K = 8
    rc = lc.make_material_rc()
    rays, rnd, gt = _case(n, K, seed=21)
    lm = lc.lossmult(n, seed=22)
    cres, mres = rc.render_material(rays, rnd, num_secondary_samples=K)
    S = CFG.sampling_strategy[-1][2]
    acc_p = rc.workspace("weights2")[: n * S].reshape(n, S).sum(-1)
    _, env_flat, loss = rc.material_data_backward(rays, rnd, gt, K, lossmult=lm, grad=False, env_grad=True)
    torch.cuda.synchronize()
    layout, total = rc.envmap_grad_layout()
    assert [(nm, tuple(s)) for nm, _, s in layout] == eg.envmap_layout(CFG)
    assert total == 175620
    got = env_flat.cpu().numpy()
    crgb = rc.workspace("md:cache_rgb")[: 3 * n].reshape(n, 3)
    fw = rc.workspace("filt_weight")[:n]
    f = _fwd(rc, n, K)
    Ks = Kd = K // 2
    wall = common.weights_material_np()
    wm = {k: v for k, v in wall.items() if "MaterialShader" in k}
    we = {k: v for k, v in wall.items() if k.startswith(eg.ENV)}
    refs = {}
    for dt in (torch.float64, torch.float32):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
        sm, rgb_in, acc_in, env_in = md.split_trace(n, Ks, Kd, t(f["sec_samples"]), t(f["sec_rgb"]), t(f["sec_acc"]),
                                                    t(f["sec_env"]))
        trace = (Ks, Kd, t(f["m_local_view"]).reshape(n, 3), sm, rgb_in, acc_in, env_in)
        w_m = {k: t(v) for k, v in wm.items()}
        w_e = {k: t(v).requires_grad_(True) for k, v in we.items()}
        ls, _ = eg.chain_loss(w_m, w_e, CFG, t(f["m_pts"]).reshape(n, 3), t(f["sec_dirs"]).reshape(-1, 3), trace, t(gt),
                              t(crgb), t(fw), t(acc_p), t(lm), bg=CFG.bg_intensity)
        gs = torch.autograd.grad(ls, list(w_e.values()), allow_unused=True)
        refs[dt] = {k: (np.zeros(v.shape) if g is None else g.detach().double().numpy()) for (k, v), g in zip(w_e.items(), gs)}
        if dt == torch.float64:
            wgt = torch.clamp(sm[..., 4], min=0.0) * (sm[..., 2] > 0)
            share = float((((1.0 - acc_in) * wgt) > 0).double().mean())
            print(f"n = {n}: share of secondary rays with (1 - acc) * weight > 0: {share:.4f}")
            assert share >= 0.25, share
    for name, off, shape in layout:
        size = int(np.prod(shape))
        r64, r32 = refs[torch.float64][name], refs[torch.float32][name]
        g = got[off: off + size].reshape(shape)
        if name.endswith("output_rgba_layer/kernel"):
            assert np.all(g[:, 3] == 0.0) and np.all(r64[:, 3] == 0.0)
            assert float(np.abs(r64[:, :3]).max()) > 0
        elif name.endswith("output_rgba_layer/bias"):
            assert g[3] == 0.0 and r64[3] == 0.0
            assert float(np.abs(r64[:3]).max()) > 0
        else:
            assert float(np.abs(r64).max()) > 0, name
        print(f"  {name}: max|ref64| {np.abs(r64).max():.3e} err {np.abs(g - r64).max():.3e} "
              f"err32 {np.abs(r32 - r64).max():.3e}")
        lc.check(g.reshape(-1), r64.reshape(-1), r32.reshape(-1), name)
    assert "params/Cache/EnvMap/output_ambient_rgb_layer/kernel" not in [nm for nm, _, _ in layout]


def test_semantics():
    K = 8
    rc = lc.make_material_rc()
    n = 777
    rays, rnd, gt = _case(n, K, seed=31)
    lm = lc.lossmult(n, seed=32)
    _, total = rc.envmap_grad_layout()
    layout_m, total_m = rc.material_grad_layout()
    dense0 = [off for name, off, _ in layout_m if name.endswith("bottleneck_layer/kernel")][0]
    f1, e1, l1 = rc.material_data_backward(rays, rnd, gt, K, lossmult=lm, env_grad=True)
    f1, e1, l1 = f1.clone(), e1.clone(), l1.clone()
    f2, e2, l2 = rc.material_data_backward(rays, rnd, gt, K, lossmult=lm, env_grad=True)
    assert torch.equal(l1, l2) and torch.equal(e1, e2) and torch.equal(f1[dense0:], f2[dense0:])   # bitwise repeat
    assert float(e1.abs().max()) > 0
    acc = torch.ones_like(e1)                                     # accumulates
    rc.material_data_backward(rays, rnd, gt, K, lossmult=lm, env_grad=acc)
    assert torch.equal(acc - 1.0, (e1 + 1.0) - 1.0)
    fz, ez, lz = rc.material_data_backward(rays, rnd, gt, K, lossmult=lm, grad=False, env_grad=True)   # material NULL
    assert fz is None and torch.equal(ez, e1) and torch.equal(lz, l1)
    fo, lo = rc.material_data_backward(rays, rnd, gt, K, lossmult=lm)                                # the old path
    assert torch.equal(lo, l1) and torch.equal(fo[dense0:], f1[dense0:])
    _, eh, lh = rc.material_data_backward(rays, rnd, gt, K, lossmult=lm, grad=False, env_grad=True, env_scale=0.5)
    assert torch.equal(lh, l1) and torch.equal(eh, 0.5 * e1)      # a power of two: exactly half, the loss unscaled
    s = torch.cuda.Stream()                                       # a non-default stream
    with torch.cuda.stream(s):
        fs, es, ls = rc.material_data_backward(rays, rnd, gt, K, lossmult=lm, env_grad=True)
    s.synchronize()
    assert torch.equal(ls, l1) and torch.equal(es, e1) and torch.equal(fs[dense0:], f1[dense0:])
    # raw calls: n = 0 writes nothing; both gradients NULL is the loss only; null loss / gt are refused
    r, held, _ = rc._rays_struct(rays)
    rr, mrd = rc._material_randoms(rnd, n, K, held)
    g_t, lm_t = torch.from_numpy(gt).cuda(), torch.from_numpy(lm).cuda()
    cfg = rc_ext.rc_material_data_loss(mult=1.0, weight=0.1, exponent=1.0, eps=1e-2, clip_val=1e4, thresh=1e6,
                                       use_gt_rawnerf=0, use_combined_rawnerf=1, use_norm_rawnerf=0)
    g0 = torch.zeros(total_m, device="cuda")
    ge = torch.zeros(total, device="cuda")
    out = torch.zeros(1, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    fn = rc.lib.rc_material_data_backward_env
    call = lambda h, rays_, gtp, nn, r_, m_, gm, gep, lp: fn(h, C.byref(rays_), gtp, lm_t.data_ptr(), nn, C.byref(r_), C.byref(m_), K,
                                                              C.byref(cfg), 1.0, gm, gep, lp, stream)
    assert call(rc._h, r, g_t.data_ptr(), 0, rr, mrd, g0.data_ptr(), ge.data_ptr(), out.data_ptr()) == 0
    torch.cuda.synchronize()
    assert float(g0.abs().max()) == 0.0 and float(ge.abs().max()) == 0.0 and float(out.abs().max()) == 0.0
    assert call(rc._h, r, g_t.data_ptr(), n, rr, mrd, None, None, out.data_ptr()) == 0
    torch.cuda.synchronize()
    assert float(ge.abs().max()) == 0.0 and torch.equal(out, l1)
    assert call(rc._h, r, g_t.data_ptr(), n, rr, mrd, None, ge.data_ptr(), None) == RC_ERR_INVALID_ARG
    assert call(rc._h, r, None, n, rr, mrd, None, ge.data_ptr(), out.data_ptr()) == RC_ERR_INVALID_ARG
    # a handle without the material weights, one without the EnvMap, and a time-resolved handle
    bare = rc_ext.RadianceCache(CFG, 0)
    bare.load_weights(common.weights_np())
    rb, heldb, _ = bare._rays_struct(rays)
    rrb, mrb = bare._material_randoms(rnd, n, K, heldb)
    assert call(bare._h, rb, g_t.data_ptr(), n, rrb, mrb, None, ge.data_ptr(), out.data_ptr()) == RC_ERR_MISSING_WEIGHT
    noenv = rc_ext.RadianceCache(CFG, 0)
    noenv.load_weights({k: v for k, v in common.weights_material_np().items() if not k.startswith(eg.ENV)})
    rn, heldn, _ = noenv._rays_struct(rays)
    rrn, mrn = noenv._material_randoms(rnd, n, K, heldn)
    assert call(noenv._h, rn, g_t.data_ptr(), n, rrn, mrn, None, ge.data_ptr(), out.data_ptr()) == RC_ERR_MISSING_WEIGHT
    tr = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    tr.load_weights(common.weights_transient_np())
    r3, held3, _ = tr._rays_struct(rays)
    rr3, mr3 = tr._material_randoms(rnd, n, K, held3)
    assert call(tr._h, r3, g_t.data_ptr(), n, rr3, mr3, None, ge.data_ptr(), out.data_ptr()) == RC_ERR_UNSUPPORTED
    assert float(ge.abs().max()) == 0.0
    del held, heldb, heldn, held3
    torch.cuda.synchronize()


def test_load_params_flat_envmap_renders_as_load_weights():
    """rc_load_params_flat(RC_LAYOUT_ENVMAP) of perturbed EnvMap tensors: the secondary-ray pass's EnvMap radiance and the
    material stage's outputs are bitwise those after load_weights of the same tensors."""
    w = lc.perturbed(common.weights_material_np(), "Cache/EnvMap", seed=77)
    ref = lc.make_material_rc(weights=w)
    want = lc.material_render(ref, 8)
    torch.cuda.synchronize()
    want_env = ref.workspace("sec_env")[: 3 * 1024 * 8].copy()
    rc = lc.make_material_rc()
    before = lc.material_render(rc, 8)
    assert not torch.equal(before["m_rgb"], want["m_rgb"])
    layout, total = rc.envmap_grad_layout()
    rc.load_params_flat("envmap", lc.flat_from_layout(layout, total, w))
    got = lc.material_render(rc, 8)
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(want[k], got[k]), k
    assert np.array_equal(want_env.view(np.uint32), rc.workspace("sec_env")[: 3 * 1024 * 8].view(np.uint32))
    rc.load_params_flat(rc_ext.RC_LAYOUT_ENVMAP, lc.flat_from_layout(layout, total, common.weights_material_np()))
    again = lc.material_render(rc, 8)
    for k in before:
        assert torch.equal(before[k], again[k]), k


LOOP_STEPS = 40


def test_envmap_loops_lower_the_data_loss_and_resume():
    """material_env_stage_step on a fixed batch at the material-stage schedule (OptimizerConfig(material=True)): (1) only
    the EnvMap optimizer steps: the data loss falls, and a state-dict resume is bitwise; (2) both optimizers step: the
    data loss ends below material_stage_step's (MaterialShader alone) on the same batch and step count.  The
    trajectories are printed; no drop ratio is asserted."""
    n = 2048
    rays, rnd, gt = _case(n, 8, seed=61)
    noise = lc.normal_noise(n, 62)
    ocfg = config.OptimizerConfig(material=True)
    data = lambda losses: float(losses["data"])
    fmt = lambda t: f"{t:.6e}"

    def each(losses):
        assert set(losses) == {"data", "material_smoothness", "regularizer/material_grid", "material_ray_sampler"}

    def fresh():
        rc = lc.make_material_rc()
        om, oe = train.MaterialOptimizer(rc, ocfg), train.EnvMapOptimizer(rc, ocfg)
        om.init_from(common.weights_material_np(), count=0)
        oe.init_from(common.weights_material_np(), count=0)
        return rc, om, oe

    rc, om, oe = fresh()
    m0 = om.params["material"].clone()
    step = lambda: train.material_env_stage_step(rc, om, oe, rays, rnd, gt, noise, step_material=False)
    lc.step_loop(step, data, oe, 0, LOOP_STEPS, lambda totals: min(totals[-3:]) < totals[0],
                 "material_env_stage_step loop, EnvMap only (data):", fmt, each=each,
                 render=lambda: lc.material_render(rc, 8))
    assert om.count == 0 and torch.equal(om.params["material"], m0)

    rc, om, oe = fresh()
    step = lambda: train.material_env_stage_step(rc, om, oe, rays, rnd, gt, noise)
    both = lc.step_loop(step, data, oe, 0, LOOP_STEPS, lambda totals: min(totals[-3:]) < totals[0],
                        "material_env_stage_step loop, both (data):", fmt, each=each)
    assert om.count == LOOP_STEPS

    rc, om, _ = fresh()
    step = lambda: train.material_stage_step(rc, om, rays, rnd, gt, noise)
    alone = lc.step_loop(step, data, om, 0, LOOP_STEPS, lambda totals: True, "material_stage_step loop (data):", fmt)
    assert both[-1] < alone[-1], (both[-1], alone[-1])
