"""The EnvMap's gradient of the material stage's data loss without a GPU: the torch restatement
(tests/envmap_grad_ref.py) against fp64 central differences on every EnvMap tensor, the exact zeros (alpha column,
output_ambient_rgb_layer), the factors of the chain (1 - acc, the clip tie, env_scale on the gradient only), the
MaterialShader gradient left as material_data_loss_ref.chain_loss gives it, the optimizer group and the layout."""
import numpy as np
import pytest
import torch

import common
import envmap_grad_ref as eg
import material_data_loss_ref as md
import nrc_amd
from nrc_amd import config, rc_ext, train

CFG = nrc_amd.hotdog_config()
D = torch.float64
KS, KD = 4, 4


def _weights(dtype=D):
    w = common.weights_material_np()
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dtype)
    return ({k: t(v) for k, v in w.items() if "MaterialShader" in k},
            {k: t(v) for k, v in w.items() if k.startswith(eg.ENV)})


def _case(n=5, seed=0, dtype=D):
    """A synthetic trace in k_brdf_sample's layout and everything else chain_loss reads."""
    g = torch.Generator().manual_seed(seed)
    K = KS + KD
    d = torch.randn(n, K, 3, generator=g, dtype=dtype)
    d[..., 2] = d[..., 2].abs() + 0.1
    d = d / d.norm(dim=-1, keepdim=True)
    sm = torch.cat([d, 0.2 + torch.rand(n, K, 1, generator=g, dtype=dtype), 0.5 + torch.rand(n, K, 1, generator=g, dtype=dtype)], -1)
    wo = torch.randn(n, 3, generator=g, dtype=dtype)
    wo[:, 2] = wo[:, 2].abs() + 0.2
    wo = wo / wo.norm(dim=-1, keepdim=True)
    rgb_in = torch.rand(n, K, 3, generator=g, dtype=dtype) * 2.0
    acc_in = torch.rand(n, K, generator=g, dtype=dtype)
    sec = torch.randn(n * K, 3, generator=g, dtype=dtype)
    sec = sec / sec.norm(dim=-1, keepdim=True)
    pts = torch.rand(n, 3, generator=g, dtype=dtype) - 0.5
    gt = 0.05 + torch.rand(n, 3, generator=g, dtype=dtype)
    crgb = 0.05 + torch.rand(n, 3, generator=g, dtype=dtype)
    w = 0.3 + torch.rand(n, generator=g, dtype=dtype)
    acc_p = torch.rand(n, generator=g, dtype=dtype)
    lm = 0.5 + torch.rand(n, generator=g, dtype=dtype)
    return dict(pts=pts, sec_dirs=sec, trace=(KS, KD, wo, sm, rgb_in, acc_in, None), gt=gt, cache_rgb=crgb, w=w,
                acc_p=acc_p, lossmult=lm)


def _loss(wm, we, case, **kw):
    return eg.chain_loss(wm, we, CFG, **case, **kw)[0]


def _env_grads(wm, we, case, **kw):
    we = {k: v.clone().requires_grad_(True) for k, v in we.items()}
    gs = torch.autograd.grad(_loss(wm, we, case, **kw), list(we.values()), allow_unused=True)
    return {k: (torch.zeros_like(v) if g is None else g) for (k, v), g in zip(we.items(), gs)}


def test_restatement_against_central_differences_on_every_tensor():
    """The loss's VALUE has twice the gradient's derivative (2 d sg(d)), so the differences are taken on the surrogate
    sum(g_rgb * rgb) with g_rgb = d loss / d rgb held fixed."""
    wm, we = _weights()
    case = _case(n=6, seed=1)
    grads = _env_grads(wm, we, case)
    rgb0 = eg.chain_loss(wm, we, CFG, **case)[1].detach().requires_grad_(True)
    (g_rgb,) = torch.autograd.grad(md.data_loss(rgb0, case["gt"], case["cache_rgb"], case["lossmult"]), rgb0)
    surrogate = lambda w_: float((g_rgb * eg.chain_loss(wm, w_, CFG, **case)[1]).sum())
    scale = float((g_rgb.abs() * rgb0.detach().abs()).sum())
    rng = np.random.Generator(np.random.PCG64(5))
    for name, shape in eg.envmap_layout(CFG):
        g = grads[name]
        assert tuple(g.shape) == shape
        if name.endswith("output_rgba_layer/kernel"):
            assert float(g[:, 3].abs().max()) == 0.0                 # alpha: exact zeros
            cols = 3
        elif name.endswith("output_rgba_layer/bias"):
            assert float(g[3]) == 0.0
            cols = 3
        else:
            cols = shape[-1]
        assert float(g.abs().max()) > 0, name
        flat = we[name].reshape(-1)
        # the largest entry and a few random ones (outside the alpha column)
        idx = [int(g.abs().reshape(-1).argmax())] + [int(i) for i in rng.integers(0, flat.numel(), 4)]
        for i in idx:
            if name.endswith("output_rgba_layer/kernel") and i % 4 >= cols:
                continue
            if name.endswith("output_rgba_layer/bias") and i >= cols:
                continue
            # step 1e-5: small enough that no ReLU of the few rows changes side, and the roundoff of the difference,
            # ~1e-16 sum|g_rgb rgb| / h, stays below the absolute bound
            h = 1e-5 * max(1.0, abs(float(flat[i])))
            vals = []
            for s in (+1, -1):
                w_ = dict(we)
                p = we[name].clone().reshape(-1)
                p[i] += s * h
                w_[name] = p.reshape(shape)
                vals.append(surrogate(w_))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert fd == pytest.approx(float(g.reshape(-1)[i]), rel=1e-5, abs=1e-15 * scale / h), (name, i)


def test_ambient_layer_gets_nothing():
    wm, we = _weights()
    w = common.weights_material_np()
    extra = {k: torch.from_numpy(np.ascontiguousarray(v)).to(D) for k, v in w.items() if "Cache/EnvMap/output_ambient" in k}
    assert len(extra) == 2
    grads = _env_grads(wm, {**we, **extra}, _case(seed=2))
    for k in extra:
        assert float(grads[k].abs().max()) == 0.0
    assert all("output_ambient" not in nm for nm, _ in eg.envmap_layout(CFG))


def test_opaque_secondary_ray_contributes_nothing():
    """acc = 1 on every secondary ray of one point: that point's rays add nothing; with acc = 1 everywhere the gradient
    is an exact zero."""
    wm, we = _weights()
    case = _case(seed=3)
    Ks, Kd, wo, sm, rgb_in, acc_in, _ = case["trace"]
    full = dict(case, trace=(Ks, Kd, wo, sm, rgb_in, torch.ones_like(acc_in), None))
    assert all(float(g.abs().max()) == 0.0 for g in _env_grads(wm, we, full).values())
    # acc = 1 on the rays of point 2 only: the gradient is the one with that point's lossmult zeroed instead (its own
    # rgb changes with acc, but rgb enters the other points' terms nowhere)
    acc1 = acc_in.clone()
    acc1[2] = 1.0
    lm = case["lossmult"].clone()
    lm[2] = 0.0
    a = _env_grads(wm, we, dict(case, trace=(Ks, Kd, wo, sm, rgb_in, acc1, None)))
    b = _env_grads(wm, we, dict(case, lossmult=lm))
    for k, _ in eg.envmap_layout(CFG):
        assert float(b[k].abs().max()) > 0, k
        torch.testing.assert_close(a[k], b[k], rtol=1e-12, atol=1e-18)


def test_clip_tie_passes_half():
    """ein * lobe exactly at rgb_max: jnp.clip passes half of the gradient there (and all of it below)."""
    n, K = 2, KS + KD
    env = torch.full((n, K, 3), 0.5, dtype=D, requires_grad=True)
    case = _case(n=n, seed=4)
    Ks, Kd, wo, sm, rgb_in, acc_in, _ = case["trace"]
    alb = torch.full((n, 3), 0.6, dtype=D)
    rough, metal = torch.full((n,), 0.5, dtype=D), torch.full((n,), 0.2, dtype=D)
    acc0 = torch.zeros_like(acc_in)
    free = eg.integrate(alb, rough, metal, Ks, Kd, wo, sm, rgb_in, acc0, env)
    (g_free,) = torch.autograd.grad(free.sum(), env)
    # rgb_max = the value of ein * lobe at one element: find the lobe from the free gradient (d / d env = lobe wd / K)
    env2 = env.detach().clone().requires_grad_(True)
    lobe_wd = g_free[0, Ks, 0] * Kd                                # diffuse lane, channel 0 of point 0
    wd = (torch.clamp(sm[0, Ks, 4], min=0.0) / torch.clamp(sm[0, Ks, 3], min=md.DENOM_EPS))
    lobe = lobe_wd / wd
    rgb_max = float(0.5 * lobe)
    tied = eg.integrate(alb, rough, metal, Ks, Kd, wo, sm, rgb_in, acc0, env2, rgb_max=rgb_max)
    (g_tied,) = torch.autograd.grad(tied.sum(), env2)
    assert float(env2.detach()[0, Ks, 0] * lobe) == rgb_max
    assert float(g_tied[0, Ks, 0]) == pytest.approx(0.5 * float(g_free[0, Ks, 0]), rel=1e-12)


def test_env_scale_scales_the_gradient_and_not_the_loss():
    wm, we = _weights()
    case = _case(seed=5)
    l1, l2 = float(_loss(wm, we, case)), float(_loss(wm, we, case, env_scale=0.25))
    assert l1 == l2
    g1, g2 = _env_grads(wm, we, case), _env_grads(wm, we, case, env_scale=0.25)
    for k in g1:
        torch.testing.assert_close(g2[k], 0.25 * g1[k], rtol=1e-12, atol=0)
    assert config.MaterialDataLossConfig().env_map_grad_weight == 1.0


def test_material_gradient_is_the_old_chain_loss():
    """With the lobe attached, the MaterialShader tensors get exactly material_data_loss_ref.chain_loss's gradient at the
    EnvMap's own radiance: nothing reaches them through env."""
    wm, we = _weights()
    case = _case(seed=6)
    Ks, Kd, wo, sm, rgb_in, acc_in, _ = case["trace"]
    n = case["pts"].shape[0]
    w1 = {k: v.clone().requires_grad_(True) for k, v in wm.items()}
    l_new = eg.chain_loss(w1, we, CFG, **case, material_grad=True)[0]
    g_new = torch.autograd.grad(l_new, list(w1.values()), allow_unused=True)
    env_in = eg.env_radiance(we, CFG, case["sec_dirs"], n, Ks, Kd).detach()
    w2 = {k: v.clone().requires_grad_(True) for k, v in wm.items()}
    l_old = md.chain_loss(w2, CFG, case["pts"], (Ks, Kd, wo, sm, rgb_in, acc_in, env_in), case["gt"], case["cache_rgb"],
                          case["w"], case["acc_p"], case["lossmult"])[0]
    g_old = torch.autograd.grad(l_old, list(w2.values()), allow_unused=True)
    assert float(l_new) == pytest.approx(float(l_old), rel=1e-14)
    for k, a, b in zip(w1, g_new, g_old):
        assert (a is None) == (b is None), k
        if a is not None:
            torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-20)


def test_optimizer_group_and_layout():
    assert train.param_group("params/Cache/EnvMap/layer_0/kernel") == "EnvMap"
    assert train.param_group("params/Cache/EnvMap/output_rgba_layer/bias", config.OptimizerConfig(material=True)) == "EnvMap"
    assert train.param_group("params/Cache/Shader/bottleneck_layer/kernel") != "EnvMap"
    lay = eg.envmap_layout(CFG)
    assert len(lay) == 10 and sum(int(np.prod(s)) for _, s in lay) == 175620
    w = common.weights_material_np()
    for name, shape in lay:
        assert tuple(w[name].shape) == shape, name
    assert rc_ext.RC_LAYOUT_ENVMAP == -4 and rc_ext._GRAD_LAYOUTS["envmap"][2] == -4
    assert issubclass(train.EnvMapOptimizer, train.CacheStageOptimizer)
    with pytest.raises(NotImplementedError):
        train.EnvMapOptimizer(None, config.OptimizerConfig(grad_max_norm=1.0))
