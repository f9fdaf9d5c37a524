"""The material stage's data loss without a GPU: the torch restatement (tests/material_data_loss_ref.py) against the
reference's expression as loops, finite differences on every MaterialShader tensor, the JAX rules (clip ties, max ties,
nan_to_num, the 2 d sg(d) factor, the stop-gradient on s), the per-ray-and-channel scale s, lossmult / thresh, the
trace's tensors as constants and MaterialDataLossConfig."""
import dataclasses

import numpy as np
import pytest
import torch

import loss_cases as lc
import material_data_loss_ref as md
import nrc_amd
from nrc_amd import config, train

CFG = nrc_amd.hotdog_config()
D = torch.float64
KS, KD = 4, 4


def _loss_case(n=6, seed=0):
    g = torch.Generator().manual_seed(seed)
    rgb = (0.05 + torch.rand(n, 3, generator=g, dtype=D)).requires_grad_(True)
    gt = 0.05 + torch.rand(n, 3, generator=g, dtype=D)
    c = 0.05 + torch.rand(n, 3, generator=g, dtype=D)
    lm = 0.5 + torch.rand(n, generator=g, dtype=D)
    return rgb, gt, c, lm


def _trace(n, seed=0, dtype=D):
    """A synthetic trace in k_brdf_sample's layout: upper-hemisphere directions, positive pdf / weight, radiance."""
    g = torch.Generator().manual_seed(seed)
    K = KS + KD
    d = torch.randn(n, K, 3, generator=g, dtype=dtype)
    d[..., 2] = d[..., 2].abs() + 0.1
    d = d / d.norm(dim=-1, keepdim=True)
    pdf = 0.2 + torch.rand(n, K, 1, generator=g, dtype=dtype)
    wgt = 0.5 + torch.rand(n, K, 1, generator=g, dtype=dtype)
    sm = torch.cat([d, pdf, wgt], -1)
    wo = torch.randn(n, 3, generator=g, dtype=dtype)
    wo[:, 2] = wo[:, 2].abs() + 0.2
    wo = wo / wo.norm(dim=-1, keepdim=True)
    rgb_in = torch.rand(n, K, 3, generator=g, dtype=dtype) * 2.0
    acc_in = torch.rand(n, K, generator=g, dtype=dtype)
    env_in = torch.rand(n, K, 3, generator=g, dtype=dtype)
    return (KS, KD, wo, sm, rgb_in, acc_in, env_in)


def test_restatement_equals_the_loop_form():
    rgb, gt, c, lm = _loss_case(n=7, seed=1)
    gt[2, 1] = 2e6                                   # above loss_thresh: its lossmult is zeroed
    c[3, 0] = -0.5                                   # clipped at 0, then max with gt
    for lmult in (None, lm):
        got = float(md.data_loss(rgb, gt, c, lmult, weight=0.1, mult=1.0, exponent=1.0, eps=1e-2))
        want = md.loop_loss(rgb.detach().numpy(), gt.numpy(), c.numpy(), None if lmult is None else lmult.numpy())
        assert got == pytest.approx(want, rel=1e-13)


@pytest.mark.parametrize("name", list(lc.MATERIAL_SETTINGS))
def test_restatement_equals_the_loop_form_at_the_settings(name):
    """data_loss against the loops at every non-default setting test_gpu_loss_settings runs on the device: the torch
    restatement is the oracle of branches only it implements, the loops are its second opinion."""
    rgb, gt, c, lm = _loss_case(n=7, seed=1)
    c[3, 0] = -0.5                                   # clipped at 0
    c[4, 1] = 0.9                                    # above clip_val = 0.5 and above gt
    kw = lc.material_loss_kw(dataclasses.replace(config.MaterialDataLossConfig(), **lc.MATERIAL_SETTINGS[name]))
    assert (gt > 0.8).any() and (gt > 0.5).any() and (c > gt).any() and (c < gt).any()
    default = md.loop_loss(rgb.detach().numpy(), gt.numpy(), c.numpy(), lm.numpy())
    for lmult in (None, lm):
        got = float(md.data_loss(rgb, gt, c, lmult, **kw))
        want = md.loop_loss(rgb.detach().numpy(), gt.numpy(), c.numpy(), None if lmult is None else lmult.numpy(), **kw)
        assert got == pytest.approx(want, rel=1e-12)
    assert want != pytest.approx(default, rel=1e-3)


def test_gradient_is_half_the_derivative_of_the_value():
    """2 (rgb - gt) sg(rgb - gt): d loss / d rgb = 2 sg(d) s lossmult, half of the value's derivative 4 d s lossmult."""
    rgb, gt, c, lm = _loss_case(seed=2)
    loss = md.data_loss(rgb, gt, c, lm)
    (g,) = torch.autograd.grad(loss, rgb)
    s = 1.0 / (torch.maximum(c.clamp(0, 1e4), gt) + 1e-2)
    want = 0.1 * lm[:, None] * 2.0 * (rgb - gt).detach() * s / rgb.numel()
    torch.testing.assert_close(g, want, rtol=1e-13, atol=0)
    eps = 1e-6                                       # finite difference of the VALUE: twice the gradient
    i = (1, 2)
    rp, rm = rgb.detach().clone(), rgb.detach().clone()
    rp[i] += eps
    rm[i] -= eps
    fd = (float(md.data_loss(rp, gt, c, lm)) - float(md.data_loss(rm, gt, c, lm))) / (2 * eps)
    assert fd == pytest.approx(2.0 * float(g[i]), rel=1e-6)


def test_s_is_stop_gradiented_and_per_ray_and_channel():
    """s carries no gradient to cache_rgb (nor to gt); scaling one ray's cache_rgb changes that ray's terms only:
    compute_unbiased_loss_rawnerf has no batch sum (the .sum(-2) of compute_unbiased_loss_rawnerf_transient belongs to
    the transient data loss, which hotdog does not use)."""
    rgb, gt, c, lm = _loss_case(n=5, seed=3)
    c = c.clone().requires_grad_(True)
    gtg = gt.clone().requires_grad_(True)
    loss = md.data_loss(rgb, gtg, c, lm)
    gc, = torch.autograd.grad(loss, c, retain_graph=True, allow_unused=True)
    assert gc is None or float(gc.abs().max()) == 0.0
    gc2 = torch.autograd.grad(loss, gtg)[0]
    assert torch.isfinite(gc2).all()                  # gt gets the (rgb - gt) path only

    def terms(cc):
        s = 1.0 / (md.rgb_clip(cc, gt) + 1e-2)
        d = (rgb - gt).detach()
        return lm[:, None] * 2.0 * d * d * s
    c0 = c.detach().clone()
    c1 = c0.clone()
    c1[2] *= 5.0
    t0, t1 = terms(c0), terms(c1)
    changed = (t0 != t1).any(dim=1)
    assert changed.tolist() == [False, False, True, False, False]


def test_clip_ties_pass_half():
    x = torch.tensor([0.0, 0.5, 1e4, -1.0, 2e4], dtype=D, requires_grad=True)
    y = md.jclip(x, 0.0, 1e4)
    (g,) = torch.autograd.grad(y.sum(), x)
    assert g.tolist() == [0.5, 1.0, 0.5, 0.0, 0.0]


def test_max_ties_split_and_nan_to_num_passes():
    u = torch.tensor([1.0, 2.0, 3.0], dtype=D, requires_grad=True)
    v = torch.tensor([1.0, 1.0, 4.0], dtype=D, requires_grad=True)
    gu, gv = torch.autograd.grad(md.jmaximum(u, v).sum(), (u, v))
    assert gu.tolist() == [0.5, 1.0, 0.0] and gv.tolist() == [0.5, 0.0, 1.0]
    x = torch.tensor([0.3, float("nan"), float("inf")], dtype=D, requires_grad=True)
    (gx,) = torch.autograd.grad((md.nan_to_num(x) * torch.tensor([2.0, 0.0, 0.0], dtype=D)).sum(), x)
    assert gx[0] == 2.0
    # the RC_EPS floor of Smith G at a tie: roughness a with n (1 - a/2) + a/2 == EPS is not reachable with n >= 0 and
    # a > 0, so the split is checked on the floor expression itself
    a = torch.tensor([md.EPS], dtype=D, requires_grad=True)
    (ga,) = torch.autograd.grad(md.jmaximum(torch.full_like(a, md.EPS), a).sum(), a)
    assert float(ga) == 0.5


def test_trace_tensors_are_constants():
    n = 5
    trace = tuple(t.clone().requires_grad_(True) if isinstance(t, torch.Tensor) else t for t in _trace(n, seed=4))
    g = torch.Generator().manual_seed(5)
    albedo = (0.1 + 0.8 * torch.rand(n, 3, generator=g, dtype=D)).requires_grad_(True)
    rough = (0.1 + 0.8 * torch.rand(n, generator=g, dtype=D)).requires_grad_(True)
    metal = (0.1 + 0.8 * torch.rand(n, generator=g, dtype=D)).requires_grad_(True)
    sh = md.integrate(albedo, rough, metal, *trace)
    loss = md.data_loss(sh, torch.rand(n, 3, generator=g, dtype=D), torch.rand(n, 3, generator=g, dtype=D))
    leaves = [trace[2], trace[3], trace[4], trace[5], trace[6]]     # wo, samples (dirs, pdf, weight), radiance, acc, env
    gs = torch.autograd.grad(loss, leaves + [albedo, rough, metal], allow_unused=True)
    for gg in gs[:5]:
        assert gg is None or float(gg.abs().max()) == 0.0
    for gg in gs[5:]:
        assert float(gg.abs().max()) > 0.0


def test_lossmult_and_thresh():
    rgb, gt, c, lm = _loss_case(n=4, seed=6)
    lm0 = torch.zeros_like(lm)
    assert float(md.data_loss(rgb, gt, c, lm0)) == 0.0
    gt2 = gt.clone()
    gt2[1, 0] = 5e6
    (g,) = torch.autograd.grad(md.data_loss(rgb, gt2, c, lm), rgb)
    assert float(g[1, 0]) == 0.0 and float(g[1, 1]) != 0.0
    two = float(md.data_loss(rgb, gt, c, 2.0 * lm))
    assert two == pytest.approx(2.0 * float(md.data_loss(rgb, gt, c, lm)), rel=1e-14)


@pytest.fixture(scope="module")
def material_weights():
    w = nrc_amd.synthetic_weights(CFG, passes=("cache", "material"), seed=4)
    return {k: torch.from_numpy(np.asarray(v)).to(D) for k, v in w.items() if "MaterialShader" in k}


def test_finite_differences_on_every_material_tensor(material_weights):
    n = 6
    g = torch.Generator().manual_seed(7)
    pts = (torch.rand(n, 3, generator=g, dtype=D) - 0.5) * 1.5
    trace = _trace(n, seed=8)
    gt = torch.rand(n, 3, generator=g, dtype=D)
    c = torch.rand(n, 3, generator=g, dtype=D)
    w = 0.3 + 0.7 * torch.rand(n, generator=g, dtype=D)
    acc = 0.5 + 0.5 * torch.rand(n, generator=g, dtype=D)
    lm = 0.5 + torch.rand(n, generator=g, dtype=D)
    wts = {k: v.clone().requires_grad_(True) for k, v in material_weights.items()}
    loss, _ = md.chain_loss(wts, CFG, pts, trace, gt, c, w, acc, lm)
    grads = dict(zip(wts, torch.autograd.grad(loss, list(wts.values()), allow_unused=True)))

    def value(name, idx, delta):
        w2 = {k: v.detach().clone() for k, v in wts.items()}
        w2[name].view(-1)[idx] += delta
        rgb = md.chain_loss(w2, CFG, pts, trace, gt, c, w, acc, lm)[1]
        d = (rgb - gt)
        s = 1.0 / (md.rgb_clip(c, gt) + 1e-2)
        return float(0.1 * (lm[:, None] * d * d * s * 2.0).mean())
    checked = 0
    for name, gr in grads.items():
        assert gr is not None, name
        flat = gr.reshape(-1)
        idx = [int(i) for i in torch.argsort(flat.abs(), descending=True)[:2]]
        for i in idx:
            if float(flat[i]) == 0.0:
                continue
            h = 1e-6 * max(1.0, abs(float(wts[name].reshape(-1)[i])))
            fd = (value(name, i, h) - value(name, i, -h)) / (2 * h)
            # the gradient of 2 d sg(d) is half the value's derivative
            assert 0.5 * fd == pytest.approx(float(flat[i]), rel=2e-5, abs=1e-13), (name, i)
            checked += 1
    assert checked >= len(grads)


def test_config_values_and_provenance():
    c = config.MaterialDataLossConfig()
    assert c.loss_type == "rawnerf_transient_unbiased"
    assert (c.loss_weight, c.data_loss_mult, c.material_loss_weight_ease, c.weight) == (0.1, 1.0, 1.0, 0.1)
    assert (c.exponent, c.eps, c.clip_val, c.loss_thresh) == (1.0, 1e-2, 1e4, 1e6)
    assert (c.use_gt_rawnerf, c.use_combined_rawnerf, c.use_norm_rawnerf, c.use_loss_clip) == (False, True, False, False)
    assert c.num_secondary_samples == 8 and c.filter_normals_thresh == 1.01
    import inspect
    src = inspect.getsource(config.MaterialDataLossConfig)
    for site in ("nerf_ngp_yobo.gin:427-428", "nerf_ngp_yobo.gin:437, 440", "ngp_yobo.gin:456", "configs.py:587-590",
                 "configs.py:447", "train_utils.py:3550-3597", "trainer.gin:327"):
        assert site in src, site
    with pytest.raises(dataclasses.FrozenInstanceError):
        c.eps = 1.0
    with pytest.raises(NotImplementedError):
        train.material_data_grads(None, None, None, None, cfg=dataclasses.replace(c, use_loss_clip=True))
