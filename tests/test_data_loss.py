"""The torch restatement of the cache pass's data loss (tests/data_loss_ref.py): its forward against the oracle, its
gradients against finite differences, the JAX tie and override rules, and which parameters the loss reaches."""
import numpy as np
import pytest
import torch

import common
import data_loss_ref as dr
import nrc_amd
from nrc_amd import train
from oracle import cache_ref, mathx

CFG = nrc_amd.hotdog_config()
N, S = 6, 4


def _inputs(seed=3, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=dtype)
    h64 = torch.relu(r(N, S, 64) * 2 - 0.8)
    app = (r(N, S, 32) - 0.5) * 0.4
    density = r(N, S) * 3
    tdist = torch.cumsum(r(N, S + 1) * 0.5 + 0.1, -1) + 1.0
    directions = r(N, 3) - 0.5
    viewdirs = directions / directions.norm(dim=-1, keepdim=True)
    gt = r(N, 3)
    lossmult = r(N) + 0.5
    lossmult[1] = 0.0
    return h64, app, density, tdist, directions, viewdirs, gt, lossmult


def _weights(dtype=torch.float64):
    return common.weights_torch(dtype=dtype)


def test_data_grads_api_exists():
    cfg = nrc_amd.DataLossConfig()
    assert (cfg.charb_padding, cfg.loss_weight, cfg.data_loss_mult) == (1e-3, 1.0, 1.0)
    assert callable(train.data_grads)


def test_forward_matches_the_oracle():
    """Restated shader + composite == oracle.cache_ref.cache_shader + volume_integrate in fp64."""
    w = _weights()
    h64, app, density, tdist, directions, viewdirs, gt, lossmult = _inputs()
    _, rgb = dr.data_loss(w, CFG, h64, app, density, tdist, directions, viewdirs, gt, lossmult)
    normals = mathx.nan_to_num(-mathx.l2_normalize(cache_ref.dense(w, "Cache/Sampler/MLP_2/pred_normals_layer", h64)))
    rays = {"viewdirs": viewdirs, "origins": torch.zeros_like(viewdirs)}
    sres = {"means": torch.zeros(N, S, 3, dtype=torch.float64), "feature": h64, "normals_to_use": normals}
    sh = cache_ref.cache_shader(w, CFG, rays, sres, app=app)
    wts, _, _ = cache_ref.compute_alpha_weights(density, tdist, directions)
    sh.update(weights=wts, weights_no_filter=wts, tdist=tdist)
    ref = cache_ref.volume_integrate(CFG, sh, CFG.bg_intensity)["rgb"]
    assert torch.allclose(rgb, ref, rtol=1e-12, atol=1e-12), float((rgb - ref).abs().max())


def test_gradients_match_finite_differences():
    """Inputs and a sample of every parameter tensor the loss reaches, central differences in fp64."""
    w = {k: v.clone().requires_grad_(True) for k, v in _weights().items()}
    ins = list(_inputs())
    for i in (0, 1, 2):
        ins[i] = ins[i].clone().requires_grad_(True)
    loss, _ = dr.data_loss(w, CFG, *ins)
    loss.backward()
    rng = np.random.Generator(np.random.PCG64(0))
    names = [k for k, v in w.items() if v.grad is not None and "grid" not in k]
    assert len(names) >= 28, names
    checks = [(ins[i], f"input{i}") for i in (0, 1, 2)] + [(w[k], k) for k in names]
    eps = 1e-6
    for t, name in checks:
        flat = t.detach().view(-1)
        for idx in rng.choice(flat.numel(), size=min(3, flat.numel()), replace=False):
            old = float(flat[idx])
            vals = []
            for d in (eps, -eps):
                flat[idx] = old + d
                with torch.no_grad():
                    args = [x.detach() for x in ins]
                    vals.append(float(dr.data_loss({k: v.detach() for k, v in w.items()}, CFG, *args)[0]))
            flat[idx] = old
            fd = (vals[0] - vals[1]) / (2 * eps)
            an = float(t.grad.view(-1)[idx])
            assert abs(fd - an) <= 1e-6 * max(1.0, abs(fd)) + 1e-8, (name, int(idx), fd, an)


def test_tie_rule_known_answers():
    """jnp.maximum / clip pass half the gradient at a tie: max(0, 1 - acc) at acc == 1 has d/d acc = -1/2."""
    acc = torch.tensor([1.0, 0.5, 1.5], dtype=torch.float64, requires_grad=True)
    dr.maximum(1.0 - acc, 0.0).sum().backward()
    assert acc.grad.tolist() == [-0.5, -1.0, 0.0]
    x = torch.tensor([0.0, 2.0, 5.0, 7.0], dtype=torch.float64, requires_grad=True)
    y = dr.clip(x, 0.0, 5.0)
    y.sum().backward()
    assert y.tolist() == [0.0, 2.0, 5.0, 5.0]
    assert x.grad.tolist() == [0.5, 1.0, 0.5, 0.0]


def test_l2_normalize_override_known_answers():
    """Forward divides by sqrt(max(tiny, |x|^2)), backward by sqrt(max(eps, |x|^2)); zero below tiny."""
    eps = mathx.EPS
    # |x|^2 well above eps: the ordinary Jacobian (I - u u^T) / |x|
    x = torch.tensor([[3.0, 4.0, 0.0]], dtype=torch.float64, requires_grad=True)
    dr.l2_normalize(x)[0, 0].backward()
    assert torch.allclose(x.grad, torch.tensor([[16 / 125, -12 / 125, 0.0]], dtype=torch.float64))
    # tiny < |x|^2 < eps: value is the unit vector, the gradient that of x / sqrt(eps)
    x = torch.tensor([[1e-5, 0.0, 0.0]], dtype=torch.float64, requires_grad=True)
    y = dr.l2_normalize(x)
    assert float(y.detach()[0, 0]) == 1.0
    y[0, 0].backward()
    assert abs(float(x.grad[0, 0]) - 1.0 / np.sqrt(eps)) <= 1e-9 / np.sqrt(eps)
    # below tiny: zero output, zero gradient
    x = torch.tensor([[1e-30, 0.0, 0.0]], dtype=torch.float64, requires_grad=True)
    y = dr.l2_normalize(x)
    assert float(y.detach().abs().sum()) == 0.0
    y.sum().backward()
    assert float(x.grad.abs().sum()) == 0.0


def test_gradients_lie_in_the_two_layouts():
    """fp64 autograd over ALL weights of the cache pass, with the level-2 hidden vector and the appearance features
    computed from the grids: every parameter with a non-zero gradient is in density_grad_layout(2) or the shader
    layout (train.shader_grad_layout, whose C twin the GPU test compares)."""
    w = {k: v.clone().requires_grad_(True) for k, v in _weights().items()}
    rays = common.rays_torch(nrc_amd.synthetic_rays(8, seed=4), torch.float64)
    out = cache_ref.cache_forward(w, CFG, rays, want_grad_normals=False)
    res = out["sampler"][-1]
    means = res["means"].detach()
    x = cache_ref.hashgrid_ref.hash_encoding(w, "params/Cache/Sampler/MLP_2/density_grid", CFG.proposal_grids[2],
                                             mathx.contract_radius(means, CFG.contract_radius))
    h = torch.relu(cache_ref.dense(w, "Cache/Sampler/MLP_2/density_layers_0", x))
    h = torch.relu(cache_ref.dense(w, "Cache/Sampler/MLP_2/density_layers_1", h))
    raw = cache_ref.dense(w, "Cache/Sampler/MLP_2/output_density_layer", h)[..., 0]
    density = mathx.safe_exp(raw + CFG.density_bias)
    valid = ((mathx.contract_radius(means, CFG.contract_radius).abs() < CFG.proposal_grids[2].bbox).all(-1))
    density = torch.where(valid, density, torch.zeros_like(density))
    app = cache_ref.hashgrid_ref.hash_encoding(w, "params/Cache/Shader/appearance_grid", CFG.appearance_grid,
                                               mathx.contract_radius(means, CFG.contract_radius))
    gt = torch.full((8, 3), 0.3, dtype=torch.float64)
    loss, _ = dr.data_loss(w, CFG, h, app, density, res["tdist"].detach(), rays["directions"], rays["viewdirs"], gt,
                           torch.ones(8, dtype=torch.float64))
    loss.backward()
    hit = {k for k, v in w.items() if v.grad is not None and bool((v.grad != 0).any())}
    dens = {k for k in w if k.startswith("params/Cache/Sampler/MLP_2/") and "pred_normals" not in k}
    app_tables = [(k, tuple(w[k].shape)) for k in w if k.startswith("params/Cache/Shader/appearance_grid/")]
    layout, total = train.shader_grad_layout(CFG, app_tables)
    shader = {name[: -len("/kernel")] if name.endswith("/kernel") else name[: -len("/bias")] if name.endswith("/bias")
              else name for name, _, _ in layout}
    allowed = dens | {k for k in w if any(k == s or k.startswith(s + "/") for s in shader)}
    assert hit <= allowed, sorted(hit - allowed)
    assert any("SurfaceLightField/layer_bottleneck" in k for k in hit)
    assert any("pred_normals_layer" in k for k in hit)
    assert total == sum(int(np.prod(s)) for _, _, s in layout)
    for name, _, shape in layout:
        key = name if name in w else None
        if key is not None:
            assert tuple(w[key].shape) == shape, name
