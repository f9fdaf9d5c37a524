"""Torch restatement of the time-resolved cache stage's sampler-side losses, for the CPU and GPU tests of
rc_transient_{interlevel,geometry,mask}_backward, rc_transient_density_regularizer and the weights path of
rc_transient_data_backward_sampler.  Test helper, not a test module.

  forward      the oracle's own proposal sampler under the time-resolved model's settings (oracle.cache_ref.proposal_sampler
               with nrc_amd.cornell_transient_config()): power-ladder distances s -> t on every ray (TransientNeRFModel:
               use_raydist_for_secondary_only = False), contract radius 5, HashEncoding.bbox_scaling = 2, at the config's
               anneal.  `linear=True` swaps in the steady-state model's linear s -> t: the sampler guard of the GPU tests.
  reading      sdist / tdist / means carry no gradient (sampling.py:354-355): the positions come from a forward without a
               graph, every level's density is then recomputed from its means with the parameters as leaves
               (level_density), as tests/test_gpu_geometry_loss.py's oracle chain does for the last level.
  losses       tests/interlevel_ref.py, geometry_loss_ref.py, mask_loss_ref.py on those densities; the regularizer is
               geometry_loss_ref.grid_l2 of a level's tables.
  weights path d loss / d density of the data loss given d loss / d weights (weights_path): the closed form of
               compute_alpha_weights' transpose, w_k = (1 - exp(-x_k)) exp(-sum_{i<k} x_i), x = density |delta|:
               d L / d x_k = g_k T_{k+1} - sum_{i>k} g_i w_i, T_{k+1} = exp(-sum_{i<=k} x_i); d L / d density = that |delta|.
               It is NOT the whole gradient of the data loss w.r.t. MLP_<last>: the paths through the geometry feature and
               the normals into the shader are left out (they need the shader's backward).
"""
from __future__ import annotations

import numpy as np
import torch

import geometry_loss_ref as gr
import interlevel_ref as ir
import mask_loss_ref as mr
import nrc_amd
from oracle import cache_ref, hashgrid_ref, mathx, train_ref

CFG = nrc_amd.cornell_transient_config()
NL = CFG.num_levels
L2 = NL - 1
P = "params/"
LEVEL_LAYERS = ("density_layers_0", "density_layers_1", "output_density_layer")
PRED = f"{P}Cache/Sampler/MLP_{L2}/pred_normals_layer"
# The batch of the GPU parity tests: synthetic_transient_rays at its own near / far (0.7, 4), nine rays = two full four-ray
# workgroups and one wave of a third.  The sampler guard (tests/test_transient_sampler.py) holds at these values.
CASE = dict(n=9, seed=101, jitter_seed=102)


def sampler_layout(cfg=CFG):
    """[(name, shape)] of RC_LAYOUT_TRANSIENT_SAMPLER (train.transient_sampler_layout: per level the grid tables in level
    order, then the three density layers; pred_normals_layer at the end)."""
    from nrc_amd import train

    return [(name, shape) for name, _, shape in train.transient_sampler_layout(cfg)[0]]


def to_torch(w_np, dtype):
    return {k: (torch.from_numpy(np.asarray(v)).to(dtype) if np.asarray(v).dtype.kind == "f" else torch.from_numpy(np.asarray(v)))
            for k, v in w_np.items()}


def positions(w, rays, jitters, cfg=CFG, linear=False):
    """The sampler's history (per level sdist, tdist, means; the last level's analytic normals), detached."""
    wd = {k: v.detach() for k, v in w.items()}
    hist = cache_ref.proposal_sampler(wd, cfg, rays, jitters, False, not linear, True)
    return [{k: (v.detach() if torch.is_tensor(v) else v) for k, v in h.items()} for h in hist]


def level_density(w, level, means, cfg=CFG):
    """(density [n, S], hidden [n, S, 64], the two pre-activations) of level `level` at `means`, differentiable in w."""
    gcfg = cfg.proposal_grids[level]
    base = f"Cache/Sampler/MLP_{level}"
    warped = mathx.contract_radius(means, cfg.contract_radius)
    x = hashgrid_ref.hash_encoding(w, f"{P}{base}/density_grid", gcfg, warped)
    z0 = cache_ref.dense(w, f"{base}/density_layers_0", x)
    z1 = cache_ref.dense(w, f"{base}/density_layers_1", torch.relu(z0))
    h = torch.relu(z1)
    raw = cache_ref.dense(w, f"{base}/output_density_layer", h)[..., 0]
    density = train_ref._SafeExp.apply(raw + cfg.density_bias)
    valid = ((warped > -gcfg.bbox) & (warped < gcfg.bbox)).all(dim=-1)
    return torch.where(valid, density, torch.zeros_like(density)), h, (z0, z1)


def weights_path(d_weights, density, tdist, directions):
    """d loss / d density [n, S] from d loss / d weights [n, S], the closed form of the module docstring (numpy / torch in,
    the inputs' dtype out)."""
    g, dens, td, dirs = (torch.as_tensor(np.asarray(a)) for a in (d_weights, density, tdist, directions))
    adelta = ((td[..., 1:] - td[..., :-1]) * torch.linalg.norm(dirs, dim=-1, keepdim=True)).abs()
    x = dens * adelta
    cum = torch.cumsum(x, dim=-1)
    t_next = torch.exp(-cum)
    w = (1 - torch.exp(-x)) * torch.exp(-(cum - x))
    gw = g * w
    after = torch.flip(torch.cumsum(torch.flip(gw, (-1,)), dim=-1), (-1,)) - gw          # sum_{i>k} g_i w_i
    return ((g * t_next - after) * adelta).numpy()


def _grads(loss, w, extra):
    names = [k for k, v in w.items() if v.requires_grad]
    gs = torch.autograd.grad(loss, [w[k] for k in names] + extra, allow_unused=True, retain_graph=True)
    z = lambda g, x: torch.zeros_like(x) if g is None else g
    byname = {k: z(g, w[k]).double().numpy() for k, g in zip(names, gs[: len(names)])}
    return byname, [z(g, x).double().numpy() for g, x in zip(gs[len(names):], extra)]


def chain(w_np, rays_np, jitters_np, dtype, lossmult=None, masks=None, il=None, geo_terms=None, mask_terms=None, reg_mult=None,
          d_weights=None, cfg=CFG, linear=False):
    """Everything the sampler-side calls compute on a batch, in `dtype`.  Each of il = (mults, blurs), geo_terms (rc_geometry_loss
    fields), mask_terms (rc_mask_loss fields), reg_mult, d_weights ([n, S2]: the data loss's adjoint of the compositing weights)
    adds an entry to the result: {"interlevel" | "geometry" | "mask" | "reg" | "weights_path": {"losses": [..], "grads": {tensor
    name: array, every parameter of the sampler layout}, "d_density": the adjoints of the densities the call exposes}}, beside
    "margin" [n, levels]: per ray and level the smallest |pre-activation| of the level's density MLP, and "preact": the
    pre-activations per level (for the margin's own size)."""
    w = to_torch(w_np, dtype)
    for name, _ in sampler_layout(cfg):
        w[name].requires_grad_(True)
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a)).to(dtype)
    rays = {k: t(v) for k, v in rays_np.items()}
    n = rays["origins"].shape[0]
    for k in ("near", "far", "lossmult"):
        rays[k] = rays[k].reshape(n, 1)
    jit = None if jitters_np is None else [t(j).reshape(-1, 1) for j in jitters_np]
    hist = positions(w, rays, jit, cfg, linear)
    lm = torch.ones(n, dtype=dtype) if lossmult is None else t(lossmult).reshape(-1)
    dens, hid, pre = [], [], []
    for l in range(cfg.num_levels):
        d, h, z = level_density(w, l, hist[l]["means"], cfg)
        d.retain_grad()
        dens.append(d); hid.append(h); pre.append(z)
    dirs = rays["directions"]
    wts = [ir.compute_alpha_weights(d, h["tdist"], dirs) for d, h in zip(dens, hist)]
    out = {"margin": np.stack([torch.minimum(z0.abs().amin(dim=(-1, -2)), z1.abs().amin(dim=(-1, -2))).detach().double().numpy()
                               for z0, z1 in pre], axis=-1),
           "preact": [torch.cat([z0, z1], dim=-1).detach().double().numpy() for z0, z1 in pre],
           "tdist": hist[L2]["tdist"].double().numpy(), "density": dens[L2].detach().double().numpy(),
           "weights": wts[L2].detach().double().numpy()}
    if il is not None:
        mults, blurs = il
        losses = ir.spline_interlevel_loss([h["sdist"] for h in hist], wts, lm.reshape(-1, 1), mults, blurs)
        g, dd = _grads(sum(losses), w, dens[:-1])
        out["interlevel"] = {"losses": np.array([float(v.detach()) for v in losses]), "grads": g, "d_density": dd}
    if geo_terms is not None:
        pred_raw = cache_ref.dense(w, f"Cache/Sampler/MLP_{L2}/pred_normals_layer", hid[L2])
        losses = gr.geometry_losses(wts[L2], lm, hist[L2]["tdist"], rays["viewdirs"], gr.normals_from_raw(pred_raw),
                                    hist[L2]["normals"], geo_terms)
        g, dd = _grads(losses.sum(), w, [dens[L2]])
        out["geometry"] = {"losses": losses.detach().double().numpy(), "grads": g, "d_density": dd}
    if mask_terms is not None:
        loss = mr.mask_terms_loss(wts[L2].sum(dim=-1), t(masks), lm, mask_terms)
        g, dd = _grads(loss, w, [dens[L2]])
        out["mask"] = {"losses": np.array([float(loss.detach())]), "grads": g, "d_density": dd}
    if reg_mult is not None:
        losses = [gr.grid_l2([w[k] for k, _ in sampler_layout(cfg) if k.startswith(f"{P}Cache/Sampler/MLP_{l}/density_grid/")],
                             reg_mult) for l in range(cfg.num_levels)]
        g, _ = _grads(sum(losses), w, [])
        out["reg"] = {"losses": np.array([float(v.detach()) for v in losses]), "grads": g}
    if d_weights is not None:
        loss = (wts[L2] * t(d_weights).reshape(n, -1)).sum()
        g, dd = _grads(loss, w, [dens[L2]])
        out["weights_path"] = {"grads": g, "d_density": dd}
    return out
