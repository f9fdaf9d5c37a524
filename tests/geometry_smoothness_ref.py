"""Torch restatement of the geometry smoothness loss and of the gradient through the analytic normals (test helper, not a
test module): train_utils.geometry_smoothness_loss (internal/train_utils.py:2703-2812) on the last sampler level, with the
JAX rules of tests/jax_rules.py (lax.abs' derivative, l2_normalize's override gradient, nan_to_num).

The analytic normals n = nan_to_num(-l2_normalize(d raw / d x)) (geometry.py:421-460, no stop-gradient) are taken with
create_graph=True from the oracle's own differentiable forward (hashgrid_ref.hash_encoding, cache_ref.dense), so a second
backward reaches the tables and the MLP kernels: what rc_normals_backward computes."""
import numpy as np
import torch

import jax_rules as jr
import nrc_amd
from oracle import hashgrid_ref, mathx
from oracle.cache_ref import P, dense
from oracle.train_ref import _SafeExp

CFG = nrc_amd.hotdog_config()
L2 = CFG.num_levels - 1
BASE = f"Cache/Sampler/MLP_{L2}"
LAYERS = ("density_layers_0", "density_layers_1", "output_density_layer")


def param_names(w):
    """The tensors of the last level's density layout: its grid tables and the three dense layers."""
    return [k for k in w if k.startswith(f"{P}{BASE}/density_grid/") or any(k.startswith(f"{P}{BASE}/{l}/") for l in LAYERS)]


def leaf_weights(w, dtype):
    """A copy of w in dtype whose last-level density tensors require a gradient."""
    names = set(param_names(w))
    t = lambda v: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))).detach().to(dtype).clone()
    return {k: t(v).requires_grad_(k in names) for k, v in w.items()}


def normals_chain(w, points, cfg=CFG):
    """(analytic normals [.., 3], converted density [..]) of the last level at world-space `points`, differentiable in the
    parameters of w (torch.autograd.grad with create_graph=True)."""
    gcfg = cfg.proposal_grids[L2]
    m = points.detach().clone().requires_grad_(True)
    warped = mathx.contract_radius(m, cfg.contract_radius)
    x = hashgrid_ref.hash_encoding(w, f"{P}{BASE}/density_grid", gcfg, warped)
    h = torch.relu(dense(w, f"{BASE}/density_layers_0", x))
    h = torch.relu(dense(w, f"{BASE}/density_layers_1", h))
    raw = dense(w, f"{BASE}/output_density_layer", h)[..., 0]
    (grad,) = torch.autograd.grad(raw.sum(), m, create_graph=True)
    normals = jr.nan_to_num(-jr.l2_normalize(grad))                       # geometry.py:460
    density = _SafeExp.apply(raw + cfg.density_bias)                      # convert_raw_density, geometry.py:318-341
    valid = ((warped > -gcfg.bbox) & (warped < gcfg.bbox)).all(dim=-1).detach()
    return normals, torch.where(valid, density, torch.zeros_like(density))


def normals_backward(w, points, d_normals, dtype):
    """({name: gradient of sum(d_normals * n(points))}, normals) over the last level's density layout; a tensor the sum
    does not reach (the biases) gets zeros."""
    lw = leaf_weights(w, dtype)
    names = param_names(lw)
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    n, _ = normals_chain(lw, t(points))
    grads = torch.autograd.grad((t(d_normals) * n).sum(), [lw[k] for k in names], allow_unused=True)
    return {k: (torch.zeros_like(lw[k]) if g is None else g).numpy() for k, g in zip(names, grads)}, n.detach().numpy()


def perturbed(means, noise, scale):
    """x' = fl(x + fl(noise * scale)) in float32, the two roundings separate."""
    step = (np.asarray(noise, np.float32) * np.float32(scale)).astype(np.float32)
    return (np.asarray(means, np.float32) + step).astype(np.float32)


def smoothness_loss(n_x, n_p, d_x, d_p, weights, lossmult, terms):
    """The loss (train_utils.py:2745-2812) from the normals [n, S, 3] and densities [n, S] at x and x', the last level's
    weights [n, S] and lossmult [n]; terms: train.geometry_smoothness_terms."""
    S = weights.shape[-1]
    c = lossmult[:, None] * (weights * S).detach()
    loss = terms["weight_normals"] * (jr.jabs(n_x - jr.nan_to_num(n_p)) * c[..., None]).mean()
    return loss + terms["weight_density"] * (jr.jabs(d_x - jr.nan_to_num(d_p)) * c).mean()


def loss_on_buffers(b, lossmult, terms, dtype):
    """(loss, {d_normals, d_normals_p, d_density, d_density_p}) of smoothness_loss on the "gs:" buffers b of a call."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    leaves = {k: t(b[k]).requires_grad_(True) for k in ("normals", "normals_p", "density", "density_p")}
    loss = smoothness_loss(leaves["normals"], leaves["normals_p"], leaves["density"], leaves["density_p"], t(b["weights"]),
                           t(lossmult), terms)
    g = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    g = [torch.zeros_like(x) if v is None else v for v, x in zip(g, leaves.values())]
    return float(loss.detach()), dict(d_normals=g[0].numpy(), d_normals_p=g[1].numpy(), d_density=g[2].numpy(),
                                      d_density_p=g[3].numpy())


def cell_face_margin(points, cfg=CFG):
    """min over the levels and axes of the distance of loc = x01 * N - 0.5 from an integer, in grid units: the trilinear
    Jacobian jumps at a cell face."""
    gcfg = cfg.proposal_grids[L2]
    x = mathx.contract_radius(torch.from_numpy(np.asarray(points)).double(), cfg.contract_radius)
    x01 = (x + gcfg.bbox) / (2.0 * gcfg.bbox)
    out = torch.full(x.shape[:-1], np.inf, dtype=torch.float64)
    for n in gcfg.grid_sizes:
        loc = x01 * n - 0.5
        out = torch.minimum(out, (loc - torch.round(loc)).abs().min(dim=-1).values)
    return out.numpy()
