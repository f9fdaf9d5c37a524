"""Differentiable torch restatement of the cache stage's geometry losses on the last sampler level (test helper, not a
test module).

  w = weights * lossmult                                                  sampling.py:645-647
  distortion   mult * mean(lossfun_distortion(power_ladder(tdist, p, premult), w))    loss_utils.py:108-123,
                                                                                      stepfun.py:253-269
  orientation  mult * mean(|sum |w min(0, n^ . v)^2| + 1e-5|), v = -viewdirs          loss_utils.py:126-165
  predicted    mult * mean(|sum |w' (1 - n . n^)| + 1e-5|), n stop-gradiented,
               w' = stopgrad_with_weight(w, 0.1)                                       loss_utils.py:168-201, utils.py:87-95
  reverse      the same with w' = stop_gradient(w)                                    train_utils.py:1073-1093
  n^ = normals_pred = nan_to_num(-l2_normalize(pred_raw))                              geometry.py:467-471

JAX rules where torch differs (jax 0.4.16, jax/_src/lax/lax.py and jax/_src/numpy; written out in tests/jax_rules.py):
  * lax.abs: the JVP is select(x >= 0, g, -g) (`_abs_jvp_rule`), so the derivative is +1 at 0; torch's is 0 there;
  * jnp.minimum(0, y)^2: lax.min's balanced JVP passes half of the gradient at the tie, times 2 min(0, y) = 0: zero
    derivative at the tie either way;
  * ref_utils.l2_normalize's override_gradient: the backward divides by sqrt(max(float32 eps, |x|^2))
    (jax_rules.l2_normalize);
  * jnp.nan_to_num: `where(isnan(x), 0, clip(x, min, max))`-shaped, so the gradient passes where x is finite;
  * each ray's + 1e-5 sits inside the outer abs: it is part of the value, and enters the gradient only through the
    sign select of that abs.
"""
from __future__ import annotations

import torch

from jax_rules import jabs, l2_normalize
from oracle import mathx


def stopgrad_with_weight(x, weight):
    """utils.stopgrad_with_weight (utils.py:87-95): the value of x, weight times its gradient."""
    if weight == 1.0:
        return x
    if weight == 0.0:
        return x.detach()
    return (x - x.detach()) * weight + x.detach()


def normals_from_raw(raw):
    """nan_to_num(-l2_normalize(pred_raw)) with l2_normalize's override gradient."""
    return mathx.nan_to_num(-l2_normalize(raw))


def distortion(c, w):
    """stepfun.lossfun_distortion(c, w, normalize=False) per ray: c [..., S + 1], w [..., S]."""
    ut = (c[..., 1:] + c[..., :-1]) / 2
    dut = torch.abs(ut[..., :, None] - ut[..., None, :])
    loss_inter = torch.sum(w * torch.sum(w[..., None, :] * dut, dim=-1), dim=-1)
    loss_intra = torch.sum(w ** 2 * torch.diff(c, dim=-1), dim=-1) / 3
    return loss_inter + loss_intra


def geometry_losses(weights, lossmult, tdist, viewdirs, normals_pred, normals, terms):
    """The four losses [4] in rc_geometry_backward's order (distortion, orientation, predicted, reverse), each with
    its mult.  weights [n, S]; lossmult [n] or None; tdist [n, S + 1]; viewdirs [n, 3]; normals_pred / normals
    [n, S, 3] (normals_pred differentiable, e.g. normals_from_raw(raw)); terms: the rc_geometry_loss fields."""
    lm = torch.ones_like(weights[:, :1]) if lossmult is None else lossmult.reshape(-1, 1).to(weights.dtype)
    w = weights * lm
    c = mathx.power_ladder(tdist.detach(), terms["distortion_p"], terms["distortion_premult"])
    l_dist = terms["distortion_mult"] * torch.mean(distortion(c, w))
    # orientation_loss(target='normals_pred', normalize=False, stopgrad=False)
    v = -viewdirs
    n_hat = mathx.nan_to_num(normals_pred)
    n_dot_v = (n_hat * v[..., None, :]).sum(dim=-1)
    l_orient = terms["orientation_mult"] * torch.mean(
        jabs(jabs(w * torch.clamp(n_dot_v, max=0.0) ** 2).sum(dim=-1) + 1e-5))
    n = mathx.nan_to_num(normals).detach()

    def predicted(wt, mult):
        beta = torch.ones_like(n[..., :1])
        return mult * torch.mean(jabs((jabs(wt * (1.0 - torch.sum(n * n_hat, dim=-1)))[..., None] * beta)
                                      .sum(dim=-2) + 1e-5))

    l_pred = predicted(stopgrad_with_weight(w, terms["pred_normal_w_grad_weight"]), terms["pred_normal_mult"])
    l_rev = predicted(w.detach(), terms["pred_normal_reverse_mult"])
    return torch.stack([l_dist, l_orient, l_pred, l_rev])


def weights_from_density(density, tdist, directions):
    """render.compute_alpha_weights (render.py:134-169): differentiable in density."""
    delta = (tdist[..., 1:] - tdist[..., :-1]) * torch.linalg.norm(directions, dim=-1, keepdim=True)
    dd = density * torch.abs(delta)
    alpha = 1 - torch.exp(-dd)
    trans = torch.exp(-torch.cat([torch.zeros_like(dd[..., :1]), torch.cumsum(dd[..., :-1], dim=-1)], dim=-1))
    return alpha * trans


def grid_l2(tables, mult):
    """param_regularizer_loss with (mult, jnp.mean, 2, 1): mult * sum over tables of 0.5 * mean(x^2)."""
    return sum(mult * 0.5 * torch.mean(t ** 2) for t in tables)
