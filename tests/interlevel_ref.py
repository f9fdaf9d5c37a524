"""Test support: a dtype-generic torch restatement of the reference's spline interlevel loss (not imported by the product).

Restates, on [..., k] tensors of any float dtype:
  math.minus_eps / plus_eps            internal/math.py:56-66
  stepfun.weight_to_pdf                internal/stepfun.py:75-79 (with math.safe_div, math.py:133-140)
  linspline.blur_stepfun               internal/linspline.py:187-222 (stable argsort, dyp gathered with idx[:-2])
  linspline.compute_integral           internal/linspline.py:95-108
  linspline.interpolate_integral       internal/linspline.py:124-141 (queries clipped to [t0, minus_eps(t_last)],
                                       searchsorted side='right')
  stepfun.blur_and_resample_weights    internal/stepfun.py:463-483
  render.compute_alpha_weights         internal/render.py:134-169
  loss_utils.spline_interlevel_loss    internal/loss_utils.py:74-104
"""
from __future__ import annotations

import numpy as np
import torch

TINY = float(np.finfo(np.float32).tiny)        # math.tiny_val
F32_MAX = float(np.finfo(np.float32).max)


def minus_eps(x):
    return torch.where(x.abs() < TINY, torch.full_like(x, -TINY), torch.nextafter(x, torch.full_like(x, -np.inf)))


def plus_eps(x):
    return torch.where(x.abs() < TINY, torch.full_like(x, TINY), torch.nextafter(x, torch.full_like(x, np.inf)))


def safe_div(n, d):
    dz = torch.where(d.abs() < TINY, torch.full_like(d, TINY), d)
    r = torch.clamp(n / dz, -F32_MAX, F32_MAX)
    return torch.where(d.abs() < TINY, torch.zeros_like(r), r)


def weight_to_pdf(t, w):
    td = torch.diff(t, dim=-1)
    return torch.where(td < TINY, torch.zeros_like(td), safe_div(w, td))


def blur_stepfun(ts, ys, halfwidth):
    ts_lo = torch.minimum(minus_eps(ts), ts - halfwidth)
    ts_hi = torch.maximum(plus_eps(ts), ts + halfwidth)
    z = torch.zeros_like(ys[..., :1])
    ys0 = torch.cat([z, ys, z], dim=-1)
    dy = torch.diff(ys0, dim=-1) / (ts_hi - ts_lo)
    tp = torch.cat([ts_lo, ts_hi], dim=-1)
    dyp = torch.cat([dy, -dy], dim=-1)
    idx = torch.argsort(tp, dim=-1, stable=True)
    tp = torch.take_along_dim(tp, idx, dim=-1)
    dyp = torch.take_along_dim(dyp, idx[..., :-2], dim=-1)
    yp = torch.cumsum(torch.diff(tp, dim=-1)[..., :-1] * torch.cumsum(dyp, dim=-1), dim=-1)
    z = torch.zeros_like(yp[..., :1])
    return tp, torch.cat([z, yp, z], dim=-1)


def compute_integral(t, y):
    eps = float(np.finfo(np.float32).eps) ** 2
    eps = float(np.float32(eps))
    dt = torch.diff(t, dim=-1)
    a = torch.diff(y, dim=-1) / torch.clamp(2 * dt, min=eps)
    b = y[..., :-1]
    c1 = 0.5 * torch.cumsum(dt[..., :-1] * (y[..., :-2] + y[..., 1:-1]), dim=-1)
    c = torch.cat([torch.zeros_like(y[..., :1]), c1], dim=-1)
    return a, b, c


def interpolate_integral(tq, t, a, b, c):
    tq = torch.minimum(torch.maximum(tq, t[..., :1]), minus_eps(t[..., -1:]))
    idx = torch.searchsorted(t.contiguous(), tq.contiguous(), right=True)
    idx0 = torch.clamp(idx - 1, min=0)
    t0 = torch.take_along_dim(t, idx0, dim=-1)
    a0 = torch.take_along_dim(a, idx0, dim=-1)
    b0 = torch.take_along_dim(b, idx0, dim=-1)
    c0 = torch.take_along_dim(c, idx0, dim=-1)
    td = tq - t0
    return a0 * td ** 2 + b0 * td + c0


def blurred_cdf(tq, t, w, halfwidth):
    """The integrated blurred PDF at tq (before the diff of blur_and_resample_weights)."""
    p = weight_to_pdf(t, w)
    tl, pl = blur_stepfun(t, p, halfwidth)
    return interpolate_integral(tq, tl, *compute_integral(tl, pl))


def blur_and_resample_weights(tq, t, w, halfwidth):
    acc = blurred_cdf(tq, t, w, halfwidth)
    return torch.clamp(torch.diff(acc, dim=-1), min=0)


def compute_alpha_weights(density, tdist, dirs):
    delta = (tdist[..., 1:] - tdist[..., :-1]) * torch.linalg.norm(dirs[..., None, :], dim=-1)
    dd = density * delta.abs()
    alpha = 1 - torch.exp(-dd)
    trans = torch.exp(-torch.cat([torch.zeros_like(dd[..., :1]), torch.cumsum(dd[..., :-1], dim=-1)], dim=-1))
    return alpha * trans


def spline_interlevel_loss(sdists, weights, lossmult, mults, blurs, eps=1e-5):
    """sdists / weights: per level [n, S+1] / [n, S] (last = target); lossmult [n, 1].  -> [loss per proposal level]."""
    c = sdists[-1]
    w = weights[-1] * lossmult
    out = []
    for mult, blur, cp, wl in zip(mults, blurs, sdists[:-1], weights[:-1]):
        wp = wl * lossmult
        w_blur = blur_and_resample_weights(cp, c, w, blur).detach()
        losses = torch.clamp(w_blur - wp, min=0) ** 2 / (wp + eps)
        out.append(mult * losses.mean())
    return out


def interlevel_forward_backward(sdists, tdists, densities, directions, lossmult, mults, blurs, dtype):
    """Losses and d loss_l / d density_l (autograd through compute_alpha_weights) from the samplers' sdist / tdist /
    density per level, in `dtype`.  Inputs are numpy / torch arrays of any float type."""
    T = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    dens = [T(d).clone().requires_grad_(i < len(densities) - 1) for i, d in enumerate(densities)]
    dirs = T(directions)
    lm = T(lossmult).reshape(-1, 1)
    sd = [T(s) for s in sdists]
    w = [compute_alpha_weights(d, T(t), dirs) for d, t in zip(dens, tdists)]
    losses = spline_interlevel_loss(sd, w, lm, mults, blurs)
    grads = [torch.autograd.grad(loss, dens[i], retain_graph=True)[0] for i, loss in enumerate(losses)]
    return [float(v.detach()) for v in losses], [g.detach() for g in grads]
