"""Torch restatement of the material stage's data loss with JAX's differentiation rules, for the CPU and
GPU tests of rc_material_data_backward.

  data loss     train_utils.compute_data_loss (internal/train_utils.py:402-528) with loss_type
                'rawnerf_transient_unbiased', which _select_data_loss_function (:664-669) maps to
                compute_unbiased_loss_rawnerf (:173-197): s = 1 / (sg(rgb_clip) ** exponent + eps) per ray and channel,
                rgb_clip from _get_rgb_clip_for_rawnerf (:369-395) on the rendering's "cache_rgb"
  integration   k_material_integrate's arithmetic: get_lobe (Disney-GGX D, Smith G with k = a / 2, Schlick F, Lambert),
                clip(radiance * lobe, 0, rgb_max) * weight / max(pdf, 1e-5), the means over the samples of each pass,
                rgb = w * (((dd + ds) + id) + is) + max(0, 1 - acc) * bg
  material head oracle.material_ref.material_mlp

The gradient is the Trainer.stopgrad = True reading: the trace's tensors (directions, pdf, weight, radiance, acc, EnvMap),
w and the primary geometry are constants (detached here).  JAX rules (jax 0.4.16, read from the source, not run):
jnp.clip = minimum(maximum(x, lo), hi), each tie passes half the gradient; jnp.maximum ties split; nan_to_num passes the
gradient where the value is finite; 2 (rgb - gt) sg(rgb - gt) has gradient 2 sg(rgb - gt), half the derivative of its
value."""
from __future__ import annotations

import math

import numpy as np
import torch

from jax_rules import F32_MAX, jmaximum, jminimum, nan_to_num  # noqa: F401
from oracle import material_ref

EPS = 1.1920929e-07          # jnp.finfo(float32).eps, the RC_EPS floors of get_lobe
DENOM_EPS = 1e-5             # render_utils.DENOMINATOR_EPS


def jclip(x, lo: float, hi: float):
    """jnp.clip(x, lo, hi) = minimum(maximum(x, lo), hi) with constant bounds."""
    return jminimum(jmaximum(x, torch.full_like(x, lo)), torch.full_like(x, hi))


def rgb_clip(cache_rgb, gt, clip_val=1e4, use_gt=False, use_combined=True, use_norm=False):
    """_get_rgb_clip_for_rawnerf: c = the rendering's "cache_rgb"."""
    if use_gt:
        r = jclip(gt, 0.0, clip_val)
    else:
        r = jclip(cache_rgb, 0.0, clip_val)
        if use_combined:
            r = jclip(jmaximum(r, gt), 0.0, clip_val)
    if use_norm:
        r = torch.linalg.norm(r, dim=-1, keepdim=True).expand_as(r)
    return r


def data_loss(rgb, gt, cache_rgb, lossmult=None, weight=0.1, mult=1.0, exponent=1.0, eps=1e-2, clip_val=1e4,
              thresh=1e6, use_gt=False, use_combined=True, use_norm=False):
    """weight * mult * mean_{n x 3}(lossmult * 2 (rgb - gt) sg(rgb - gt) s), s = 1 / (sg(rgb_clip) ** exponent + eps)
    per ray and channel; lossmult [n] (None: 1) is zeroed where gt > thresh."""
    lm = torch.ones_like(gt) if lossmult is None else lossmult[:, None].expand_as(gt)
    lm = torch.where(gt > thresh, torch.zeros_like(lm), lm)
    s = 1.0 / (torch.pow(rgb_clip(cache_rgb, gt, clip_val, use_gt, use_combined, use_norm).detach(), exponent) + eps)
    d = rgb - gt
    return weight * mult * (lm * (2.0 * d * d.detach() * s)).mean()


def loop_loss(rgb, gt, cache_rgb, lossmult=None, weight=0.1, mult=1.0, exponent=1.0, eps=1e-2, clip_val=1e4, thresh=1e6,
              use_gt=False, use_combined=True, use_norm=False):
    """The reference's expression as plain loops over rays and channels (floats), with _get_rgb_clip_for_rawnerf's three
    switches (train_utils.py:369-395): use_gt takes clip(gt), else clip(cache_rgb), combined with gt when use_combined;
    use_norm replaces every channel of a ray by the norm over its three."""
    rgb, gt, c = (np.asarray(t, np.float64) for t in (rgb, gt, cache_rgb))
    n = len(rgb)
    tot = 0.0
    for i in range(n):
        cr = [0.0, 0.0, 0.0]
        for k in range(3):
            if use_gt:
                cr[k] = min(max(gt[i, k], 0.0), clip_val)
            else:
                cr[k] = min(max(c[i, k], 0.0), clip_val)
                if use_combined:
                    cr[k] = min(max(max(cr[k], gt[i, k]), 0.0), clip_val)
        if use_norm:
            cr = [math.sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2])] * 3
        for k in range(3):
            lm = 1.0 if lossmult is None else float(lossmult[i])
            if gt[i, k] > thresh:
                lm = 0.0
            s = 1.0 / (cr[k] ** exponent + eps)
            d = rgb[i, k] - gt[i, k]
            tot += lm * 2.0 * d * d * s
    return weight * mult * tot / (3 * n)


def split_trace(n, Ks, Kd, samples, sec_rgb, sec_acc, sec_env):
    """The trace's tensors in k_brdf_sample's layout ([n*Ks specular | n*Kd diffuse] rays, samples [n][K][5]) as
    per-point [n][K] arrays, lanes [0, Ks) specular."""
    K = Ks + Kd
    sm = samples.reshape(n, K, 5)

    def per_point(x, w):
        x = x.reshape(-1, *w)
        a = x[: n * Ks].reshape(n, Ks, *w)
        b = x[n * Ks: n * K].reshape(n, Kd, *w)
        return torch.cat([a, b], dim=1)
    return sm, per_point(sec_rgb, (3,)), per_point(sec_acc, ()), per_point(sec_env, (3,))


def integrate(albedo, rough, metal, Ks, Kd, wo, sm, rgb_in, acc_in, env_in, f0=0.04, rgb_max=F32_MAX):
    """sh_rgb [n, 3]: the four integration means summed in k_material_integrate's order.  albedo [n, 3], rough / metal
    [n] carry the gradient; wo [n, 3] (local view), sm [n, K, 5], rgb_in / env_in [n, K, 3], acc_in [n, K] are constants."""
    sm, rgb_in, acc_in, env_in, wo = (t.detach() for t in (sm, rgb_in, acc_in, env_in, wo))
    K = Ks + Kd
    wi = sm[..., 0:3]
    pdf = sm[..., 3]
    weight = torch.clamp(sm[..., 4], min=0.0) * (wi[..., 2] > 0)
    denom = torch.clamp(pdf, min=DENOM_EPS)
    wo_ = wo[:, None, :].expand_as(wi)
    h = material_ref.ir_normalize(wi + wo_)
    n_v = torch.clamp(wo_[..., 2], min=0.0)
    n_l = torch.clamp(wi[..., 2], min=0.0)
    n_h = torch.clamp(h[..., 2], min=0.0)
    l_h = torch.clamp((wi * h).sum(-1), min=0.0)
    a = rough[:, None]
    t = n_h * n_h * (a * a - 1.0) + 1.0
    den = math.pi * (t * t)
    D = (a * a) / jmaximum(torch.full_like(den, EPS), den)
    k = a / 2.0
    gv = n_v * (1.0 - k) + k
    gl = n_l * (1.0 - k) + k
    G = (n_v / jmaximum(torch.full_like(gv, EPS), gv)) * (n_l / jmaximum(torch.full_like(gl, EPS), gl))
    c5 = torch.clamp(1.0 - l_h, 0.0, 1.0) ** 5
    m = metal[:, None, None]
    alb = albedo[:, None, :]
    F0 = alb * m + f0 * (1.0 - m)
    F = F0 + (1.0 - F0) * c5[..., None]
    ggx = D[..., None] * F * G[..., None] / torch.clamp(4.0 * n_v, min=EPS)[..., None]
    lam = n_l[..., None] * alb / math.pi
    spec = (torch.arange(K) < Ks)[None, :, None]
    lobe = torch.where(spec, ggx, lam * (1.0 - m))
    rin = torch.clamp(nan_to_num(rgb_in), min=0.0)
    ein = nan_to_num(torch.clamp(env_in, min=0.0) * (1.0 - acc_in[..., None]))
    wd = (weight / denom)[..., None]
    ind = jclip(rin * lobe, 0.0, rgb_max) * wd
    dr = jclip(ein * lobe, 0.0, rgb_max) * wd
    o_is, o_ds = ind[:, :Ks].sum(1) / Ks, dr[:, :Ks].sum(1) / Ks
    o_id, o_dd = ind[:, Ks:].sum(1) / Kd, dr[:, Ks:].sum(1) / Kd
    return ((o_dd + o_ds) + o_id) + o_is


def chain_loss(weights, cfg, pts, trace, gt, cache_rgb, w, acc_p, lossmult=None, bg=1.0, **loss_kw):
    """material MLP at the shading points pts [n, 3] -> integration -> loss, with the trace's tensors
    (Ks, Kd, wo, sm, rgb_in, acc_in, env_in) and w, acc_p [n] as constants."""
    Ks, Kd, wo, sm, rgb_in, acc_in, env_in = trace
    mm = material_ref.material_mlp(weights, cfg, pts.detach())
    sh = integrate(mm["albedo"], mm["roughness"][..., 0], mm["metalness"][..., 0], Ks, Kd, wo, sm, rgb_in, acc_in, env_in,
                   cfg.default_F_0, cfg.rgb_max)
    rgb = w.detach()[:, None] * sh + (torch.clamp(1.0 - acc_p.detach(), min=0.0) * bg)[:, None]
    return data_loss(rgb, gt, cache_rgb, lossmult, **loss_kw), rgb
