"""Torch restatement of the EnvMap's gradient of the material stage's data loss with JAX's
differentiation rules, for the CPU and GPU tests of rc_material_data_backward_env.  Test helper, not a test module.

  EnvMap        Model._handle_env_map (internal/models.py:360-421) -> oracle.cache_ref.model_env_map_rgb at the secondary
                rays' directions; env_map_fn's jnp.maximum(., 0) (internal/material.py:2305);
                stopgrad_with_weight(incoming_rgb, stopgrad_env_map_weight[1]) (models.py:412-418,
                configs/nerf_ngp_yobo.gin:420): the value unchanged, the gradient times env_scale
  integration   material_data_loss_ref.integrate's arithmetic, with the EnvMap radiance carrying the gradient (that
                function detaches it); the lobe carries it too, so that a caller sees where each gradient goes
  loss          material_data_loss_ref.data_loss

The reading is Trainer.stopgrad = True (engine/trainer.py:547-554): the trace's directions, pdf, MIS weight, cache radiance
and acc, w and the primary geometry are constants; pos_enc of a stopped direction passes nothing further."""
from __future__ import annotations

import math

import torch

import material_data_loss_ref as md
from jax_rules import F32_MAX, jmax, jmaximum, nan_to_num, value_with_grad_of
from oracle import cache_ref, material_ref

ENV = "params/Cache/EnvMap/"
LAYERS = ("layer_0", "layer_1", "layer_2", "layer_bottleneck", "output_rgba_layer")


def envmap_layout(cfg=None):
    """[(name, shape)] of rc_envmap_grad_layout for hotdog: the five layers the model-level path reads, kernel then bias."""
    dims = ((27, 256), (256, 256), (256, 256), (283, 128), (128, 4))
    out = []
    for l, (i, o) in zip(LAYERS, dims):
        out += [(f"{ENV}{l}/kernel", (i, o)), (f"{ENV}{l}/bias", (o,))]
    return out


def per_point(x, n, Ks, Kd, w):
    """[n Ks | n Kd] rays (k_brdf_sample's order) -> [n][Ks + Kd], lanes [0, Ks) specular."""
    x = x.reshape(-1, *w)
    return torch.cat([x[: n * Ks].reshape(n, Ks, *w), x[n * Ks: n * (Ks + Kd)].reshape(n, Kd, *w)], dim=1)


def env_radiance(weights_env, cfg, sec_dirs, n, Ks, Kd, env_scale=1.0):
    """[n, K, 3]: the EnvMap at the (stopped) secondary directions [n Ks | n Kd][3], env_map_fn's maximum, and
    stopgrad_with_weight's factor on the gradient."""
    env = cache_ref.model_env_map_rgb(weights_env, cfg, sec_dirs.detach())
    env = jmax(env, 0.0)
    env = value_with_grad_of(env, env_scale * env)
    return per_point(env, n, Ks, Kd, (3,))


def integrate(albedo, rough, metal, Ks, Kd, wo, sm, rgb_in, acc_in, env, f0=0.04, rgb_max=F32_MAX):
    """material_data_loss_ref.integrate with `env` [n, K, 3] (already >= 0) carrying the gradient."""
    sm, rgb_in, acc_in, wo = (t.detach() for t in (sm, rgb_in, acc_in, wo))
    K = Ks + Kd
    wi = sm[..., 0:3]
    pdf = sm[..., 3]
    weight = torch.clamp(sm[..., 4], min=0.0) * (wi[..., 2] > 0)
    denom = torch.clamp(pdf, min=md.DENOM_EPS)
    wo_ = wo[:, None, :].expand_as(wi)
    h = material_ref.ir_normalize(wi + wo_)
    n_v = torch.clamp(wo_[..., 2], min=0.0)
    n_l = torch.clamp(wi[..., 2], min=0.0)
    n_h = torch.clamp(h[..., 2], min=0.0)
    l_h = torch.clamp((wi * h).sum(-1), min=0.0)
    a = rough[:, None]
    t = n_h * n_h * (a * a - 1.0) + 1.0
    den = math.pi * (t * t)
    D = (a * a) / jmaximum(torch.full_like(den, md.EPS), den)
    k = a / 2.0
    gv = n_v * (1.0 - k) + k
    gl = n_l * (1.0 - k) + k
    G = (n_v / jmaximum(torch.full_like(gv, md.EPS), gv)) * (n_l / jmaximum(torch.full_like(gl, md.EPS), gl))
    c5 = torch.clamp(1.0 - l_h, 0.0, 1.0) ** 5
    m = metal[:, None, None]
    alb = albedo[:, None, :]
    F0 = alb * m + f0 * (1.0 - m)
    F = F0 + (1.0 - F0) * c5[..., None]
    ggx = D[..., None] * F * G[..., None] / torch.clamp(4.0 * n_v, min=md.EPS)[..., None]
    lam = n_l[..., None] * alb / math.pi
    spec = (torch.arange(K) < Ks)[None, :, None]
    lobe = torch.where(spec, ggx, lam * (1.0 - m))
    rin = torch.clamp(nan_to_num(rgb_in), min=0.0)
    ein = nan_to_num(env * (1.0 - acc_in[..., None]))
    wd = (weight / denom)[..., None]
    ind = md.jclip(rin * lobe, 0.0, rgb_max) * wd
    dr = md.jclip(ein * lobe, 0.0, rgb_max) * wd
    o_is, o_ds = ind[:, :Ks].sum(1) / Ks, dr[:, :Ks].sum(1) / Ks
    o_id, o_dd = ind[:, Ks:].sum(1) / Kd, dr[:, Ks:].sum(1) / Kd
    return ((o_dd + o_ds) + o_id) + o_is


def chain_loss(weights_mat, weights_env, cfg, pts, sec_dirs, trace, gt, cache_rgb, w, acc_p, lossmult=None, bg=1.0,
               env_scale=1.0, material_grad=False, **loss_kw):
    """material MLP at pts [n, 3] -> EnvMap at sec_dirs -> integration -> loss.  trace = (Ks, Kd, wo, sm, rgb_in,
    acc_in, _): the last member (the trace's own EnvMap radiance) is replaced by the EnvMap evaluated here.
    material_grad = False detaches the lobe's inputs: the gradient of the EnvMap tensors alone."""
    Ks, Kd, wo, sm, rgb_in, acc_in = trace[:6]
    n = pts.shape[0]
    mm = material_ref.material_mlp(weights_mat, cfg, pts.detach())
    alb, rough, metal = mm["albedo"], mm["roughness"][..., 0], mm["metalness"][..., 0]
    if not material_grad:
        alb, rough, metal = alb.detach(), rough.detach(), metal.detach()
    env = env_radiance(weights_env, cfg, sec_dirs, n, Ks, Kd, env_scale)
    sh = integrate(alb, rough, metal, Ks, Kd, wo, sm, rgb_in, acc_in, env, cfg.default_F_0, cfg.rgb_max)
    rgb = w.detach()[:, None] * sh + (torch.clamp(1.0 - acc_p.detach(), min=0.0) * bg)[:, None]
    return md.data_loss(rgb, gt, cache_rgb, lossmult, **loss_kw), rgb
