"""Differentiable torch restatement of the cache pass's charb data loss from the level-2 hidden vector on
(test helper, not a test module).

  feature64 -> pred_normals_layer -> normals_pred = nan_to_num(-l2_normalize(.))      geometry.py:467-471
  [feature64 | app32] -> Cache/Shader (heads, integrated BRDF, IDE, SLF)             nerf.py:461-482, 940-1090
  composite sum w rgb_s + max(0, 1 - acc) bg                                         render.py:172-247
  L = mult * mean_{n x 3}(lossmult * sqrt((rgb - gt)^2 + padding^2))                 train_utils.py:402-528

built on oracle.cache_ref / oracle.mathx, with the two JAX derivative rules torch does not share (tests/jax_rules.py):
  * jnp.maximum / jnp.clip pass half of the gradient to each side at a tie (lax.max's balanced-eq JVP);
  * ref_utils.l2_normalize's override_gradient: the backward divides by sqrt(max(float32 eps, |x|^2)).
"""
from __future__ import annotations

import math

import torch

from jax_rules import l2_normalize, value_with_grad_of  # noqa: F401  (l2_normalize at its default grad_eps, float32 eps)
from oracle import cache_ref, mathx

P = "params/"


def maximum(x, lo):
    """jnp.maximum(x, lo) with scalar lo: the gradient is 1/2 at x == lo."""
    return value_with_grad_of(torch.clamp(x, min=lo), 0.5 * (x + lo + torch.abs(x - lo)))


def minimum(x, hi):
    return value_with_grad_of(torch.clamp(x, max=hi), 0.5 * (x + hi - torch.abs(x - hi)))


def clip(x, lo, hi):
    """jnp.clip = minimum(maximum(x, lo), hi)."""
    return minimum(maximum(x, lo), hi)


def normals_pred(weights, cfg, h64):
    raw = cache_ref.dense(weights, f"Cache/Sampler/MLP_{cfg.num_levels - 1}/pred_normals_layer", h64)
    return mathx.nan_to_num(-l2_normalize(raw)), raw


def shader_rgb(weights, cfg, h64, app, viewdirs, taps=None):
    """Per-sample rgb of the cache shader.  h64 [..., 64] (reference column order), app [..., 32], viewdirs [..., 3]
    (broadcast against the sample axis by the caller).  taps: a dict that receives pred_raw (gradient retained)."""
    normals, raw = normals_pred(weights, cfg, h64)
    if taps is not None and raw.requires_grad:
        raw.retain_grad()
        taps["pred_raw"] = raw
    feature = torch.cat([h64, app], dim=-1)
    sp = mathx.softplus
    bottleneck = cache_ref.dense(weights, "Cache/Shader/bottleneck_layer", feature)
    roughness = sp(cache_ref.dense(weights, "Cache/Shader/roughness_layer", feature) + cfg.roughness_bias)
    ambient_diffuse = clip(sp(cache_ref.dense(weights, "Cache/Shader/ambient_irradiance_layer", feature)
                              + cfg.ambient_irradiance_bias), 0.0, cfg.rgb_max)
    tint = torch.sigmoid(cache_ref.dense(weights, "Cache/Shader/tint_layer", feature))
    dotprod = (normals * -viewdirs).sum(-1, keepdim=True)
    x = torch.cat([bottleneck, dotprod], dim=-1)
    x = torch.relu(cache_ref.dense(weights, "Cache/Shader/integrated_brdf_layers_0", x))
    x = torch.relu(cache_ref.dense(weights, "Cache/Shader/integrated_brdf_layers_1", x))
    ibrdf = torch.sigmoid(cache_ref.dense(weights, "Cache/Shader/output_integrated_brdf_layer", x) + math.log(3.0))
    refdirs = mathx.reflect(-viewdirs, normals)
    indirect_diffuse = clip(sp(cache_ref.dense(weights, "Cache/Shader/irradiance_layer", feature) + cfg.irradiance_bias),
                            0.0, cfg.rgb_max)
    x = torch.cat([bottleneck, mathx.ide(refdirs, roughness, cfg.slf_deg_view)], dim=-1)
    x = cache_ref.slf_trunk(weights, "Cache/Shader/SurfaceLightField", x)
    ref_rgb = maximum(sp(cache_ref.dense(weights, "Cache/Shader/SurfaceLightField/output_ambient_rgb_layer", x)
                         + cfg.slf_ambient_bias), 0.0)
    ambient_specular = clip(tint * ibrdf * (torch.zeros_like(ref_rgb) * 0.0), 0.0, cfg.rgb_max)   # env * (1 - ref_acc)
    indirect_specular = clip(tint * ibrdf * ref_rgb, 0.0, cfg.rgb_max)
    return (ambient_diffuse + ambient_specular) + (indirect_diffuse + indirect_specular)


def composite(cfg, rgb_s, density, tdist, directions):
    """rgb = sum w rgb_s + max(0, 1 - acc) bg, w from compute_alpha_weights."""
    w, _, _ = cache_ref.compute_alpha_weights(density, tdist, directions)
    acc = w.sum(-1)
    return (w[..., None] * rgb_s).sum(-2) + maximum(1.0 - acc[..., None], 0.0) * cfg.bg_intensity, w


def charb(rgb, gt, lossmult, padding, mult):
    return mult * (lossmult[:, None] * torch.sqrt((rgb - gt) ** 2 + padding ** 2)).mean()


def data_loss(weights, cfg, h64, app, density, tdist, directions, viewdirs, gt, lossmult, padding=1e-3, mult=1.0, taps=None):
    """h64 [n, S, 64], app [n, S, 32], density [n, S], tdist [n, S + 1], directions / viewdirs / gt [n, 3], lossmult [n]."""
    rgb_s = shader_rgb(weights, cfg, h64, app, viewdirs[:, None, :], taps)
    rgb, _ = composite(cfg, rgb_s, density, tdist, directions)
    return charb(rgb, gt, lossmult, padding, mult), rgb
