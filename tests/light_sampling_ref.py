"""Torch restatement of the light sampler's own loss with JAX's differentiation rules, for the CPU and
GPU tests of rc_light_sampling_backward.

  vmf_loss_fn      internal/inverse_render/render_utils.py:1493-1547 (eval_vmf :1335-1347, safe_exp
                   inverse_render/math.py:116-117, l2_normalize ref_utils.py:45-70, linear_to_srgb image.py:192-200)
  light_sampling   internal/train_utils.py:1985-2067: both suffixes, lossmult / K inside the mean, / 2 each
  light head       oracle.material_ref.light_vmfs (hash grid, three dense layers) with get_vmfs' activations under
                   jnp.maximum / jnp.minimum's tie rule (half the gradient to each side on a tie)

Everything the loss reads besides the lobes is stop-gradiented here, as the reference does."""
from __future__ import annotations

import math

import numpy as np
import torch

from jax_rules import FLT_EPS, TINY, jmax, jmin, l2_normalize  # noqa: F401
from oracle import cache_ref, hashgrid_ref, mathx

P = "params/"


def safe_exp(x):
    """inverse_render.math.safe_exp: exp(minimum(x, 80)); no custom JVP."""
    return torch.exp(jmin(x, 80.0))


def eval_vmf(x, means, kappa):
    val = kappa * safe_exp(kappa * (x * means).sum(-1)) / (4 * math.pi * torch.sinh(kappa))
    return torch.where(kappa <= FLT_EPS, torch.full_like(val, 1.0 / (4.0 * math.pi)), val)


def linear_to_srgb(x):
    s0 = 323.0 / 25.0 * x
    s1 = (211.0 * jmax(x, FLT_EPS) ** (5.0 / 12.0) - 11.0) / 200.0
    return torch.where(x <= 0.0031308, s0, s1)


def vmf_params(weights, cfg, pts):
    """The light head before get_vmfs: light_grid(contract(pts)) -> Dense64-ReLU x2 -> Dense(640), [N, 128, 5]."""
    g = hashgrid_ref.hash_encoding(weights, f"{P}LightSampler/light_grid", cfg.light_grid,
                                   mathx.contract_radius(pts, cfg.contract_radius))
    x = torch.relu(cache_ref.dense(weights, "LightSampler/layers_0", g))
    x = torch.relu(cache_ref.dense(weights, "LightSampler/layers_1", x))
    return cache_ref.dense(weights, "LightSampler/output_layer", x).reshape(pts.shape[:-1] + (cfg.num_vmf, 5))


def get_vmfs(vp, noise, pts, vmf_scale: float):
    """get_vmfs (light_sampler.py:135-160) minus the stop-gradiented point: (means, kappas, logits)."""
    vm = vp[..., 0:3] * vmf_scale + 0.0 + noise.to(vp.dtype) * vmf_scale / 2.0 - pts.detach()[..., None, :]
    kap = jmin(mathx.softplus(vp[..., 3] + 1.0), 50.0)
    lg = jmax(vp[..., 4] + 1.0, -50.0)
    return vm, kap, lg


def vmf_loss(vm, kap, lg, dirs, normals, pdf, weight, rgb, lossmult, srgb: bool = True):
    """vmf_loss_fn for one suffix: dirs / rgb [N, K, 3], pdf / weight [N, K], normals [N, 3], lossmult [N] (the
    light_sampling caller's lossmult / K is applied here)."""
    dirs, normals, pdf, weight, rgb, lossmult = (t.detach() for t in (dirs, normals, pdf, weight, rgb, lossmult))
    K = dirs.shape[1]
    means = l2_normalize(vm, grad_eps=1e-5)
    w_exp = safe_exp(lg)
    like = (w_exp[:, None, :] * eval_vmf(dirs[:, :, None, :], means[:, None, :, :], kap[:, None, :])).sum(-1)
    den = torch.clamp(pdf, min=1e-2)
    dot = (dirs * normals[:, None, :]).sum(-1)
    w = torch.clamp(weight, 0.0, 10.0)
    w = torch.where(dot > 0.0, w, torch.zeros_like(w))
    f = torch.linalg.norm(mathx.nan_to_num(rgb), dim=-1)
    f = torch.clamp(f, min=1e-5)
    lk = jmax(like, 1e-5)
    if srgb:
        f, lk = linear_to_srgb(f), linear_to_srgb(lk)
    lm = (lossmult[:, None] * torch.ones_like(pdf)) / K
    return torch.mean((f - lk) * (f - lk).detach() * w * lm / den)


def light_sampling_loss(vm, kap, lg, spec, diff, lossmult, mult: float = 1.0, srgb: bool = True):
    """train_utils.light_sampling_loss: spec / diff = dict(dirs, pdf, weight, rgb) of the two suffixes, normals shared."""
    out = 0.0
    for s in (diff, spec):          # the reference's suffix order
        out = out + vmf_loss(vm, kap, lg, s["dirs"], s["normals"], s["pdf"], s["weight"], s["rgb"], lossmult, srgb) / 2.0
    return mult * out


def split_samples(sec_dirs, sec_samples, sec_rgb, normals, n: int, Ks: int, Kd: int, dtype=torch.float64):
    """The forward's buffers (sec_dirs / sec_rgb [n Ks | n Kd][3], sec_samples [n][Ks + Kd][5]) -> the two suffixes."""
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    K = Ks + Kd
    d = t(sec_dirs).reshape(-1, 3)
    c = t(sec_rgb).reshape(-1, 3)
    sm = t(sec_samples).reshape(n, K, 5)
    nr = t(normals).reshape(n, 3)
    spec = dict(dirs=d[: n * Ks].reshape(n, Ks, 3), rgb=c[: n * Ks].reshape(n, Ks, 3), pdf=sm[:, :Ks, 3],
                weight=sm[:, :Ks, 4], normals=nr)
    diff = dict(dirs=d[n * Ks:].reshape(n, Kd, 3), rgb=c[n * Ks:].reshape(n, Kd, 3), pdf=sm[:, Ks:, 3],
                weight=sm[:, Ks:, 4], normals=nr)
    return spec, diff


def loop_loss(vm, kap, lg, spec, diff, lossmult, mult=1.0, srgb=True):
    """The reference's expression as plain loops over points, samples and lobes (float64, no torch ops): a check of
    vmf_loss / light_sampling_loss's vectorised form."""
    def s_(x):
        return 323.0 / 25.0 * x if x <= 0.0031308 else (211.0 * max(FLT_EPS, x) ** (5.0 / 12.0) - 11.0) / 200.0
    vm, kap, lg = (np.asarray(a.detach(), np.float64) for a in (vm, kap, lg))
    total = 0.0
    for s in (diff, spec):
        dirs, pdf, weight, rgb, nrm = (np.asarray(s[k], np.float64) for k in ("dirs", "pdf", "weight", "rgb", "normals"))
        N, K = pdf.shape
        acc = 0.0
        for r in range(N):
            for k in range(K):
                like = 0.0
                for j in range(vm.shape[1]):
                    m = vm[r, j] / math.sqrt(max(TINY, float(vm[r, j] @ vm[r, j])))
                    kp = kap[r, j]
                    if kp <= FLT_EPS:
                        v = 1.0 / (4.0 * math.pi)
                    else:
                        v = kp * math.exp(min(kp * float(dirs[r, k] @ m), 80.0)) / (4 * math.pi * math.sinh(kp))
                    like += math.exp(min(lg[r, j], 80.0)) * v
                f = max(math.sqrt(float(rgb[r, k] @ rgb[r, k])), 1e-5)
                lk = max(like, 1e-5)
                if srgb:
                    f, lk = s_(f), s_(lk)
                w = min(max(weight[r, k], 0.0), 10.0) if float(dirs[r, k] @ nrm[r]) > 0.0 else 0.0
                acc += (f - lk) ** 2 * w * (float(lossmult[r]) / K) / max(pdf[r, k], 1e-2)
        total += acc / (N * K) / 2.0
    return mult * total


def light_layout(cfg):
    """The light layout's (name, shape) in order: light_grid tables, then layers_0, layers_1, output_layer."""
    from nrc_amd import weights as W
    return [(k, tuple(v)) for k, v in W.param_shapes(cfg, ("light",)).items() if k.startswith(f"{P}LightSampler/")]
