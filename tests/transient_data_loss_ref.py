"""Torch restatement of the time-resolved cache's data loss, for the CPU and GPU tests of
rc_transient_data_backward.  Test helper, not a test module.

  data loss    train_utils.compute_transient_data_loss (internal/train_utils.py:531-640) as
               configs/transient_simulation_ngp_yobo_cornell.gin:51-64 resolves it: loss type 'rawnerf_transient_unbiased'
               (_select_transient_data_loss_function, :725-732) =
                 compute_unbiased_loss_rawnerf_transient (:200-219)
                 + compute_unbiased_loss_rawnerf_transient_gauss (:244-263) * data_loss_gauss_mult / n_bins, summed over its
                   bin axis and broadcast back over the bins (:730-732);
               compute_unbiased_loss (:108-125) and compute_unbiased_loss_transient_gauss (:152-171): 2 (rgb - gt)
               sg(rgb_nocorr - gt_nocorr), the latter on dtof_to_gauss of both differences; the nocorr pair defaults to rgb, gt
               (:604-610); the scale 1 / (sg(sum_bins c) ** exponent + eps) per ray and channel (:217, :261) with c from
               _get_rgb_clip_for_rawnerf (:369-393).  The cache stage's rendering is the TransientVolumeIntegrator's own
               dict, which has no "cache_rgb" key (oracle.transient_ref.transient_integrate lists its keys): c is built
               from the pass's own rgb (:387), then combined with gt (use_combined_rawnerf, configs.py:588);
               render_utils.dtof_to_gauss (internal/inverse_render/render_utils.py:1678-1696) with
               transient_gauss_sigma_scales = [] is its constant row: sum over the bins times constant_scale, ONE row, so
               "/ n_bins, sum over the rows, broadcast over n_bins bins, sum over the bins" counts it once;
               lossmult is zeroed per ray and channel where any bin of gt exceeds loss_thresh (:586-590); the final form is
               (lossmult * data_loss).sum(-2).mean() (:628); the mses stat (:601, :631) is returned beside it.
  forward      oracle.transient_ref: proposal sampler -> transient_shader -> transient_integrate, the three stages of
               transient_forward in its order, use_occlusions = False (the training gin).  The gradient reading is §4.7's and
               §4.8's: sample positions, tdist, means and with them every travel time and time shift carry no gradient --
               here the compositing weights and direct_rgb enter the integrator as leaves, and the inputs of the two head
               layers and the tint pre-activation are cut into leaves inside the shader (a wrapper around
               transient_ref.dense), so autograd gives exactly the adjoints the device call leaves in its workspace.

JAX rules: jnp.clip ties pass half (jax_rules); the forward's clamps are torch.clamp inside the oracle, whose ties (a
zero_invalid_bins zero clamped at 0) sit behind a `where` that stops the gradient either way.
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

import nrc_amd
from jax_rules import jmaximum, jminimum
from nrc_amd.config import TransientDataLossConfig
from oracle import cache_ref, transient_ref

HEAD_IRR = "params/Cache/Shader/transient_indirect_layer"
HEAD_SLF = "params/Cache/Shader/SurfaceLightField/output_rgba_layer"
HEAD_TENSORS = (HEAD_IRR + "/kernel", HEAD_IRR + "/bias", HEAD_SLF + "/kernel", HEAD_SLF + "/bias")


def jclip(x, lo: float, hi: float):
    return jminimum(jmaximum(x, torch.full_like(x, lo)), torch.full_like(x, hi))


def rgb_clip(rgb, gt, cfg):
    """_get_rgb_clip_for_rawnerf (:369-393) on a rendering without "cache_rgb" (use_norm_rawnerf False)."""
    if cfg.use_gt_rawnerf:
        return jclip(gt, 0.0, cfg.clip_val)
    c = jclip(rgb, 0.0, cfg.clip_val)
    if cfg.use_combined_rawnerf:
        c = jclip(jmaximum(c, gt), 0.0, cfg.clip_val)
    return c


def dtof_to_gauss(x, cfg):
    """render_utils.dtof_to_gauss with sigma_scales = []: the constant row [.., 1, 3]."""
    assert not tuple(cfg.transient_gauss_sigma_scales)
    return x.sum(-2, keepdim=True) * cfg.transient_gauss_constant_scale


def data_loss(rgb, gt, rgb_nocorr=None, gt_nocorr=None, lossmult=None, cfg: TransientDataLossConfig = TransientDataLossConfig()):
    """rgb, gt [n, n_bins, 3]; lossmult [n] or None -> (loss, mse), both times data_loss_mult (losses["data"],
    train_utils.py:2917; stats["mses"], :631)."""
    n_bins = rgb.shape[-2]
    lm = torch.ones_like(gt[:, 0, :]) if lossmult is None else lossmult[:, None].expand(-1, 3)
    lm = torch.where((gt > cfg.loss_thresh).sum(-2) > 0, torch.zeros_like(lm), lm)               # :586-590
    mse = (lm[:, None, :] * (rgb - gt) ** 2).sum(-2).mean()                                       # :599-601
    rn = rgb if rgb_nocorr is None else rgb_nocorr                                                # :604-610
    gn = gt if gt_nocorr is None else gt_nocorr
    scale = 1.0 / (torch.pow(rgb_clip(rgb, gt, cfg).detach().sum(-2)[:, None, :], cfg.rawnerf_exponent) + cfg.rawnerf_eps)
    main = 2.0 * (rgb - gt) * (rn - gn).detach() * scale                                          # :200-219
    gauss = 2.0 * dtof_to_gauss(rgb - gt, cfg) * dtof_to_gauss(rn - gn, cfg).detach() * scale     # :244-263
    gauss = gauss * cfg.data_loss_gauss_mult / n_bins                                             # :728-731
    dl = main + gauss.sum(-2, keepdim=True)                                                       # :732
    loss = (lm[:, None, :] * dl).sum(-2).mean()                                                   # :628
    return cfg.data_loss_mult * loss, cfg.data_loss_mult * mse


def loop_loss(rgb, gt, rgb_nocorr=None, gt_nocorr=None, lossmult=None, cfg: TransientDataLossConfig = TransientDataLossConfig()):
    """The same two numbers as plain loops over rays, channels and bins (floats)."""
    rgb, gt = np.asarray(rgb, np.float64), np.asarray(gt, np.float64)
    rn = rgb if rgb_nocorr is None else np.asarray(rgb_nocorr, np.float64)
    gn = gt if gt_nocorr is None else np.asarray(gt_nocorr, np.float64)
    n, B, _ = rgb.shape
    tot = tot_mse = 0.0
    for i in range(n):
        for c in range(3):
            lm = 1.0 if lossmult is None else float(lossmult[i])
            if any(gt[i, b, c] > cfg.loss_thresh for b in range(B)):
                lm = 0.0
            csum = 0.0
            for b in range(B):
                v = min(max(rgb[i, b, c], 0.0), cfg.clip_val)
                if cfg.use_gt_rawnerf:
                    v = min(max(gt[i, b, c], 0.0), cfg.clip_val)
                elif cfg.use_combined_rawnerf:
                    v = min(max(max(v, gt[i, b, c]), 0.0), cfg.clip_val)
                csum += v
            s = 1.0 / (csum ** cfg.rawnerf_exponent + cfg.rawnerf_eps)
            sd = sum(rgb[i, b, c] - gt[i, b, c] for b in range(B)) * cfg.transient_gauss_constant_scale
            sdn = sum(rn[i, b, c] - gn[i, b, c] for b in range(B)) * cfg.transient_gauss_constant_scale
            row = 2.0 * sd * sdn * s * cfg.data_loss_gauss_mult / B
            for b in range(B):
                tot += lm * (2.0 * (rgb[i, b, c] - gt[i, b, c]) * (rn[i, b, c] - gn[i, b, c]) * s + row)
                tot_mse += lm * (rgb[i, b, c] - gt[i, b, c]) ** 2
    return cfg.data_loss_mult * tot / (3 * n), cfg.data_loss_mult * tot_mse / (3 * n)


# ---- the integrator's two linear maps and their transposes as explicit gathers (no autograd) ------------------------

def shift_direct_T(dists, G, n_bins):
    """Transpose of transient_ref.shift_direct w.r.t. val = weights * direct_rgb: G [n, n_bins, 3] -> [n, S, 3], each sample
    gathering its two bins of the flattened [n * n_bins] histogram (the next ray's for bins >= n_bins, nothing past the
    end)."""
    n, S = dists.shape
    low = torch.clamp(torch.floor(dists), min=0.0)
    high = torch.ceil(dists)
    w_high = dists - low
    w_low = 1.0 - w_high
    flat = G.reshape(n * n_bins, 3)
    base = (torch.arange(n) * n_bins)[:, None]

    def take(idx):
        idx = base + idx.to(torch.int64)
        ok = (idx >= 0) & (idx < n * n_bins)
        v = flat[torch.clamp(idx, 0, n * n_bins - 1)]
        return torch.where(ok[..., None], v, torch.zeros_like(v))
    return take(low) * w_low[..., None] + take(high) * w_high[..., None]


def shift_map_coordinates_T(G, d, n_bins):
    """Transpose of transient_ref.shift_map_coordinates: G [N, n_bins, 3], d [N] (bins) -> [N, n_bins, 3]; source bin i
    gathers from the targets y whose interpolation reads it: i0(y) = i with weight 1 - f(y), i0(y) + 1 = i with f(y)."""
    y = torch.arange(n_bins, dtype=G.dtype)[None, :] - d[:, None]
    i0 = torch.floor(y)
    f = y - i0
    i0 = i0.long()
    out = torch.zeros_like(G)
    for idx, w in ((i0, 1.0 - f), (i0 + 1, f)):
        ok = (idx >= 0) & (idx < n_bins)
        contrib = torch.where(ok[..., None], G * w[..., None], torch.zeros_like(G))
        out.scatter_add_(1, torch.clamp(idx, 0, n_bins - 1)[..., None].expand(-1, -1, 3), contrib)
    return out


# ---- the chain: forward with leaves, loss, autograd -----------------------------------------------------------------

@contextlib.contextmanager
def _tapped_dense(taps):
    orig = transient_ref.dense

    def dense(weights, path, x):
        if path.endswith("transient_indirect_layer") or path.endswith("SurfaceLightField/output_rgba_layer"):
            x = x.detach().requires_grad_(True)
            taps["x_irr" if path.endswith("transient_indirect_layer") else "x_slf"] = x
        y = orig(weights, path, x)
        if path.endswith("/tint_layer"):
            y = y.detach().requires_grad_(True)
            taps["tint_raw"] = y
        return y
    transient_ref.dense = dense
    try:
        yield
    finally:
        transient_ref.dense = orig


def forward(weights, cfg, rays, jitters=None):
    """-> (rgb [n, n_bins, 3], taps): the oracle's three stages with the leaves of the module docstring.  `weights`: torch
    dict whose four HEAD_TENSORS may require grad."""
    with torch.no_grad():
        history = cache_ref.proposal_sampler(weights, cfg, rays, jitters, False, True, False)
        filtered, _ = cache_ref.maybe_resample(cfg, history[-1], False)
    taps = {}
    with _tapped_dense(taps):
        sh = dict(transient_ref.transient_shader(weights, cfg, rays, filtered, None))
    for k in ("weights", "direct_rgb"):
        sh[k] = sh[k].detach().requires_grad_(True)
        taps[k] = sh[k]
    taps["shader"] = sh
    integ = transient_ref.transient_integrate(cfg, sh)
    return integ["rgb"], taps


def near_tie_samples(cfg, rays, sh, rel=8 * 1.1920929e-07):
    """[n, S] bool: samples with a zero_invalid_bins comparison within `rel` of equality at some bin (fp32 and fp64 may
    then disagree about a whole bin).  rel = 8 float32 eps: both sides of a comparison are a handful of fp32 operations
    away from the sample position (a difference, a norm, a sum, a product), each worth up to an ulp.  The clamps' ties need no entry: a softplus is never within round-off of 0 unless it
    is killed, and rgb_max is float32 max.  From the restatement's own tensors alone."""
    t = cfg.transient
    means = sh["means"]
    bins = torch.arange(t.n_bins, dtype=means.dtype)
    ld = torch.linalg.norm(rays["lights"][..., None, :] - means, dim=-1)
    cd = (torch.linalg.norm(rays["origins"][..., None, :] - means, dim=-1)
          + torch.linalg.norm(rays["origins"] - rays["cam_origins"], dim=-1)[:, None])
    a = (bins + t.bin_zero_threshold_light) * t.exposure_time
    close = (torch.abs(a[None, None, :] - ld[..., None]) <= rel * ld[..., None]).any(-1)
    md = (t.n_bins - 1) * t.exposure_time
    far = (torch.abs(bins[None, None, :] * t.exposure_time + cd[..., None] - md) <= rel * md).any(-1)
    near = torch.abs(ld - t.light_near) <= rel * t.light_near if t.light_zero else torch.zeros_like(close)
    return close | far | near


def chain(weights_np, rays_np, jitters_np, gt, rgb_nocorr=None, gt_nocorr=None, lossmult=None, dtype=torch.float64,
          cfg=None, loss_cfg: TransientDataLossConfig = TransientDataLossConfig()):
    """Everything rc_transient_data_backward computes, from numpy inputs, in `dtype`: {"loss", "mse", "rgb", "G",
    "grads": {tensor name: array}, "d_t_irr" [n S, 64], "d_t_slf" [n S, 128], "d_tint_ibrdf" [n S, 3], "d_direct" [n S, 3],
    "d_weights" [n S], "near_tie" [n S]}.  gt may be a callable rgb -> gt (a target built from the render)."""
    cfg = nrc_amd.cornell_transient_config() if cfg is None else cfg
    w = {k: torch.from_numpy(np.asarray(v)).to(dtype) if np.asarray(v).dtype.kind == "f" else torch.from_numpy(np.asarray(v))
         for k, v in weights_np.items()}
    for k in HEAD_TENSORS:
        w[k].requires_grad_(True)
    rays = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in rays_np.items()}
    jit = None if jitters_np is None else [torch.from_numpy(np.asarray(j)).to(dtype).reshape(-1, 1) for j in jitters_np]
    rgb, taps = forward(w, cfg, rays, jit)
    rgb.retain_grad()
    tt = lambda x: None if x is None else torch.from_numpy(np.asarray(x)).to(dtype)
    gt_t = tt(gt(rgb.detach().numpy()) if callable(gt) else gt)
    loss, mse = data_loss(rgb, gt_t, tt(rgb_nocorr), tt(gt_nocorr), tt(lossmult), loss_cfg)
    loss.backward()
    sh = taps["shader"]
    tint = torch.sigmoid(taps["tint_raw"].detach())
    d_tint = taps["tint_raw"].grad / (tint * (1.0 - tint))
    ibrdf = sh["tint_ibrdf"].detach() / tint
    # tint * ibrdf is no node of the oracle's graph (it multiplies tint_exp * ibrdf * ref_rgb in one expression), so its
    # adjoint is d tint / ibrdf with d tint = d tint_raw / sigmoid'.  Both divisors are sigmoids of O(1) pre-activations; a
    # saturated one (0 or 1 after rounding) would make this reference 0/0, so it is refused here rather than compared.
    assert float((tint * (1.0 - tint)).min()) > 1e-6 and float(ibrdf.min()) > 1e-6, "saturated tint / ibrdf: no reference"
    out = {"loss": float(loss.detach()), "mse": float(mse.detach()), "rgb": rgb.detach().numpy(), "G": rgb.grad.numpy(),
           "grads": {k: w[k].grad.numpy() for k in HEAD_TENSORS},
           "d_t_irr": taps["x_irr"].grad.reshape(-1, 64).numpy(), "d_t_slf": taps["x_slf"].grad.reshape(-1, 128).numpy(),
           "d_tint_ibrdf": (d_tint / ibrdf).reshape(-1, 3).numpy(), "d_direct": taps["direct_rgb"].grad.reshape(-1, 3).numpy(),
           "d_weights": taps["weights"].grad.reshape(-1).numpy(),
           "near_tie": near_tie_samples(cfg, rays, sh).reshape(-1).numpy()}
    return out
