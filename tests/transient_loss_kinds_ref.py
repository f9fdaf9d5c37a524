"""Torch restatement of the time-resolved cache's data loss under every loss type of rc_transient_data_backward_kind
(DESIGN.md §4.15), for the CPU and GPU tests.  Test helper, not a test module.

  dtof_to_itof   render_utils.dtof_to_itof (internal/inverse_render/render_utils.py:1648-1676) with jnp's evaluation order in
                 the given dtype: t = linspace(0, T E, T, endpoint=False) / c, then 2 pi f (one Python float) * t + phi, cos /
                 sin, + 1; per pair a cos row and a sin row, then the constant row sum / 2.
  data_loss      train_utils.compute_transient_data_loss (internal/train_utils.py:531-640) with
                 _select_transient_data_loss_function (:686-750) for the eight types of rc_ext.TRANSIENT_LOSS_TYPES: the
                 lossmult zeroing (:586-590), the mses stat in its plain or iToF form (:595-601), the nocorr defaults
                 (:604-610), the selection, "/ shape[-2]" under use_itof (:622-623), (lossmult * data_loss).sum(-2).mean()
                 (:628).  The rawnerf scale and clip are transient_data_loss_ref's.
  loop_loss      the same two numbers as plain loops over rays, channels, bins and rows (floats).
  closed_G       d loss / d rgb by the formulas of DESIGN.md §4.15, no autograd.
  chain_kind     transient_data_loss_ref.chain with this data loss in the place of its own.

exposure_time is the handle's own value: the float32 of TransientConfig.exposure_time (handle_exposure).
"""
from __future__ import annotations

import contextlib
import math

import numpy as np
import torch

import transient_data_loss_ref as tref
from nrc_amd.config import TransientDataLossConfig

C_LIGHT = 299792458
ITOF_TYPES = ("mse_itof", "mse_itof_unbiased", "rawnerf_transient_itof", "rawnerf_transient_itof_unbiased")
UNBIASED = {"rawnerf_transient_unbiased": "rawnerf_transient", "mse_unbiased": "mse", "mse_itof_unbiased": "mse_itof",
            "rawnerf_transient_itof_unbiased": "rawnerf_transient_itof"}
RAWNERF_TYPES = ("rawnerf_transient_unbiased", "rawnerf_transient", "rawnerf_transient_itof", "rawnerf_transient_itof_unbiased")


def handle_exposure(cfg) -> float:
    """The exposure_time a handle of render config `cfg` holds: rc_transient_config's float."""
    return float(np.float32(cfg.transient.exposure_time))


def itof_table(n_bins, pairs, exposure_time, dtype=torch.float64):
    """W [2 P + 1, n_bins] in `dtype`, jnp's order of operations."""
    # jnp.linspace(0, stop, T, endpoint=False) = 0 * (1 - i / T) + stop * (i / T)
    stop = torch.tensor(n_bins * exposure_time, dtype=dtype)
    t = stop * (torch.arange(n_bins, dtype=dtype) / n_bins) / torch.tensor(C_LIGHT, dtype=dtype)
    rows = []
    for f, ph in pairs:
        arg = torch.tensor(2 * np.pi * f, dtype=dtype) * t + torch.tensor(ph, dtype=dtype)
        rows += [torch.cos(arg) + 1.0, torch.sin(arg) + 1.0]
    rows.append(torch.full((n_bins,), 0.5, dtype=dtype))
    return torch.stack(rows)


def dtof_to_itof(x, pairs, exposure_time):
    """x [n, n_bins, 3] -> [n, 2 P + 1, 3] in x's dtype."""
    rows = []
    W = itof_table(x.shape[-2], pairs, exposure_time, x.dtype)
    for r in range(2 * len(pairs)):
        rows.append((W[r][None, :, None] * x).sum(-2, keepdim=True))
    rows.append(x.sum(-2, keepdim=True) / 2.0)
    return torch.cat(rows, -2)


def data_loss(rgb, gt, rgb_nocorr=None, gt_nocorr=None, lossmult=None, cfg: TransientDataLossConfig = TransientDataLossConfig(),
              exposure_time: float = 0.01):
    """rgb, gt [n, n_bins, 3]; lossmult [n] or None -> (loss, mse), both times data_loss_mult."""
    assert not tuple(cfg.transient_gauss_sigma_scales) and not cfg.mask_lossmult and not cfg.clip_eval
    n_bins = rgb.shape[-2]
    pairs = tuple(cfg.itof_frequency_phase_shifts)
    itof = lambda x: dtof_to_itof(x, pairs, exposure_time)
    lm = torch.ones_like(gt[:, 0, :]) if lossmult is None else lossmult[:, None].expand(-1, 3)
    lm = torch.where((gt > cfg.loss_thresh).sum(-2) > 0, torch.zeros_like(lm), lm)               # :586-590
    d = rgb - gt
    if cfg.use_itof:                                                                              # :595-597
        resid = itof(d) ** 2
        resid = resid / resid.shape[-2]
    else:
        resid = d ** 2
    mse = (lm[:, None, :] * resid).sum(-2).mean()                                                 # :601
    rn = rgb if rgb_nocorr is None else rgb_nocorr                                                # :604-610
    gn = gt if gt_nocorr is None else gt_nocorr
    dn = (rn - gn).detach()
    t = cfg.loss_type
    scale = 1.0
    if t in RAWNERF_TYPES:
        scale = 1.0 / (torch.pow(tref.rgb_clip(rgb, gt, cfg).detach().sum(-2)[:, None, :], cfg.rawnerf_exponent) + cfg.rawnerf_eps)
    if t == "mse":                                                                                # :700-702
        dl = d ** 2
    elif t == "mse_unbiased":                                                                     # :709-710
        dl = 2.0 * d * dn
    elif t == "mse_itof":                                                                         # :703-705
        dl = itof(d) ** 2
    elif t == "mse_itof_unbiased":                                                                # :711-712
        dl = 2.0 * itof(d) * itof(dn)
    elif t == "rawnerf_transient":                                                                # :717-724
        gauss = tref.dtof_to_gauss(d, cfg) ** 2 * scale * cfg.data_loss_gauss_mult / n_bins
        dl = d ** 2 * scale + gauss.sum(-2, keepdim=True)
    elif t == "rawnerf_transient_unbiased":                                                       # :725-732
        gauss = 2.0 * tref.dtof_to_gauss(d, cfg) * tref.dtof_to_gauss(dn, cfg) * scale * cfg.data_loss_gauss_mult / n_bins
        dl = 2.0 * d * dn * scale + gauss.sum(-2, keepdim=True)
    elif t == "rawnerf_transient_itof":                                                           # :733-734
        dl = itof(d) ** 2 * scale
    elif t == "rawnerf_transient_itof_unbiased":                                                  # :735-736
        dl = 2.0 * itof(d) * itof(dn) * scale
    else:
        raise ValueError(t)
    if cfg.use_itof:                                                                              # :622-623
        dl = dl / dl.shape[-2]
    loss = (lm[:, None, :] * dl).sum(-2).mean()                                                   # :628
    return cfg.data_loss_mult * loss, cfg.data_loss_mult * mse


def _loop_rows(x, pairs, exposure_time):
    """I_r(x) of one ray and channel: x a list of n_bins floats -> list of 2 P + 1 floats."""
    B = len(x)
    out = []
    for f, ph in pairs:
        for fn in (math.cos, math.sin):
            tot = 0.0
            for b in range(B):
                tb = (B * exposure_time) * (b / B) / C_LIGHT
                tot += (fn(2 * math.pi * f * tb + ph) + 1.0) * x[b]
            out.append(tot)
    out.append(sum(x) / 2.0)
    return out


def loop_loss(rgb, gt, rgb_nocorr=None, gt_nocorr=None, lossmult=None, cfg: TransientDataLossConfig = TransientDataLossConfig(),
              exposure_time: float = 0.01):
    """data_loss' two numbers as plain loops (floats)."""
    rgb, gt = np.asarray(rgb, np.float64), np.asarray(gt, np.float64)
    rn = rgb if rgb_nocorr is None else np.asarray(rgb_nocorr, np.float64)
    gn = gt if gt_nocorr is None else np.asarray(gt_nocorr, np.float64)
    n, B, _ = rgb.shape
    pairs = tuple(cfg.itof_frequency_phase_shifts)
    t = cfg.loss_type
    k = cfg.transient_gauss_constant_scale
    tot = tot_mse = 0.0
    for i in range(n):
        for c in range(3):
            lm = 1.0 if lossmult is None else float(lossmult[i])
            if any(gt[i, b, c] > cfg.loss_thresh for b in range(B)):
                lm = 0.0
            s = 1.0
            if t in RAWNERF_TYPES:
                csum = 0.0
                for b in range(B):
                    v = min(max(rgb[i, b, c], 0.0), cfg.clip_val)
                    if cfg.use_gt_rawnerf:
                        v = min(max(gt[i, b, c], 0.0), cfg.clip_val)
                    elif cfg.use_combined_rawnerf:
                        v = min(max(max(v, gt[i, b, c]), 0.0), cfg.clip_val)
                    csum += v
                s = 1.0 / (csum ** cfg.rawnerf_exponent + cfg.rawnerf_eps)
            d = [rgb[i, b, c] - gt[i, b, c] for b in range(B)]
            dn = [rn[i, b, c] - gn[i, b, c] for b in range(B)]
            Id, Idn = _loop_rows(d, pairs, exposure_time), _loop_rows(dn, pairs, exposure_time)
            if t == "mse":
                rows = [x * x for x in d]
            elif t == "mse_unbiased":
                rows = [2.0 * x * y for x, y in zip(d, dn)]
            elif t == "rawnerf_transient":
                g = (k * sum(d)) ** 2 * s * cfg.data_loss_gauss_mult / B
                rows = [x * x * s + g for x in d]
            elif t == "rawnerf_transient_unbiased":
                g = 2.0 * (k * sum(d)) * (k * sum(dn)) * s * cfg.data_loss_gauss_mult / B
                rows = [2.0 * x * y * s + g for x, y in zip(d, dn)]
            elif t in ("mse_itof", "rawnerf_transient_itof"):
                rows = [x * x * s for x in Id]
            elif t in ("mse_itof_unbiased", "rawnerf_transient_itof_unbiased"):
                rows = [2.0 * x * y * s for x, y in zip(Id, Idn)]
            else:
                raise ValueError(t)
            q = 1.0 / len(rows) if cfg.use_itof else 1.0
            for v in rows:
                tot += lm * v * q
            if cfg.use_itof:
                for x in Id:
                    tot_mse += lm * x * x / len(Id)
            else:
                for x in d:
                    tot_mse += lm * x * x
    return cfg.data_loss_mult * tot / (3 * n), cfg.data_loss_mult * tot_mse / (3 * n)


def closed_G(rgb, gt, rgb_nocorr=None, gt_nocorr=None, lossmult=None, cfg: TransientDataLossConfig = TransientDataLossConfig(),
             exposure_time: float = 0.01):
    """G = d loss / d rgb [n, n_bins, 3] by the closed forms: coef lm q [s] times 2 x_b (+ 2 k^2 gauss_mult sum x for the
    per-bin rawnerf types) or sum_r 2 I_r(x) W_r[b], x = d for a biased type and dn for an unbiased one."""
    n, B, _ = rgb.shape
    t = cfg.loss_type
    lm = torch.ones_like(gt[:, 0, :]) if lossmult is None else lossmult[:, None].expand(-1, 3)
    lm = torch.where((gt > cfg.loss_thresh).sum(-2) > 0, torch.zeros_like(lm), lm)
    rn = rgb if rgb_nocorr is None else rgb_nocorr
    gn = gt if gt_nocorr is None else gt_nocorr
    x = (rn - gn) if t in UNBIASED else (rgb - gt)
    coef = cfg.data_loss_mult / (3 * n)
    s = torch.ones_like(lm)
    if t in RAWNERF_TYPES:
        s = 1.0 / (torch.pow(tref.rgb_clip(rgb, gt, cfg).sum(-2), cfg.rawnerf_exponent) + cfg.rawnerf_eps)
    if t in ITOF_TYPES:
        W = itof_table(B, tuple(cfg.itof_frequency_phase_shifts), exposure_time, rgb.dtype)      # [Nr, B]
        core = torch.einsum("nrc,rb->nbc", 2.0 * torch.einsum("rb,nbc->nrc", W, x), W)
        rows = W.shape[0]
    else:
        core = 2.0 * x
        if t in ("rawnerf_transient", "rawnerf_transient_unbiased"):
            core = core + 2.0 * cfg.transient_gauss_constant_scale ** 2 * cfg.data_loss_gauss_mult * x.sum(-2, keepdim=True)
        rows = B
    q = 1.0 / rows if cfg.use_itof else 1.0
    return coef * q * (lm * s)[:, None, :] * core


def loss_and_G(rgb_np, gt, rgb_nocorr, gt_nocorr, lossmult, cfg, exposure_time, dtype):
    """(loss, mse, G) of data_loss in `dtype` from numpy inputs, G by autograd; returned as float64 numpy."""
    tt = lambda a: None if a is None else torch.from_numpy(np.asarray(a)).to(dtype)
    rgb = tt(rgb_np).requires_grad_(True)
    loss, mse = data_loss(rgb, tt(gt), tt(rgb_nocorr), tt(gt_nocorr), tt(lossmult), cfg, exposure_time)
    loss.backward()
    return float(loss.detach()), float(mse.detach()), rgb.grad.double().numpy()


@contextlib.contextmanager
def _patched_data_loss(exposure_time):
    orig = tref.data_loss
    tref.data_loss = lambda rgb, gt, rn=None, gn=None, lm=None, cfg=TransientDataLossConfig(): data_loss(
        rgb, gt, rn, gn, lm, cfg, exposure_time)
    try:
        yield
    finally:
        tref.data_loss = orig


def chain_kind(weights_np, rays_np, jitters_np, gt, rgb_nocorr=None, gt_nocorr=None, lossmult=None, dtype=torch.float64, cfg=None,
               loss_cfg: TransientDataLossConfig = TransientDataLossConfig()):
    """transient_data_loss_ref.chain (the forward with its leaves, the loss, autograd) under loss_cfg's loss type: chain
    resolves data_loss as a global of its module, which is this module's for the length of the call."""
    import nrc_amd

    cfg = nrc_amd.cornell_transient_config() if cfg is None else cfg
    with _patched_data_loss(handle_exposure(cfg)):
        return tref.chain(weights_np, rays_np, jitters_np, gt, rgb_nocorr, gt_nocorr, lossmult, dtype, cfg=cfg, loss_cfg=loss_cfg)
