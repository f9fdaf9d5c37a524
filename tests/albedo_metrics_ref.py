"""numpy restatement of the albedo evaluation, for the CPU and GPU tests of rc_eval_albedo and
rc_albedo_ratio.  Test helper, not a test module.  Every function takes a `dtype` (np.float64: the reference value;
np.float32: the same arithmetic at the kernels' precision -- the pair rows, the valid count and the median ratio of the
kernels equal it exactly, and its distance from fp64 sets the tolerance of everything else).

  evaluate   Trainer._compute_and_log_albedo_metrics (engine/trainer.py:1499-1567), line by line: the boolean masks, the
             ground truth and the prediction set to 1 outside the mask, the pair rows, the visualisation ratio, the ratio
             applied (the one handed in, else the median of this view), the gamma, the masked mse and its psnr.
  ratio      Trainer._compute_albedo_ratio (:2207-2234) over the collected rows: np.median, or np.linalg.lstsq of the
             literal construction (three stacked copies, zeroed columns).
  closed_form  what that lstsq solves to: its system is block-diagonal.
"""
from __future__ import annotations

import warnings

import numpy as np

SLOTS = ("mse", "psnr")
C = 3                                           # config.num_rgb_channels


def mse_to_psnr(mse):
    with np.errstate(divide="ignore", invalid="ignore"):
        return -10.0 / np.log(10.0) * np.log(mse)


def _median(x):
    """np.median(x, axis=0, keepdims=True) without the warnings of an empty or NaN-holding input."""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return np.median(x, axis=0, keepdims=True)


def evaluate(albedo, acc, albedo_gt, mask=None, ratio=None, albedo_clip=1.0, dtype=np.float64):
    """{"pairs_gt", "pairs_pred" [M, 3], "valid" M, "ratio_im", "post_pred", "post_gt" [H, W, 3], "ratio" [3], "mse",
    "psnr"} of one view; ratio None: the view's own median (trainer.py:1546-1559)."""
    H, W = np.shape(albedo)[:2]
    albedo = np.array(albedo, dtype).reshape(-1, C)
    acc = np.array(acc, dtype).reshape(-1)
    masks = np.ones(H * W, dtype) if mask is None else np.array(mask, dtype).reshape(-1)
    mask = np.repeat((masks > 0.0).reshape(-1, 1), C, axis=-1)
    albedo_mask = mask & (acc[..., None] > 0.5)
    albedo_gt = np.array(albedo_gt, dtype).reshape(-1, C)
    albedo_gt[~mask] = 1
    albedo = (albedo + (dtype(1.0) - acc[..., None])).reshape(-1, C)
    albedo[~mask] = 1.0
    out = {"pairs_gt": albedo_gt[albedo_mask].reshape(-1, C), "pairs_pred": albedo[albedo_mask].reshape(-1, C)}
    out["valid"] = out["pairs_gt"].shape[0]
    with np.errstate(all="ignore"):
        out["ratio_im"] = np.clip((albedo_gt / albedo).reshape(H, W, C), dtype(0.0), dtype(1.0))
        masked_albedo_gt = albedo_gt[albedo_mask].reshape(-1, C)
        masked_albedo = albedo[albedo_mask].reshape(-1, C)
        if ratio is not None:
            used = np.asarray(ratio, dtype).reshape(1, C)
        else:
            used = _median(masked_albedo_gt / np.clip(masked_albedo, dtype(1e-6), dtype(1.0)))
        albedo[albedo_mask] = np.clip(masked_albedo * used, dtype(0.0), dtype(albedo_clip)).reshape(-1)
        albedo_gt = albedo_gt ** dtype(1.0 / 2.2)
        albedo = albedo ** dtype(1.0 / 2.2)
        m = masks.reshape(-1, 1)
        mse = ((albedo * m - albedo_gt * m) ** 2).mean()
    out.update(ratio=used.reshape(C), post_pred=albedo.reshape(H, W, C), post_gt=albedo_gt.reshape(H, W, C), mse=mse,
               psnr=mse_to_psnr(mse))
    return out


def both(*args, **kw):
    """(fp64, fp32) results of evaluate."""
    return evaluate(*args, dtype=np.float64, **kw), evaluate(*args, dtype=np.float32, **kw)


def ratio(all_albedo_gt, all_albedo_pred, use_median, gamma=True, dtype=np.float64):
    """_compute_albedo_ratio's ratio [1, 3] of the lists of per-view rows."""
    all_gt = [np.asarray(x, dtype) for x in all_albedo_gt]
    all_pred = [np.asarray(x, dtype) for x in all_albedo_pred]
    with np.errstate(all="ignore"):
        if use_median:
            gt, pred = np.concatenate(all_gt, axis=0), np.concatenate(all_pred, axis=0)
            return _median(gt / np.clip(pred, dtype(1e-6), dtype(1.0)))
        pred = np.concatenate(all_pred + all_pred + all_pred, axis=0)
        gt = np.transpose(np.concatenate(all_gt, axis=0), (1, 0)).reshape(-1)
        temp = np.copy(pred)
        temp[0 * temp.shape[0] // 3:1 * temp.shape[0] // 3, 0] = 0
        temp[1 * temp.shape[0] // 3:2 * temp.shape[0] // 3, 1] = 0
        temp[2 * temp.shape[0] // 3:3 * temp.shape[0] // 3, 2] = 0
        pred = pred - temp
        if gamma:
            pred = pred ** dtype(1.0 / 2.2)
            gt = gt ** dtype(1.0 / 2.2)
        r = np.linalg.lstsq(pred, gt, rcond=None)[0].reshape(-1, 3)
        if gamma:
            r = r ** dtype(2.2)
    return r


def closed_form(all_albedo_gt, all_albedo_pred, gamma=True):
    """The solution of that block-diagonal system in fp64: per channel sum(p g) / sum(p p) of the (gamma-corrected) rows."""
    g = np.concatenate([np.asarray(x, np.float64) for x in all_albedo_gt], axis=0)
    p = np.concatenate([np.asarray(x, np.float64) for x in all_albedo_pred], axis=0)
    if gamma:
        g, p = g ** (1.0 / 2.2), p ** (1.0 / 2.2)
    r = (p * g).sum(0) / (p * p).sum(0)
    return (r ** 2.2 if gamma else r).reshape(1, 3)
