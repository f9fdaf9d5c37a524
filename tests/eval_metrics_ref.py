"""numpy restatement of the per-view evaluation, for the CPU and GPU tests of rc_eval_image.  Test
helper, not a test module.  Every function takes a `dtype` (np.float64: the reference value; np.float32: the same
arithmetic at the kernels' precision, whose distance from fp64 sets the tolerance of the GPU tests).

  post-process  engine/trainer.py:617-637: p_fn sums a 4-D input over its bin axis and clips binsum / img_scale to
                [0, 1] (:627-629), then image.linear_to_srgb(x * exposure) (internal/image_utils.py:192-198, eps =
                float32's); under clip_eval the post-process is clip(linear_to_srgb(x * exposure), 0, 1) and sums no bins
                (:617-620).  The caller multiplies by the masks before the metrics.
  psnr          image.MetricHarness.__call__ (image_utils.py:464): mse_to_psnr(((pred - gt) ** 2).mean()), the mean over
                all H W 3 values; mse_to_psnr = -10 / ln 10 * ln(mse) (image_utils.py:54-56).
  ssim          dm_pix.ssim at its defaults (max_val 1, filter_size 11, filter_sigma 1.5, k1 0.01, k2 0.03), which
                MetricHarness jits as it is (image_utils.py:426).  dm_pix is not part of the reference tree: the formula
                is restated from its published source and is not pinned against a run of it.
  iou           trainer.py:1633-1636: sum(minimum(pred, gt)) / sum(maximum(pred, gt)) over the raw histograms.
  depth         trainer.py:1766-1779: (|distance - depth| masks).sum() / masks.sum(), plain means without masks.
  normals       trainer.py:1810-1855: normals_gt + (1 - masks), normals + (1 - acc), each normalised or zero where its
                norm is below 1e-5; arccos(clip(dot, -1, 1)) 180 / pi, times masks, np.mean over ALL pixels.

The window is a constant: it is computed in double and rounded once to `dtype` (the library's host code does the same),
and the two passes add their 11 products in tap order, along H first.
"""
from __future__ import annotations

import numpy as np

F32_EPS = np.finfo(np.float32).eps
FILTER_SIZE, FILTER_SIGMA, K1, K2, MAX_VAL = 11, 1.5, 0.01, 0.03, 1.0
SLOTS = ("mse", "psnr", "ssim", "transient_iou", "l1_mean", "l1_median", "mae")


def linear_to_srgb(linear, dtype=np.float64):
    """image_utils.linear_to_srgb with eps = finfo(float32).eps."""
    linear = np.asarray(linear, dtype)
    eps = dtype(F32_EPS)
    srgb0 = dtype(323 / 25) * linear
    srgb1 = (dtype(211) * np.maximum(eps, linear) ** dtype(5 / 12) - dtype(11)) / dtype(200)
    return np.where(linear <= dtype(0.0031308), srgb0, srgb1)


def bin_sums(x, dtype=np.float64):
    """p_fn's x.sum(-2) of [H, W, n_bins, 3]."""
    return np.asarray(x, dtype).sum(-2)


def postprocess(x, exposure=1.0, img_scale=1.0, clip_eval=False, dtype=np.float64):
    """postprocess_fn of an [H, W, 3] image or an [H, W, n_bins, 3] histogram image (clip_eval: images only)."""
    x = np.asarray(x, dtype)
    if x.ndim == 4:
        if clip_eval:
            raise ValueError("clip_eval's post-process does not sum bins")
        x = np.clip(bin_sums(x, dtype) / dtype(img_scale), dtype(0), dtype(1))
    y = linear_to_srgb(x * dtype(exposure), dtype)
    return np.clip(y, dtype(0), dtype(1)) if clip_eval else y


def window(dtype=np.float64):
    """dm_pix.ssim's normalised Gaussian window."""
    f = (np.arange(FILTER_SIZE, dtype=np.float64) - FILTER_SIZE // 2) / FILTER_SIGMA
    w = np.exp(-0.5 * (f * f))
    total = 0.0
    for v in w:
        total += float(v)
    return (w / total).astype(dtype)


def _valid(x, w, axis):
    """Valid correlation of x with w along `axis`, the products added in tap order."""
    n = x.shape[axis] - len(w) + 1
    acc = np.zeros_like(np.take(x, range(n), axis=axis))
    for k, wk in enumerate(w):
        acc = acc + wk * np.take(x, range(k, k + n), axis=axis)
    return acc


def moments(a, b, dtype=np.float64):
    """The five Gaussian moments E[a], E[b], E[a^2], E[b^2], E[ab] over the valid window of [H, W, C] images: the
    separable correlation per channel, along H then W."""
    a, b, w = np.asarray(a, dtype), np.asarray(b, dtype), window(dtype)
    return tuple(_valid(_valid(z, w, 0), w, 1) for z in (a, b, a * a, b * b, a * b))


def ssim(a, b, dtype=np.float64):
    """dm_pix.ssim(a, b) at its defaults -> (ssim, map [H - 10, W - 10, C])."""
    if a.shape[0] < FILTER_SIZE or a.shape[1] < FILTER_SIZE:
        raise ValueError("no valid window")
    mu0, mu1, m00, m11, m01 = moments(a, b, dtype)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    eps2 = dtype(F32_EPS) * dtype(F32_EPS)
    s00 = np.maximum(eps2, m00 - mu00)
    s11 = np.maximum(eps2, m11 - mu11)
    s01 = m01 - mu01
    s01 = np.sign(s01) * np.minimum(np.sqrt(s00 * s11), np.abs(s01))
    c1, c2 = dtype((K1 * MAX_VAL) ** 2), dtype((K2 * MAX_VAL) ** 2)
    numer = (dtype(2) * mu01 + c1) * (dtype(2) * s01 + c2)
    denom = ((mu00 + mu11) + c1) * ((s00 + s11) + c2)
    smap = numer / denom
    return smap.mean(), smap


def mse_to_psnr(mse):
    with np.errstate(divide="ignore"):
        return -10.0 / np.log(10.0) * np.log(mse)


def transient_iou(pred, gt, dtype=np.float64):
    pred, gt = np.asarray(pred, dtype), np.asarray(gt, dtype)
    return np.minimum(pred, gt).sum() / np.maximum(pred, gt).sum()


def depth_l1(distance, depth, mask=None, dtype=np.float64):
    l1 = np.abs(np.asarray(distance, dtype) - np.asarray(depth, dtype))
    if mask is None:
        return l1.mean()
    mask = np.asarray(mask, dtype)
    return (l1 * mask).sum() / mask.sum()


def _shifted_unit(n, shift, dtype):
    n = np.asarray(n, dtype).reshape(-1, 3) + shift.reshape(-1, 1)
    norm = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(norm < dtype(1e-5), np.zeros_like(n), n / norm)


def normal_angles(normals, acc, normals_gt, mask=None, dtype=np.float64):
    """Per-pixel angular error in degrees (times mask), [H W]."""
    acc = np.asarray(acc, dtype).reshape(-1)
    m = np.ones_like(acc) if mask is None else np.asarray(mask, dtype).reshape(-1)
    ng = _shifted_unit(normals_gt, dtype(1) - m, dtype)
    n = _shifted_unit(normals, dtype(1) - acc, dtype)
    dot = (ng[:, 0] * n[:, 0] + ng[:, 1] * n[:, 1]) + ng[:, 2] * n[:, 2]
    deg = np.arccos(np.clip(dot, dtype(-1), dtype(1))) * dtype(180) / dtype(np.pi)
    return deg if mask is None else deg * m


def normal_mae(normals, acc, normals_gt, mask=None, dtype=np.float64):
    return normal_angles(normals, acc, normals_gt, mask, dtype).mean()      # over ALL pixels, as the reference


def evaluate(pred, gt, mask=None, acc=None, normals=None, normals_gt=None, distance_mean=None, distance_median=None,
             depth_gt=None, exposure=1.0, img_scale=1.0, clip_eval=False, skip_postprocess=False, dtype=np.float64):
    """rc_eval_image: {"post_pred", "post_gt", "ssim_map", the SLOTS (NaN where the inputs are missing)}, and for
    histogram inputs "binsum_pred" / "binsum_gt"."""
    pred, gt = np.asarray(pred, dtype), np.asarray(gt, dtype)
    out = {k: float("nan") for k in SLOTS}
    if pred.ndim == 4:
        out["binsum_pred"], out["binsum_gt"] = bin_sums(pred, dtype), bin_sums(gt, dtype)
        out["transient_iou"] = transient_iou(pred, gt, dtype)
    post = (lambda x: x) if skip_postprocess else (lambda x: postprocess(x, exposure, img_scale, clip_eval, dtype))
    p, g = post(pred), post(gt)
    if mask is not None:
        m = np.asarray(mask, dtype).reshape(p.shape[:2] + (1,))
        p, g = p * m, g * m
    out["post_pred"], out["post_gt"] = p, g
    out["mse"] = ((p - g) ** 2).mean()
    out["psnr"] = mse_to_psnr(out["mse"])
    out["ssim"], out["ssim_map"] = ssim(p, g, dtype)
    if depth_gt is not None and distance_mean is not None:
        out["l1_mean"] = depth_l1(distance_mean, depth_gt, mask, dtype)
    if depth_gt is not None and distance_median is not None:
        out["l1_median"] = depth_l1(distance_median, depth_gt, mask, dtype)
    if normals is not None:
        out["mae"] = normal_mae(normals, acc, normals_gt, mask, dtype)
    return out


def both(*args, **kw):
    """(fp64, fp32) results of evaluate."""
    return evaluate(*args, dtype=np.float64, **kw), evaluate(*args, dtype=np.float32, **kw)
