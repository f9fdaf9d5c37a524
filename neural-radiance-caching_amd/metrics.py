"""Evaluation of a rendered view on the device (rc_eval_image).

What the reference's trainer computes per test view -- postprocess_fn (engine/trainer.py:617-637), image.MetricHarness'
PSNR and SSIM (internal/image_utils.py:411-489), the transient IoU (trainer.py:1633-1636), the depth L1 errors
(:1766-1779) and the normals' mean angular error (:1810-1855) -- on images that stay in HBM: the only device-to-host
traffic of a view is the result array.  Not built: LPIPS (a network download), the shift-invariant variants (off in the
reference's eval config, configs.py:846) and the albedo PSNR.
"""
from __future__ import annotations

from typing import Dict, Tuple

from . import rc_ext


class MetricHarness:
    """image_utils.MetricHarness on a RadianceCache: `harness(rgb_pred, rgb_gt, name_fn)` -> {"psnr", "ssim"} of two
    post-processed [H, W, 3] images (cuda tensors, or numpy arrays that are uploaded), compared as they are."""

    def __init__(self, rc=None, disable_ssim: bool = False, disable_lpips: bool = True,
                 disable_search_invariant: bool = True):
        if not disable_lpips:
            raise NotImplementedError("LPIPS is not built (its network is a download): pass disable_lpips=True")
        if not disable_search_invariant:
            raise NotImplementedError("the shift-invariant metrics (psnr_si, ssim_si) are not built: pass "
                                      "disable_search_invariant=True")
        self.rc = rc
        self.disable_ssim = bool(disable_ssim)

    def __call__(self, rgb_pred, rgb_gt, name_fn=lambda s: s) -> Dict[str, float]:
        if self.rc is None:
            raise ValueError("MetricHarness needs the RadianceCache it runs on: MetricHarness(rc)")
        r = self.rc.eval_image(rgb_pred, rgb_gt, skip_postprocess=True)
        keys = ("psnr",) if self.disable_ssim else ("psnr", "ssim")
        return {name_fn(k): float(r[k]) for k in keys}


def postprocess(rc, x, exposure: float = 1.0, img_scale: float = 1.0, clip_eval: bool = False):
    """The trainer's postprocess_fn of an [H, W, 3] image or an [H, W, n_bins, 3] histogram image -> [H, W, 3] cuda
    tensor.  Runs rc_eval_image of x against itself and keeps its post-processed image, so H and W must be >= 11."""
    return rc.eval_image(x, x, exposure=exposure, img_scale=img_scale, clip_eval=clip_eval, keep_images=True,
                         sync=False)["post_pred"]


def _hw(t, n, what):
    if t is None:
        return None
    if t.numel() != n:
        raise ValueError(f"{what} must hold one value per pixel")
    return t


def evaluate_view(model, dataset, cam_idx: int, passes: Tuple[str, ...] = ("cache",), masks=None, depth=None,
                  normals=None, exposure: float = 1.0, img_scale: float = 1.0, clip_eval: bool = False, rng=None,
                  gt=None) -> Dict[str, float]:
    """Render camera `cam_idx` of a DeviceDataset with `model` (this package's Model) and score it: the rays of
    generate_ray_batch in chunks of config.render_chunk_size that stay on the device, only the outputs the metrics need,
    then rc_eval_image against dataset.images[cam_idx] (or `gt`).  masks, depth: [H, W]; normals: [H, W, 3] ground
    truth, compared with the rendering's "normals" and "acc".  rng: as Model.apply's (None: the deterministic pass).
    On a time-resolved handle the rendering's rgb is [H, W, n_bins, 3] and `gt` of that shape must be given (the data
    set holds [C, H, W, 3] images); "transient_iou" is then filled.  Returns the metrics as floats (NaN where an input
    was not given) plus "rays_per_sec", the render's rate by device events."""
    import torch

    from .model import _draw_randoms

    if tuple(passes) != ("cache",):
        raise NotImplementedError("evaluate_view renders the cache pass only")
    rc, cfg = model.rc, model.config
    batch = dataset.generate_ray_batch(cam_idx)
    H, W = dataset.height, dataset.width
    n = H * W
    transient = cfg.transient is not None
    if transient and gt is None:
        raise ValueError("a time-resolved handle renders [H, W, n_bins, 3]: pass the ground truth histograms as gt")
    fields = {k: v.reshape(n, -1) for k, v in batch.rays.hot_fields().items() if v is not None and k != "lossmult"}
    if not transient:
        fields.pop("cam_origins", None)
    names = ["rgb"]
    if depth is not None:
        names += ["distance_mean", "distance_median"]
    if normals is not None:
        names += ["normals", "acc"]
    dev = f"cuda:{rc.device}"
    table = rc_ext.TRANSIENT_OUTPUTS if transient else rc_ext.OUTPUTS
    ids = rc_ext.TRANSIENT_OUTPUT_ID if transient else rc_ext.OUTPUT_ID

    def tail(nm):
        kind = table[ids[nm]][1]
        return (cfg.transient.n_bins, 3) if kind == "bins" else ((3,) if kind == 3 else ())

    image = {nm: torch.zeros((n,) + tail(nm), dtype=torch.float32, device=dev) for nm in names}
    chunk = int(cfg.render_chunk_size)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        sub = {k: v[i0:i1] for k, v in fields.items()}
        randoms, rng = _draw_randoms(rng, i1 - i0, cfg, False)
        if transient:
            res = rc.render_transient(sub, randoms, outputs=names)
            for nm in names:
                image[nm][i0:i1].copy_(res[nm])
        else:
            rc.render_rays(sub, randoms, out={nm: image[nm][i0:i1] for nm in names})
    stop.record()
    truth = batch.rgb if gt is None else rc._dev(gt)
    shape = (H, W, cfg.transient.n_bins) if transient else (H, W)
    dv = lambda x, what: None if x is None else _hw(rc._dev(x), n, what)
    res = rc.eval_image(image["rgb"], truth, mask=dv(masks, "masks"), acc=image.get("acc"), normals=image.get("normals"),
                        normals_gt=None if normals is None else rc._dev(normals),
                        distance_mean=image.get("distance_mean"), distance_median=image.get("distance_median"),
                        depth_gt=dv(depth, "depth"), exposure=exposure, img_scale=img_scale, clip_eval=clip_eval,
                        shape=shape)
    ms = start.elapsed_time(stop)               # the result copy above has synchronised
    res["rays_per_sec"] = n / (ms * 1e-3) if ms > 0 else float("inf")
    return res
