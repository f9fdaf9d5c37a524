"""Evaluation of a rendered view on the device (rc_eval_image; rc_eval_albedo, §4.17).

What the reference's trainer computes per test view -- postprocess_fn (engine/trainer.py:617-637), image.MetricHarness'
PSNR and SSIM (internal/image_utils.py:411-489), the transient IoU (trainer.py:1633-1636), the depth L1 errors
(:1766-1779) and the normals' mean angular error (:1810-1855) -- on images that stay in HBM: the only device-to-host
traffic of a view is the result array.  The albedo metric (_compute_and_log_albedo_metrics, trainer.py:1499-1582, with
the test-set ratio of _compute_albedo_ratio, :2202-2240) is scored the same way: its per-channel median and least squares
run on the device.  The shift-invariant psnr_si / ssim_si (image_utils.py:74-189, rc_eval_shift_invariant, §4.16.1) are
SearchInvariantHarness' and evaluate_view(search_invariant=...)'s.  Not built: LPIPS (a network download).
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, Optional, Sequence, Tuple

from . import rc_ext


class MetricHarness:
    """image_utils.MetricHarness on a RadianceCache: `harness(rgb_pred, rgb_gt, name_fn)` -> {"psnr", "ssim"} of two
    post-processed [H, W, 3] images (cuda tensors, or numpy arrays that are uploaded), compared as they are."""

    def __init__(self, rc=None, disable_ssim: bool = False, disable_lpips: bool = True,
                 disable_search_invariant: bool = True):
        if not disable_lpips:
            raise NotImplementedError("LPIPS is not built (its network is a download): pass disable_lpips=True")
        if not disable_search_invariant:
            raise NotImplementedError("the shift-invariant metrics (psnr_si, ssim_si) are SearchInvariantHarness': pass "
                                      "disable_search_invariant=True")
        self.rc = rc
        self.disable_ssim = bool(disable_ssim)

    def __call__(self, rgb_pred, rgb_gt, name_fn=lambda s: s) -> Dict[str, float]:
        if self.rc is None:
            raise ValueError("MetricHarness needs the RadianceCache it runs on: MetricHarness(rc)")
        r = self.rc.eval_image(rgb_pred, rgb_gt, skip_postprocess=True)
        keys = ("psnr",) if self.disable_ssim else ("psnr", "ssim")
        return {name_fn(k): float(r[k]) for k in keys}


def si_suffix(search_radii, window_halfwidth) -> str:
    """image_utils.MetricHarness' suffix of the shift-invariant keys: "_(4,_4)_8" at the defaults.  search_radii is
    rendered as a tuple, as the reference's default is one."""
    return f" {tuple(rc_ext.search_radii_pair(search_radii))} {window_halfwidth}".replace(" ", "_")


def shift_invariant_mse(rc, img0, img1, search_radii=(4, 4), window_halfwidth: int = 8):
    """image_utils.shift_invariant_mse on a RadianceCache -> (score, opt_di, opt_dj): the float, and the chosen shifts
    as int32 [H, W] cuda tensors.  img0 is the image that is shifted."""
    r = rc.eval_shift_invariant(img0, img1, search_radii, window_halfwidth, ssim=False, keep_maps=True)
    return r["mse"], r["mse_di"], r["mse_dj"]


def shift_invariant_ssim(rc, img0, img1, search_radii=(4, 4), window_halfwidth: int = 8):
    """image_utils.shift_invariant_ssim on a RadianceCache -> (score, opt_di, opt_dj)."""
    r = rc.eval_shift_invariant(img0, img1, search_radii, window_halfwidth, ssim=True, keep_maps=True)
    return r["ssim"], r["ssim_di"], r["ssim_dj"]


class SearchInvariantHarness:
    """image_utils.MetricHarness as the reference constructs it (disable_search_invariant=False, LPIPS off) on a
    RadianceCache: `harness(rgb_pred, rgb_gt, name_fn)` -> {"psnr", "ssim", "psnr_si_(4,_4)_8", "ssim_si_(4,_4)_8"} of two
    post-processed [H, W, 3] images, compared as they are; under disable_ssim only "psnr" and "psnr_si...", as there."""

    def __init__(self, rc, disable_ssim: bool = False, search_radii=(4, 4), window_halfwidth: int = 8):
        if rc is None:
            raise ValueError("SearchInvariantHarness needs the RadianceCache it runs on: SearchInvariantHarness(rc)")
        self.rc = rc
        self.disable_ssim = bool(disable_ssim)
        self.search_radii = rc_ext.search_radii_pair(search_radii)
        self.window_halfwidth = int(window_halfwidth)
        self.si_suffix = si_suffix(search_radii, window_halfwidth)

    def __call__(self, rgb_pred, rgb_gt, name_fn=lambda s: s) -> Dict[str, float]:
        pred, gt = self.rc._dev(rgb_pred), self.rc._dev(rgb_gt)
        plain = self.rc.eval_image(pred, gt, skip_postprocess=True)
        si = self.rc.eval_shift_invariant(pred, gt, self.search_radii, self.window_halfwidth, ssim=not self.disable_ssim)
        out = {"psnr": plain["psnr"]}
        if not self.disable_ssim:
            out["ssim"] = plain["ssim"]
        out["psnr_si" + self.si_suffix] = si["psnr"]
        if not self.disable_ssim:
            out["ssim_si" + self.si_suffix] = si["ssim"]
        return {name_fn(k): float(v) for k, v in out.items()}


def postprocess(rc, x, exposure: float = 1.0, img_scale: float = 1.0, clip_eval: bool = False):
    """The trainer's postprocess_fn of an [H, W, 3] image or an [H, W, n_bins, 3] histogram image -> [H, W, 3] cuda
    tensor.  Runs rc_eval_image of x against itself and keeps its post-processed image, so H and W must be >= 11."""
    return rc.eval_image(x, x, exposure=exposure, img_scale=img_scale, clip_eval=clip_eval, keep_images=True,
                         sync=False)["post_pred"]


# outputs of rc_render_transient that vis.visualize_transient_suite reads (under their names or their cache_ aliases)
_TRANSIENT_VIS_KEYS = ("rgb", "direct_rgb", "indirect_rgb", "diffuse_rgb", "specular_rgb", "albedo_rgb", "occ", "indirect_occ",
                       "irradiance_rgb", "light_radiance_rgb", "n_dot_l_rgb", "direct_diffuse_rgb", "direct_specular_rgb",
                       "indirect_diffuse_rgb", "indirect_specular_rgb", "direct_rgb_viz", "acc", "distance_mean",
                       "distance_median", "normals", "normals_pred")


def _hw(t, n, what):
    if t is None:
        return None
    if t.numel() != n:
        raise ValueError(f"{what} must hold one value per pixel")
    return t


def _slice_randoms(r, i0, i1, total):
    """Rows [i0, i1) of every tensor / array of an explicit randoms dict that holds `total` rows (the padded image); what
    is sized otherwise (a chunk's worth, constants) passes as it is."""
    if isinstance(r, dict):
        return {k: _slice_randoms(v, i0, i1, total) for k, v in r.items()}
    if isinstance(r, (list, tuple)):
        return type(r)(_slice_randoms(v, i0, i1, total) for v in r)
    shape = getattr(r, "shape", None)
    return r[i0:i1] if shape is not None and len(shape) > 0 and shape[0] == total else r


def _render_material(model, fields, names, image, n, passes, rng, every_key=False):
    """The material pass of one view into `image`, chunked as models.render_image chunks it: config.render_chunk_size
    rays, the last chunk edge-padded to a full one, a key split per chunk by prng.chunk_keys; an explicit randoms dict
    that covers the padded image is sliced per chunk.  every_key: every per-ray tensor of the pass is kept (the
    visualisation suite), its image made when the first chunk shows its shape."""
    import torch

    from . import prng

    chunk = int(model.config.render_chunk_size)
    n_chunks = -(-n // chunk)
    total = n_chunks * chunk
    if total > n:                                   # np.pad(mode="edge") of the last chunk
        fields = {k: torch.cat([v, v[-1:].expand(total - n, -1)]) for k, v in fields.items()}
    for c in range(n_chunks):
        i0, i1 = c * chunk, (c + 1) * chunk
        sub = {k: v[i0:i1] for k, v in fields.items()}
        if prng.is_key(rng):
            key, rng = prng.chunk_keys(rng)
        else:
            key = _slice_randoms(rng, i0, i1, total)
        render = model.apply(None, key, sub, passes=tuple(passes))["render"]
        m = min(i1, n) - i0
        if every_key and c == 0:
            for nm, v in render.items():
                if nm not in image and torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == chunk and v.dtype == torch.float32:
                    image[nm] = torch.zeros((n,) + tuple(v.shape[1:]), dtype=torch.float32, device=v.device)
                    names.append(nm)
        for nm in names:
            image[nm][i0: i0 + m].view(m, -1).copy_(render[nm].reshape(chunk, -1)[:m])


def evaluate_view(model, dataset, cam_idx: int, passes: Tuple[str, ...] = ("cache",), masks=None, depth=None,
                  normals=None, exposure: float = 1.0, img_scale: float = 1.0, clip_eval: bool = False, rng=None,
                  gt=None, albedo=None, albedo_ratio=None, albedo_clip: float = 1.0, albedo_pairs=None,
                  visualize: bool = False, search_invariant=None) -> Dict[str, float]:
    """Render camera `cam_idx` of a DeviceDataset with `model` (this package's Model) and score it: the rays of
    generate_ray_batch in chunks of config.render_chunk_size that stay on the device, only the outputs the metrics need,
    then rc_eval_image against dataset.images[cam_idx] (or `gt`).  masks, depth: [H, W]; normals: [H, W, 3] ground
    truth, compared with the rendering's "normals" and "acc".  rng: as Model.apply's (None: the deterministic pass).
    On a time-resolved handle the rendering's rgb is [H, W, n_bins, 3] and `gt` of that shape must be given (the data
    set holds [C, H, W, 3] images); "transient_iou" is then filled.  Returns the metrics as floats (NaN where an input
    was not given) plus "rays_per_sec", the render's rate by device events.

    passes that contain "material" render the material stage (chunked and keyed as models.render_image does, so the
    images equal its images for the same rng bit for bit; rng must be a key or the explicit randoms) and score its "rgb",
    "distance_*", "normals" and "acc".  albedo: [H, W, 3] ground truth; the rendering's "albedo_rgb" (cache pass) or
    "material_albedo" (material pass) is then scored with rc_eval_albedo and "albedo_mse", "albedo_psnr" and
    "albedo_ratio" (the 3 floats that were applied) are added.  albedo_ratio: 3 values (tensor or array, as
    metrics.albedo_ratio returns them) applied instead of this view's own median; albedo_clip: Trainer.albedo_clip;
    albedo_pairs: an rc_ext.AlbedoPairs to which the view's valid rows are appended.

    visualize: the keys the reference's visualisation suite reads are rendered in the same chunk loop and "vis" is added:
    vis.visualize_suite (visualize_transient_suite on a time-resolved handle; vis_material with the material pass) of the
    view as uint8 [H, W, 3] cuda tensors, with `img_scale` as the suite's config.img_scale and the depth pictures masked
    by `masks`.  The scores do not change.

    search_invariant: None, or (search_radii, window_halfwidth): "psnr_si<suffix>" and "ssim_si<suffix>" (si_suffix) of
    the post-processed, masked images that rc_eval_image leaves on the device are added (rc_eval_shift_invariant,
    DESIGN.md §4.16.1); every other key is what None returns."""
    import torch

    from . import vis
    from .model import _CACHE_DEVICE_KEYS, _FINAL_INTEGRATOR_KEYS, _draw_randoms

    passes = tuple(passes)
    material = "material" in passes
    if not material and passes != ("cache",):
        raise NotImplementedError("evaluate_view renders the cache pass (\"cache\",) or the material pass")
    if material and rng is None:
        raise ValueError("the material pass needs randoms: pass rng as a uint32[2] key or as the explicit random tensors")
    rc, cfg = model.rc, model.config
    batch = dataset.generate_ray_batch(cam_idx)
    H, W = dataset.height, dataset.width
    n = H * W
    transient = cfg.transient is not None
    if transient and material:
        raise NotImplementedError("a time-resolved handle has no material pass")
    if transient and albedo is not None:
        raise NotImplementedError("the albedo metric is not defined on a time-resolved handle")
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
    albedo_name = "material_albedo" if material else "albedo_rgb"
    if albedo is not None:
        names += [albedo_name] + (["acc"] if "acc" not in names else [])
    if visualize and not material:
        wanted = _TRANSIENT_VIS_KEYS if transient else _CACHE_DEVICE_KEYS
        names += [k for k in wanted if k not in names]
    dev = f"cuda:{rc.device}"
    table = rc_ext.TRANSIENT_OUTPUTS if transient else rc_ext.OUTPUTS
    ids = rc_ext.TRANSIENT_OUTPUT_ID if transient else rc_ext.OUTPUT_ID

    def tail(nm):
        if nm == "material_albedo":
            return (3,)
        kind = table[ids[nm]][1]
        return (cfg.transient.n_bins, 3) if kind == "bins" else ((3,) if kind == 3 else ())

    image = {nm: torch.zeros((n,) + tail(nm), dtype=torch.float32, device=dev) for nm in names}
    chunk = int(cfg.render_chunk_size)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    if material:
        _render_material(model, fields, names, image, n, passes, rng, every_key=visualize)
    else:
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
    scored = lambda nm, on: image[nm] if on else None          # `visualize` renders more keys than the scores read
    res = rc.eval_image(image["rgb"], truth, mask=dv(masks, "masks"), acc=scored("acc", normals is not None),
                        normals=scored("normals", normals is not None),
                        normals_gt=None if normals is None else rc._dev(normals),
                        distance_mean=scored("distance_mean", depth is not None),
                        distance_median=scored("distance_median", depth is not None),
                        depth_gt=dv(depth, "depth"), exposure=exposure, img_scale=img_scale, clip_eval=clip_eval,
                        shape=shape, keep_images=search_invariant is not None)
    ms = start.elapsed_time(stop)               # the result copy above has synchronised
    res["rays_per_sec"] = n / (ms * 1e-3) if ms > 0 else float("inf")
    if search_invariant is not None:
        radii, halfwidth = search_invariant
        si = rc.eval_shift_invariant(res.pop("post_pred"), res.pop("post_gt"), radii, halfwidth)
        res["psnr_si" + si_suffix(radii, halfwidth)] = si["psnr"]
        res["ssim_si" + si_suffix(radii, halfwidth)] = si["ssim"]
    if albedo is not None:
        a = rc.eval_albedo(image[albedo_name], image["acc"], rc._dev(albedo), mask=dv(masks, "masks"), ratio=albedo_ratio,
                           albedo_clip=albedo_clip, pairs=albedo_pairs, shape=(H, W))
        res.update(albedo_mse=a["mse"], albedo_psnr=a["psnr"], albedo_ratio=a["ratio"])
    if visualize:
        if material:
            rendering = dict(image)
        elif transient:
            rendering = dict(image)
            rendering.update({"cache_" + k: image[k] for k in _FINAL_INTEGRATOR_KEYS if k in image})
            rendering["vignette"] = torch.ones((n, 1), dtype=torch.float32, device=dev)
            rendering["lossmult"] = torch.ones((n, 3), dtype=torch.float32, device=dev)
        else:
            rendering = model._finalize(image, {})
        rendering = {k: v.reshape((H, W) + tuple(v.shape[1:])) for k, v in rendering.items()}
        suite = vis.visualize_transient_suite if transient else vis.visualize_suite
        scales = SimpleNamespace(img_scale=img_scale, var_scale=getattr(cfg, "var_scale", 1.0))
        res["vis"] = suite(rendering, scales, vis_material=material, masks=dv(masks, "masks"), u8=True, rc=rc)
    return res


def pairs_ratio(rc, pairs, correct_median: bool = False, gamma: bool = True):
    """rc_albedo_ratio over an AlbedoPairs -> [1, 3] cuda tensor; raises when more rows were appended than the buffer
    holds (the device then wrote NaN).  Reading the row count for that check is the one readback."""
    ratio = rc.albedo_ratio(pairs, use_median=correct_median, gamma=gamma)
    count = int(pairs.count.item())
    if count > pairs.capacity:
        raise RuntimeError(f"albedo_ratio: {count} valid rows were appended to a buffer of {pairs.capacity}")
    return ratio


def albedo_ratio(model, dataset, albedos, cams: Optional[Sequence[int]] = None, passes: Tuple[str, ...] = ("cache",),
                 masks=None, rng=None, correct_median: bool = False, gamma: bool = True):
    """Trainer._compute_albedo_ratio (engine/trainer.py:2202-2234) on the device: the cameras `cams` (default: every
    tenth, the reference's loop) are rendered and their valid (ground truth, prediction) albedo rows collected in one
    AlbedoPairs of len(cams) H W rows; then ONE rc_albedo_ratio call -- the per-channel median (correct_median,
    Trainer.albedo_correct_median) or the least squares, with Trainer.albedo_gamma.  albedos: [C, H, W, 3] ground truth,
    masks: [C, H, W] or None, indexed by camera; rng: a key is split per camera.  Returns the [1, 3] cuda tensor that
    evaluate_view(albedo_ratio=...) takes.  The overflow check is the function's one readback."""
    from . import prng

    n_cams = int(dataset.images.shape[0])
    cams = list(range(0, n_cams, 10)) if cams is None else [int(c) for c in cams]
    pairs = rc_ext.AlbedoPairs(model.rc, len(cams) * dataset.height * dataset.width)
    for c in cams:
        key = rng
        if prng.is_key(rng):
            key, rng = prng.chunk_keys(rng)
        evaluate_view(model, dataset, c, passes=passes, masks=None if masks is None else masks[c], rng=key,
                      albedo=albedos[c], albedo_pairs=pairs)
    return pairs_ratio(model.rc, pairs, correct_median=correct_median, gamma=gamma)
