"""The reference's visualisation suite on the device: vis.weighted_percentile, visualize_cmap,
visualize_suite and visualize_transient_suite (internal/vis.py:50-137, 319-743) and the 8-bit form of utils.save_img_u8
(internal/utils.py:394-400), on images that stay in HBM.

A suite of one view is a handful of calls: rc_image_max once per image that another one is divided by, rc_weighted_percentile
once per depth picture (the bounds of all of them come from distance_median; each picture's own percentiles only replace a
bound that is exactly 0, which Python's `lo or ...` treats as missing) and ONE rc_vis_images for every picture.

An entry is left out when the rendering lacks its source key (the reference draws zeros or ones for some of them and
raises a KeyError for the others).  This package renders no cache_incoming_* (slf_rgb, slf_rgb0, slf_depth, slf_acc),
irradiance_cache (color_irradiance_cache), lighting_irradiance (material_lighting_irradiance), rgb_variance (color_var) and,
outside the time-resolved cache, no cache_occ; the passive cache has no env map picture unless "cache_env_map_rgb" is
handed in.  transient_plot (a matplotlib figure) and vis_depth_triplet (computed and never returned by the reference) are
not built.  Every picture is [H, W, 3]: the reference's one-channel entries ("acc") are broadcast.
"""
from __future__ import annotations

import os
from typing import Dict

from . import rc_ext

# (vis key, source key) of the entries that are linear_to_srgb of a rendered colour as it is
_SRGB = (
    ("cache_ambient_color", "cache_ambient_rgb"), ("cache_albedo_color", "cache_albedo_rgb"),
    ("cache_ambient_diffuse_color", "cache_ambient_diffuse_rgb"),
    ("cache_ambient_specular_color", "cache_ambient_specular_rgb"),
)
# ... and of those the transient suite first divides by config.img_scale
_SRGB_SCALED = (
    ("cache_diffuse_color", "cache_diffuse_rgb"), ("cache_specular_color", "cache_specular_rgb"),
    ("cache_direct_color", "cache_direct_rgb"), ("cache_indirect_color", "cache_indirect_rgb"),
    ("cache_direct_diffuse_color", "cache_direct_diffuse_rgb"), ("cache_direct_specular_color", "cache_direct_specular_rgb"),
    ("cache_indirect_diffuse_color", "cache_indirect_diffuse_rgb"),
    ("cache_indirect_specular_color", "cache_indirect_specular_rgb"),
)
# the material stage's colours (vis_material, only when the rendering holds "material_rgb")
_MATERIAL_SRGB = (
    ("material_diffuse_color", "diffuse_rgb"), ("material_specular_color", "specular_rgb"),
    ("material_direct_color", "direct_rgb"), ("material_indirect_color", "indirect_rgb"),
    ("material_direct_diffuse_color", "direct_diffuse_rgb"), ("material_direct_specular_color", "direct_specular_rgb"),
    ("material_indirect_diffuse_color", "indirect_diffuse_rgb"), ("material_indirect_specular_color", "indirect_specular_rgb"),
)
_MATERIAL_MATTE = ("material_roughness", "material_F_0", "material_metalness", "material_diffuseness", "material_mirrorness")


def weighted_percentile(rc, x, w, ps):
    """vis.weighted_percentile(x, w, ps) -> float64 cuda tensor [len(ps)] (rc_weighted_percentile)."""
    return rc.weighted_percentile(x, w, ps)


def _hw(rendering):
    acc = rendering["acc"]
    return int(acc.shape[0]), int(acc.shape[1])


def visualize_cmap(rc, value, weight, lo=None, hi=None, percentile: float = 99.0, mask=None, u8: bool = False):
    """vis.visualize_cmap(value, weight, cm.get_cmap("turbo"), lo, hi, percentile, curve_fn=-log(x + eps)) of one [H, W]
    image -> [H, W, 3] cuda tensor (float32, or uint8 with u8).  lo, hi: None, a number, or a float64 cuda tensor [2] as
    `lo` holding both bounds (what weighted_percentile returns); a bound that is None or exactly 0 becomes the image's own
    percentile -/+ eps.  mask: the picture is 1 where it is not > 0."""
    import torch

    H, W = int(value.shape[0]), int(value.shape[1])
    auto = rc.weighted_percentile(value, weight, [50 - percentile / 2, 50 + percentile / 2])
    if isinstance(lo, torch.Tensor):
        bounds = lo
    else:
        bounds = torch.tensor([float(lo or 0.0), float(hi or 0.0)], dtype=torch.float64, device=auto.device)
    item = dict(src=value, op="turbo", channels=1, bounds=bounds, auto_bounds=auto, mask=mask, f32=not u8, u8=u8)
    return rc.vis_images([item], H, W)[0]["u8" if u8 else "f32"]


class _Suite:
    """The item table of one suite: entries are added under their vis key when their source keys are rendered.  The
    table holds every tensor the calls read (sources, uploaded masks, maxima, percentiles) until run() has enqueued the
    last call; all calls go to torch's current stream, whose allocator keeps a freed block from being reused earlier."""

    def __init__(self, rc, rendering, masks, u8, nan_to_num):
        self.rc, self.r, self.u8, self.nan_to_num = rc, rendering, u8, nan_to_num
        self.masks = None if masks is None else rc._dev(masks)
        self.H, self.W = _hw(rendering)
        self.keys, self.items, self.maxima = [], [], {}

    def max_of(self, key):
        """np.max of a rendered image as a device float: one rc_image_max per image."""
        if key not in self.maxima:
            self.maxima[key] = self.rc.image_max(self.r[key])
        return self.maxima[key]

    def add(self, vis_key, src_key, op, divide_by_max_of=None, **kw):
        if src_key not in self.r or (divide_by_max_of is not None and divide_by_max_of not in self.r):
            return
        src = self.r[src_key]
        n_bins = int(src.shape[2]) if op.startswith("binsum") else 0
        channels = src.numel() // (self.H * self.W * max(n_bins, 1))
        if divide_by_max_of is not None:
            kw["divisor"] = self.max_of(divide_by_max_of)
        self.keys.append(vis_key)
        self.items.append(dict(src=src, op=op, channels=channels, n_bins=n_bins, nan_to_num=self.nan_to_num,
                               f32=not self.u8, u8=self.u8, **kw))

    def depth(self, acc, with_gt):
        """depth_mean, depth_median (and, with_gt: the transient suite, depth_gt): bounds from distance_median, each
        picture's own percentiles for a bound of exactly 0; 1 where the mask is not > 0 (engine/trainer.py:1949-1953)."""
        if "distance_median" not in self.r:
            return
        ps = [0.5, 99.5]
        bounds = self.rc.weighted_percentile(self.r["distance_median"], acc, ps)
        for vis_key, src_key in (("depth_mean", "distance_mean"), ("depth_median", "distance_median"), ("depth_gt", "depth_gt")):
            if src_key not in self.r or (src_key == "depth_gt" and not with_gt):
                continue
            auto = bounds if src_key == "distance_median" else self.rc.weighted_percentile(self.r[src_key], acc, ps)
            self.add(vis_key, src_key, "turbo", bounds=bounds, auto_bounds=auto, mask=self.masks)

    def normals(self, acc):
        for key in self.r:
            if key.startswith("normals"):
                self.add(key, key, "matte", divide=2.0, offset=0.5, acc=acc)

    def material(self, acc, divide, irradiance_max_of):
        self.add("color_irradiance_cache", "irradiance_cache", "srgb")
        self.add("material_albedo", "material_albedo", "matte", exponent=1.0 / 2.2, acc=acc)
        for key in _MATERIAL_MATTE:
            self.add(key, key, "matte", acc=acc)
        if "material_rgb" in self.r:
            for vis_key, src_key in _MATERIAL_SRGB:
                self.add(vis_key, src_key, "srgb", divide=divide)
            self.add("material_occ", "occ", "matte")
            self.add("material_indirect_occ", "indirect_occ", "matte")
        self.add("material_lighting_irradiance", "lighting_irradiance", "srgb", divide_by_max_of=irradiance_max_of)

    def run(self):
        out = self.rc.vis_images(self.items, self.H, self.W) if self.items else []
        return {k: o["u8" if self.u8 else "f32"] for k, o in zip(self.keys, out)}


def _acc_for_depth(rendering):
    """acc = where(isnan(distance_mean), 0, acc) (vis.py:429): the weight of the percentiles and the matte of the pictures."""
    import torch

    acc = rendering["acc"].reshape(_hw(rendering))
    if "distance_mean" not in rendering:
        return acc
    return torch.where(torch.isnan(rendering["distance_mean"].reshape(acc.shape)), torch.zeros_like(acc), acc)


def visualize_suite(rendering: Dict[str, object], config, vis_material: bool = False, masks=None, u8: bool = True, rc=None):
    """vis.visualize_suite on the device.  rendering: [H, W, ...] float32 cuda tensors under the reference's key names
    (Model.apply's "render" dict, reshaped to the image, carries the `cache_*` aliases); config: img_scale and var_scale
    are read where present (default 1); masks: [H, W], the depth pictures are 1 where it is not > 0; rc: the RadianceCache
    the calls run on (any handle of the tensors' device).  Returns the reference's vis keys as [H, W, 3] cuda tensors,
    uint8 (save_img_u8's form) with u8, else float32 after the suite's nan_to_num.  Every call is enqueued on torch's
    current stream."""
    if rc is None:
        raise ValueError("visualize_suite needs the RadianceCache it runs on: pass rc=")
    s = _Suite(rc, rendering, masks, u8, nan_to_num=True)
    img_scale, var_scale = float(getattr(config, "img_scale", 1.0)), float(getattr(config, "var_scale", 1.0))
    acc = _acc_for_depth(rendering)
    s.items.append(dict(src=acc, op="matte", channels=1, nan_to_num=True, f32=not u8, u8=u8))
    s.keys.append("acc")
    s.depth(acc, with_gt=False)                    # the reference draws depth_gt in the transient suite only
    s.add("lossmult", "lossmult", "matte")
    s.add("color", "rgb", "srgb")
    s.add("color_var", "rgb_variance", "abs", scale=var_scale / img_scale)
    s.add("color_cache", "cache_rgb", "srgb")
    s.add("color_cache0", "cache_rgb", "srgb", divide_by_max_of="cache_rgb")
    for vis_key, src_key in _SRGB_SCALED + _SRGB + (("cache_irradiance_color", "cache_irradiance_rgb"),
                                                    ("slf_rgb", "cache_incoming_rgb"), ("env_map_rgb", "cache_env_map_rgb")):
        s.add(vis_key, src_key, "srgb")
    s.add("cache_occ", "cache_occ", "matte")
    s.add("cache_indirect_occ", "cache_indirect_occ", "matte")
    s.add("slf_rgb0", "cache_incoming_rgb", "srgb", divide_by_max_of="cache_rgb")
    s.add("env_map_rgb0", "cache_env_map_rgb", "srgb", divide_by_max_of="cache_rgb")
    s.add("slf_depth", "cache_incoming_s_dist", "matte")
    s.add("slf_acc", "cache_incoming_acc", "matte")
    if vis_material:
        s.material(acc, divide=1.0, irradiance_max_of=None)
    s.normals(acc)
    return s.run()


def visualize_transient_suite(rendering: Dict[str, object], config, vis_material: bool = False, masks=None, u8: bool = True,
                              rc=None):
    """vis.visualize_transient_suite on the device: as visualize_suite, with "rgb" and "cache_rgb" [H, W, n_bins, 3]
    summed over the bins, the colours divided by config.img_scale or by their own maximum as the reference does, "depth_gt"
    when the rendering holds one, and no closing nan_to_num."""
    if rc is None:
        raise ValueError("visualize_transient_suite needs the RadianceCache it runs on: pass rc=")
    s = _Suite(rc, rendering, masks, u8, nan_to_num=False)
    img_scale, var_scale = float(getattr(config, "img_scale", 1.0)), float(getattr(config, "var_scale", 1.0))
    acc = _acc_for_depth(rendering)
    s.items.append(dict(src=acc, op="matte", channels=1, f32=not u8, u8=u8))
    s.keys.append("acc")
    s.depth(acc, with_gt=True)
    s.add("lossmult", "lossmult", "matte")
    s.add("vignette", "vignette", "matte", divide_by_max_of="vignette")
    s.add("color", "rgb", "binsum_clip_srgb", divide=img_scale)
    s.add("color_cache", "cache_rgb", "binsum_srgb")
    s.add("color_cache0", "cache_rgb", "binsum_clip_srgb", divide=img_scale)
    for vis_key, src_key in _SRGB_SCALED:
        s.add(vis_key, src_key, "srgb", divide=img_scale)
    for vis_key, src_key in _SRGB:
        s.add(vis_key, src_key, "srgb")
    s.add("cache_occ", "cache_occ", "matte")
    s.add("cache_indirect_occ", "cache_indirect_occ", "matte")
    s.add("cache_irradiance_color", "cache_irradiance_rgb", "srgb", divide_by_max_of="cache_irradiance_rgb")
    s.add("cache_light_radiance_color", "cache_light_radiance_rgb", "matte", divide_by_max_of="cache_light_radiance_rgb")
    s.add("cache_n_dot_l_color", "cache_n_dot_l_rgb", "srgb", divide_by_max_of="cache_n_dot_l_rgb")
    if vis_material:
        s.material(acc, divide=img_scale, irradiance_max_of="cache_irradiance_rgb")
        s.add("direct_rgb_no_integration", "direct_rgb_viz", "srgb", divide_by_max_of="direct_rgb_viz")
    s.normals(acc)
    return s.run()


def save_suite(vis: Dict[str, object], directory: str, index: int):
    """Writes every uint8 entry of a suite as <directory>/<key>/<index:04d>.png, as the reference's trainer lays them out:
    ONE copy of the stacked pictures to the host, then PIL.  Returns the paths by key."""
    import torch

    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("save_suite writes PNGs with PIL (the pillow package), which is not installed") from e
    keys = [k for k, v in vis.items() if v.dtype == torch.uint8]
    if len(keys) != len(vis):
        raise ValueError("save_suite takes the uint8 pictures of a suite made with u8=True")
    if not keys:
        return {}
    host = torch.stack([vis[k] for k in keys]).cpu().numpy()
    paths = {}
    for k, img in zip(keys, host):
        os.makedirs(os.path.join(directory, k), exist_ok=True)
        paths[k] = os.path.join(directory, k, f"{int(index):04d}.png")
        Image.fromarray(img).save(paths[k], "PNG")
    return paths
