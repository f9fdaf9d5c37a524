"""The probe of a surface point on the device: the `vis_secondary` block of the reference's evaluation
loop (engine/trainer.py:1287, :1905-2052).

    default_pixel, panorama_size    the selected pixel and the panorama's size          engine/trainer.py:752-758
    mark_pixel                      the red square on the ground-truth picture          engine/trainer.py:1358
    probe_view                      the few rows of a rendered view the probe reads
    light_lobes                     the light sampler's 128 lobes at the selected pixels
    surface_probe                   _visualize_secondary_rays + _visualize_vmf          engine/trainer.py:848-1069
    save_probe                      the PNG files of one probe

The incoming-light panorama is what the cache believes arrives at the hit point of a pixel: a latitude-longitude
panorama of secondary rays (rc_probe_rays) rendered with passes ("cache", "is_secondary") and drawn by the visualisation
suite.  The vMF panorama (rc_vmf_panorama) is what the light sampler's mixture of the same pixel believes about the same
light.  The view stays in HBM: the hit point never reaches the host.

Not built: the "light" and "surface_light_field_vis" passes inside the secondary render (for secondary rays "light" only
adds the per-ray vmf_* keys, which render_vmf does not read from the secondary rendering), and the time-resolved cache,
whose model refuses secondary rays.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import prng, rc_ext, vis
from .camera import Camera, cast_ray_batch
from .rays import Rays

NORMAL_OFFSET = 4e-1            # engine/trainer.py:871
_TRANSIENT_REFUSAL = ("the time-resolved cache renders primary rays without resampling "
                      "(TransientNeRFModel.resample_render = False)")


def default_pixel(height: int, width: int, vis_decimate: int = 1) -> Tuple[int, int]:
    """(select_x, select_y) of a [height, width] view (engine/trainer.py:752-754; np.round: half to even)."""
    d = int(vis_decimate)
    return int(np.round(width * 0.3)) // d, int(np.round(height * 0.6)) // d


def panorama_size(height: int, width: int) -> Tuple[int, int]:
    """(light_H, light_W) of the panoramas of a [height, width] view (engine/trainer.py:757-758)."""
    return min(256, int(height)), min(512, int(width) * 2)


def mark_pixel(img, x: int, y: int):
    """The red 10 x 10 square img[y - 5: y + 5, x - 5: x + 5] = (1, 0, 0) of engine/trainer.py:1358, written into an
    [H, W, 3] cuda tensor (float, or uint8 with 255 for 1) with the reference's slice arithmetic (a pixel nearer than 5
    to the top or left edge gives a negative start, which Python counts from the far edge).  Returns img."""
    import torch

    red = torch.tensor([255, 0, 0] if img.dtype == torch.uint8 else [1.0, 0.0, 0.0], dtype=img.dtype, device=img.device)
    img[y - 5: y + 5, x - 5: x + 5, :] = red
    return img


def _pixel_pairs(pixels) -> np.ndarray:
    """[P, 2] int64 (x, y) pairs of one pair or a sequence of pairs."""
    p = np.asarray(pixels, dtype=np.int64)
    p = p.reshape(1, 2) if p.ndim == 1 else p
    if p.ndim != 2 or p.shape[1] != 2 or not 1 <= p.shape[0] <= rc_ext.RC_PROBE_MAX:
        raise ValueError(f"pixels: 1 to {rc_ext.RC_PROBE_MAX} (x, y) pairs, not an array of shape {p.shape}")
    return p


def probe_view(model, camera: Camera, rendering: Dict[str, object], pixels) -> Dict[str, object]:
    """The `view` of rc.probe_rays for pixels [(x, y), ...] of a view rendered from `camera`: rows 0 .. P - 1 are the
    selected pixels and row P is pixel (0, 0), whose lights, imageplane, look and up every probe ray takes
    (_update_secondary_rays, engine/trainer.py:944-1012).  Only these P + 1 primary rays are cast again (rc.cast_rays);
    distance_median and normals_to_use are gathered from the device-resident `rendering` ([H, W, ...] cuda tensors, what
    render_camera(..., to_host=False) returns).  Nothing is synchronised and nothing goes to the host."""
    import torch

    p = _pixel_pairs(pixels)
    dm, nrm = rendering["distance_median"], rendering["normals_to_use"]
    H, W = int(dm.shape[0]), int(dm.shape[1])
    if np.any(p[:, 0] < 0) or np.any(p[:, 0] >= W) or np.any(p[:, 1] < 0) or np.any(p[:, 1] >= H):
        raise ValueError(f"pixels {p.tolist()} outside the {H} x {W} view")
    xs = np.concatenate([p[:, 0], [0]]).astype(np.int32)
    ys = np.concatenate([p[:, 1], [0]]).astype(np.int32)
    rays = cast_ray_batch(model.rc, camera, xs, ys)
    rows = torch.from_numpy(p[:, 1] * W + p[:, 0]).to(dm.device)
    P = p.shape[0]
    return {"origins": rays.origins[:P], "directions": rays.directions[:P],
            "distance_median": dm.reshape(H * W)[rows], "normals": nrm.reshape(H * W, 3)[rows],
            "lights": rays.lights[P:], "imageplane": rays.imageplane[P:], "look": rays.look[P:], "up": rays.up[P:],
            "viewdirs": rays.viewdirs[:P], "near": rays.near[:P], "far": rays.far[:P]}


def light_lobes(model, rays_P, rng=None):
    """The light sampler's lobes at the shading points of P primary rays -> (means [P, V, 3] (unit), kappas [P, V], logits
    [P, V], normals [P, 3]) as cuda tensors, read from the workspace rows "l_vmf", "l_vmf_logit" and "m_nrm" that one
    material forward leaves on the handle.  rays_P: a Rays or a dict of hot fields; rng: as Model.apply's material pass
    (None: PRNGKey(0); the lobes depend on it only through the cache pass's sample jitter).  Raises ValueError on a handle
    without a light sampler (cache-only weights)."""
    rc = model.rc
    if model.config.transient is not None:
        raise NotImplementedError(_TRANSIENT_REFUSAL)
    try:
        model.apply(None, prng.PRNGKey(0) if rng is None else rng, rays_P, passes=("cache", "light", "material"))
    except rc_ext.RcError as e:
        if e.code == rc_ext.RC_ERR_MISSING_WEIGHT:
            raise ValueError("light_lobes: the handle has no light sampler (cache-only weights)") from e
        raise
    fields = rays_P.hot_fields() if isinstance(rays_P, Rays) else rays_P
    P, V = int(np.prod(np.shape(fields["near"]))), int(model.config.num_vmf)
    vmf = rc.workspace_tensor("l_vmf", P * V * 5).reshape(P, V, 5)
    logits = rc.workspace_tensor("l_vmf_logit", P * V).reshape(P, V)
    normals = rc.workspace_tensor("m_nrm", P * 3).reshape(P, 3)
    return vmf[..., 0:3].contiguous(), vmf[..., 3].contiguous(), logits, normals


def _primary_rays(view, P: int) -> Dict[str, object]:
    """The hot fields of the P selected primary rays of a probe_view."""
    return {k: view[k][:P] for k in ("origins", "directions", "viewdirs", "near", "far")} | {"lights": view["lights"][:1].expand(P, 3)}


def surface_probe(model, camera: Camera, rendering: Dict[str, object], pixels=None, rng=None, vmf: bool = True,
                  u8: bool = True, size: Optional[Sequence[int]] = None, flip: bool = False) -> Dict[str, object]:
    """The whole block for pixels [(x, y), ...] (default: default_pixel) of a view of `camera` whose device-resident
    `rendering` holds "distance_median" and "normals_to_use" ([H, W, ...] cuda tensors):

      "pixels"         [P, 2] the (x, y) pairs (numpy)
      "positions"      [P, 3] the hit points the panoramas are cast from
      "secondary"      the rendering of the P [Hl, Wl] panoramas, passes ("cache", "is_secondary"), in chunks of
                       config.render_chunk_size rounded to whole panorama rows: {key: [P, Hl, Wl, ...]}
      "secondary_vis"  a list of P dicts: vis.visualize_suite of each panorama ([Hl, Wl, 3]; uint8 with u8)
      "vmf"            [P, Hl, Wl, 3] the light sampler's mixture over the panorama (uint8 with u8, else float32 sRGB);
                       only with vmf, which needs a light sampler (ValueError on cache-only weights)

    size: (Hl, Wl), default panorama_size of the view; near / far of the secondary rays are config.secondary_near /
    secondary_far; rng: a key (None: PRNGKey(0)) for the material forward behind the lobes and, split per chunk as
    render_image does, for the secondary render, whose resampling always draws.  A time-resolved model raises
    NotImplementedError."""
    cfg = model.config
    if cfg.transient is not None:
        raise NotImplementedError(_TRANSIENT_REFUSAL)
    dm = rendering["distance_median"]
    H, W = int(dm.shape[0]), int(dm.shape[1])
    p = _pixel_pairs(default_pixel(H, W) if pixels is None else pixels)
    P = p.shape[0]
    Hl, Wl = panorama_size(H, W) if size is None else (int(size[0]), int(size[1]))
    view = probe_view(model, camera, rendering, p)
    result = {"pixels": p}
    if vmf:                                   # first: a handle without a light sampler is refused before anything is rendered
        means, kappas, logits, _ = light_lobes(model, _primary_rays(view, P), rng)
        pano = model.rc.vmf_panorama(means, kappas, logits, Hl, Wl, flip=flip, srgb=not u8, u8=u8)
        result["vmf"] = pano["u8" if u8 else "srgb"]
    rays, positions = model.rc.probe_rays(view, np.arange(P), Hl, Wl, cfg.secondary_near, cfg.secondary_far,
                                          NORMAL_OFFSET, flip)
    result["positions"] = positions
    result["secondary"] = render_probe_rays(model, rays, rng)
    result["secondary_vis"] = [vis.visualize_suite({k: v[i] for k, v in result["secondary"].items()}, cfg, u8=u8, rc=model.rc)
                               for i in range(P)]
    return result


def secondary_randoms(model, apply_key, n: int) -> Dict[str, object]:
    """The random tensors of one secondary cache pass on n rays, drawn in HBM (rc_prng_fill) from the keys the reference
    derives from model.apply's rng: per level the sampler's jitter (sampling.py:341 / :408, as render_camera draws it) and
    the Gumbel noise of the resampling draw (models.py:240-247); prng.cache_pass_randoms is the host twin."""
    ck = prng.cache_keys(prng.model_cache_rng(apply_key))
    levels = [lvl[2] for lvl in model.config.sampling_strategy]
    s_key, jit = ck["sampler"], []
    for _ in levels:
        k, s_key = prng.random_split(s_key)
        jit.append(model.rc.prng_fill(k, (n,), "uniform"))
        _, s_key = prng.random_split(s_key)
    g_key, _ = prng.random_split(ck["resample"])
    return {"jitter": jit, "gumbel": model.rc.prng_fill(g_key, (n, levels[-1]), "gumbel")}


def probe_chunk(model, width: int) -> int:
    """Rays per chunk of the secondary render: config.render_chunk_size rounded down to whole panorama rows, at least one."""
    return max(1, int(model.config.render_chunk_size) // int(width)) * int(width)


def render_probe_rays(model, rays: Rays, rng=None) -> Dict[str, object]:
    """model.apply(None, randoms, rays, passes=("cache", "is_secondary")) on the [P, Hl, Wl] rays of rc.probe_rays, in chunks
    of probe_chunk rays -> {key: [P, Hl, Wl, ...]} cuda tensors of every key of the render.  Secondary rays are always
    resampled, which takes random numbers: rng is a key (None: PRNGKey(0)), split per chunk as render_image does
    (prng.chunk_keys); each chunk's tensors are secondary_randoms of its key."""
    import torch

    if model.config.transient is not None:
        raise NotImplementedError(_TRANSIENT_REFUSAL)
    P, Hl, Wl = (int(s) for s in rays.near.shape[:3])
    n = P * Hl * Wl
    flat = {k: v.reshape((n,) + tuple(v.shape[3:])) for k, v in rays.hot_fields().items()}
    chunk = probe_chunk(model, Wl)
    key = prng.PRNGKey(0) if rng is None else prng.as_key(rng)
    dev = flat["near"].device
    images, names = {}, {}               # one image per distinct output of the render; the aliases share it
    for i0 in range(0, n, chunk):
        m = min(chunk, n - i0)
        apply_key, key = prng.chunk_keys(key)
        r = model.apply(None, secondary_randoms(model, apply_key, m), {k: v[i0: i0 + m] for k, v in flat.items()},
                        passes=("cache", "is_secondary"))["render"]
        first = {}                         # region of this chunk's plan -> the first key that names it
        for k in r:
            kind, at, shape = r.layout[k]
            region = (kind, at, tuple(shape[1:]))
            if region in first:
                names[k] = first[region]
                continue
            first[region] = names[k] = k
            if kind == "const":
                if k not in images:
                    images[k] = torch.full((n,) + region[2], at, dtype=torch.float32, device=dev)
                continue
            if k not in images:
                images[k] = torch.empty((n,) + region[2], dtype=torch.float32, device=dev)
            images[k][i0: i0 + m] = r[k]
    return {k: images[c].reshape((P, Hl, Wl) + tuple(images[c].shape[1:])) for k, c in names.items()}


def save_probe(result: Dict[str, object], directory: str, index: int, probe: int = 0) -> Dict[str, str]:
    """Writes probe `probe` of a surface_probe result (made with u8=True) as the reference's trainer lays the files out:
    <directory>/<key>/secondary/<index:04d>.png for every picture of "secondary_vis" and <directory>/vmfs/<index:04d>.png,
    through vis.save_suite's PNG writer.  Returns the paths ("vmfs" and the suite's keys)."""
    suite = {os.path.join(k, "secondary"): v for k, v in result["secondary_vis"][probe].items()}
    if "vmf" in result:
        suite["vmfs"] = result["vmf"][probe]
    paths = vis.save_suite(suite, directory, index)
    return {(k if k == "vmfs" else os.path.dirname(k)): v for k, v in paths.items()}
