"""Light-in-flight frames of the time-resolved cache: a camera view at one instant of the time axis, without the histograms.

The reference's trainer makes them under `eval_path` (engine/trainer.py:1693-1726, _save_path_evaluation):

    t = transient_start_idx + frac * (transient_end_idx - transient_start_idx)
    cache_time_slice = w * cache_rgb[..., ceil t, :] + (1 - w) * cache_rgb[..., floor t, :],   w = t - floor t

from the whole [H, W, n_bins, 3] rendering.  Here a frame comes from rc_render_transient_slices, which
evaluates the bins that reach floor t and ceil t only: 12 bytes per ray and time instead of 8.4 KB.

    slice_weights(t)                      -> (floor, ceil, w)
    path_times(num_frames, start, end)    -> the t of every frame of a path
    render_time_slices(model, camera, ..) -> {"rgb": [H, W, T, 3], ...} of one camera at T times
    render_time_slice_path(model, cams, ..) -> one frame per camera, each at its own t
    save_time_slice(frame, directory, i)  -> cache_time_slice/NNNN.npy and .png
"""
from __future__ import annotations

import math
import os
from typing import Dict, Optional, Sequence

import numpy as np

from . import camera as camera_lib
from . import vis


def slice_weights(t: float):
    """(floor t, ceil t, w = t - floor t) of a fractional bin index: the frame is w * v[ceil] + (1 - w) * v[floor].  An
    integral t gives floor == ceil and w == 0."""
    t = float(t)
    if not math.isfinite(t):
        raise ValueError(f"slice_weights: t must be finite, got {t}")
    lo, hi = int(math.floor(t)), int(math.ceil(t))
    return lo, hi, t - lo


def path_times(num_frames: int, start_idx: float, end_idx: float) -> np.ndarray:
    """The t of the frames of a path as the trainer sets them: frame k of num_frames gets frac = k / num_frames and
    t = start_idx + frac * (end_idx - start_idx), so the last frame stops one step short of end_idx."""
    if num_frames < 1:
        raise ValueError("path_times: num_frames must be positive")
    frac = np.arange(num_frames, dtype=np.float64) / float(num_frames)
    return float(start_idx) + frac * (float(end_idx) - float(start_idx))


def render_time_slices(model, camera, height: int, width: int, times, rows_per_chunk: Optional[int] = None,
                       outputs: Sequence[str] = ("rgb",), rng=None, to_host: bool = True) -> Dict[str, object]:
    """Time slices of one camera: {output: [height, width, len(times), 3]} (numpy, or cuda tensors with to_host=False),
    outputs of rc_ext.TRANSIENT_SLICE_OUTPUTS.  The chunk loop and the key derivation are camera.render_camera's: rows of
    pixels are cast on the device and rendered chunk by chunk, and with a key `rng` every chunk draws the jitter
    render_camera would draw for it.  A chunk is a batch: the direct light that spills into the next ray of a batch
    (render.py:447-475) follows the chunking exactly as it does for render_camera(keys=("rgb",), ...) with the same
    rows_per_chunk, whose histograms these slices are taken from."""
    import torch

    from . import prng
    if model.config.transient is None:
        raise ValueError("render_time_slices needs a time-resolved model (config.transient)")
    times = [float(t) for t in np.asarray(times, dtype=np.float64).reshape(-1)]
    if rng is not None:
        rng = prng.as_key(rng)
    rows = camera_lib.chunk_rows(model, width, rows_per_chunk)
    dev = torch.device(f"cuda:{model.device}")
    model._ensure_variables(None)
    out = {k: torch.empty((height, width, len(times), 3), dtype=torch.float32, device=dev) for k in outputs}
    for y0 in range(0, height, rows):
        hgt = min(rows, height - y0)
        rays = camera_lib.cast_ray_batch(model.rc, camera, rect=(0, y0, width, hgt))
        randoms, rng = camera_lib.chunk_randoms(model, rng, hgt * width)
        r = model.rc.render_transient_slices(rays.hot_fields(), randoms, times, outputs=outputs)
        for k in outputs:
            out[k][y0:y0 + hgt] = r[k].reshape(hgt, width, len(times), 3)
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in out.items()} if to_host else out


def render_time_slice_path(model, cameras, height: int, width: int, start_idx: float = 0.0, end_idx: Optional[float] = None,
                           rows_per_chunk: Optional[int] = None, output: str = "rgb", rng=None, to_host: bool = True):
    """The light-in-flight frames of a camera path: frame k is camera k at path_times(len(cameras), start_idx, end_idx)[k]
    (end_idx: n_bins - 1 by default, the last bin).  Returns (frames [len(cameras), height, width, 3], times).  With a key
    `rng` every frame is rendered from that key, as the trainer renders every path frame from the same key."""
    import torch

    cameras = list(cameras)
    end = float(model.config.transient.n_bins - 1) if end_idx is None else float(end_idx)
    times = path_times(len(cameras), start_idx, end)
    frames = [render_time_slices(model, cam, height, width, [t], rows_per_chunk, (output,), rng, to_host=False)[output][:, :, 0]
              for cam, t in zip(cameras, times)]
    frames = torch.stack(frames)
    return (frames.cpu().numpy() if to_host else frames), times


def save_time_slice(frame, directory: str, index: int) -> Dict[str, str]:
    """Writes one [H, W, 3] frame as the trainer does: <directory>/cache_time_slice/<index:04d>.npy (the float32 values)
    and .png (clipped to [0, 1], 8 bits, through vis.save_suite's PNG writer).  Returns the two paths."""
    import torch

    f = frame if isinstance(frame, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frame, dtype=np.float32))
    if f.dim() != 3 or f.shape[-1] != 3:
        raise ValueError(f"save_time_slice: one [H, W, 3] frame, got {tuple(f.shape)}")
    f = f.detach().to(torch.float32)
    u8 = (torch.clamp(torch.nan_to_num(f), 0.0, 1.0) * 255.0).to(torch.uint8)
    paths = {"png": vis.save_suite({"cache_time_slice": u8}, directory, index)["cache_time_slice"]}
    paths["npy"] = os.path.join(directory, "cache_time_slice", f"{int(index):04d}.npy")
    np.save(paths["npy"], f.cpu().numpy())
    return paths
