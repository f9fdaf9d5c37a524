"""The training loop's feeder on the device: cameras and images uploaded once, one launch per batch.

    DeviceDataset.next_train(key)          Dataset._next_train + _make_ray_batch   internal/datasets.py:948-993, 850-946
    DeviceDataset.generate_ray_batch(i)    Dataset.generate_ray_batch              internal/datasets.py:1009-1022
    patch_indices(key, ...)                the picks of next_train, in numpy

The reference draws cameras and pixels with `np.random.randint` on numpy's GLOBAL Mersenne Twister (datasets.py:954-981):
which batch a step sees depends on everything else in the process that touched that generator, and no caller can
reproduce it across processes.  The index rule here is therefore this package's own, keyed like every other random input
of the package (prng.py): the picks are a pure function of a uint32[2] key.

    w = prng.random_bits(key, (P, 3))                     three words per patch: camera, column, row
    idx = lo + ((uint64) w * range) >> 32                 multiply-shift: exact integers, no rejection loop, every index's
                                                          probability within range / 2^32 of uniform
    camera in [0, C)   ("single_image": the camera of w[0, 0] for every patch, datasets.py:981)
    x0 in [border, W - border - p + 1),  y0 in [border, H - border - p + 1)          (datasets.py:965-971)
    pixel j of a patch: (x0 + j % p, y0 + j // p)         camera_utils.pixel_coordinates(p, p), row-major

Out of scope: per-pixel light_idx images, masks, alphas, normals, disparity, the Bayer mask, flattened data sets and the
loaders themselves.
"""
from __future__ import annotations

import dataclasses
from typing import Any

import numpy as np

from . import prng
from .rays import Rays

BATCHING = ("all_images", "single_image")


@dataclasses.dataclass
class Batch:
    """utils.Batch (internal/utils.py) as far as the cache stage reads it."""
    rays: Rays
    rgb: Any


def pick(words, lo: int, rng: int) -> np.ndarray:
    """lo + floor(w * rng / 2^32) for uint32 words, in 64-bit integers."""
    return (int(lo) + ((np.asarray(words, np.uint32).astype(np.uint64) * np.uint64(rng)) >> np.uint64(32))).astype(np.int32)


def patch_indices(key, num_patches: int, patch_size: int, border: int, height: int, width: int, num_cameras: int,
                  batching: str = "all_images"):
    """(cam_idx, pix_x, pix_y), int32 [num_patches * patch_size^2]: the index rule of the module docstring."""
    if batching not in BATCHING:
        raise ValueError(f"unknown batching {batching!r}")
    P, p = int(num_patches), int(patch_size)
    xr, yr = width - 2 * border - p + 1, height - 2 * border - p + 1
    if P < 0 or p < 1 or border < 0 or num_cameras < 1 or xr < 1 or yr < 1:
        raise ValueError("no admissible patch position")
    w = prng.random_bits(key, (P, 3))
    cam = pick(w[:, 0] if batching == "all_images" else np.broadcast_to(w[:1, 0], (P,)), 0, num_cameras)
    x0, y0 = pick(w[:, 1], border, xr), pick(w[:, 2], border, yr)
    j = np.arange(p * p, dtype=np.int32)
    px = (x0[:, None] + j[None, :] % p).reshape(-1)
    py = (y0[:, None] + j[None, :] // p).reshape(-1)
    return np.repeat(cam, p * p).astype(np.int32), px.astype(np.int32), py.astype(np.int32)


class DeviceDataset:
    """Cameras and images of an image-shaped data set in HBM.  images: [C, H, W, 3] float32 or uint8 (numpy or torch;
    uint8 is read as u / 255 in float32); cam_lossmult: [C] or None (Dataset.lossmult, datasets.py:989-990); the camera
    arguments as in RadianceCache.camera_set.  batch_size rays per batch = batch_size // patch_size^2 patches."""

    def __init__(self, rc, pixtocams, camtoworlds, images, lights=None, near: float = 2.0, far: float = 6.0,
                 camtype="perspective", distortion_params=None, pixtocam_ndc=None, z_range=None, cam_lossmult=None,
                 patch_size: int = 1, border: int = 0, batching: str = "all_images", batch_size: int = 1024):
        import torch

        if batching not in BATCHING:
            raise ValueError(f"unknown batching {batching!r}")
        self.rc = rc
        self.cameras = rc.camera_set(pixtocams, camtoworlds, lights, near, far, camtype, distortion_params, pixtocam_ndc,
                                     z_range)
        img = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images))
        if img.dim() != 4 or img.shape[-1] != 3 or img.shape[0] != self.cameras.count:
            raise ValueError("images must be [C, H, W, 3] with one image per camera")
        if img.dtype != torch.uint8:
            img = img.to(torch.float32)
        self.images = img.to(f"cuda:{rc.device}").contiguous()
        self.height, self.width = int(img.shape[1]), int(img.shape[2])
        self.cam_lossmult = None if cam_lossmult is None else rc._dev(np.asarray(cam_lossmult, np.float32).reshape(-1))
        self.patch_size, self.border, self.batching = int(patch_size), int(border), batching
        self.num_patches = int(batch_size) // self.patch_size ** 2                 # datasets.py:965
        self.batch_size = self.num_patches * self.patch_size ** 2

    def host_indices(self, key):
        """(cam_idx, pix_x, pix_y) of next_train(key), int32 numpy [batch_size]."""
        return patch_indices(key, self.num_patches, self.patch_size, self.border, self.height, self.width,
                             self.cameras.count, self.batching)

    def next_train(self, key, pix_jitter=None) -> Batch:
        """The batch of key `key`: rays [batch_size, .] (lossmult, near, far, cam_idx, pix_x_int, pix_y_int filled in)
        and rgb [batch_size, 3], cuda tensors from one launch; nothing is read back."""
        rays, rgb = self.rc.train_batch(self.cameras, self.images, key, self.batch_size, self.patch_size, self.border,
                                        self.batching, self.cam_lossmult, pix_jitter)
        return Batch(rays=rays, rgb=rgb)

    def generate_ray_batch(self, cam_idx: int) -> Batch:
        """Every pixel of camera cam_idx, rays [H, W, .] (lossmult 1) and rgb [H, W, 3] (datasets.py:1009-1022)."""
        import torch

        c = int(cam_idx)
        if not 0 <= c < self.cameras.count:
            raise IndexError(f"camera {c} of {self.cameras.count}")
        dev = self.images.device
        ys, xs = torch.meshgrid(torch.arange(self.height, dtype=torch.int32, device=dev),
                                torch.arange(self.width, dtype=torch.int32, device=dev), indexing="ij")
        rays = self.rc.cast_rays_multi(self.cameras, torch.full_like(xs, c), xs.contiguous(), ys.contiguous())
        rgb = self.images[c]
        return Batch(rays=rays, rgb=rgb if rgb.dtype == torch.float32 else rgb.to(torch.float32) / 255.0)
