"""Relighting the material stage under an HDR environment image.

The reference hands `dataset.env_map`, its sampling tables and `albedo_ratio` to `model.apply` at render time
(internal/train_utils.py:3796-3812): the image replaces the EnvMap MLP (internal/models.py:382-393) and, under
`Config.compute_relight_metrics`, `EnvironmentSampler` replaces both importance-sampler sets (internal/material.py:658,
1228-1247).  Here an `EnvImage` owns the device copies and binds them to a handle; `relight` renders under it.

    env = EnvImage(model.rc, hdr, scale=2.5)           # upload, tables on the device, bind
    out = relight(model, rays, key, env, mode="env")   # == model.apply(None, key, rays, passes=(..., "material"), env_map=env)

Orientation: the tables' `dirs` use world z as their polar axis (internal/datasets.py:2134-2142), the lookup world -y
(render_utils.py:1558-1564).  The reference's sampler and lookup disagree about where a texel is; the image is read only
through the lookup and `dirs` is taken as data.  Not reconciled here.

Reading `.hdr` / `.exr` files is dataset IO and not part of this module: `EnvImage` takes an array.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Tuple

import numpy as np

from . import prng

SAMPLES_TO_TAKE = 256      # EnvironmentSampler.samples_to_take (render_utils.py:195)


def expected_T(n: int, k: int) -> int:
    """Picks one leg of `n` shading points with `k` samples each draws (render_utils.py:208-213)."""
    return SAMPLES_TO_TAKE if (n * k) % SAMPLES_TO_TAKE == 0 else n * k


def leg_counts(cfg) -> Tuple[int, int]:
    """(Ks, Kd): the specular and the diffuse leg's samples per shading point."""
    K = int(cfg.num_secondary_samples)
    return int(round(K * (1.0 - cfg.diffuse_sample_fraction))), int(round(K * cfg.diffuse_sample_fraction))


def check_picks(n: int, cfg, picks_spec, picks_diff):
    """The refusals of rc_relight_args in RC_RELIGHT_ENV, raised before the call with the expected T in the message."""
    Ks, Kd = leg_counts(cfg)
    for name, picks, k in (("picks_spec", picks_spec, Ks), ("picks_diff", picks_diff, Kd)):
        if picks is None:
            raise ValueError(f"mode 'env' needs {name}")
        got = int(np.prod(np.shape(picks)))
        if got != expected_T(n, k):
            raise ValueError(f"{name}: {n} rays x {k} samples draw T = {expected_T(n, k)} picks, got {got}")


class EnvImage:
    """An environment image on the device with its sampling tables, bound to one handle.

    rgb [H, W, 3] is uploaded and multiplied by `scale` (the reference's loader: hdr * 2.5); pmf, pdf and dirs are built by
    rc_env_tables and everything is bound with rc_set_env_image, which copies: this object only keeps its tensors to be
    able to bind again after another image was bound to the same handle."""

    def __init__(self, rc, rgb, scale: float = 1.0, tables=None):
        import torch

        self.rc = rc
        raw = rc._dev(rgb)
        if raw.dim() != 3 or raw.shape[2] != 3:
            raise ValueError("rgb must be [H, W, 3]")
        self.height, self.width = int(raw.shape[0]), int(raw.shape[1])
        self.rgb = raw * torch.tensor(float(scale), dtype=torch.float32, device=raw.device)
        if tables is None:
            tables = rc.env_tables(raw, scale)
        self.pmf, self.pdf, self.dirs = (rc._dev(t) for t in tables)
        self.bind()

    @classmethod
    def from_arrays(cls, rc, env_map, env_map_w, env_map_h, env_map_pmf, env_map_pdf, env_map_dirs):
        """The reference's dataset attributes: env_map [1, H W, L, 3], env_map_pmf / _pdf [1, H W, L], env_map_dirs
        [1, H W, L, 3] with L = 1 illumination (a different L is refused)."""
        H, W = int(env_map_h), int(env_map_w)
        for nm, a, last in (("env_map", env_map, 3), ("env_map_pmf", env_map_pmf, 1), ("env_map_pdf", env_map_pdf, 1),
                            ("env_map_dirs", env_map_dirs, 3)):
            if a is None:
                raise ValueError(f"{nm} is required with env_map")
            if int(np.prod(np.shape(a))) != H * W * last:
                raise NotImplementedError(f"{nm}: expected {H * W * last} values (single illumination, L = 1), got "
                                          f"{int(np.prod(np.shape(a)))}")
        flat = lambda a, last: rc._dev(a).reshape((H * W, last) if last > 1 else (H * W,))
        return cls(rc, rc._dev(env_map).reshape(H, W, 3), 1.0,
                   tables=(flat(env_map_pmf, 1), flat(env_map_pdf, 1), flat(env_map_dirs, 3)))

    def bind(self):
        self.rc.set_env_image(self.rgb, self.pmf, self.pdf, self.dirs)
        self.rc._env_bound = self

    def _ensure_bound(self):
        if getattr(self.rc, "_env_bound", None) is not self:
            self.bind()

    def unbind(self):
        if getattr(self.rc, "_env_bound", None) is self:
            self.rc.set_env_image(None)
            self.rc._env_bound = None

    def lookup(self, dirs):
        """get_environment_color of directions [..., 3] -> [n, 3] (rc_env_lookup)."""
        self._ensure_bound()
        return self.rc.env_lookup(dirs)

    def picks(self, key, T: int):
        """jax.random.categorical(key, safe_log(pmf), axis=-2, shape=(1, T, 1)) as int32 [T] (rc_env_pick)."""
        self._ensure_bound()
        return self.rc.env_pick(key, T)


def as_env_image(rc, env_map, render_kwargs: Dict[str, Any]) -> EnvImage:
    """`env_map=` of Model.apply: an EnvImage, or the reference's arrays with env_map_w / _h / _pmf / _pdf / _dirs."""
    if isinstance(env_map, EnvImage):
        if env_map.rc is not rc:
            raise ValueError("the EnvImage belongs to another handle")
        return env_map
    need = ("env_map_w", "env_map_h", "env_map_pmf", "env_map_pdf", "env_map_dirs")
    missing = [k for k in need if render_kwargs.get(k) is None]
    if missing:
        raise ValueError(f"env_map given as an array needs {', '.join(missing)}")
    return EnvImage.from_arrays(rc, env_map, *(render_kwargs[k] for k in need))


def relight_inputs(env: EnvImage, rng, n: int, cfg, mode: str):
    """(randoms dict, picks_spec, picks_diff) of one relit forward.  rng: a uint32[2] key (the tensors and, in mode
    "env", the categorical keys are derived at the reference's split sites: prng.material_pass_randoms /
    prng.relight_pass_randoms) or the dict of explicit tensors, which in mode "env" holds the picks themselves
    ("picks_spec", "picks_diff") or their keys ("picks_key_spec", "picks_key_diff")."""
    if mode not in ("env", "brdf"):
        raise ValueError(f"unknown relight mode {mode!r}")
    if prng.is_key(rng):
        rng = (prng.relight_pass_randoms if mode == "env" else prng.material_pass_randoms)(rng, n, cfg)
    if not isinstance(rng, dict):
        raise ValueError("relighting needs a uint32[2] key or the dict of explicit random tensors")
    if mode == "brdf":
        if "vmf_noise" not in rng:
            rng = dict(rng, vmf_noise=prng.light_vmf_noise((n, 1, cfg.num_vmf, 3))[:, 0])
        return rng, None, None
    Ks, Kd = leg_counts(cfg)
    picks = []
    for leg, k in (("spec", Ks), ("diff", Kd)):
        p = rng.get("picks_" + leg)
        if p is None:
            if rng.get("picks_key_" + leg) is None:
                raise ValueError(f"mode 'env' needs picks_{leg} or picks_key_{leg}")
            p = env.picks(rng["picks_key_" + leg], expected_T(n, k))
        picks.append(p)
    check_picks(n, cfg, *picks)
    return rng, picks[0], picks[1]


def relight(model, rays, rng, env: EnvImage, mode: str = "env", albedo_ratio=None):
    """The material stage of `model` on `rays` under `env`: what Model.apply(passes=(..., "material"), env_map=env,
    albedo_ratio=...) returns, with the sampler mode chosen here instead of by config.compute_relight_metrics."""
    return model._apply_material(None, rng, rays, env=env, mode=mode, albedo_ratio=albedo_ratio)
