"""Python host layer: the reference's call signatures on top of the C ABI.

Mirrors, for the radiance-cache hot path only:
  * model.apply(variables, rng, rays, **render_kwargs) -> {"render": {...}, ...}
      BaseMaterialModel.__call__              internal/models.py:1144-1254
  * create_render_fn(model, dataset, mapping_fn) -> render_eval_pfn(variables, rng, train_frac, cameras, lights,
                                                                    rays, passes, resample) -> (renderings, rng)
      train_utils.create_render_fn            internal/train_utils.py:3742-3831
      (called as at engine/trainer.py:822-832; `bind_render_fn` builds the 4-argument closure the Trainer wraps
       around it, engine/trainer.py:821-832)
  * render_image(render_fn, rng, rays, config, passes, ...) -> (rendering, rng)
      models.render_image                     internal/models.py:2361-2525
      (ONE chunk loop, one mean over repeats and one image sink, for a foreign callable -- host slices in, numpy out
       per chunk -- and for this package's own render function, whose chunks and results stay on the device)
  * utils.shard / utils.unshard               internal/utils.py:333-343

One process drives one GPU (torch.distributed rank); `n_local_devices` is therefore 1 and the
leading device axis of the reference's pmap outputs is kept with size 1 so callers that index
`v[0]` keep working.  Ray batches are sharded across ranks at image granularity by
`render_image_distributed`, with one all-gather of the consumed keys per image (RCCL over xGMI
via torch.distributed's "nccl" backend; "gloo" on CPU for the tests).

Randomness: `rng` may be
  * None                         -> the reference's rng=None deterministic branch,
  * a uint32[2] key (prng.PRNGKey)-> the tensors jax.random would draw from that key at the reference's
                                    random_split sites (prng.py; threefry2x32 pinned by published known answers,
                                    the call order restated from the source and not checkable without jax),
  * a numpy Generator / int seed -> per-level ray jitter (and Gumbel noise) drawn here,
  * a dict {"jitter": [...], "gumbel": ..., "resample_inds": ...} of explicit tensors.
"""
from __future__ import annotations

import contextlib
import time
from collections.abc import Mapping
from typing import Any, Dict, Optional, Tuple

import numpy as np

from . import prng, rc_ext
from .config import RenderConfig
from .rays import Pixels, Rays

# keys of _finalize_outputs (internal/models.py:2087-2111) that get a `cache_` alias
_FINAL_INTEGRATOR_KEYS = (
    "rgb", "normals", "normals_pred", "incoming_rgb", "env_map_rgb", "incoming_s_dist", "diffuse_rgb",
    "specular_rgb", "occ", "indirect_occ", "direct_rgb", "indirect_rgb", "ambient_rgb", "irradiance_rgb",
    "light_radiance_rgb", "n_dot_l_rgb", "albedo_rgb", "direct_diffuse_rgb", "direct_specular_rgb",
    "indirect_diffuse_rgb", "indirect_specular_rgb", "ambient_diffuse_rgb", "ambient_specular_rgb",
)
# device outputs the primary cache pass computes
_SECONDARY_DEVICE_KEYS = ("env_map_rgb", "rgb_no_env")
_CACHE_DEVICE_KEYS = ("rgb", "acc", "distance_mean", "distance_percentile_5", "distance_median",
                      "distance_percentile_95", "diffuse_rgb", "specular_rgb", "direct_rgb", "indirect_rgb",
                      "albedo_rgb", "indirect_diffuse_rgb", "indirect_specular_rgb", "indirect_occ", "means",
                      "normals", "normals_pred", "ray_dists", "light_dists")


def flatten_variables(variables: Dict[str, Any], prefix: str = "") -> Dict[str, Any]:
    """Flax variable tree {"params": {"Cache": {...}}} -> {"params/Cache/...": array}."""
    flat = {}
    for k, v in variables.items():
        name = f"{prefix}/{k}" if prefix else k
        if isinstance(v, dict):
            flat.update(flatten_variables(v, name))
        else:
            flat[name] = v
    return flat


def _leaf_refs(variables, out):
    """(container, key, leaf, version) of every leaf: what `Model.apply` re-checks to notice an updated tree."""
    for k, v in variables.items():
        if isinstance(v, dict):
            _leaf_refs(v, out)
        else:
            out.append((variables, k, v, getattr(v, "_version", None)))
    return out


def _draw_randoms(rng, n: int, cfg: RenderConfig, need_gumbel: bool):
    if rng is None:
        return None, None
    if isinstance(rng, dict):
        return rng, None
    if prng.is_key(rng):
        return prng.cache_pass_randoms(rng, n, [lvl[2] for lvl in cfg.sampling_strategy], need_gumbel), None
    if isinstance(rng, (int, np.integer)):
        rng = np.random.Generator(np.random.PCG64(int(rng)))
    out = {"jitter": [rng.uniform(size=(n,)).astype(np.float32) for _ in range(cfg.num_levels)]}
    if need_gumbel:
        out["gumbel"] = rng.gumbel(size=(n, cfg.sampling_strategy[-1][2])).astype(np.float32)
    return out, rng


class RenderDict(Mapping):
    """The `render` dict of one ray batch (keys of _finalize_outputs, internal/models.py:2074-2171) over ONE flat
    device allocation: the kernel writes every output slot into `flat`; a key's tensor ([n, 3], [n, 1] or [n], plus
    `lead` leading axes of size 1) is a view made when the key is read.  Aliases (`cache_<k>`, `ambient_rgb`, ...)
    share a region, exact constants (`occ`, `vignette`, ...) share one cached tensor per batch size.  The chunk loop
    of render_image never touches the views: it keeps `flat` per chunk and unpacks the whole image once."""

    __slots__ = ("flat", "layout", "consts", "extras", "lead", "_views")

    def __init__(self, flat, layout, consts, extras=(), lead=0):
        self.flat, self.layout, self.consts, self.extras, self.lead = flat, layout, consts, extras, lead
        self._views = {}

    def with_lead(self, lead: int) -> "RenderDict":
        return RenderDict(self.flat, self.layout, self.consts, self.extras, lead)

    def __getitem__(self, key):
        v = self._views.get(key)
        if v is None:
            kind, a, shape = self.layout[key]
            if kind == "flat":
                cnt = 1
                for d in shape:
                    cnt *= d
                v = self.flat[a: a + cnt].view(shape)
            elif kind == "const":
                v = self.consts(a, shape)
            else:
                v = self.extras[a]
            for _ in range(self.lead):
                v = v[None]
            self._views[key] = v
        return v

    def __iter__(self):
        return iter(self.layout)

    def __len__(self):
        return len(self.layout)


def _cache_layout(offs, n: int, secondary: bool, lossmult_extra: bool):
    """Key -> ("flat", offset, shape) | ("const", value, shape) | ("extra", index, shape): the integrator keys plus the
    aliases / exact constants of the configured passive shader and of _finalize_outputs (internal/nerf.py:1044-1084,
    internal/models.py:2074-2171)."""
    lay = {}
    for k in _CACHE_DEVICE_KEYS + (("env_map_rgb",) if secondary else ()):
        off, shape = offs[k]
        lay[k] = ("flat", off, (n, 1) if k in ("ray_dists", "light_dists") else shape)
    for k in ("ambient_rgb", "direct_diffuse_rgb", "ambient_diffuse_rgb"):
        lay[k] = lay["direct_rgb"]
    for k in ("occ", "irradiance_rgb", "light_radiance_rgb", "n_dot_l_rgb", "direct_specular_rgb", "ambient_specular_rgb"):
        lay[k] = ("const", 0.0, (n, 3))
    lay["normals_to_use"] = lay["normals_pred"]
    for k in _FINAL_INTEGRATOR_KEYS:
        if k in lay:
            lay["cache_" + k] = lay[k]
    lay["vignette"] = ("const", 1.0, (n, 1))
    lay["lossmult"] = ("extra", 0, (n, 3)) if lossmult_extra else ("const", 1.0, (n, 3))
    if secondary:
        # Model._handle_secondary (internal/models.py:309-460): *_no_stopgrad copies (the env composite runs on the device)
        lay["rgb_no_stopgrad"] = lay["rgb"]
        lay["acc_no_stopgrad"] = lay["acc"]
    return lay


class Model:
    """Cache stage of MaterialModel (use_material=False): `apply` keeps the reference signature."""

    def __init__(self, config: Optional[RenderConfig] = None, device: int = 0):
        self.config = config or RenderConfig()
        self.device = device
        self.rc = rc_ext.RadianceCache(self.config, device)   # raises if librc_hip.so is missing
        self._variables_ref = None
        self._variables_checked = False       # render_image's device loop: the tree was checked for this image already
        self._out_arena = None                # render_image's device loop: (arena [n_chunks, floats], next row)
        self._leaves = []
        self._plans = {}
        self._const_cache = {}

    # -- weights ------------------------------------------------------------------------------------
    def load_variables(self, variables: Dict[str, Any]):
        """Upload a parameter tree (nested Flax tree or the flat {"params/...": array} dict).  A tree replicated for
        pmap (flax.jax_utils.replicate: every leaf with a leading [n_local_devices = 1] axis, engine/trainer.py:647-670)
        is accepted as it is."""
        nested = any(isinstance(v, dict) for v in variables.values())
        flat = flatten_variables(variables) if nested else dict(variables)
        bias = next((v for k, v in flat.items() if k.endswith("/bias")), None)
        if bias is not None and len(np.shape(bias)) == 2:          # replicated: strip the device axis
            flat = {k: v[0] for k, v in flat.items()}
        self.rc.load_weights(flat)
        self._variables_ref = variables
        self._leaves = _leaf_refs(variables, [])                   # holds the leaves: their ids cannot be recycled

    def _ensure_variables(self, variables):
        """Re-upload when `variables` is another tree than the loaded one, when a leaf of the same tree was replaced
        (functional update in place of the container) or when a torch leaf was written in place (its `_version` moved).
        In-place writes into numpy leaves cannot be seen: call load_variables after those."""
        if variables is None:
            return
        if self._variables_checked and variables is self._variables_ref:
            return                                                 # same tree, verified once for the image being rendered
        if variables is self._variables_ref:
            for cont, key, leaf, ver in self._leaves:
                cur = cont.get(key)
                if cur is not leaf or (ver is not None and cur._version != ver):
                    break
            else:
                return
        self.load_variables(variables)

    # -- per-batch-size plans and constants -----------------------------------------------------------
    def _consts(self, value: float, shape):
        import torch
        key = (value, shape)
        t = self._const_cache.get(key)
        if t is None:
            if len(self._const_cache) > 64:
                self._const_cache.clear()
            t = torch.full(shape, value, dtype=torch.float32, device=f"cuda:{self.device}")
            self._const_cache[key] = t
        return t

    def _plan(self, n: int, secondary: bool, lossmult_extra: bool):
        key = (n, secondary, lossmult_extra)
        p = self._plans.get(key)
        if p is None:
            if len(self._plans) > 64:
                self._plans.clear()
            names = _CACHE_DEVICE_KEYS + (_SECONDARY_DEVICE_KEYS if secondary else ())
            rc_plan = self.rc.output_plan(names, n)
            p = (rc_plan, _cache_layout(rc_plan[1], n, secondary, lossmult_extra))
            self._plans[key] = p
        return p

    # -- model.apply --------------------------------------------------------------------------------------
    def apply(self, variables, rng, rays: Rays, *, train_frac: float = 1.0, train: bool = False,
              passes: Tuple[str, ...] = ("cache",), compute_extras: bool = False, is_secondary: bool = False,
              resample: Any = None, sampling_strategy=None, **unused_render_kwargs):
        """model.apply(variables, rng, rays, ...) (internal/models.py:1144-1254).

        `variables` may be None once `load_variables` was called (they live on the device).
        Only the inference branch exists here: train must be False and train_frac 1.0.
        """
        if train or train_frac != 1.0:
            raise NotImplementedError("only the render-time path (train=False, train_frac=1.0) is accelerated")
        if sampling_strategy is not None and tuple(sampling_strategy) != tuple(self.config.sampling_strategy):
            raise NotImplementedError("sampling_strategy is fixed when the handle is created")
        env_map = unused_render_kwargs.get("env_map")
        if "material" in passes:
            if env_map is None:
                return self._apply_material(variables, rng, rays)
            # relighting: dataset.env_map and its tables handed on by render_eval_fn (train_utils.py:3796-3812);
            # EnvironmentSampler in both sampler sets under compute_relight_metrics (material.py:658, 1228-1247)
            from . import relight
            env = relight.as_env_image(self.rc, env_map, unused_render_kwargs)
            mode = "env" if getattr(self.config, "compute_relight_metrics", False) else "brdf"
            return self._apply_material(variables, rng, rays, env=env, mode=mode,
                                        albedo_ratio=unused_render_kwargs.get("albedo_ratio"))
        if self.config.transient is not None:
            return self._apply_transient(variables, rng, rays, is_secondary or "is_secondary" in passes, resample)
        self._ensure_variables(variables)
        fields = rays.hot_fields() if isinstance(rays, Rays) else rays
        near = fields["near"]
        n = near.numel() if hasattr(near, "numel") else int(np.prod(np.shape(near)))
        mask = rc_ext.RC_PASS_CACHE
        if is_secondary or "is_secondary" in passes:
            mask |= rc_ext.RC_PASS_SECONDARY
        if resample:
            mask |= rc_ext.RC_PASS_RESAMPLE
        need_gumbel = bool(mask & (rc_ext.RC_PASS_SECONDARY | rc_ext.RC_PASS_RESAMPLE))
        randoms, _ = _draw_randoms(rng, n, self.config, need_gumbel)
        secondary = bool(mask & rc_ext.RC_PASS_SECONDARY)
        if secondary and unused_render_kwargs.get("use_env_map") is False:
            mask |= rc_ext.RC_PASS_NO_ENVMAP
        if secondary and env_map is not None:
            # Model._handle_env_map with an explicit image (models.py:382-393): the lookup instead of the EnvMap MLP
            from . import relight
            relight.as_env_image(self.rc, env_map, unused_render_kwargs)._ensure_bound()
            mask |= rc_ext.RC_PASS_ENV_IMAGE
        lossmult = fields.get("lossmult")
        rc_plan, layout = self._plan(n, secondary, lossmult is not None)
        out_flat = None
        if self._out_arena is not None:                            # a row of the image's output arena (device loop)
            arena, row = self._out_arena
            if row < arena.shape[0] and arena.shape[1] == rc_plan[0]:
                out_flat = arena[row]
                self._out_arena = (arena, row + 1)
        flat, _ = self.rc.render_chunk(fields, randoms, mask, rc_plan, out_flat)
        extras = ()
        if lossmult is not None:       # models.py:2055-2063: rays.lossmult broadcast over the colour channels
            extras = (self.rc._dev(lossmult).reshape(-1, 1).expand(-1, 3),)
        render = RenderDict(flat, layout, self._consts, extras)
        return {"render": render, "main": {"integrator": render}, "cache_main": {"integrator": render}}

    __call__ = apply

    def _apply_transient(self, variables, rng, rays, is_secondary, resample):
        """TransientNeRFModel (internal/models.py:912-985) as the cache of TransientMaterialModel with
        use_material=False: sampler -> TransientNeRFMLP -> TransientVolumeIntegrator on primary rays.
        `rgb` is the [n, n_bins, 3] transient; models.render_image drops every other `transient*` key except
        the two `*_viz` ones (internal/models.py:2403, 2459-2472)."""
        import torch

        if is_secondary or resample:
            raise NotImplementedError("the time-resolved cache renders primary rays without resampling "
                                      "(TransientNeRFModel.resample_render = False)")
        self._ensure_variables(variables)
        fields = rays.hot_fields() if isinstance(rays, Rays) else dict(rays)
        if fields.get("lights") is None or fields.get("cam_origins") is None:
            raise ValueError("transient rays need `lights` and `cam_origins`")
        n = int(np.prod(np.shape(fields["near"])))
        randoms, _ = _draw_randoms(rng, n, self.config, False)
        r = dict(self.rc.render_transient(fields, randoms))
        zeros3 = torch.zeros_like(r["integrated_rgb"])
        r["transient_indirect"] = r["transient_indirect_viz"]           # render.py:503 (final value of the key)
        r["transient_direct"] = r["transient_direct_viz"]               # dark_level = 0
        for k in ("ambient_rgb", "ambient_diffuse_rgb", "ambient_specular_rgb"):   # use_ambient = False
            r[k] = zeros3
        r["normals_to_use"] = r["normals_pred"]
        r["ray_dists"] = r["ray_dists"][:, None]
        r["light_dists"] = r["light_dists"][:, None]
        for k in _FINAL_INTEGRATOR_KEYS:
            if k in r:
                r["cache_" + k] = r[k]
        r["vignette"] = torch.ones_like(r["integrated_rgb"][:, :1])
        lossmult = fields.get("lossmult")
        lm = torch.ones_like(r["vignette"]) if lossmult is None else self.rc._dev(lossmult).reshape(-1, 1)
        r["lossmult"] = lm * torch.ones_like(r["integrated_rgb"])
        return {"render": r, "main": {"integrator": r}, "cache_main": {"integrator": r}}

    def _apply_material(self, variables, rng, rays, env=None, mode="brdf", albedo_ratio=None):
        """passes ("cache", "light", "material") with use_material / use_light_sampler /
        MaterialModel.resample_render (stage material_light_from_scratch_resample; internal/models.py:1144-1254,
        1398-1694).  `rng`: the dict of explicit random tensors (see rc_material_randoms in include/rc_abi.h;
        oracle-compatible generator: oracle.material_ref.draw_randoms), or a uint32[2] key, from which the tensors are
        derived at the reference's split sites (prng.material_pass_randoms) on the device: bits and uniforms are those
        of the host twin bit for bit, normal and Gumbel values agree to a few ulp (rc.material_randoms).

        NOT parity-verified: the threefry primitives are pinned by published known answers, but the ~30 split sites
        material_pass_randoms restates by hand have never been compared with a jax run (none is possible in this
        pipeline): a mis-ordered split would yield a different, equally valid-looking stream.  Parity claims of the
        material stage are made on explicit random tensors only.

        env (a relight.EnvImage): the stage is relit under it (rc_render_relight): the image in place of the EnvMap and,
        in mode "env", the environment sampler in place of the stage's own (relight.relight_inputs says what `rng` holds
        then); albedo_ratio scales the albedo (material.py:2106-2116).  The output keys are the same."""
        import torch

        n_rays = int(np.prod(np.shape(rays.origins if isinstance(rays, Rays) else rays["origins"])[:-1]))
        if env is not None:
            from . import relight
            rng, picks_spec, picks_diff = relight.relight_inputs(env, rng, n_rays, self.config, mode)
            env._ensure_bound()
            self._ensure_variables(variables)
            fields = rays.hot_fields() if isinstance(rays, Rays) else dict(rays)
            cres, mres = self.rc.render_relight(fields, rng, mode, picks_spec, picks_diff, albedo_ratio)
            return self._material_outputs(cres, mres, fields)
        if albedo_ratio is not None:
            raise NotImplementedError("albedo_ratio is applied on the relighting path (env_map=)")
        if prng.is_key(rng):              # drawn in HBM by one launch; on the host for a handle
            # without the call (a stand-in that records calls)
            rng = prng.material_pass_randoms(rng, n_rays, self.config, rc=self.rc if hasattr(self.rc, "material_randoms") else None)
        if not isinstance(rng, dict):
            raise ValueError("the material stage needs a uint32[2] key or explicit random tensors: pass rng as the dict "
                             "described by rc_material_randoms")
        if "vmf_noise" not in rng:
            # the reference's constant: normal(random_split(PRNGKey(1))[0], [R, 1, 128, 3]) (light_sampler.py:135-144)
            rng = dict(rng, vmf_noise=prng.light_vmf_noise((n_rays, 1, self.config.num_vmf, 3))[:, 0])
        self._ensure_variables(variables)
        fields = rays.hot_fields() if isinstance(rays, Rays) else dict(rays)
        cres, mres = self.rc.render_material(fields, rng)
        return self._material_outputs(cres, mres, fields)

    def _material_outputs(self, cres, mres, fields):
        """The material stage's output dict from the two device tables (cache and material side)."""
        import torch

        cache = self._finalize(cres, fields)
        r = dict(mres)
        zeros3 = torch.zeros_like(r["rgb"])
        for k in ("indirect_occ", "material_roughness", "material_metalness", "material_F_0", "ray_dists", "light_dists"):
            r[k] = r[k][:, None]
        r["material_diffuseness"] = torch.zeros_like(r["material_F_0"])     # constants of the configured
        r["material_mirrorness"] = torch.zeros_like(r["material_F_0"])      # microfacet material
        r["occ"] = zeros3
        for k in ("distance_mean", "distance_median", "distance_percentile_5", "distance_percentile_95"):
            r[k] = cache[k]
        for k, v in cache.items():
            if k.startswith("cache_"):
                r[k] = v
        r["material_rgb"] = r["rgb"]
        r["normals"] = cache["normals"]
        r["normals_pred"] = cache["normals_pred"]
        r["vignette"] = torch.ones_like(r["rgb"][:, :1])
        r["lossmult"] = torch.ones_like(r["rgb"][:, :1])
        return {"render": r, "main": {"integrator": r}, "cache_main": {"integrator": cache}}

    def _finalize(self, dev: Dict[str, Any], fields) -> Dict[str, Any]:
        """Integrator keys + the aliases/constants of _finalize_outputs (internal/models.py:2074-2171)."""
        import torch

        r = dict(dev)
        zeros3 = torch.zeros_like(r["rgb"])
        # exact duplicates / exact zeros of the configured passive shader (internal/nerf.py:1044-1084)
        r["ambient_rgb"] = r["direct_rgb"]
        r["direct_diffuse_rgb"] = r["direct_rgb"]
        r["ambient_diffuse_rgb"] = r["direct_rgb"]
        for k in ("occ", "irradiance_rgb", "light_radiance_rgb", "n_dot_l_rgb", "direct_specular_rgb",
                  "ambient_specular_rgb"):
            r[k] = zeros3
        r["normals_to_use"] = r["normals_pred"]
        r["ray_dists"] = r["ray_dists"][:, None]
        r["light_dists"] = r["light_dists"][:, None]
        for k in _FINAL_INTEGRATOR_KEYS:
            if k in r:
                r["cache_" + k] = r[k]
        r["vignette"] = torch.ones_like(r["rgb"][:, :1])
        lossmult = fields.get("lossmult")
        lm = torch.ones_like(r["rgb"][:, :1]) if lossmult is None else self.rc._dev(lossmult).reshape(-1, 1)
        r["lossmult"] = lm * torch.ones_like(r["rgb"])
        return r


# ------------------------------------------------------------------------------------------------
# utils.shard / unshard, create_render_fn, render_image
# ------------------------------------------------------------------------------------------------
def shard(xs, n_local_devices: int = 1):
    """utils.shard (internal/utils.py:333-335) with jax.local_device_count() == 1 per process."""
    fn = lambda x: x.reshape((n_local_devices, -1) + tuple(x.shape[1:]))
    return xs.tree_map(fn) if isinstance(xs, (Rays, Pixels)) else fn(xs)


def unshard(x, padding: int = 0):
    """utils.unshard (internal/utils.py:338-343)."""
    y = x.reshape((x.shape[0] * x.shape[1],) + tuple(x.shape[2:]))
    return y[:-padding] if padding > 0 else y


def _strip_device_axis(a, ndim: int):
    """Arguments the Trainer replicates for pmap (flax.jax_utils.replicate) carry a leading [n_local_devices = 1]."""
    a = np.asarray(a)
    while a.ndim > ndim:
        a = a[0]
    return a


def _cast_pixels(model: Model, cameras, lights, pixels: Pixels, camtype) -> Rays:
    """camera_utils.cast_ray_batch(cameras, lights, pixels, camtype) (internal/camera_utils.py:1225-1329) on the device
    (rc_cast_rays): per-pixel camera lookup by `cam_idx`, rays with the batch shape of the pixels.  cameras =
    (pixtocams, camtoworlds, distortion_params, pixtocam_ndc[, z_range]) as the reference's tuple."""
    import torch

    from .camera import Camera
    if cameras is None or camtype is None:
        raise AssertionError("When passing Pixels into render_eval_fn, cameras and camtype needs to be not None. "
                             f"Got cameras={cameras} camtype={camtype}.")      # train_utils.py:3785-3789
    cams = tuple(cameras)
    z_range = None if len(cams) <= 4 or cams[4] is None else tuple(float(v) for v in np.asarray(_strip_device_axis(cams[4], 1)).reshape(-1)[:2])
    distortion = cams[2] if len(cams) > 2 else None
    ndc = None if len(cams) <= 3 or cams[3] is None else _strip_device_axis(cams[3], 2)
    ctype = getattr(camtype, "value", camtype)
    pixtocams = _strip_device_axis(cameras[0], 3)
    camtoworlds = _strip_device_axis(cameras[1], 3)
    lights = None if lights is None else _strip_device_axis(lights, 2)
    to_np = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    on_dev = lambda a: isinstance(a, torch.Tensor) and a.is_cuda
    sh = tuple(np.shape(pixels.near)[:-1])                      # batch shape SH; metadata fields are SH + [1]

    def cam(i):
        p2c = pixtocams if pixtocams.ndim == 2 else pixtocams[i]
        c2w = camtoworlds if camtoworlds.ndim == 2 else camtoworlds[i]
        light = None if lights is None else (lights if lights.ndim == 1 else lights[i])     # lights[cam_idx], :1288
        return Camera(pixtocam=p2c, camtoworld=c2w[:3, :4], light=light, near=0.0, far=0.0, camtype=ctype,
                      distortion_params=distortion, pixtocam_ndc=ndc, z_range=z_range)

    count = max([t.shape[0] for t in (pixtocams, camtoworlds) if t.ndim == 3], default=0)
    dev_idx = all(on_dev(a) for a in (pixels.cam_idx, pixels.pix_x_int, pixels.pix_y_int))
    if dev_idx:
        cam_idx, px, py = (a.reshape(-1).to(torch.int32) for a in (pixels.cam_idx, pixels.pix_x_int, pixels.pix_y_int))
        several = True                                          # not looked at on the host: the tables serve any mix
        if count == 0:                                          # one camera for every pixel, whatever cam_idx says
            count, cam_idx = 1, torch.zeros_like(cam_idx)
    else:
        cam_idx = to_np(pixels.cam_idx).reshape(-1).astype(np.int64)
        px = to_np(pixels.pix_x_int).reshape(-1).astype(np.int32)
        py = to_np(pixels.pix_y_int).reshape(-1).astype(np.int32)
        several = count > 0 and cam_idx.size > 0 and bool((cam_idx != cam_idx[0]).any())
        if several and not (0 <= int(cam_idx.min()) and int(cam_idx.max()) < count):
            raise IndexError(f"cam_idx outside [0, {count})")
    if px.shape[0] != cam_idx.shape[0]:
        raise ValueError("Pixels fields must share their batch shape")
    if not several:
        rays = model.rc.cast_rays(cam(int(cam_idx[0]) if count > 0 and cam_idx.shape[0] else 0), px, py)
    else:
        # one launch for any mix of cameras (rc_cast_rays_multi): the tables go up once per call, the indices stay
        # where they are; each ray is bitwise the one the single-camera call yields
        c2w = np.broadcast_to(camtoworlds, (count,) + camtoworlds.shape[-2:])
        cams = model.rc.camera_set(pixtocams, c2w, lights, 0.0, 0.0, ctype, distortion, ndc, z_range)
        rays = model.rc.cast_rays_multi(cams, cam_idx, px, py)
    dev = rays.origins.device
    meta = lambda a, dt=torch.float32: (a if on_dev(a) else torch.as_tensor(to_np(a))).to(device=dev, dtype=dt).reshape(sh + (1,))
    rays = rays.tree_map(lambda t: t.reshape(sh + (t.shape[-1],)))
    return rays.replace(lossmult=meta(pixels.lossmult), near=meta(pixels.near), far=meta(pixels.far),
                        cam_idx=meta(pixels.cam_idx, torch.int32), light_idx=meta(pixels.light_idx, torch.int32),
                        pix_x_int=pixels.pix_x_int, pix_y_int=pixels.pix_y_int)


def create_render_fn(model: Model, dataset: Any = None, mapping_fn: Any = None):
    """train_utils.create_render_fn(model, dataset, mapping_fn) (internal/train_utils.py:3742-3831).

    Returns `render_eval_pfn(variables, rng, train_frac, cameras, lights, rays, passes, resample=None)` ->
    (renderings, rng), called exactly as at engine/trainer.py:822-832.  One process drives one GPU, so the pmap axes
    have size 1: `rng` is the per-device key array [1, 2] (or a single key / None / seed / dict, see the module
    docstring), `rays` is sharded [1, m, .] (or a `Pixels` batch, cast on the device), and every value of the result
    carries the [n_dev = 1, n_dev = 1, m, ...] leading axes of pmap + all_gather so `unshard(v[0], padding)` applies
    unchanged.  `mapping_fn` (jax.pmap / jax.vmap in the reference) has nothing to map here and is ignored.
    `dataset` supplies `camtype` for the Pixels branch; a dataset whose `env_map` is set (an EnvImage, or the reference's arrays
    env_map / env_map_w / _h / _pmf / _pdf / _dirs) relights: the image and `albedo_ratio` go to every model.apply call as
    the reference's render_eval_fn hands them on.  `dataset.mesh` must be unset."""
    camtype = getattr(dataset, "camtype", None) if dataset is not None else None
    if dataset is not None and getattr(dataset, "mesh", None) is not None:
        raise NotImplementedError("dataset.mesh is not part of the accelerated path")
    # dataset.env_map and its tables: handed to model.apply with every call (train_utils.py:3796-3812), uploaded and bound
    # once here
    env_kwargs = {}
    if dataset is not None and getattr(dataset, "env_map", None) is not None:
        from . import relight
        env_kwargs["env_map"] = relight.as_env_image(model.rc, dataset.env_map, {
            k: getattr(dataset, k, None) for k in ("env_map_w", "env_map_h", "env_map_pmf", "env_map_pdf", "env_map_dirs")})
        if getattr(dataset, "albedo_ratio", None) is not None:
            env_kwargs["albedo_ratio"] = dataset.albedo_ratio

    def render_eval_pfn(variables, rng, train_frac, cameras, lights, rays, passes, resample=None):
        if isinstance(rays, Pixels):
            rays = _cast_pixels(model, cameras, lights, rays, camtype)
        dev_keys = isinstance(rng, np.ndarray) and rng.dtype == np.uint32 and rng.shape == (1, 2)
        key = rng[0] if dev_keys else rng
        if prng.is_key(key):
            apply_key, next_key = prng.chunk_keys(key)
            next_rng = next_key[None] if dev_keys else next_key
        else:
            apply_key, next_rng = rng, rng
        out = model.apply(variables, apply_key, rays, train_frac=train_frac, train=False, passes=tuple(passes),
                          resample=resample, compute_extras=True, **env_kwargs)
        render = out["render"]
        if isinstance(render, RenderDict):
            render = render.with_lead(2)
        else:
            render = {k: v[None, None] for k, v in render.items()}
        return render, next_rng

    render_eval_pfn.device = model.device
    render_eval_pfn.model = model
    render_eval_pfn.plain = True           # made by create_render_fn: a bound closure may be short-cut (bind_render_fn)
    return render_eval_pfn


def bind_render_fn(render_eval_pfn, variables=None, train_frac: float = 1.0, cameras=None, lights=None):
    """The closure Trainer.render_primary_rays hands to render_image (engine/trainer.py:821-832):
    render_fn(rng, rays, passes, resample) -> render_eval_pfn(variables, rng, train_frac, cameras, lights, rays, ...)."""

    def render_fn(rng, rays, passes, resample=None):
        return render_eval_pfn(variables, rng, train_frac, cameras, lights, rays, passes, resample)

    render_fn.device = getattr(render_eval_pfn, "device", None)
    render_fn.model = getattr(render_eval_pfn, "model", None)
    # render_image's device loop may call the model directly for the plain cache pass: this closure adds nothing to
    # what Model.apply receives but `variables`
    render_fn.variables = variables
    render_fn.direct_ok = render_fn.model is not None and train_frac == 1.0 and getattr(render_eval_pfn, "plain", False)
    return render_fn


_STAT_KEYS = ("rgb", "integrated_rgb", "lighting_irradiance", "direct_rgb", "indirect_rgb", "material_rgb",
              "specular_rgb", "diffuse_rgb", "material_albedo", "acc")
_VAR_KEYS = ("rgb", "integrated_rgb")
_TRANSIENT_KEEP = ("transient_direct_viz", "transient_indirect_viz")


def _skip_key(k: str) -> bool:
    """`transient*` outputs stay out of an image, the two visualisations excepted."""
    return ("transient" in k) and (k not in _TRANSIENT_KEEP)


class _RepeatMean:
    """Running (Welford) mean of one chunk's {key: array} over its repeats, numpy arrays or torch tensors alike.
    `_STAT_KEYS` are averaged, every other key keeps the first repeat's value (a mean of unit normals is not a unit
    normal) and the first repeat's arrays are never written to.  With `variance`, M2 is kept for `_VAR_KEYS` and comes
    back as `<key>_variance` = M2 / (n - 1) * n.  One repeat has nothing to average: render_image does not come here
    for it, and its sink writes the zero variance images."""

    def __init__(self, variance: bool = False):
        self.n, self.variance, self.mean, self.m2 = 0, variance, {}, {}

    def add(self, cur):
        self.n += 1
        if self.n == 1:
            for k, v in cur.items():
                tensor = hasattr(v, "clone")
                self.mean[k] = v if k not in _STAT_KEYS else v.clone() if tensor else v.copy()
                if self.variance and k in _VAR_KEYS:
                    self.m2[k] = v.new_zeros(v.shape) if tensor else np.zeros_like(v)
            return
        for k, mean in self.mean.items():
            if k in _STAT_KEYS:
                delta = cur[k] - mean
                mean += delta / self.n
                if k in self.m2:
                    self.m2[k] += delta * (cur[k] - mean)

    def result(self):
        out = dict(self.mean)
        for k, v in self.m2.items():
            out[f"{k}_variance"] = (v / (self.n - 1)) * self.n if self.n > 1 else v
        return out


def render_image(render_fn, rng, rays: Rays, config, passes: Tuple[str, ...], verbose: bool = True,
                 resample: Any = None, num_repeats: int = 1, compute_variance: bool = False):
    """models.render_image: `rays` [H, W, .] are rendered in batches of `config.render_chunk_size` rays, the last one
    edge-padded to a full chunk, and assembled row-major into {key: [H, W, ...]} numpy arrays of render_fn's dtypes.
    `render_fn(rng, rays [1, m, .], passes, resample)` -> ({key: [1, 1, m, ...]}, rng); the rng it hands back goes into
    the next call, the last one is returned.  With `num_repeats` > 1 every chunk is rendered that often and averaged
    (`_RepeatMean`); `compute_variance` adds `rgb_variance` / `integrated_rgb_variance`, zeros for a single repeat.
    `transient*` keys but the two visualisations are left out.

    A foreign callable gets host slices of the rays, and its results are brought to numpy chunk by chunk.  When
    `render_fn` comes from this module (`render_fn.device` names a GPU) the same loop stays on the device
    (`_device_state`): the rays are uploaded once, every chunk is enqueued without a host synchronisation, the results
    stay in HBM, and the image is unpacked and copied to the host ONCE at the end; aliased keys (`cache_rgb` is `rgb`)
    share one array."""
    height, width = rays.origins.shape[:2]
    num_rays = height * width
    chunk = config.render_chunk_size
    n_chunks = -(-num_rays // chunk)
    padding = n_chunks * chunk - num_rays
    dev = getattr(render_fn, "device", None)
    mdl = getattr(render_fn, "model", None) if dev is not None else None
    sink = _ImageSink(height, width, chunk, compute_variance)
    join = row = None
    on_stream = lambda i: contextlib.nullcontext()
    start = time.time()
    if dev is None:
        flat = rays.tree_map(lambda r: np.asarray(r).reshape((num_rays, -1)) if np.size(r) >= num_rays else np.asarray(r))

        def chunk_rays(i):
            sub = flat.tree_map(lambda r: r[i * chunk: (i + 1) * chunk])
            if padding and i == n_chunks - 1:
                sub = sub.tree_map(lambda r: np.pad(r, ((0, padding), (0, 0)), mode="edge"))
            return shard(sub)

    def strip(v):                          # [1, 1, m, ...] -> [m, ...]; a foreign callable's results come to the host
        v = v[0]
        if dev is None:
            v = np.array(v.cpu().numpy() if hasattr(v, "cpu") else v)
        return v.reshape((-1,) + tuple(v.shape[2:]))

    try:
        if dev is not None:
            chunk_rays, on_stream, join, row = _device_state(render_fn, mdl, dev, rng, rays, chunk, n_chunks, padding,
                                                             passes, resample, num_repeats)
        for i_chunk in range(n_chunks):
            if verbose and i_chunk % max(1, n_chunks // 10) == 0:
                print(f"Rendering chunk {i_chunk}/{n_chunks-1}")
            if row is not None:                                        # already enqueued: only the sink is filled
                sink.add(row(i_chunk))
                continue
            crays = chunk_rays(i_chunk)
            with on_stream(i_chunk):
                acc = _RepeatMean(compute_variance) if num_repeats > 1 else None
                for _ in range(num_repeats):
                    cur, rng = render_fn(rng, crays, passes, resample)
                    if acc is None and dev is not None and isinstance(cur, RenderDict):
                        if mdl is not None:
                            mdl._variables_checked = True              # the variable tree: on the first chunk only
                        continue
                    cur = {k: strip(v) for k, v in cur.items() if not _skip_key(k)}
                    if acc is not None:
                        acc.add(cur)
                sink.add(cur if acc is None else acc.result())
    finally:
        if mdl is not None:
            mdl._variables_checked = False
            mdl._out_arena = None
    if join is not None:
        join()
    rendering = sink.finish(num_rays)
    if verbose:
        print("Milliseconds per ray", (time.time() - start) * 1000 / num_rays)
    return rendering, rng


class _ImageSink:
    """Per-chunk results of render_image -> [H, W, ...] numpy arrays: chunks are contiguous and row-major, so the image
    is their concatenation, trimmed to `num_rays` once.  RenderDicts over one layout are kept as their flat buffers
    only; the image is assembled on the device (one gather per distinct region) into a key-major buffer that is copied
    to the host once; aliased keys share a numpy array.  Anything else (dicts of numpy arrays or tensors, means over
    repeats with their variances) goes key by key.  With `compute_variance`, a variance image that no chunk brought
    (a single repeat) is zeros."""

    def __init__(self, height, width, chunk, compute_variance):
        self.h, self.w, self.chunk, self.var = height, width, chunk, compute_variance
        self.flats, self.layout, self.consts, self.extras = [], None, None, []
        self.generic = []                  # per chunk {key: [chunk, ...] array}

    def add(self, cur):
        if isinstance(cur, RenderDict):
            if self.layout is None:
                self.layout, self.consts = cur.layout, cur.consts
            if cur.layout is self.layout and not self.generic:
                self.flats.append(cur.flat)
                self.extras.append(cur.extras)
                return
            cur = {k: cur[k][0, 0] if cur.lead == 2 else cur[k] for k in cur if not _skip_key(k)}
        if self.flats:
            raise RuntimeError("render_fn changed its result type between chunks")
        self.generic.append(cur)

    def finish(self, num_rays):
        H, W = self.h, self.w
        out: Dict[str, np.ndarray] = {}
        if self.flats:
            import torch
            A = torch.stack(self.flats)                                # [n_chunks, flat_size]
            regions, order = {}, []
            for k, ent in self.layout.items():
                if _skip_key(k):
                    continue
                if ent not in regions:
                    regions[ent] = None
                    order.append(ent)
            sizes, total = {}, 0
            for ent in order:
                kind, a, shape = ent
                width = int(np.prod(shape[1:])) if len(shape) > 1 else 1
                if kind == "const":
                    continue
                sizes[ent] = (total, width)
                total += num_rays * width
            packed = torch.empty(total, dtype=torch.float32, device=A.device)
            m = self.chunk
            for ent, (off, width) in sizes.items():
                kind, a, shape = ent
                dst = packed[off: off + num_rays * width].view(num_rays, width)
                if kind == "flat":
                    dst.copy_(A[:, a: a + m * width].reshape(-1, width)[:num_rays])
                else:                                                  # per-chunk extra tensors (lossmult)
                    dst.copy_(torch.cat([e[a].reshape(m, width) for e in self.extras])[:num_rays])
            host = np.empty(total, dtype=np.float32)
            torch.from_numpy(host).copy_(packed)                       # the one device-to-host copy (synchronises)
            arrays = {}
            for ent in order:
                kind, a, shape = ent
                tail = tuple(shape[1:])
                if kind == "const":
                    arrays[ent] = np.full((H, W) + tail, a, dtype=np.float32)
                else:
                    off, width = sizes[ent]
                    arrays[ent] = host[off: off + num_rays * width].reshape((H, W) + tail)
            for k, ent in self.layout.items():
                if not _skip_key(k):
                    out[k] = arrays[ent]
        for k in (self.generic[0] if self.generic else ()):
            parts = [c[k] for c in self.generic]
            if isinstance(parts[0], np.ndarray):
                v = np.concatenate(parts)[:num_rays]
            else:
                import torch
                v = torch.cat(parts)[:num_rays].cpu().numpy()
            out[k] = v.reshape((H, W) + tuple(v.shape[1:]))
        if self.var:
            for k in _VAR_KEYS:
                if k in out and f"{k}_variance" not in out:
                    out[f"{k}_variance"] = np.zeros_like(out[k])
        return out


def _device_state(render_fn, mdl, dev, rng, rays, chunk, n_chunks, padding, passes, resample, num_repeats):
    """What render_image sets up once when the chunks stay on GPU `dev`: `chunk_rays(i)`, chunk i of the rays uploaded
    once as [n_chunks, 1, chunk, .] (edge padding and utils.shard done); `on_stream(i)`, the context of the stream
    chunk i runs on (two streams forked from the current one); `join()`, which makes the current stream wait for them;
    `row`, None or (direct path) row(i) -> the RenderDict of chunk i after ALL chunks were enqueued here.  For one repeat
    of this package's own model the chunks write into rows of ONE zero-filled arena made here, on the main stream the
    pool forks from (no allocation + fill launch per chunk); it is left in `mdl._out_arena`, which the caller resets."""
    import torch

    device = torch.device("cuda", dev)
    num_rays = n_chunks * chunk - padding

    def upload(r):
        t = r if isinstance(r, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(r))
        if t.numel() < num_rays:
            return t.to(device)
        t = t.to(device).reshape(num_rays, -1)
        if padding:                                                    # np.pad(mode="edge") of the last chunk
            t = torch.cat([t, t[-1:].expand(padding, -1)])
        return t.reshape(n_chunks, 1, chunk, -1)

    main = torch.cuda.current_stream(device)
    drays = rays.tree_map(upload)
    names = [k for k, v in vars(drays).items() if v is not None and v.dim() == 4]
    cols = {k: getattr(drays, k).unbind(0) for k in names}
    rest = {k: v for k, v in vars(drays).items() if k not in names}
    pool = [torch.cuda.Stream(device=device), torch.cuda.Stream(device=device)] if n_chunks > 1 else [main]
    arena = None
    if (mdl is not None and num_repeats == 1 and n_chunks > 1 and "material" not in passes
            and getattr(mdl.config, "transient", None) is None and hasattr(mdl, "_plan")):
        total = mdl._plan(chunk, "is_secondary" in passes, "lossmult" in names)[0][0]
        arena = torch.zeros((n_chunks, total), dtype=torch.float32, device=device)
        mdl._out_arena = (arena, 0)
    ready = torch.cuda.Event()
    ready.record(main)
    for s in pool:
        s.wait_event(ready)

    def join():
        for s in pool:
            main.wait_stream(s)

    # Direct path for the plain deterministic cache pass of this package's own model (rng None: nothing to thread from
    # chunk to chunk): the calls render_fn -> render_eval_pfn -> Model.apply would make, looped over the chunks in the
    # library (rc_render_chunks: chunk i on stream i % 2 into row i of the arena; host time per chunk 38 -> ~15 us)
    row = None
    if (arena is not None and rng is None and tuple(passes) == ("cache",) and not resample
            and getattr(render_fn, "direct_ok", False)):
        hot = [k for k in names if k in ("origins", "directions", "viewdirs", "near", "far", "lights", "lossmult")]
        rc_plan, layout = mdl._plan(chunk, False, "lossmult" in names)
        mdl._ensure_variables(getattr(render_fn, "variables", None))
        full = {k: getattr(drays, k) for k in hot if k != "lossmult"}
        mdl.rc.render_chunks(full, chunk, n_chunks, rc_ext.RC_PASS_CACHE, rc_plan, arena, [s.cuda_stream for s in pool])
        lossmult = cols["lossmult"] if "lossmult" in hot else None

        def row(i):
            extras = (lossmult[i][0].reshape(-1, 1).expand(-1, 3),) if lossmult is not None else ()
            return RenderDict(arena[i], layout, mdl._consts, extras)

    chunk_rays = lambda i: Rays(**rest, **{k: cols[k][i] for k in names})
    on_stream = lambda i: torch.cuda.stream(pool[i % len(pool)])
    return chunk_rays, on_stream, join, row


# ------------------------------------------------------------------------------------------------
# Multi-GPU: one process per GPU, rays sharded at image granularity, one all-gather per image
# ------------------------------------------------------------------------------------------------
GATHER_KEYS = ("rgb", "acc", "distance_median", "normals_pred")


def shard_bounds(num_rays: int, rank: int, world: int) -> Tuple[int, int]:
    """Static contiguous split: rank r owns rays [r*ceil(N/G), ...)."""
    per = -(-num_rays // world)
    lo = min(rank * per, num_rays)
    return lo, min(lo + per, num_rays)


def _advance_rng(rng, rank: int, first: bool):
    """Per-chunk random stream of a rank: the key is folded with the rank once (ranks draw different numbers, as the
    per-device keys of the reference's pmap do), then threaded from chunk to chunk like render_image threads the key
    render_fn hands back (prng.chunk_keys).  Returns (key for this chunk, carry for the next one).  Seeds / Generators advance by themselves; dicts of explicit tensors and None pass."""
    if prng.is_key(rng):
        if first:
            rng = prng.fold_in(rng, rank)
        return prng.chunk_keys(rng)
    if first and isinstance(rng, (int, np.integer)):
        rng = np.random.Generator(np.random.PCG64([int(rng), rank]))
    return rng, rng


_PINNED: Dict[Tuple[int, ...], Any] = {}


def _to_host_once(t):
    """One device-to-host copy of a [rays, columns] float32 tensor into a (cached) pinned buffer; returns numpy."""
    import torch
    if not t.is_cuda:
        return t.numpy()
    shape = tuple(t.shape)
    host = _PINNED.get(shape)
    if host is None:
        _PINNED.clear()                                   # one image size at a time: do not hoard pinned memory
        host = _PINNED[shape] = torch.empty(shape, dtype=torch.float32, pin_memory=True)
    host.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return host.numpy().copy()                            # the caller owns its arrays; the staging buffer is reused


def render_image_distributed(model_apply, rng, rays: Rays, config, passes=("cache",), keys=GATHER_KEYS,
                             group=None, device=None, key_widths: Optional[Dict[str, int]] = None,
                             num_repeats: int = 1, to_host: bool = False):
    """Each rank renders its contiguous share of the image in `render_chunk_size` batches, keeps the
    results on its device, packs the consumed keys into one [rays_per_rank, sum(widths)] buffer and
    issues ONE all_gather per image (the reference all-gathers the whole ~45-key dict per chunk per
    repeat, internal/train_utils.py:3795-3815).  With num_repeats > 1 the repeats of a chunk are averaged on the
    device BEFORE the gather, by the `_RepeatMean` of render_image: the mean of the reference's
    stat_keys (`_STAT_KEYS`), the first repeat of every other key.

    model_apply(rng, rays) -> {"render": {key: tensor[n, ...]}}; runs on "nccl" (= RCCL over xGMI)
    with the HIP model and on "gloo" with any CPU callable (tests).  `device`: where a rank with an empty shard
    allocates its (all-padding) contribution; defaults to the current cuda device under the nccl backend.
    `to_host=True` returns float32 numpy arrays, as `render_image` does (internal/models.py:2448-2450 copies every chunk of
    every key; here the gathered keys cross PCIe as ONE device-to-host copy per image, into a pinned staging buffer)."""
    import torch
    import torch.distributed as dist

    on = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if on else 1
    rank = dist.get_rank(group) if on else 0
    widths = dict(rc_ext.OUTPUTS)
    if key_widths:
        widths.update(key_widths)
    cols = np.cumsum([0] + [widths[k] for k in keys])
    height, width = rays.origins.shape[:2]
    num_rays = height * width
    numel = lambda r: r.numel() if hasattr(r, "numel") else np.size(r)
    flat = rays.tree_map(lambda r: (r if hasattr(r, "reshape") else np.asarray(r)).reshape((num_rays, -1))
                         if numel(r) >= num_rays else r)
    lo, hi = shard_bounds(num_rays, rank, world)
    per = -(-num_rays // world)
    chunk = config.render_chunk_size
    buf = None
    first = True
    for idx0 in range(lo, hi, chunk):
        sub = flat.tree_map(lambda r: r[idx0: min(idx0 + chunk, hi)])
        m = min(idx0 + chunk, hi) - idx0
        acc = _RepeatMean() if num_repeats > 1 else None
        for _ in range(num_repeats):
            key, rng = _advance_rng(rng, rank, first)
            first = False
            out = model_apply(key, sub)["render"]
            if acc is not None:
                acc.add({k: out[k] for k in keys})
        if acc is not None:
            out = acc.result()
        mean = torch.cat([out[k].reshape(m, -1) for k in keys], dim=1)
        if buf is None:
            dev = device or mean.device
            buf = torch.zeros((per, int(cols[-1])), dtype=torch.float32, device=dev)
        buf[idx0 - lo: idx0 - lo + m] = mean
    if buf is None:
        if device is None:
            nccl = on and dist.get_backend(group) == "nccl"
            device = torch.device("cuda", torch.cuda.current_device()) if nccl else "cpu"
        buf = torch.zeros((per, int(cols[-1])), dtype=torch.float32, device=device)
    if on:        # also with one rank: the collective (RCCL under "nccl") then runs the way it does with eight
        gathered = torch.empty((world * per, int(cols[-1])), dtype=torch.float32, device=buf.device)
        if buf.is_cuda:
            dist.all_gather_into_tensor(gathered, buf, group=group)
        else:
            dist.all_gather(list(gathered.chunk(world, dim=0)), buf, group=group)
    else:
        gathered = buf
    if to_host:
        gathered = _to_host_once(gathered[:num_rays])
    result = {}
    for i, k in enumerate(keys):
        v = gathered[:num_rays, cols[i]: cols[i + 1]]
        result[k] = v.reshape((height, width) + ((widths[k],) if widths[k] > 1 else ()))
    return result
