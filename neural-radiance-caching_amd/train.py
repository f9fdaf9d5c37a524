"""First piece of the training path: gradients of the proposal levels' density fields and
their data-parallel reduction.

The reference's train step (internal/train_utils.py:3100-3177) is `jax.value_and_grad(loss_fn)` over the whole
model followed by `jax.lax.pmean(grad, "batch")` across devices and the optimizer.  Here:

  * `density_grads(rc, level, points, d_density, d_feature)` -> {tensor name: gradient} for the hash-grid tables and
    the density MLP of one level (rc_density_backward: hand-written backward on the matrix cores + atomic scatter
    into the tables), named like the reference's parameter tree so an optimizer keyed on those names can consume it;
  * `allreduce_grads(flat_buffers)` -> the pmean: ONE all-reduce per level over the flat gradient buffer
    (torch.distributed; backend "nccl" = RCCL over xGMI on the GPUs, "gloo" in the CPU tests).  The buffers are the
    bucket: ~45-180 MB per level, large enough to run the xGMI ring at its per-link bound, no per-tensor launches.

  * `interlevel_grads(rc, rays, jitters, train_frac)` -> the spline interlevel loss of the proposal samplers
    (loss_utils.spline_interlevel_loss) and the exact gradients of both proposal networks, in one device call
    (rc_interlevel_backward: training forward, loss backward to the densities, density backward of levels 0 and 1);
  * `anneal_at(train_frac)` -> the train-time resampling exponent of the proposal sampler;
  * `data_grads(rc, rays, rgb, jitters, train_frac)` -> the charb data loss of the cache pass
    (train_utils.compute_data_loss) and the exact gradients of the last density level (MLP_2) and the shader side
    (pred_normals_layer, appearance grid, Cache/Shader layers), in one device call (rc_data_backward: training forward,
    loss backward through the compositing, shader recompute + backward, density and appearance-grid backward).

  * `geometry_grads(rc, rays, jitters, train_frac)` -> the distortion, orientation, predicted-normal and reverse
    predicted-normal losses of the last sampler level (loss_utils.py:108-201) and their exact gradients of MLP_2 and
    pred_normals_layer, in one device call (rc_geometry_backward: training forward, per-ray loss backward, density
    backward); `normal_weight_ease(train_frac)` -> the ease the predicted-normal terms are scaled by;
  * `mask_grads(rc, rays, jitters, train_frac, masks, ...)` -> the mask loss of the last level's opacity
    (train_utils.compute_mask_loss) and, given the cameras' look vectors and the backward rays' draws, its backward term
    (train_utils._compute_backward_mask_loss: rc_backward_mask_rays, then the same loss with zero masks), with their
    exact gradients of MLP_2 (rc_mask_backward: sampler-only training forward, per-ray loss backward, density
    backward); `mask_terms(train_frac)` -> the weights with the mask-weight decay / ease folded in;
  * `cache_stage_grads(rc, rays, rgb, jitters, train_frac)` -> the cache-stage loss: interlevel, data and geometry
    terms counted for "main" and "cache_main", the density-grid regularizer once, with the per-level and shader
    gradients and a loss dict keyed like the reference's losses_flat (the light / material grid regularizer keys left
    out, see its docstring); with mask_cfg the two mask terms as well; with smoothness_cfg the geometry smoothness term;
  * `geometry_smoothness_grads(rc, rays, jitters, noise, train_frac)` -> the geometry_smoothness extra loss of the stages
    without a material and its exact gradient of MLP_2 THROUGH the analytic normals at the sample means and at the
    perturbed means (rc_geometry_smoothness_backward on rc_normals_backward, DESIGN.md §4.23: second order in the density
    field); `geometry_smoothness_terms(train_frac)` -> the weights with the extra loss's mult folded in.

The terms above geometry_smoothness_grads are all first order here (the analytic normals are stop-gradiented where they appear).  The
predicted-normal terms follow that first-order reading; whether it matches the reference is not settled (DESIGN.md,
Oddities: train_utils.py:1060-1070 passes gt="normals_pred", pred="normals" to the forward term, and
nerf_ngp_yobo.gin:57 disables the analytic normals).

The optimizer:

  * `learning_rate_decay(step, ...)` -> math.learning_rate_decay (internal/math.py:356-409) in float32;
    `param_group(name, cfg)` -> which of create_optimizer's chained Adams (train_utils.py:3834-3934) updates a tensor;
    `adam_scalars(count, cfg)` -> the per-group float32 scalars of one step;
  * `CacheStageOptimizer(rc, cfg)` -> flat params / mu / nu in the four gradient layouts, one rc_adam_update per step
    (nan_to_num, clip_gradients, optax.adam, apply_updates) and the stream-ordered refresh of the handle
    (rc_load_params_flat per layout);
  * `cache_stage_step(rc, opt, rays, rgb, jitters)` -> one reference train step (train_utils.py:3128-3161) of the
    cache stage: cache_stage_grads into the optimizer's gradient buffers, the pmean, the update.

The light sampler, first piece of the material_light_from_scratch stage:

  * `light_sampling_grads(rc, rays, randoms, train_frac)` -> the light_sampling loss (train_utils.light_sampling_loss ->
    render_utils.vmf_loss_fn) and the light_grid regularizer with their exact gradients of the LightSampler parameters
    (rc_light_sampling_backward: the material forward up to the secondary trace, the loss backward, the light head's
    backward and the light grid's scatter; rc_light_regularizer);
  * `LightSamplerOptimizer(rc, cfg)` / `light_sampler_step(...)` -> the same optimizer state and step on the one light
    layout (group "LightSampler").  The LightSampler's gradient from the material data loss (through the vMF-sampled
    directions) is not part of these.

The material network, second piece of that stage:

  * `material_smoothness_grads(rc, rays, randoms, noise, train_frac)` -> the material_smoothness loss
    (train_utils.material_smoothness_loss), the material_grid regularizer and material_ray_sampler (identically 0 for
    hotdog) with the exact gradients of the MaterialShader parameters (rc_material_smoothness_backward: the primary pass
    and shading point, both material evaluations and the head's backward in one kernel, the material grid's scatter;
    rc_material_regularizer);
  * `MaterialOptimizer(rc, cfg)` / `material_step(...)` -> the optimizer state and step on the material layout (group
    "MaterialShader").  The material data loss's gradient (the Disney-GGX integration) is not part of these.

The time-resolved cache, first piece of its training:

  * `transient_data_grads(rc, rays, cam_origins, jitters, gt, ...)` -> the transient data loss
    (train_utils.compute_transient_data_loss) of rc_render_transient's histograms and the exact gradient of the two per-bin
    head layers; the adjoints at the rest of the shader stay in the handle's "td:" workspace.  cfg picks the reading:
    'rawnerf_transient_unbiased' by default (rc_transient_data_backward), or through rc_transient_data_backward_kind the
    per-bin types 'rawnerf_transient', 'mse', 'mse_unbiased' and the iToF types 'mse_itof', 'rawnerf_transient_itof' and
    their unbiased forms, with or without use_itof -- config.transient_data_loss_preset("cornell_itof"), "steady_state",
    "mse", ... name the gins' readings;
  * `TransientHeadOptimizer(rc, cfg)` / `transient_head_step(...)` -> the optimizer state and step on that layout
    (transient_indirect_layer in group "Cache", SurfaceLightField/output_rgba_layer in group "SurfaceLightField").
"""
from __future__ import annotations

import dataclasses
from typing import Dict, Iterable, List, Optional

import numpy as np

from . import prng
from .config import (DataLossConfig, GeometryLossConfig, GeometrySmoothnessConfig, InterlevelConfig, LightSamplingConfig, MaskLossConfig,
                     MaterialDataLossConfig, MaterialSmoothnessConfig, OptimizerConfig, TransientDataLossConfig)


def grads_as_dict(flat, layout) -> Dict[str, object]:
    """Views of the flat gradient buffer by tensor name (layout: RadianceCache.density_grad_layout(level)[0])."""
    return {name: flat[off: off + int(np.prod(shape))].reshape(shape) for name, off, shape in layout}


def density_grads(rc, level: int, points, d_density, d_feature=None, flat=None):
    """-> ({name: gradient view}, flat buffer, density [n])."""
    layout, _ = rc.density_grad_layout(level)
    flat, density = rc.density_backward(level, points, d_density, d_feature, flat)
    return grads_as_dict(flat, layout), flat, density


def allreduce_grads(buffers: Iterable, average: bool = True, group=None) -> List:
    """jax.lax.pmean(grad, axis_name="batch") (internal/train_utils.py:3133-3135) for per-level flat gradient
    buffers: one in-place all-reduce each, divided by the world size."""
    import torch.distributed as dist

    buffers = list(buffers)
    if not dist.is_available() or not dist.is_initialized() or dist.get_world_size(group) == 1:
        return buffers
    world = dist.get_world_size(group)
    handles = [dist.all_reduce(b, op=dist.ReduceOp.SUM, group=group, async_op=True) for b in buffers]
    for b, hnd in zip(buffers, handles):
        hnd.wait()
        if average:
            b.div_(world)
    return buffers


def anneal_at(train_frac: float, cfg: InterlevelConfig = InterlevelConfig()) -> float:
    """clip(bias(train_frac / anneal_end, anneal_slope), 0, anneal_clip), bias(x, s) = s x / ((s - 1) x + 1)
    (Schlick's bias, internal/sampling.py:326-335).  anneal_at(1) = 0.4 = RenderConfig.anneal."""
    x = float(train_frac) / cfg.anneal_end
    s = cfg.anneal_slope
    return float(min(max((s * x) / ((s - 1.0) * x + 1.0), 0.0), cfg.anneal_clip))


def interlevel_grads(rc, rays, jitters, train_frac: float, lossmult=None, flats: Optional[List] = None,
                     cfg: InterlevelConfig = InterlevelConfig(), levels=None):
    """The spline interlevel loss of a batch and its gradients (rc_interlevel_backward).
    rays: the ray dict of render_rays; jitters: per-level [n] sampler jitter (None = deterministic); train_frac sets
    the anneal; lossmult: [n] or None; flats: per proposal level a flat gradient buffer to accumulate into (allocated
    zeroed when None).  -> ({level: {tensor name: gradient view}}, flats, losses [num_levels - 1]) -- the flats are what
    allreduce_grads averages across ranks; each rank's losses are its local batch mean."""
    flats, losses = rc.interlevel_backward(rays, jitters, anneal_at(train_frac, cfg), cfg.mults, cfg.blurs, lossmult,
                                           flats, levels)
    grads = {}
    for level, flat in enumerate(flats):
        if flat is not None:
            grads[level] = grads_as_dict(flat, rc.density_grad_layout(level)[0])
    return grads, flats, losses


# The shader side of the data loss's gradient (rc_shader_grad_layout): [(name, (in, out))] of the dense layers, with the
# appearance-grid tables (rc_hashgrid_grad_layout(3)) between pred_normals_layer and the Cache/Shader layers.
SHADER_DENSE_LAYERS = (
    ("Cache/Shader/bottleneck_layer", (96, 128)),
    ("Cache/Shader/roughness_layer", (96, 1)),
    ("Cache/Shader/ambient_irradiance_layer", (96, 3)),
    ("Cache/Shader/tint_layer", (96, 3)),
    ("Cache/Shader/irradiance_layer", (96, 3)),
    ("Cache/Shader/integrated_brdf_layers_0", (129, 64)),
    ("Cache/Shader/integrated_brdf_layers_1", (64, 64)),
    ("Cache/Shader/output_integrated_brdf_layer", (64, 1)),
    ("Cache/Shader/SurfaceLightField/layer_0", (200, 128)),
    ("Cache/Shader/SurfaceLightField/layer_1", (128, 128)),
    ("Cache/Shader/SurfaceLightField/layer_2", (128, 128)),
    ("Cache/Shader/SurfaceLightField/layer_bottleneck", (328, 128)),
    ("Cache/Shader/SurfaceLightField/output_ambient_rgb_layer", (128, 3)),
)


def shader_grad_layout(cfg, appearance_tables):
    """Python mirror of rc_shader_grad_layout: [(name, offset, shape)] and the total size.  appearance_tables: the
    [(name, shape)] of the appearance grid's tables in level order (rc_hashgrid_grad_layout(3))."""
    out, off = [], 0

    def add(name, shape):
        nonlocal off
        out.append((name, off, tuple(shape)))
        off += int(np.prod(shape))

    def dense(path, shape):
        add(f"params/{path}/kernel", shape)
        add(f"params/{path}/bias", (shape[1],))

    dense(f"Cache/Sampler/MLP_{cfg.num_levels - 1}/pred_normals_layer", (64, 3))
    for name, shape in appearance_tables:
        add(name, shape)
    for path, shape in SHADER_DENSE_LAYERS:
        dense(path, shape)
    return out, off


def data_grads(rc, rays, rgb, jitters, train_frac: float, lossmult=None, flats=None, cfg: DataLossConfig = DataLossConfig(),
               anneal_cfg: InterlevelConfig = InterlevelConfig()):
    """The cache pass's charb data loss of a batch against target colours rgb [n, 3] and its gradients
    (rc_data_backward).  jitters: per-level [n] sampler jitter (None = deterministic); train_frac sets the anneal
    (anneal_at); lossmult: [n] or None; flats: (density flat, shader flat) to accumulate into (allocated zeroed when
    None).  -> ({"MLP_2": {name: view}, "Shader": {name: view}}, flats, loss [1]) -- the flats are what allreduce_grads
    averages across ranks; loss is the local batch's term, one copy (the reference adds it under "main" and
    "cache_main")."""
    mult = cfg.loss_weight * cfg.data_loss_mult
    flats, loss = rc.data_backward(rays, rgb, jitters, anneal_at(train_frac, anneal_cfg), lossmult, cfg.charb_padding,
                                   mult, flats)
    last = rc.cfg.num_levels - 1
    grads = {f"MLP_{last}": grads_as_dict(flats[0], rc.density_grad_layout(last)[0]),
             "Shader": grads_as_dict(flats[1], rc.shader_grad_layout()[0])}
    return grads, list(flats), loss


def normal_weight_ease(train_frac: float, cfg: GeometryLossConfig = GeometryLossConfig()) -> float:
    """weight_ease_in (train_utils.compute_weight_ease_in) with the normal-weight settings."""
    return weight_ease_in(train_frac, cfg.use_normal_weight_ease, cfg.normal_weight_ease_start, cfg.normal_weight_ease_frac,
                          cfg.normal_weight_ease_min)


def geometry_terms(train_frac: float, cfg: GeometryLossConfig = GeometryLossConfig(), scale: float = 1.0):
    """The rc_geometry_loss fields of one copy of the terms at train_frac (train_utils.py:3256-3300): the
    predicted-normal term times the ease, the reverse term times the ease when use_normal_weight_ease_backward; the
    weight decay is off.  scale multiplies every mult."""
    ease = normal_weight_ease(train_frac, cfg)
    return dict(distortion_mult=cfg.distortion_mult * scale, distortion_p=cfg.distortion_p,
                distortion_premult=cfg.distortion_premult, orientation_mult=cfg.orientation_mult * scale,
                pred_normal_mult=cfg.pred_normal_mult * ease * scale, pred_normal_w_grad_weight=cfg.pred_normal_w_grad_weight,
                pred_normal_reverse_mult=cfg.pred_normal_reverse_mult * (ease if cfg.use_normal_weight_ease_backward else 1.0)
                * scale)


GEOMETRY_KEYS = ("distortion", "orientation", "predicted_normals", "predicted_normals_reverse")


def geometry_grads(rc, rays, jitters, train_frac: float, lossmult=None, flats=None,
                   cfg: GeometryLossConfig = GeometryLossConfig(), anneal_cfg: InterlevelConfig = InterlevelConfig(),
                   scale: float = 1.0):
    """The geometry losses of a batch and their gradients (rc_geometry_backward).  jitters / train_frac / lossmult /
    flats as data_grads; scale multiplies every term (cache_stage_grads passes 2: "main" and "cache_main").
    -> ({"MLP_2": {name: view}, "Shader": {name: view}}, flats, losses [4] in GEOMETRY_KEYS order)."""
    flats, losses = rc.geometry_backward(rays, jitters, anneal_at(train_frac, anneal_cfg), lossmult,
                                         geometry_terms(train_frac, cfg, scale), flats)
    last = rc.cfg.num_levels - 1
    grads = {f"MLP_{last}": grads_as_dict(flats[0], rc.density_grad_layout(last)[0]),
             "Shader": grads_as_dict(flats[1], rc.shader_grad_layout()[0])}
    return grads, list(flats), losses


def weight_ease_in(train_frac: float, use: bool, start: float, frac: float, min_value: float = 0.0) -> float:
    """train_utils.compute_weight_ease_in (internal/train_utils.py:839-867): 1 when the schedule is off;
    min (1 - w) + w, w = clip((train_frac - start) / frac, 0, 1), for frac > 0; else the step float(train_frac >= start)."""
    if not use:
        return 1.0
    if frac > 0:
        w = min(max((float(train_frac) - start) / frac, 0.0), 1.0)
        return min_value * (1.0 - w) + w
    return float(float(train_frac) >= start)


def weight_decay(train_frac: float, use: bool, start: float, frac: float, min_value: float = 0.0) -> float:
    """train_utils.compute_weight_decay (internal/train_utils.py:870-894): 1 when the schedule is off; else
    min w + (1 - w), w = clip((train_frac - start) / frac, 0, 1) (frac = 0 divides by zero there as well)."""
    if not use:
        return 1.0
    w = min(max((float(train_frac) - start) / frac, 0.0), 1.0)
    return min_value * w + (1.0 - w)


def mask_terms(train_frac: float, cfg: MaskLossConfig = MaskLossConfig(), scale: float = 1.0):
    """The rc_mask_loss fields of one copy of the two mask terms at train_frac: {"mask": ..., "mask_backwards": ...}.
    _compute_mask_weight_decay and _compute_mask_weight_ease (train_utils.py:897-932) multiply the Charbonnier value
    before the weights do (:815-832), so they are folded into the weights; the backward term is the empty_loss_weight=
    branch (:821-826): (0, backward_mask_loss_weight) on zero masks.  scale multiplies every weight."""
    sched = (weight_decay(train_frac, cfg.use_mask_weight_decay, cfg.mask_weight_decay_start, cfg.mask_weight_decay_frac,
                          cfg.mask_weight_decay_min)
             * weight_ease_in(train_frac, cfg.use_mask_weight_ease, cfg.mask_weight_ease_start, cfg.mask_weight_ease_frac,
                              cfg.mask_weight_ease_min)) * scale
    return {"mask": dict(charb_padding=cfg.charb_padding, weight_opaque=cfg.opaque_loss_weight * sched,
                         weight_empty=cfg.empty_loss_weight * sched, zero_masks=0),
            "mask_backwards": dict(charb_padding=cfg.charb_padding, weight_opaque=0.0,
                                   weight_empty=cfg.backward_mask_loss_weight * sched, zero_masks=1)}


MASK_KEYS = ("mask", "mask_backwards")


def mask_grads(rc, rays, jitters, train_frac: float, masks=None, lossmult=None, flat=None, look=None, backward_randoms=None,
               cfg: MaskLossConfig = MaskLossConfig(), anneal_cfg: InterlevelConfig = InterlevelConfig(), scale: float = 1.0):
    """The mask loss of a batch, its backward term and their gradients (rc_mask_backward, rc_backward_mask_rays).
    jitters / train_frac / lossmult as data_grads; masks: [n] or None (ones); flat: the last level's density flat to
    accumulate into (allocated zeroed when None).  The backward term runs when cfg.backward_mask_loss is set and both
    look ([n, 3] camera look vectors) and backward_randoms ({"u1", "u2": [n], "jitter": per-level [n]} of the backward
    rays, prng.backward_mask_randoms) are given: its rays start shadow_near_max in front of the camera, carry the batch
    rays' lossmult and zero masks.  scale multiplies both terms (cache_stage_grads passes 2).
    -> ({"MLP_<last>": {name: view}}, flat, {"mask": 0-d tensor, "mask_backwards": 0-d tensor}); a term that did not
    run is left out of the dict."""
    terms = mask_terms(train_frac, cfg, scale)
    anneal = anneal_at(train_frac, anneal_cfg)
    flat, loss = rc.mask_backward(rays, jitters, anneal, masks, lossmult, terms["mask"], flat)
    losses = {"mask": loss[0]}
    if cfg.backward_mask_loss and look is not None and backward_randoms is not None:
        back = rc.backward_mask_rays(rays["origins"], look, backward_randoms["u1"], backward_randoms["u2"],
                                     cfg.shadow_near_max, cfg.secondary_normal_eps, cfg.secondary_far)
        flat, loss = rc.mask_backward(back, backward_randoms.get("jitter"), anneal, None, lossmult, terms["mask_backwards"], flat)
        losses["mask_backwards"] = loss[0]
    last = rc.cfg.num_levels - 1
    return {f"MLP_{last}": grads_as_dict(flat, rc.density_grad_layout(last)[0])}, flat, losses


def geometry_smoothness_terms(train_frac: float, cfg: GeometrySmoothnessConfig = GeometrySmoothnessConfig(), scale: float = 1.0):
    """The rc_geometry_smoothness fields of the term at train_frac: the three weights times the extra loss's mult (0
    before cfg.start_frac of training, as material_smoothness_grads gates its term) and scale; the noise magnitude as it is."""
    mult = (cfg.mult if train_frac >= cfg.start_frac else 0.0) * scale
    return dict(noise=cfg.noise, weight_normals=cfg.weight_normals * mult, weight_normals_pred=cfg.weight_normals_pred * mult,
                weight_density=cfg.weight_density * mult)


def geometry_smoothness_grads(rc, rays, jitters, noise, train_frac: float, lossmult=None, flat=None,
                              cfg: GeometrySmoothnessConfig = GeometrySmoothnessConfig(),
                              anneal_cfg: InterlevelConfig = InterlevelConfig(), scale: float = 1.0):
    """The geometry smoothness loss of a batch and its gradient through the analytic normals (and the density, when its
    weight is set) of the last level (rc_geometry_smoothness_backward).  jitters / train_frac / lossmult as
    data_grads; noise: [n, S, 3] N(0, 1) (prng.geometry_smoothness_noise); flat: the last level's density flat to
    accumulate into (allocated zeroed when None).
    -> ({"MLP_<last>": {name: view}}, flat, loss [1])."""
    flat, loss = rc.geometry_smoothness_backward(rays, jitters, anneal_at(train_frac, anneal_cfg), noise, lossmult,
                                                 geometry_smoothness_terms(train_frac, cfg, scale), flat)
    last = rc.cfg.num_levels - 1
    return {f"MLP_{last}": grads_as_dict(flat, rc.density_grad_layout(last)[0])}, flat, loss


def cache_stage_grads(rc, rays, rgb, jitters, train_frac: float, lossmult=None, flats=None,
                      geometry_cfg: GeometryLossConfig = GeometryLossConfig(), data_cfg: DataLossConfig = DataLossConfig(),
                      interlevel_cfg: InterlevelConfig = InterlevelConfig(), mask_cfg: Optional[MaskLossConfig] = None,
                      masks=None, look=None, backward_randoms=None,
                      smoothness_cfg: Optional[GeometrySmoothnessConfig] = None, smoothness_noise=None):
    """The hotdog cache stage's loss on a batch and its gradients (train_utils.py:3000-3098).  The interlevel,
    data and geometry terms are computed for "main" and "cache_main" on the same model results, so each counts twice
    (the device calls run once with their mults doubled; the dict reports each copy); the density-grid regularizer
    (param_regularizer_loss) counts once, over the three proposal grids.
    flats: {level: density flat, "shader": shader flat} to accumulate into (allocated zeroed when None).
    -> (flats, losses): losses maps the reference's losses_flat keys (interlevel_<l>, distortion, orientation,
    predicted_normals, predicted_normals_reverse, data, their cache_main_* copies, regularizer/density_grid) to
    0-d cuda tensors.
    mask_cfg (None: the mask terms are left out and the result is what it was without them): the mask loss on `masks`
    ([n] or None: ones) and, with look and backward_randoms (mask_grads), its backward term, added to flats[last] and to
    the dict as mask, mask_backwards and their cache_main_* copies.  per_output_loss_fn computes both whenever not
    config.is_material (train_utils.py:2919-2945), and the cache stage's loop over the output keys (:2998-3024:
    model.use_material is False) leaves is_material False for "main" and for "cache_main"; "mask" is in the exclude_list
    (:3058-3060), so neither copy is scaled by loss_weight.  They therefore count twice like the other terms: the device
    calls run once with doubled weights.  For the backward term that is a reading, not an identity: the reference draws
    the backward rays of each output key from that key's own rng (:3036), so its two copies are two samples of the same
    expectation, where this function counts one sample twice.
    smoothness_cfg with smoothness_noise (None: left out, the result is what it is without them): the geometry_smoothness
    extra loss (geometry_smoothness_grads), added to flats[last] and to the dict as geometry_smoothness.  It counts ONCE: the
    trainer registers it under "main" only (engine/trainer.py:318-320), and it is in the exclude_list (:3058-3060), so it
    is not scaled by loss_weight.
    What the sum of the dict is: with the mask terms, the reference's stats["loss"] (:3098) except for
    regularizer/light_grid and regularizer/material_grid (param_regularizer_loss starts its dict with every prefix of
    Config.param_regularizers, :1183; they regularize parameters outside the cache stage's layouts and are not computed
    here) and up to that one-sample reading; without mask_cfg it also lacks the four mask keys.  The predicted-normal
    terms follow the first-order reading of the module docstring."""
    nl = rc.cfg.num_levels
    flats = dict(flats or {})
    il_cfg = dataclasses.replace(interlevel_cfg, mults=tuple(2.0 * m for m in interlevel_cfg.mults))
    _, il_flats, il_losses = interlevel_grads(rc, rays, jitters, train_frac, lossmult,
                                              [flats.get(l) for l in range(nl - 1)], il_cfg)
    for l in range(nl - 1):
        flats[l] = il_flats[l]
    d_cfg = dataclasses.replace(data_cfg, data_loss_mult=2.0 * data_cfg.data_loss_mult)
    _, d_flats, d_loss = data_grads(rc, rays, rgb, jitters, train_frac, lossmult, (flats.get(nl - 1), flats.get("shader")),
                                    d_cfg, interlevel_cfg)
    flats[nl - 1], flats["shader"] = d_flats
    _, g_flats, g_losses = geometry_grads(rc, rays, jitters, train_frac, lossmult, (flats[nl - 1], flats["shader"]),
                                          geometry_cfg, interlevel_cfg, scale=2.0)
    flats[nl - 1], flats["shader"] = g_flats
    reg = None
    for l in range(nl):
        flats[l], r = rc.density_regularizer(l, geometry_cfg.density_grid_mult, flats[l])
        reg = r if reg is None else reg + r
    main = {}
    for l in range(nl - 1):
        main[f"interlevel_{l}"] = il_losses[l] / 2
    for k, key in enumerate(GEOMETRY_KEYS):
        main[key] = g_losses[k] / 2
    main["data"] = d_loss[0] / 2
    losses = dict(main)
    losses.update({f"cache_main_{k}": v for k, v in main.items()})
    losses["regularizer/density_grid"] = reg[0]
    if mask_cfg is not None:
        _, flats[nl - 1], m_losses = mask_grads(rc, rays, jitters, train_frac, masks, lossmult, flats[nl - 1], look,
                                                backward_randoms, mask_cfg, interlevel_cfg, scale=2.0)
        for k in MASK_KEYS:
            if k in m_losses:
                losses[k] = losses[f"cache_main_{k}"] = m_losses[k] / 2
    if smoothness_cfg is not None:
        if smoothness_noise is None:
            raise ValueError("smoothness_cfg needs smoothness_noise (prng.geometry_smoothness_noise)")
        _, flats[nl - 1], s_loss = geometry_smoothness_grads(rc, rays, jitters, smoothness_noise, train_frac, lossmult,
                                                             flats[nl - 1], smoothness_cfg, interlevel_cfg)
        losses["geometry_smoothness"] = s_loss[0]
    return flats, losses


# ---- the optimizer ---------------------------------------------------------------------------------------------------

def learning_rate_decay(step, lr_init: float, lr_final: float, max_steps: int, lr_delay_steps: int = 0,
                        lr_delay_mult: float = 1.0) -> np.float32:
    """math.learning_rate_decay (internal/math.py:356-409) as jax evaluates it on optax's int32 count, in float32:
    delay_rate * log_lerp(step / max_steps, lr_init, lr_final), log_lerp(t, a, b) = exp(clip(t, 0, 1) (log b - log a)
    + log a), delay_rate = mult + (1 - mult) sin(pi/2 clip(step / delay_steps, 0, 1)) when delay_steps > 0, else 1."""
    f = np.float32
    if lr_init == 0.0 and lr_final == 0.0:
        return f(0.0)
    if lr_init <= 0 or lr_final <= 0:
        raise ValueError(f"Interpolants {lr_init} and {lr_final} must be positive.")
    if lr_delay_steps > 0:
        x = np.clip(f(step) / f(lr_delay_steps), f(0), f(1))
        delay_rate = f(lr_delay_mult) + f(1 - lr_delay_mult) * np.sin(f(0.5 * np.pi) * x)
    else:
        delay_rate = f(1.0)
    lv0, lv1 = np.log(f(lr_init)), np.log(f(lr_final))
    t = np.clip(f(step) / f(max_steps), f(0), f(1))
    return f(delay_rate * np.exp(t * (lv1 - lv0) + lv0))


def train_frac_at(step: int, max_steps: int) -> float:
    """clip(step / (max_steps - 1), 0, 1) (engine/trainer.py:2116-2126): what the anneal and the normal-loss ease read."""
    return float(min(max(step / (max_steps - 1), 0.0), 1.0))


def param_group(name: str, cfg: OptimizerConfig = OptimizerConfig()) -> str:
    """The Adam that updates tensor `name` ("params/Cache/..." or "Cache/..."): create_optimizer folds each
    extra_opt_params prefix in as chain(masked(tx_prev, prefix not in path), masked(adam_prefix, prefix in path)) with
    path.split("/") matched element by element, and optax.masked passes masked-out updates through, so the LAST listed
    prefix on the path wins; "main" when none is on it."""
    parts = name.split("/")
    if parts and parts[0] == "params":
        parts = parts[1:]
    group = "main"
    for e in cfg.extra_opt_params:
        if e.prefix in parts:
            group = e.prefix
    return group


def adam_scalars(count: int, cfg: OptimizerConfig = OptimizerConfig(), zero_grads: bool = True):
    """The rc_adam_step of the step at optax count `count` (before the update), per group of cfg.groups(): lr(count),
    the decays, 1 - b rounded from the double (optax's (1 - decay) * g on a float32 array), eps, and the bias
    corrections 1 - b^(count+1) in float32; the clip thresholds."""
    f = np.float32
    out = {k: [] for k in ("lr", "b1", "b2", "one_minus_b1", "one_minus_b2", "eps", "bias_correction1",
                           "bias_correction2")}
    for _, sched in cfg.groups():
        out["lr"].append(learning_rate_decay(count, **sched))
        out["b1"].append(f(cfg.b1))
        out["b2"].append(f(cfg.b2))
        out["one_minus_b1"].append(f(1.0 - cfg.b1))
        out["one_minus_b2"].append(f(1.0 - cfg.b2))
        out["eps"].append(f(cfg.eps))
        out["bias_correction1"].append(f(1) - np.power(f(cfg.b1), f(count + 1)))
        out["bias_correction2"].append(f(1) - np.power(f(cfg.b2), f(count + 1)))
    out.update(grad_max_val=cfg.grad_max_val, grad_max_norm=cfg.grad_max_norm, zero_grads=zero_grads)
    return out


class CacheStageOptimizer:
    """The cache stage's optimizer state on the device: flat params, mu, nu and gradient buffers in the layouts
    rc.density_grad_layout(l) (l = 0 .. num_levels-1) and rc.shader_grad_layout() ("shader"), and the optax count.
    step() = one rc_adam_update over the four buffers (nan_to_num, clip_gradients, the chained Adams), then
    rc_load_params_flat per layout: the handle renders the updated parameters, ordered on the current stream.
    `keys` (the subclasses'): other gradient layouts of the handle ("light", "material") instead of the cache stage's."""

    def __init__(self, rc, cfg: OptimizerConfig = OptimizerConfig(), keys=None):
        import torch
        from . import rc_ext

        self.rc, self.cfg, self._rc_ext = rc, cfg, rc_ext
        self.keys = list(range(rc.cfg.num_levels)) + ["shader"] if keys is None else list(keys)
        self.layouts = {k: rc._grad_layout(k) for k in self.keys}
        self.group_names = [g for g, _ in cfg.groups()]
        dev = f"cuda:{rc.device}"
        z = lambda k: torch.zeros(self.layouts[k][1], dtype=torch.float32, device=dev)
        self.params = {k: z(k) for k in self.keys}
        self.mu = {k: z(k) for k in self.keys}
        self.nu = {k: z(k) for k in self.keys}
        self.grads = {k: z(k) for k in self.keys}
        self.segments = {k: [(off, int(np.prod(shape)), self.group_names.index(param_group(name, cfg)))
                             for name, off, shape in self.layouts[k][0]] for k in self.keys}
        self._table = self._adam_table(self.grads)
        self.count = 0

    def _adam_table(self, grads):
        return self._rc_ext.AdamTable([(self.params[k], grads[k], self.mu[k], self.nu[k], self.segments[k])
                                       for k in self.keys])

    def names(self):
        return [name for k in self.keys for name, _, _ in self.layouts[k][0]]

    def init_from(self, weights: Dict[str, object], count: int = 0):
        """Parameters from a {"params/...": array} dict (weights.py, checkpoint.load_params); zero moments and
        gradients; the optax count; the handle refreshed."""
        import torch
        for k in self.keys:
            for name, off, shape in self.layouts[k][0]:
                if name not in weights:
                    raise KeyError(f"init_from: {name} missing")
                w = weights[name]
                t = w if isinstance(w, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32))
                if tuple(t.shape) != tuple(shape):
                    raise ValueError(f"init_from: {name} has shape {tuple(t.shape)}, expected {shape}")
                self.params[k][off: off + int(np.prod(shape))].copy_(t.reshape(-1))
            self.mu[k].zero_()
            self.nu[k].zero_()
            self.grads[k].zero_()
        self.count = int(count)
        self.refresh()

    def refresh(self):
        """rc_load_params_flat of every layout (ordered on the current stream)."""
        for k in self.keys:
            self.rc.load_params_flat(k, self.params[k])

    def step(self, flats=None, zero_grads: bool = True):
        """One update from the gradients `flats` ({key: flat buffer}; None = the optimizer's own gradient buffers,
        which cache_stage_step fills), then the refresh; `zero_grads` leaves the gradient buffers zeroed."""
        table = self._table if flats is None or all(flats[k] is self.grads[k] for k in self.keys) else \
            self._adam_table({k: flats[k] for k in self.keys})
        self.rc.adam_update(table, adam_scalars(self.count, self.cfg, zero_grads))
        self.count += 1
        self.refresh()

    def params_dict(self) -> Dict[str, object]:
        """{"params/...": view of the flat parameters}: what checkpoint.save_params and load_weights accept."""
        return {name: v for k in self.keys for name, v in grads_as_dict(self.params[k], self.layouts[k][0]).items()}

    def state_dict(self):
        """params, mu, nu (copies of the flat buffers by layout key) and the count: training stops and resumes on it."""
        c = lambda d: {str(k): v.detach().clone() for k, v in d.items()}
        return {"count": int(self.count), "params": c(self.params), "mu": c(self.mu), "nu": c(self.nu)}

    def load_state_dict(self, sd):
        for k in self.keys:
            self.params[k].copy_(sd["params"][str(k)])
            self.mu[k].copy_(sd["mu"][str(k)])
            self.nu[k].copy_(sd["nu"][str(k)])
            self.grads[k].zero_()
        self.count = int(sd["count"])
        self.refresh()


def _train_step(opt: CacheStageOptimizer, group, grads):
    """The body of the *_step functions: train_frac from opt.count, grads(train_frac) -> ({key: flat buffer}, or the one
    flat buffer of a single-layout optimizer; losses), the pmean over `group` (allreduce_grads), opt.step().  -> losses."""
    tf = train_frac_at(opt.count, opt.cfg.scaled_steps(opt.cfg.max_steps))
    flats, losses = grads(tf)
    if not isinstance(flats, dict):
        flats = {opt.keys[0]: flats}
    allreduce_grads([flats[k] for k in opt.keys], group=group)
    opt.step({k: flats[k] for k in opt.keys})
    return losses


def cache_stage_step(rc, opt: CacheStageOptimizer, rays, rgb, jitters, lossmult=None, group=None,
                     geometry_cfg: GeometryLossConfig = GeometryLossConfig(), data_cfg: DataLossConfig = DataLossConfig(),
                     interlevel_cfg: InterlevelConfig = InterlevelConfig(), mask_cfg: Optional[MaskLossConfig] = None,
                     masks=None, look=None, backward_randoms=None):
    """One train step of the cache stage (train_utils.py:3128-3161): train_frac from opt.count
    (trainer.py:2116-2126), cache_stage_grads into the optimizer's zeroed gradient buffers, the pmean over `group`
    when torch.distributed runs (allreduce_grads), then opt.step() (nan_to_num, clip_gradients, the Adams, the handle's
    refresh).  mask_cfg / masks / look / backward_randoms: the mask terms, as cache_stage_grads takes them.
    -> the losses dict of cache_stage_grads (the local batch's values)."""
    return _train_step(opt, group, lambda tf: cache_stage_grads(rc, rays, rgb, jitters, tf, lossmult, dict(opt.grads),
                                                                geometry_cfg, data_cfg, interlevel_cfg, mask_cfg, masks,
                                                                look, backward_randoms))


def cache_stage_fit(rc, opt: CacheStageOptimizer, dataset, key, steps: int, group=None,
                    geometry_cfg: GeometryLossConfig = GeometryLossConfig(), data_cfg: DataLossConfig = DataLossConfig(),
                    interlevel_cfg: InterlevelConfig = InterlevelConfig(), mask_cfg: Optional[MaskLossConfig] = None,
                    masks_of=None):
    """`steps` train steps of the cache stage fed by a data.DeviceDataset, from one PRNG key.  Per step: key, rng =
    random_split(rng); dataset.next_train (one launch: cameras, pixels, rays, colours); one more split per proposal level
    for its per-ray jitter, drawn in HBM (rc.prng_fill); cache_stage_step.  With mask_cfg the mask terms run as well:
    the batch's masks are the caller's (masks_of(batch) -> [n] cuda tensor or None for ones; the batch kernel does not
    write masks), the backward rays start from the batch's look vectors, and their uniform pair and per-level jitter
    are drawn in HBM from further splits of the step's jitter key.  The host handles keys and scalars only: no tensor
    crosses PCIe inside the loop and nothing is read back.  -> the steps' loss dicts (0-d cuda tensors)."""
    rng = prng.as_key(key)
    n = dataset.batch_size
    history = []
    for _ in range(int(steps)):
        step_key, rng = prng.random_split(rng)
        batch_key, jitter_key = prng.random_split(step_key)
        batch = dataset.next_train(batch_key)
        jitters = []
        for _ in range(rc.cfg.num_levels):
            k, jitter_key = prng.random_split(jitter_key)
            jitters.append(rc.prng_fill(k, (n, 1), "uniform"))
        masks = look = back = None
        if mask_cfg is not None:
            masks = masks_of(batch) if masks_of is not None else None
            if mask_cfg.backward_mask_loss:
                look = batch.rays.look
                k, jitter_key = prng.random_split(jitter_key)
                u = rc.prng_fill(k, (n, 2), "uniform")
                back = {"u1": u[:, 0].contiguous(), "u2": u[:, 1].contiguous(), "jitter": []}
                for _ in range(rc.cfg.num_levels):
                    k, jitter_key = prng.random_split(jitter_key)
                    back["jitter"].append(rc.prng_fill(k, (n, 1), "uniform"))
        history.append(cache_stage_step(rc, opt, batch.rays.hot_fields(), batch.rgb, jitters, batch.rays.lossmult, group,
                                        geometry_cfg, data_cfg, interlevel_cfg, mask_cfg, masks, look, back))
    return history


# ---- the light sampler ---------------------------------------------------------------------------------------------

def light_sampling_grads(rc, rays, randoms, train_frac: float, lossmult=None, flat=None,
                         cfg: LightSamplingConfig = LightSamplingConfig()):
    """The light sampler's own loss on a batch and its gradient: the light_sampling extra loss
    (train_utils.py:1985-2067, active from cfg.start_frac of training) and param_regularizer_loss for 'light_grid', both
    accumulated into `flat` (layout rc.light_grad_layout(); allocated zeroed when None).  randoms: render_material's.
    -> (flat, losses) with losses keyed like the reference's losses_flat ("light_sampling", "regularizer/light_grid"),
    0-d cuda tensors (the local batch's values)."""
    mult = cfg.mult if train_frac >= cfg.start_frac else 0.0
    flat, loss = rc.light_sampling_backward(rays, randoms, cfg.num_secondary_samples, lossmult, mult, cfg.linear_to_srgb,
                                            flat)
    flat, reg = rc.light_regularizer(cfg.light_grid_mult, flat)
    return flat, {"light_sampling": loss[0], "regularizer/light_grid": reg[0]}


class LightSamplerOptimizer(CacheStageOptimizer):
    """The LightSampler's optimizer state on the device: flat params, mu, nu and gradients in the layout
    rc.light_grad_layout() (key "light") and the optax count.  Every tensor is in param_group "LightSampler"; clip_gradients
    takes its norm per top-level module, so a step is ONE rc_adam_update over this buffer, then rc_load_params_flat
    (RC_LAYOUT_LIGHT).  init_from / params_dict / state_dict / load_state_dict as CacheStageOptimizer."""

    def __init__(self, rc, cfg: OptimizerConfig = OptimizerConfig()):
        super().__init__(rc, cfg, ["light"])


def light_sampler_step(rc, opt: LightSamplerOptimizer, rays, randoms, lossmult=None, group=None,
                       cfg: LightSamplingConfig = LightSamplingConfig()):
    """One train step of the light sampler on its own loss: train_frac from opt.count, light_sampling_grads into the
    optimizer's zeroed gradient buffer, the pmean over `group` when torch.distributed runs, then opt.step().
    -> the losses dict of light_sampling_grads."""
    return _train_step(opt, group, lambda tf: light_sampling_grads(rc, rays, randoms, tf, lossmult, opt.grads["light"], cfg))


# ---- the material network ------------------------------------------------------------------------------------------

def material_ray_sampler_loss(cfg: MaterialSmoothnessConfig = MaterialSmoothnessConfig(), interlevel=0.0, distortion=0.0,
                              orientation=0.0, normal=0.0) -> float:
    """train_utils.material_ray_sampler_loss (internal/train_utils.py:2273-2351) times its "main" mult, given the values
    of its four terms on the reference rays: interlevel * interlevel_mult + distortion * normal_mult * distortion_mult
    + orientation * orientation_mult + (predicted normal + reverse) * normal_mult.  Every term mult is 0 for hotdog
    (nerf_ngp_yobo.gin:52-53, configs.py:531-534), so the loss is identically 0 and no backward is needed."""
    total = (interlevel * cfg.ray_sampler_interlevel_mult
             + distortion * cfg.ray_sampler_normal_mult * cfg.ray_sampler_distortion_mult
             + orientation * cfg.ray_sampler_orientation_mult + normal * cfg.ray_sampler_normal_mult)
    return cfg.ray_sampler_mult * total


def material_smoothness_grads(rc, rays, randoms, noise, train_frac: float, lossmult=None, flat=None,
                              cfg: MaterialSmoothnessConfig = MaterialSmoothnessConfig()):
    """The material network's own losses on a batch and their gradient: the material_smoothness extra
    loss (train_utils.py:2505-2700, active from cfg.start_frac of training) and param_regularizer_loss for
    'material_grid', both accumulated into `flat` (layout rc.material_grad_layout(); allocated zeroed when None), and
    material_ray_sampler (0: no gradient).  randoms: render_material's (jitter, gumbel or resample_inds are read); noise:
    [n, 3] N(0, 1) (prng.material_smoothness_noise).  -> (flat, losses) with losses keyed like the reference's
    losses_flat ("material_smoothness", "regularizer/material_grid", "material_ray_sampler"), 0-d cuda tensors (the local
    batch's values)."""
    import torch

    if not (cfg.l1_loss and not cfg.irradiance_weight and not cfg.albedo_stopgrad):
        raise NotImplementedError("material_smoothness: only the l1 form without irradiance weight or albedo stopgrad")
    mult = cfg.mult if train_frac >= cfg.start_frac else 0.0
    flat, loss = rc.material_smoothness_backward(rays, randoms, noise, lossmult, mult, cfg.weight_albedo, cfg.weight_other,
                                                 cfg.noise, cfg.tensoir_albedo, flat)
    flat, reg = rc.material_regularizer(cfg.material_grid_mult * cfg.material_grid_ease, flat)
    zero = torch.zeros((), dtype=torch.float32, device=loss.device) + material_ray_sampler_loss(cfg)
    return flat, {"material_smoothness": loss[0], "regularizer/material_grid": reg[0], "material_ray_sampler": zero}


class MaterialOptimizer(CacheStageOptimizer):
    """The MaterialShader's optimizer state on the device: flat params, mu, nu and gradients in the layout
    rc.material_grad_layout() (key "material") and the optax count.  Every tensor is in param_group "MaterialShader";
    clip_gradients takes its norm per top-level module, so a step is ONE rc_adam_update over this buffer, then
    rc_load_params_flat (RC_LAYOUT_MATERIAL).  init_from / params_dict / state_dict / load_state_dict as
    CacheStageOptimizer."""

    def __init__(self, rc, cfg: OptimizerConfig = OptimizerConfig()):
        super().__init__(rc, cfg, ["material"])


def material_step(rc, opt: MaterialOptimizer, rays, randoms, noise, lossmult=None, group=None,
                  cfg: MaterialSmoothnessConfig = MaterialSmoothnessConfig()):
    """One train step of the material network on its own losses: train_frac from opt.count, material_smoothness_grads
    into the optimizer's zeroed gradient buffer, the pmean over `group` when torch.distributed runs, then opt.step().
    -> the losses dict of material_smoothness_grads."""
    return _train_step(opt, group, lambda tf: material_smoothness_grads(rc, rays, randoms, noise, tf, lossmult,
                                                                        opt.grads["material"], cfg))


def material_data_grads(rc, rays, randoms, gt_rgb, lossmult=None, flat=None,
                        cfg: MaterialDataLossConfig = MaterialDataLossConfig(), env_flat=None):
    """The material stage's data loss on a batch and its MaterialShader gradient: compute_data_loss of
    the MaterialIntegrator's rgb against gt_rgb ([n, 3]) times loss_weight, material_loss_weight_ease and data_loss_mult,
    accumulated into `flat` (layout rc.material_grad_layout(); allocated zeroed when None).  The gradient is the
    Trainer.stopgrad = True reading (path (a)); the Cache, EnvMap and LightSampler get none from this call.  randoms:
    render_material's.  -> (flat, {"data": 0-d cuda tensor}), the key of the reference's losses_flat.
    env_flat: True, or a flat buffer of rc.envmap_grad_layout() to accumulate into, adds the EnvMap's
    gradient of the same loss times cfg.env_map_grad_weight: -> (flat, env_flat, losses)."""
    if cfg.loss_type != "rawnerf_transient_unbiased" or cfg.use_loss_clip:
        raise NotImplementedError("material data loss: only the rawnerf unbiased form without loss clip")
    if env_flat is None:
        flat, loss = rc.material_data_backward(rays, randoms, gt_rgb, cfg.num_secondary_samples, lossmult, cfg, flat)
        return flat, {"data": loss[0]}
    flat, env_flat, loss = rc.material_data_backward(rays, randoms, gt_rgb, cfg.num_secondary_samples, lossmult, cfg, flat,
                                                     env_grad=env_flat, env_scale=cfg.env_map_grad_weight)
    return flat, env_flat, {"data": loss[0]}


def material_stage_grads(rc, rays, randoms, gt_rgb, noise, train_frac: float, lossmult=None, flat=None,
                         data_cfg: MaterialDataLossConfig = MaterialDataLossConfig(),
                         smooth_cfg: MaterialSmoothnessConfig = MaterialSmoothnessConfig()):
    """Every loss of the material stage that reaches params/MaterialShader, accumulated into one flat buffer: the data
    loss (material_data_grads) and material_smoothness_grads (material_smoothness, regularizer/material_grid,
    material_ray_sampler).  -> (flat, losses) keyed like losses_flat."""
    flat, losses = material_data_grads(rc, rays, randoms, gt_rgb, lossmult, flat, data_cfg)
    flat, more = material_smoothness_grads(rc, rays, randoms, noise, train_frac, lossmult, flat, smooth_cfg)
    losses.update(more)
    return flat, losses


def material_stage_step(rc, opt: MaterialOptimizer, rays, randoms, gt_rgb, noise, lossmult=None, group=None,
                        data_cfg: MaterialDataLossConfig = MaterialDataLossConfig(),
                        smooth_cfg: MaterialSmoothnessConfig = MaterialSmoothnessConfig()):
    """One train step of the material network on the stage's losses: train_frac from opt.count, material_stage_grads into
    the optimizer's zeroed gradient buffer, the pmean over `group` when torch.distributed runs, then opt.step().
    -> the losses dict of material_stage_grads."""
    return _train_step(opt, group, lambda tf: material_stage_grads(rc, rays, randoms, gt_rgb, noise, tf, lossmult,
                                                                   opt.grads["material"], data_cfg, smooth_cfg))


# ---- the EnvMap ----------------------------------------------------------------------------------------------------

class EnvMapOptimizer(CacheStageOptimizer):
    """The model-level EnvMap's optimizer state on the device: flat params, mu, nu and gradients in the layout
    rc.envmap_grad_layout() (key "envmap") and the optax count.  Every tensor is in param_group "EnvMap" (the last listed
    prefix on "Cache/EnvMap/..." wins over none: "Cache" is no group).  clip_gradients takes its norm per top-level module
    and Cache/EnvMap sits under Cache, whose other tensors this optimizer does not hold: with grad_max_norm > 0 that norm
    cannot be formed here, so it is refused (hotdog has both clips off).  A step is ONE rc_adam_update over this buffer,
    then rc_load_params_flat (RC_LAYOUT_ENVMAP).  init_from / params_dict / state_dict / load_state_dict as
    CacheStageOptimizer."""

    def __init__(self, rc, cfg: OptimizerConfig = OptimizerConfig()):
        if cfg.grad_max_norm > 0:
            raise NotImplementedError("EnvMapOptimizer: grad_max_norm needs the norm over all of params/Cache")
        super().__init__(rc, cfg, ["envmap"])


def material_env_stage_step(rc, opt_material: MaterialOptimizer, opt_envmap: EnvMapOptimizer, rays, randoms, gt_rgb, noise,
                            lossmult=None, group=None, data_cfg: MaterialDataLossConfig = MaterialDataLossConfig(),
                            smooth_cfg: MaterialSmoothnessConfig = MaterialSmoothnessConfig(), step_material: bool = True,
                            step_envmap: bool = True):
    """One train step of the material stage on the MaterialShader and the EnvMap: one forward, the data
    loss into both optimizers' zeroed gradient buffers (rc_material_data_backward_env), material_smoothness_grads into the
    material buffer, ONE pmean over both (allreduce_grads), then both optimizer steps.  train_frac is read from
    opt_material.count; the two counts advance together.  step_material / step_envmap = False leaves that optimizer's
    parameters, moments and count alone (its gradient buffer is zeroed).  -> the losses dict of material_stage_grads."""
    tf = train_frac_at(opt_material.count, opt_material.cfg.scaled_steps(opt_material.cfg.max_steps))
    gm, ge = opt_material.grads["material"], opt_envmap.grads["envmap"]
    _, _, losses = material_data_grads(rc, rays, randoms, gt_rgb, lossmult, gm, data_cfg, env_flat=ge)
    _, more = material_smoothness_grads(rc, rays, randoms, noise, tf, lossmult, gm, smooth_cfg)
    losses.update(more)
    allreduce_grads([gm, ge], group=group)
    for opt, on, g in ((opt_material, step_material, gm), (opt_envmap, step_envmap, ge)):
        if on:
            opt.step()
        else:
            g.zero_()
    return losses


def material_stage_fit(rc, opt_material: MaterialOptimizer, opt_envmap: EnvMapOptimizer, dataset, key, steps: int,
                       opt_light: Optional[LightSamplerOptimizer] = None, group=None,
                       data_cfg: MaterialDataLossConfig = MaterialDataLossConfig(),
                       smooth_cfg: MaterialSmoothnessConfig = MaterialSmoothnessConfig(),
                       light_cfg: LightSamplingConfig = LightSamplingConfig()):
    """`steps` train steps of the material stage fed by a data.DeviceDataset, from one PRNG key.  Per
    step: step_key, rng = random_split(rng); batch_key, k = random_split(step_key); model_key, loss_key = random_split(k);
    dataset.next_train(batch_key) (one launch); rc.material_randoms(model_key, n, data_cfg.num_secondary_samples,
    train=True, loss_key=extra_loss_keys(loss_key)["material_smoothness"]) -- every random tensor of the forward and the
    smoothness noise in one launch, in HBM; material_env_stage_step; with opt_light also light_sampler_step on the same rays
    and randoms (light_cfg.num_secondary_samples must be the data loss's).  The host handles keys and scalars only: no
    tensor is made on the host or crosses PCIe inside the loop and nothing is read back.  The way the step's three keys
    come from `key` is this package's convention, as cache_stage_fit's is; neither it nor the tree behind material_randoms
    is pinned against a jax run.  -> the steps' loss dicts (0-d cuda tensors): "data", "material_smoothness",
    "regularizer/material_grid", "material_ray_sampler", and with opt_light "light_sampling", "regularizer/light_grid"."""
    K = int(data_cfg.num_secondary_samples)
    if opt_light is not None and int(light_cfg.num_secondary_samples) != K:
        raise ValueError("material_stage_fit: light_cfg.num_secondary_samples must equal data_cfg.num_secondary_samples "
                         "(both steps read the same randoms)")
    rng = prng.as_key(key)
    n = dataset.batch_size
    history = []
    for _ in range(int(steps)):
        step_key, rng = prng.random_split(rng)
        batch_key, k = prng.random_split(step_key)
        model_key, loss_key = prng.random_split(k)
        batch = dataset.next_train(batch_key)
        randoms = rc.material_randoms(model_key, n, K, train=True,
                                      loss_key=prng.extra_loss_keys(loss_key)["material_smoothness"])
        rays = batch.rays.hot_fields()
        losses = material_env_stage_step(rc, opt_material, opt_envmap, rays, randoms, batch.rgb, randoms["noise"],
                                         batch.rays.lossmult, group, data_cfg, smooth_cfg)
        if opt_light is not None:
            losses.update(light_sampler_step(rc, opt_light, rays, randoms, batch.rays.lossmult, group, light_cfg))
        history.append(losses)
    return history


# ---- the time-resolved cache ---------------------------------------------------------------------------------------

def transient_data_grads(rc, rays, cam_origins, jitters, gt, rgb_nocorr=None, gt_nocorr=None, lossmult=None, flat=None,
                         cfg: TransientDataLossConfig = TransientDataLossConfig()):
    """The time-resolved cache's data loss on a batch and its gradient of the two per-bin head layers:
    compute_transient_data_loss of rc_render_transient's rgb against gt ([n, n_bins, 3]) times data_loss_mult, under the loss
    type, use_itof and (frequency, phase) pairs of cfg (config.transient_data_loss_preset; an iToF or steady-state reading
    compares dtof_to_itof of the histograms, gt stays a histogram), accumulated into `flat` (layout rc.transient_head_grad_layout(); allocated zeroed when None).  rays: render_transient's fields
    (lights included); cam_origins: [n, 3] (replaces rays["cam_origins"] when given); jitters: per-level [n] sampler jitter
    (None = deterministic); rgb_nocorr / gt_nocorr: the unbiased loss's second pair (None: this render, gt).
    -> (flat, {"data": ..., "mse": ...}), 0-d cuda tensors: the reference's losses_flat key and its "mses" stat."""
    rays = dict(rays)
    if cam_origins is not None:
        rays["cam_origins"] = cam_origins
    randoms = None if jitters is None else {"jitter": list(jitters)}
    flat, losses = rc.transient_data_backward(rays, randoms, gt, rgb_nocorr, gt_nocorr, lossmult, cfg, flat)
    return flat, {"data": losses[0], "mse": losses[1]}


class TransientHeadOptimizer(CacheStageOptimizer):
    """The optimizer state of the time-resolved cache's two per-bin head layers on the device: flat params, mu, nu and
    gradients in the layout rc.transient_head_grad_layout() (key "transient_heads") and the optax count.
    param_group puts transient_indirect_layer in "Cache" and SurfaceLightField/output_rgba_layer in "SurfaceLightField" (the
    last listed prefix on the path wins), as create_optimizer does.  clip_gradients takes its norm per top-level module and
    both layers sit under Cache, whose other tensors this optimizer does not hold: with grad_max_norm > 0 that norm cannot
    be formed here, so it is refused.  A step is ONE rc_adam_update over this buffer, then rc_load_params_flat
    (RC_LAYOUT_TRANSIENT_HEADS).  init_from / params_dict / state_dict / load_state_dict as CacheStageOptimizer."""

    def __init__(self, rc, cfg: OptimizerConfig = OptimizerConfig()):
        if cfg.grad_max_norm > 0:
            raise NotImplementedError("TransientHeadOptimizer: grad_max_norm needs the norm over all of params/Cache")
        super().__init__(rc, cfg, ["transient_heads"])


def transient_head_step(rc, opt: TransientHeadOptimizer, rays, cam_origins, jitters, gt, rgb_nocorr=None, gt_nocorr=None,
                        lossmult=None, group=None, cfg: TransientDataLossConfig = TransientDataLossConfig()):
    """One train step of the per-bin heads on the transient data loss: transient_data_grads into the optimizer's zeroed
    gradient buffer, the pmean over `group` when torch.distributed runs, then opt.step().  cfg: the loss reading, as
    transient_data_grads takes it (any of config.transient_data_loss_preset's).  -> the losses dict of
    transient_data_grads."""
    return _train_step(opt, group, lambda tf: transient_data_grads(rc, rays, cam_origins, jitters, gt, rgb_nocorr, gt_nocorr,
                                                                   lossmult, opt.grads["transient_heads"], cfg))


# ---- the time-resolved cache's density fields and proposal samplers ---------------------------------

def transient_sampler_layout(cfg):
    """Python mirror of rc_transient_sampler_grad_layout: ([(name, offset, shape)], total floats).  Per level the density
    grid's tables in level order and the three density layers (kernel, bias each) -- weights.param_shapes lists them in
    this order --, then MLP_<last>/pred_normals_layer."""
    from .weights import param_shapes

    shapes = param_shapes(cfg)
    pred = f"params/Cache/Sampler/MLP_{cfg.num_levels - 1}/pred_normals_layer/"
    names = [k for l in range(cfg.num_levels) for k in shapes
             if k.startswith(f"params/Cache/Sampler/MLP_{l}/") and not k.startswith(pred)]
    names += [pred + "kernel", pred + "bias"]
    out, off = [], 0
    for k in names:
        out.append((k, off, tuple(shapes[k])))
        off += int(np.prod(shapes[k]))
    return out, off


def transient_sampler_grads(rc, rays, cam_origins, jitters, gt, train_frac: float, rgb_nocorr=None, gt_nocorr=None,
                            lossmult=None, flats=None, data_cfg: TransientDataLossConfig = TransientDataLossConfig(),
                            interlevel_cfg: Optional[InterlevelConfig] = None, geometry_cfg: Optional[GeometryLossConfig] = None,
                            mask_cfg: Optional[MaskLossConfig] = None, masks=None, look=None, backward_randoms=None,
                            scale: float = 1.0):
    """The time-resolved cache stage's losses on a batch and their gradients of the per-bin heads and of the sampler side
    (the three density fields and pred_normals_layer): the transient data loss with its weights path into MLP_<last>
    (rc_transient_data_backward_sampler), the spline interlevel loss, the four geometry terms, the mask loss and -- with
    look and backward_randoms, as mask_grads takes them -- its backward term, and the density-grid regularizer of every
    level.  The configs default to the cornell gin's (config.cornell_transient_*_config); train_frac sets the anneal.
    flats: {"transient_heads": flat, "transient_sampler": flat} to accumulate into (allocated zeroed when missing).
    scale multiplies the interlevel, geometry and mask terms (one copy of each is computed; the data loss and the
    regularizer count once).  The shader trunk and the appearance grid get no gradient, and the data loss reaches MLP_<last>
    through the compositing weights only.
    -> (flats, losses): data, mse, interlevel_<l>, the GEOMETRY_KEYS, mask[, mask_backwards], regularizer/density_grid."""
    from . import config as _config

    il = _config.cornell_transient_interlevel_config() if interlevel_cfg is None else interlevel_cfg
    ge = _config.cornell_transient_geometry_config() if geometry_cfg is None else geometry_cfg
    mk = _config.cornell_transient_mask_config() if mask_cfg is None else mask_cfg
    flats = dict(flats or {})
    rays = dict(rays)
    if cam_origins is not None:
        rays["cam_origins"] = cam_origins
    randoms = None if jitters is None else {"jitter": list(jitters)}
    anneal = anneal_at(train_frac, il)
    heads, sampler, d_losses = rc.transient_data_backward_sampler(rays, randoms, gt, rgb_nocorr, gt_nocorr, lossmult, data_cfg,
                                                                  flats.get("transient_heads"), flats.get("transient_sampler"))
    losses = {"data": d_losses[0], "mse": d_losses[1]}
    sampler, il_losses = rc.transient_interlevel_backward(rays, jitters, anneal, tuple(scale * m for m in il.mults), il.blurs,
                                                          lossmult, sampler)
    for l in range(rc.cfg.num_levels - 1):
        losses[f"interlevel_{l}"] = il_losses[l]
    sampler, g_losses = rc.transient_geometry_backward(rays, jitters, anneal, lossmult, geometry_terms(train_frac, ge, scale),
                                                       sampler)
    for k, key in enumerate(GEOMETRY_KEYS):
        losses[key] = g_losses[k]
    terms = mask_terms(train_frac, mk, scale)
    sampler, m_loss = rc.transient_mask_backward(rays, jitters, anneal, masks, lossmult, terms["mask"], sampler)
    losses["mask"] = m_loss[0]
    if mk.backward_mask_loss and look is not None and backward_randoms is not None:
        back = rc.backward_mask_rays(rays["origins"], look, backward_randoms["u1"], backward_randoms["u2"], mk.shadow_near_max,
                                     mk.secondary_normal_eps, mk.secondary_far)
        sampler, m_loss = rc.transient_mask_backward(back, backward_randoms.get("jitter"), anneal, None, lossmult,
                                                     terms["mask_backwards"], sampler)
        losses["mask_backwards"] = m_loss[0]
    reg = None
    for l in range(rc.cfg.num_levels):
        sampler, r = rc.transient_density_regularizer(l, ge.density_grid_mult, sampler)
        reg = r if reg is None else reg + r
    losses["regularizer/density_grid"] = reg[0]
    flats["transient_heads"], flats["transient_sampler"] = heads, sampler
    return flats, losses


class TransientSamplerOptimizer(CacheStageOptimizer):
    """The optimizer state of the time-resolved cache stage on the device: the sampler side in ONE flat buffer (key
    "transient_sampler": rc.transient_sampler_grad_layout()) and, with heads=True, the two per-bin head layers beside it (key
    "transient_heads"); params, mu, nu, gradients and the optax count.  param_group puts every sampler tensor in "Cache", as
    create_optimizer folds the prefixes (TransientHeadOptimizer names the heads' groups).  grad_max_norm > 0 is refused for
    TransientHeadOptimizer's reason: the norm is per top-level module, and params/Cache holds the shader trunk and the
    appearance grid, which this optimizer does not.  A step is ONE rc_adam_update over its buffers, then rc_load_params_flat
    per layout."""

    def __init__(self, rc, cfg: OptimizerConfig = OptimizerConfig(), heads: bool = True):
        if cfg.grad_max_norm > 0:
            raise NotImplementedError("TransientSamplerOptimizer: grad_max_norm needs the norm over all of params/Cache")
        super().__init__(rc, cfg, (["transient_heads"] if heads else []) + ["transient_sampler"])


def transient_cache_stage_step(rc, opt: TransientSamplerOptimizer, rays, cam_origins, jitters, gt, rgb_nocorr=None,
                               gt_nocorr=None, lossmult=None, group=None,
                               data_cfg: TransientDataLossConfig = TransientDataLossConfig(),
                               interlevel_cfg: Optional[InterlevelConfig] = None,
                               geometry_cfg: Optional[GeometryLossConfig] = None, mask_cfg: Optional[MaskLossConfig] = None,
                               masks=None, look=None, backward_randoms=None, scale: float = 1.0):
    """One train step of the time-resolved cache stage, heads and sampler side together: transient_sampler_grads into the
    optimizer's zeroed gradient buffers, the pmean over `group` when torch.distributed runs, then opt.step() (ONE
    rc_adam_update, the handle's refresh).  opt: a TransientSamplerOptimizer with heads=True.
    -> the losses dict of transient_sampler_grads."""
    if "transient_heads" not in opt.keys:
        raise ValueError("transient_cache_stage_step needs TransientSamplerOptimizer(heads=True)")
    return _train_step(opt, group, lambda tf: transient_sampler_grads(
        rc, rays, cam_origins, jitters, gt, tf, rgb_nocorr, gt_nocorr, lossmult, dict(opt.grads), data_cfg, interlevel_cfg,
        geometry_cfg, mask_cfg, masks, look, backward_randoms, scale))
