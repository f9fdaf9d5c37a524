"""ctypes binding of the C ABI in include/rc_abi.h (librc_hip.so).

This is the reference-side binding a maintainer would add: plain pointers and sizes,
no torch types cross the boundary.  torch is used only for device memory and streams.
The product path fails loudly when the HIP library is missing -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Iterable, Optional

import numpy as np

from .config import GridConfig, RenderConfig

RC_ABI_VERSION = 5
RC_MAX_LEVELS = 3
RC_ERR_MISSING_WEIGHT = -3          # the rc_status code probe.light_lobes tells apart (RcError.code)

RC_PASS_CACHE = 0x1
RC_PASS_SECONDARY = 0x2
RC_PASS_RESAMPLE = 0x4
RC_PASS_NO_ENVMAP = 0x8
RC_PASS_ENV_IMAGE = 0x10

RC_RELIGHT_BRDF = 0
RC_RELIGHT_ENV = 1

# rc_output_id -> (name, width); order must match include/rc_abi.h
OUTPUTS = (
    ("rgb", 3), ("acc", 1), ("distance_mean", 1), ("distance_percentile_5", 1), ("distance_median", 1),
    ("distance_percentile_95", 1), ("diffuse_rgb", 3), ("specular_rgb", 3), ("direct_rgb", 3),
    ("indirect_rgb", 3), ("albedo_rgb", 3), ("indirect_diffuse_rgb", 3), ("indirect_specular_rgb", 3),
    ("indirect_occ", 3), ("means", 3), ("normals", 3), ("normals_pred", 3), ("ray_dists", 1),
    ("light_dists", 1), ("env_map_rgb", 3), ("rgb_no_env", 3),
)
OUTPUT_ID = {name: i for i, (name, _) in enumerate(OUTPUTS)}
RC_OUT_COUNT = len(OUTPUTS)


class rc_grid_config(C.Structure):
    _fields_ = [("hash_map_size", C.c_int32), ("max_grid_size", C.c_int32), ("min_grid_size", C.c_int32),
                ("num_features", C.c_int32), ("bbox", C.c_float), ("precondition_scaling", C.c_float)]


class rc_config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32), ("num_levels", C.c_int32), ("num_samples", C.c_int32 * RC_MAX_LEVELS),
        ("proposal_grids", rc_grid_config * RC_MAX_LEVELS), ("appearance_grid", rc_grid_config),
        ("material_grid", rc_grid_config), ("light_grid", rc_grid_config),
        ("anneal", C.c_float), ("resample_padding", C.c_float), ("raydist_p", C.c_float),
        ("raydist_premult", C.c_float), ("shadow_normal_eps_dot_min", C.c_float), ("density_bias", C.c_float),
        ("contract_radius", C.c_float), ("roughness_bias", C.c_float), ("irradiance_bias", C.c_float),
        ("ambient_irradiance_bias", C.c_float), ("rgb_max", C.c_float), ("slf_ambient_bias", C.c_float),
        ("env_rgb_bias", C.c_float), ("env_map_distance", C.c_float), ("bg_intensity", C.c_float),
        ("percentiles", C.c_float * 3), ("num_resample", C.c_int32),
        ("diffuse_sample_fraction", C.c_float), ("secondary_normal_eps", C.c_float), ("secondary_near", C.c_float),
        ("secondary_far", C.c_float), ("min_roughness", C.c_float), ("default_F_0", C.c_float),
        ("vmf_scale", C.c_float), ("num_vmf", C.c_int32),
    ]


class rc_tensor_desc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("ndim", C.c_int32), ("shape", C.c_int64 * 4),
                ("on_device", C.c_int32)]


class rc_rays(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("origins", "directions", "viewdirs", "near", "far", "lights", "normals")]


class rc_grad_segment(C.Structure):
    _fields_ = [("name", C.c_char * 160), ("offset", C.c_int64), ("size", C.c_int64), ("ndim", C.c_int32),
                ("shape", C.c_int64 * 4)]


class rc_randoms(C.Structure):
    _fields_ = [("jitter", C.c_void_p * RC_MAX_LEVELS), ("gumbel", C.c_void_p), ("resample_inds", C.c_void_p)]


class rc_outputs(C.Structure):
    _fields_ = [("ptr", C.c_void_p * RC_OUT_COUNT)]


# rc_mat_output_id -> (name, width); order must match include/rc_abi.h
MAT_OUTPUTS = (
    ("rgb", 3), ("acc", 1), ("direct_rgb", 3), ("indirect_rgb", 3), ("diffuse_rgb", 3), ("specular_rgb", 3),
    ("direct_diffuse_rgb", 3), ("direct_specular_rgb", 3), ("indirect_diffuse_rgb", 3), ("indirect_specular_rgb", 3),
    ("indirect_occ", 1), ("lighting_irradiance", 3), ("material_albedo", 3), ("material_roughness", 1),
    ("material_metalness", 1), ("material_F_0", 1), ("means", 3), ("normals_to_use", 3), ("ray_dists", 1),
    ("light_dists", 1),
)
MAT_OUTPUT_ID = {name: i for i, (name, _) in enumerate(MAT_OUTPUTS)}
RC_MOUT_COUNT = len(MAT_OUTPUTS)


class rc_material_randoms(C.Structure):
    _fields_ = [("gumbel", C.c_void_p), ("vmf_noise", C.c_void_p), ("spec_u1", C.c_void_p), ("spec_u2", C.c_void_p),
                ("cos_u1", C.c_void_p), ("cos_u2", C.c_void_p), ("vmf_lobe", C.c_void_p), ("vmf_v", C.c_void_p),
                ("vmf_tmp", C.c_void_p), ("sec_jitter", C.c_void_p * RC_MAX_LEVELS), ("sec_gumbel", C.c_void_p),
                ("resample_inds", C.c_void_p), ("sec_resample_inds", C.c_void_p), ("vmf_lobe_gumbel", C.c_void_p)]


class rc_prng_segment(C.Structure):
    _fields_ = [("key", C.c_uint32 * 2), ("mode", C.c_int32), ("id", C.c_int32), ("lo", C.c_float), ("hi", C.c_float),
                ("n", C.c_int64), ("offset", C.c_int64), ("offset2", C.c_int64)]


RC_PRNG_MAX_SEGMENTS = 32
RC_PRNG_PLAN_TRAIN, RC_PRNG_PLAN_ENV_SAMPLER, RC_PRNG_PLAN_VMF_NOISE = 0x1, 0x2, 0x4


class rc_mat_outputs(C.Structure):
    _fields_ = [("ptr", C.c_void_p * RC_MOUT_COUNT)]


class rc_relight_args(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("picks_spec", C.c_void_p), ("picks_diff", C.c_void_p), ("T_spec", C.c_int32),
                ("T_diff", C.c_int32), ("albedo_ratio", C.c_void_p)]


class rc_transient_config(C.Structure):
    _fields_ = [("n_bins", C.c_int32), ("exposure_time", C.c_float), ("tfilter_sigma", C.c_float),
                ("transient_shift", C.c_float), ("bin_zero_threshold_light", C.c_int32), ("light_near", C.c_float),
                ("light_zero", C.c_int32), ("use_falloff", C.c_int32), ("indirect_scale", C.c_float),
                ("rgb_max", C.c_float), ("albedo_bias", C.c_float), ("brdf_bias", C.c_float),
                ("irradiance_bias", C.c_float), ("slf_rgb_bias", C.c_float), ("use_occlusions", C.c_int32),
                ("occ_threshold", C.c_float), ("shadow_near", C.c_float), ("shadow_far", C.c_float),
                ("reserved", C.c_int32 * 6)]


# rc_transient_output_id -> (name, trailing shape); order must match include/rc_abi.h
TRANSIENT_OUTPUTS = (
    ("rgb", "bins"), ("transient_direct_viz", "bins"), ("transient_indirect_viz", "bins"),
    ("transient_indirect_diffuse", "bins"), ("transient_indirect_specular", "bins"), ("integrated_rgb", 3),
    ("direct_rgb", 3), ("indirect_rgb", 3), ("diffuse_rgb", 3), ("specular_rgb", 3), ("albedo_rgb", 3), ("occ", 3),
    ("indirect_occ", 3), ("irradiance_rgb", 3), ("light_radiance_rgb", 3), ("n_dot_l_rgb", 3),
    ("direct_diffuse_rgb", 3), ("direct_specular_rgb", 3), ("indirect_diffuse_rgb", 3), ("indirect_specular_rgb", 3),
    ("direct_rgb_viz", 3), ("acc", 1), ("distance_mean", 1), ("distance_median", 1), ("distance_percentile_5", 1),
    ("distance_percentile_95", 1), ("means", 3), ("normals", 3), ("normals_pred", 3), ("ray_dists", 1),
    ("light_dists", 1),
)
TRANSIENT_OUTPUT_ID = {name: i for i, (name, _) in enumerate(TRANSIENT_OUTPUTS)}
RC_TOUT_COUNT = len(TRANSIENT_OUTPUTS)


class rc_transient_outputs(C.Structure):
    _fields_ = [("ptr", C.c_void_p * RC_TOUT_COUNT)]


RC_TSLICE_MAX = 8
# rc_render_transient_slices: the slice outputs (fields of rc_transient_slices) and the outputs `extra` may ask for
TRANSIENT_SLICE_OUTPUTS = ("rgb", "direct", "indirect")
TRANSIENT_SLICE_EXTRAS = ("acc", "distance_mean", "distance_median", "distance_percentile_5", "distance_percentile_95",
                          "means", "normals", "normals_pred", "ray_dists", "light_dists")


class rc_transient_slices(C.Structure):
    _fields_ = [("count", C.c_int32), ("t", C.c_float * RC_TSLICE_MAX), ("rgb", C.c_void_p), ("direct", C.c_void_p),
                ("indirect", C.c_void_p)]


# outputs table -> (its struct of pointers, name -> slot)
_OUTPUT_TABLES = {OUTPUTS: (rc_outputs, OUTPUT_ID), MAT_OUTPUTS: (rc_mat_outputs, MAT_OUTPUT_ID),
                  TRANSIENT_OUTPUTS: (rc_transient_outputs, TRANSIENT_OUTPUT_ID)}


class rc_camera(C.Structure):
    _fields_ = [("pixtocam", C.c_float * 9), ("camtoworld", C.c_float * 12), ("light", C.c_float * 3),
                ("near", C.c_float), ("far", C.c_float), ("camtype", C.c_int32),
                ("has_distortion", C.c_int32), ("distortion", C.c_float * 6),
                ("has_ndc", C.c_int32), ("pixtocam_ndc", C.c_float * 9),
                ("has_z_range", C.c_int32), ("z_range", C.c_float * 2), ("pix_dx", C.c_void_p), ("pix_dy", C.c_void_p)]


CAST_OUTPUTS = (("origins", 3), ("directions", 3), ("viewdirs", 3), ("radii", 1), ("imageplane", 2), ("look", 3), ("up", 3),
                ("lights", 3), ("near", 1), ("far", 1))


class rc_cast_outputs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _ in CAST_OUTPUTS]


class rc_camera_set(C.Structure):
    _fields_ = [("count", C.c_int32), ("pixtocams", C.c_void_p), ("camtoworlds", C.c_void_p), ("lights", C.c_void_p),
                ("near", C.c_float), ("far", C.c_float), ("camtype", C.c_int32),
                ("has_distortion", C.c_int32), ("distortion", C.c_float * 6),
                ("has_ndc", C.c_int32), ("pixtocam_ndc", C.c_float * 9),
                ("has_z_range", C.c_int32), ("z_range", C.c_float * 2), ("pix_dx", C.c_void_p), ("pix_dy", C.c_void_p)]


class rc_train_batch_outputs(C.Structure):
    _fields_ = [("rays", rc_cast_outputs)] + [(k, C.c_void_p) for k in ("rgb", "lossmult", "cam_idx", "pix_x", "pix_y")]


RC_IMAGE_F32, RC_IMAGE_U8 = 0, 1
BATCHING = {"all_images": 0, "single_image": 1}
CAMTYPES = {"perspective": 0, "pano": 1, "fisheye": 2, "fisheye_equisolid": 3}


class rc_geometry_loss(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("distortion_mult", "distortion_p", "distortion_premult", "orientation_mult",
                                         "pred_normal_mult", "pred_normal_w_grad_weight", "pred_normal_reverse_mult")]


class rc_geometry_smoothness(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("noise", "weight_normals", "weight_normals_pred", "weight_density")]


class rc_mask_loss(C.Structure):
    _fields_ = [("charb_padding", C.c_float), ("weight_opaque", C.c_float), ("weight_empty", C.c_float),
                ("zero_masks", C.c_int32)]


RC_ADAM_MAX_GROUPS = 8
RC_LAYOUT_SHADER = -1
RC_LAYOUT_LIGHT = -2
RC_LAYOUT_MATERIAL = -3
RC_LAYOUT_ENVMAP = -4
RC_LAYOUT_TRANSIENT_HEADS = -5
RC_LAYOUT_TRANSIENT_SAMPLER = -6


class rc_light_sampling_loss(C.Structure):
    _fields_ = [("mult", C.c_float), ("linear_to_srgb", C.c_int32)]


class rc_material_smoothness_loss(C.Structure):
    _fields_ = [("mult", C.c_float), ("weight_albedo", C.c_float), ("weight_other", C.c_float), ("noise", C.c_float),
                ("tensoir_albedo", C.c_int32)]


class rc_material_data_loss(C.Structure):
    _fields_ = [("mult", C.c_float), ("weight", C.c_float), ("exponent", C.c_float), ("eps", C.c_float),
                ("clip_val", C.c_float), ("thresh", C.c_float), ("use_gt_rawnerf", C.c_int32),
                ("use_combined_rawnerf", C.c_int32), ("use_norm_rawnerf", C.c_int32)]


class rc_transient_data_loss(C.Structure):
    _fields_ = [("mult", C.c_float), ("gauss_mult", C.c_float), ("gauss_constant_scale", C.c_float), ("exponent", C.c_float),
                ("eps", C.c_float), ("clip_val", C.c_float), ("thresh", C.c_float), ("use_gt_rawnerf", C.c_int32),
                ("use_combined_rawnerf", C.c_int32)]


# rc_transient_loss_type -> name; order must match include/rc_abi.h
TRANSIENT_LOSS_TYPES = ("rawnerf_transient_unbiased", "rawnerf_transient", "mse", "mse_unbiased", "mse_itof", "mse_itof_unbiased",
                        "rawnerf_transient_itof", "rawnerf_transient_itof_unbiased")
RC_TLOSS_COUNT = len(TRANSIENT_LOSS_TYPES)
RC_ITOF_MAX_PAIRS = 8


class rc_transient_data_loss_kind(C.Structure):
    _fields_ = [("base", rc_transient_data_loss), ("loss_type", C.c_int32), ("use_itof", C.c_int32), ("n_pairs", C.c_int32),
                ("pad", C.c_int32), ("frequency", C.c_double * RC_ITOF_MAX_PAIRS), ("phase_shift", C.c_double * RC_ITOF_MAX_PAIRS)]


def _itof_pairs(pairs):
    """[(frequency, phase)] floats of Config.itof_frequency_phase_shifts; more than RC_ITOF_MAX_PAIRS is refused here,
    where the C struct could not hold them."""
    pairs = [(float(f), float(ph)) for f, ph in pairs]
    if len(pairs) > RC_ITOF_MAX_PAIRS:
        raise ValueError(f"at most {RC_ITOF_MAX_PAIRS} (frequency, phase) pairs")
    return pairs


def transient_data_loss_c(cfg) -> rc_transient_data_loss:
    """The constants of a config.TransientDataLossConfig that every loss type shares."""
    return rc_transient_data_loss(mult=float(cfg.data_loss_mult), gauss_mult=float(cfg.data_loss_gauss_mult),
                                  gauss_constant_scale=float(cfg.transient_gauss_constant_scale),
                                  exponent=float(cfg.rawnerf_exponent), eps=float(cfg.rawnerf_eps),
                                  clip_val=float(cfg.clip_val), thresh=float(cfg.loss_thresh),
                                  use_gt_rawnerf=int(bool(cfg.use_gt_rawnerf)),
                                  use_combined_rawnerf=int(bool(cfg.use_combined_rawnerf)))


def transient_data_loss_kind_c(cfg) -> rc_transient_data_loss_kind:
    """rc_transient_data_backward_kind's struct of a config.TransientDataLossConfig."""
    pairs = _itof_pairs(cfg.itof_frequency_phase_shifts)
    ck = rc_transient_data_loss_kind(base=transient_data_loss_c(cfg), loss_type=TRANSIENT_LOSS_TYPES.index(cfg.loss_type),
                                     use_itof=int(bool(cfg.use_itof)), n_pairs=len(pairs))
    for i, (f, ph) in enumerate(pairs):
        ck.frequency[i], ck.phase_shift[i] = f, ph
    return ck


# rc_eval_slot -> name; order must match include/rc_abi.h
EVAL_SLOTS = ("mse", "psnr", "ssim", "transient_iou", "l1_mean", "l1_median", "mae")
RC_EVAL_COUNT = len(EVAL_SLOTS)
_EVAL_INPUTS = ("pred", "gt", "mask", "acc", "normals", "normals_gt", "distance_mean", "distance_median", "depth_gt")


class rc_eval_images(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in _EVAL_INPUTS + ("post_pred", "post_gt", "ssim_map")]
                + [("height", C.c_int32), ("width", C.c_int32), ("n_bins", C.c_int32), ("exposure", C.c_float),
                   ("img_scale", C.c_float), ("clip_eval", C.c_int32), ("skip_postprocess", C.c_int32)])


# rc_eval_si_slot -> name; order must match include/rc_abi.h
EVAL_SI_SLOTS = ("mse", "psnr", "ssim")
RC_EVAL_SI_COUNT = len(EVAL_SI_SLOTS)
RC_EVAL_SI_MAX_RADIUS = 8
RC_EVAL_SI_MAX_HALFWIDTH = 16
_EVAL_SI_MAPS = ("mse_map", "ssim_map", "mse_di", "mse_dj", "ssim_di", "ssim_dj")


class rc_eval_si_images(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("pred", "gt") + _EVAL_SI_MAPS]
                + [(k, C.c_int32) for k in ("height", "width", "radius_i", "radius_j", "window_halfwidth", "want_ssim")])


def search_radii_pair(search_radii):
    """(ri, rj) of the reference's `search_radii`: two integers."""
    try:
        ri, rj = search_radii
        ok = int(ri) == ri and int(rj) == rj
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"search_radii must be a pair of integers (i, j), not {search_radii!r}")
    return int(ri), int(rj)


# rc_albedo_slot -> name; order must match include/rc_abi.h
ALBEDO_SLOTS = ("mse", "psnr", "ratio_r", "ratio_g", "ratio_b", "valid")
RC_ALBEDO_COUNT = len(ALBEDO_SLOTS)


class rc_albedo_images(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in ("albedo", "acc", "albedo_gt", "mask")]
                + [("height", C.c_int32), ("width", C.c_int32), ("albedo_clip", C.c_float)]
                + [(k, C.c_void_p) for k in ("ratio", "post_pred", "post_gt", "ratio_im", "pairs")]
                + [("pairs_capacity", C.c_int64), ("pairs_count", C.c_void_p)])


# rc_vis_op -> name; order must match include/rc_abi.h
VIS_OPS = ("srgb", "binsum_srgb", "binsum_clip_srgb", "matte", "abs", "turbo")
VIS_OP_ID = {name: i for i, name in enumerate(VIS_OPS)}
RC_VIS_MAX_PERCENTILES = 8


class rc_vis_item(C.Structure):
    _fields_ = ([("src", C.c_void_p), ("channels", C.c_int32), ("n_bins", C.c_int32), ("op", C.c_int32),
                 ("nan_to_num", C.c_int32), ("scale", C.c_float), ("divide", C.c_float), ("offset", C.c_float),
                 ("exponent", C.c_float)]
                + [(k, C.c_void_p) for k in ("divisor", "acc", "mask", "bounds", "auto_bounds", "out_f32", "out_u8")])


RC_PROBE_MAX, RC_PROBE_MAX_LOBES = 16, 128
_PROBE_VIEW_REQUIRED = ("origins", "directions", "distance_median", "normals")
_PROBE_VIEW_BROADCAST = (("lights", 3), ("imageplane", 2), ("look", 3), ("up", 3))


class rc_probe_view(C.Structure):
    _fields_ = ([(k, C.c_void_p) for k in _PROBE_VIEW_REQUIRED] + [(k, C.c_void_p) for k, _ in _PROBE_VIEW_BROADCAST]
                + [("n_view", C.c_int64)])


ATLAS_OUTPUTS = (("density", 1), ("normals_pred", 3), ("normals", 3), ("material", 5), ("diffuse", 6), ("coverage", 1))


class rc_atlas_outputs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _ in ATLAS_OUTPUTS]


class rc_adam_buffer(C.Structure):
    _fields_ = [("params", C.c_void_p), ("grads", C.c_void_p), ("mu", C.c_void_p), ("nu", C.c_void_p), ("n", C.c_int64),
                ("nseg", C.c_int32), ("seg_offset", C.c_void_p), ("seg_size", C.c_void_p), ("seg_group", C.c_void_p)]


class rc_adam_step(C.Structure):
    _fields_ = ([("ngroups", C.c_int32)]
                + [(k, C.c_float * RC_ADAM_MAX_GROUPS) for k in ("lr", "b1", "b2", "one_minus_b1", "one_minus_b2", "eps",
                                                                 "bias_correction1", "bias_correction2")]
                + [("grad_max_val", C.c_float), ("grad_max_norm", C.c_float), ("zero_grads", C.c_int32)])


# Gradient layouts by key -- a density level (int), "shader", "light", "material", "envmap", "transient_heads", "transient_sampler": the C functions of its size and of its
# segments (a density level is their first argument) and its RC_LAYOUT_* id (rc_load_params_flat; a level is its own).
_GRAD_LAYOUTS = {
    int: ("rc_density_grad_size", "rc_density_grad_layout", None),
    "shader": ("rc_shader_grad_size", "rc_shader_grad_layout", RC_LAYOUT_SHADER),
    "light": ("rc_light_grad_size", "rc_light_grad_layout", RC_LAYOUT_LIGHT),
    "material": ("rc_material_grad_size", "rc_material_grad_layout", RC_LAYOUT_MATERIAL),
    "envmap": ("rc_envmap_grad_size", "rc_envmap_grad_layout", RC_LAYOUT_ENVMAP),
    "transient_heads": ("rc_transient_head_grad_size", "rc_transient_head_grad_layout", RC_LAYOUT_TRANSIENT_HEADS),
    "transient_sampler": ("rc_transient_sampler_grad_size", "rc_transient_sampler_grad_layout", RC_LAYOUT_TRANSIENT_SAMPLER),
}
_LAYOUT_KEYS = {row[2]: key for key, row in _GRAD_LAYOUTS.items() if key is not int}

# The prototype of every export of include/rc_abi.h: name -> (restype, [argtypes]).  The one source of load_library's
# ctypes prototypes and of EXPORTS; tests/test_abi_exports.py compares it with the header's declarations.
_H, _P, _I32, _I64, _F = C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_float        # _H: rc_handle*, _P: any other pointer
_RAYS, _RND, _MRND, _OUT = C.POINTER(rc_rays), C.POINTER(rc_randoms), C.POINTER(rc_material_randoms), C.POINTER(rc_outputs)
_PROTOTYPES = {
    "rc_create": (C.c_int, [C.POINTER(rc_config), C.c_int, C.POINTER(C.c_void_p)]),
    "rc_destroy": (None, [_H]),
    "rc_last_error": (C.c_char_p, [_H]),
    "rc_abi_version": (C.c_int, []),
    "rc_mlp_arithmetic": (C.c_int, []),
    "rc_load_weights": (C.c_int, [_H, C.POINTER(rc_tensor_desc), _I32]),
    "rc_render_rays": (C.c_int, [_H, _RAYS, _I64, _RND, C.c_uint32, _OUT, _P]),
    "rc_render_chunks": (C.c_int, [_H, _RAYS, _I64, _I64, C.c_uint32, _OUT, _I64, C.POINTER(C.c_void_p), _I32]),
    "rc_render_material": (C.c_int, [_H, _RAYS, _I64, _RND, _MRND, _I32, _OUT, C.POINTER(rc_mat_outputs), _P]),
    "rc_allgather_outputs": (C.c_int, [_H, _P, _OUT, _I64, _OUT, _P]),
    "rc_hashgrid_lookup": (C.c_int, [_H, _I32, _P, _I64, _P, _I32, _P]),
    "rc_sample_intervals": (C.c_int, [_H, _P, _P, _I64, _I32, _I32, _P, _P, _P]),
    "rc_workspace_ptr": (C.c_int, [_H, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "rc_set_profiling": (C.c_int, [_H, _I32]),
    "rc_set_graph_mode": (C.c_int, [_H, _I32]),
    "rc_set_fused": (C.c_int, [_H, _I32]),
    "rc_stage_count": (C.c_int, []),
    "rc_stage_name": (C.c_char_p, [_I32]),
    "rc_stage_times_ms": (C.c_int, [_H, C.POINTER(C.c_float), _I32]),
    "rc_set_transient": (C.c_int, [_H, _P]),
    "rc_render_transient": (C.c_int, [_H, _P, _P, _I64, _P, _P, _P, _P]),
    "rc_render_transient_slices": (C.c_int, [_H, _RAYS, _P, _I64, _P, _P, C.POINTER(rc_transient_slices),
                                             C.POINTER(rc_transient_outputs), _P]),
    "rc_cast_rays": (C.c_int, [_H, _P, _P, _P, _I64, _I32, _I32, _I32, _I32, _P, _P]),
    "rc_cast_rays_multi": (C.c_int, [_H, _P, _P, _P, _P, _I64, _P, _P, _P, _P]),
    "rc_train_batch": (C.c_int, [_H, _P, _P, _I32, _I32, _I32, _P, _P, _I32, _I32, _I32, _I64, _P, _P]),
    "rc_prng_fill": (C.c_int, [_H, _P, _I32, _F, _F, _I64, _P, _P]),
    "rc_material_randoms_plan": (C.c_int, [_P, _P, _I64, _I32, _F, _I32, _P, _I32, C.c_uint32, _P, _I32, _P, _P]),
    "rc_prng_fill_segments": (C.c_int, [_H, _P, _I32, _P, _I64, _P]),
    "rc_density_grad_size": (C.c_int64, [_H, _I32]),
    "rc_density_grad_layout": (C.c_int, [_H, _I32, _P, _I32, C.POINTER(C.c_int32)]),
    "rc_density_backward": (C.c_int, [_H, _I32, _P, _I64, _P, _P, _P, _P, _P]),
    "rc_hashgrid_grad_layout": (C.c_int, [_H, _I32, _P, _I32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "rc_hashgrid_backward": (C.c_int, [_H, _I32, _P, _I64, _P, _P, _I32, _P]),
    "rc_interlevel_backward": (C.c_int, [_H, _RAYS, _P, _I64, _RND, _F, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                         C.POINTER(C.c_void_p), _P, _P]),
    "rc_data_backward": (C.c_int, [_H, _RAYS, _P, _P, _I64, _RND, _F, _F, _F, _P, _P, _P, _P]),
    "rc_geometry_backward": (C.c_int, [_H, _RAYS, _P, _I64, _RND, _F, C.POINTER(rc_geometry_loss), _P, _P, _P, _P]),
    "rc_density_regularizer": (C.c_int, [_H, _I32, _F, _P, _P, _P]),
    "rc_normals_backward": (C.c_int, [_H, _P, _I64, _P, _P, _P, _P]),
    "rc_geometry_smoothness_backward": (C.c_int, [_H, _RAYS, _P, _I64, _RND, _F, _P, C.POINTER(rc_geometry_smoothness), _P,
                                                  _P, _P]),
    "rc_mask_backward": (C.c_int, [_H, _RAYS, _P, _P, _I64, _RND, _F, C.POINTER(rc_mask_loss), _P, _P, _P]),
    "rc_backward_mask_rays": (C.c_int, [_H, _P, _P, _P, _P, _I64, _F, _F, _F, _P, _P, _P, _P, _P]),
    "rc_adam_update": (C.c_int, [_H, C.POINTER(rc_adam_buffer), _I32, C.POINTER(rc_adam_step), _P]),
    "rc_load_params_flat": (C.c_int, [_H, _I32, _P, _P]),
    "rc_light_sampling_backward": (C.c_int, [_H, _RAYS, _P, _I64, _RND, _MRND, _I32, C.POINTER(rc_light_sampling_loss),
                                             _P, _P, _P]),
    "rc_light_regularizer": (C.c_int, [_H, _F, _P, _P, _P]),
    "rc_material_smoothness_backward": (C.c_int, [_H, _RAYS, _P, _I64, _RND, _MRND, _P,
                                                  C.POINTER(rc_material_smoothness_loss), _P, _P, _P]),
    "rc_material_regularizer": (C.c_int, [_H, _F, _P, _P, _P]),
    "rc_material_data_backward": (C.c_int, [_H, _RAYS, _P, _P, _I64, _RND, _MRND, _I32, C.POINTER(rc_material_data_loss),
                                            _P, _P, _P]),
    "rc_material_data_backward_env": (C.c_int, [_H, _RAYS, _P, _P, _I64, _RND, _MRND, _I32,
                                                C.POINTER(rc_material_data_loss), _F, _P, _P, _P, _P]),
    "rc_transient_data_backward": (C.c_int, [_H, _RAYS, _P, _I64, _RND, _P, _P, _P, _P, C.POINTER(rc_transient_data_loss),
                                             _P, _P, _P]),
    "rc_transient_data_backward_kind": (C.c_int, [_H, _RAYS, _P, _I64, _RND, _P, _P, _P, _P,
                                                  C.POINTER(rc_transient_data_loss_kind), _P, _P, _P]),
    "rc_transient_data_backward_sampler": (C.c_int, [_H, _RAYS, _P, _I64, _RND, _P, _P, _P, _P,
                                                     C.POINTER(rc_transient_data_loss_kind), _P, _P, _P, _P]),
    "rc_transient_interlevel_backward": (C.c_int, [_H, _RAYS, _P, _I64, _RND, _F, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                   _P, _P, _P]),
    "rc_transient_geometry_backward": (C.c_int, [_H, _RAYS, _P, _I64, _RND, _F, C.POINTER(rc_geometry_loss), _P, _P, _P]),
    "rc_transient_mask_backward": (C.c_int, [_H, _RAYS, _P, _P, _I64, _RND, _F, C.POINTER(rc_mask_loss), _P, _P, _P]),
    "rc_transient_density_regularizer": (C.c_int, [_H, _I32, _F, _P, _P, _P]),
    "rc_dtof_to_itof": (C.c_int, [_H, _P, _I64, _I32, C.POINTER(C.c_double), C.POINTER(C.c_double), _P, _P]),
    "rc_eval_image": (C.c_int, [_H, C.POINTER(rc_eval_images), _P, _P]),
    "rc_eval_shift_invariant": (C.c_int, [_H, C.POINTER(rc_eval_si_images), _P, _P]),
    "rc_eval_albedo": (C.c_int, [_H, C.POINTER(rc_albedo_images), _P, _P]),
    "rc_albedo_ratio": (C.c_int, [_H, _P, _I64, _P, _I32, _I32, _P, _P]),
    "rc_weighted_percentile": (C.c_int, [_H, _P, _P, _I64, _P, _I32, _P, _P]),
    "rc_image_max": (C.c_int, [_H, _P, _I64, _P, _P]),
    "rc_vis_images": (C.c_int, [_H, C.POINTER(rc_vis_item), _I32, _I32, _I32, _P]),
    "rc_vis_turbo_lut": (C.c_int, [_P]),
    "rc_probe_rays": (C.c_int, [_H, C.POINTER(rc_probe_view), _P, _I32, _I32, _I32, _F, _F, _F, _I32,
                                C.POINTER(rc_cast_outputs), _P, _P]),
    "rc_vmf_panorama": (C.c_int, [_H, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P]),
    "rc_query_points": (C.c_int, [_H, _P, _I64, _I32, _P, _P, _P, _P, _P]),
    "rc_density_lattice": (C.c_int, [_H, C.POINTER(C.c_float), C.POINTER(C.c_float), _I32, _I32, _I32, _I32, _P, _P]),
    "rc_isosurface": (C.c_int, [_H, _P, _I32, _I32, _I32, _F, C.POINTER(C.c_float), C.POINTER(C.c_float), _P, _P, _I64, _P,
                                _I64, _P, _P]),
    "rc_atlas_layout": (C.c_int, [_I64, _I32, C.POINTER(C.c_int32)]),
    "rc_atlas_uvs": (C.c_int, [_H, _I64, _I32, _P, _P]),
    "rc_atlas_points": (C.c_int, [_H, _P, _I64, _P, _I64, _I32, _I64, _I64, _P, _P, _P]),
    "rc_query_cache_diffuse": (C.c_int, [_H, _P, _I64, _P, _P]),
    "rc_bake_atlas": (C.c_int, [_H, _P, _I64, _P, _I64, _I32, _I32, C.POINTER(rc_atlas_outputs), _P]),
    "rc_set_env_image": (C.c_int, [_H, _P, _P, _P, _P, _I32, _I32, _P]),
    "rc_env_tables": (C.c_int, [_H, _P, _I32, _I32, _F, _P, _P, _P, _P]),
    "rc_env_lookup": (C.c_int, [_H, _P, _I64, _P, _P]),
    "rc_env_pick": (C.c_int, [_H, _P, _I32, _P, _P]),
    "rc_render_relight": (C.c_int, [_H, _RAYS, _I64, _RND, _MRND, _I32, C.POINTER(rc_relight_args), _OUT,
                                    C.POINTER(rc_mat_outputs), _P]),
}
for _size, _layout, _ in (row for key, row in _GRAD_LAYOUTS.items() if key is not int):        # the named layouts
    _PROTOTYPES[_size] = (C.c_int64, [_H])
    _PROTOTYPES[_layout] = (C.c_int, [_H, _P, _I32, C.POINTER(C.c_int32)])
EXPORTS = tuple(_PROTOTYPES)

_LIB = None
_RAY_FIELDS = ("origins", "directions", "viewdirs", "near", "far", "lights", "normals")


def library_path() -> str:
    # RC_HIP_LIBRARY: a diagnostic / A-B build of the same ABI (tools/README.md); the product is the in-tree library
    return os.environ.get("RC_HIP_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "librc_hip.so")


def mlp_arithmetic() -> str:
    """'f32-mfma' or 'bf16x3-split' (include/rc_abi.h rc_mlp_arithmetic): how the loaded library multiplies in the shader MLPs."""
    return "bf16x3-split" if load_library().rc_mlp_arithmetic() == 1 else "f32-mfma"


def source_hash() -> str:
    """sha256 over the kernel / ABI sources the library is built from: what measurement files kept under profiles/
    (PMC traffic, in-kernel phase stamps) are tagged with, so that a bench run can tell a stale file from a current one."""
    import hashlib
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "csrc")
    files = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".inc")))
    files.append(os.path.join(os.path.dirname(here), "include", "rc_abi.h"))
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def load_library():
    """dlopen librc_hip.so.  Raises (never falls back) when it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the render path.")
    lib = C.CDLL(path)
    for name, (restype, argtypes) in _PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _LIB = lib
    return lib


def _grid_c(g: GridConfig) -> rc_grid_config:
    return rc_grid_config(g.hash_map_size, g.max_grid_size, g.min_grid_size, g.num_features, g.bbox,
                          g.precondition_scaling)


def config_to_c(cfg: RenderConfig) -> rc_config:
    c = rc_config()
    c.abi_version = RC_ABI_VERSION
    c.num_levels = cfg.num_levels
    for i, (_, _, n) in enumerate(cfg.sampling_strategy):
        c.num_samples[i] = n
        c.proposal_grids[i] = _grid_c(cfg.proposal_grids[i])
    c.appearance_grid = _grid_c(cfg.appearance_grid)
    c.material_grid = _grid_c(cfg.material_grid)
    c.light_grid = _grid_c(cfg.light_grid)
    for k in ("anneal", "resample_padding", "raydist_p", "raydist_premult", "shadow_normal_eps_dot_min",
              "density_bias", "contract_radius", "roughness_bias", "irradiance_bias", "ambient_irradiance_bias",
              "rgb_max", "slf_ambient_bias", "env_rgb_bias", "env_map_distance"):
        setattr(c, k, float(getattr(cfg, k)))
    c.bg_intensity = float(cfg.bg_intensity)
    for i, p in enumerate(cfg.percentiles):
        c.percentiles[i] = float(p)
    c.num_resample = cfg.num_resample
    for k in ("diffuse_sample_fraction", "secondary_normal_eps", "secondary_near", "secondary_far", "min_roughness",
              "default_F_0", "vmf_scale"):
        setattr(c, k, float(getattr(cfg, k)))
    c.num_vmf = cfg.num_vmf
    return c


def transient_config_to_c(t) -> rc_transient_config:
    c = rc_transient_config()
    for k in ("n_bins", "bin_zero_threshold_light"):
        setattr(c, k, int(getattr(t, k)))
    for k in ("light_zero", "use_falloff", "use_occlusions"):
        setattr(c, k, 1 if getattr(t, k) else 0)
    for k in ("exposure_time", "tfilter_sigma", "transient_shift", "light_near", "indirect_scale", "rgb_max", "albedo_bias",
              "brdf_bias", "irradiance_bias", "slf_rgb_bias", "occ_threshold", "shadow_near", "shadow_far"):
        setattr(c, k, float(getattr(t, k)))
    return c


def _ptr(x):
    """Device address of a tensor, NULL for None."""
    return None if x is None else x.data_ptr()


def _camera_options(s, camtype="perspective", distortion_params=None, pixtocam_ndc=None, z_range=None):
    """The optional members that rc_camera and rc_camera_set share.  distortion_params: dict of floats like the reference's
    (k1..k4, p1, p2; missing = 0)."""
    s.camtype = CAMTYPES[getattr(camtype, "value", camtype)]
    if distortion_params is not None:
        s.has_distortion = 1
        for i, k in enumerate(("k1", "k2", "k3", "k4", "p1", "p2")):
            s.distortion[i] = float(distortion_params.get(k, 0.0))
    if pixtocam_ndc is not None:
        s.has_ndc = 1
        for i, v in enumerate(np.asarray(pixtocam_ndc, np.float32).reshape(9)):
            s.pixtocam_ndc[i] = float(v)
    if z_range is not None:
        s.has_z_range = 1
        s.z_range[0], s.z_range[1] = float(z_range[0]), float(z_range[1])


def _rays_of_cast(t, lossmult, cam_idx, light_idx, pix_x_int=None, pix_y_int=None):
    """The Rays of one cast: the tensors of CAST_OUTPUTS (the camera is its own virtual camera) plus the per-ray extras."""
    from .rays import Rays
    return Rays(origins=t["origins"], lights=t["lights"], directions=t["directions"], viewdirs=t["viewdirs"],
                radii=t["radii"], imageplane=t["imageplane"], look=t["look"], up=t["up"], cam_origins=t["origins"],
                vcam_look=t["look"], vcam_up=t["up"], vcam_origins=t["origins"], lossmult=lossmult, near=t["near"],
                far=t["far"], cam_idx=cam_idx, light_idx=light_idx, pix_x_int=pix_x_int, pix_y_int=pix_y_int)


class AdamTable:
    """The rc_adam_buffer array of a fixed set of flat buffers, built once (the segment arrays stay alive with it)."""

    def __init__(self, buffers):
        if not 1 <= len(buffers) <= 8:
            raise ValueError("1 to 8 buffers per rc_adam_update call")
        self.bufs = (rc_adam_buffer * len(buffers))()
        self._keep = []
        for i, (p, g, m, v, segs) in enumerate(buffers):
            n = p.numel()
            for t in (p, g, m, v):
                if t.numel() != n or not t.is_cuda or not t.is_contiguous() or str(t.dtype) != "torch.float32":
                    raise ValueError("params, grads, mu, nu: contiguous float32 cuda tensors of one size")
            off = np.ascontiguousarray([s[0] for s in segs], dtype=np.int64)
            size = np.ascontiguousarray([s[1] for s in segs], dtype=np.int64)
            grp = np.ascontiguousarray([s[2] for s in segs], dtype=np.int32)
            self._keep += [p, g, m, v, off, size, grp]
            b = self.bufs[i]
            b.params, b.grads, b.mu, b.nu = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
            b.n, b.nseg = n, len(segs)
            b.seg_offset, b.seg_size, b.seg_group = off.ctypes.data, size.ctypes.data, grp.ctypes.data


class CameraSet:
    """rc_camera_set with its device tables (RadianceCache.camera_set): uploaded once, reused by every call."""

    def __init__(self, rc, pixtocams, camtoworlds, lights=None, near=0.0, far=0.0, camtype="perspective",
                 distortion_params=None, pixtocam_ndc=None, z_range=None):
        torch = rc._torch
        host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        c2w = np.asarray(host(camtoworlds), np.float32)
        if c2w.ndim != 3 or c2w.shape[1] < 3 or c2w.shape[2] != 4:
            raise ValueError("camtoworlds must be [C, 3, 4] or [C, 4, 4]")
        c2w = np.array(c2w[:, :3, :4], np.float32, order="C")
        self.count = int(c2w.shape[0])
        p2c = np.asarray(host(pixtocams), np.float32)
        p2c = np.array(np.broadcast_to(p2c, (self.count, 3, 3)), np.float32, order="C")      # a copy: broadcast views are read-only
        self.pixtocams = rc._dev(p2c.reshape(self.count, 9))
        self.camtoworlds = rc._dev(c2w.reshape(self.count, 12))
        self.lights = None
        if lights is not None:
            self.lights = rc._dev(np.array(np.broadcast_to(np.asarray(host(lights), np.float32), (self.count, 3)), np.float32, order="C"))
        self.near, self.far = float(near), float(far)
        s = rc_camera_set()
        s.count = self.count
        s.pixtocams, s.camtoworlds = self.pixtocams.data_ptr(), self.camtoworlds.data_ptr()
        s.lights = _ptr(self.lights)
        s.near, s.far = self.near, self.far
        _camera_options(s, camtype, distortion_params, None if pixtocam_ndc is None else host(pixtocam_ndc), z_range)
        self.struct = s


class RcError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"rc error {code}: {msg}")
        self.code = code


class RadianceCache:
    """One rc_handle: the cache renderer bound to one GPU."""

    def __init__(self, cfg: RenderConfig, device: int = 0):
        import torch  # device memory / streams only

        self._torch = torch
        self.lib = load_library()
        self.cfg = cfg
        self.device = device
        self._h = C.c_void_p()
        ccfg = config_to_c(cfg)
        rc = self.lib.rc_create(C.byref(ccfg), device, C.byref(self._h))
        if rc != 0:
            raise RcError(rc, (self.lib.rc_last_error(None) or b"").decode())
        self._keep = []
        self._vmf_noise_cache = {}          # n -> the PRNGKey(1) constant [n, num_vmf, 3] (material_randoms)
        if cfg.transient is not None:
            self._check(self.lib.rc_set_transient(self._h, C.byref(transient_config_to_c(cfg.transient))))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.rc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            raise RcError(rc, (self.lib.rc_last_error(self._h) or b"").decode())

    # -- weights ----------------------------------------------------------------------------
    def load_weights(self, weights: Dict[str, object]):
        """weights: flat dict 'params/...' -> numpy array or torch tensor (float32)."""
        torch = self._torch
        descs = (rc_tensor_desc * len(weights))()
        keep = []
        for i, (name, w) in enumerate(weights.items()):
            if isinstance(w, torch.Tensor):
                t = w.detach().to(torch.float32).contiguous()
                keep.append(t)
                ptr, on_dev, shape = t.data_ptr(), int(t.is_cuda), tuple(t.shape)
            else:
                a = np.ascontiguousarray(w, dtype=np.float32)
                keep.append(a)
                ptr, on_dev, shape = a.ctypes.data, 0, a.shape
            bname = name.encode()
            keep.append(bname)
            descs[i].name = bname
            descs[i].data = ptr
            descs[i].ndim = len(shape)
            for k, s in enumerate(shape):
                descs[i].shape[k] = s
            descs[i].on_device = on_dev
        # rc_load_weights copies with blocking hipMemcpy on the null stream, which is NOT ordered against torch's
        # non-blocking side streams: finish whatever produced device-resident tensors first (an optimizer step)
        if any(isinstance(w, torch.Tensor) and w.is_cuda for w in weights.values()):
            torch.cuda.synchronize(self.device)
        self._check(self.lib.rc_load_weights(self._h, descs, len(weights)))

    # -- marshalling shared by the entry points ----------------------------------------------
    def _zeros_like_many(self, shapes):
        """Zero-filled float32 cuda tensors of the given shapes as views of ONE allocation (one fill kernel instead of
        one per output; every view starts on a 256-byte boundary)."""
        torch = self._torch
        offs, total = [], 0
        for shp in shapes:
            offs.append(total)
            total += (int(np.prod(shp)) + 63) // 64 * 64
        flat = torch.zeros(max(total, 1), dtype=torch.float32, device=f"cuda:{self.device}")
        return [flat[o: o + int(np.prod(shp))].view(shp) for o, shp in zip(offs, shapes)]

    def _dev(self, x, dtype=None):
        torch = self._torch
        dtype = dtype or torch.float32
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(x))
        elif x.is_cuda and x.dtype == dtype and x.is_contiguous() and x.device.index == self.device:
            return x                    # already where and how the library wants it (the per-call path of a training loop)
        return x.to(device=f"cuda:{self.device}", dtype=dtype).contiguous()

    def _stream(self, handle=None):
        """The raw hipStream_t a call is enqueued on: `handle`, or torch's current stream of this device."""
        return self._torch.cuda.current_stream(self.device).cuda_stream if handle is None else handle

    def _fill_rays(self, rays, held, checked):
        """rc_rays of a dict of ray fields (_RAY_FIELDS; a missing one stays NULL), every device tensor registered in
        `held` -> (struct, ray count).  checked: the fields are viewed as [n, 3] / [n] and must agree on n.  Otherwise
        (the lean path) a float32 cuda tensor is passed by pointer as it is and n is the size of `near`."""
        r, n = rc_rays(), None
        for k in _RAY_FIELDS:
            v = rays.get(k)
            if v is None:
                continue
            t = self._dev(v)
            if checked:
                t = t.reshape(-1, 3) if k not in ("near", "far") else t.reshape(-1)
                n = t.shape[0] if n is None else n
                if t.shape[0] != n:
                    raise ValueError(f"ray field {k} has {t.shape[0]} rows, expected {n}")
            elif k == "near":
                n = t.numel()
            held[k] = t
            setattr(r, k, t.data_ptr())
        return r, n

    def _rays_struct(self, rays):
        held = {}
        r, n = self._fill_rays(rays, held, checked=True)
        return r, held, n

    def _randoms(self, held, jitter=None, gumbel=None, resample_inds=None, n=None, tag=""):
        """rc_randoms of a per-level jitter list (None, or a None level, stays NULL) and optional gumbel / resample_inds.
        The launch that reads them is asynchronous: every device copy and the struct itself are registered in `held`
        (keys prefixed with `tag`).  n: when given, the number of values each level's jitter must hold."""
        rnd = rc_randoms()
        if jitter is not None:
            for l, j in enumerate(jitter):
                if j is not None:
                    t = held[f"{tag}jit{l}"] = self._dev(j)
                    if n is not None and t.numel() != n:
                        raise ValueError(f"jitter of level {l} has {t.numel()} values, expected {n}")
                    rnd.jitter[l] = t.data_ptr()
        if gumbel is not None:
            held[tag + "gumbel"] = self._dev(gumbel)
            rnd.gumbel = held[tag + "gumbel"].data_ptr()
        if resample_inds is not None:
            held[tag + "inds"] = self._dev(resample_inds, self._torch.int32)
            rnd.resample_inds = held[tag + "inds"].data_ptr()
        held[tag + "rnd"] = rnd
        return rnd

    def _pass_randoms(self, randoms, held):
        """rc_render_rays' `rnd` argument of a randoms dict (jitter, gumbel, resample_inds), NULL for None."""
        if randoms is None:
            return None
        return C.byref(self._randoms(held, randoms.get("jitter"), randoms.get("gumbel"), randoms.get("resample_inds")))

    def _jitter_struct(self, jitters, held, n):
        return None if jitters is None else C.byref(self._randoms(held, jitters, n=n))

    def _outputs(self, table, names, shape_of, out=None):
        """The outputs `names` of `table` (OUTPUTS, MAT_OUTPUTS or TRANSIENT_OUTPUTS), shaped by shape_of(name) -> (dict
        name -> float32 cuda tensor, outputs struct holding their pointers).  The tensors are views of ONE zero-filled
        allocation, or the caller's buffers `out`, checked."""
        torch = self._torch
        struct, ids = _OUTPUT_TABLES[table]
        if out is None:
            out = dict(zip(names, self._zeros_like_many([shape_of(nm) for nm in names])))
        cout, res = struct(), {}
        for nm in names:
            t, shape = out[nm], shape_of(nm)
            if tuple(t.shape) != shape or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"output buffer {nm}: expected contiguous float32 cuda tensor of shape {shape}")
            res[nm] = t
            cout.ptr[ids[nm]] = t.data_ptr()
        return res, cout

    # -- hot path ---------------------------------------------------------------------------
    def render_rays(self, rays: Dict[str, object], randoms: Optional[Dict[str, object]] = None,
                    pass_mask: int = RC_PASS_CACHE, outputs: Optional[Iterable[str]] = None,
                    out: Optional[Dict[str, object]] = None):
        """rays: dict with origins, directions, viewdirs [n,3], near, far [n] or [n,1], optional lights,
        normals.  Returns dict name -> torch cuda tensor ([n,3] or [n]).  Passing the dict returned by
        an earlier call as `out` reuses its buffers (same pointers -> the captured hipGraph is replayed)."""
        r, held, n = self._rays_struct(rays)
        rnd_p = self._pass_randoms(randoms, held)
        names = [nm for nm, _ in OUTPUTS] if outputs is None else list(outputs)
        if out is not None:
            names = list(out.keys())
        res, cout = self._outputs(OUTPUTS, names, lambda nm: (n, 3) if OUTPUTS[OUTPUT_ID[nm]][1] == 3 else (n,), out)
        self._check(self.lib.rc_render_rays(self._h, C.byref(r), n, rnd_p, pass_mask, C.byref(cout), self._stream()))
        self._keep = [held]   # keep inputs alive until the next call (async enqueue)
        return res

    # -- lean per-chunk launch (models.render_image's hot loop at render_chunk_size = 1024) ------------
    def output_plan(self, names, n: int):
        """Layout of ONE flat float32 allocation holding the outputs `names` of an n-ray batch (every output starts on a
        256-byte boundary): (total floats, {name: (offset, shape)}, [(rc_output_id, offset)])."""
        offs, total, ids = {}, 0, []
        for nm in names:
            width = OUTPUTS[OUTPUT_ID[nm]][1]
            offs[nm] = (total, (n, 3) if width == 3 else (n,))
            ids.append((OUTPUT_ID[nm], total))
            total += (n * width + 63) // 64 * 64
        return max(total, 1), offs, ids

    @staticmethod
    def _plan_outputs(plan, base: int) -> rc_outputs:
        """rc_outputs pointing into a flat float32 buffer at address `base` that `plan` (output_plan) lays out."""
        cout = rc_outputs()
        for oid, off in plan[2]:
            cout.ptr[oid] = base + 4 * off
        return cout

    def render_chunk(self, rays: Dict[str, object], randoms, pass_mask: int, plan, out_flat=None, stream_handle=None):
        """rc_render_rays into one fresh flat buffer laid out by `plan` (output_plan).  The hot-loop variant of
        render_rays: device-resident float32 ray fields are passed by pointer as they are (no reshape / copy), the
        outputs are not wrapped into per-key tensors.  Returns (flat tensor, n)."""
        held = {}
        r, n = self._fill_rays(rays, held, checked=False)
        rnd_p = self._pass_randoms(randoms, held)
        # out_flat: a zero-filled float32 cuda buffer of `total` elements the caller provides (a row of its arena)
        flat = out_flat
        if flat is None:
            flat = self._torch.zeros(plan[0], dtype=self._torch.float32, device=f"cuda:{self.device}")
        cout = self._plan_outputs(plan, flat.data_ptr())
        # stream_handle: the raw hipStream_t to enqueue on (a caller that alternates streams skips torch's context manager)
        self._check(self.lib.rc_render_rays(self._h, C.byref(r), n, rnd_p, pass_mask, C.byref(cout),
                                            self._stream(stream_handle)))
        self._keep = held          # inputs stay alive until the next call (async enqueue)
        return flat, n

    def render_chunks(self, rays: Dict[str, object], chunk: int, n_chunks: int, pass_mask: int, plan, arena, stream_handles):
        """rc_render_chunks: the chunk loop of render_image in native code.  `rays`: float32 cuda tensors holding
        n_chunks * chunk rays each (contiguous, the last chunk edge-padded by the caller); `arena`: zero-filled
        [n_chunks, total] float32 cuda tensor whose rows are laid out by `plan`; chunk i goes to
        stream_handles[i % len] (raw hipStream_t values).  One ABI call for the whole image."""
        held = {}
        r, _ = self._fill_rays(rays, held, checked=False)
        for k, v in held.items():
            assert v is rays[k], k          # passed as it is: a contiguous float32 tensor on this device
            assert v.numel() == n_chunks * chunk * (1 if k in ("near", "far") else 3), (k, tuple(v.shape))
        total = plan[0]
        assert arena.is_contiguous() and tuple(arena.shape) == (n_chunks, total)
        cout = self._plan_outputs(plan, arena.data_ptr())
        hs = (C.c_void_p * len(stream_handles))(*stream_handles)
        self._check(self.lib.rc_render_chunks(self._h, C.byref(r), chunk, n_chunks, pass_mask, C.byref(cout), total, hs,
                                              len(stream_handles)))
        self._keep = held

    # -- gradient layouts and the shared head of the loss calls --------------------------------
    def _segments(self, query, args, tail=()):
        """The two calls of an rc_*_grad_layout query (count, then the segments): [(tensor name, offset, shape)]."""
        cnt = C.c_int32()
        self._check(query(self._h, *args, None, 0, C.byref(cnt), *tail))
        segs = (rc_grad_segment * cnt.value)()
        self._check(query(self._h, *args, segs, cnt.value, C.byref(cnt), *tail))
        return [(s.name.decode(), int(s.offset), tuple(int(v) for v in s.shape[: s.ndim])) for s in segs]

    def _layout_fn(self, key, which):
        """(C function, leading arguments) of gradient layout `key`'s size (which=0) or segments (which=1) query."""
        if isinstance(key, str):
            return getattr(self.lib, _GRAD_LAYOUTS[key][which]), ()
        return getattr(self.lib, _GRAD_LAYOUTS[int][which]), (key,)

    def _grad_size(self, key):
        """Floats of gradient layout `key` (_GRAD_LAYOUTS; fixed by the config: asked once)."""
        sizes = self.__dict__.setdefault("_grad_sizes", {})
        total = sizes.get(key)
        if total is None:
            fn, args = self._layout_fn(key, 0)
            total = int(fn(self._h, *args))
            if total < 0:
                self._check(total)
            sizes[key] = total
        return total

    def _grad_layout(self, key):
        """[(tensor name, offset, shape)] of gradient layout `key` and its size in floats."""
        fn, args = self._layout_fn(key, 1)
        return self._segments(fn, args), self._grad_size(key)

    def _grad_buffer(self, flat, total, what="grads"):
        """A flat gradient buffer of `total` floats: `flat` checked, or a zeroed one when it is None."""
        torch = self._torch
        if flat is None:
            return torch.zeros(total, dtype=torch.float32, device=f"cuda:{self.device}")
        if flat.numel() != total or flat.dtype != torch.float32 or not flat.is_cuda or not flat.is_contiguous():
            raise ValueError(f"{what} must be a contiguous float32 cuda tensor of {total} elements")
        return flat

    def _loss_prologue(self, key, grad, stream_handle=None, slots=1):
        """The head of a loss call with one gradient buffer: the buffer of layout `key` (None for grad=False; `grad`
        checked, or allocated zeroed when None), the zeroed float32 loss tensor [slots] (2 for the transient loss, 4 for
        the geometry terms) and the stream (the current one when stream_handle is None)."""
        flat = None if grad is False else self._grad_buffer(grad, self._grad_size(key))
        loss = self._torch.zeros(slots, dtype=self._torch.float32, device=f"cuda:{self.device}")
        return flat, loss, self._stream(stream_handle)

    def _loss_prologue_pair(self, grads, slots=1):
        """_loss_prologue of data_backward / geometry_backward, whose gradient goes to two buffers: (density flat of the
        last level, shader flat), either one None (allocated zeroed); grads=False gives (None, None)."""
        flats = [None, None]
        if grads is not False:
            given = list(grads) if grads is not None else [None, None]
            for i, key in enumerate((self.cfg.num_levels - 1, "shader")):
                flats[i] = self._grad_buffer(given[i], self._grad_size(key), f"grads[{i}]")
        _, loss, stream = self._loss_prologue(None, False, slots=slots)
        return flats, loss, stream

    def _regularizer(self, fn, key, args, grad):
        """rc_{density,light,material}_regularizer: fn(handle, *args, grad flat, loss, stream) -> (grad flat or None, loss)."""
        flat, loss, stream = self._loss_prologue(key, grad)
        self._check(fn(self._h, *args, _ptr(flat), loss.data_ptr(), stream))
        return flat, loss

    def _lossmult(self, lossmult, held, n):
        """Per-ray loss weights [n] (kept alive in `held`), or None."""
        if lossmult is None:
            return None
        lm = self._dev(lossmult).reshape(-1)
        if lm.shape[0] != n:
            raise ValueError("lossmult must have one value per ray")
        held["lossmult"] = lm
        return lm

    def _cache_loss_head(self, rays, jitters, lossmult):
        """What every per-ray cache loss marshals first: (rc_rays, the tensors kept alive, n, rc_randoms of the per-level
        jitters or None, lossmult [n] or None)."""
        r, held, n = self._rays_struct(rays)
        return r, held, n, self._jitter_struct(jitters, held, n), self._lossmult(lossmult, held, n)

    @staticmethod
    def _terms_struct(ctype, what, defaults, terms):
        """The ctypes struct of a loss's `terms` dict laid over `defaults`; a key that is no field of the struct is refused."""
        t = dict(defaults)
        t.update(terms or {})
        unknown = set(t) - {k for k, _ in ctype._fields_}
        if unknown:
            raise ValueError(f"unknown {what} fields {sorted(unknown)}")
        return ctype(**{k: float(t[k]) if typ is C.c_float else int(bool(t[k])) for k, typ in ctype._fields_ if k in t})

    def _interlevel(self, transient, rays, jitters, anneal, mults, blurs, lossmult, grads, levels=None):
        """interlevel_backward (grads: per proposal level a flat or None, `levels` those whose backward runs) and
        transient_interlevel_backward (grads: the one sampler flat, None or False)."""
        r, held, n = self._rays_struct(rays)
        nprop = self.cfg.num_levels - 1
        if len(mults) != nprop or len(blurs) != nprop:
            raise ValueError(f"mults and blurs need {nprop} values")
        rnd_p = self._jitter_struct(jitters, held, n)
        lm = self._lossmult(lossmult, held, n)
        if transient:
            fn = self.lib.rc_transient_interlevel_backward
            flats, losses, stream = self._loss_prologue("transient_sampler", grads, slots=max(nprop, 1))
            where = _ptr(flats)
        else:
            fn = self.lib.rc_interlevel_backward
            levels = tuple(range(nprop)) if levels is None else tuple(levels)
            flats = list(grads) if grads is not None else [None] * nprop
            where = (C.c_void_p * nprop)()
            for l in range(nprop):
                if l not in levels:
                    flats[l] = None
                    continue
                flats[l] = self._grad_buffer(flats[l], self._grad_size(l), f"grads[{l}]")
                where[l] = flats[l].data_ptr()
            _, losses, stream = self._loss_prologue(None, False, slots=max(nprop, 1))
        m = (C.c_float * nprop)(*[float(v) for v in mults])
        b = (C.c_float * nprop)(*[float(v) for v in blurs])
        self._check(fn(self._h, C.byref(r), _ptr(lm), n, rnd_p, float(anneal), m, b, where, losses.data_ptr(), stream))
        self._keep = [held]
        return flats, losses

    def _geometry(self, transient, rays, jitters, anneal, lossmult, terms, grads):
        """geometry_backward (grads: (density flat, shader flat), None or False) and transient_geometry_backward (grads: the
        one sampler flat, None or False)."""
        r, held, n, rnd_p, lm = self._cache_loss_head(rays, jitters, lossmult)
        cfg = self._terms_struct(rc_geometry_loss, "geometry loss", {"distortion_p": -0.25, "distortion_premult": 1e4}, terms)
        if transient:
            fn = self.lib.rc_transient_geometry_backward
            flats, losses, stream = self._loss_prologue("transient_sampler", grads, slots=4)
            where = (_ptr(flats),)
        else:
            fn = self.lib.rc_geometry_backward
            flats, losses, stream = self._loss_prologue_pair(grads, slots=4)
            where, flats = (_ptr(flats[0]), _ptr(flats[1])), (flats[0], flats[1])
        self._check(fn(self._h, C.byref(r), _ptr(lm), n, rnd_p, float(anneal), C.byref(cfg), *where, losses.data_ptr(), stream))
        self._keep = [held]
        return flats, losses

    def _mask(self, transient, rays, jitters, anneal, masks, lossmult, terms, grads):
        """mask_backward (grads: the last level's density flat) and transient_mask_backward (grads: the sampler flat)."""
        r, held, n, rnd_p, lm = self._cache_loss_head(rays, jitters, lossmult)
        mk = None
        if masks is not None:
            mk = self._dev(masks).reshape(-1)
            if mk.shape[0] != n:
                raise ValueError("masks must have one value per ray")
            held["masks"] = mk
        cfg = self._terms_struct(rc_mask_loss, "mask loss", {"charb_padding": 1e-3, "weight_opaque": 1.0, "weight_empty": 1.0,
                                                             "zero_masks": 0}, terms)
        fn = self.lib.rc_transient_mask_backward if transient else self.lib.rc_mask_backward
        flat, loss, stream = self._loss_prologue("transient_sampler" if transient else self.cfg.num_levels - 1, grads)
        self._check(fn(self._h, C.byref(r), _ptr(mk), _ptr(lm), n, rnd_p, float(anneal), C.byref(cfg), _ptr(flat), loss.data_ptr(),
                       stream))
        self._keep = [held]
        return flat, loss

    def density_grad_layout(self, level: int):
        """rc_density_grad_layout: [(tensor name, offset, shape)] of the gradient buffer of proposal level `level`
        (the reference's parameter-tree names), and its total size in floats."""
        return self._grad_layout(level)

    def shader_grad_layout(self):
        """rc_shader_grad_layout: [(tensor name, offset, shape)] of the gradient buffer of the data loss's shader side
        (MLP_<last>/pred_normals_layer, the appearance-grid tables, the Cache/Shader dense layers), and its size."""
        return self._grad_layout("shader")

    def hashgrid_grad_layout(self, grid_id: int):
        """rc_hashgrid_grad_layout: [(tensor name, offset, shape)] of the table-gradient buffer of a grid, and its size."""
        total = C.c_int64()
        return self._segments(self.lib.rc_hashgrid_grad_layout, (grid_id,), (C.byref(total),)), int(total.value)

    def hashgrid_backward(self, grid_id: int, points, d_features, grads=None, apply_contraction: bool = True):
        """rc_hashgrid_backward: scatter d L / d features [n, L*F] (the layout hashgrid_lookup returns) into the tables'
        gradient buffer (flat float32 cuda tensor of hashgrid_grad_layout(grid_id)[1] elements; accumulated into when given)."""
        pts = self._dev(points).reshape(-1, 3).contiguous()
        n = pts.shape[0]
        df = self._dev(d_features).reshape(n, -1).contiguous()
        grads = self._grad_buffer(grads, self.hashgrid_grad_layout(grid_id)[1])
        g = self.cfg_grid(grid_id)
        if df.shape[1] != g.out_dim:
            raise ValueError(f"d_features must have {g.out_dim} columns")
        self._check(self.lib.rc_hashgrid_backward(self._h, grid_id, pts.data_ptr(), n, df.data_ptr(), grads.data_ptr(),
                                                  1 if apply_contraction else 0, self._stream()))
        self._keep = [pts, df]
        return grads

    def density_backward(self, level: int, points, d_density, d_feature=None, grads=None):
        """rc_density_backward: gradients of L w.r.t. the hash-grid tables and the density MLP of proposal level `level`
        given d L / d density [n] (and d L / d feature [n, 64]) at the world-space sample means `points` [n, 3].
        Returns (grads, density): `grads` is the flat float32 cuda buffer of density_grad_layout(level), accumulated
        into when passed in (zeroed and allocated otherwise)."""
        torch = self._torch
        pts = self._dev(points).reshape(-1, 3).contiguous()
        n = pts.shape[0]
        dd = self._dev(d_density).reshape(-1).contiguous()
        if dd.shape[0] != n:
            raise ValueError("d_density must have one value per point")
        df = None
        if d_feature is not None:
            df = self._dev(d_feature).reshape(n, 64).contiguous()
        grads = self._grad_buffer(grads, self._grad_size(level))
        dens = torch.empty(n, dtype=torch.float32, device=f"cuda:{self.device}")
        self._check(self.lib.rc_density_backward(self._h, level, pts.data_ptr(), n, dd.data_ptr(), _ptr(df),
                                                 grads.data_ptr(), dens.data_ptr(), self._stream()))
        self._keep = [pts, dd, df]
        return grads, dens

    def interlevel_backward(self, rays: Dict[str, object], jitters=None, anneal: float = 0.4, mults=(0.01, 0.01),
                            blurs=(0.03, 0.003), lossmult=None, grads=None, levels=None):
        """rc_interlevel_backward: the spline interlevel loss of the proposal levels on a batch of rays and its gradient
        w.r.t. the hash-grid tables and density MLP of each proposal level (loss_utils.spline_interlevel_loss).
        jitters: per-level [n] sampler jitter (None = the deterministic sampler); anneal: the train-time resampling
        exponent (train.anneal_at); lossmult: [n] or None (1).  grads: per proposal level a flat float32 cuda buffer
        (density_grad_layout(level)), accumulated into; a missing one is allocated zeroed.  levels: the proposal levels
        whose backward runs (default all); the others get no gradient (None in the result).
        Returns (flat buffers, losses [num_levels - 1] cuda tensor)."""
        return self._interlevel(False, rays, jitters, anneal, mults, blurs, lossmult, grads, levels)

    def data_backward(self, rays: Dict[str, object], rgb, jitters=None, anneal: float = 0.4, lossmult=None,
                      charb_padding: float = 1e-3, mult: float = 1.0, grads=None):
        """rc_data_backward: the charb data loss of the cache pass against target colours `rgb` [n, 3] and its
        gradient w.r.t. the last density level (density_grad_layout(num_levels - 1)) and the shader side
        (shader_grad_layout).  jitters / anneal as interlevel_backward; lossmult: [n] or None (1).  grads: (density
        flat, shader flat) to accumulate into, either None (allocated zeroed); grads=False computes the loss only.
        Returns ((density flat, shader flat), loss [1] cuda tensor); one copy of the term (the reference adds it twice)."""
        r, held, n = self._rays_struct(rays)
        rnd_p = self._jitter_struct(jitters, held, n)
        gt = self._dev(rgb).reshape(-1, 3).contiguous()
        if gt.shape[0] != n:
            raise ValueError("rgb must be [n, 3]")
        held["gt"] = gt
        lm = self._lossmult(lossmult, held, n)
        flats, loss, stream = self._loss_prologue_pair(grads)
        self._check(self.lib.rc_data_backward(self._h, C.byref(r), gt.data_ptr(), _ptr(lm), n, rnd_p, float(anneal),
                                              float(charb_padding), float(mult), _ptr(flats[0]), _ptr(flats[1]),
                                              loss.data_ptr(), stream))
        self._keep = [held]
        return (flats[0], flats[1]), loss

    def geometry_backward(self, rays: Dict[str, object], jitters=None, anneal: float = 0.4, lossmult=None, terms=None,
                          grads=None):
        """rc_geometry_backward: the distortion, orientation, predicted-normal and reverse predicted-normal losses of the
        last sampler level and their gradient w.r.t. the last density level (density_grad_layout(num_levels - 1)) and
        pred_normals_layer (its segment of shader_grad_layout).  terms: {rc_geometry_loss field: value} (multipliers
        with the ease / decay applied; missing fields are 0, distortion_p / _premult default to the hotdog gin's
        -0.25 / 1e4).  jitters / anneal / lossmult as data_backward.  grads: (density flat, shader flat) to accumulate
        into, either None (allocated zeroed); grads=False computes the losses only.
        Returns ((density flat, shader flat), losses [4] cuda tensor); one copy of each term."""
        return self._geometry(False, rays, jitters, anneal, lossmult, terms, grads)

    def density_regularizer(self, level: int, mult: float, grad=None):
        """rc_density_regularizer: mult * sum over the tables of density grid `level` of 0.5 * mean(x^2)
        (param_regularizer_loss, 'density_grid').  grad: flat buffer of density_grad_layout(level) to accumulate
        mult * x / numel into (allocated zeroed when None); grad=False computes the loss only.
        Returns (grad flat or None, loss [1] cuda tensor)."""
        return self._regularizer(self.lib.rc_density_regularizer, level, (int(level), float(mult)), grad)

    def normals_backward(self, points, d_normals, grads=None):
        """rc_normals_backward: the gradient THROUGH the analytic normals of the last sampler level: of
        sum(d_normals * n(points)), n = nan_to_num(-l2_normalize(d raw / d x)), w.r.t. the last level's hash-grid tables
        and the kernels of its density MLP (the bias segments are left as they are: their gradient is an exact zero).
        points, d_normals: [n, 3].  Returns (grads, normals): `grads` is the flat float32 cuda buffer of
        density_grad_layout(num_levels - 1), accumulated into when passed in (zeroed and allocated otherwise)."""
        torch = self._torch
        pts = self._dev(points).reshape(-1, 3).contiguous()
        n = pts.shape[0]
        dn = self._dev(d_normals).reshape(-1, 3).contiguous()
        if dn.shape[0] != n:
            raise ValueError("d_normals must have one row per point")
        grads = self._grad_buffer(grads, self._grad_size(self.cfg.num_levels - 1))
        normals = torch.empty(n, 3, dtype=torch.float32, device=f"cuda:{self.device}")
        self._check(self.lib.rc_normals_backward(self._h, pts.data_ptr(), n, dn.data_ptr(), grads.data_ptr(),
                                                 normals.data_ptr(), self._stream()))
        self._keep = [pts, dn]
        return grads, normals

    def geometry_smoothness_backward(self, rays: Dict[str, object], jitters, anneal: float, noise, lossmult=None, terms=None,
                                     grads=None):
        """rc_geometry_smoothness_backward: train_utils.geometry_smoothness_loss on the last sampler level and its
        gradient w.r.t. the last density level (density_grad_layout(num_levels - 1)), the analytic normals differentiable
        at the sample means and at the perturbed means.  noise: [n, S, 3] standard normals
        (prng.geometry_smoothness_noise); terms: {rc_geometry_smoothness field: value} (weights with the caller's mult
        applied; noise defaults to 0.1, weight_normals to 0.001, the other two weights to 0).  jitters / anneal /
        lossmult as data_backward.  grads: the density flat to accumulate into, None (allocated zeroed) or False (the
        loss only).  Returns (density flat or None, loss [1] cuda tensor); one copy of the term."""
        r, held, n, rnd_p, lm = self._cache_loss_head(rays, jitters, lossmult)
        S = self.cfg.sampling_strategy[-1][2]
        nz = self._dev(noise).reshape(-1).contiguous()
        if nz.shape[0] != n * S * 3:
            raise ValueError(f"noise must be [n, {S}, 3]")
        held["noise"] = nz
        cfg = self._terms_struct(rc_geometry_smoothness, "geometry smoothness",
                                 {"noise": 0.1, "weight_normals": 0.001, "weight_normals_pred": 0.0, "weight_density": 0.0}, terms)
        flat, loss, stream = self._loss_prologue(self.cfg.num_levels - 1, grads)
        self._check(self.lib.rc_geometry_smoothness_backward(self._h, C.byref(r), _ptr(lm), n, rnd_p, float(anneal),
                                                             _ptr(nz), C.byref(cfg), _ptr(flat), loss.data_ptr(), stream))
        self._keep = [held]
        return flat, loss

    def backward_mask_rays(self, origins, look, u1, u2, shadow_near_max: float = 0.2, normal_eps: float = 1e-2,
                           far: float = 2.0):
        """rc_backward_mask_rays: the rays of the backward mask term (train_utils._compute_backward_mask_loss), one per
        batch ray from origins [n, 3] and the camera look vectors look [n, 3]; u1, u2: [n] uniforms in [0, 1) (the two
        columns of prng.backward_mask_randoms' draw).  Returns the ray dict mask_backward takes: origins, directions, viewdirs
        (the directions' own tensor), near, far -- cuda tensors, written on the current stream."""
        torch = self._torch
        o = self._dev(origins).reshape(-1, 3).contiguous()
        n = o.shape[0]
        lk = self._dev(look).reshape(-1, 3).contiguous()
        a, b = self._dev(u1).reshape(-1).contiguous(), self._dev(u2).reshape(-1).contiguous()
        if lk.shape[0] != n or a.shape[0] != n or b.shape[0] != n:
            raise ValueError("origins, look, u1 and u2 must have one row per ray")
        dev = f"cuda:{self.device}"
        out = {"origins": torch.empty(n, 3, dtype=torch.float32, device=dev),
               "directions": torch.empty(n, 3, dtype=torch.float32, device=dev),
               "near": torch.empty(n, dtype=torch.float32, device=dev), "far": torch.empty(n, dtype=torch.float32, device=dev)}
        self._check(self.lib.rc_backward_mask_rays(self._h, o.data_ptr(), lk.data_ptr(), a.data_ptr(), b.data_ptr(), n,
                                                   float(shadow_near_max), float(normal_eps), float(far),
                                                   out["origins"].data_ptr(), out["directions"].data_ptr(),
                                                   out["near"].data_ptr(), out["far"].data_ptr(), self._stream()))
        self._keep = [o, lk, a, b]
        out["viewdirs"] = out["directions"]
        return out

    def mask_backward(self, rays: Dict[str, object], jitters=None, anneal: float = 0.4, masks=None, lossmult=None,
                      terms=None, grads=None):
        """rc_mask_backward: the mask loss of the last sampler level's opacity (train_utils.compute_mask_loss) and its
        gradient w.r.t. the last density level (density_grad_layout(num_levels - 1)).  masks: [n] or None (ones);
        terms: {rc_mask_loss field: value} (weights with the ease / decay applied; charb_padding defaults to 1e-3, the
        weights to 1, zero_masks to 0).  jitters / anneal / lossmult as data_backward.  grads: the density flat to
        accumulate into, None (allocated zeroed) or False (the loss only).
        Returns (density flat or None, loss [1] cuda tensor); one copy of the term."""
        return self._mask(False, rays, jitters, anneal, masks, lossmult, terms, grads)

    def light_grad_layout(self):
        """rc_light_grad_layout: [(tensor name, offset, shape)] of the LightSampler gradient buffer (the light_grid tables,
        then layers_0, layers_1, output_layer), and its size in floats."""
        return self._grad_layout("light")

    def light_sampling_backward(self, rays: Dict[str, object], randoms: Dict[str, object], num_secondary_samples: int = None,
                                lossmult=None, mult: float = 1.0, linear_to_srgb: bool = True, grad=None,
                                stream_handle=None):
        """rc_light_sampling_backward: render_material's forward with the same rays / randoms / num_secondary_samples
        (up to the secondary trace), the light_sampling loss (vmf_loss_fn over both suffixes) and its gradient w.r.t.
        the LightSampler parameters (light_grad_layout).  grad: flat buffer to accumulate into (allocated zeroed when
        None); grad=False computes the loss only.  Returns (grad flat or None, loss [1] cuda tensor)."""
        K = num_secondary_samples or self.cfg.num_secondary_samples
        r, held, n = self._rays_struct(rays)
        rnd, mr = self._material_randoms(randoms, n, K, held)
        lm = self._lossmult(lossmult, held, n)
        cfg = rc_light_sampling_loss(mult=float(mult), linear_to_srgb=int(bool(linear_to_srgb)))
        flat, loss, stream = self._loss_prologue("light", grad, stream_handle)
        self._check(self.lib.rc_light_sampling_backward(self._h, C.byref(r), _ptr(lm), n, C.byref(rnd), C.byref(mr), K,
                                                        C.byref(cfg), _ptr(flat), loss.data_ptr(), stream))
        self._keep = [held]
        return flat, loss

    def light_regularizer(self, mult: float, grad=None):
        """rc_light_regularizer: mult * sum over the light grid's tables of 0.5 * mean(x^2) (param_regularizer_loss,
        'light_grid').  grad: flat buffer of light_grad_layout to accumulate mult * x / numel into (allocated zeroed when
        None); grad=False computes the loss only.  Returns (grad flat or None, loss [1] cuda tensor)."""
        return self._regularizer(self.lib.rc_light_regularizer, "light", (float(mult),), grad)

    # -- optimizer ------------------------------------------------------------------------------
    def adam_update(self, buffers, step: Dict[str, object], stream_handle=None):
        """rc_adam_update: one launch of the Adam step over flat buffers (plus two with the norm clip).
        buffers: [(params, grads, mu, nu, segments)] -- contiguous float32 cuda tensors of one size each and
        segments = [(offset, size, group)] covering the buffer in order (AdamTable builds them once);
        step: per-group lists lr, b1, b2, one_minus_b1, one_minus_b2, eps, bias_correction1, bias_correction2
        (float32 values of the reference's expressions, nrc_amd.train.adam_scalars) and grad_max_val, grad_max_norm,
        zero_grads.  Ordered on the current stream."""
        table = buffers if isinstance(buffers, AdamTable) else AdamTable(buffers)
        st = rc_adam_step()
        st.ngroups = len(step["lr"])
        if not 1 <= st.ngroups <= RC_ADAM_MAX_GROUPS:
            raise ValueError(f"1 to {RC_ADAM_MAX_GROUPS} groups")
        for k in ("lr", "b1", "b2", "one_minus_b1", "one_minus_b2", "eps", "bias_correction1", "bias_correction2"):
            arr = getattr(st, k)
            for g, v in enumerate(step[k]):
                arr[g] = float(v)
        st.grad_max_val = float(step.get("grad_max_val", 0.0))
        st.grad_max_norm = float(step.get("grad_max_norm", 0.0))
        st.zero_grads = int(bool(step.get("zero_grads", False)))
        self._check(self.lib.rc_adam_update(self._h, table.bufs, len(table.bufs), C.byref(st), self._stream(stream_handle)))

    def load_params_flat(self, layout, params, stream_handle=None):
        """rc_load_params_flat: load every tensor of one gradient layout (a density level, "shader", "light", "material",
        "envmap" or, on a time-resolved handle, "transient_heads" / "transient_sampler") from a flat float32 cuda buffer in that layout -- table
        copies ordered on the current stream, the dense layers in one copy to the host (the call waits for the stream
        there).  Renders afterwards equal those after load_weights of the same tensors, bitwise."""
        torch = self._torch
        key = layout if isinstance(layout, str) else _LAYOUT_KEYS.get(int(layout), int(layout))
        lay = _GRAD_LAYOUTS[key][2] if isinstance(key, str) else key
        total = self._grad_size(key)
        if params.numel() != total or params.dtype != torch.float32 or not params.is_cuda or not params.is_contiguous():
            raise ValueError(f"params must be a contiguous float32 cuda tensor of {total} elements")
        self._check(self.lib.rc_load_params_flat(self._h, lay, params.data_ptr(), self._stream(stream_handle)))

    def prng_fill(self, key, shape, mode: str = "uniform", minval: float = 0.0, maxval: float = 1.0):
        """rc_prng_fill: the tensor jax.random.{bits,uniform,normal,gumbel}(key, shape) of the reference's pinned jax
        holds, generated in HBM.  key: uint32[2] (prng.PRNGKey / prng.split)."""
        from . import prng
        torch = self._torch
        modes = {"bits": prng.MODE_BITS, "uniform": prng.MODE_UNIFORM, "normal": prng.MODE_NORMAL, "gumbel": prng.MODE_GUMBEL}
        if mode not in modes:
            raise ValueError(f"unknown mode {mode!r}")
        k = (C.c_uint32 * 2)(*[int(v) for v in prng.as_key(key)])
        shape = tuple(int(v) for v in shape)
        n = int(np.prod(shape)) if shape else 1
        out = torch.empty(shape, dtype=torch.int32 if mode == "bits" else torch.float32, device=f"cuda:{self.device}")
        self._check(self.lib.rc_prng_fill(self._h, k, modes[mode], float(minval), float(maxval), n, out.data_ptr(),
                                          self._stream()))
        return out

    def prng_fill_segments(self, segs, arena):
        """rc_prng_fill_segments: every segment of `segs` (a ctypes array or a list of rc_prng_segment) into `arena`, a
        32-bit cuda tensor, in one launch."""
        if not isinstance(segs, C.Array):
            segs = (rc_prng_segment * len(segs))(*segs)
        if not (arena.is_cuda and arena.is_contiguous() and arena.element_size() == 4):
            raise ValueError("arena must be a contiguous cuda tensor of 32-bit words")
        self._check(self.lib.rc_prng_fill_segments(self._h, segs, len(segs), arena.data_ptr(), arena.numel(), self._stream()))

    def material_randoms(self, key, n: int, K: int = None, train: bool = False, env_sampler: bool = False, loss_key=None,
                         vmf_noise_in_arena: bool = False):
        """Every random tensor of one material-stage forward from the model's rng `key`, drawn in HBM: the plan in C
        (rc_material_randoms_plan, the tree of prng.material_stage_plan), ONE arena allocation, ONE launch
        (rc_prng_fill_segments).  Returns the randoms dict render_material / the *_backward calls / render_relight take:
        jitter[levels], gumbel, spec_u1/u2, cos_u1/u2, vmf_lobe_gumbel, vmf_v, vmf_tmp, sec_jitter[levels] and sec_gumbel in
        the ABI's [spec | diff] layout, `noise` [n, 3] when loss_key (the key material_smoothness receives) is given, and
        with env_sampler the two host keys picks_key_spec / picks_key_diff instead of the sampler members.  Every tensor is
        a cuda view of the one arena, except vmf_noise: the PRNGKey(1) constant depends on n alone and comes from a per-n
        cache of the handle (vmf_noise_in_arena=True draws it with the plan instead).  train: prng.material_stage_plan."""
        from . import prng
        torch = self._torch
        cfg = self.cfg
        n, K = int(n), int(K or cfg.num_secondary_samples)
        flags = ((RC_PRNG_PLAN_TRAIN if train else 0) | (RC_PRNG_PLAN_ENV_SAMPLER if env_sampler else 0)
                 | (RC_PRNG_PLAN_VMF_NOISE if vmf_noise_in_arena else 0))
        segs, count, words = material_randoms_plan(key, n, K, cfg.diffuse_sample_fraction, cfg.num_vmf,
                                                   [lvl[2] for lvl in cfg.sampling_strategy], flags, loss_key)
        arena = torch.empty(words, dtype=torch.float32, device=f"cuda:{self.device}")
        self._check(self.lib.rc_prng_fill_segments(self._h, segs, count, arena.data_ptr(), words, self._stream()))
        Ks, Kd, Kc, Kl = prng.material_split(cfg, K)
        S, V = int(cfg.sampling_strategy[-1][2]), int(cfg.num_vmf)
        by_id = {segs[i].id: segs[i] for i in range(count)}
        view = lambda off, shape: arena[off:off + int(np.prod(shape))].view(shape)
        out = {}
        ids = prng.MEMBER_IDS
        NL = len(cfg.sampling_strategy)
        out["jitter"] = [view(by_id[ids["jitter"] + l].offset, (n, 1)) for l in range(NL)]
        out["gumbel"] = view(by_id[ids["gumbel"]].offset, (n, S))
        if not env_sampler:
            if vmf_noise_in_arena:
                out["vmf_noise"] = view(by_id[ids["vmf_noise"]].offset, (n, V, 3))
            else:
                cache = self._vmf_noise_cache
                if n not in cache:
                    cache[n] = self.prng_fill(prng.random_split(prng.PRNGKey(1))[0], (n, V, 3), "normal")
                out["vmf_noise"] = cache[n]
            for name, cnt in (("spec_u", Ks), ("cos_u", Kc)):
                g = by_id[ids[name]]
                out[name + "1"], out[name + "2"] = view(g.offset, (n, cnt)), view(g.offset2, (n, cnt))
            out["vmf_lobe_gumbel"] = view(by_id[ids["vmf_lobe_gumbel"]].offset, (n, V))
            out["vmf_v"] = view(by_id[ids["vmf_v"]].offset, (n, Kl, 2))
            out["vmf_tmp"] = view(by_id[ids["vmf_tmp"]].offset, (n, Kl))
        else:
            for name in ("picks_key_spec", "picks_key_diff"):
                out[name] = np.array(list(by_id[ids[name]].key), dtype=np.uint32)
        out["sec_jitter"] = [view(by_id[ids["spec_jitter"] + l].offset, (n * K, 1)) for l in range(NL)]
        out["sec_gumbel"] = view(by_id[ids["spec_gumbel"]].offset, (n * K, S))
        if loss_key is not None:
            out["noise"] = view(by_id[ids["noise"]].offset, (n, 3))
        return out

    # -- rays from cameras ------------------------------------------------------------------------
    def _cast_tensors(self, shape, out):
        torch = self._torch
        t = {}
        for k, width in CAST_OUTPUTS:
            t[k] = torch.empty(tuple(shape) + (width,), dtype=torch.float32, device=f"cuda:{self.device}")
            setattr(out, k, t[k].data_ptr())
        return t

    def _pix_jitter(self, pix_jitter, n, per="pixel"):
        """The two sub-pixel offset arrays (dx, dy) on the device, flat with n values each; None for None."""
        if pix_jitter is None:
            return None
        torch = self._torch
        jit = [self._dev(j if isinstance(j, torch.Tensor) else np.ascontiguousarray(j, dtype=np.float32)).reshape(-1)
               for j in pix_jitter]
        if jit[0].numel() != n or jit[1].numel() != n:
            raise ValueError(f"pix_jitter: two arrays with one value per {per}")
        return jit

    def cast_rays(self, camera, pix_x_int=None, pix_y_int=None, rect=None, pix_jitter=None):
        """rc_cast_rays: rays of `camera` (pixtocam [3,3], camtoworld [3,4], light, near, far; optional camtype,
        distortion_params, pixtocam_ndc, z_range as in camera_utils.pixels_to_rays / cast_ray_batch) for an explicit
        pixel batch (two int arrays of one shape) or for rect = (x0, y0, width, height), as a Rays of cuda tensors
        with the batch shape of the pixels ([h, w, .] for a rectangle).  pix_jitter = (dx, dy): the sub-pixel offsets
        the reference draws when jitter > 0 (camera_utils.py:943-957), float32 arrays of the pixels' shape."""
        torch = self._torch
        cam = rc_camera()
        p2c = np.asarray(camera.pixtocam, np.float32).reshape(9)
        c2w = np.asarray(camera.camtoworld, np.float32).reshape(12)
        light = c2w.reshape(3, 4)[:, 3] if camera.light is None else np.asarray(camera.light, np.float32).reshape(3)
        for dst, src in ((cam.pixtocam, p2c), (cam.camtoworld, c2w), (cam.light, light)):
            for i, v in enumerate(src):
                dst[i] = float(v)
        cam.near, cam.far = float(camera.near), float(camera.far)
        _camera_options(cam, getattr(camera, "camtype", "perspective"), getattr(camera, "distortion_params", None),
                        getattr(camera, "pixtocam_ndc", None), getattr(camera, "z_range", None))
        dev = f"cuda:{self.device}"
        if rect is not None:
            x0, y0, w, hgt = (int(v) for v in rect)
            shape, n, px, py = (hgt, w), w * hgt, None, None
        else:
            px = self._dev(np.ascontiguousarray(pix_x_int), torch.int32)
            py = self._dev(np.ascontiguousarray(pix_y_int), torch.int32)
            if px.shape != py.shape:
                raise ValueError("pix_x_int and pix_y_int must have the same shape")
            shape, n, x0, y0, w, hgt = tuple(px.shape), px.numel(), 0, 0, 0, 0
        jit = self._pix_jitter(pix_jitter, n)
        if jit is not None:
            cam.pix_dx, cam.pix_dy = jit[0].data_ptr(), jit[1].data_ptr()
        out = rc_cast_outputs()
        t = self._cast_tensors(shape, out)
        self._check(self.lib.rc_cast_rays(self._h, C.byref(cam), _ptr(px), _ptr(py), n, x0, y0, w, hgt, C.byref(out),
                                          self._stream()))
        self._keep = [px, py, jit]
        zi = torch.zeros(shape + (1,), dtype=torch.int32, device=dev)
        return _rays_of_cast(t, torch.ones(shape + (1,), dtype=torch.float32, device=dev), zi, zi)

    def camera_set(self, pixtocams, camtoworlds, lights=None, near: float = 0.0, far: float = 0.0, camtype="perspective",
                   distortion_params=None, pixtocam_ndc=None, z_range=None):
        """The reference's `cameras` tuple uploaded once: -> CameraSet for cast_rays_multi / train_batch.  pixtocams
        [C, 3, 3] (or one [3, 3] for all), camtoworlds [C, 3, 4] (or [C, 4, 4]), lights [C, 3] or None (the camera centres);
        the other arguments as in cast_rays' camera."""
        return CameraSet(self, pixtocams, camtoworlds, lights, near, far, camtype, distortion_params, pixtocam_ndc, z_range)

    def cast_rays_multi(self, cameras: "CameraSet", cam_idx, pix_x_int, pix_y_int, pix_jitter=None):
        """rc_cast_rays_multi: the rays of pixels (pix_x_int, pix_y_int) of cameras cam_idx (three int arrays of one shape;
        cuda int32 tensors are used where they are) in ONE launch, as a Rays of cuda tensors with the pixels' batch
        shape; every field is bitwise what cast_rays yields per camera.  cam_idx must lie in [0, cameras.count): the
        kernel only clamps it for memory safety.  lossmult is 1, cam_idx is carried over, light_idx is 0."""
        torch = self._torch
        as_i32 = lambda a: self._dev(a if isinstance(a, torch.Tensor) else np.ascontiguousarray(a), torch.int32)
        ci, px, py = as_i32(cam_idx), as_i32(pix_x_int), as_i32(pix_y_int)
        if not (ci.shape == px.shape == py.shape):
            raise ValueError("cam_idx, pix_x_int and pix_y_int must have the same shape")
        shape, n = tuple(px.shape), px.numel()
        jit = self._pix_jitter(pix_jitter, n) or [None, None]
        out = rc_cast_outputs()
        t = self._cast_tensors(shape, out)
        self._check(self.lib.rc_cast_rays_multi(self._h, C.byref(cameras.struct), _ptr(ci), _ptr(px), _ptr(py), n,
                                                _ptr(jit[0]), _ptr(jit[1]), C.byref(out), self._stream()))
        self._keep = [ci, px, py, jit, cameras]
        ones = torch.ones(shape + (1,), dtype=torch.float32, device=px.device)
        return _rays_of_cast(t, ones, ci.reshape(shape + (1,)), torch.zeros_like(ci).reshape(shape + (1,)))

    def train_batch(self, cameras: "CameraSet", images, key, n: int, patch_size: int = 1, border: int = 0,
                    batching: str = "all_images", cam_lossmult=None, pix_jitter=None):
        """rc_train_batch: the batch of one train step from a PRNG key in ONE launch.  images: cuda tensor [C, H, W, 3],
        float32 or uint8 (read as u / 255); cam_lossmult: cuda float32 [C] or None; key: uint32[2].  -> (Rays of
        [n, .] cuda tensors with lossmult, cam_idx, pix_x_int, pix_y_int filled in, rgb [n, 3]).  The index rule is
        data.patch_indices, this package's own."""
        from . import prng
        torch = self._torch
        if batching not in BATCHING:
            raise ValueError(f"unknown batching {batching!r}")
        if not isinstance(images, torch.Tensor) or not images.is_cuda or not images.is_contiguous() or images.dim() != 4 \
                or images.shape[-1] != 3 or images.dtype not in (torch.float32, torch.uint8):
            raise ValueError("images must be a contiguous cuda tensor [C, H, W, 3] of float32 or uint8")
        if images.shape[0] != cameras.count:
            raise ValueError(f"{images.shape[0]} images for {cameras.count} cameras")
        n = int(n)
        dev = f"cuda:{self.device}"
        k = (C.c_uint32 * 2)(*[int(v) for v in prng.as_key(key)])
        cs = cameras.struct
        jit = self._pix_jitter(pix_jitter, n, per="ray")
        if jit is not None:
            cs = rc_camera_set.from_buffer_copy(cs)
            cs.pix_dx, cs.pix_dy = jit[0].data_ptr(), jit[1].data_ptr()
        lm = None if cam_lossmult is None else self._dev(cam_lossmult).reshape(-1)
        if lm is not None and lm.numel() != cameras.count:
            raise ValueError("cam_lossmult: one value per camera")
        out = rc_train_batch_outputs()
        t = self._cast_tensors((max(n, 0),), out.rays)
        rgb = torch.empty((max(n, 0), 3), dtype=torch.float32, device=dev)
        lossmult = torch.empty((max(n, 0), 1), dtype=torch.float32, device=dev)
        idx = torch.empty((3, max(n, 0), 1), dtype=torch.int32, device=dev)
        out.rgb, out.lossmult = rgb.data_ptr(), lossmult.data_ptr()
        out.cam_idx, out.pix_x, out.pix_y = idx[0].data_ptr(), idx[1].data_ptr(), idx[2].data_ptr()
        self._check(self.lib.rc_train_batch(self._h, C.byref(cs), images.data_ptr(),
                                            RC_IMAGE_U8 if images.dtype == torch.uint8 else RC_IMAGE_F32, int(images.shape[1]),
                                            int(images.shape[2]), _ptr(lm), k, int(patch_size), int(border),
                                            BATCHING[batching], n, C.byref(out), self._stream()))
        self._keep = [jit, lm, cameras, images]
        return _rays_of_cast(t, lossmult, idx[0], torch.zeros_like(idx[0]), idx[1], idx[2]), rgb

    # -- time-resolved cache ------------------------------------------------------------------------
    def render_transient(self, rays: Dict[str, object], randoms: Optional[Dict[str, object]] = None,
                         outputs: Optional[Iterable[str]] = None):
        """Time-resolved cache (rc_render_transient).  rays needs `lights` and `cam_origins` besides the usual
        fields; randoms: {"jitter": [u0, u1, u2], "shadow_jitter": [v0, v1, v2]} or None (shadow_jitter: per-level jitter of
        the n * 32 shadow rays when the config has use_occlusions).  Returns dict name -> cuda tensor: [n, n_bins, 3] for the
        histograms, [n, 3] / [n] otherwise."""
        r, held, n = self._rays_struct(rays)
        cam = self._dev(rays["cam_origins"]).reshape(-1, 3)
        held["cam_origins"] = cam
        rnd_p, shadow_p = None, None                   # shadow_jitter: [3][n * 32], use_occlusions only
        if randoms is not None and randoms.get("jitter") is not None:
            rnd_p = C.byref(self._randoms(held, randoms["jitter"]))
        if randoms is not None and randoms.get("shadow_jitter") is not None:
            shadow_p = C.byref(self._randoms(held, randoms["shadow_jitter"], tag="shadow_"))
        names = [nm for nm, _ in TRANSIENT_OUTPUTS] if outputs is None else list(outputs)
        nb = self.cfg.transient.n_bins

        def tshape(nm):
            kind = TRANSIENT_OUTPUTS[TRANSIENT_OUTPUT_ID[nm]][1]
            return (n, nb, 3) if kind == "bins" else ((n, 3) if kind == 3 else (n,))

        res, cout = self._outputs(TRANSIENT_OUTPUTS, names, tshape)
        self._check(self.lib.rc_render_transient(self._h, C.byref(r), cam.data_ptr(), n, rnd_p, shadow_p, C.byref(cout),
                                                 self._stream()))
        self._keep = [held]
        return res

    def render_transient_slices(self, rays: Dict[str, object], randoms: Optional[Dict[str, object]], times,
                                outputs: Iterable[str] = ("rgb",), extra: Optional[Iterable[str]] = None):
        """rc_render_transient_slices: the time slices  w * v[ceil t] + (1 - w) * v[floor t],  w = t - floor t,  of the
        histograms render_transient would give for the same rays / randoms, without the histograms.
        times: fractional bin indices in [0, n_bins - 1]; outputs: of TRANSIENT_SLICE_OUTPUTS ("rgb", the filtered
        "direct" part, the "indirect" part); extra: of TRANSIENT_SLICE_EXTRAS, the outputs of the steady-state composite.
        Returns {output: [n, len(times), 3] cuda tensor} plus the extras ([n, 3] / [n]).  A call serves RC_TSLICE_MAX times;
        more are served by several calls, and EACH CALL REPEATS THE TRACE up to the per-bin heads -- ask for the times of
        a view together."""
        torch = self._torch
        times = [float(t) for t in np.asarray(times, dtype=np.float64).reshape(-1)]
        outputs, extra = list(outputs), list(extra or ())
        bad = [k for k in outputs if k not in TRANSIENT_SLICE_OUTPUTS] + [k for k in extra if k not in TRANSIENT_SLICE_EXTRAS]
        if bad or not outputs:
            raise ValueError(f"render_transient_slices: outputs of {TRANSIENT_SLICE_OUTPUTS} (at least one), extra of "
                             f"{TRANSIENT_SLICE_EXTRAS}; got {bad or outputs}")
        if not times:
            raise ValueError("render_transient_slices: no times")
        r, held, n = self._rays_struct(rays)
        cam = self._dev(rays["cam_origins"]).reshape(-1, 3)
        held["cam_origins"] = cam
        rnd_p, shadow_p = None, None
        if randoms is not None and randoms.get("jitter") is not None:
            rnd_p = C.byref(self._randoms(held, randoms["jitter"]))
        if randoms is not None and randoms.get("shadow_jitter") is not None:
            shadow_p = C.byref(self._randoms(held, randoms["shadow_jitter"], tag="shadow_"))
        xres, xout = self._outputs(TRANSIENT_OUTPUTS, extra,
                                   lambda nm: (n, 3) if TRANSIENT_OUTPUTS[TRANSIENT_OUTPUT_ID[nm]][1] == 3 else (n,))
        res = {}
        groups = [times[i: i + RC_TSLICE_MAX] for i in range(0, len(times), RC_TSLICE_MAX)]
        for gi, group in enumerate(groups):
            bufs = dict(zip(outputs, self._zeros_like_many([(n, len(group), 3)] * len(outputs))))
            s = rc_transient_slices(count=len(group))
            for i, t in enumerate(group):
                s.t[i] = t
            for k in outputs:
                setattr(s, k, bufs[k].data_ptr())
            if n > 0:                      # (an empty tensor has no address to hand over, and there is nothing to write)
                self._check(self.lib.rc_render_transient_slices(self._h, C.byref(r), cam.data_ptr(), n, rnd_p, shadow_p,
                                                                C.byref(s), C.byref(xout) if extra and gi == 0 else None,
                                                                self._stream()))
            for k in outputs:
                res.setdefault(k, []).append(bufs[k])
        self._keep = [held]
        out = {k: v[0] if len(v) == 1 else torch.cat(v, dim=1) for k, v in res.items()}
        out.update(xres)
        return out

    def transient_head_grad_layout(self):
        """rc_transient_head_grad_layout: [(tensor name, offset, shape)] of the time-resolved cache's per-bin head layers
        (params/Cache/Shader/transient_indirect_layer, .../SurfaceLightField/output_rgba_layer), and its size in floats."""
        return self._grad_layout("transient_heads")

    def _transient_data_args(self, rays, randoms, gt, rgb_nocorr, gt_nocorr, lossmult, cfg):
        """What transient_data_backward and transient_data_backward_sampler hand to their exports: (cfg, whether it is the
        default reading, rc_rays, the tensors kept alive, n, cam_origins, rc_randoms or None, lossmult, the three histogram
        pointers)."""
        from .config import TransientDataLossConfig

        cfg = TransientDataLossConfig() if cfg is None else cfg
        if (cfg.loss_type not in TRANSIENT_LOSS_TYPES or tuple(cfg.transient_gauss_sigma_scales) or cfg.mask_lossmult
                or cfg.clip_eval):
            raise NotImplementedError(f"transient data loss: loss_type is one of {TRANSIENT_LOSS_TYPES}, with the constant gauss "
                                      "row only (no sigma scales), without mask_lossmult and clip_eval")
        plain = cfg.loss_type == TRANSIENT_LOSS_TYPES[0] and not cfg.use_itof
        r, held, n = self._rays_struct(rays)
        cam = self._dev(rays["cam_origins"]).reshape(-1, 3)
        held["cam_origins"] = cam
        rnd_p = None if randoms is None else self._jitter_struct(randoms.get("jitter"), held, n)
        lm = self._lossmult(lossmult, held, n)
        # without a time-resolved config there is no n_bins to check against: the call itself refuses such a handle
        count = None if self.cfg.transient is None else n * self.cfg.transient.n_bins * 3

        def hist(x, what):
            if x is None:
                return None
            t = self._dev(x).reshape(-1)
            if count is not None and t.numel() != count:
                raise ValueError(f"{what} must hold [n, n_bins, 3] values")
            held[what] = t
            return t.data_ptr()

        gt_p, rn_p, gn_p = hist(gt, "gt"), hist(rgb_nocorr, "rgb_nocorr"), hist(gt_nocorr, "gt_nocorr")
        if gt_p is None:
            raise ValueError("gt is required")
        return cfg, plain, r, held, n, cam, rnd_p, lm, gt_p, rn_p, gn_p

    def transient_data_backward(self, rays: Dict[str, object], randoms: Optional[Dict[str, object]], gt, rgb_nocorr=None,
                                gt_nocorr=None, lossmult=None, cfg=None, grad=None, stream_handle=None):
        """rc_transient_data_backward / rc_transient_data_backward_kind: render_transient with the same rays (lights and
        cam_origins included) / randoms ({"jitter": [u0, u1, u2]} or None), the time-resolved data loss against gt
        ([n, n_bins, 3]) with the constants of cfg (config.TransientDataLossConfig; config.transient_data_loss_preset names
        the gins' readings) and its gradient w.r.t. the two per-bin head layers (transient_head_grad_layout; DESIGN.md
        §4.15).  cfg.loss_type is one of TRANSIENT_LOSS_TYPES; cfg.use_itof and cfg.itof_frequency_phase_shifts
        ((frequency, phase) pairs, at most RC_ITOF_MAX_PAIRS) as the reference's Config.  The default reading goes through
        the first export, every other one through the second.  rgb_nocorr / gt_nocorr: [n, n_bins, 3] or None (this render,
        gt).  grad: flat buffer to accumulate into (allocated zeroed when None); grad=False leaves the heads' gradient out
        (the loss and the "td:" adjoints are still computed).  Returns (grad flat or None, losses [2] cuda tensor: loss,
        mse)."""
        cfg, plain, r, held, n, cam, rnd_p, lm, gt_p, rn_p, gn_p = self._transient_data_args(rays, randoms, gt, rgb_nocorr,
                                                                                             gt_nocorr, lossmult, cfg)
        c = transient_data_loss_c(cfg)
        flat, losses, stream = self._loss_prologue("transient_heads", grad, stream_handle, slots=2)
        if plain:
            self._check(self.lib.rc_transient_data_backward(self._h, C.byref(r), cam.data_ptr(), n, rnd_p, gt_p, rn_p, gn_p,
                                                            _ptr(lm), C.byref(c), _ptr(flat), losses.data_ptr(), stream))
        else:
            ck = transient_data_loss_kind_c(cfg)
            self._check(self.lib.rc_transient_data_backward_kind(self._h, C.byref(r), cam.data_ptr(), n, rnd_p, gt_p, rn_p,
                                                                 gn_p, _ptr(lm), C.byref(ck), _ptr(flat), losses.data_ptr(),
                                                                 stream))
        self._keep = [held]
        return flat, losses

    # -- the time-resolved cache's density fields and proposal samplers -----------------
    def transient_sampler_grad_layout(self):
        """rc_transient_sampler_grad_layout: [(tensor name, offset, shape)] of the time-resolved cache's sampler side in one
        buffer (density_grad_layout(0), (1), (2) in turn, then MLP_<last>/pred_normals_layer), and its size in floats."""
        return self._grad_layout("transient_sampler")

    def transient_data_backward_sampler(self, rays: Dict[str, object], randoms: Optional[Dict[str, object]], gt, rgb_nocorr=None,
                                        gt_nocorr=None, lossmult=None, cfg=None, grad=None, sampler_grad=None,
                                        stream_handle=None):
        """rc_transient_data_backward_sampler: transient_data_backward (same arguments, same losses, adjoints and head
        gradient, bitwise) plus the data loss's gradient of MLP_<last> through the compositing weights -- the weights path
        only, see DESIGN.md §4.15b -- accumulated into sampler_grad (transient_sampler_grad_layout; allocated zeroed when
        None; False: left out, nothing beyond transient_data_backward runs).  "td:d_density" holds d loss / d density.
        Returns (head flat or None, sampler flat or None, losses [2])."""
        cfg, _, r, held, n, cam, rnd_p, lm, gt_p, rn_p, gn_p = self._transient_data_args(rays, randoms, gt, rgb_nocorr,
                                                                                         gt_nocorr, lossmult, cfg)
        ck = transient_data_loss_kind_c(cfg)
        flat, losses, stream = self._loss_prologue("transient_heads", grad, stream_handle, slots=2)
        sflat = None if sampler_grad is False else self._grad_buffer(sampler_grad, self._grad_size("transient_sampler"),
                                                                     "sampler_grad")
        self._check(self.lib.rc_transient_data_backward_sampler(self._h, C.byref(r), cam.data_ptr(), n, rnd_p, gt_p, rn_p, gn_p,
                                                                _ptr(lm), C.byref(ck), _ptr(flat), _ptr(sflat),
                                                                losses.data_ptr(), stream))
        self._keep = [held]
        return flat, sflat, losses

    def transient_interlevel_backward(self, rays: Dict[str, object], jitters=None, anneal: float = 0.4, mults=(0.01, 0.01),
                                      blurs=(0.03, 0.003), lossmult=None, grad=None):
        """rc_transient_interlevel_backward: interlevel_backward on a time-resolved handle (its own sampler's forward).
        grad: the flat buffer of transient_sampler_grad_layout to accumulate into (allocated zeroed when None; False: the
        losses only).  Returns (sampler flat or None, losses [num_levels - 1] cuda tensor)."""
        return self._interlevel(True, rays, jitters, anneal, mults, blurs, lossmult, grad)

    def transient_geometry_backward(self, rays: Dict[str, object], jitters=None, anneal: float = 0.4, lossmult=None, terms=None,
                                    grad=None):
        """rc_transient_geometry_backward: geometry_backward on a time-resolved handle; the density gradient goes to the
        last level's segments of the sampler flat, pred_normals_layer's to its tail.  terms as geometry_backward (the
        distortion curve defaults to the gins' -0.25 / 1e4).  grad as transient_interlevel_backward.
        Returns (sampler flat or None, losses [4] cuda tensor)."""
        return self._geometry(True, rays, jitters, anneal, lossmult, terms, grad)

    def transient_mask_backward(self, rays: Dict[str, object], jitters=None, anneal: float = 0.4, masks=None, lossmult=None,
                                terms=None, grad=None):
        """rc_transient_mask_backward: mask_backward on a time-resolved handle (rays of backward_mask_rays included); the
        gradient goes to the last level's segments of the sampler flat.  grad as transient_interlevel_backward.
        Returns (sampler flat or None, loss [1] cuda tensor)."""
        return self._mask(True, rays, jitters, anneal, masks, lossmult, terms, grad)

    def transient_density_regularizer(self, level: int, mult: float, grad=None):
        """rc_transient_density_regularizer: density_regularizer of grid `level` on a time-resolved handle, the gradient
        into that level's table segments of the sampler flat.  Returns (sampler flat or None, loss [1] cuda tensor)."""
        return self._regularizer(self.lib.rc_transient_density_regularizer, "transient_sampler", (int(level), float(mult)), grad)

    def dtof_to_itof(self, x, pairs, stream_handle=None):
        """rc_dtof_to_itof (render_utils.dtof_to_itof): x [n, n_bins, 3] histograms (a cuda tensor is used where it is) ->
        cuda tensor [n, 2 P + 1, 3]: per (frequency, phase) pair of `pairs` the cos row and the sin row, then the constant
        row (half the bin sum: the steady-state image), with the handle's exposure_time."""
        torch = self._torch
        pairs = _itof_pairs(pairs)
        t = self._dev(x)
        if self.cfg.transient is not None and (t.dim() != 3 or tuple(t.shape[1:]) != (self.cfg.transient.n_bins, 3)):
            raise ValueError("x must be [n, n_bins, 3]")
        t = t.contiguous()
        n, P = int(t.shape[0]), len(pairs)
        out = torch.empty((n, 2 * P + 1, 3), dtype=torch.float32, device=t.device)
        f = (C.c_double * max(P, 1))(*[p[0] for p in pairs])
        ph = (C.c_double * max(P, 1))(*[p[1] for p in pairs])
        stream = self._stream(stream_handle)
        self._check(self.lib.rc_dtof_to_itof(self._h, t.data_ptr(), n, P, f, ph, out.data_ptr(), stream))
        self._keep = [t]
        return out

    # -- evaluation of a rendered view ------------------------------------------------------------------
    def eval_image(self, pred, gt, mask=None, acc=None, normals=None, normals_gt=None, distance_mean=None,
                   distance_median=None, depth_gt=None, exposure: float = 1.0, img_scale: float = 1.0,
                   clip_eval: bool = False, skip_postprocess: bool = False, shape=None, keep_images: bool = False, ssim_map: bool = False,
                   stream_handle=None, sync: bool = True):
        """rc_eval_image: the reference trainer's per-view metrics of a rendered image against its
        ground truth, on the device.  pred, gt: [H, W, 3] images or [H, W, n_bins, 3] histograms (cuda tensors are used
        where they are, numpy arrays are uploaded); mask, acc, distance_mean, distance_median, depth_gt: [H, W] (a
        trailing 1 is accepted) or None; normals, normals_gt: [H, W, 3] or None.  shape: (H, W) or (H, W, n_bins) where
        it cannot be read off pred / gt.  Returns {"mse", "psnr", "ssim", "transient_iou", "l1_mean", "l1_median",
        "mae"} as floats (skip_postprocess: pred and gt are compared as they are, MetricHarness' call; NaN where the inputs of a slot were not given) after ONE copy of the result array to the host;
        with sync=False the array stays on the device under "result" (float64 [RC_EVAL_COUNT] in EVAL_SLOTS' order) and
        nothing waits.  keep_images adds "post_pred" / "post_gt" ([H, W, 3] cuda tensors, the post-processed images),
        ssim_map "ssim_map" ([H - 10, W - 10, 3])."""
        torch = self._torch
        held = {k: None if v is None else self._dev(v) for k, v in
                zip(_EVAL_INPUTS, (pred, gt, mask, acc, normals, normals_gt, distance_mean, distance_median, depth_gt))}
        if shape is None:
            lead = held["pred"] if held["pred"] is not None else held["gt"]
            if lead is None or lead.dim() not in (3, 4) or lead.shape[-1] != 3:
                raise ValueError("pred / gt must be [H, W, 3] or [H, W, n_bins, 3] (or give shape)")
            shape = tuple(lead.shape[:-1])
        H, W = int(shape[0]), int(shape[1])
        nb = int(shape[2]) if len(shape) > 2 else 0
        widths = {"pred": 3 * max(nb, 1), "gt": 3 * max(nb, 1), "normals": 3, "normals_gt": 3}
        im = rc_eval_images(height=H, width=W, n_bins=nb, exposure=float(exposure), img_scale=float(img_scale),
                            clip_eval=int(bool(clip_eval)), skip_postprocess=int(bool(skip_postprocess)))
        for k, t in held.items():
            if t is None:
                continue
            if t.numel() != H * W * widths.get(k, 1):
                raise ValueError(f"{k} holds {t.numel()} values, expected {H * W * widths.get(k, 1)}")
            setattr(im, k, t.data_ptr())
        dev = f"cuda:{self.device}"
        res = {}
        if H >= 11 and W >= 11:                        # smaller images are refused by the call itself
            if keep_images:
                res["post_pred"] = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
                res["post_gt"] = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
                im.post_pred, im.post_gt = res["post_pred"].data_ptr(), res["post_gt"].data_ptr()
            if ssim_map:
                res["ssim_map"] = torch.empty((H - 10, W - 10, 3), dtype=torch.float32, device=dev)
                im.ssim_map = res["ssim_map"].data_ptr()
        out = torch.empty(RC_EVAL_COUNT, dtype=torch.float64, device=dev)
        self._check(self.lib.rc_eval_image(self._h, C.byref(im), out.data_ptr(), self._stream(stream_handle)))
        self._keep = [held]
        if not sync:
            res["result"] = out
            return res
        if stream_handle is not None:                  # a foreign stream: torch's copy below is not ordered behind it
            torch.cuda.synchronize(self.device)
        res.update(zip(EVAL_SLOTS, out.cpu().tolist()))                 # the one device-to-host copy
        return res

    def eval_shift_invariant(self, pred, gt, search_radii=(4, 4), window_halfwidth: int = 8, ssim: bool = True,
                             keep_maps: bool = False, stream_handle=None, sync: bool = True):
        """rc_eval_shift_invariant: image_utils.shift_invariant_mse / shift_invariant_ssim of two
        post-processed [H, W, 3] images, compared as they are (cuda tensors are used where they are, numpy arrays are
        uploaded); pred is the image that is shifted.  Returns {"mse", "psnr", "ssim"} as floats ("ssim" is NaN with
        ssim=False) after ONE copy of the result array to the host; with sync=False the array stays on the device under
        "result" (float64 [RC_EVAL_SI_COUNT] in EVAL_SI_SLOTS' order) and nothing waits.  keep_maps adds "mse_map"
        (float32 [H, W], the chosen shifts' unpooled metric), "mse_di" and "mse_dj" (int32 [H, W], the chosen shifts), and
        with ssim the three "ssim_" ones."""
        torch = self._torch
        ri, rj = search_radii_pair(search_radii)
        if int(window_halfwidth) != window_halfwidth:
            raise ValueError(f"window_halfwidth must be an integer, not {window_halfwidth!r}")
        held = {"pred": self._dev(pred), "gt": self._dev(gt)}
        lead = held["pred"]
        if lead.dim() != 3 or lead.shape[-1] != 3:
            raise ValueError("pred / gt must be [H, W, 3]")
        if held["gt"].shape != lead.shape:
            raise ValueError(f"gt is {tuple(held['gt'].shape)}, pred {tuple(lead.shape)}")
        H, W = int(lead.shape[0]), int(lead.shape[1])
        im = rc_eval_si_images(pred=lead.data_ptr(), gt=held["gt"].data_ptr(), height=H, width=W, radius_i=ri, radius_j=rj,
                               window_halfwidth=int(window_halfwidth), want_ssim=int(bool(ssim)))
        dev = f"cuda:{self.device}"
        res = {}
        if keep_maps:
            for k in _EVAL_SI_MAPS:
                if ssim or not k.startswith("ssim"):
                    res[k] = torch.empty((H, W), dtype=torch.float32 if k.endswith("map") else torch.int32, device=dev)
                    setattr(im, k, res[k].data_ptr())
        out = torch.empty(RC_EVAL_SI_COUNT, dtype=torch.float64, device=dev)
        self._check(self.lib.rc_eval_shift_invariant(self._h, C.byref(im), out.data_ptr(), self._stream(stream_handle)))
        self._keep = [held]
        if not sync:
            res["result"] = out
            return res
        if stream_handle is not None:                  # a foreign stream: torch's copy below is not ordered behind it
            torch.cuda.synchronize(self.device)
        res.update(zip(EVAL_SI_SLOTS, out.cpu().tolist()))              # the one device-to-host copy
        return res

    # -- evaluation of the albedo ------------------------------------------------------------------------
    def eval_albedo(self, albedo, acc, albedo_gt, mask=None, ratio=None, albedo_clip: float = 1.0, pairs=None,
                    keep_images: bool = False, shape=None, stream_handle=None, sync: bool = True):
        """rc_eval_albedo: the reference trainer's albedo metric of one view, on the device.  albedo,
        albedo_gt: [H, W, 3]; acc, mask: [H, W] (a trailing 1 is accepted; cuda tensors are used where they are, numpy
        arrays are uploaded); shape: (H, W) where it cannot be read off albedo.  ratio: 3 floats (tensor or array) that
        are applied, or None: this view's own per-channel median.  pairs: an AlbedoPairs to which the view's valid rows
        are appended.  Returns {"mse", "psnr", "ratio" (3 floats), "valid"} after ONE copy of the result array to the
        host; with sync=False the array stays on the device under "result" (float64 [RC_ALBEDO_COUNT] in ALBEDO_SLOTS'
        order) and nothing waits.  keep_images adds "post_pred" / "post_gt" (the gamma-corrected images) and "ratio_im",
        [H, W, 3] cuda tensors."""
        torch = self._torch
        held = {k: None if v is None else self._dev(v) for k, v in
                (("albedo", albedo), ("acc", acc), ("albedo_gt", albedo_gt), ("mask", mask), ("ratio", ratio))}
        if shape is None:
            lead = held["albedo"] if held["albedo"] is not None else held["albedo_gt"]
            if lead is None or lead.dim() != 3 or lead.shape[-1] != 3:
                raise ValueError("albedo / albedo_gt must be [H, W, 3] (or give shape)")
            shape = tuple(lead.shape[:-1])
        H, W = int(shape[0]), int(shape[1])
        im = rc_albedo_images(height=H, width=W, albedo_clip=float(albedo_clip))
        for k, t in held.items():
            if t is None:
                continue
            want = 3 if k == "ratio" else H * W * (3 if k in ("albedo", "albedo_gt") else 1)
            if t.numel() != want:
                raise ValueError(f"{k} holds {t.numel()} values, expected {want}")
            setattr(im, k, t.data_ptr())
        if pairs is not None:
            im.pairs, im.pairs_capacity, im.pairs_count = pairs.buffer.data_ptr(), pairs.capacity, pairs.count.data_ptr()
        dev = f"cuda:{self.device}"
        res = {}
        if keep_images and H >= 1 and W >= 1:
            for k in ("post_pred", "post_gt", "ratio_im"):
                res[k] = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
                setattr(im, k, res[k].data_ptr())
        out = torch.empty(RC_ALBEDO_COUNT, dtype=torch.float64, device=dev)
        self._check(self.lib.rc_eval_albedo(self._h, C.byref(im), out.data_ptr(), self._stream(stream_handle)))
        self._keep = [held, pairs]
        if not sync:
            res["result"] = out
            return res
        if stream_handle is not None:                  # a foreign stream: torch's copy below is not ordered behind it
            torch.cuda.synchronize(self.device)
        v = out.cpu().tolist()                         # the one device-to-host copy
        res.update(mse=v[0], psnr=v[1], ratio=v[2:5], valid=int(v[5]))
        return res

    def albedo_ratio(self, pairs, use_median: bool = False, gamma: bool = True, stream_handle=None):
        """rc_albedo_ratio: the ratio of the reference's _compute_albedo_ratio over the rows of an AlbedoPairs -- the
        exact per-channel median, or the least squares (with or without the 1/2.2 gamma).  Returns a [1, 3] cuda tensor,
        NaN when the pairs overflowed their buffer or hold no row; nothing is read back."""
        torch = self._torch
        out = torch.empty((1, 3), dtype=torch.float32, device=f"cuda:{self.device}")
        self._check(self.lib.rc_albedo_ratio(self._h, pairs.buffer.data_ptr(), pairs.capacity, pairs.count.data_ptr(),
                                             int(bool(use_median)), int(bool(gamma)), out.data_ptr(),
                                             self._stream(stream_handle)))
        self._keep = [pairs]
        return out

    # -- visualisation of a rendered view ------------------------------------------------------------------
    def weighted_percentile(self, value, weight=None, ps=(0.5, 99.5), stream_handle=None):
        """rc_weighted_percentile: the reference's vis.weighted_percentile of all values of `value`
        with the weights `weight` (None: all ones), read in float64 with a stable sort.  ps: at most 8 percentiles.
        Returns a float64 cuda tensor [len(ps)]; nothing is read back.  A negative, NaN or infinite weight gives NaN."""
        torch = self._torch
        held = [self._dev(value), None if weight is None else self._dev(weight)]
        n = held[0].numel()
        if held[1] is not None and held[1].numel() != n:
            raise ValueError(f"weight holds {held[1].numel()} values, expected {n}")
        ps = [float(p) for p in ps]
        arr = (C.c_double * max(len(ps), 1))(*ps)
        out = torch.empty(len(ps), dtype=torch.float64, device=f"cuda:{self.device}")
        ptr = lambda x: None if x is None else x.data_ptr()
        self._check(self.lib.rc_weighted_percentile(self._h, ptr(held[0]), ptr(held[1]), n, arr, len(ps),
                                                    out.data_ptr(), self._stream(stream_handle)))
        self._keep = [held]
        return out

    def image_max(self, src, stream_handle=None):
        """rc_image_max: np.max over every value of `src` as a float32 cuda tensor [1] (a NaN is handed on); nothing is
        read back."""
        src = self._dev(src)
        out = self._torch.empty(1, dtype=self._torch.float32, device=f"cuda:{self.device}")
        self._check(self.lib.rc_image_max(self._h, src.data_ptr(), src.numel(), out.data_ptr(), self._stream(stream_handle)))
        self._keep = [src]
        return out

    def vis_images(self, items, height: int, width: int, stream_handle=None):
        """rc_vis_images: the pictures of one [height, width] view in one call.  items: dicts with "src" ([H, W, c] or, for
        the bin-summing operations, [H, W, n_bins, c]; c = 1 may be left out) and "op" (a name of VIS_OPS), and optionally
        n_bins, channels (default: read off src), scale, divide, offset, exponent, divisor (cuda float tensor [1]), acc,
        mask ([H, W]), bounds / auto_bounds (cuda float64 tensors [2]), nan_to_num, and f32 / u8 (which outputs to write;
        default u8 only).  Returns one dict per item with "f32" and / or "u8": [H, W, 3] cuda tensors."""
        torch = self._torch
        H, W = int(height), int(width)
        n_pix = H * W
        dev = f"cuda:{self.device}"
        table = (rc_vis_item * max(len(items), 1))()
        held, res = [], []
        for c_item, it in zip(table, items):
            unknown = set(it) - {"src", "op", "n_bins", "channels", "scale", "divide", "offset", "exponent", "divisor",
                                 "acc", "mask", "bounds", "auto_bounds", "nan_to_num", "f32", "u8"}
            if unknown:
                raise ValueError(f"vis_images: unknown item fields {sorted(unknown)}")
            src = self._dev(it["src"])
            n_bins = int(it.get("n_bins", 0))
            per_pixel = src.numel() // max(n_pix * max(n_bins, 1), 1)
            channels = int(it.get("channels", per_pixel))
            if n_pix < 1 or src.numel() != n_pix * max(n_bins, 1) * channels:
                raise ValueError(f"vis_images: src holds {src.numel()} values, expected {n_pix} x {max(n_bins, 1)} x {channels}")
            c_item.src, c_item.channels, c_item.n_bins = src.data_ptr(), channels, n_bins
            c_item.op, c_item.nan_to_num = VIS_OP_ID[it["op"]], int(bool(it.get("nan_to_num", False)))
            c_item.scale, c_item.divide = float(it.get("scale", 1.0)), float(it.get("divide", 1.0))
            c_item.offset, c_item.exponent = float(it.get("offset", 0.0)), float(it.get("exponent", 1.0))
            keep = [src]
            for k, dtype, want in (("divisor", torch.float32, 1), ("acc", torch.float32, n_pix), ("mask", torch.float32, n_pix),
                                   ("bounds", torch.float64, 2), ("auto_bounds", torch.float64, 2)):
                if it.get(k) is None:
                    continue
                t = self._dev(it[k], dtype)
                if t.numel() != want:
                    raise ValueError(f"vis_images: {k} holds {t.numel()} values, expected {want}")
                setattr(c_item, k, t.data_ptr())
                keep.append(t)
            out = {}
            if it.get("f32", False):
                out["f32"] = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
                c_item.out_f32 = out["f32"].data_ptr()
            if it.get("u8", not it.get("f32", False)):
                out["u8"] = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
                c_item.out_u8 = out["u8"].data_ptr()
            held.append(keep)
            res.append(out)
        self._check(self.lib.rc_vis_images(self._h, table, len(items), H, W, self._stream(stream_handle)))
        self._keep = [held]
        return res

    # -- the probe of a surface point ---------------------------------------------------
    def probe_rays(self, view, pixels, height: int, width: int, near: float, far: float, normal_offset: float = 0.4,
                   flip: bool = False, stream_handle=None):
        """rc_probe_rays: the [height, width] panoramas of secondary rays cast from the hit points of rows `pixels` (host
        integers, at most RC_PROBE_MAX) of `view`: a dict of "origins", "directions", "normals" ([n_view, 3]) and
        "distance_median" ([n_view]), and optionally "lights", "imageplane", "look", "up", whose row 0 every ray takes (a
        missing one keeps the panoramic cast's own value).  cuda tensors are used where they are.  Returns (Rays of
        [P, height, width, .] cuda tensors, positions [P, 3]); cam_origins and the vcam_* fields are None (only the
        time-resolved cache reads them)."""
        torch = self._torch
        from .rays import Rays
        pix = np.ascontiguousarray(np.asarray(pixels).reshape(-1), dtype=np.int64)
        P, H, W = int(pix.size), int(height), int(width)
        v, held = rc_probe_view(), {}
        for k in _PROBE_VIEW_REQUIRED:
            t = held[k] = self._dev(view[k]).reshape(-1) if k == "distance_median" else self._dev(view[k]).reshape(-1, 3)
            setattr(v, k, t.data_ptr())
        v.n_view = n_view = held["origins"].shape[0]
        for k in _PROBE_VIEW_REQUIRED:
            if held[k].shape[0] != n_view:
                raise ValueError(f"probe_rays: view[{k!r}] has {held[k].shape[0]} rows, expected {n_view}")
        for k, width_k in _PROBE_VIEW_BROADCAST:
            if view.get(k) is not None:
                t = held[k] = self._dev(view[k]).reshape(-1, width_k)
                if t.shape[0] < 1:
                    raise ValueError(f"probe_rays: view[{k!r}] is empty")
                setattr(v, k, t.data_ptr())
        if not (1 <= P <= RC_PROBE_MAX and H >= 1 and W >= 1 and P * H * W < 2 ** 31):
            raise ValueError(f"probe_rays: {P} probes of {H} x {W} rays (1..{RC_PROBE_MAX} probes, below 2^31 rays in all)")
        out = rc_cast_outputs()
        t = self._cast_tensors((P, H, W), out)
        dev = f"cuda:{self.device}"
        positions = torch.empty((P, 3), dtype=torch.float32, device=dev)
        self._check(self.lib.rc_probe_rays(self._h, C.byref(v), pix.ctypes.data_as(C.c_void_p), P, H, W, float(near), float(far),
                                           float(normal_offset), int(bool(flip)), C.byref(out), positions.data_ptr(),
                                           self._stream(stream_handle)))
        self._keep = [held]
        zi = torch.zeros((P, H, W, 1), dtype=torch.int32, device=dev)
        rays = Rays(origins=t["origins"], lights=t["lights"], directions=t["directions"], viewdirs=t["viewdirs"],
                    radii=t["radii"], imageplane=t["imageplane"], look=t["look"], up=t["up"], cam_origins=None,
                    vcam_look=None, vcam_up=None, vcam_origins=None,
                    lossmult=torch.ones((P, H, W, 1), dtype=torch.float32, device=dev), near=t["near"], far=t["far"],
                    cam_idx=zi, light_idx=zi)
        return rays, positions

    def vmf_panorama(self, means, kappas, logits, height: int, width: int, flip: bool = False, linear: bool = False,
                     srgb: bool = True, u8: bool = False, stream_handle=None):
        """rc_vmf_panorama: the reference's render_vmf of P mixtures over the [height, width] panorama.  means [P, V, 3]
        (raw: they are normalised with max(|m|, 1e-5)), kappas [P, V], logits [P, V] (a single mixture may leave P out).
        Returns the requested of "linear" ([P, H, W] float32, the mixture's density), "srgb" ([P, H, W, 3] float32) and "u8"
        ([P, H, W, 3] uint8, save_img_u8's form of "srgb") as cuda tensors."""
        torch = self._torch
        m, k, l = self._dev(means), self._dev(kappas), self._dev(logits)
        if m.dim() == 2:
            m, k, l = m[None], k[None], l[None]
        if m.dim() != 3 or m.shape[-1] != 3 or tuple(k.shape) != tuple(m.shape[:2]) or tuple(l.shape) != tuple(m.shape[:2]):
            raise ValueError(f"vmf_panorama: means {tuple(m.shape)}, kappas {tuple(k.shape)}, logits {tuple(l.shape)}: "
                             "expected [P, V, 3], [P, V], [P, V]")
        P, V, H, W = int(m.shape[0]), int(m.shape[1]), int(height), int(width)
        if not (1 <= P <= RC_PROBE_MAX and 1 <= V <= RC_PROBE_MAX_LOBES and H >= 1 and W >= 1 and P * H * W < 2 ** 31):
            raise ValueError(f"vmf_panorama: {P} mixtures of {V} lobes over {H} x {W} pixels (1..{RC_PROBE_MAX} mixtures, "
                             f"1..{RC_PROBE_MAX_LOBES} lobes, below 2^31 pixels in all)")
        if not (linear or srgb or u8):
            raise ValueError("vmf_panorama: no output requested")
        dev = f"cuda:{self.device}"
        res = {}
        if linear:
            res["linear"] = torch.empty((P, H, W), dtype=torch.float32, device=dev)
        if srgb:
            res["srgb"] = torch.empty((P, H, W, 3), dtype=torch.float32, device=dev)
        if u8:
            res["u8"] = torch.empty((P, H, W, 3), dtype=torch.uint8, device=dev)
        self._check(self.lib.rc_vmf_panorama(self._h, m.data_ptr(), k.data_ptr(), l.data_ptr(), P, V, H, W, int(bool(flip)),
                                             _ptr(res.get("linear")), _ptr(res.get("srgb")), _ptr(res.get("u8")),
                                             self._stream(stream_handle)))
        self._keep = [m, k, l]
        return res

    def workspace_tensor(self, name: str, count: int = None):
        """The first `count` floats (default: all) of an internal buffer of the last call as a cuda tensor: a copy made on
        torch's current stream, behind the call that filled the buffer; nothing waits and nothing reaches the host."""
        torch = self._torch
        ptr, cnt = C.c_void_p(), C.c_int64()
        self._check(self.lib.rc_workspace_ptr(self._h, name.encode(), C.byref(ptr), C.byref(cnt)))
        count = cnt.value if count is None else int(count)
        if not 0 <= count <= cnt.value:
            raise ValueError(f"workspace {name!r} holds {cnt.value} floats, {count} were asked for")
        out = torch.empty(count, dtype=torch.float32, device=f"cuda:{self.device}")
        if count:
            _memcpy_d2d_async(out.data_ptr(), ptr.value, count * 4, self._stream())
        return out

    # -- material stage -------------------------------------------------------------------------------
    def material_grad_layout(self):
        """rc_material_grad_layout: [(tensor name, offset, shape)] of the MaterialShader gradient buffer (the material_grid
        tables, then bottleneck_layer, pred_brdf_layer), and its size in floats."""
        return self._grad_layout("material")

    def envmap_grad_layout(self):
        """rc_envmap_grad_layout: [(tensor name, offset, shape)] of the model-level EnvMap's gradient buffer
        (params/Cache/EnvMap: layer_0, layer_1, layer_2, layer_bottleneck, output_rgba_layer), and its size in floats."""
        return self._grad_layout("envmap")

    def _shading_randoms(self, randoms, held):
        """The rc_randoms / rc_material_randoms of material_smoothness_backward: the primary pass's jitter and the shading
        point's pick (gumbel or resample_inds) of render_material's randoms; the sampler members stay NULL."""
        rnd = self._randoms(held, randoms.get("jitter"))
        mr = held["mrnd"] = rc_material_randoms()
        if randoms.get("resample_inds") is not None:
            held["m_inds"] = self._dev(randoms["resample_inds"], self._torch.int32).reshape(-1)
            mr.resample_inds = held["m_inds"].data_ptr()
        elif randoms.get("gumbel") is not None:
            held["m_gumbel"] = self._dev(randoms["gumbel"])
            mr.gumbel = held["m_gumbel"].data_ptr()
        return rnd, mr

    def material_smoothness_backward(self, rays: Dict[str, object], randoms: Dict[str, object], noise, lossmult=None,
                                     mult: float = 1.0, weight_albedo: float = 1e-4, weight_other: float = 1e-4,
                                     noise_scale: float = 0.01, tensoir_albedo: bool = True, grad=None,
                                     stream_handle=None):
        """rc_material_smoothness_backward: render_material's primary pass and shading point with the same rays /
        randoms (jitter, gumbel or resample_inds), the material_smoothness loss at x and x' = x + noise_scale * noise
        (noise: [n, 3], N(0, 1)) and its gradient w.r.t. the MaterialShader parameters (material_grad_layout).  grad: flat
        buffer to accumulate into (allocated zeroed when None); grad=False computes the loss only.
        Returns (grad flat or None, loss [1] cuda tensor)."""
        r, held, n = self._rays_struct(rays)
        rnd, mr = self._shading_randoms(randoms, held)
        lm = self._lossmult(lossmult, held, n)
        nz = self._dev(noise).reshape(-1)
        if nz.numel() != 3 * n:
            raise ValueError("noise must hold [n, 3] values")
        held["ms_noise"] = nz
        cfg = rc_material_smoothness_loss(mult=float(mult), weight_albedo=float(weight_albedo),
                                          weight_other=float(weight_other), noise=float(noise_scale),
                                          tensoir_albedo=int(bool(tensoir_albedo)))
        flat, loss, stream = self._loss_prologue("material", grad, stream_handle)
        self._check(self.lib.rc_material_smoothness_backward(self._h, C.byref(r), _ptr(lm), n, C.byref(rnd), C.byref(mr),
                                                             nz.data_ptr(), C.byref(cfg), _ptr(flat), loss.data_ptr(),
                                                             stream))
        self._keep = [held]
        return flat, loss

    def material_regularizer(self, mult: float, grad=None):
        """rc_material_regularizer: mult * sum over the material grid's tables of 0.5 * mean(x^2) (param_regularizer_loss,
        'material_grid', the ease factor folded into mult).  grad: flat buffer of material_grad_layout to accumulate
        mult * x / numel into (allocated zeroed when None); grad=False computes the loss only.
        Returns (grad flat or None, loss [1] cuda tensor)."""
        return self._regularizer(self.lib.rc_material_regularizer, "material", (float(mult),), grad)

    def material_data_backward(self, rays: Dict[str, object], randoms: Dict[str, object], gt_rgb,
                               num_secondary_samples: int = None, lossmult=None, cfg=None, grad=None, stream_handle=None,
                               env_grad=None, env_scale: float = 1.0):
        """rc_material_data_backward: render_material with the same rays / randoms / num_secondary_samples, the material
        stage's data loss against gt_rgb ([n, 3]) with the constants of cfg (config.MaterialDataLossConfig) and its
        gradient w.r.t. the MaterialShader parameters (material_grad_layout; the Trainer.stopgrad = True reading,
        DESIGN.md §4.12).  grad: flat buffer to accumulate into (allocated zeroed when None); grad=False computes the
        loss only.  Returns (grad flat or None, loss [1] cuda tensor).
        env_grad: None leaves everything above as it is.  True, or a flat buffer of envmap_grad_layout to
        accumulate into, makes the call rc_material_data_backward_env: the same loss and MaterialShader gradient, and the
        gradient w.r.t. the params/Cache/EnvMap tensors times env_scale (MaterialMLP.stopgrad_env_map_weight[1]).
        Returns (grad flat or None, EnvMap grad flat, loss)."""
        from .config import MaterialDataLossConfig

        cfg = MaterialDataLossConfig() if cfg is None else cfg
        K = num_secondary_samples or self.cfg.num_secondary_samples
        r, held, n = self._rays_struct(rays)
        rnd, mr = self._material_randoms(randoms, n, K, held)
        lm = self._lossmult(lossmult, held, n)
        gt = self._dev(gt_rgb).reshape(-1)
        if gt.numel() != 3 * n:
            raise ValueError("gt_rgb must hold [n, 3] values")
        held["md_gt"] = gt
        c = rc_material_data_loss(mult=float(cfg.data_loss_mult), weight=float(cfg.weight), exponent=float(cfg.exponent),
                                  eps=float(cfg.eps), clip_val=float(cfg.clip_val), thresh=float(cfg.loss_thresh),
                                  use_gt_rawnerf=int(bool(cfg.use_gt_rawnerf)),
                                  use_combined_rawnerf=int(bool(cfg.use_combined_rawnerf)),
                                  use_norm_rawnerf=int(bool(cfg.use_norm_rawnerf)))
        flat, loss, stream = self._loss_prologue("material", grad, stream_handle)
        head = (self._h, C.byref(r), gt.data_ptr(), _ptr(lm), n, C.byref(rnd), C.byref(mr), K, C.byref(c))
        if env_grad is None or env_grad is False:
            env = None
            self._check(self.lib.rc_material_data_backward(*head, _ptr(flat), loss.data_ptr(), stream))
        else:
            env = self._grad_buffer(None if env_grad is True else env_grad, self._grad_size("envmap"), "env_grad")
            self._check(self.lib.rc_material_data_backward_env(*head, float(env_scale), _ptr(flat), env.data_ptr(),
                                                               loss.data_ptr(), stream))
        self._keep = [held]
        return (flat, loss) if env is None else (flat, env, loss)

    def _material_randoms(self, randoms, n, K, held, own_samplers=True):
        """The rc_randoms / rc_material_randoms of render_material and light_sampling_backward (device copies kept in
        `held`).  own_samplers=False (render_relight's "env" mode): the BRDF and vMF members stay NULL."""
        torch = self._torch
        rnd = self._randoms(held, randoms.get("jitter"))
        mr = held["mrnd"] = rc_material_randoms()
        for k in ("gumbel", "vmf_noise", "spec_u1", "spec_u2", "cos_u1", "cos_u2", "vmf_v", "vmf_tmp"):
            if k == "gumbel" and randoms.get(k) is None:
                continue                      # the primary pick is handed over as resample_inds
            if k != "gumbel" and not own_samplers:
                continue
            held["m_" + k] = self._dev(randoms[k])
            setattr(mr, k, held["m_" + k].data_ptr())
        if own_samplers and randoms.get("vmf_lobe") is not None:
            held["m_lobe"] = self._dev(randoms["vmf_lobe"], torch.int32).reshape(-1)
            mr.vmf_lobe = held["m_lobe"].data_ptr()
        elif own_samplers:                    # the lobe is drawn on the device: argmax(logits + Gumbel noise)
            held["m_lobe_g"] = self._dev(randoms["vmf_lobe_gumbel"]).reshape(n, -1)
            mr.vmf_lobe_gumbel = held["m_lobe_g"].data_ptr()
        # secondary trace randoms: [specular block | diffuse block]
        # (a caller that keeps them in the ABI's layout passes sec_jitter[3] [n*K] / sec_gumbel [n*K, S] and skips the copies)
        for l in range(RC_MAX_LEVELS):
            if randoms.get("sec_jitter") is not None:
                held[f"sj{l}"] = self._dev(randoms["sec_jitter"][l]).reshape(-1)
                if held[f"sj{l}"].numel() != n * K:
                    raise ValueError(f"sec_jitter[{l}]: expected {n * K} values")
            else:
                held[f"sj{l}"] = torch.cat([self._dev(randoms["spec_jitter"][l]).reshape(-1),
                                            self._dev(randoms["diff_jitter"][l]).reshape(-1)])
            mr.sec_jitter[l] = held[f"sj{l}"].data_ptr()
        if randoms.get("sec_gumbel") is not None:
            held["sg"] = self._dev(randoms["sec_gumbel"])
            if held["sg"].shape[0] != n * K:
                raise ValueError(f"sec_gumbel: expected {n * K} rows")
            mr.sec_gumbel = held["sg"].data_ptr()
        elif randoms.get("spec_gumbel") is not None and randoms.get("diff_gumbel") is not None:
            held["sg"] = torch.cat([self._dev(randoms["spec_gumbel"]), self._dev(randoms["diff_gumbel"])], dim=0).contiguous()
            mr.sec_gumbel = held["sg"].data_ptr()
        # explicit categorical picks (filtered_sampler_inds) instead of the Gumbel draws
        if randoms.get("resample_inds") is not None:
            held["m_inds"] = self._dev(randoms["resample_inds"], torch.int32).reshape(-1)
            mr.resample_inds = held["m_inds"].data_ptr()
        if randoms.get("spec_resample_inds") is not None and randoms.get("diff_resample_inds") is not None:
            held["s_inds"] = torch.cat([self._dev(randoms["spec_resample_inds"], torch.int32).reshape(-1),
                                        self._dev(randoms["diff_resample_inds"], torch.int32).reshape(-1)])
            mr.sec_resample_inds = held["s_inds"].data_ptr()
        return rnd, mr

    def render_material(self, rays: Dict[str, object], randoms: Dict[str, object], num_secondary_samples: int = None):
        """Material stage (rc_render_material).  randoms: dict with the keys of
        oracle-compatible `draw_randoms` (jitter[3], gumbel, vmf_noise, spec_u1/u2, cos_u1/u2, vmf_lobe, vmf_v,
        vmf_tmp, spec_jitter[3], spec_gumbel, diff_jitter[3], diff_gumbel) and optionally the categorical picks
        themselves (resample_inds [n]; spec_resample_inds [n*Ks] + diff_resample_inds [n*Kd]), which replace the draws.
        Returns (cache_outputs, material_outputs) as dicts of cuda tensors."""
        K = num_secondary_samples or self.cfg.num_secondary_samples
        r, held, n = self._rays_struct(rays)
        rnd, mr = self._material_randoms(randoms, n, K, held)
        c_names = [nm for nm, _ in OUTPUTS if nm not in ("env_map_rgb", "rgb_no_env")]
        m_names = [nm for nm, _ in MAT_OUTPUTS]
        cshape = lambda nm: (n, 3) if OUTPUTS[OUTPUT_ID[nm]][1] == 3 else (n,)
        mshape = lambda nm: (n, 3) if MAT_OUTPUTS[MAT_OUTPUT_ID[nm]][1] == 3 else (n,)
        # both tables' outputs in ONE zero-filled allocation
        bufs = self._zeros_like_many([cshape(nm) for nm in c_names] + [mshape(nm) for nm in m_names])
        cres, cout = self._outputs(OUTPUTS, c_names, cshape, dict(zip(c_names, bufs)))
        mres, mout = self._outputs(MAT_OUTPUTS, m_names, mshape, dict(zip(m_names, bufs[len(c_names):])))
        self._check(self.lib.rc_render_material(self._h, C.byref(r), n, C.byref(rnd), C.byref(mr), K, C.byref(cout),
                                                C.byref(mout), self._stream()))
        self._keep = [held]
        return cres, mres

    # -- relighting under an explicit environment image (include/rc_abi.h) ---------------
    def set_env_image(self, rgb, pmf=None, pdf=None, dirs=None):
        """rc_set_env_image: bind rgb [H, W, 3] and, optionally, its tables pmf / pdf [H W] and dirs [H W, 3] (all three or
        none); the handle keeps copies of its own.  rgb=None unbinds."""
        if rgb is None:
            self._check(self.lib.rc_set_env_image(self._h, None, None, None, None, 0, 0, self._stream()))
            return
        img = self._dev(rgb)
        if img.dim() != 3 or img.shape[2] != 3:
            raise ValueError("rgb must be [H, W, 3]")
        H, W = int(img.shape[0]), int(img.shape[1])
        tabs = [None if t is None else self._dev(t).reshape(-1) for t in (pmf, pdf, dirs)]
        for t, cnt, nm in zip(tabs, (H * W, H * W, 3 * H * W), ("pmf", "pdf", "dirs")):
            if t is not None and t.numel() != cnt:
                raise ValueError(f"{nm}: expected {cnt} values")
        self._check(self.lib.rc_set_env_image(self._h, img.data_ptr(), _ptr(tabs[0]), _ptr(tabs[1]), _ptr(tabs[2]), H, W,
                                              self._stream()))
        self._keep = [img, tabs]

    def env_tables(self, rgb, scale: float = 1.0):
        """rc_env_tables: (pmf [H W], pdf [H W], dirs [H W, 3]) of rgb * scale as float32 cuda tensors."""
        torch = self._torch
        img = self._dev(rgb)
        if img.dim() != 3 or img.shape[2] != 3:
            raise ValueError("rgb must be [H, W, 3]")
        H, W = int(img.shape[0]), int(img.shape[1])
        dev = f"cuda:{self.device}"
        pmf, pdf = (torch.empty(H * W, dtype=torch.float32, device=dev) for _ in range(2))
        dirs = torch.empty((H * W, 3), dtype=torch.float32, device=dev)
        self._check(self.lib.rc_env_tables(self._h, img.data_ptr(), H, W, float(scale), pmf.data_ptr(), pdf.data_ptr(),
                                           dirs.data_ptr(), self._stream()))
        self._keep = [img]
        return pmf, pdf, dirs

    def env_lookup(self, viewdirs):
        """rc_env_lookup: the bound image's colour [n, 3] at directions [n, 3]."""
        d = self._dev(viewdirs).reshape(-1, 3)
        out = self._torch.empty_like(d)
        self._check(self.lib.rc_env_lookup(self._h, d.data_ptr(), d.shape[0], out.data_ptr(), self._stream()))
        self._keep = [d]
        return out

    def env_pick(self, key, T: int):
        """rc_env_pick: jax.random.categorical(key, safe_log(pmf), axis=-2, shape=(1, T, 1)) over the bound pmf as an
        int32 cuda tensor [T]."""
        from . import prng
        k = (C.c_uint32 * 2)(*[int(v) for v in prng.as_key(key)])
        out = self._torch.empty(int(T), dtype=self._torch.int32, device=f"cuda:{self.device}")
        self._check(self.lib.rc_env_pick(self._h, k, int(T), out.data_ptr(), self._stream()))
        return out

    def render_relight(self, rays: Dict[str, object], randoms: Dict[str, object], mode: str = "brdf", picks_spec=None,
                       picks_diff=None, albedo_ratio=None, num_secondary_samples: int = None):
        """rc_render_relight: render_material under the bound image.  mode "brdf": the stage's own samplers, the image in
        place of the EnvMap; "env": the environment sampler on the texel picks picks_spec [T_spec] / picks_diff [T_diff]
        (int32), whose sampler tensors may be missing from `randoms`.  albedo_ratio: three floats or None.  Returns
        (cache_outputs, material_outputs) as render_material does."""
        torch = self._torch
        if mode not in ("brdf", "env"):
            raise ValueError(f"unknown relight mode {mode!r}")
        K = num_secondary_samples or self.cfg.num_secondary_samples
        r, held, n = self._rays_struct(rays)
        rnd, mr = self._material_randoms(randoms, n, K, held, own_samplers=mode == "brdf")
        a = held["rl_args"] = rc_relight_args()
        a.mode = RC_RELIGHT_ENV if mode == "env" else RC_RELIGHT_BRDF
        if mode == "env":
            if picks_spec is None or picks_diff is None:
                raise ValueError("mode 'env' needs picks_spec and picks_diff")
            ps = held["rl_ps"] = self._dev(picks_spec, torch.int32).reshape(-1)
            pd = held["rl_pd"] = self._dev(picks_diff, torch.int32).reshape(-1)
            a.picks_spec, a.picks_diff, a.T_spec, a.T_diff = ps.data_ptr(), pd.data_ptr(), ps.numel(), pd.numel()
        if albedo_ratio is not None:
            ar = held["rl_ratio"] = self._dev(albedo_ratio).reshape(-1)
            if ar.numel() != 3:
                raise ValueError("albedo_ratio must hold three values")
            a.albedo_ratio = ar.data_ptr()
        c_names = [nm for nm, _ in OUTPUTS if nm not in ("env_map_rgb", "rgb_no_env")]
        m_names = [nm for nm, _ in MAT_OUTPUTS]
        cshape = lambda nm: (n, 3) if OUTPUTS[OUTPUT_ID[nm]][1] == 3 else (n,)
        mshape = lambda nm: (n, 3) if MAT_OUTPUTS[MAT_OUTPUT_ID[nm]][1] == 3 else (n,)
        bufs = self._zeros_like_many([cshape(nm) for nm in c_names] + [mshape(nm) for nm in m_names])
        cres, cout = self._outputs(OUTPUTS, c_names, cshape, dict(zip(c_names, bufs)))
        mres, mout = self._outputs(MAT_OUTPUTS, m_names, mshape, dict(zip(m_names, bufs[len(c_names):])))
        self._check(self.lib.rc_render_relight(self._h, C.byref(r), n, C.byref(rnd), C.byref(mr), K, C.byref(a),
                                               C.byref(cout), C.byref(mout), self._stream()))
        self._keep = [held]
        return cres, mres

    def allgather_outputs(self, nccl_comm: int, local: Dict[str, object], world: int):
        """rc_allgather_outputs: gather this rank's outputs (dict name -> [n, .] cuda tensor, as render_rays returns) over
        an RCCL communicator the caller owns (ncclComm_t as an integer address).  Returns name -> [world * n, .]."""
        torch = self._torch
        lo, fu, res = rc_outputs(), rc_outputs(), {}
        n = None
        for nm, t in local.items():
            n = t.shape[0] if n is None else n
            if t.shape[0] != n or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"output {nm}: expected contiguous float32 cuda tensors with one row count")
            res[nm] = torch.empty((world * n,) + tuple(t.shape[1:]), dtype=torch.float32, device=t.device)
            lo.ptr[OUTPUT_ID[nm]] = t.data_ptr()
            fu.ptr[OUTPUT_ID[nm]] = res[nm].data_ptr()
        self._check(self.lib.rc_allgather_outputs(self._h, C.c_void_p(nccl_comm), C.byref(lo), n, C.byref(fu), self._stream()))
        self._keep = [local]
        return res

    # -- single operators ---------------------------------------------------------------------
    def cfg_grid(self, grid_id: int):
        """GridConfig of grid 0-2 (proposal density grids), 3 (appearance), 4 (material), 5 (light)."""
        return (list(self.cfg.proposal_grids) + [self.cfg.appearance_grid, self.cfg.material_grid, self.cfg.light_grid])[grid_id]

    def hashgrid_lookup(self, grid_id: int, points, apply_contraction: bool = True):
        torch = self._torch
        g = self.cfg_grid(grid_id)
        p = self._dev(points).reshape(-1, 3)
        out = torch.empty((p.shape[0], g.out_dim), dtype=torch.float32, device=p.device)
        self._check(self.lib.rc_hashgrid_lookup(self._h, grid_id, p.data_ptr(), p.shape[0], out.data_ptr(),
                                                int(apply_contraction), self._stream()))
        self._keep = [p]
        return out

    # -- surface export (mesh.py) ---------------------------------------------------------------
    QUERY_OUTPUTS = (("density", 1), ("normals_pred", 3), ("normals", 3), ("material", 5))

    def query_points(self, points, outputs=("density",), level=None):
        """rc_query_points: the handle's fields at points [n, 3] (world coordinates) -> {name: cuda tensor} for the names
        of `outputs` among "density" [n] (sampler level `level`, None: the last), "normals_pred" [n, 3], "normals" [n, 3]
        (the analytic normals; both of the last level, unrectified) and "material" [n, 5] (albedo rgb, roughness,
        metalness)."""
        torch = self._torch
        widths = dict(self.QUERY_OUTPUTS)
        unknown = [k for k in outputs if k not in widths]
        if unknown:
            raise ValueError(f"query_points: unknown outputs {unknown}")
        p = self._dev(points).reshape(-1, 3)
        n = p.shape[0]
        out = {k: torch.empty((n,) if widths[k] == 1 else (n, widths[k]), dtype=torch.float32, device=p.device) for k in outputs}
        self._check(self.lib.rc_query_points(self._h, p.data_ptr(), n, -1 if level is None else int(level),
                                             *[_ptr(out.get(k)) for k, _ in self.QUERY_OUTPUTS], self._stream()))
        self._keep = [p]
        return out

    def density_lattice(self, lo, hi, dims, level=None):
        """rc_density_lattice: the density of sampler level `level` (None: the last), nan_to_num applied, on the
        [nx, ny, nz] lattice whose axis a has point i at lo[a] + float32(i) * ((hi[a] - lo[a]) / float32(n_a - 1))."""
        torch = self._torch
        nx, ny, nz = (int(d) for d in dims)
        field = torch.empty((max(nx, 0), max(ny, 0), max(nz, 0)), dtype=torch.float32, device=f"cuda:{self.device}")
        self._check(self.lib.rc_density_lattice(self._h, (C.c_float * 3)(*[float(v) for v in lo]),
                                                (C.c_float * 3)(*[float(v) for v in hi]), nx, ny, nz,
                                                -1 if level is None else int(level), field.data_ptr(), self._stream()))
        return field

    def isosurface_into(self, field, iso, lo, hi, vertices, normals, triangles, counts):
        """rc_isosurface, one call: field [nx, ny, nz] float32 cuda; vertices / normals [cap_v, 3] float32, triangles
        [cap_t, 3] int32 (None: capacity 0; normals may be None on its own); counts: int64 [2] cuda, always written."""
        nx, ny, nz = (int(d) for d in field.shape)
        self._check(self.lib.rc_isosurface(self._h, field.data_ptr(), nx, ny, nz, float(iso),
                                           (C.c_float * 3)(*[float(v) for v in lo]), (C.c_float * 3)(*[float(v) for v in hi]),
                                           _ptr(vertices), _ptr(normals), 0 if vertices is None else vertices.shape[0],
                                           _ptr(triangles), 0 if triangles is None else triangles.shape[0],
                                           counts.data_ptr(), self._stream()))
        self._keep = [field]

    def isosurface(self, field, iso, lo, hi, normals=True):
        """The two passes of rc_isosurface on a [nx, ny, nz] lattice (any float32 cuda tensor in rc_density_lattice's
        layout): count, read {V, T} (the one host synchronisation), allocate, extract ->
        (vertices [V, 3], normals [V, 3] or None, triangles [T, 3] int32)."""
        torch = self._torch
        field = self._dev(field)
        if field.dim() != 3:
            raise ValueError("isosurface: field must be [nx, ny, nz]")
        dev = field.device
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        self.isosurface_into(field, iso, lo, hi, None, None, None, counts)
        V, T = (int(c) for c in counts.tolist())
        vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
        vnormals = torch.empty((V, 3), dtype=torch.float32, device=dev) if normals else None
        triangles = torch.empty((T, 3), dtype=torch.int32, device=dev)
        if V > 0:
            self.isosurface_into(field, iso, lo, hi, vertices, vnormals, triangles, counts)
        return vertices, vnormals, triangles

    # -- textured export (mesh.py) ----------------------------------------------------------------
    def query_cache_diffuse(self, points):
        """rc_query_cache_diffuse: [n, 6] = ambient_diffuse rgb, indirect_diffuse rgb of the cache's shader at points
        [n, 3] -- its two heads that need no view direction."""
        torch = self._torch
        p = self._dev(points).reshape(-1, 3)
        out = torch.empty((p.shape[0], 6), dtype=torch.float32, device=p.device)
        self._check(self.lib.rc_query_cache_diffuse(self._h, p.data_ptr(), p.shape[0], out.data_ptr(), self._stream()))
        self._keep = [p]
        return out

    def _mesh_arrays(self, vertices, triangles):
        torch = self._torch
        v = self._dev(vertices).reshape(-1, 3)
        t = self._dev(triangles, torch.int32).reshape(-1, 3)
        return v, t

    def atlas_uvs(self, T: int, r: int):
        """rc_atlas_uvs: the normalised uv of every triangle corner, [T, 3, 2] float32."""
        torch = self._torch
        atlas_layout(T, r)                               # refuses before anything is allocated
        uvs = torch.empty((int(T), 3, 2), dtype=torch.float32, device=f"cuda:{self.device}")
        self._check(self.lib.rc_atlas_uvs(self._h, int(T), int(r), uvs.data_ptr(), self._stream()))
        return uvs

    def atlas_points(self, vertices, triangles, r: int, first: int = 0, count: Optional[int] = None):
        """rc_atlas_points: (points [count, 3] float32, owner [count] int32) of the texels with linear index y W + x in
        first .. first + count - 1 (count None: to the end of the atlas)."""
        torch = self._torch
        v, t = self._mesh_arrays(vertices, triangles)
        W, H = atlas_layout(t.shape[0], r)[2:]
        count = W * H - int(first) if count is None else int(count)
        points = torch.empty((max(count, 0), 3), dtype=torch.float32, device=v.device)
        owner = torch.empty((max(count, 0),), dtype=torch.int32, device=v.device)
        self._check(self.lib.rc_atlas_points(self._h, v.data_ptr(), v.shape[0], t.data_ptr(), t.shape[0], int(r), int(first),
                                             count, points.data_ptr(), owner.data_ptr(), self._stream()))
        self._keep = [v, t]
        return points, owner

    def bake_atlas(self, vertices, triangles, r: int, outputs=("material",), level=None):
        """rc_bake_atlas: the planes named in `outputs` (ATLAS_OUTPUTS) of the atlas of a mesh -> {name: [H, W] or
        [H, W, channels] cuda tensor}, float32 but for "coverage" (uint8)."""
        torch = self._torch
        widths = dict(ATLAS_OUTPUTS)
        unknown = [k for k in outputs if k not in widths]
        if unknown:
            raise ValueError(f"bake_atlas: unknown outputs {unknown}")
        v, t = self._mesh_arrays(vertices, triangles)
        W, H = atlas_layout(t.shape[0], r)[2:]
        out, a = {}, rc_atlas_outputs()
        for k in outputs:
            out[k] = torch.empty((H, W) if widths[k] == 1 else (H, W, widths[k]), device=v.device,
                                 dtype=torch.uint8 if k == "coverage" else torch.float32)
            setattr(a, k, out[k].data_ptr())
        self._check(self.lib.rc_bake_atlas(self._h, v.data_ptr(), v.shape[0], t.data_ptr(), t.shape[0], int(r),
                                           -1 if level is None else int(level), C.byref(a), self._stream()))
        self._keep = [v, t]
        return out

    def sample_intervals(self, t, logits, num_samples: int, jitter=None):
        torch = self._torch
        t = self._dev(t)
        logits = self._dev(logits)
        n, P = logits.shape
        out = torch.empty((n, num_samples + 1), dtype=torch.float32, device=t.device)
        j = None if jitter is None else self._dev(jitter).reshape(-1)
        self._check(self.lib.rc_sample_intervals(self._h, t.data_ptr(), logits.data_ptr(), n, P, num_samples, _ptr(j),
                                                 out.data_ptr(), self._stream()))
        self._keep = [t, logits, j]
        return out

    # -- introspection ------------------------------------------------------------------------
    def workspace(self, name: str, dtype=None):
        """Copy of an internal buffer of the last render (tests / debugging)."""
        torch = self._torch
        ptr, cnt = C.c_void_p(), C.c_int64()
        self._check(self.lib.rc_workspace_ptr(self._h, name.encode(), C.byref(ptr), C.byref(cnt)))
        torch.cuda.synchronize(self.device)
        host = np.empty(cnt.value, dtype=np.float32)
        _memcpy_d2h(host.ctypes.data, ptr.value, cnt.value * 4)
        return host.view(np.int32) if dtype == np.int32 else host

    def set_profiling(self, enabled):
        self._check(self.lib.rc_set_profiling(self._h, int(enabled)))

    def set_graph_mode(self, mode: int):
        """0 eager launches, 1 capture a hipGraph when a call repeats (default), 2 capture at once."""
        self._check(self.lib.rc_set_graph_mode(self._h, int(mode)))

    def set_fused(self, on: bool):
        """Plain cache pass: True (default) one fused launch per batch with every intermediate on chip,
        False one launch per stage (fills the workspace that `workspace()` shows)."""
        self._check(self.lib.rc_set_fused(self._h, int(on) if not isinstance(on, bool) else (1 if on else 0)))

    def stage_times_ms(self) -> Dict[str, float]:
        n = self.lib.rc_stage_count()
        arr = (C.c_float * n)()
        self._check(self.lib.rc_stage_times_ms(self._h, arr, n))
        return {self.lib.rc_stage_name(i).decode(): float(arr[i]) for i in range(n)}


class AlbedoPairs:
    """The pair rows rc_eval_albedo appends to and rc_albedo_ratio reads: `buffer` [capacity, 6] float32 (gt'[3], p[3]
    per valid pixel) and `count`, the device int64 row count that only the kernels read and advance.  It may pass the
    capacity: rows behind the buffer are counted, never stored."""

    def __init__(self, rc: "RadianceCache", capacity: int, fill=None):
        torch = rc._torch
        dev = f"cuda:{rc.device}"
        self.capacity = int(capacity)
        self.buffer = torch.empty((self.capacity, 6), dtype=torch.float32, device=dev)
        if fill is not None:
            self.buffer.fill_(fill)
        self.count = torch.zeros(1, dtype=torch.int64, device=dev)

    def rows(self):
        """(rows stored [min(count, capacity), 6] as numpy, count): a readback, for tests."""
        n = int(self.count.item())
        return self.buffer[: max(0, min(n, self.capacity))].cpu().numpy(), n


def material_randoms_plan(key, n: int, K: int, diffuse_fraction: float, num_vmf: int, level_samples, flags: int = 0,
                          loss_key=None, capacity: int = RC_PRNG_MAX_SEGMENTS):
    """rc_material_randoms_plan (needs no GPU and no handle): the segment table of one material-stage forward's random
    tensors -> (ctypes array of rc_prng_segment, number of rows, arena size in 32-bit words)."""
    from . import prng

    k = (C.c_uint32 * 2)(*[int(v) for v in prng.as_key(key)])
    lk = None if loss_key is None else (C.c_uint32 * 2)(*[int(v) for v in prng.as_key(loss_key)])
    levels = (C.c_int32 * len(level_samples))(*[int(v) for v in level_samples])
    segs = (rc_prng_segment * max(1, int(capacity)))()
    count, words = C.c_int32(0), C.c_int64(0)
    rc = load_library().rc_material_randoms_plan(k, lk, int(n), int(K), float(diffuse_fraction), int(num_vmf), levels,
                                                 len(level_samples), int(flags), segs, int(capacity), C.byref(count),
                                                 C.byref(words))
    if rc != 0:
        raise RcError(rc, f"rc_material_randoms_plan(n={n}, K={K}): refused (rounded sample counts, sizes or capacity)")
    return segs, count.value, words.value


def vis_turbo_lut():
    """rc_vis_turbo_lut: the [256, 3] float32 colour table of RC_VIS_TURBO (matplotlib's "turbo")."""
    out = np.empty((256, 3), np.float32)
    rc = load_library().rc_vis_turbo_lut(out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RcError(rc, "rc_vis_turbo_lut")
    return out


def atlas_layout(T: int, r: int):
    """rc_atlas_layout: (cols, rows, W, H) of the per-triangle atlas of T triangles with cells of r x r texels
    (include/rc_abi.h states the rule); RcError where the library refuses (T < 1, r outside 4 .. 64, a side above 16384)."""
    dims = (C.c_int32 * 4)()
    rc = load_library().rc_atlas_layout(int(T), int(r), dims)
    if rc != 0:
        raise RcError(rc, f"rc_atlas_layout: T = {T}, r = {r} is outside the supported range")
    return tuple(int(d) for d in dims)


def _memcpy_d2h(dst: int, src: int, nbytes: int):
    """hipMemcpy device->host through the HIP runtime torch already loaded."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    rc = hip.hipMemcpy(dst, src, nbytes, 2)  # hipMemcpyDeviceToHost
    if rc != 0:
        raise RuntimeError(f"hipMemcpy failed: {rc}")


def _memcpy_d2d_async(dst: int, src: int, nbytes: int, stream):
    """hipMemcpyAsync device->device on `stream` through the HIP runtime torch already loaded."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    rc = hip.hipMemcpyAsync(dst, src, nbytes, 3, stream)  # hipMemcpyDeviceToDevice
    if rc != 0:
        raise RuntimeError(f"hipMemcpyAsync failed: {rc}")
