"""Restatement of the cache stage's mask loss and of the rays of its backward term, from the reference's source
(test helper, not a test module).

  mask_loss            train_utils.compute_mask_loss (internal/train_utils.py:785-836) in torch, dtype-generic: both weight
                       branches (:821-832) and the decay / ease schedules (:839-932) as train_utils applies them.
  schedule_ease_in /   train_utils.compute_weight_ease_in (:839-867) / compute_weight_decay (:870-894).
  schedule_decay
  backward_rays        numpy, dtype-generic: _compute_backward_mask_loss's call of render_utils.get_secondary_rays
                       (train_utils.py:3348-3401, render_utils.py:927-1056) for its fixed arguments: one sample of
                       UniformHemisphereSampler (render_utils.py:395-403) in get_rotation_matrix(-look) (:145-168),
                       local_to_global, origins = means + normals * normal_eps (:947) with means = origins + look *
                       shadow_near_max (:3367), near overwritten with shadow_near_max (:3381-3383).
  weights_from_density geometry_loss_ref's (render.compute_alpha_weights).

A note on shapes.  In the backward term acc is [n, 1], masks = zeros_like(acc) and lossmult is [n, 1, 1], so
`acc[..., None] - masks` broadcasts to [n, n, 1] and lossmult * data_loss to [n, n, 1] with lossmult along the first axis.
Because the masks are all zero, entry (i, j) is lossmult_i * w * sqrt(acc_i^2 + pad^2) for every j: the mean of that
array is exactly the plain mean over the n rays, which is what mask_loss computes (mask_loss_literal_shapes writes the
broadcast out; tests/test_mask_loss.py compares the two).
"""
from __future__ import annotations

import numpy as np
import torch

from geometry_loss_ref import weights_from_density  # noqa: F401  (re-exported)


def schedule_ease_in(train_frac, use, start, frac, min_value=0.0):
    if not use:
        return 1.0
    if frac > 0:
        w = float(np.clip((train_frac - start) / frac, 0.0, 1.0))
        return min_value * (1.0 - w) + w
    return float(train_frac >= start)


def schedule_decay(train_frac, use, start, frac, min_value=0.0):
    if not use:
        return 1.0
    w = float(np.clip((train_frac - start) / frac, 0.0, 1.0))
    return min_value * w + (1.0 - w)


def mask_loss(acc, masks, lossmult, padding, opaque_weight, empty_weight, empty_loss_weight=None, decay=1.0, ease=1.0):
    """compute_mask_loss on acc [n]: masks [n] or None (ones, :801-804); lossmult [n] or None (ones).  With
    empty_loss_weight given the :821-826 branch (0 where masks > 0.5, empty_loss_weight elsewhere), otherwise
    (opaque_weight, empty_weight).  The plain mean over the n rays (see the module docstring for the backward term)."""
    lm = torch.ones_like(acc) if lossmult is None else lossmult.to(acc.dtype)
    m = torch.ones_like(acc) if masks is None else masks.to(acc.dtype)
    data = torch.sqrt((acc - m) ** 2 + padding ** 2) * decay * ease
    if empty_loss_weight is not None:
        data = torch.where(m > 0.5, data * 0.0, data * empty_loss_weight)
    else:
        data = torch.where(m > 0.5, data * opaque_weight, data * empty_weight)
    return torch.mean(lm * data)


def mask_loss_literal_shapes(acc, lossmult, padding, empty_loss_weight):
    """The backward term with the reference's literal shapes in numpy broadcasting: acc [n, 1], masks = zeros_like(acc),
    lossmult [n, 1, 1]; rendering["acc"][..., None] - masks is [n, 1, 1] - [n, 1] -> [n, n, 1]."""
    acc = np.asarray(acc, np.float64).reshape(-1, 1)
    masks = np.zeros_like(acc)
    lm = np.asarray(lossmult, np.float64).reshape(-1, 1, 1)
    data = np.sqrt((acc[..., None] - masks) ** 2 + padding ** 2)
    data = np.where(masks > 0.5, data * 0.0, data * empty_loss_weight)
    full = lm * data
    assert full.shape == (len(acc), len(acc), 1)
    return float(np.mean(full))


def mask_terms_loss(acc, masks, lossmult, terms):
    """mask_loss under the rc_mask_loss fields `terms` (charb_padding, weight_opaque, weight_empty, zero_masks)."""
    if terms.get("zero_masks"):
        masks = torch.zeros_like(acc)
    return mask_loss(acc, masks, lossmult, terms["charb_padding"], terms["weight_opaque"], terms["weight_empty"])


def restated(density, tdist, directions, masks, lossmult, terms, dtype):
    """(loss, d loss / d density [n, S]) of the mask loss on a call's last-level density / tdist, by autograd."""
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a)).to(dtype)
    dens = t(density).requires_grad_(True)
    acc = weights_from_density(dens, t(tdist), t(directions)).sum(dim=-1)
    loss = mask_terms_loss(acc, t(masks), t(lossmult), terms)
    (g,) = torch.autograd.grad(loss, dens)
    return float(loss.detach()), g.double().numpy(), acc.detach().double().numpy()


def rotation_matrix(normal):
    """render_utils.get_rotation_matrix (y_up=False), [..., 3] -> [..., 3, 3] with columns (new_x, new_y, normal)."""
    dt = normal.dtype
    old_z = np.array([0.0, 0.0, 1.0], dt)[None]
    old_y = np.array([0.0, 1.0, 0.0], dt)[None]
    # the reference compares float32 values with the weakly typed 0.9, i.e. with float32(0.9): kept in every dtype
    up = np.where(np.abs(normal[..., 2:3]) < dt.type(np.float32(0.9)), old_z, old_y)
    new_x = np.cross(up, normal).astype(dt)
    new_x = new_x / (np.linalg.norm(new_x, axis=-1, keepdims=True) + dt.type(1e-10))
    new_y = np.cross(normal, new_x).astype(dt)
    new_y = new_y / (np.linalg.norm(new_y, axis=-1, keepdims=True) + dt.type(1e-10))
    return np.stack([new_x, new_y, normal], axis=-1).astype(dt)


def backward_rays(origins, look, u1, u2, shadow_near_max, normal_eps, far, dtype=np.float64):
    """{origins, directions, viewdirs, near, far} of the backward mask rays in `dtype`."""
    dt = np.dtype(dtype)
    f = lambda a: np.asarray(a, np.float32).astype(dt)          # the inputs are float32 on the device
    o, lk, u1, u2 = f(origins), f(look), f(u1).reshape(-1), f(u2).reshape(-1)
    s, e = dt.type(np.float32(shadow_near_max)), dt.type(np.float32(normal_eps))
    nrm = -lk
    means = o + lk * s                                          # train_utils.py:3367
    new_o = means + nrm * e                                     # render_utils.py:947
    costheta = dt.type(1.0) - u1
    sintheta = np.sqrt((dt.type(2.0) - u1) * u1)
    pi = dt.type(np.float32(np.pi)) if dt == np.float32 else dt.type(np.pi)
    phi = u2 * dt.type(2.0) * pi - pi
    wi = np.stack([sintheta * np.cos(phi), sintheta * np.sin(phi), costheta], axis=-1).astype(dt)
    R = rotation_matrix(nrm)
    d = (wi[..., 0:1] * R[..., 0] + wi[..., 1:2] * R[..., 1] + wi[..., 2:3] * R[..., 2]).astype(dt)   # local_to_global (:705-710)
    n = len(o)
    return dict(origins=new_o.astype(dt), directions=d, viewdirs=d, near=np.full(n, s, dt),
                far=np.full(n, dt.type(np.float32(far)), dt))
