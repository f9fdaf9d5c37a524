"""JAX's differentiation rules where torch's differ, for the torch restatements of the losses (tests/*_ref.py; test
helper, not a test module).  One definition of each rule: the restatements import them, and the CPU tests that pin a
rule (derivative of abs at 0, tie splitting of max / min / clip, nan_to_num, l2_normalize's override) pin it for all.

Read from jax 0.4.16 (jax/_src/lax/lax.py, jax/_src/numpy), not run:
  * lax.abs: the JVP is select(x >= 0, g, -g) (`_abs_jvp_rule`): +1 at 0, where torch's sign gives 0;
  * lax.max / lax.min: the balanced-eq JVP passes half of the gradient to each side at a tie; jnp.clip is
    minimum(maximum(x, lo), hi), so each bound splits its tie the same way;
  * jnp.nan_to_num: `where(isnan(x), 0, clip(x, min, max))`-shaped, so the gradient passes where x is finite;
  * math.override_gradient: the value of one expression, the gradient of another.
"""
from __future__ import annotations

import torch

from oracle.mathx import EPS as FLT_EPS, MAXV as F32_MAX, TINY  # noqa: F401  (float32 eps / max / tiny, math.py:24-26)


def value_with_grad_of(value, surrogate):
    """value in the forward pass, the gradient of `surrogate` in the backward pass (math.override_gradient)."""
    return value.detach() + (surrogate - surrogate.detach())


def jabs(x):
    """jnp.abs with lax.abs' JVP: d|x|/dx = +1 at x = 0 (torch.abs would give 0)."""
    return torch.where(x >= 0, x, -x)


def jmaximum(u, v):
    """jnp.maximum(u, v) of two traced arrays: the larger side takes the gradient, half each on a tie."""
    return torch.where(u > v, u, torch.where(u < v, v, 0.5 * (u + v)))


def jminimum(u, v):
    """jnp.minimum(u, v): the smaller side takes the gradient, half each on a tie."""
    return torch.where(u < v, u, torch.where(u > v, v, 0.5 * (u + v)))


def jmax(x, c: float):
    """jnp.maximum(x, c) with a constant c (vmf_loss_fn, render_utils.py:1493-1547): the gradient passes where x > c,
    half of it where x == c."""
    out = torch.where(x > c, x, torch.full_like(x, c))
    return out + torch.where(x == c, 0.5 * (x - x.detach()), torch.zeros_like(x))


def jmax_const(c: float, x):
    """jnp.maximum(c, x), the constant first as material_smoothness writes it (train_utils.py:2505-2700): lax.max is
    symmetric, so this is jmax, tie rule included."""
    return jmax(x, c)


def jmin(x, c: float):
    """jnp.minimum of a traced x and a constant c: the gradient passes where x < c, half of it where x == c."""
    out = torch.where(x < c, x, torch.full_like(x, c))
    return out + torch.where(x == c, 0.5 * (x - x.detach()), torch.zeros_like(x))


def nan_to_num(x):
    """jnp.nan_to_num: nan -> 0, +-inf -> +-float32 max; the gradient passes unchanged where x is finite."""
    fixed = torch.nan_to_num(x.detach(), nan=0.0, posinf=F32_MAX, neginf=-F32_MAX)
    return torch.where(torch.isfinite(x), x, fixed)


def l2_normalize(x, grad_eps: float = FLT_EPS):
    """ref_utils.l2_normalize (ref_utils.py:45-70): forward x / sqrt(max(tiny, |x|^2)), backward through
    x / sqrt(max(grad_eps, |x|^2)), zero where |x|^2 < tiny.  The default grad_eps is the function's own
    (ref_utils.py:45, float32 eps), which normals_pred uses (geometry.py:471); vmf_loss_fn passes grad_eps=1e-5
    (render_utils.py:1503).  The backward's maximum splits its tie as lax.max does."""
    s = (x * x).sum(-1, keepdim=True)
    val = x / torch.sqrt(torch.clamp(s, min=TINY))
    grad = x / torch.sqrt(jmax(s, max(TINY, grad_eps)))
    out = value_with_grad_of(val, grad)
    return torch.where(s < TINY, torch.zeros_like(out), out)
