"""numpy restatement of the probe of a surface point (engine/trainer.py:848-1069), for the CPU and GPU
tests of rc_probe_rays and rc_vmf_panorama.  Test helper, not a test module.  Every function takes a `dtype`
(np.float64: the reference value; np.float32: the same arithmetic at the kernels' precision).

  sphere_directions   utils.get_sphere_directions (internal/utils.py:55-83).  jnp.linspace(a, b, n, endpoint=False)[i]
                      is a (1 - s) + b s with s = i / n (jax's formula without the appended end point, oracle/JAX_CALLS.md
                      N4); the half-pixel offsets 2 pi / (2 W) and pi / (2 H) are Python doubles that meet the array as
                      weak scalars, so they are rounded to `dtype` once.  meshgrid's default "xy" indexing: phi runs along
                      a row, theta down the rows, ray = row W + col.
  position            origins + directions * distance_median + normal_offset * normals (trainer.py:863-871).
  panoramic_radii     camera_utils.pixels_to_rays for ProjectionType.PANORAMIC with pixtocam = diag(2 pi / W, pi / H, 1)
                      and the identity rotation (camera_utils.py:1013-1070, :1415-1443): the directions of the pixel centre
                      and of its +1 neighbours in x and y, radii = 0.5 (|dx - d| + |dy - d|) 2 / sqrt(12).
  probe_rays          the rc_cast_outputs fields of P probes, probe-major; lights, imageplane, look, up are row 0 of the
                      view's arrays (_update_secondary_rays, :944-1012), or the panoramic cast's own value.
  vmf_image           render_vmf (:1026-1069): means / max(|means|, 1e-5), math.safe_exp (the clip at 70) of the logits,
                      normalised; eval_vmf (render_utils.py:1335-1346) with inverse_render.math.safe_exp = exp(min(x, 80))
                      and 1 / 4 pi for kappa <= FLT_EPSILON; the sum over the lobes; linear_to_srgb; save_img_u8.
"""
from __future__ import annotations

import numpy as np

import vis_ref

EPS = np.finfo(np.float32).eps


def _pi(dtype):
    """jnp.pi as it reaches the arrays: the float32 value under jax's default dtype."""
    return dtype(np.float32(np.pi)) if dtype == np.float32 else dtype(np.pi)


def _linspace_open(a, b, n, dtype):
    s = np.arange(n).astype(dtype) / dtype(n)
    return dtype(a) * (dtype(1) - s) + dtype(b) * s


def sphere_angles(height, width, dtype=np.float64):
    """(theta [H], phi [W])"""
    pi = _pi(dtype)
    phi = _linspace_open(pi, -pi, width, dtype) - dtype(2.0 * np.pi / (2.0 * width))
    theta = _linspace_open(0.0, pi, height, dtype) + dtype(np.pi / (2.0 * height))
    return theta, phi


def sphere_directions(height, width, flip=False, dtype=np.float64):
    """[H W, 3] unit directions, ray = row W + col."""
    theta, phi = sphere_angles(height, width, dtype)
    phi, theta = np.meshgrid(phi, theta)
    theta, phi = theta.reshape(-1), phi.reshape(-1)
    if flip:
        x, y, z = -np.cos(theta), np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi)
    else:
        x, y, z = np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)
    return np.stack([x, y, z], -1).astype(dtype)


def position(origins, directions, distance_median, normals, normal_offset=0.4, dtype=np.float64):
    o, d, n = (np.asarray(a, dtype) for a in (origins, directions, normals))
    return (o + d * np.asarray(distance_median, dtype)[..., None]) + dtype(normal_offset) * n


def _pano_direction(x, y, height, width, dtype):
    """The world direction of pixel coordinates (x, y) (centres already added) and its image-plane pair."""
    # pixtocam is built in double and handed over in float32 (the binding's rounding of every camera matrix)
    sx = dtype(np.float32(2.0 * np.pi / width)) if dtype == np.float32 else dtype(2.0 * np.pi / width)
    sy = dtype(np.float32(np.pi / height)) if dtype == np.float32 else dtype(np.pi / height)
    theta, phi = sx * x, sy * y
    cx, cy, cz = -np.sin(phi) * np.sin(theta), -np.cos(phi), -np.sin(phi) * np.cos(theta)
    return np.stack([cx, -cy, -cz], -1)                     # OpenCV -> OpenGL axes; the rotation is the identity


def panoramic_radii(height, width, dtype=np.float64):
    """([H W] radii, [H W, 2] imageplane) of the panoramic cast."""
    ys, xs = np.meshgrid(np.arange(height).astype(dtype), np.arange(width).astype(dtype), indexing="ij")
    half = dtype(0.5)
    d0 = _pano_direction(xs + half, ys + half, height, width, dtype)
    dx = _pano_direction((xs + dtype(1)) + half, ys + half, height, width, dtype)
    dy = _pano_direction(xs + half, (ys + dtype(1)) + half, height, width, dtype)
    dist = lambda a: np.sqrt(((a[..., 0] - d0[..., 0]) ** 2 + (a[..., 1] - d0[..., 1]) ** 2) + (a[..., 2] - d0[..., 2]) ** 2)
    radii = (half * (dist(dx) + dist(dy))) * dtype(2) / dtype(3.4641016151377544)
    return radii.reshape(-1).astype(dtype), d0[..., :2].reshape(-1, 2).astype(dtype)


def probe_rays(view, pixels, height, width, near, far, normal_offset=0.4, flip=False, dtype=np.float64):
    """{field: [P H W, .]} of rc_cast_outputs, and positions [P, 3].  view: dict of arrays; a missing broadcast field
    keeps the panoramic cast's own value."""
    pix = np.asarray(pixels, np.int64)
    P, hw = pix.size, height * width
    pos = position(np.asarray(view["origins"])[pix], np.asarray(view["directions"])[pix],
                   np.asarray(view["distance_median"]).reshape(-1)[pix], np.asarray(view["normals"])[pix], normal_offset, dtype)
    dirs = sphere_directions(height, width, flip, dtype)
    radii, ip = panoramic_radii(height, width, dtype)
    rep = lambda a: np.repeat(np.asarray(a, dtype)[:, None, :], hw, axis=1).reshape(P * hw, -1)
    tile = lambda a: np.tile(np.asarray(a, dtype), (P,) + (1,) * (np.ndim(a) - 1))
    row0 = lambda k, own: (np.broadcast_to(np.asarray(view[k], dtype).reshape(-1, own.shape[-1])[0], own.shape).copy()
                           if view.get(k) is not None else own)
    out = {"origins": rep(pos), "directions": tile(dirs), "viewdirs": tile(dirs), "radii": tile(radii),
           "near": np.full(P * hw, near, dtype), "far": np.full(P * hw, far, dtype)}
    out["lights"] = row0("lights", rep(pos))
    out["imageplane"] = row0("imageplane", tile(ip))
    out["look"] = row0("look", np.broadcast_to(np.asarray([0.0, 0.0, -1.0], dtype), (P * hw, 3)).copy())
    out["up"] = row0("up", np.broadcast_to(np.asarray([0.0, 1.0, 0.0], dtype), (P * hw, 3)).copy())
    return out, pos


def safe_exp70(x, dtype):
    """internal/math.py:186 safe_exp: exp(clip(x, finfo.min, 70))."""
    return np.exp(np.minimum(np.asarray(x, dtype), dtype(70.0)))


def eval_vmf(x, means, kappa, dtype=np.float64):
    """render_utils.eval_vmf; x [..., 1, 3], means [V, 3], kappa [V]."""
    with np.errstate(all="ignore"):
        dot = (x[..., 0] * means[..., 0] + x[..., 1] * means[..., 1]) + x[..., 2] * means[..., 2]
        val = kappa * np.exp(np.minimum(kappa * dot, dtype(80.0))) / (dtype(4) * _pi(dtype) * np.sinh(kappa))
    return np.where(kappa <= dtype(EPS), dtype(1) / (dtype(4) * _pi(dtype)), val)


def lobe_table(means, kappas, logits, dtype=np.float64):
    """(unit means [V, 3], kappas [V], weights [V]) of one mixture."""
    m = np.asarray(means, dtype)
    norm = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
    m = m / np.maximum(norm, dtype(1e-5))[:, None]
    e = safe_exp70(logits, dtype)
    total = dtype(0)
    for v in e:                                              # j ascending
        total = total + v
    return m, np.asarray(kappas, dtype), e / total


def vmf_linear(means, kappas, logits, height, width, flip=False, dtype=np.float64):
    """[H, W] mixture density of one probe, the lobes added over j ascending."""
    m, k, w = lobe_table(means, kappas, logits, dtype)
    xyz = sphere_directions(height, width, flip, dtype)
    val = eval_vmf(xyz[:, None, :], m[None], k[None], dtype)            # [H W, V]
    out = np.zeros(height * width, dtype)
    for j in range(m.shape[0]):
        out = out + w[j] * val[:, j]
    return out.reshape(height, width)


def vmf_image(means, kappas, logits, height, width, flip=False, dtype=np.float64):
    """(linear [P, H, W], srgb [P, H, W, 3]) of P mixtures."""
    lin = np.stack([vmf_linear(m, k, l, height, width, flip, dtype) for m, k, l in zip(means, kappas, logits)])
    srgb = vis_ref.linear_to_srgb(lin, dtype)
    return lin, np.repeat(srgb[..., None], 3, axis=-1)


to_u8 = vis_ref.to_u8
