"""numpy restatement of the per-triangle texture atlas (include/rc_abi.h states the rule), for the CPU and
GPU tests of rc_atlas_layout, rc_atlas_uvs, rc_atlas_points and rc_bake_atlas.  Test helper, not a test module.

T >= 1 triangles, a cell of r x r texels (4 <= r <= 64), two triangles per cell:
    ncells = ceil(T / 2); cols = the smallest integer with cols^2 >= ncells; rows = ceil(ncells / cols); W = cols r, H = rows r
    texel (x, y) (x from the left, y from the top; image element [y, x]; linear index y W + x):
        cx = x // r, cy = y // r, cell = cy cols + cx, i = x - cx r, j = y - cy r, half = (i + j >= r), t = 2 cell + half
        empty when cell >= ncells or t >= T
    barycentrics of the texel centre:  half 0: b1 = i / (r - 2), b2 = j / (r - 2)
                                       half 1: b1 = (r - 1 - i) / (r - 3), b2 = (r - 1 - j) / (r - 3);  b0 = 1 - b1 - b2
    world point:  p = (V0 + b1 (V1 - V0)) + b2 (V2 - V0), every operation in float32
    corners in local texel units (texel (i, j) has its centre at (i + 0.5, j + 0.5)):
        half 0: (0.5, 0.5), (r - 1.5, 0.5), (0.5, r - 1.5);   half 1: (r - 0.5, r - 0.5), (2.5, r - 0.5), (r - 0.5, 2.5)
    uv of a corner at global texel coordinates (X, Y):  u = X / W, v = 1 - Y / H in float32
"""
import math

import numpy as np

MAX_SIDE = 16384


def layout(T, r):
    """(cols, rows, W, H) by the rule alone, in Python integers (no refusal: `refused` tells)."""
    ncells = (T + 1) // 2
    cols = math.isqrt(ncells - 1) + 1 if ncells > 0 else 0           # the smallest integer with cols^2 >= ncells
    rows = -(-ncells // cols)
    return cols, rows, cols * r, rows * r


def refused(T, r):
    """None, or the reason the library refuses: "invalid" (T < 1, r outside 4 .. 64) before "unsupported" (a side above 16384)."""
    if T < 1 or r < 4 or r > 64:
        return "invalid"
    _, _, W, H = layout(T, r)
    return "unsupported" if W > MAX_SIDE or H > MAX_SIDE else None


def texels(T, r, first=0, count=None):
    """Per texel of the linear range: owner (-1: empty), half, i, j as int64 arrays."""
    cols, rows, W, H = layout(T, r)
    count = W * H - first if count is None else count
    lin = first + np.arange(count, dtype=np.int64)
    y, x = lin // W, lin % W
    cx, cy = x // r, y // r
    i, j = x - cx * r, y - cy * r
    cell = cy * cols + cx
    half = (i + j >= r).astype(np.int64)
    t = 2 * cell + half
    owner = np.where((cell >= (T + 1) // 2) | (t >= T), -1, t)
    return owner, half, i, j


def barycentrics(r, half, i, j, dtype=np.float32):
    """(b1, b2) of the texel centres, one division each in `dtype`."""
    f = lambda a: np.asarray(a).astype(dtype)
    b1 = np.where(half == 1, f(r - 1 - i) / dtype(r - 3), f(i) / dtype(r - 2)).astype(dtype)
    b2 = np.where(half == 1, f(r - 1 - j) / dtype(r - 3), f(j) / dtype(r - 2)).astype(dtype)
    return b1, b2


def points(vertices, triangles, r, first=0, count=None):
    """(points [count, 3] float32, owner [count] int32): the world point of each texel, (0, 0, 0) where it is empty."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    owner, half, i, j = texels(tri.shape[0], r, first, count)
    b1, b2 = barycentrics(r, half, i, j)
    t = np.maximum(owner, 0)
    v0, v1, v2 = v[tri[t, 0]], v[tri[t, 1]], v[tri[t, 2]]
    p = (v0 + b1[:, None] * (v1 - v0)) + b2[:, None] * (v2 - v0)
    assert p.dtype == np.float32
    p[owner < 0] = 0.0
    return p, owner.astype(np.int32)


def corners(r, half):
    """The three corners of a half's uv triangle in local texel units, [3, 2] float64."""
    if half == 0:
        return np.array([[0.5, 0.5], [r - 1.5, 0.5], [0.5, r - 1.5]])
    return np.array([[r - 0.5, r - 0.5], [2.5, r - 0.5], [r - 0.5, 2.5]])


def uvs(T, r):
    """[T, 3, 2] float32: (u, v) of every triangle corner."""
    cols, rows, W, H = layout(T, r)
    t = np.arange(T, dtype=np.int64)
    cell, half = t // 2, t % 2
    cx, cy = cell % cols, cell // cols
    local = np.where(half[:, None, None] == 0, corners(r, 0)[None], corners(r, 1)[None]).astype(np.float32)      # [T, 3, 2]
    X = (cx * r).astype(np.float32)[:, None] + local[..., 0]
    Y = (cy * r).astype(np.float32)[:, None] + local[..., 1]
    u = X / np.float32(W)
    v = np.float32(1) - Y / np.float32(H)
    out = np.stack([u, v], axis=-1)
    assert out.dtype == np.float32
    return out


def owned_count(T, r):
    """Texels that have an owner: r (r + 1) / 2 per half 0, r (r - 1) / 2 per half 1."""
    n0, n1 = (T + 1) // 2, T // 2
    return n0 * (r * (r + 1) // 2) + n1 * (r * (r - 1) // 2)


def bilinear_taps(r, half, k, n):
    """The bilinear taps of the local uv  sum (k_c / n) corner_c  (k [m, 3] integers that sum to n: exact barycentrics)
    inside one cell: (ti, tj [m, 4] texel indices, w [m, 4] weights), texel centres at (i + 0.5, j + 0.5).  The position
    among the texel centres is worked out in integers (units of 1 / (2 n)), so a uv on a texel centre or on the line
    between two of them has exactly zero weight on the far side."""
    k = np.asarray(k, np.int64)
    g = k @ np.round(2 * corners(r, half)).astype(np.int64) - n          # 2 n (uv - 0.5)
    i0, j0 = g[:, 0] // (2 * n), g[:, 1] // (2 * n)
    fx, fy = (g[:, 0] - i0 * 2 * n) / (2.0 * n), (g[:, 1] - j0 * 2 * n) / (2.0 * n)
    ti = np.stack([i0, i0 + 1, i0, i0 + 1], axis=1)
    tj = np.stack([j0, j0, j0 + 1, j0 + 1], axis=1)
    w = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], axis=1)
    return ti, tj, w
