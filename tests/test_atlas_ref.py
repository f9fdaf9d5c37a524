"""The atlas rule as tests/atlas_ref.py restates it, on the CPU: the three properties the layout promises
-- one owner per texel with the stated counts, every bilinear tap of non-zero weight on a texel the triangle owns, affine
functions reproduced by bilinear sampling -- the corner texels, the cols / rows rule, and the library's host-side layout and
refusals (rc_atlas_layout needs no GPU)."""
import numpy as np
import pytest

import atlas_ref as ar

RS = (4, 5, 7, 8, 16)
TS = (1, 2, 3, 7, 8, 9, 1000, 123457, 2 ** 31 - 1)
RC_ERR_INVALID_ARG, RC_ERR_UNSUPPORTED = -1, -5
N = 24                              # denominator of the dense barycentric sample


def dense_barycentrics(n=N):
    """Every (b0, b1, b2) = (a, b, c) / n with a + b + c = n, as the integers (a, b, c): the corners, the edges and the
    inside."""
    a, b = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    keep = a + b <= n
    a, b = a[keep], b[keep]
    return np.stack([n - a - b, a, b], axis=1)


@pytest.mark.parametrize("r", RS)
def test_ownership_counts(r):
    for T in (1, 2, 3, 7):
        owner, half, i, j = ar.texels(T, r)
        cols, rows, W, H = ar.layout(T, r)
        assert owner.shape == (W * H,)
        counts = np.bincount(owner[owner >= 0], minlength=T)
        assert np.all(counts[0::2] == r * (r + 1) // 2) and np.all(counts[1::2] == r * (r - 1) // 2)
        assert counts.sum() == ar.owned_count(T, r) == (owner >= 0).sum()
        assert np.array_equal(half[owner >= 0], owner[owner >= 0] % 2)


@pytest.mark.parametrize("r", RS)
@pytest.mark.parametrize("half", (0, 1))
def test_every_tap_of_non_zero_weight_is_owned(r, half):
    ti, tj, w = ar.bilinear_taps(r, half, dense_barycentrics(), N)
    live = w > 0
    assert live.any(axis=1).all()
    inside = (ti >= 0) & (ti < r) & (tj >= 0) & (tj < r)
    assert np.all(inside[live])
    assert np.all(((ti + tj >= r).astype(int) == half)[live])      # in the cell and on this half's side of the diagonal
    assert np.allclose(w.sum(axis=1), 1.0, atol=1e-14)


@pytest.mark.parametrize("r", RS)
def test_corner_texels_reproduce_the_vertices(r):
    rng = np.random.Generator(np.random.PCG64(r))
    v = rng.uniform(-1, 1, size=(6, 3)).astype(np.float32)
    tri = np.array([[0, 1, 2], [3, 4, 5]])
    p, owner = ar.points(v, tri, r)
    at = lambda i, j: p[j * r + i]                                  # one cell: W == r
    assert ar.layout(2, r) == (1, 1, r, r)
    for (i, j), vertex in (((0, 0), 0), ((r - 2, 0), 1), ((0, r - 2), 2), ((r - 1, r - 1), 3), ((2, r - 1), 4), ((r - 1, 2), 5)):
        assert owner[j * r + i] == vertex // 3
        assert np.allclose(at(i, j), v[vertex], rtol=0, atol=4 * np.finfo(np.float32).eps), (i, j)
    assert np.array_equal(at(0, 0), v[0]) and np.array_equal(at(r - 1, r - 1), v[3])      # b1 = b2 = 0: exact


@pytest.mark.parametrize("r", RS)
@pytest.mark.parametrize("half", (0, 1))
def test_affine_functions_survive_bilinear_sampling(r, half):
    """f baked at the texel points (float64 barycentrics of the rule) and sampled bilinearly at uv(b) is f at sum b V."""
    rng = np.random.Generator(np.random.PCG64(100 + r))
    V = rng.uniform(-1, 1, size=(3, 3))
    g, c = rng.uniform(-1, 1, size=3), 0.3
    f = lambda x: x @ g + c
    i, j = np.meshgrid(np.arange(r), np.arange(r), indexing="ij")
    b1, b2 = ar.barycentrics(r, np.full(i.shape, half), i, j, np.float64)
    baked = f(V[0] + b1[..., None] * (V[1] - V[0]) + b2[..., None] * (V[2] - V[0]))      # [i, j]
    k = dense_barycentrics()
    b = k / float(N)
    ti, tj, w = ar.bilinear_taps(r, half, k, N)
    ti, tj = np.clip(ti, 0, r - 1), np.clip(tj, 0, r - 1)         # taps of zero weight may fall outside the cell
    sampled = (baked[ti, tj] * w).sum(axis=1)
    assert np.abs(sampled - f(b @ V)).max() <= 1e-13


def test_cols_and_rows():
    for T in TS:
        cols, rows, W, H = ar.layout(T, 4)
        ncells = (T + 1) // 2
        assert cols * cols >= ncells and (cols - 1) * (cols - 1) < ncells
        assert rows * cols >= ncells and (rows - 1) * cols < ncells
        assert (W, H) == (4 * cols, 4 * rows)
    assert ar.layout(1, 4)[:2] == (1, 1) and ar.layout(3, 4)[:2] == (2, 1) and ar.layout(9, 4)[:2] == (3, 2)
    assert ar.layout(1000, 4)[:2] == (23, 22) and ar.layout(2 ** 31 - 1, 4)[:2] == (32768, 32768)


def test_uvs_are_the_corners():
    T, r = 7, 5
    cols, rows, W, H = ar.layout(T, r)
    uv = ar.uvs(T, r)
    assert uv.shape == (T, 3, 2) and uv.dtype == np.float32
    # triangle 5: cell 2 of a 2 x 2 atlas (cx 0, cy 1), half 1
    assert np.allclose(uv[5, 0], [(r - 0.5) / W, 1 - (r + r - 0.5) / H], atol=1e-7)
    assert np.allclose(uv[5, 1], [2.5 / W, 1 - (r + r - 0.5) / H], atol=1e-7)
    assert (uv >= 0).all() and (uv <= 1).all()
    # orientation: both halves keep the sign of the triangle's area (in the image's x right, y down frame)
    X, Y = uv[..., 0] * W, (1 - uv[..., 1]) * H
    area = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (X[:, 2] - X[:, 0]) * (Y[:, 1] - Y[:, 0])
    assert (area > 0).all()


def test_library_layout_and_refusals():
    """rc_atlas_layout is host code: the rule's numbers, and RC_ERR_INVALID_ARG / RC_ERR_UNSUPPORTED where it refuses."""
    import __graft_entry__ as g
    g.build()
    from nrc_amd import mesh, rc_ext

    for T in (1, 2, 3, 7, 8, 9, 1000, 123457):
        for r in RS + (64,):
            if ar.refused(T, r) is None:
                assert mesh.atlas_layout(T, r) == ar.layout(T, r), (T, r)
    code = {"invalid": RC_ERR_INVALID_ARG, "unsupported": RC_ERR_UNSUPPORTED}
    refusals = [(1, 3), (1, 65), (0, 8), (-5, 8), (2 ** 31 - 1, 4), (2 * 4096 * 4096 + 1, 4), (2 * 257 * 257, 64), (2 * 256 * 257, 64)]
    for T, r in refusals:
        assert ar.refused(T, r) is not None, (T, r)
        with pytest.raises(rc_ext.RcError) as e:
            mesh.atlas_layout(T, r)
        assert e.value.code == code[ar.refused(T, r)], (T, r)
    assert mesh.atlas_layout(2 * 4096 * 4096, 4) == (4096, 4096, 16384, 16384)      # the largest atlas
    assert mesh.atlas_layout(2 * 256 * 256, 64) == (256, 256, 16384, 16384)
