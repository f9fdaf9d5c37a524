"""tests/iso_ref.py, the numpy restatement of rc_isosurface, on analytic lattices whose surface stays strictly inside the
box: the mesh is a closed, consistently oriented 2-manifold of the right genus, its vertices sit on their lattice edges
where the linear interpolant meets the iso value, its normals point outwards, and the enclosed volume converges at second
order.  The GPU suite then holds the kernels to this restatement (tests/test_gpu_isosurface.py)."""
import numpy as np
import pytest

import iso_ref

F = np.float32


def lattice(lo, hi, dims):
    axes = [iso_ref.lattice_axis(lo[a], hi[a], dims[a])[0].astype(np.float64) for a in range(3)]
    return np.meshgrid(*axes, indexing="ij")


def sphere(n, r=0.63):
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    x, y, z = lattice(lo, hi, (n, n, n))
    return (r - np.sqrt(x * x + y * y + z * z)).astype(F), lo, hi


def torus():
    lo, hi = (-1.0, -1.0, -0.5), (1.0, 1.0, 0.5)             # spacing 1/16 on every axis; tube radius 0.25 = 4 spacings
    x, y, z = lattice(lo, hi, (33, 33, 17))
    return (0.25 - np.sqrt((np.sqrt(x * x + y * y) - 0.55) ** 2 + z * z)).astype(F), lo, hi


def two_spheres():
    lo, hi = (-2.0, -1.0, -1.0), (2.0, 1.0, 1.0)
    x, y, z = lattice(lo, hi, (33, 17, 17))
    d = lambda cx: 0.6 - np.sqrt((x - cx) ** 2 + y * y + z * z)
    return np.maximum(d(-1.0), d(1.0)).astype(F), lo, hi


CASES = {"sphere": (lambda: sphere(17), 2), "torus": (torus, 0), "two_spheres": (two_spheres, 4)}


@pytest.fixture(scope="module")
def meshes():
    out = {}
    for name, (make, chi) in CASES.items():
        f, lo, hi = make()
        out[name] = (f, lo, hi, chi) + iso_ref.isosurface(f, 0.0, lo, hi)
    return out


def signed_volume(v, t):
    v = v.astype(np.float64)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


@pytest.mark.parametrize("name", list(CASES))
def test_closed_oriented_manifold_of_the_right_genus(meshes, name):
    _, _, _, chi, v, n, t = meshes[name]
    assert v.dtype == F and n.dtype == F and t.dtype == np.int32 and len(t) > 0
    assert t.min() == 0 and t.max() == len(v) - 1 and len(np.unique(t)) == len(v)
    directed = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]).astype(np.int64)
    assert (directed[:, 0] != directed[:, 1]).all()
    key = directed[:, 0] * len(v) + directed[:, 1]
    assert len(np.unique(key)) == len(key)                    # every directed edge once ...
    back = directed[:, 1] * len(v) + directed[:, 0]
    assert np.array_equal(np.sort(key), np.sort(back))        # ... and once the other way: two triangles per edge
    edges = len(key) // 2
    assert len(v) - edges + len(t) == chi
    assert signed_volume(v, t) > 0.0


def test_vertices_sit_on_their_owned_edges_at_the_iso_value(meshes):
    f, lo, hi, _, v, _, _ = meshes["sphere"]
    dims = f.shape
    axes = [iso_ref.lattice_axis(lo[a], hi[a], dims[a])[0].astype(np.float64) for a in range(3)]
    inside = f >= 0
    k = 0
    for ix in range(dims[0]):
        for iy in range(dims[1]):
            for iz in range(dims[2]):
                for dx, dy, dz in iso_ref.DIRS:
                    jx, jy, jz = ix + dx, iy + dy, iz + dz
                    if jx >= dims[0] or jy >= dims[1] or jz >= dims[2] or inside[ix, iy, iz] == inside[jx, jy, jz]:
                        continue
                    p0 = np.array([axes[0][ix], axes[1][iy], axes[2][iz]])
                    p1 = np.array([axes[0][jx], axes[1][jy], axes[2][jz]])
                    d = p1 - p0
                    t = float(np.dot(v[k] - p0, d) / np.dot(d, d))
                    assert -1e-6 <= t <= 1 + 1e-6
                    assert np.abs(p0 + t * d - v[k]).max() < 1e-6
                    assert abs(float(f[ix, iy, iz]) + t * (float(f[jx, jy, jz]) - float(f[ix, iy, iz]))) < 1e-6
                    k += 1
    assert k == len(v)


def test_sphere_normals_point_outwards(meshes):
    _, _, _, _, v, n, _ = meshes["sphere"]
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-5
    assert (np.einsum("ij,ij->i", n, v) > 0).all()


def test_sphere_volume_converges_at_second_order():
    r = 0.63
    exact = 4.0 / 3.0 * np.pi * r ** 3
    err = {}
    for n in (17, 33):
        f, lo, hi = sphere(n, r)
        v, _, t = iso_ref.isosurface(f, 0.0, lo, hi, normals=False)
        err[n] = abs(signed_volume(v, t) - exact)
    assert err[33] < 0.5 * err[17], err
