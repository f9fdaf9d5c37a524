"""The whole export path on the GPU (nrc_amd/mesh.py) on make_rc weights with the material stage's, at 24^3: extract_mesh
is isosurface(density_lattice(...)) bit for bit, its attributes are query_points at its vertices, and save_obj round-trips
through a small parser."""
import numpy as np
import pytest
import torch

import common
from nrc_amd import mesh

pytestmark = pytest.mark.gpu
LO, HI, DIMS = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (24, 24, 24)
ATTRIBUTES = ("albedo", "roughness", "metalness", "normals_pred", "normals", "density")


@pytest.fixture(scope="module")
def case():
    rc = common.make_rc(weights=common.weights_material_np())
    field = mesh.density_lattice(rc, LO, HI, DIMS)
    iso = float(field.median())                     # half of the lattice inside: a surface through the whole box
    m = mesh.extract_mesh(rc, iso, LO, HI, DIMS, attributes=ATTRIBUTES)
    torch.cuda.synchronize()
    return rc, field, iso, m


def test_extract_mesh_is_the_three_calls(case):
    rc, field, iso, m = case
    assert torch.equal(field, mesh.density_lattice(rc, LO, HI, DIMS))
    v, n, t = mesh.isosurface(rc, field, iso, LO, HI)
    assert len(v) > 100 and len(t) > 100
    assert torch.equal(m.vertices, v) and torch.equal(m.normals, n) and torch.equal(m.triangles, t)
    assert m.triangles.dtype == torch.int32 and int(m.triangles.min()) == 0 and int(m.triangles.max()) == len(v) - 1
    lo, hi = torch.tensor(LO, device="cuda"), torch.tensor(HI, device="cuda")
    assert bool((m.vertices >= lo - 1e-6).all()) and bool((m.vertices <= hi + 1e-6).all())      # lo + 23 step is hi up to an ulp
    v2, n2, t2 = mesh.isosurface(rc, field, iso, LO, HI, normals=False)
    assert n2 is None and torch.equal(v2, v) and torch.equal(t2, t)


def test_attributes_are_the_query_at_the_vertices(case):
    rc, _, _, m = case
    assert set(m.attributes) == set(ATTRIBUTES)
    q = mesh.query_points(rc, m.vertices, ATTRIBUTES)
    V = m.vertices.shape[0]
    for k in ATTRIBUTES:
        assert m.attributes[k].shape[0] == V and torch.equal(m.attributes[k], q[k]), k
    assert m.attributes["albedo"].shape == (V, 3) and m.attributes["roughness"].shape == (V,)
    empty = mesh.extract_mesh(rc, 1e30, LO, HI, (4, 4, 4), attributes=("albedo", "density"))
    assert empty.vertices.shape == (0, 3) and empty.triangles.shape == (0, 3) and empty.attributes["albedo"].shape == (0, 3)


def parse_obj(path):
    v, vn, f = [], [], []
    for line in open(path):
        kind, *rest = line.split()
        if kind == "v":
            v.append([float(x) for x in rest])
        elif kind == "vn":
            vn.append([float(x) for x in rest])
        elif kind == "f":
            corners = [c.split("//") for c in rest]
            assert all(len(c) == 2 and c[0] == c[1] for c in corners), line
            f.append([int(c[0]) for c in corners])
        else:
            raise AssertionError(line)
    return np.asarray(v, np.float64), np.asarray(vn, np.float64), np.asarray(f, np.int64)


@pytest.mark.parametrize("colors", [False, True])
def test_save_obj_round_trips(case, tmp_path, colors):
    _, _, _, m = case
    path = str(tmp_path / "mesh.obj")
    mesh.save_obj(path, m, colors=m.attributes["albedo"] if colors else None)
    v, vn, f = parse_obj(path)
    V, T = m.vertices.shape[0], m.triangles.shape[0]
    assert v.shape == (V, 6 if colors else 3) and vn.shape == (V, 3) and f.shape == (T, 3)
    assert f.min() == 1 and f.max() == V                                         # 1-based and in range
    assert np.array_equal(f - 1, m.triangles.cpu().numpy())
    assert np.array_equal(v[:, :3].astype(np.float32), m.vertices.cpu().numpy())   # printed with the digits that round-trip
    assert np.array_equal(vn.astype(np.float32), m.normals.cpu().numpy())
    if colors:
        assert np.array_equal(v[:, 3:].astype(np.float32), m.attributes["albedo"].cpu().numpy())
