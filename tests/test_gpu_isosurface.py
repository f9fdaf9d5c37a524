"""rc_isosurface on the GPU against tests/iso_ref.py (which tests/test_iso_ref.py holds to the properties of a surface):
both sides get the same float32 lattice; counts and triangles must be equal exactly, row by row; vertices within 2 ulp of
the box extent (the device may contract p0 + t d into an FMA), normals within 1e-5.

Shapes: one cell with all 254 non-trivial corner masks (the only place every case of every tetrahedron is hit), 5 x 7 x 9
(odd, no multiple of any block), 3 x 2 x 130 (a long iz run across wavefront boundaries) and 70^3 = 343 000 points: the
scan works on tiles of kRcIsoTile = 1024 points (one workgroup) in groups of kRcIsoGroup = 256 tiles (one workgroup of
k_iso_scan_tiles), so 70^3 has 335 tiles in 2 groups -- more than one scan block and more than one level of the hierarchy."""
import ctypes as C

import numpy as np
import pytest
import torch

import common
import iso_ref

pytestmark = pytest.mark.gpu
F = np.float32
SHAPES = ((5, 7, 9), (3, 2, 130), (70, 70, 70))
FIELDS = ("smooth", "sphere", "plane", "nan", "all_inside", "all_outside")
LO, HI = (-1.0, -0.5, -1.5), (1.0, 1.5, 0.25)
SENTINEL = -777.0


@pytest.fixture(scope="module")
def rc():
    return common.make_rc()


def make_field(kind, dims):
    """(lattice float32 [nx, ny, nz], iso)"""
    ax = [np.linspace(-1.0, 1.0, n) for n in dims]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    smooth = np.sin(3.1 * x + 1.0) + np.sin(4.3 * y * z + 2.0) + np.sin(5.2 * z - 2.2 * x + 0.5) + 0.5 * np.sin(7.0 * (x + y))
    if kind == "smooth":
        return smooth.astype(F), 0.3
    if kind == "sphere":
        return (1.2 - np.sqrt(x * x + y * y + z * z)).astype(F), 0.0      # leaves the box: an open surface, inside on every shape
    if kind == "plane":           # integers: f == iso exactly on a diagonal plane of lattice points, t = 0 and t = 1
        i, j, k = np.meshgrid(*[np.arange(n) for n in dims], indexing="ij")
        return ((sum(dims) // 2 - 1) - (i + j + k)).astype(F), 0.0
    if kind == "nan":
        f = smooth.astype(F)
        rng = np.random.Generator(np.random.PCG64(11))
        f[rng.uniform(size=f.shape) < 0.05] = np.nan
        return f, 0.3
    return np.full(dims, 1.0 if kind == "all_inside" else -1.0, dtype=F), 0.0


_REF = {}


def reference(kind, dims):
    if (kind, dims) not in _REF:
        f, iso = make_field(kind, dims)
        _REF[(kind, dims)] = (f, iso) + iso_ref.isosurface(f, iso, LO, HI)
    return _REF[(kind, dims)]


def raw_call(rc, field, iso, lo, hi, vertices, normals, v_cap, triangles, t_cap, counts):
    """rc_isosurface with explicit capacities -> status"""
    nx, ny, nz = field.shape
    vec = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    ptr = lambda t: None if t is None else t.data_ptr()
    return rc.lib.rc_isosurface(rc._h, field.data_ptr(), nx, ny, nz, float(iso), vec(lo), vec(hi), ptr(vertices), ptr(normals),
                                v_cap, ptr(triangles), t_cap, counts.data_ptr(), torch.cuda.current_stream().cuda_stream)


def compare(got, want, what):
    v, n, t = (x.cpu().numpy() for x in got)
    rv, rn, rt = want
    assert v.shape == rv.shape and t.shape == rt.shape, (what, v.shape, rv.shape, t.shape, rt.shape)
    assert np.array_equal(t, rt), what
    extent = max(h - l for l, h in zip(LO, HI))
    err = float(np.abs(v.astype(np.float64) - rv).max()) if len(v) else 0.0
    nerr = np.abs(n.astype(np.float64) - rn)
    assert np.array_equal(np.isnan(n), np.isnan(rn)), what
    nerr = float(np.nanmax(nerr)) if nerr.size and not np.isnan(nerr).all() else 0.0
    print(what, "V", len(v), "T", len(t), "vertex err", err, "normal err", nerr)
    assert err <= 2.0 * float(np.spacing(F(extent))), (what, err)
    assert nerr <= 1e-5, (what, nerr)


@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_against_the_restatement(rc, dims, kind):
    f, iso, rv, rn, rt = reference(kind, dims)
    got = rc.isosurface(torch.from_numpy(f).cuda(), iso, LO, HI)
    if kind.startswith("all_"):
        assert len(rv) == 0 and len(rt) == 0
    else:
        assert len(rv) > 0 and len(rt) > 0
    compare(got, (rv, rn, rt), f"{kind} {dims}")


def test_single_cell_every_corner_mask(rc):
    """2 x 2 x 2: all 254 non-trivial inside / outside assignments of the 8 corners, random magnitudes."""
    rng = np.random.Generator(np.random.PCG64(5))
    for mask in range(1, 255):
        mag = rng.uniform(0.2, 1.0, size=8).astype(F)
        bits = np.array([(mask >> c) & 1 for c in range(8)], dtype=bool)          # corner code dx | dy << 1 | dz << 2
        f = np.zeros((2, 2, 2), dtype=F)
        for c in range(8):
            f[c & 1, (c >> 1) & 1, c >> 2] = mag[c] if bits[c] else -mag[c]
        want = iso_ref.isosurface(f, 0.0, LO, HI)
        assert len(want[2]) > 0
        got = rc.isosurface(torch.from_numpy(f).cuda(), 0.0, LO, HI)
        v, n, t = (x.cpu().numpy() for x in got)
        assert np.array_equal(t, want[2]), mask
        assert v.shape == want[0].shape and np.abs(v - want[0]).max() <= 2.0 * float(np.spacing(F(2.0))), mask
        assert np.abs(n - want[1]).max() <= 1e-5, mask


def test_two_pass_protocol_and_determinism(rc):
    dims = (5, 7, 9)
    f, iso, rv, rn, rt = reference("smooth", dims)
    V, T = len(rv), len(rt)
    field = torch.from_numpy(f).cuda()
    fresh = lambda: (torch.full((V + 4, 3), SENTINEL, device="cuda"), torch.full((V + 4, 3), SENTINEL, device="cuda"),
                     torch.full((T + 4, 3), -7, dtype=torch.int32, device="cuda"), torch.full((2,), -1, dtype=torch.int64, device="cuda"))
    untouched = lambda v, n, t: bool((v == SENTINEL).all()) and bool((n == SENTINEL).all()) and bool((t == -7).all())
    # capacities 0, and one short on either side: only the counts
    for v_cap, t_cap in ((0, 0), (V - 1, T), (V, T - 1), (0, T), (V, 0)):
        v, n, t, counts = fresh()
        assert raw_call(rc, field, iso, LO, HI, v, n, v_cap, t, t_cap, counts) == 0
        torch.cuda.synchronize()
        assert counts.tolist() == [V, T], (v_cap, t_cap)
        assert untouched(v, n, t), (v_cap, t_cap)
    # exact capacities: everything, and nothing behind it
    runs = []
    for _ in range(2):
        v, n, t, counts = fresh()
        assert raw_call(rc, field, iso, LO, HI, v, n, V, t, T, counts) == 0
        torch.cuda.synchronize()
        assert counts.tolist() == [V, T]
        assert untouched(v[V:], n[V:], t[T:])
        runs.append((v[:V].clone(), n[:V].clone(), t[:T].clone()))
    compare(runs[0], (rv, rn, rt), "exact capacities")
    assert all(torch.equal(a, b) for a, b in zip(*runs))                          # bitwise
    # without normals
    v, n, t, counts = fresh()
    assert raw_call(rc, field, iso, LO, HI, v, None, V + 4, t, T + 4, counts) == 0
    torch.cuda.synchronize()
    assert torch.equal(v[:V], runs[0][0]) and torch.equal(t[:T], runs[0][2]) and untouched(v[V:], n, t[T:])


def test_refusals(rc):
    field = torch.zeros((3, 3, 3), device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    v = torch.zeros((4, 3), device="cuda")
    t = torch.zeros((4, 3), dtype=torch.int32, device="cuda")
    ok = lambda **kw: raw_call(rc, kw.get("field", field), 0.0, kw.get("lo", LO), kw.get("hi", HI), kw.get("v", v), None,
                               kw.get("v_cap", 4), kw.get("t", t), kw.get("t_cap", 4), counts)
    assert ok() == 0
    assert ok(v_cap=2 ** 31) == -1                                   # v_capacity > INT32_MAX
    assert ok(v_cap=-1) == -1 and ok(t_cap=-1) == -1
    assert ok(v=None) == -1 and ok(t=None) == -1                     # a capacity without its array
    assert ok(hi=(1.0, LO[1], 0.25)) == -1                           # hi[a] <= lo[a]
    assert ok(field=torch.zeros((1, 3, 3), device="cuda")) == -1     # a dimension outside 2 .. 1024
    assert ok(field=torch.zeros((2, 1025, 2), device="cuda")) == -1
    torch.cuda.synchronize()
