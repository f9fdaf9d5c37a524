"""The grid kernels on grid geometries other than the reference's, against the oracle (fp32 bitwise where every step is
exactly rounded, fp64 elsewhere).

rc_create accepts any grid layout with 1 or 4 features, at most 8 levels, K0 / K1 in {5..8, 31, 32} and K2 = KA = 32;
the host then picks kernels by geometry.  Three geometries reach the paths the hotdog layout never does:

  A  every hash table 2^17 entries: two dense levels instead of three.  The level kernels take their run-time layout
     form (<1,6,-1>, <1,7,-1>, <4,8,-1>), the fused plan is refused, the F = 1 scatter runs its hashed levels in 4
     slices, the F = 4 dense levels go to k_grid_scatter_small<4> (16^3) and k_grid_scatter<4> (32^3).
  B  non-power-of-two tables and odd feature counts: grid 0 10..160 cells against 100 003 entries (5 levels, K = 5),
     grid 1 12..1536 against 2^17 (8 levels, K = 8), grids 2 / 3 against 393 216 = 3 * 2^17.  The `hash % entries`
     path of k_hashgrid_fwd and k_grid_scatter<1|4>, the separate gather + k_density_mlp, k_density_bwd<4> (K = 5) and
     <5> (K = 8), k_grid_scatter_small<1> (10^3 = 1000 floats, not a multiple of 64).
  C  the reference layout with bbox 2, precondition_scaling 4 and contract_radius 5: the fused plan and every backward
     on a non-unit box (the `inside` test of k_density_bwd).
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import common
import interlevel_ref as ir
import loss_cases as lc
import nrc_amd
from nrc_amd import rc_ext, train
from nrc_amd.config import GridConfig
from oracle import hashgrid_ref, mathx, train_ref

pytestmark = pytest.mark.gpu

_H = nrc_amd.hotdog_config()
_r = dataclasses.replace


def _all_grids(cfg, **kw):
    return _r(cfg, proposal_grids=tuple(_r(g, **kw) for g in cfg.proposal_grids), appearance_grid=_r(cfg.appearance_grid, **kw),
              material_grid=_r(cfg.material_grid, **kw), light_grid=_r(cfg.light_grid, **kw))


CFGS = {
    "A": _all_grids(_H, hash_map_size=2 ** 17),
    "B": _r(_H, proposal_grids=(GridConfig(hash_map_size=100003, min_grid_size=10, max_grid_size=160, num_features=1),
                                GridConfig(hash_map_size=2 ** 17, min_grid_size=12, max_grid_size=1536, num_features=1),
                                _r(_H.proposal_grids[2], hash_map_size=393216)),
            appearance_grid=_r(_H.appearance_grid, hash_map_size=393216), material_grid=_r(_H.material_grid, hash_map_size=393216),
            light_grid=_r(_H.light_grid, hash_map_size=393216)),
    "C": _r(_all_grids(_H, bbox=2.0, precondition_scaling=4.0), contract_radius=5.0),
}
GEOMS = tuple(CFGS)
GEOM_IDS = lambda g: f"geom{g}"       # -k geomA selects one geometry
PREFIXES = ("params/Cache/Sampler/MLP_0/density_grid", "params/Cache/Sampler/MLP_1/density_grid",
            "params/Cache/Sampler/MLP_2/density_grid", "params/Cache/Shader/appearance_grid",
            "params/MaterialShader/material_grid", "params/LightSampler/light_grid")
EPS32 = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def weights_np(geom, smooth):
    """Cache + material weights of a geometry: white-noise tables, or smooth ones (amplitude 0.2 * 0.5**level) where
    fp32 is held to fp64 -- white noise at 2048 cells a side turns a coordinate ulp into a visible feature change."""
    kw = dict(level_decay=0.5, table_range=0.2) if smooth else {}
    return nrc_amd.synthetic_weights(CFGS[geom], passes=("cache", "material"), seed=3, **kw)


def weights_t(geom, smooth, dtype=torch.float64):
    return common.to_torch(weights_np(geom, smooth), dtype)


_HANDLES = {}


def handle(geom, smooth=False):
    key = (geom, smooth)
    if key not in _HANDLES:
        _HANDLES[key] = common.make_rc(cfg=CFGS[geom], weights=weights_np(geom, smooth))
    return _HANDLES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()


def grid(geom, gid):
    cfg = CFGS[geom]
    return (list(cfg.proposal_grids) + [cfg.appearance_grid, cfg.material_grid, cfg.light_grid])[gid]


def encode(geom, smooth, gid, pts, contract=True, dtype=torch.float64, tables=None):
    """hashgrid_ref.hash_encoding of grid `gid` at the world-space points (contracted with the config's radius)."""
    x = torch.from_numpy(np.asarray(pts)).to(dtype)
    if contract:
        x = mathx.contract_radius(x, CFGS[geom].contract_radius)
    return hashgrid_ref.hash_encoding(tables if tables is not None else weights_t(geom, smooth, dtype), PREFIXES[gid],
                                      grid(geom, gid), x)


def _points(n, seed, spread):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.normal(size=(n, 3)) * spread).astype(np.float32)


def assert_same_entries(name, a, b, n, F):
    """Table gradients `a` (fp32 kernel) and `b` (fp64 oracle) of one level touch the same entries, up to corners whose
    trilinear weight is exactly 0 in one precision only: the fp32 cell coordinate x01 * size - 0.5 rounded onto an
    integer, which befalls about size * ulp(x01) <= size * 2^-23 of n points per axis.  Each such point leaves 4 corners
    (4 F floats) on one side only, carrying the gradient of a weight of a few rounding errors: <= 1e-3 of the scale."""
    size = int(name.rsplit("_", 1)[1])
    lam = 3 * n * size * 2.0 ** -23
    only = (a != 0.0) != (b != 0.0)
    assert np.count_nonzero(only) <= 4 * F * (2 + 4 * lam), (name, np.count_nonzero(only), lam)
    scale = max(1e-12, float(np.abs(b).max()))
    assert float(np.abs(np.where(only, a - b, 0.0)).max(initial=0.0)) <= 1e-3 * scale, name


# ---------------------------------------------------------------------------------------------
# rc_create: geometries the kernels are not built for
# ---------------------------------------------------------------------------------------------
REJECTED = {
    "two features": _r(_H, proposal_grids=(_r(_H.proposal_grids[0], num_features=2),) + _H.proposal_grids[1:]),
    "nine levels": _r(_H, proposal_grids=_H.proposal_grids[:2] + (_r(_H.proposal_grids[2], max_grid_size=4096),)),
    "K0 = 4": _r(_H, proposal_grids=(_r(_H.proposal_grids[0], max_grid_size=128),) + _H.proposal_grids[1:]),
    "KA = 28": _r(_H, appearance_grid=_r(_H.appearance_grid, max_grid_size=1024)),
}


def test_rc_create_refuses_unsupported_geometries():
    assert [g.num_levels for g in (REJECTED["nine levels"].proposal_grids[2], REJECTED["K0 = 4"].proposal_grids[0],
                                   REJECTED["KA = 28"].appearance_grid)] == [9, 4, 7]
    for what, cfg in REJECTED.items():
        with pytest.raises(rc_ext.RcError) as e:
            rc_ext.RadianceCache(cfg, 0)
        assert e.value.code == -5, (what, e.value.code)                    # RC_ERR_UNSUPPORTED
        assert "rc_create:" in str(e.value) and len(str(e.value)) > 30, (what, str(e.value))
    # the refusals leave nothing behind: a valid handle made afterwards renders
    rc = common.make_rc()
    out = rc.render_rays(nrc_amd.synthetic_rays(7, seed=2).hot_fields(), None, outputs=["rgb", "acc"])
    assert out["rgb"].shape == (7, 3) and bool(torch.isfinite(out["rgb"]).all()) and float(out["acc"].max()) > 0.0
    rc.close()


# ---------------------------------------------------------------------------------------------
# rc_hashgrid_lookup, grids 0-5
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 33, 4097])
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_lookup_inside_the_unit_ball_is_bit_exact(geom, n):
    """Where the contraction is the identity (|x / radius| < 1) every step of the lookup is one exactly rounded fp32
    operation in the same order as the oracle's: bitwise equal, dense, hashed and `hash % entries` levels alike."""
    cfg = CFGS[geom]
    rng = np.random.default_rng(100 + n)
    pts = rng.uniform(-0.55, 0.55, size=(n, 3)).astype(np.float32) * np.float32(cfg.contract_radius)
    if geom == "C":
        # the box arithmetic: the oracle's (x - lo) / (hi - lo), the kernel's unit_box -- rc_div by 2 * bbox = 4, a
        # power of two, as the product with the exact reciprocal -- are the same fp32 values
        x = torch.from_numpy(pts)
        lo, hi = -cfg.appearance_grid.bbox, cfg.appearance_grid.bbox
        assert torch.equal((x - lo) / (hi - lo), (x + np.float32(2.0)) * np.float32(0.25))
        # and the contraction's x / 5 (not a power of two: an IEEE division on both sides)
        assert torch.equal(x / cfg.contract_radius, torch.from_numpy(pts / np.float32(5.0)))
    rc = handle(geom)
    for gid in range(6):
        out = rc.hashgrid_lookup(gid, pts).cpu()
        ref = encode(geom, False, gid, pts, dtype=torch.float32)
        assert out.shape == ref.shape == (n, grid(geom, gid).out_dim)
        assert torch.equal(out, ref), (gid, float((out - ref).abs().max()))


@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_lookup_without_contraction_negative_and_outside_the_box(geom):
    """apply_contraction=False at coordinates in [-3, 3] * bbox: dense levels outside the box read the zero padding
    (exact zeros), hashed levels hash the negative corner coordinates through the uint32 wrap."""
    cfg = CFGS[geom]
    rng = np.random.default_rng(7)
    b = cfg.appearance_grid.bbox
    pts = rng.uniform(-3.0 * b, 3.0 * b, size=(2047, 3)).astype(np.float32)
    pts[:3] = np.array([[-1.7, 0.3, 1.9], [-0.999, -0.999, -0.999], [1.0, 1.0, 1.0]], np.float32) * np.float32(b)
    far = np.abs(pts).max(axis=1) >= 1.2 * b
    assert 100 < far.sum() < len(pts)
    rc = handle(geom)
    for gid in range(6):
        g = grid(geom, gid)
        out = rc.hashgrid_lookup(gid, pts, apply_contraction=False).cpu()
        ref = encode(geom, False, gid, pts, contract=False, dtype=torch.float32)
        assert torch.equal(out, ref), (gid, float((out - ref).abs().max()))
        ndense = sum(g.is_dense(s) for s in g.grid_sizes) * g.num_features
        assert bool((out[far, :ndense] == 0.0).all()) and bool((out[far, ndense:] != 0.0).any()), gid
        assert bool((out[~far] != 0.0).any()), gid


@pytest.mark.parametrize("n", [1, 33, 4097])
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_lookup_with_contraction_against_fp64(geom, n):
    """Points out to 2.5 contraction radii (smooth tables): within 4x the fp32 oracle's own distance from fp64."""
    cfg = CFGS[geom]
    pts = _points(n, 200 + n, 1.2 * cfg.contract_radius)
    rc = handle(geom, smooth=True)
    for gid in range(6):
        out = rc.hashgrid_lookup(gid, pts).cpu().double()
        r64 = encode(geom, True, gid, pts)
        r32 = encode(geom, True, gid, pts, dtype=torch.float32).double()
        scale = float(r64.abs().max())
        err, err32 = float((out - r64).abs().max()), float((r32 - r64).abs().max())
        assert err <= 4.0 * err32 + 1e-5 * scale, (gid, err, err32, scale)


# ---------------------------------------------------------------------------------------------
# rc_hashgrid_backward, grids 0-3
# ---------------------------------------------------------------------------------------------
def _backward_points(geom, gid, case):
    """(points, apply_contraction) of a point set."""
    cfg, g = CFGS[geom], grid(geom, gid)
    b = g.bbox
    if case.startswith("n="):
        n = int(case[2:])
        p = _points(n, 31 + n, 0.6 * cfg.contract_radius)           # some beyond the contraction radius
        p[: n // 8] = 0.0                                           # coincident samples: colliding table updates
        return p, True
    if case == "faces":
        # corner coordinates of the cells of the first (dense) level, x01 * size - 0.5 an integer, on every axis (cell
        # vertices) or one (faces), and points on the box's faces +-bbox.  Every coordinate is dyadic with a few bits
        # (for sizes 10 and 12 only the corners whose x01 = (2k + 1) / (2 size) is), so x01 * size - 0.5 is the same
        # number in fp32 and fp64 and both sides give the same corners a weight of exactly 0
        s = g.grid_sizes[0]
        odd = s // (s & -s)
        rng = np.random.default_rng(gid)
        ks = np.array([k for k in range(-1, s + 1) if (2 * k + 1) % odd == 0])
        p = b * (2.0 * (rng.choice(ks, size=(300, 3)) + 0.5) / s - 1.0)
        dy = lambda *shape: b * rng.integers(-4096, 4097, size=shape) / 4096.0
        p[100:200, 1:] = dy(100, 2)
        p[200:260] = rng.choice([-b, b], size=(60, 3))
        p[260:] = dy(40, 3)
        p[260:, 0] = rng.choice([-b, b], size=40)
        assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
        return p.astype(np.float32), False
    if case == "uncontracted":
        rng = np.random.default_rng(gid + 50)
        return rng.uniform(-3.0, 3.0, size=(900, 3)).astype(np.float32), False
    raise ValueError(case)


def _fp64_table_grads(geom, gid, pts, d, contract, absolute=False):
    """autograd of sum(d * encoding) w.r.t. the tables of grid `gid` in fp64 (with |d| and |tables| for `absolute`:
    per entry the sum of |trilinear weight * d| over the adds it receives, times the precondition factor)."""
    w = weights_t(geom, False)
    layout = handle(geom).hashgrid_grad_layout(gid)[0]
    names = [name for name, _, _ in layout]
    ww = dict(w)
    for k in names:
        ww[k] = w[k].detach().clone().requires_grad_(True)
    x = encode(geom, False, gid, pts, contract, tables=ww)
    dd = torch.from_numpy(d).double()
    grads = torch.autograd.grad(((dd.abs() if absolute else dd) * x).sum(), [ww[k] for k in names])
    return layout, [gr.numpy().reshape(-1) for gr in grads]


def _adjoint(rc, geom, gid, pts, d, flat, contract):
    names = [name for name, _, _ in rc.hashgrid_grad_layout(gid)[0]]
    tables = torch.cat([torch.from_numpy(weights_np(geom, False)[name]).reshape(-1) for name in names]).cuda()
    fwd = rc.hashgrid_lookup(gid, pts, apply_contraction=contract)
    lhs = float((fwd.double() * torch.from_numpy(d).cuda().double()).sum())
    rhs = float((tables.double() * flat.double()).sum())
    return lhs, rhs


@pytest.mark.parametrize("case", ["n=1", "n=33", "n=777", "faces", "uncontracted"])
@pytest.mark.parametrize("gid", [0, 1, 2, 3])
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_hashgrid_backward_against_fp64(geom, gid, case):
    """rc_hashgrid_backward against fp64 autograd of the oracle's encoding, per table, the same entries touched
    (assert_same_entries), and the adjoint identity <lookup(T), d> == <T, backward(d)> with the device's own lookup."""
    rc = handle(geom)
    pts, contract = _backward_points(geom, gid, case)
    n = len(pts)
    d = np.random.default_rng(32 + gid).normal(size=(n, grid(geom, gid).out_dim)).astype(np.float32)
    flat = rc.hashgrid_backward(gid, pts, d, apply_contraction=contract)
    layout, refs = _fp64_table_grads(geom, gid, pts, d, contract)
    got = flat.cpu().numpy().astype(np.float64)
    for (name, off, shape), ref in zip(layout, refs):
        a = got[off: off + ref.size]
        scale = max(1e-12, float(np.abs(ref).max()))
        # float32 trilinear weights at up to 2048 cells a side: a coordinate ulp is 1e-4 of a cell
        assert float(np.abs(a - ref).max()) <= 5e-4 * scale + 1e-7, (name, float(np.abs(a - ref).max()), scale)
        assert_same_entries(name, a, ref, n, grid(geom, gid).num_features)
    lhs, rhs = _adjoint(rc, geom, gid, pts, d, flat, contract)
    assert abs(lhs - rhs) <= 1e-4 * max(1.0, abs(lhs)), (lhs, rhs)


@pytest.mark.parametrize("gid", [0, 1, 2, 3])
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_hashgrid_backward_coincident_points(geom, gid):
    """256 copies of one point: every add of a level lands on the same 8 entries (LDS and global atomic pile-ups).  The
    point is dyadic, so every trilinear weight is exact in fp32; what is left is the rounding of the n-term sums, bounded
    by 2n eps times the sum of |term| an entry receives (2n: two corners of a hashed level may share an entry)."""
    rc = handle(geom)
    n = 256
    b = grid(geom, gid).bbox
    pts = np.tile(np.array([[0.3125, -0.5390625, 0.7578125]], np.float32) * np.float32(b), (n, 1))
    d = np.random.default_rng(60 + gid).normal(size=(n, grid(geom, gid).out_dim)).astype(np.float32)
    flat = rc.hashgrid_backward(gid, pts, d, apply_contraction=False)
    layout, refs = _fp64_table_grads(geom, gid, pts, d, False)
    _, absr = _fp64_table_grads(geom, gid, pts, d, False, absolute=True)
    got = flat.cpu().numpy().astype(np.float64)
    for (name, off, shape), ref, ab in zip(layout, refs, absr):
        a = got[off: off + ref.size]
        assert np.array_equal(a != 0.0, ref != 0.0), name
        assert np.all(np.abs(a - ref) <= (2 * n + 8) * EPS32 * np.abs(ab)), (name, float(np.abs(a - ref).max()))
        assert 8 * grid(geom, gid).num_features >= np.count_nonzero(ref) > 0, name


@pytest.mark.parametrize("gid", [0, 1])
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_scatter_at_batch_size_adjoint_and_level_sums(geom, gid):
    """The F = 1 scatter at batch scale (65 536 + 37 points: every sliced, small and generic workgroup of the plan busy):
    the adjoint identity with the device's own lookup, and per level sum of the table gradient == precondition * sum of
    d[:, level] (the eight trilinear weights of a point sum to one; the points stay inside the box, away from its faces,
    so no corner of a dense level is zero padding)."""
    cfg, g = CFGS[geom], grid(geom, gid)
    rc = handle(geom)
    n = 65536 + 37
    pts = np.clip(_points(n, 41, 0.25 * cfg.contract_radius), -0.9 * cfg.contract_radius, 0.9 * cfg.contract_radius)
    d = np.random.default_rng(42).normal(size=(n, g.out_dim)).astype(np.float32)
    layout, _ = rc.hashgrid_grad_layout(gid)
    flat = rc.hashgrid_backward(gid, pts, d)
    assert bool(torch.isfinite(flat).all())
    lhs, rhs = _adjoint(rc, geom, gid, pts, d, flat, True)
    assert abs(lhs - rhs) <= 2e-4 * max(1.0, abs(lhs)), (lhs, rhs)
    dsum = torch.from_numpy(d).double().sum(0).numpy()
    for l, (name, off, shape) in enumerate(layout):
        got = float(flat[off: off + int(np.prod(shape))].double().sum())
        want = float(g.precondition_scaling * dsum[l])
        assert abs(got - want) <= 2e-3 * max(1.0, float(np.abs(d[:, l]).sum()) * g.precondition_scaling * 1e-3), (name, got, want)


# ---------------------------------------------------------------------------------------------
# rc_density_backward, every level
# ---------------------------------------------------------------------------------------------
def _points_off_kinks(geom, level, n, seed=3, margin=2e-4):
    """Points (out to beyond the contraction radius: contracted coordinates past a unit box) whose hidden
    pre-activations all stay `margin` away from a ReLU kink in the fp64 oracle (test_train._points_off_kinks)."""
    cfg = CFGS[geom]
    pts = _points(2 * n + 64, seed, 0.6 * cfg.contract_radius)
    m = train_ref.relu_margin(weights_t(geom, True), cfg, level, torch.from_numpy(pts).double()).numpy()
    keep = np.nonzero(m > margin)[0][:n]
    assert len(keep) == n
    return np.ascontiguousarray(pts[keep])


@pytest.mark.parametrize("with_feature", [False, True])
@pytest.mark.parametrize("n", [1, 33, 1001])
@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_density_backward_against_fp64(geom, level, n, with_feature):
    """rc_density_backward (grid lookup, density MLP, k_density_bwd / k_wgrad, the table scatter) against
    train_ref.density_backward in fp64, odd batch sizes (k_wgrad pairs points along K), the bounds of
    test_train.test_density_backward_matches_oracle; the touched entries as in assert_same_entries (a 2048-cell level
    puts about one point in a thousand on a cell face in fp32 only)."""
    cfg = CFGS[geom]
    rc = handle(geom, smooth=True)
    pts = _points_off_kinks(geom, level, n, seed=5 + n)
    rng = np.random.Generator(np.random.PCG64(4 + n))
    dd = rng.normal(size=(n,)).astype(np.float32)
    df = (rng.normal(size=(n, 64)) * 0.1).astype(np.float32) if with_feature else None
    layout, total = rc.density_grad_layout(level)
    flat, dens = rc.density_backward(level, pts, dd, df)
    g, dens_ref, _ = train_ref.density_backward(weights_t(geom, True), cfg, level, torch.from_numpy(pts).double(),
                                                torch.from_numpy(dd).double(), None if df is None else torch.from_numpy(df).double())
    np.testing.assert_allclose(dens.cpu().numpy(), dens_ref.numpy(), rtol=2e-4, atol=1e-6)
    got = flat.cpu().numpy().astype(np.float64)
    assert total == sum(int(np.prod(s)) for _, _, s in layout)
    for name, off, shape in layout:
        b = g[name].double().numpy().reshape(-1)
        a = got[off: off + b.size]
        scale = max(1e-12, float(np.abs(b).max()))
        assert float(np.abs(a - b).max()) <= 5e-4 * scale + 1e-7, (name, float(np.abs(a - b).max()), scale)
        if "density_grid" in name:
            assert_same_entries(name, a, b, n, cfg.proposal_grids[level].num_features)


# ---------------------------------------------------------------------------------------------
# rc_render_rays, cache pass, on each launch plan
# ---------------------------------------------------------------------------------------------
CHECK_3 = ("diffuse_rgb", "specular_rgb", "direct_rgb", "indirect_rgb", "albedo_rgb", "indirect_diffuse_rgb",
           "indirect_specular_rgb", "indirect_occ")


@pytest.mark.parametrize("jitter_seed", [None, 7])
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_cache_render_against_the_oracle_on_every_plan(geom, jitter_seed):
    """The 256-ray cache pass against cache_ref in fp32 with the bounds of test_cache_render_256_vs_oracle_fp32, on
    rc_set_fused 0 (one kernel per stage), 2 (proposal levels through the level kernels where rc_level_supported: A and
    C) and 1.  Plan 1 is the fused kernel where fused_geometry_ok holds (C); elsewhere it falls back to the
    launch-per-stage plan with the level kernels (below 24 576 rays: plan 2's launches).  All three are bitwise equal."""
    cfg = CFGS[geom]
    rc = handle(geom, smooth=True)
    n = 256
    rays = nrc_amd.synthetic_rays(n, seed=20200823)
    rnd = None if jitter_seed is None else {"jitter": common.jitters(n, seed=jitter_seed)}
    res = {}
    try:
        for mode in (0, 2, 1):
            rc.set_fused(mode)
            o = rc.render_rays(rays.hot_fields(), rnd)
            torch.cuda.synchronize()
            res[mode] = {k: v.cpu().numpy() for k, v in o.items()}
    finally:
        rc.set_fused(1)
    for mode in (2, 1):
        for k in res[0]:
            assert np.array_equal(res[0][k], res[mode][k]), (mode, k)
    out = res[0]
    ref = common.oracle_cache(n, jitter_seed=jitter_seed, cfg=cfg, weights=weights_np(geom, True), want_grad_normals=False)
    r = {k: v.numpy() for k, v in ref["render"].items()}
    for k in ("rgb", "acc") + CHECK_3:
        assert np.abs(out[k] - r[k]).max() <= 1e-4, k
    for k in ("means", "normals_pred"):
        assert np.abs(out[k] - r[k]).max() <= 5e-4, k
    for k in ("ray_dists", "light_dists"):
        assert np.abs(out[k] - r[k][:, 0]).max() <= 5e-4, k
    for k in ("distance_mean", "distance_median", "distance_percentile_5", "distance_percentile_95"):
        assert np.abs(out[k] - r[k]).max() <= 1e-3, k
    assert float(out["acc"].max()) > 0.1


@pytest.mark.parametrize("n", [257, 24577])
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_level_kernels_equal_the_separate_kernels(geom, n):
    """test_gpu_abi_robustness.test_level_kernels_equal_the_separate_gather_and_mlp_kernels on this geometry: the lean
    resampling pass (every level density-only: k_level<4, 8, -1> on A) and secondary rays, on plans 0, 2 and 1 (from
    24 576 rays on plan 1 runs a proposal level with its sampling in front, k_level_ray): densities, fence posts and
    outputs bitwise equal.  On B no level kernel applies (a modulo table, 5 / 8 levels): all three plans are plan 0."""
    rc = handle(geom)
    rc.set_graph_mode(0)
    rays = nrc_amd.synthetic_rays(n, seed=31).hot_fields()
    jit = common.jitters(n, seed=9)
    srays, srnd = common.secondary_case(n, seed=12)
    g = np.random.default_rng(4).gumbel(size=(n, 32)).astype(np.float32)
    cases = [(rays, {"jitter": jit, "gumbel": g}, rc_ext.RC_PASS_CACHE | rc_ext.RC_PASS_RESAMPLE, ["rgb", "acc", "distance_median", "means"]),
             (srays, srnd, rc_ext.RC_PASS_CACHE | rc_ext.RC_PASS_SECONDARY | rc_ext.RC_PASS_NO_ENVMAP, ["rgb", "acc", "distance_mean"])]
    try:
        for fields, rnd, mask, outs in cases:
            res = {}
            for mode in (0, 2, 1):
                rc.set_fused(mode)
                o = rc.render_rays(fields, rnd, mask, outputs=outs)
                torch.cuda.synchronize()
                res[mode] = {k: v.cpu() for k, v in o.items()}
                for nm, cnt in (("density0", n * 64), ("density1", n * 64), ("density2", n * 32), ("tdist1", n * 65), ("tdist2", n * 33)):
                    res[mode][nm] = torch.from_numpy(rc.workspace(nm)[:cnt].copy())
            for mode in (2, 1):
                for k in res[0]:
                    assert torch.equal(res[0][k], res[mode][k]), (mask, mode, k)
            assert float(res[0]["density1"].abs().sum()) > 0.0 and bool(torch.isfinite(res[0]["rgb"]).all())
    finally:
        rc.set_fused(1)
        rc.set_graph_mode(1)


# ---------------------------------------------------------------------------------------------
# rc_interlevel_backward: the proposal levels' gradients
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["A", "B"], ids=GEOM_IDS)
def test_interlevel_whole_chain_against_fp64(geom):
    """test_gpu_interlevel.test_whole_chain_against_oracle on this geometry: HIP gradients of MLP_0 / MLP_1 vs
    train_ref.density_backward (fp64) at the HIP forward's means, fed d_density of the fp64 restatement; rays with a
    sample within 3e-5 of a ReLU kink are left out; the touched entries as in assert_same_entries."""
    cfg = CFGS[geom]
    il = nrc_amd.InterlevelConfig()
    S = [s for _, _, s in cfg.sampling_strategy]
    NP = cfg.num_levels - 1
    rc = handle(geom, smooth=True)
    n0 = 1500
    rays, jit = lc.cache_case(n0, seed=21)
    rc.interlevel_backward(rays, jit, 0.4, il.mults, il.blurs, levels=())
    _, _, _, means, _ = lc.interlevel_buffers(rc, n0)
    w64 = weights_t(geom, True)
    ok = np.ones(n0, bool)
    for l in range(NP):
        m = train_ref.relu_margin(w64, cfg, l, torch.from_numpy(means[l]).double()).numpy().reshape(n0, S[l])
        ok &= (m > 3e-5).all(axis=1)
    keep = np.nonzero(ok)[0]
    assert len(keep) >= 64, len(keep)
    rays = {k: np.ascontiguousarray(v[keep]) for k, v in rays.items()}
    jit = [np.ascontiguousarray(j[keep]) for j in jit]
    n = len(keep)
    g, _, losses = train.interlevel_grads(rc, rays, jit, 1.0)
    assert bool((losses > 0).all())
    sd, td, dens, means, dd = lc.interlevel_buffers(rc, n)
    _, d64 = ir.interlevel_forward_backward(sd, td, dens, rays["directions"], np.ones(n), il.mults, il.blurs, torch.float64)
    for l in range(NP):
        r = d64[l].numpy()
        differ = (dd[l] == 0.0) != (r == 0.0)
        assert float(np.abs(np.where(differ, r - dd[l], 0.0)).max()) <= 1e-6 * float(np.abs(r).max()), l
        layout, _ = rc.density_grad_layout(l)
        ref, _, _ = train_ref.density_backward(w64, cfg, l, torch.from_numpy(means[l]).double(),
                                               torch.from_numpy(np.where(differ, dd[l].astype(np.float64), r)).reshape(-1))
        for name, _, _ in layout:
            a, b = g[l][name].cpu().double().numpy(), ref[name].numpy()
            scale = max(1e-12, float(np.abs(b).max()))
            assert float(np.abs(a - b).max()) <= 5e-4 * scale + 1e-7, (name, float(np.abs(a - b).max()), scale)
            if "density_grid" in name:
                assert_same_entries(name, a, b, n * S[l], cfg.proposal_grids[l].num_features)
