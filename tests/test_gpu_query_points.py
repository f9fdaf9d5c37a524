"""rc_query_points and rc_density_lattice on the GPU against the oracle: density of every sampler level
(oracle/train_ref.py's forward), the last level's predicted and analytic normals (oracle/cache_ref.density_mlp) and the
material head (oracle/material_ref.material_mlp), each in fp64 and in fp32.

Bound (the project's rule, tests/test_gpu_transient_sampler.py -> loss_cases.check): the HIP error against fp64 is at most
3x the fp32 restatement's own error against fp64 plus 1e-6 of the tensor's scale, per output, no point left out -- except,
for the analytic normals, the points closer than 3e-5 to a ReLU kink (oracle/train_ref.relu_margin; the threshold of
tests/test_gpu_normals_backward.py), at most 5 % of them.

257 points (no multiple of 32 or 64): 129 inside the unit box, 128 drawn wide, so the contraction and the gate of the
contracted box are in play; at least a dozen lie beyond the contracted box, where the density must be exactly 0.
test_points_meet_their_conditions_on_the_oracle holds the seed to all of that on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import common
import iso_ref
import loss_cases as lc
import nrc_amd
from nrc_amd import mesh, rc_ext
from oracle import cache_ref, material_ref, mathx, train_ref

gpu = pytest.mark.gpu
CFG = nrc_amd.hotdog_config()
NL = CFG.num_levels
L2 = NL - 1
N = 257
MARGIN = 3e-5
RC_ERR_INVALID_ARG, RC_ERR_MISSING_WEIGHT, RC_ERR_UNSUPPORTED = -1, -3, -5


def points():
    rng = np.random.Generator(np.random.PCG64(2024))
    inside = rng.uniform(-0.95, 0.95, size=(129, 3))
    wide = rng.standard_normal((N - 129, 3)) * 2.5
    return np.concatenate([inside, wide]).astype(np.float32)


_ORACLE = {}


def oracle(dtype):
    """{"density<l>", "normals", "normals_pred", "material"} of the oracle at points() in `dtype` (numpy), computed once."""
    if dtype not in _ORACLE:
        w = common.to_torch(common.weights_material_np(), dtype)
        p = torch.from_numpy(points()).to(dtype)
        out = {}
        for l in range(NL):
            out[f"density{l}"] = train_ref.density_backward(w, CFG, l, p, torch.zeros(N, dtype=dtype))[1].numpy()
        rays = {"origins": torch.zeros(N, 3, dtype=dtype), "lights": torch.zeros(N, 3, dtype=dtype)}
        last = cache_ref.density_mlp(w, CFG, L2, rays, p[:, None, :])
        out["normals"] = last["normals"][:, 0].detach().numpy()
        out["normals_pred"] = last["normals_pred"][:, 0].detach().numpy()
        assert np.array_equal(last["density"][:, 0].numpy(), out[f"density{L2}"])
        m = material_ref.material_mlp(w, CFG, p)
        out["material"] = torch.cat([m["albedo"], m["roughness"], m["metalness"]], dim=-1).numpy()
        _ORACLE[dtype] = out
    return _ORACLE[dtype]


def kept_for_normals():
    w64 = common.to_torch(common.weights_material_np(), torch.float64)
    m = train_ref.relu_margin(w64, CFG, L2, torch.from_numpy(points()).double()).numpy()
    return m >= MARGIN


def gated(dtype):
    """Points beyond the contracted box of level `l`'s grid (the same box on every level of this config)."""
    warped = mathx.contract_radius(torch.from_numpy(points()).to(dtype), CFG.contract_radius)
    b = CFG.proposal_grids[L2].bbox
    return ~((warped > -b) & (warped < b)).all(dim=-1).numpy()


def test_points_meet_their_conditions_on_the_oracle():
    p = points()
    assert p.shape == (N, 3) and N % 32 != 0
    assert {g.bbox for g in CFG.proposal_grids} == {CFG.proposal_grids[L2].bbox}
    out = gated(torch.float64)
    assert np.array_equal(out, gated(torch.float32))                  # no point sits within rounding of the box
    assert out.sum() >= 12 and (~out).sum() >= 129, out.sum()
    assert (np.abs(p) > 1.0).any(axis=1).sum() >= 64                  # beyond the unit box: the contraction is in play
    for l in range(NL):
        d = oracle(torch.float64)[f"density{l}"]
        assert np.all(d[out] == 0.0) and np.all(d[~out] > 0.0), l
    keep = kept_for_normals()
    print("points left out of the analytic normals:", int((~keep).sum()), "of", N)
    assert (~keep).mean() <= 0.05, (~keep).mean()


@pytest.fixture(scope="module")
def rc():
    return common.make_rc(weights=common.weights_material_np())


@pytest.fixture(scope="module")
def got(rc):
    p = torch.from_numpy(points()).cuda()
    out = {f"density{l}": rc.query_points(p, ("density",), l)["density"] for l in range(NL)}
    out.update(rc.query_points(p, ("density", "normals_pred", "normals", "material")))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@gpu
@pytest.mark.parametrize("key", [f"density{l}" for l in range(NL)] + ["normals_pred", "material"])
def test_fields_against_the_oracle(got, key):
    r64, r32 = oracle(torch.float64)[key], oracle(torch.float32)[key]
    assert got[key].shape == r64.shape
    err, err32 = np.abs(got[key] - r64).max(), np.abs(r32 - r64).max()
    print(key, "err", err, "fp32 restatement", err32, "scale", np.abs(r64).max())
    lc.check(got[key].astype(np.float64), r64, r32.astype(np.float64), key)


@gpu
def test_density_is_zero_beyond_the_contracted_box(got):
    out = gated(torch.float64)
    for l in range(NL):
        assert np.all(got[f"density{l}"][out] == 0.0) and np.all(got[f"density{l}"][~out] > 0.0), l
    assert np.array_equal(got["density"], got[f"density{L2}"])         # level None is the last; with or without the other outputs


@gpu
def test_analytic_normals_against_the_oracle(got):
    keep = kept_for_normals()
    assert (~keep).mean() <= 0.05
    r64, r32 = oracle(torch.float64)["normals"][keep], oracle(torch.float32)["normals"][keep]
    g = got["normals"][keep].astype(np.float64)
    print("normals err", np.abs(g - r64).max(), "fp32 restatement", np.abs(r32 - r64).max(), "kept", int(keep.sum()))
    lc.check(g, r64, r32.astype(np.float64), "normals")


def lattice_points(lo, hi, dims):
    axes = [iso_ref.lattice_axis(lo[a], hi[a], dims[a])[0] for a in range(3)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)


@gpu
@pytest.mark.parametrize("lo,hi,dims", [((-0.9, -0.8, -0.7), (0.8, 0.9, 0.6), (5, 6, 7)),
                                        ((-3.0, -2.5, -4.0), (3.0, 2.5, 4.0), (3, 3, 40))])
@pytest.mark.parametrize("level", [None, 0])
def test_lattice_equals_the_query_at_its_points(rc, lo, hi, dims, level):
    """Both calls go through the same two launches per chunk, so the lattice is the query bit for bit (nan_to_num
    applied); the lattice's coordinates are the fp32 formula exactly (read from the workspace: one chunk holds it all)."""
    f = mesh.density_lattice(rc, lo, hi, dims, level)
    torch.cuda.synchronize()
    assert tuple(f.shape) == dims and f.dtype == torch.float32
    p = lattice_points(lo, hi, dims)
    soa = rc.workspace("q:means").reshape(3, -1)
    assert np.array_equal(soa.T, p)
    q = mesh.query_points(rc, p, ("density",), level)["density"]
    assert torch.equal(f.reshape(-1), torch.nan_to_num(q))
    assert bool(torch.isfinite(f).all())
    if max(np.abs(hi)) > 2.0:
        assert int((f == 0).sum()) > 0 and int((f > 0).sum()) > 0      # the box reaches beyond the gate


@gpu
def test_mesh_query_splits_the_material_row(rc, got):
    out = mesh.query_points(rc, points(), ("albedo", "roughness", "metalness", "density"))
    assert np.array_equal(out["albedo"].cpu().numpy(), got["material"][:, 0:3])
    assert np.array_equal(out["roughness"].cpu().numpy(), got["material"][:, 3])
    assert np.array_equal(out["metalness"].cpu().numpy(), got["material"][:, 4])
    assert np.array_equal(out["density"].cpu().numpy(), got["density"])
    with pytest.raises(ValueError):
        mesh.query_points(rc, points(), ("rgb",))


@gpu
def test_chunks_do_not_show(rc):
    """More points than one chunk of 131 072: the rows of the first 257 are those of the small call."""
    p = np.concatenate([points()] * 512)[: 131072 + 77]
    big = rc.query_points(p, ("density", "normals", "material"))
    small = rc.query_points(p[-300:], ("density", "normals", "material"))
    for k in big:
        assert torch.equal(big[k][-300:], small[k]), k


@gpu
def test_error_codes(rc):
    p = torch.from_numpy(points()).cuda()
    d = torch.empty(N, device="cuda")
    n3 = torch.empty(N, 3, device="cuda")
    m5 = torch.full((N, 5), -7.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    q = lambda h, pts, n, level, dens=None, npred=None, nrm=None, mat=None: h.lib.rc_query_points(
        h._h, pts, n, level, None if dens is None else dens.data_ptr(), None if npred is None else npred.data_ptr(),
        None if nrm is None else nrm.data_ptr(), None if mat is None else mat.data_ptr(), st)
    assert q(rc, p.data_ptr(), N, -1, d) == 0
    assert q(rc, p.data_ptr(), -1, -1, d) == RC_ERR_INVALID_ARG
    assert q(rc, None, N, -1, d) == RC_ERR_INVALID_ARG
    assert q(rc, p.data_ptr(), N, NL, d) == RC_ERR_INVALID_ARG
    assert q(rc, p.data_ptr(), N, 0, d, npred=n3) == RC_ERR_UNSUPPORTED
    assert q(rc, p.data_ptr(), N, 1, d, nrm=n3) == RC_ERR_UNSUPPORTED
    d.fill_(-7.0)
    assert q(rc, None, 0, -1, d) == 0                                  # n == 0: nothing launched
    torch.cuda.synchronize()
    assert bool((d == -7.0).all())
    cache_only = common.make_rc()
    assert q(cache_only, p.data_ptr(), N, -1, d, mat=m5) == RC_ERR_MISSING_WEIGHT
    assert q(cache_only, p.data_ptr(), N, -1, d) == 0
    torch.cuda.synchronize()
    assert bool((m5 == -7.0).all())
    # the lattice
    f = torch.empty(8 * 8 * 8, device="cuda")
    vec = lambda v: (C.c_float * 3)(*v)
    lat = lambda lo, hi, dims, level=-1: rc.lib.rc_density_lattice(rc._h, vec(lo), vec(hi), *dims, level, f.data_ptr(), st)
    assert lat((-1, -1, -1), (1, 1, 1), (8, 8, 8)) == 0
    assert lat((-1, -1, -1), (1, 1, 1), (1, 8, 8)) == RC_ERR_INVALID_ARG
    assert lat((-1, -1, -1), (1, 1, 1), (2, 1025, 2)) == RC_ERR_INVALID_ARG
    assert lat((-1, -1, -1), (1, -1, 1), (8, 8, 8)) == RC_ERR_INVALID_ARG
    assert lat((-1, -1, 2), (1, 1, 1), (8, 8, 8)) == RC_ERR_INVALID_ARG
    assert lat((-1, -1, -1), (1, 1, 1), (8, 8, 8), NL) == RC_ERR_INVALID_ARG
    torch.cuda.synchronize()


@gpu
def test_time_resolved_handle():
    """Accepted for density and both normals (its sampler uses the same density fields), refused for the material."""
    tcfg = nrc_amd.cornell_transient_config()
    wt = common.weights_transient_np()
    tr = rc_ext.RadianceCache(tcfg, 0)
    tr.load_weights(wt)
    p = (points() * 2.0).astype(np.float32)
    out = tr.query_points(p, ("density", "normals_pred", "normals"))
    torch.cuda.synchronize()
    refs = [train_ref.density_backward(common.to_torch(wt, dt), tcfg, tcfg.num_levels - 1, torch.from_numpy(p).to(dt),
                                       torch.zeros(N, dtype=dt))[1].numpy() for dt in (torch.float64, torch.float32)]
    lc.check(out["density"].cpu().numpy().astype(np.float64), refs[0], refs[1].astype(np.float64), "transient density")
    assert bool(torch.isfinite(out["normals"]).all()) and bool(torch.isfinite(out["normals_pred"]).all())
    with pytest.raises(rc_ext.RcError) as e:
        tr.query_points(p, ("material",))
    assert e.value.code == RC_ERR_UNSUPPORTED
    f = tr.density_lattice((-2, -2, -2), (2, 2, 2), (4, 5, 6))
    assert torch.equal(f.reshape(-1), torch.nan_to_num(tr.query_points(lattice_points((-2, -2, -2), (2, 2, 2), (4, 5, 6)))["density"]))
