"""rc_query_cache_diffuse on the GPU against the oracle composed from oracle/cache_ref: the last sampler
level's hidden feature (density_mlp's "feature"), the appearance grid's encoding at the contracted point, and the shader's
two view-independent heads, clip(softplus(Dense(96 -> 3) + bias), 0, rgb_max), in fp64 and in fp32.

Bound (the project's rule, loss_cases.check): the HIP error against fp64 is at most 3x the fp32 restatement's own error
against fp64 plus 1e-6 of the tensor's scale, no point left out.  The points are the 257 of tests/test_gpu_query_points.py:
129 inside the unit box, 128 drawn wide, a dozen or more beyond the contracted box -- where, like the launch-per-stage
plan's shader, the heads are not gated."""
import numpy as np
import pytest
import torch

import common
import loss_cases as lc
import nrc_amd
from nrc_amd import mesh, rc_ext
from oracle import cache_ref, hashgrid_ref, mathx
from test_gpu_query_points import N, gated, points

gpu = pytest.mark.gpu
CFG = nrc_amd.hotdog_config()
RC_ERR_INVALID_ARG, RC_ERR_UNSUPPORTED = -1, -5

_ORACLE = {}


def oracle(dtype):
    """[N, 6] = ambient_diffuse rgb, indirect_diffuse rgb of the oracle at points() in `dtype`, computed once."""
    if dtype not in _ORACLE:
        w = common.to_torch(common.weights_material_np(), dtype)
        p = torch.from_numpy(points()).to(dtype)
        rays = {"origins": torch.zeros(N, 3, dtype=dtype), "lights": torch.zeros(N, 3, dtype=dtype)}
        hidden = cache_ref.density_mlp(w, CFG, CFG.num_levels - 1, rays, p[:, None, :], want_grad_normals=False)["feature"][:, 0]
        app = hashgrid_ref.hash_encoding(w, "params/Cache/Shader/appearance_grid", CFG.appearance_grid,
                                         mathx.contract_radius(p, CFG.contract_radius))
        feature = torch.cat([hidden, app], dim=-1)
        assert feature.shape == (N, 96)
        head = lambda layer, bias: torch.clamp(mathx.softplus(cache_ref.dense(w, f"Cache/Shader/{layer}", feature) + bias), 0.0, CFG.rgb_max)
        _ORACLE[dtype] = torch.cat([head("ambient_irradiance_layer", CFG.ambient_irradiance_bias),
                                    head("irradiance_layer", CFG.irradiance_bias)], dim=-1).numpy()
    return _ORACLE[dtype]


def test_oracle_is_the_shaders_own_value():
    """The composition above is what cache_ref.cache_shader calls ambient_diffuse_rgb / indirect_diffuse_rgb (fp64)."""
    dtype = torch.float64
    w = common.to_torch(common.weights_material_np(), dtype)
    p = torch.from_numpy(points()).to(dtype)
    rays = {"origins": torch.zeros(N, 3, dtype=dtype), "lights": torch.zeros(N, 3, dtype=dtype),
            "viewdirs": torch.nn.functional.normalize(torch.ones(N, 3, dtype=dtype), dim=-1)}
    sres = cache_ref.density_mlp(w, CFG, CFG.num_levels - 1, rays, p[:, None, :], want_grad_normals=False)
    sres["means"] = p[:, None, :]
    sh = cache_ref.cache_shader(w, CFG, rays, sres)
    got = oracle(dtype)
    keys = [k for k in sh if "ambient_diffuse" in k] + [k for k in sh if "indirect_diffuse" in k]
    assert len(keys) == 2, sorted(sh)
    assert np.array_equal(sh[keys[0]][:, 0].numpy(), got[:, :3]) and np.array_equal(sh[keys[1]][:, 0].numpy(), got[:, 3:])
    assert gated(dtype).sum() >= 12 and np.all(got[gated(dtype)] > 0)          # no gate beyond the contracted box
    assert got.std() > 1e-3                                                   # the heads vary over the points


@pytest.fixture(scope="module")
def rc():
    return common.make_rc(weights=common.weights_material_np())


@gpu
def test_diffuse_heads_against_the_oracle(rc):
    got = rc.query_cache_diffuse(points())
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    r64, r32 = oracle(torch.float64), oracle(torch.float32)
    assert got.shape == (N, 6) and got.dtype == np.float32
    for name, cols in (("ambient_diffuse", slice(0, 3)), ("indirect_diffuse", slice(3, 6))):
        err, err32 = np.abs(got[:, cols] - r64[:, cols]).max(), np.abs(r32[:, cols] - r64[:, cols]).max()
        print(name, "err", err, "fp32 restatement", err32, "scale", np.abs(r64[:, cols]).max())
        lc.check(got[:, cols].astype(np.float64), r64[:, cols], r32[:, cols].astype(np.float64), name)


@gpu
def test_call_size_and_keys(rc):
    p = torch.from_numpy(points()).cuda()
    whole = rc.query_cache_diffuse(p)
    parts = torch.cat([rc.query_cache_diffuse(p[:100]), rc.query_cache_diffuse(p[100:])])
    assert torch.equal(whole, parts)                                          # 257 at once equal 100 + 157
    q = mesh.query_points(rc, p, ("ambient_diffuse", "cache_diffuse", "indirect_diffuse", "density"))
    assert torch.equal(q["ambient_diffuse"], whole[:, :3]) and torch.equal(q["indirect_diffuse"], whole[:, 3:])
    assert torch.equal(q["cache_diffuse"], whole[:, :3] + whole[:, 3:])
    assert torch.equal(q["density"], rc.query_points(p, ("density",))["density"])
    big = torch.cat([p] * 512)[: 131072 + 77]                                 # more than one chunk
    assert torch.equal(rc.query_cache_diffuse(big)[-257:], rc.query_cache_diffuse(big[-257:]))


@gpu
def test_error_codes_and_the_time_resolved_handle(rc):
    p = torch.from_numpy(points()).cuda()
    out = torch.full((N, 6), -7.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    call = lambda h, pts, n, o=out: h.lib.rc_query_cache_diffuse(h._h, pts, n, None if o is None else o.data_ptr(), st)
    assert call(rc, p.data_ptr(), -1) == RC_ERR_INVALID_ARG and call(rc, None, N) == RC_ERR_INVALID_ARG
    assert call(rc, None, 0) == 0 and call(rc, p.data_ptr(), N, None) == 0    # n == 0 / no output: nothing launched
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    tr = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    tr.load_weights(common.weights_transient_np())
    assert call(tr, p.data_ptr(), N) == RC_ERR_UNSUPPORTED
    with pytest.raises(rc_ext.RcError) as e:
        mesh.query_points(tr, p, ("cache_diffuse",))
    assert e.value.code == RC_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
