"""rc_normals_backward on the GPU: the gradient through the analytic normals of the last level, every tensor of the
level-2 density layout against fp64 double-backward of the torch restatement (tests/geometry_smoothness_ref.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import common
import geometry_smoothness_ref as gs
import loss_cases as lc
import nrc_amd
from nrc_amd import train
from oracle import train_ref

CFG = nrc_amd.hotdog_config()
L2 = CFG.num_levels - 1
GUARD, SENTINEL, BIAS_FILL = 4096, 123.5, 1.25
SHAPES = (1, 31, 33, 129)          # a partial wave, two waves, a second workgroup holding one valid point

pytestmark = pytest.mark.gpu


def _kept_points():
    """The first 1 000 of 4 096 candidates N(0, 1.2^2) that are farther than 3e-5 from a ReLU kink (filter A) and farther
    than 1e-3 grid units from a cell face on every level (filter B: the trilinear Jacobian jumps there, and fp32 loc at
    N = 2048 carries about 2.4e-4).  The filters may leave out at most 10 % of the candidates."""
    rng = np.random.Generator(np.random.PCG64(61))
    cand = (rng.standard_normal((4096, 3)) * 1.2).astype(np.float32)
    m = train_ref.relu_margin(common.weights_torch(dtype=torch.float64), CFG, L2, torch.from_numpy(cand).double()).numpy()
    ok = (m > 3e-5) & (gs.cell_face_margin(cand) > 1e-3)
    print("share of the candidates kept:", ok.mean())
    assert ok.mean() >= 0.9, ok.mean()
    keep = np.nonzero(ok)[0][:1000]
    assert len(keep) == 1000
    pts = cand[keep]
    outside = float((np.linalg.norm(pts, axis=-1) > CFG.contract_radius).mean())
    assert 0.2 < outside < 0.7, outside                         # both branches of the contraction's Jacobian
    return pts, rng.standard_normal((1000, 3)).astype(np.float32)


def _fresh_flat(rc):
    """Zeros over the layout with the bias segments at BIAS_FILL, and a guard band of SENTINEL behind it."""
    layout, total = rc.density_grad_layout(L2)
    big = torch.zeros(total + GUARD, dtype=torch.float32, device="cuda")
    big[total:] = SENTINEL
    for name, off, shape in layout:
        if name.endswith("/bias"):
            big[off: off + int(np.prod(shape))] = BIAS_FILL
    return big, big[:total], layout


def _run(rc, pts, v):
    big, flat, layout = _fresh_flat(rc)
    _, normals = rc.normals_backward(pts, v, flat)
    torch.cuda.synchronize()
    assert bool((big[flat.numel():] == SENTINEL).all())         # nothing written beyond the layout
    return {k: t.cpu().numpy() for k, t in train.grads_as_dict(flat, layout).items()}, normals.cpu().numpy(), flat


def _compare(rc, got, normals, pts, v, what):
    """Every tensor of the layout within 3x the fp32 restatement's own distance from fp64 plus 2e-3 of the tensor's scale
    (the project's whole-chain form); the tables' support; the bias segments untouched; the normals by lc.check's rule."""
    w = common.weights_np()
    r64, n64 = gs.normals_backward(w, pts, v, torch.float64)
    r32, n32 = gs.normals_backward(w, pts, v, torch.float32)
    layout = rc.density_grad_layout(L2)[0]
    tables = 0
    for name, _, _ in layout:
        a = got[name].astype(np.float64)
        if name.endswith("/bias"):
            assert np.all(got[name] == np.float32(BIAS_FILL)), name
            assert not r64[name].any(), name                    # and the restatement's gradient is an exact zero
            continue
        r, r32n = r64[name], r32[name].astype(np.float64)
        scale = float(np.abs(r).max())
        assert scale > 0, name
        err, err32 = float(np.abs(a - r).max()), float(np.abs(r32n - r).max())
        print(what, name, "err", err, "err32", err32, "scale", scale)
        assert err <= 3.0 * err32 + 2e-3 * scale, (what, name, err, err32, scale)
        if "_grid/" in name:
            tables += 1
            only = (a != 0.0) != (r != 0.0)
            assert np.count_nonzero(only) <= 1e-4 * np.count_nonzero(r), (name, np.count_nonzero(only))
    assert tables == len(rc.hashgrid_grad_layout(L2)[0]) == 8
    lc.check(normals.astype(np.float64), n64, n32.astype(np.float64), what + " normals")


@pytest.fixture(scope="module")
def case():
    rc = common.make_rc()
    pts, v = _kept_points()
    got, normals, flat = _run(rc, pts, v)
    rows = {k: rc.workspace("nb:" + k)[: 1000 * width].reshape(1000, width).copy()
            for k, width in (("u", 32), ("t0", 64), ("a0", 64), ("t1", 64), ("a2", 64), ("ghat", 3))}
    return dict(rc=rc, pts=pts, v=v, got=got, normals=normals, flat=flat.clone(), rows=rows)


def test_every_tensor_against_fp64(case):
    _compare(case["rc"], case["got"], case["normals"], case["pts"], case["v"], "n=1000")


@pytest.mark.parametrize("n", SHAPES)
def test_shapes_where_the_kernel_can_go_wrong(case, n):
    """The first n kept points as a call of their own: against fp64 as above, nothing written beyond the layout (the guard
    band), and the per-point arrays the MLP segments are contracted from -- u, t0, a0, t1, a2 -- with G^ and the normals
    bitwise the rows of the same points inside the 1 000-point call.  (The segments themselves are sums over the call's
    points in an order fixed by its size, so a restriction of the large call has no segment to compare with.)"""
    rc, pts, v = case["rc"], case["pts"][:n], case["v"][:n]
    got, normals, _ = _run(rc, pts, v)
    for k, big in case["rows"].items():
        mine = rc.workspace("nb:" + k)[: n * big.shape[1]].reshape(n, -1)
        assert np.array_equal(mine, big[:n]), k
    assert np.array_equal(normals, case["normals"][:n])
    _compare(rc, got, normals, pts, v, f"n={n}")


def test_semantics(case):
    rc, pts, v = case["rc"], case["pts"], case["v"]
    _, _, f1 = _run(rc, pts, v)
    assert torch.equal(lc.mlp_part(rc, f1, 0), lc.mlp_part(rc, case["flat"], 0))      # bitwise stable across calls
    first = f1.clone()
    layout = rc.density_grad_layout(L2)[0]
    for name, off, shape in layout:                            # the doubling below starts from zeroed bias segments
        if name.endswith("/bias"):
            f1[off: off + int(np.prod(shape))] = 0.0
            first[off: off + int(np.prod(shape))] = 0.0
    rc.normals_backward(pts, v, f1)                            # accumulates: a second call doubles
    torch.cuda.synchronize()
    assert torch.equal(lc.mlp_part(rc, f1, 0), 2 * lc.mlp_part(rc, first, 0))
    ref = 2 * first.cpu().numpy()
    np.testing.assert_allclose(f1.cpu().numpy(), ref, rtol=1e-5, atol=1e-6 * float(np.abs(ref).max()))
    # n == 0 writes nothing
    big, flat, _ = _fresh_flat(rc)
    before = big.clone()
    rc.normals_backward(pts[:0], v[:0], flat)
    torch.cuda.synchronize()
    assert torch.equal(big, before)
    # NULL arguments and n < 0
    p, d = torch.from_numpy(pts).cuda(), torch.from_numpy(v).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda *a: rc.lib.rc_normals_backward(rc._h, *a, None, stream)
    assert call(None, 1000, d.data_ptr(), flat.data_ptr()) == -1
    assert call(p.data_ptr(), 1000, None, flat.data_ptr()) == -1
    assert call(p.data_ptr(), 1000, d.data_ptr(), None) == -1
    assert call(p.data_ptr(), -1, d.data_ptr(), flat.data_ptr()) == -1
    assert call(p.data_ptr(), 0, d.data_ptr(), flat.data_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(big, before)
