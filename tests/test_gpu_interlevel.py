"""rc_interlevel_backward on the GPU: the spline interlevel loss of the proposal samplers and the gradients of both
proposal networks, against the torch restatement (tests/interlevel_ref.py) and the fp64 density-backward oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

import common
import interlevel_ref as ir
import loss_cases as lc
import nrc_amd
from nrc_amd import train
from oracle import train_ref

CFG = nrc_amd.hotdog_config()
IL = nrc_amd.InterlevelConfig()
S = [s for _, _, s in CFG.sampling_strategy]
NP = CFG.num_levels - 1

pytestmark = pytest.mark.gpu


def test_kernel_against_restatement():
    """Losses and d loss / d density within 3x the fp32 restatement's distance from fp64, on the HIP forward's buffers
    (loss_cases.interlevel_compare)."""
    rc = common.make_rc()
    n = 1000
    rays, jit = lc.cache_case(n)
    lm = lc.lossmult(n)
    _, losses = rc.interlevel_backward(rays, jit, 0.4, IL.mults, IL.blurs, lossmult=lm, levels=())
    lc.interlevel_compare(rc, n, rays, lm, losses.cpu().numpy(), IL.mults, IL.blurs)


def test_forward_matches_the_render_workspace():
    """The training forward's per-level buffers are bitwise those of a launch-per-stage render at anneal 0.4, on the
    per-stage (1000 rays) and the per-ray level-kernel (>= 24 576 rays) forms of the plan."""
    for n in (1000, 24577):
        rays, jit = lc.cache_case(n, seed=11)
        rc = common.make_rc()
        rc.interlevel_backward(rays, jit, 0.4, IL.mults, IL.blurs, levels=())
        torch.cuda.synchronize()
        rc.set_fused(False)
        rc.render_rays(rays, {"jitter": jit}, outputs=["acc"])
        torch.cuda.synchronize()
        for l in range(NP + 1):
            for name in ("sdist", "tdist", "means", "density"):
                a, b = rc.workspace(f"i:{name}{l}"), rc.workspace(f"{name}{l}")
                assert a.shape == b.shape and np.array_equal(a, b), (n, name, l)
        for l in range(NP):
            assert np.array_equal(rc.workspace(f"i:weights{l}"), rc.workspace(f"weights{l}")), (n, l)


def test_whole_chain_against_oracle():
    """HIP gradients of MLP_0 / MLP_1 vs train_ref.density_backward (fp64) at the HIP forward's means, fed d_density of
    the fp64 restatement.  Rays whose samples sit within 3e-5 of a ReLU kink (where fp32 and fp64 may take different
    sides) are left out: each ray's forward is independent of the others, so the subset's buffers are the same bits."""
    rc = common.make_rc()
    rays, jit = lc.cache_case(1500, seed=21)
    rc.interlevel_backward(rays, jit, 0.4, IL.mults, IL.blurs, levels=())
    _, _, _, means, _ = lc.interlevel_buffers(rc, 1500)
    w64 = common.weights_torch(dtype=torch.float64)
    ok = np.ones(1500, bool)
    for l in range(NP):
        m = train_ref.relu_margin(w64, CFG, l, torch.from_numpy(means[l]).double()).numpy().reshape(1500, S[l])
        ok &= (m > 3e-5).all(axis=1)
    keep = np.nonzero(ok)[0]
    assert len(keep) >= 64, len(keep)
    rays = {k: np.ascontiguousarray(v[keep]) for k, v in rays.items()}
    jit = [np.ascontiguousarray(j[keep]) for j in jit]
    n = len(keep)
    g, flats, _ = train.interlevel_grads(rc, rays, jit, 1.0)
    sd, td, dens, means, dd = lc.interlevel_buffers(rc, n)
    _, d64 = ir.interlevel_forward_backward(sd, td, dens, rays["directions"], np.ones(n), IL.mults, IL.blurs, torch.float64)
    for l in range(NP):
        # a sample whose upstream is exactly 0 on one side (every term at and behind it truncated by max(0, .)) may carry
        # a vanishing one on the other where a term sits at the truncation: such upstreams must be negligible, and the
        # oracle takes the HIP value there so that both sides touch the same table entries
        r = d64[l].numpy()
        differ = (dd[l] == 0.0) != (r == 0.0)
        assert float(np.abs(np.where(differ, r - dd[l], 0.0)).max()) <= 1e-6 * float(np.abs(r).max()), l
        layout, _ = rc.density_grad_layout(l)
        ref, _, _ = train_ref.density_backward(w64, CFG, l, torch.from_numpy(means[l]).double(),
                                               torch.from_numpy(np.where(differ, dd[l].astype(np.float64), r)).reshape(-1))
        for name, _, _ in layout:
            a, b = g[l][name].cpu().double().numpy(), ref[name].numpy()
            scale = max(1e-12, float(np.abs(b).max()))
            assert float(np.abs(a - b).max()) <= 5e-4 * scale + 1e-7, (name, float(np.abs(a - b).max()), scale)
            if "density_grid" in name:
                # the same entries are touched, up to corners whose trilinear weight is 0 in one precision only (a sample
                # on a cell face): those carry nothing
                only = (a != 0.0) != (b != 0.0)
                assert np.count_nonzero(only) <= 1e-4 * np.count_nonzero(b), (name, np.count_nonzero(only))
                assert float(np.abs(np.where(only, a - b, 0.0)).max()) <= 1e-6 * scale, name


def _mlp_offset(rc, level):
    layout, _ = rc.density_grad_layout(level)
    return next(o for name, o, _ in layout if name.endswith("density_layers_0/kernel"))


def test_semantics():
    rc = common.make_rc()
    n = 777
    rays, jit = lc.cache_case(n, seed=31)
    lm = lc.lossmult(n, seed=32)
    f1, l1 = rc.interlevel_backward(rays, jit, 0.3, IL.mults, IL.blurs, lossmult=lm)
    f1 = [f.clone() for f in f1]
    l1 = l1.clone()
    # bitwise stable: losses and MLP gradients
    f2, l2 = rc.interlevel_backward(rays, jit, 0.3, IL.mults, IL.blurs, lossmult=lm)
    assert torch.equal(l1, l2)
    for l in range(NP):
        o = _mlp_offset(rc, l)
        assert torch.equal(f1[l][o:], f2[l][o:])
        assert float(f1[l].abs().max()) > 0
    # linear in mults, losses too
    f3, l3 = rc.interlevel_backward(rays, jit, 0.3, tuple(2 * m for m in IL.mults), IL.blurs, lossmult=lm)
    for l in range(NP):
        ref = 2 * f1[l].cpu().numpy()       # table entries: float atomics, order-dependent in the last bits
        np.testing.assert_allclose(f3[l].cpu().numpy(), ref, rtol=1e-5, atol=1e-6 * float(np.abs(ref).max()))
    np.testing.assert_allclose(l3.cpu().numpy(), 2 * l1.cpu().numpy(), rtol=1e-6)
    # accumulates into given buffers
    acc = [f.clone() for f in f1]
    rc.interlevel_backward(rays, jit, 0.3, IL.mults, IL.blurs, lossmult=lm, grads=acc)
    for l in range(NP):
        ref = 2 * f1[l].cpu().numpy()
        np.testing.assert_allclose(acc[l].cpu().numpy(), ref, rtol=1e-5, atol=1e-6 * float(np.abs(ref).max()))
    # lossmult 0 rays: d_density 0
    dd = [rc.workspace(f"i:d_density{l}")[: n * S[l]].reshape(n, S[l]) for l in range(NP)]
    for l in range(NP):
        assert np.all(dd[l][lm == 0.0] == 0.0) and np.any(dd[l][lm > 0.0] != 0.0)
    # a NULL grads[l] skips only that level
    z = [torch.zeros_like(f) for f in f1]
    fs, ls = rc.interlevel_backward(rays, jit, 0.3, IL.mults, IL.blurs, lossmult=lm, grads=z, levels=(1,))
    assert fs[0] is None and float(z[0].abs().max()) == 0.0
    o = _mlp_offset(rc, 1)
    assert torch.equal(fs[1][o:], f1[1][o:]) and torch.equal(ls, l1)
    # a non-default stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        f4, l4 = rc.interlevel_backward(rays, jit, 0.3, IL.mults, IL.blurs, lossmult=lm)
    s.synchronize()
    assert torch.equal(l4, l1)
    for l in range(NP):
        assert torch.equal(f4[l][_mlp_offset(rc, l):], f1[l][_mlp_offset(rc, l):])
    # anneal reaches the sampler: a different anneal moves the samples
    rc.interlevel_backward(rays, jit, 0.0, IL.mults, IL.blurs, levels=())
    sd0 = rc.workspace("i:sdist1").copy()
    rc.interlevel_backward(rays, jit, 0.4, IL.mults, IL.blurs, levels=())
    assert not np.array_equal(sd0, rc.workspace("i:sdist1"))
    # n = 0
    empty = {k: v[:0] for k, v in rays.items()}
    fe, le = rc.interlevel_backward(empty, [j[:0] for j in jit], 0.4, IL.mults, IL.blurs)
    assert float(le.abs().max()) == 0.0 and all(float(f.abs().max()) == 0.0 for f in fe)


def test_bad_arguments():
    rc = common.make_rc()
    n = 64
    rays, _ = lc.cache_case(n)
    r, held, _ = rc._rays_struct(rays)
    lib = rc.lib
    losses = torch.zeros(NP, device="cuda")
    fl = lambda *v: (C.c_float * NP)(*v)
    good_m, good_b = fl(*IL.mults), fl(*IL.blurs)
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda rays_p=C.byref(r), nn=n, anneal=0.4, m=good_m, b=good_b, out=losses.data_ptr(): \
        lib.rc_interlevel_backward(rc._h, rays_p, None, nn, None, anneal, m, b, None, out, stream)
    assert call() == 0
    for kw in (dict(rays_p=None), dict(nn=-1), dict(anneal=float("nan")), dict(anneal=-0.1), dict(m=None), dict(b=None),
               dict(m=fl(float("inf"), 0.01)), dict(b=fl(0.03, -1.0)), dict(out=None)):
        assert call(**kw) == -1, kw
        assert lib.rc_last_error(rc._h), kw
    assert call(nn=0, out=None) == 0
    del held
    torch.cuda.synchronize()


def test_training_loop_reduces_the_loss():
    """Adam on the parameters of MLP_0 / MLP_1 driven by interlevel_grads + load_weights on a fixed 4096-ray batch."""
    rc = common.make_rc()
    n = 4096
    rays, jit = lc.cache_case(n, seed=41)
    names = [name for l in range(NP) for name, _, _ in rc.density_grad_layout(l)[0]]

    def grads():
        g, _, losses = train.interlevel_grads(rc, rays, jit, 1.0)
        return float(losses.sum()), {name: v for l in range(NP) for name, v in g[l].items()}

    hist = lc.adam_loop(rc, names, LOOP_LR, LOOP_STEPS, grads)
    assert min(hist[-3:]) < LOOP_DROP * hist[0], hist


# Adam at 1e-2 on every parameter of both levels: -21 % in 40 steps on this batch when the loop was tried out; the
# 0.85 bound at 60 steps leaves margin
LOOP_LR, LOOP_STEPS, LOOP_DROP = 1e-2, 60, 0.85
