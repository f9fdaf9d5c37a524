"""rc_geometry_smoothness_backward on the GPU: the loss kernel on the call's own buffers against the fp64 restatement
(tests/geometry_smoothness_ref.py), the shared training forward, the call as a composition of rc_normals_backward (whose
own fp64 test, tests/test_gpu_normals_backward.py, then pins the whole chain), its semantics and a training loop."""
import ctypes as C

import numpy as np
import pytest
import torch

import common
import geometry_smoothness_ref as gs
import loss_cases as lc
import nrc_amd
from nrc_amd import rc_ext, train

CFG = nrc_amd.hotdog_config()
S2 = CFG.sampling_strategy[-1][2]
L2 = CFG.num_levels - 1
RC_ERR_UNSUPPORTED = -5
CHUNK = 32768                      # samples per chunk of the call's backward (kDataChunk)
TERMS = train.geometry_smoothness_terms(1.0)
TERMS_DENSITY = dict(TERMS, weight_density=0.01)
GEOMETRY_TERMS = train.geometry_terms(1.0)

pytestmark = pytest.mark.gpu


def _noise(n, seed):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((n, S2, 3)).astype(np.float32)


def _buffers(rc, n):
    """The "gs:" set as the call left it: the forward's last level, the perturbed evaluation, the upstream gradients."""
    b = lc.buffers(rc, "gs:", n, ("means", "weights", "density", "tdist", "normals_grad", "d_density"))
    np_ = n * S2
    soa3 = lambda a: a[: 3 * np_].reshape(3, np_).T.reshape(n, S2, 3).copy()
    aos3 = lambda a: a[: 3 * np_].reshape(n, S2, 3).copy()
    b["normals"] = b["normals_grad"]
    b["means_p"], b["normals_p"] = soa3(rc.workspace("gs:means_p")), soa3(rc.workspace("gs:normals_p"))
    b["density_p"] = rc.workspace("gs:density_p")[:np_].reshape(n, S2).copy()
    b["d_density_p"] = rc.workspace("gs:d_density_p")[:np_].reshape(n, S2).copy()
    for k in ("points", "points_p", "d_normals", "d_normals_p"):
        b[k] = aos3(rc.workspace("gs:" + k))
    return b


def test_loss_kernel_against_restatement():
    """The loss, d loss / d normals at both point sets and d loss / d density (weight_density 0.01) within lc.check's rule of
    the fp64 restatement fed the call's own buffers; the perturbed means bitwise fl(x + fl(noise * 0.1))."""
    n = 3000
    rc = common.make_rc()
    rays, jit = lc.cache_case(n)
    lm, noise = lc.lossmult(n), _noise(n, 71)
    for terms, what in ((TERMS, "normals"), (TERMS_DENSITY, "normals+density")):
        _, loss = rc.geometry_smoothness_backward(rays, jit, 0.4, noise, lm, terms)
        torch.cuda.synchronize()
        b = _buffers(rc, n)
        means = b["means"].reshape(n, S2, 3)
        assert np.array_equal(b["means_p"], gs.perturbed(means, noise, 0.1))
        assert np.array_equal(b["points"], means) and np.array_equal(b["points_p"], b["means_p"])
        l64, g64 = gs.loss_on_buffers(b, lm, terms, torch.float64)
        l32, g32 = gs.loss_on_buffers(b, lm, terms, torch.float32)
        print(what, "loss", float(loss[0]), l64, l32)
        assert l64 > 0
        lc.check(np.float64([float(loss[0])]), np.float64([l64]), np.float64([l32]), what + " loss")
        keys = ("d_normals", "d_normals_p") + (("d_density", "d_density_p") if terms["weight_density"] else ())
        for k in keys:
            assert np.abs(g64[k]).max() > 0, k
            lc.check(b[k].astype(np.float64), g64[k], g32[k].astype(np.float64), f"{what} {k}")
        assert np.array_equal(b["d_normals_p"], -b["d_normals"])
        assert np.all(b["d_normals"][lm == 0.0] == 0.0)             # lossmult 0: no gradient


def test_forward_is_the_shared_one():
    """The gs: level buffers are bitwise the g: set's after rc_geometry_backward on the same rays."""
    n = 1000
    rc = common.make_rc()
    rays, jit = lc.cache_case(n, seed=11)
    rc.geometry_smoothness_backward(rays, jit, 0.4, _noise(n, 72), None, TERMS, grads=False)
    rc.geometry_backward(rays, jit, 0.4, None, GEOMETRY_TERMS, grads=False)
    torch.cuda.synchronize()
    np_ = n * S2
    for l in range(L2 + 1):
        for k in ("sdist", "tdist", "means", "density", "weights"):
            assert np.array_equal(rc.workspace(f"gs:{k}{l}"), rc.workspace(f"g:{k}{l}")), (k, l)
    cnt = ((np_ + 31) // 32) * 2048
    assert np.array_equal(rc.workspace("gs:hbuf")[:cnt], rc.workspace("g:hbuf")[:cnt])
    for name in ("normals_grad", "normals_pred"):
        assert np.array_equal(rc.workspace("gs:" + name)[: 3 * np_], rc.workspace("g:" + name)[: 3 * np_]), name


def test_call_is_a_composition_of_normals_backward():
    """1 200 rays = 38 400 samples: the call runs two chunks.  Its flat equals rc_normals_backward at x with d_normals and at
    x' with its negative, both from the gs: buffers, issued as the call issues them (per chunk: x, then x'): the MLP segments
    bitwise, the tables up to the order of their atomics."""
    n = 1200
    rc = common.make_rc()
    rays, jit = lc.cache_case(n, seed=21)
    lm = lc.lossmult(n, seed=23)
    flat, _ = rc.geometry_smoothness_backward(rays, jit, 0.4, _noise(n, 73), lm, TERMS)
    torch.cuda.synchronize()
    b = _buffers(rc, n)
    np_ = n * S2
    assert np_ > CHUNK
    x, xp = b["points"].reshape(np_, 3), b["points_p"].reshape(np_, 3)
    d = b["d_normals"].reshape(np_, 3)
    assert np.abs(d).max() > 0
    mine = None
    for c0 in range(0, np_, CHUNK):
        mine, _ = rc.normals_backward(x[c0: c0 + CHUNK], d[c0: c0 + CHUNK], mine)
        mine, _ = rc.normals_backward(xp[c0: c0 + CHUNK], -d[c0: c0 + CHUNK], mine)
    torch.cuda.synchronize()
    assert float(lc.mlp_part(rc, flat, 0).abs().max()) > 0
    assert torch.equal(lc.mlp_part(rc, flat, 0), lc.mlp_part(rc, mine, 0))
    ref = mine.cpu().numpy()
    np.testing.assert_allclose(flat.cpu().numpy(), ref, rtol=1e-5, atol=1e-6 * float(np.abs(ref).max()))


def test_semantics():
    rc = common.make_rc()
    n = 777
    rays, jit = lc.cache_case(n, seed=31)
    lm, noise = lc.lossmult(n, seed=32), _noise(n, 74)
    f1, l1 = rc.geometry_smoothness_backward(rays, jit, 0.3, noise, lm, TERMS_DENSITY)
    f1, l1 = f1.clone(), l1.clone()
    f2, l2 = rc.geometry_smoothness_backward(rays, jit, 0.3, noise, lm, TERMS_DENSITY)
    assert torch.equal(l1, l2) and float(l1[0]) > 0               # bitwise stable
    assert torch.equal(lc.mlp_part(rc, f1, 0), lc.mlp_part(rc, f2, 0))
    fz, lz = rc.geometry_smoothness_backward(rays, jit, 0.3, noise, lm, TERMS_DENSITY, grads=False)    # the loss only
    assert fz is None and torch.equal(lz, l1)
    acc = f1.clone()                                             # accumulates: a second call doubles
    rc.geometry_smoothness_backward(rays, jit, 0.3, noise, lm, TERMS_DENSITY, grads=acc)
    ref = 2 * f1.cpu().numpy()
    np.testing.assert_allclose(acc.cpu().numpy(), ref, rtol=1e-5, atol=1e-6 * float(np.abs(ref).max()))
    empty = {k: v[:0] for k, v in rays.items()}                 # n = 0: nothing written
    fe, le = rc.geometry_smoothness_backward(empty, [j[:0] for j in jit], 0.4, noise[:0], None, TERMS)
    assert float(le.abs().max()) == 0.0 and float(fe.abs().max()) == 0.0
    # noise of all zeros: x' = x, loss 0, and +1 / -1 of jabs at 0 meet on the same point: the MLP gradients cancel exactly
    f0, l0 = rc.geometry_smoothness_backward(rays, jit, 0.3, np.zeros_like(noise), lm, TERMS)
    torch.cuda.synchronize()
    assert float(l0[0]) == 0.0
    assert float(lc.mlp_part(rc, f0, 0).abs().max()) == 0.0
    assert float(np.abs(rc.workspace("gs:d_normals")[: 3 * n * S2]).max()) > 0
    assert float(f0.abs().max()) <= 1e-5 * float(f1.abs().max())
    # weight_normals_pred != 0 is refused before any launch: the loss keeps its sentinel; NULL loss / noise; n < 0
    r, held, _ = rc._rays_struct(rays)
    nz = torch.from_numpy(noise).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.full((1,), 7.0, device="cuda")
    cfg = rc_ext.rc_geometry_smoothness(**{k: float(v) for k, v in TERMS.items()})
    bad = rc_ext.rc_geometry_smoothness(**{k: float(v) for k, v in dict(TERMS, weight_normals_pred=1.0).items()})
    call = lambda h, rr, nn, noise_p, c, loss_p: h.lib.rc_geometry_smoothness_backward(h._h, C.byref(rr), None, nn, None, 0.4, noise_p,
                                                                                      C.byref(c), None, loss_p, stream)
    assert call(rc, r, n, nz.data_ptr(), bad, out.data_ptr()) == RC_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert float(out[0]) == 7.0
    assert call(rc, r, n, nz.data_ptr(), cfg, None) == -1
    assert call(rc, r, n, None, cfg, out.data_ptr()) == -1
    assert call(rc, r, -1, nz.data_ptr(), cfg, out.data_ptr()) == -1
    torch.cuda.synchronize()
    assert float(out[0]) == 7.0
    del held
    # a time-resolved handle
    tr = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    tr.load_weights(common.weights_transient_np())
    r3, held3, _ = tr._rays_struct(rays)
    assert call(tr, r3, n, nz.data_ptr(), cfg, out.data_ptr()) == RC_ERR_UNSUPPORTED
    del held3
    torch.cuda.synchronize()
    assert float(out[0]) == 7.0


def test_noise_drawn_on_the_device_is_the_hosts():
    """One rc_prng_fill in normal mode under the loss's key: bitwise that fill, and the host twin's values within the
    normal mode's tolerance (tests/test_gpu_material_randoms.py: rtol 2e-6 / atol 2e-7, an ulp or two of erfinv)."""
    from nrc_amd import prng

    rc = common.make_rc()
    key = prng.PRNGKey(20200823)
    dev = prng.geometry_smoothness_noise(key, 37, S2, rc=rc)
    torch.cuda.synchronize()
    assert tuple(dev.shape) == (37, S2, 3)
    assert torch.equal(dev, rc.prng_fill(prng.split(prng.split(key)[1])[0], (37, S2, 3), "normal"))
    np.testing.assert_allclose(dev.cpu().numpy(), prng.geometry_smoothness_noise(key, 37, S2), rtol=2e-6, atol=2e-7)


def test_cache_stage_grads_counts_the_term_once():
    """cache_stage_grads with smoothness_cfg: the key geometry_smoothness holds the loss of geometry_smoothness_grads alone
    (one copy, no cache_main_ twin), every other key is bitwise what it is without it, and the last level's flat grows by the
    term's own gradient."""
    from nrc_amd.config import GeometrySmoothnessConfig

    n = 512
    rc = common.make_rc()
    rays, jit = lc.cache_case(n, seed=51)
    gt = lc.uniform_gt(n, 52)
    noise = _noise(n, 76)
    base_flats, base = train.cache_stage_grads(rc, rays, gt, jit, 1.0)
    base_flats = {k: v.clone() for k, v in base_flats.items()}
    flats, losses = train.cache_stage_grads(rc, rays, gt, jit, 1.0, smoothness_cfg=GeometrySmoothnessConfig(),
                                            smoothness_noise=noise)
    _, own, loss = train.geometry_smoothness_grads(rc, rays, jit, noise, 1.0)
    torch.cuda.synchronize()
    assert set(losses) == set(base) | {"geometry_smoothness"}
    assert torch.equal(losses["geometry_smoothness"], loss[0]) and float(loss[0]) > 0
    for k in base:
        assert torch.equal(losses[k], base[k]), k
    assert torch.equal(lc.mlp_part(rc, flats["shader"], 1), lc.mlp_part(rc, base_flats["shader"], 1))
    got = (flats[L2] - base_flats[L2]).cpu().numpy()
    ref = own.cpu().numpy()
    assert np.abs(ref).max() > 0
    # the difference of two sums that are orders of magnitude larger than the term: their rounding is the tolerance
    tol = 4 * np.finfo(np.float32).eps * float(base_flats[L2].abs().max())
    np.testing.assert_allclose(got, ref, rtol=1e-3, atol=tol + 1e-6 * float(np.abs(ref).max()))


def test_training_loop_reduces_the_loss():
    """Adam on the last level only, driven by geometry_smoothness_grads alone + load_weights on a fixed batch and fixed
    noise: the loss falls."""
    rc = common.make_rc()
    n = 2048
    rays, jit = lc.cache_case(n, seed=41)
    noise = _noise(n, 75)
    layout = rc.density_grad_layout(L2)[0]
    names = {name for name, _, _ in layout}

    def grads():
        g, _, loss = train.geometry_smoothness_grads(rc, rays, jit, noise, 1.0)
        return float(loss[0]), dict(g[f"MLP_{L2}"])

    hist = lc.adam_loop(rc, names, LOOP_LR, LOOP_STEPS, grads)
    print("geometry smoothness loop:", hist[0], hist[-1], [f"{v:.3e}" for v in hist])
    assert all(np.isfinite(hist))
    assert min(hist[-3:]) < LOOP_DROP * hist[0], hist


# Adam at 1e-3 on the last level's tables and density MLP, 40 steps on a fixed batch of 2 048 rays.  The first run, made with
# no bar beyond "below its start", lowered the loss from 4.746e-4 to 9.11e-5 (ratio 0.19, monotone); 0.5 leaves margin on that.
LOOP_LR, LOOP_STEPS, LOOP_DROP = 1e-3, 40, 0.5
