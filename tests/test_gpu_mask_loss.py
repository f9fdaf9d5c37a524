"""rc_mask_backward and rc_backward_mask_rays on the GPU: the mask loss of the last level's opacity, its backward term and
their gradients, against the torch / numpy restatements (tests/mask_loss_ref.py) and the oracle chain."""
import ctypes as C

import numpy as np
import pytest
import torch

import common
import loss_cases as lc
import mask_loss_ref as mr
import nrc_amd
from nrc_amd import rc_ext, train
from nrc_amd.config import MaskLossConfig
from oracle import cache_ref, hashgrid_ref, mathx, train_ref

CFG = nrc_amd.hotdog_config()
S2 = CFG.sampling_strategy[-1][2]
L2 = CFG.num_levels - 1
RC_ERR_INVALID_ARG, RC_ERR_UNSUPPORTED = -1, -5
TERMS = train.mask_terms(1.0)
MAIN, BACK = TERMS["mask"], TERMS["mask_backwards"]

pytestmark = pytest.mark.gpu


def _buffers(rc, n):
    return lc.buffers(rc, "mk:", n, ("means", "density", "tdist", "weights", "d_density"))


def _planted_masks(n, seed=13):
    """0, 1, exactly 0.5, 0.5 plus one ulp and fractional values, in turn."""
    above = np.nextafter(np.float32(0.5), np.float32(1.0))
    frac = np.random.Generator(np.random.PCG64(seed)).uniform(0.0, 1.0, n).astype(np.float32)
    m = np.stack([np.zeros(n, np.float32), np.ones(n, np.float32), np.full(n, 0.5, np.float32), np.full(n, above, np.float32),
                  frac], axis=1)
    return np.ascontiguousarray(m[np.arange(n), np.arange(n) % 5])


def _compare(rc, n, rays, lm, masks, terms, loss, what):
    b = _buffers(rc, n)
    r64 = mr.restated(b["density"], b["tdist"], rays["directions"], masks, lm, terms, torch.float64)
    r32 = mr.restated(b["density"], b["tdist"], rays["directions"], masks, lm, terms, torch.float32)
    got = loss.cpu().numpy().astype(np.float64).reshape(1)
    print(what, "loss", got[0], r64[0], r32[0], "max|d_density|", np.abs(r64[1]).max(), "acc", r64[2].min(), r64[2].max())
    lc.check(got, np.array([r64[0]]), np.array([r32[0]]), what + " loss", rel_floor=1e-5)
    lc.check(b["d_density"], r64[1], r32[1], what + " d_density")
    if lm is not None:
        assert np.all(b["d_density"][np.asarray(lm) == 0.0] == 0.0)
    # the weights the kernel left are the composite's: their sum is the restatement's acc to fp32 rounding
    assert np.abs(b["weights"].astype(np.float64).sum(-1) - r64[2]).max() < 1e-5
    return r64


@pytest.mark.parametrize("n", [3000, 1, 65])
def test_kernel_against_restatement(n):
    """The loss and d density within 3x the fp32 restatement's distance from fp64 (plus 1e-5 / 1e-6 of the scale), on the
    call's own forward buffers: planted masks (0, 1, 0.5, 0.5 + 1 ulp, fractional), lossmult with zeros, a block of rays
    aimed away from the scene; then masks=None (and lossmult=None) and zero_masks.  3000 rays: the last workgroup is partial."""
    rc = common.make_rc()
    rays, jit = lc.cache_case(n)
    away = slice(n // 2, n // 2 + max(n // 10, 0))
    for k in ("directions", "viewdirs"):
        rays[k] = rays[k].copy()
        rays[k][away] = rays["origins"][away] / np.linalg.norm(rays["origins"][away], axis=-1, keepdims=True)
    lm = lc.lossmult(n)
    masks = _planted_masks(n)
    terms = dict(MAIN, weight_opaque=1.0, weight_empty=0.6)     # the two weights differ, so a wrong branch shows
    _, loss = rc.mask_backward(rays, jit, 0.4, masks, lm, terms, grads=False)
    r64 = _compare(rc, n, rays, lm, masks, terms, loss, f"n={n} planted")
    assert r64[0] > 0 or not lm.any()                           # n = 1: lossmult(1) is the one zero
    if n >= 10:
        print("acc of the rays aimed away:", r64[2][away].min(), r64[2][away].max())
    _, loss = rc.mask_backward(rays, jit, 0.4, None, None, terms, grads=False)          # ones, and no lossmult
    assert _compare(rc, n, rays, None, None, terms, loss, f"n={n} masks=None")[0] > 0
    _, loss = rc.mask_backward(rays, jit, 0.4, masks, lm, BACK, grads=False)          # masks given but not read
    _compare(rc, n, rays, lm, masks, BACK, loss, f"n={n} zero_masks")


def test_forward_matches_the_interlevel_buffers():
    """The mk: set's sdist, tdist, means and density of every level and the proposal levels' weights are bitwise the i:
    set's after rc_interlevel_backward on the same rays, jitter and anneal 0.4.  rc_interlevel_backward never writes the
    last level's weights (its kernel keeps them in registers), so those are compared with the g: set's, which
    k_geometry_loss_bwd writes from the same density with the same arithmetic."""
    n = 1000
    rc = common.make_rc()
    rays, jit = lc.cache_case(n, seed=11)
    rc.mask_backward(rays, jit, 0.4, None, None, MAIN, grads=False)
    rc.interlevel_backward(rays, jit, 0.4, levels=())
    rc.geometry_backward(rays, jit, 0.4, None, train.geometry_terms(1.0), grads=False)
    torch.cuda.synchronize()
    for l in range(L2 + 1):
        for k in ("sdist", "tdist", "means", "density"):
            a, b = rc.workspace(f"mk:{k}{l}"), rc.workspace(f"i:{k}{l}")
            assert a.shape == b.shape and np.array_equal(a, b), (k, l)
        other = "i:" if l < L2 else "g:"
        assert np.array_equal(rc.workspace(f"mk:weights{l}"), rc.workspace(f"{other}weights{l}")), l
    assert float(np.abs(rc.workspace(f"mk:weights{L2}")).max()) > 0


def _look_cases(n, seed):
    """Unit look vectors: random ones, both `up` branches ((0,0,-1), (1,0,0)) and |look_z| either side of float32(0.9)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    look = rng.normal(size=(n, 3))
    look /= np.linalg.norm(look, axis=-1, keepdims=True)
    z_hi = np.float64(np.float32(0.9))
    z_lo = np.float64(np.nextafter(np.float32(0.9), np.float32(0.0)))
    planted = [[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    for z in (z_lo, z_hi):
        for sign in (1.0, -1.0):
            planted.append([np.sqrt(1.0 - z * z), 0.0, sign * z])
    look[: len(planted)] = planted
    look = look.astype(np.float32)
    for i, z in enumerate((z_lo, z_lo, z_hi, z_hi)):
        assert abs(look[3 + i, 2]) == np.float32(z)
    return look


def test_backward_rays_against_restatement():
    """rc_backward_mask_rays against the fp64 numpy restatement within 3x the fp32 restatement's own distance from fp64
    plus 1e-6; near and far exact; the buffers go straight into rc_mask_backward with zero_masks."""
    n = 1027
    rc = common.make_rc()
    rays, _ = lc.cache_case(n, seed=51)
    look = _look_cases(n, 52)
    rng = np.random.Generator(np.random.PCG64(53))
    u1 = rng.uniform(size=n).astype(np.float32)
    u2 = rng.uniform(size=n).astype(np.float32)
    u1[:40:2] = 0.0
    u1[1:40:2] = np.float32(1.0 - 2.0 ** -24)
    u2[:40:4] = 0.0
    u2[2:40:4] = 0.5
    c = MaskLossConfig()
    back = rc.backward_mask_rays(rays["origins"], look, u1, u2, c.shadow_near_max, c.secondary_normal_eps, c.secondary_far)
    torch.cuda.synchronize()
    r64 = mr.backward_rays(rays["origins"], look, u1, u2, c.shadow_near_max, c.secondary_normal_eps, c.secondary_far, np.float64)
    r32 = mr.backward_rays(rays["origins"], look, u1, u2, c.shadow_near_max, c.secondary_normal_eps, c.secondary_far, np.float32)
    assert back["viewdirs"] is back["directions"]
    for k in ("origins", "directions"):
        got = back[k].cpu().numpy().astype(np.float64)
        err, tol = lc.bound(got, r64[k], r32[k].astype(np.float64), floor=1e-6)
        print(k, "err", err, "granted", tol)
        assert err <= tol, (k, err, tol)
    d = back["directions"].cpu().numpy()
    assert np.array_equal(d[u1 == 0.0], -look[u1 == 0.0])                    # u1 = 0: exactly the normal
    assert np.all(back["near"].cpu().numpy() == np.float32(c.shadow_near_max))
    assert np.all(back["far"].cpu().numpy() == np.float32(c.secondary_far))
    # fed straight into the loss
    jit = [j.reshape(-1) for j in common.jitters(n, seed=54)]
    lm = lc.lossmult(n, seed=55)
    _, loss = rc.mask_backward(back, jit, 0.4, None, lm, BACK, grads=False)
    host = {k: v.cpu().numpy() for k, v in back.items()}
    _compare(rc, n, host, lm, None, BACK, loss, "backward rays")
    # refused calls launch nothing and leave the outputs alone
    before = back["origins"].clone()
    o, lk, a, b = (rc._dev(x) for x in (rays["origins"], look, u1, u2))
    outs = [back[k].data_ptr() for k in ("origins", "directions", "near", "far")]
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda *args: rc.lib.rc_backward_mask_rays(rc._h, *args)
    good = (o.data_ptr(), lk.data_ptr(), a.data_ptr(), b.data_ptr())
    assert call(*good, -1, 0.2, 1e-2, 2.0, *outs, stream) == RC_ERR_INVALID_ARG
    assert call(*good, n, float("nan"), 1e-2, 2.0, *outs, stream) == RC_ERR_INVALID_ARG
    assert call(*good, n, 0.2, 1e-2, float("inf"), *outs, stream) == RC_ERR_INVALID_ARG
    assert call(good[0], None, good[2], good[3], n, 0.2, 1e-2, 2.0, *outs, stream) == RC_ERR_INVALID_ARG
    assert call(*good, n, 0.2, 1e-2, 2.0, outs[0], outs[1], outs[2], None, stream) == RC_ERR_INVALID_ARG
    assert call(*good, 0, 0.3, 1e-2, 2.0, *outs, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(before, back["origins"])


def _oracle_acc(w, means, tdist, directions):
    """acc of the last level in the oracle's arithmetic from the sample means on: level-2 density grid -> density MLP ->
    compute_alpha_weights -> sum (oracle hashgrid_ref / cache_ref pieces + weights_from_density)."""
    warped = mathx.contract_radius(means, CFG.contract_radius)
    x = hashgrid_ref.hash_encoding(w, f"params/Cache/Sampler/MLP_{L2}/density_grid", CFG.proposal_grids[L2], warped)
    h = torch.relu(cache_ref.dense(w, f"Cache/Sampler/MLP_{L2}/density_layers_0", x))
    h = torch.relu(cache_ref.dense(w, f"Cache/Sampler/MLP_{L2}/density_layers_1", h))
    raw = cache_ref.dense(w, f"Cache/Sampler/MLP_{L2}/output_density_layer", h)[..., 0]
    valid = ((warped > -CFG.proposal_grids[L2].bbox) & (warped < CFG.proposal_grids[L2].bbox)).all(dim=-1)
    density = torch.where(valid, mathx.safe_exp(raw + CFG.density_bias), torch.zeros_like(raw))
    return mr.weights_from_density(density, tdist, directions).sum(dim=-1)


def _margin_keep(rc, n0, count):
    """The first `count` of the n0 rays of the last rc_mask_backward call whose level-2 samples all keep a ReLU margin
    above 3e-5 (as test_gpu_geometry_loss / test_gpu_data_loss choose theirs)."""
    means = rc.workspace(f"mk:means{L2}")[: 3 * n0 * S2].reshape(3, -1).T.copy()
    m = train_ref.relu_margin(common.weights_torch(dtype=torch.float64), CFG, L2, torch.from_numpy(means).double())
    ok = np.nonzero((m.numpy().reshape(n0, S2) > 3e-5).all(axis=1))[0]
    return ok[:count], len(ok)


# Backward candidates of the whole-chain test: seed of their (u1, u2); jitters from seed + 1.  Chosen beforehand with the
# oracle's own fp64 sampler forward (cache_ref.proposal_sampler) on these rays, which keeps 2 381 of the 4 096 (mean acc
# 0.013: nearly empty space, as in front of a camera).
BACK_SEED = 61


def test_whole_chain_against_oracle():
    """Every tensor of the level-2 density layout (tables included) against fp64 autograd of the oracle chain (density
    grid -> density MLP -> weights_from_density -> mask loss) from the HIP forward's sample means, relative to each
    tensor's scale, with test_gpu_geometry_loss's bound.  The main term on 1 200 primary rays (two sample chunks of the
    density backward) and the backward term on 600 backward rays go into one flat; rays with a level-2 sample within
    3e-5 of a density-MLP ReLU kink are left out (each ray's forward is independent of the others)."""
    rc = common.make_rc()
    n0 = 8192
    rays0, jit0 = lc.cache_case(n0, seed=21)
    rc.mask_backward(rays0, jit0, 0.4, None, None, MAIN, grads=False)
    keep, _ = _margin_keep(rc, n0, 1200)
    assert len(keep) == 1200, len(keep)        # 38 400 samples: two chunks
    rays = {k: np.ascontiguousarray(v[keep]) for k, v in rays0.items()}
    jit, n = [np.ascontiguousarray(j[keep]) for j in jit0], len(keep)
    lm = lc.lossmult(n, seed=23)
    masks = _planted_masks(n, seed=24)
    # backward candidates from the batch's first 4 096 origins and a planted look (towards the scene centre)
    nb0 = 4096
    o = rays0["origins"][:nb0]
    look = (-o / np.linalg.norm(o, axis=-1, keepdims=True)).astype(np.float32)
    rng = np.random.Generator(np.random.PCG64(BACK_SEED))
    u1, u2 = rng.uniform(size=nb0).astype(np.float32), rng.uniform(size=nb0).astype(np.float32)
    jb0 = [j.reshape(-1) for j in common.jitters(nb0, seed=BACK_SEED + 1)]
    c = MaskLossConfig()
    back0 = rc.backward_mask_rays(o, look, u1, u2, c.shadow_near_max, c.secondary_normal_eps, c.secondary_far)
    rc.mask_backward(back0, jb0, 0.4, None, None, BACK, grads=False)
    keepb, found = _margin_keep(rc, nb0, 600)
    print("backward candidates keeping the margin:", found, "of", nb0)
    assert len(keepb) == 600, found
    back = {k: np.ascontiguousarray(v.cpu().numpy()[keepb]) for k, v in back0.items()}
    jb, nb = [np.ascontiguousarray(j[keepb]) for j in jb0], len(keepb)
    lmb = lc.lossmult(nb, seed=25)

    flat, l_main = rc.mask_backward(rays, jit, 0.4, masks, lm, MAIN)
    torch.cuda.synchronize()
    b = _buffers(rc, n)
    flat, l_back = rc.mask_backward(back, jb, 0.4, None, lmb, BACK, flat)
    torch.cuda.synchronize()
    bb = _buffers(rc, nb)
    g = train.grads_as_dict(flat, rc.density_grad_layout(L2)[0])
    ref, loss_ref = {}, {}
    for dt in (torch.float64, torch.float32):
        w = {k: v.clone().requires_grad_(True) for k, v in common.weights_torch(dtype=dt).items()}
        t = lambda a: torch.from_numpy(np.asarray(a)).to(dt)
        acc = _oracle_acc(w, t(b["means"]).reshape(n, S2, 3), t(b["tdist"]), t(rays["directions"]))
        accb = _oracle_acc(w, t(bb["means"]).reshape(nb, S2, 3), t(bb["tdist"]), t(back["directions"]))
        parts = (mr.mask_terms_loss(acc, t(masks), t(lm), MAIN), mr.mask_terms_loss(accb, None, t(lmb), BACK))
        (parts[0] + parts[1]).backward()
        ref[dt] = {k: v.grad for k, v in w.items() if v.grad is not None}
        loss_ref[dt] = [float(p.detach()) for p in parts]
    got = np.array([float(l_main[0]), float(l_back[0])])
    print("losses", got, loss_ref[torch.float64], loss_ref[torch.float32])
    lc.check(got, np.array(loss_ref[torch.float64]), np.array(loss_ref[torch.float32]), "losses", rel_floor=1e-5)
    checked, tables = 0, 0
    for name, v in g.items():
        a = v.cpu().double().numpy()
        assert name in ref[torch.float64], name
        r, r32 = ref[torch.float64][name].numpy(), ref[torch.float32][name].double().numpy()
        scale = float(np.abs(r).max())
        assert scale > 0, name
        err, err32 = float(np.abs(a - r).max()), float(np.abs(r32 - r).max())
        print(name, "err", err, "err32", err32, "scale", scale)
        assert err <= 3.0 * err32 + 2e-3 * scale, (name, err, err32, scale)
        checked += 1
        if "_grid/" in name:
            tables += 1
            only = (a != 0.0) != (r != 0.0)
            assert np.count_nonzero(only) <= 1e-4 * np.count_nonzero(r), (name, np.count_nonzero(only))
    assert tables == len(rc.hashgrid_grad_layout(L2)[0])
    assert checked == len(rc.density_grad_layout(L2)[0])


def test_semantics():
    rc = common.make_rc()
    n = 777
    rays, jit = lc.cache_case(n, seed=31)
    lm = lc.lossmult(n, seed=32)
    masks = _planted_masks(n, seed=33)
    f1, l1 = rc.mask_backward(rays, jit, 0.3, masks, lm, MAIN)
    f1, l1 = f1.clone(), l1.clone()
    f2, l2 = rc.mask_backward(rays, jit, 0.3, masks, lm, MAIN)
    assert torch.equal(l1, l2) and float(l1[0]) > 0                # bitwise stable
    assert torch.equal(lc.mlp_part(rc, f1, 0), lc.mlp_part(rc, f2, 0))
    assert float(f1.abs().max()) > 0
    acc = f1.clone()                                             # accumulates: a second call doubles
    rc.mask_backward(rays, jit, 0.3, masks, lm, MAIN, grads=acc)
    assert torch.equal(lc.mlp_part(rc, acc, 0), 2 * lc.mlp_part(rc, f1, 0))
    ref = 2 * f1.cpu().numpy()
    np.testing.assert_allclose(acc.cpu().numpy(), ref, rtol=1e-5, atol=1e-6 * float(np.abs(ref).max()))
    fz, lz = rc.mask_backward(rays, jit, 0.3, masks, lm, MAIN, grads=False)   # NULL buffer: the loss only
    assert fz is None and torch.equal(lz, l1)
    empty = {k: v[:0] for k, v in rays.items()}                 # n = 0: nothing written
    fe, le = rc.mask_backward(empty, [j[:0] for j in jit], 0.4, None, None, MAIN)
    assert float(le.abs().max()) == 0.0 and float(fe.abs().max()) == 0.0

    def still_first():
        _, la = rc.mask_backward(rays, jit, 0.3, masks, lm, MAIN, grads=False)
        assert torch.equal(la, l1)

    # charb_padding of 0, negative and non-finite is refused before any launch
    for pad in (0.0, -1e-3, float("nan"), float("inf")):
        with pytest.raises(rc_ext.RcError) as e:
            rc.mask_backward(rays, jit, 0.3, masks, lm, dict(MAIN, charb_padding=pad), grads=False)
        assert e.value.code == RC_ERR_UNSUPPORTED
        still_first()
    # NULL loss / cfg / rays and n = -1
    r, held, _ = rc._rays_struct(rays)
    cfg = rc_ext.rc_mask_loss(1e-3, 1.0, 1.0, 0)
    out = torch.zeros(1, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    call = rc.lib.rc_mask_backward
    assert call(rc._h, C.byref(r), None, None, n, None, 0.4, C.byref(cfg), None, None, stream) == RC_ERR_INVALID_ARG
    still_first()
    assert call(rc._h, C.byref(r), None, None, n, None, 0.4, None, None, out.data_ptr(), stream) == RC_ERR_INVALID_ARG
    still_first()
    assert call(rc._h, None, None, None, n, None, 0.4, C.byref(cfg), None, out.data_ptr(), stream) == RC_ERR_INVALID_ARG
    assert call(rc._h, C.byref(r), None, None, -1, None, 0.4, C.byref(cfg), None, out.data_ptr(), stream) == RC_ERR_INVALID_ARG
    still_first()
    assert float(out[0]) == 0.0
    del held
    # the time-resolved handle
    tr = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    tr.load_weights(common.weights_transient_np())
    r3, held3, _ = tr._rays_struct(rays)
    assert tr.lib.rc_mask_backward(tr._h, C.byref(r3), None, None, n, None, 0.4, C.byref(cfg), None, out.data_ptr(),
                                   stream) == RC_ERR_UNSUPPORTED
    del held3
    still_first()
    torch.cuda.synchronize()


def _split(rc, flat, key):
    """(dense segments, table segments) of the flat of layout `key` (a level or "shader"), each concatenated."""
    layout = rc.shader_grad_layout()[0] if key == "shader" else rc.density_grad_layout(key)[0]
    parts = ([], [])
    for name, o, shape in layout:
        parts["grid" in name].append(flat[o:o + int(np.prod(shape))])
    return torch.cat(parts[0]), torch.cat(parts[1])


def test_cache_stage_grads_with_the_mask_terms():
    """cache_stage_grads with the mask inputs: every earlier key and the other flats are what the call without them
    returns, flats[last] grows by the mask_grads flat, the new keys are mask_grads' losses.  "What it returns" is bitwise
    for the losses and the dense segments; the table segments are summed by memory-side float atomics whose order
    differs from call to call (rc_train.hip), so two calls on the same inputs agree there only to accumulation order:
    rtol 1e-5 as in test_semantics."""
    rc = common.make_rc()
    n = 512
    rays, jit = lc.cache_case(n, seed=71)
    gt = lc.uniform_gt(n, 72)
    lm = lc.lossmult(n, seed=73)
    masks = _planted_masks(n, seed=74)
    look = (-rays["origins"] / np.linalg.norm(rays["origins"], axis=-1, keepdims=True)).astype(np.float32)
    rng = np.random.Generator(np.random.PCG64(75))
    back = {"u1": rng.uniform(size=n).astype(np.float32), "u2": rng.uniform(size=n).astype(np.float32),
            "jitter": [j.reshape(-1) for j in common.jitters(n, seed=76)]}
    f0, l0 = train.cache_stage_grads(rc, rays, gt, jit, 1.0, lm)
    f0 = {k: v.clone() for k, v in f0.items()}
    l0 = {k: v.clone() for k, v in l0.items()}
    f1, l1 = train.cache_stage_grads(rc, rays, gt, jit, 1.0, lm, mask_cfg=MaskLossConfig(), masks=masks, look=look,
                                     backward_randoms=back)
    _, mflat, ml = train.mask_grads(rc, rays, jit, 1.0, masks, lm, None, look, back, scale=2.0)
    _, _, ml1 = train.mask_grads(rc, rays, jit, 1.0, masks, lm, None, look, back)
    torch.cuda.synchronize()
    for k, v in l0.items():
        assert torch.equal(v, l1[k]), k
    assert set(l1) - set(l0) == {"mask", "mask_backwards", "cache_main_mask", "cache_main_mask_backwards"}
    for k in (0, 1, "shader"):
        (d0, t0), (d1, t1) = _split(rc, f0[k], k), _split(rc, f1[k], k)
        assert torch.equal(d0, d1), k
        np.testing.assert_allclose(t1.cpu().numpy(), t0.cpu().numpy(), rtol=1e-5, atol=1e-6 * float(t0.abs().max()))
    want = (f0[L2] + mflat).cpu().numpy()
    np.testing.assert_allclose(f1[L2].cpu().numpy(), want, rtol=1e-5, atol=1e-6 * float(np.abs(want).max()))
    assert float(mflat.abs().max()) > 0
    for k in train.MASK_KEYS:
        assert float(ml[k]) > 0
        assert torch.equal(l1[k], ml[k] / 2) and torch.equal(l1[f"cache_main_{k}"], ml[k] / 2), k
        assert torch.equal(l1[k], ml1[k]), k                     # doubling the weights and halving the loss is exact
    # without look / backward_randoms only the main term runs
    _, l2 = train.cache_stage_grads(rc, rays, gt, jit, 1.0, lm, mask_cfg=MaskLossConfig(), masks=masks)
    assert "mask" in l2 and "mask_backwards" not in l2 and torch.equal(l2["mask"], l1["mask"])


def test_training_loop_empties_the_space():
    """Adam on MLP_2 driven by mask_grads alone with masks = 0 (the target is empty space) on a fixed batch: the loss
    falls and so does the mean acc of a render."""
    rc = common.make_rc()
    n = 2048
    rays, jit = lc.cache_case(n, seed=41)
    masks = np.zeros(n, np.float32)
    layout = rc.density_grad_layout(L2)[0]
    names = {name for name, _, _ in layout}

    def mean_acc():
        rc.set_fused(False)
        acc = rc.render_rays(rays, {"jitter": jit}, outputs=["acc"])["acc"]
        return float(acc.mean())

    def grads():
        g, _, losses = train.mask_grads(rc, rays, jit, 1.0, masks)
        return float(losses["mask"]), g[f"MLP_{L2}"]

    before = mean_acc()
    hist = lc.adam_loop(rc, names, LOOP_LR, LOOP_STEPS, grads)
    after = mean_acc()
    print("mask loss", hist[0], "->", hist[-1], "mean acc", before, "->", after)
    assert min(hist[-3:]) < hist[0], hist
    assert after < before, (before, after)


# Adam at 1e-3 on every parameter of MLP_2 (tables included), 40 steps on a fixed batch with masks = 0.
# First run: the loss fell from 0.7122 to 0.00194 and the mean acc of the render from 0.7122 to 0.00147 (the criterion
# above was set before it and needs neither number).
LOOP_LR, LOOP_STEPS = 1e-3, 40
