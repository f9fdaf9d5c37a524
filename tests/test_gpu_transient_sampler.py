"""The time-resolved cache stage's sampler side on the GPU: rc_transient_{interlevel,geometry,mask}_backward,
rc_transient_density_regularizer and the weights path of rc_transient_data_backward_sampler against the fp64 restatement of
tests/transient_sampler_ref.py, which runs the oracle's own power-ladder sampler; the new layout and its load; the refusals; the
step loop.

Every parity comparison is loss_cases.check: 3 x the fp32 restatement's own distance from fp64 plus 1e-6 of the quantity's
scale (the bound of DESIGN.md §4.15's tests).  No ray is left out: at nine rays the restatement's two precisions already land
on different sides of ReLU kinks (its own fp32-fp64 distance of the pre-activations, up to 2e-4, exceeds most samples'
margin), so that effect is inside the fp32 restatement's distance and a margin rule would leave no ray."""
import ctypes as C

import numpy as np
import pytest
import torch

import common
import loss_cases as lc
import nrc_amd
import transient_data_loss_ref as tref
import transient_sampler_ref as ts
from nrc_amd import config, rc_ext, train

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -5, -1
N = ts.CASE["n"]
S2 = 32
IL, GE, MK = (config.cornell_transient_interlevel_config(), config.cornell_transient_geometry_config(),
              config.cornell_transient_mask_config())
ANNEAL = 0.4                                     # RenderConfig.anneal: what the oracle's sampler runs at (train_frac = 1)
GEO_TERMS = train.geometry_terms(1.0, GE)
MASK_TERMS = train.mask_terms(1.0, MK)["mask"]


def _rc(weights=None, **kw):
    h = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(**kw), 0)
    h.load_weights(common.weights_transient_np() if weights is None else weights)
    return h


@pytest.fixture(scope="module")
def rc():
    return _rc()


@pytest.fixture(scope="module")
def batch():
    rays, jit = lc.transient_batch(N, seed=ts.CASE["seed"], jitter_seed=ts.CASE["jitter_seed"])
    lm = lc.lossmult(N, seed=ts.CASE["seed"] + 2)
    masks = (np.arange(N) % 3 != 0).astype(np.float32)
    return rays, jit, lm, masks


@pytest.fixture(scope="module")
def refs(batch):
    """The fp64 and fp32 restatements of the four loss calls on the batch, computed once."""
    rays, jit, lm, masks = batch
    kw = dict(lossmult=lm, masks=masks, il=(IL.mults, IL.blurs), geo_terms=GEO_TERMS, mask_terms=MASK_TERMS,
              reg_mult=GE.density_grid_mult)
    w = common.weights_transient_np()
    return ts.chain(w, rays, jit, torch.float64, **kw), ts.chain(w, rays, jit, torch.float32, **kw)


def _flat_check(rc, flat, r64, r32, what, touched):
    """Every element of the flat gradient: the tensors of `touched` (name predicate) against the restatement, tables and
    dense segments reported apart; every other segment untouched (exact zeros)."""
    layout, total = rc.transient_sampler_grad_layout()
    assert flat.numel() == total
    got = {k: v.cpu().double().numpy() for k, v in train.grads_as_dict(flat, layout).items()}
    worst = {"tables": (0.0, None), "dense": (0.0, None)}
    fails = []
    for name, _, _ in layout:
        a, b = r64[name], r32[name]
        if not touched(name):
            assert not got[name].any() and not a.any(), (what, name)
            continue
        assert np.abs(a).max() > 0, (what, name)
        err, tol = float(np.abs(got[name] - a).max()), lc.granted(a, b)
        kind = "tables" if "density_grid/" in name else "dense"
        if err / tol > worst[kind][0]:
            worst[kind] = (err / tol, name)
        print(f"{what} {name}: err {err:.3e} err32 {float(np.abs(b - a).max()):.3e} bound {tol:.3e} scale {float(np.abs(a).max()):.3e}")
        if err > tol:
            fails.append((name, err, tol))
    print(what, "worst err / bound: tables", worst["tables"], "dense", worst["dense"])
    assert not fails, (what, fails)


def test_layout_is_the_mirror(rc):
    layout, total = rc.transient_sampler_grad_layout()
    assert (layout, total) == train.transient_sampler_layout(rc.cfg)
    at = 0
    for l in range(rc.cfg.num_levels):            # the density layouts in turn, shifted
        lay, size = rc.density_grad_layout(l)
        mine = [s for s in layout if f"MLP_{l}/" in s[0] and "pred_normals_layer" not in s[0]]
        assert [(k, off - at, sh) for k, off, sh in mine] == lay
        at += size
    assert total == at + 64 * 3 + 3


def test_interlevel_vs_fp64(rc, batch, refs):
    rays, jit, lm, _ = batch
    r64, r32 = (r["interlevel"] for r in refs)
    flat, losses = rc.transient_interlevel_backward(rays, jit, ANNEAL, IL.mults, IL.blurs, lm)
    losses = losses.cpu().double().numpy()
    print("interlevel losses", losses, r64["losses"], r32["losses"])
    for l in range(2):
        lc.check(losses[l:l + 1], r64["losses"][l:l + 1], r32["losses"][l:l + 1], f"interlevel_{l}")
        dd = rc.workspace(f"i:d_density{l}")[: N * 64].reshape(N, 64)
        lc.check(dd, r64["d_density"][l], r32["d_density"][l], f"interlevel d_density{l}")
    _flat_check(rc, flat, r64["grads"], r32["grads"], "interlevel", lambda k: "MLP_0/" in k or "MLP_1/" in k)
    none, l2 = rc.transient_interlevel_backward(rays, jit, ANNEAL, IL.mults, IL.blurs, lm, grad=False)
    assert none is None and np.array_equal(l2.cpu().double().numpy(), losses)


def test_geometry_vs_fp64(rc, batch, refs):
    rays, jit, lm, _ = batch
    r64, r32 = (r["geometry"] for r in refs)
    flat, losses = rc.transient_geometry_backward(rays, jit, ANNEAL, lm, GEO_TERMS)
    losses = losses.cpu().double().numpy()
    print("geometry losses", losses, r64["losses"], r32["losses"])
    for k in range(4):
        lc.check(losses[k:k + 1], r64["losses"][k:k + 1], r32["losses"][k:k + 1], train.GEOMETRY_KEYS[k])
    dd = rc.workspace("g:d_density")[: N * S2].reshape(N, S2)
    lc.check(dd, r64["d_density"][0], r32["d_density"][0], "geometry d_density")
    _flat_check(rc, flat, r64["grads"], r32["grads"], "geometry", lambda k: "MLP_2/" in k)
    none, l2 = rc.transient_geometry_backward(rays, jit, ANNEAL, lm, GEO_TERMS, grad=False)
    assert none is None and np.array_equal(l2.cpu().double().numpy(), losses)


def test_mask_vs_fp64(rc, batch, refs):
    rays, jit, lm, masks = batch
    r64, r32 = (r["mask"] for r in refs)
    flat, loss = rc.transient_mask_backward(rays, jit, ANNEAL, masks, lm, MASK_TERMS)
    loss = loss.cpu().double().numpy()
    print("mask loss", loss, r64["losses"], r32["losses"])
    lc.check(loss, r64["losses"], r32["losses"], "mask")
    dd = rc.workspace("mk:d_density")[: N * S2].reshape(N, S2)
    lc.check(dd, r64["d_density"][0], r32["d_density"][0], "mask d_density")
    _flat_check(rc, flat, r64["grads"], r32["grads"], "mask", lambda k: "MLP_2/" in k and "pred_normals_layer" not in k)


def test_backward_mask_term_vs_fp64(rc, batch):
    """The backward term's rays (rc_backward_mask_rays at the cornell gin's shadow_near_max, normal_eps and secondary_far)
    through rc_transient_mask_backward with zero masks."""
    rays, _, lm, _ = batch
    o = rays["origins"]
    look = (-o / np.linalg.norm(o, axis=-1, keepdims=True)).astype(np.float32)
    rng = np.random.Generator(np.random.PCG64(71))
    u1, u2 = rng.uniform(size=N).astype(np.float32), rng.uniform(size=N).astype(np.float32)
    jb = [j.reshape(-1) for j in common.jitters(N, seed=72)]
    back = rc.backward_mask_rays(o, look, u1, u2, MK.shadow_near_max, MK.secondary_normal_eps, MK.secondary_far)
    terms = train.mask_terms(1.0, MK)["mask_backwards"]
    flat, loss = rc.transient_mask_backward(back, jb, ANNEAL, None, lm, terms)
    loss = loss.cpu().double().numpy()
    rb = {k: v.cpu().numpy() for k, v in back.items()}
    rb.update(lights=rays["lights"], lossmult=rays["lossmult"])
    w = common.weights_transient_np()
    r64, r32 = (ts.chain(w, rb, jb, dt, lossmult=lm, mask_terms=terms)["mask"] for dt in (torch.float64, torch.float32))
    print("mask_backwards loss", loss, r64["losses"], r32["losses"])
    lc.check(loss, r64["losses"], r32["losses"], "mask_backwards")
    _flat_check(rc, flat, r64["grads"], r32["grads"], "mask_backwards", lambda k: "MLP_2/" in k and "pred_normals_layer" not in k)


def test_regularizer_vs_fp64(rc, refs):
    r64, r32 = (r["reg"] for r in refs)
    flat = None
    for l in range(3):
        flat, loss = rc.transient_density_regularizer(l, GE.density_grid_mult, flat)
        lc.check(loss.cpu().double().numpy(), r64["losses"][l:l + 1], r32["losses"][l:l + 1], f"regularizer {l}")
    _flat_check(rc, flat, r64["grads"], r32["grads"], "regularizer", lambda k: "density_grid/" in k)
    none, loss = rc.transient_density_regularizer(2, GE.density_grid_mult, False)
    assert none is None and float(loss[0]) > 0


def test_weights_path_vs_fp64_and_bitwise(rc, batch):
    rays, jit, lm, _ = batch
    rnd = {"jitter": jit}
    gt = lc.transient_target(rc, rays, jit, 33)
    # bitwise: the _kind entry, the new entry without and with a sampler buffer
    kind = config.transient_data_loss_preset("mse")                # a reading that goes through rc_transient_data_backward_kind
    for cfg in (None, kind):
        h0, l0 = rc.transient_data_backward(rays, rnd, gt, lossmult=lm, cfg=cfg)
        g0 = rc.workspace("td:G")[: N * 2100].copy()
        adj0 = {k: rc.workspace("td:" + k)[: N * 32 * wd].copy() for k, wd in lc.TRANSIENT_ADJOINTS}
        h1, s1, l1 = rc.transient_data_backward_sampler(rays, rnd, gt, lossmult=lm, cfg=cfg, sampler_grad=False)
        assert s1 is None and torch.equal(h0, h1) and torch.equal(l0, l1)
        assert np.array_equal(g0, rc.workspace("td:G")[: N * 2100])
        for k, wd in lc.TRANSIENT_ADJOINTS:
            assert np.array_equal(adj0[k], rc.workspace("td:" + k)[: N * 32 * wd]), k
        h2, s2, l2 = rc.transient_data_backward_sampler(rays, rnd, gt, lossmult=lm, cfg=cfg)
        assert torch.equal(h0, h2) and torch.equal(l0, l2) and float(s2.abs().max()) > 0
    # the default reading: two calls on the same inputs
    h, s, l = rc.transient_data_backward_sampler(rays, rnd, gt, lossmult=lm)
    dd = rc.workspace("td:d_density")[: N * S2].reshape(N, S2).copy()
    _, _, lb = rc.transient_data_backward_sampler(rays, rnd, gt, lossmult=lm)
    assert torch.equal(l, lb) and np.array_equal(dd, rc.workspace("td:d_density")[: N * S2].reshape(N, S2))
    # parity: d_weights of the data loss's own restatement, through the closed form and the oracle's density chain
    w = common.weights_transient_np()
    d64, d32 = (tref.chain(w, rays, jit, gt, None, None, lm, dt) for dt in (torch.float64, torch.float32))
    lc.check(rc.workspace("td:d_weights")[: N * S2], d64["d_weights"], d32["d_weights"], "d_weights")
    r64, r32 = (ts.chain(w, rays, jit, dt, d_weights=d["d_weights"].reshape(N, S2))
                for dt, d in ((torch.float64, d64), (torch.float32, d32)))
    closed = ts.weights_path(d64["d_weights"].reshape(N, S2), r64["density"], r64["tdist"], rays["directions"].astype(np.float64))
    np.testing.assert_allclose(closed, r64["weights_path"]["d_density"][0], rtol=1e-9, atol=1e-12 * np.abs(closed).max())
    lc.check(dd, r64["weights_path"]["d_density"][0], r32["weights_path"]["d_density"][0], "weights path d_density")
    _flat_check(rc, s, r64["weights_path"]["grads"], r32["weights_path"]["grads"], "weights path",
                lambda k: "MLP_2/" in k and "pred_normals_layer" not in k)


def test_load_params_flat_renders_like_load_weights():
    w = common.weights_transient_np()
    w2 = w
    for i, sub in enumerate(("MLP_0/density_grid", "MLP_1/density_layers_1", "MLP_2/density_grid", "MLP_2/output_density_layer",
                             "pred_normals_layer")):
        w2 = lc.perturbed(w2, sub, 11 + i)
    a, b = _rc(weights=w2), _rc()
    rays, jit = lc.transient_batch(64, seed=81, jitter_seed=82)
    rnd = {"jitter": jit}
    before = b.render_transient(rays, rnd, outputs=["rgb"])["rgb"].clone()
    layout, total = b.transient_sampler_grad_layout()
    b.load_params_flat("transient_sampler", lc.flat_from_layout(layout, total, w2))
    ra, rb = a.render_transient(rays, rnd), b.render_transient(rays, rnd)
    assert not torch.equal(before, rb["rgb"])
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k
    # and the training forward after the load: the interlevel losses of both handles, bitwise
    la = a.transient_interlevel_backward(rays, jit, ANNEAL, IL.mults, IL.blurs, grad=False)[1]
    lb = b.transient_interlevel_backward(rays, jit, ANNEAL, IL.mults, IL.blurs, grad=False)[1]
    assert torch.equal(la, lb)


def test_refusals(rc, batch):
    rays, jit, lm, masks = batch
    gt = np.zeros((N, 700, 3), np.float32)
    hot = common.make_rc()
    occ = _rc(use_occlusions=True)
    for h in (hot, occ):
        calls = (lambda: h.transient_interlevel_backward(rays, jit, ANNEAL, IL.mults, IL.blurs, grad=False),
                 lambda: h.transient_geometry_backward(rays, jit, ANNEAL, None, GEO_TERMS, grad=False),
                 lambda: h.transient_mask_backward(rays, jit, ANNEAL, masks, None, MASK_TERMS, grad=False),
                 lambda: h.transient_density_regularizer(0, 0.01, False),
                 lambda: h.transient_data_backward_sampler(rays, None, gt, grad=False, sampler_grad=False))
        for i, call in enumerate(calls):
            with pytest.raises(rc_ext.RcError) as e:
                call()
            assert e.value.code == UNSUPPORTED, (h is hot, i)
    with pytest.raises(rc_ext.RcError) as e:
        hot.transient_sampler_grad_layout()
    assert e.value.code == UNSUPPORTED
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(16, device="cuda")
    assert hot.lib.rc_load_params_flat(hot._h, rc_ext.RC_LAYOUT_TRANSIENT_SAMPLER, buf.data_ptr(), st) == UNSUPPORTED
    assert hot.lib.rc_transient_sampler_grad_size(hot._h) == UNSUPPORTED
    # every other layout id keeps its answer on a time-resolved handle
    for lay in (0, 1, 2, rc_ext.RC_LAYOUT_SHADER, rc_ext.RC_LAYOUT_LIGHT, rc_ext.RC_LAYOUT_MATERIAL, rc_ext.RC_LAYOUT_ENVMAP):
        assert rc.lib.rc_load_params_flat(rc._h, lay, buf.data_ptr(), st) == UNSUPPORTED, lay
    assert rc.lib.rc_load_params_flat(rc._h, -7, buf.data_ptr(), st) == UNSUPPORTED
    assert rc.lib.rc_load_params_flat(rc._h, rc_ext.RC_LAYOUT_TRANSIENT_SAMPLER, None, st) == INVALID
    # NULL and negative-n arguments: the counterparts' rules
    lib = rc.lib
    r, held, _ = rc._rays_struct(rays)
    out = torch.zeros(4, device="cuda")
    m = (C.c_float * 2)(0.01, 0.01)
    b = (C.c_float * 2)(0.03, 0.003)
    g = rc_ext.rc_geometry_loss(**{k: float(v) for k, v in GEO_TERMS.items()})
    k = rc_ext.rc_mask_loss(1e-3, 0.1, 0.1, 0)
    assert lib.rc_transient_interlevel_backward(rc._h, C.byref(r), None, -1, None, 0.4, m, b, None, out.data_ptr(), st) == INVALID
    assert lib.rc_transient_interlevel_backward(rc._h, None, None, N, None, 0.4, m, b, None, out.data_ptr(), st) == INVALID
    assert lib.rc_transient_interlevel_backward(rc._h, C.byref(r), None, N, None, 0.4, m, b, None, None, st) == INVALID
    assert lib.rc_transient_interlevel_backward(rc._h, C.byref(r), None, 0, None, 0.4, m, b, None, None, st) == 0
    assert lib.rc_transient_geometry_backward(rc._h, C.byref(r), None, -1, None, 0.4, C.byref(g), None, out.data_ptr(), st) == INVALID
    assert lib.rc_transient_geometry_backward(rc._h, C.byref(r), None, N, None, 0.4, None, None, out.data_ptr(), st) == INVALID
    assert lib.rc_transient_geometry_backward(rc._h, C.byref(r), None, N, None, 0.4, C.byref(g), None, None, st) == INVALID
    assert lib.rc_transient_mask_backward(rc._h, C.byref(r), None, None, -1, None, 0.4, C.byref(k), None, out.data_ptr(), st) == INVALID
    assert lib.rc_transient_mask_backward(rc._h, C.byref(r), None, None, N, None, 0.4, C.byref(k), None, None, st) == INVALID
    assert lib.rc_transient_density_regularizer(rc._h, 3, 0.01, None, out.data_ptr(), st) == INVALID
    assert lib.rc_transient_density_regularizer(rc._h, 0, 0.01, None, None, st) == INVALID
    ck = rc_ext.transient_data_loss_kind_c(config.TransientDataLossConfig())
    cam = torch.zeros(N, 3, device="cuda")
    args = lambda n, cfg, gt_p, loss_p: (rc._h, C.byref(r), cam.data_ptr(), n, None, gt_p, None, None, None, cfg, None, None, loss_p, st)
    gt_d = torch.zeros(N * 2100, device="cuda")
    assert lib.rc_transient_data_backward_sampler(*args(-1, C.byref(ck), gt_d.data_ptr(), out.data_ptr())) == INVALID
    assert lib.rc_transient_data_backward_sampler(*args(N, None, gt_d.data_ptr(), out.data_ptr())) == INVALID
    assert lib.rc_transient_data_backward_sampler(*args(N, C.byref(ck), None, out.data_ptr())) == INVALID
    assert lib.rc_transient_data_backward_sampler(*args(0, C.byref(ck), None, None)) == 0
    del held
    torch.cuda.synchronize()


def test_step_loop():
    """Five transient_cache_stage_steps at 64 rays: finite losses, every segment group with a non-zero gradient moves, and
    the handle renders afterwards."""
    w = common.weights_transient_np()
    n = 64
    rays, jit = lc.transient_batch(n, seed=91, jitter_seed=92)
    rc = _rc()
    gt = lc.transient_target(rc, rays, jit, 93)
    lr = 1e-4
    ocfg = config.OptimizerConfig(lr_init=lr, lr_final=lr, lr_delay_steps=0, extra_opt_params=tuple(
        config.ExtraOptParams(g, lr, lr, 0, lr, lr, 0) for g in ("Cache", "SurfaceLightField")))
    opt = train.TransientSamplerOptimizer(rc, ocfg)
    opt.init_from(w)
    assert opt.keys == ["transient_heads", "transient_sampler"]
    assert {train.param_group(k) for k in opt.names() if "Sampler" in k} == {"Cache"}
    o = rays["origins"]
    look = (-o / np.linalg.norm(o, axis=-1, keepdims=True)).astype(np.float32)
    rng = np.random.Generator(np.random.PCG64(94))
    back = {"u1": rng.uniform(size=n).astype(np.float32), "u2": rng.uniform(size=n).astype(np.float32),
            "jitter": [j.reshape(-1) for j in common.jitters(n, seed=95)]}
    # which segments the losses reach: one gradient evaluation into fresh buffers
    flats, _ = train.transient_sampler_grads(rc, rays, None, jit, gt, 0.0, look=look, backward_randoms=back)
    nonzero = {key: {name for name, v in train.grads_as_dict(flats[key], opt.layouts[key][0]).items() if float(v.abs().max()) > 0}
               for key in opt.keys}
    assert any("MLP_0/" in k for k in nonzero["transient_sampler"]) and any("pred_normals" in k for k in nonzero["transient_sampler"])
    start = {key: opt.params[key].clone() for key in opt.keys}
    hist = []
    for _ in range(5):
        losses = train.transient_cache_stage_step(rc, opt, rays, None, jit, gt, look=look, backward_randoms=back)
        hist.append({k: float(v) for k, v in losses.items()})
    print("transient_cache_stage_step:", [f"{h['data']:.5e}" for h in hist])
    assert opt.count == 5
    assert all(np.isfinite(v) for h in hist for v in h.values())
    assert {"data", "mse", "interlevel_0", "interlevel_1", "mask", "mask_backwards", "regularizer/density_grid"} <= set(hist[0])
    for key in opt.keys:
        moved = train.grads_as_dict(opt.params[key] - start[key], opt.layouts[key][0])
        for name in nonzero[key]:
            assert float(moved[name].abs().max()) > 0, name
        assert float(opt.grads[key].abs().max()) == 0.0          # zeroed by the step
    out = rc.render_transient(rays, {"jitter": jit}, outputs=["rgb", "acc"])
    assert bool(torch.isfinite(out["rgb"]).all()) and bool(torch.isfinite(out["acc"]).all())
