"""Every device loss at its non-default settings: each run-time loss setting selects a branch of a HIP
kernel, and the sibling modules run each kernel at the one point of its settings space the hotdog / cornell gin resolves to.
Here each entry point is called through the public Python path (the config dataclass, or train.*_grads where that is where
a field is mapped) with one setting off its default, and compared with the loss's fp64 / fp32 restatement under the same
setting, rebuilt from the call's own workspace buffers exactly as the sibling default-settings test does.  No tolerance is
new: loss_cases.check (3 x the fp32 restatement's distance from fp64 plus 1e-6 of the tensor's scale; rel_floor = 1e-5 for
the geometry loss scalars) and the two shared comparisons of test_gpu_data_loss / test_gpu_interlevel.

Every case carries a guard that rests on the reference alone (loss_cases.guard): the fp64 restatement under the setting
differs from the fp64 restatement at the defaults, on the same buffers, by more than 100 x the granted tolerance, in the loss
or in the largest gradient tensor -- a call that dropped the setting on its way to the kernel could not pass."""
import dataclasses

import numpy as np
import pytest
import torch

import common
import envmap_grad_ref as eg
import interlevel_ref as ir
import light_sampling_ref as lr
import loss_cases as lc
import material_data_loss_ref as md
import material_smoothness_ref as mr
import nrc_amd
from nrc_amd import config, rc_ext, train

CFG = nrc_amd.hotdog_config()
K = 8
N_MATERIAL = 200                # 200 x 8 secondary rays: 12.5 tiles of 128 rows
N_CACHE = 130                   # 33 workgroups of four waves, the last half empty

pytestmark = pytest.mark.gpu

f64 = lambda x: np.atleast_1d(np.asarray(x, np.float64))


@pytest.fixture(scope="module")
def cache_rc():
    return common.make_rc()


@pytest.fixture(scope="module")
def material_rc():
    return lc.make_material_rc()


# ---- 1. the time-resolved cache's data loss ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def transient():
    """The batch of test_gpu_transient_data_loss.test_loss_grads_and_adjoints_vs_fp64 on the smooth = False handle, and the
    fp64 restatement at the default settings."""
    rc = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    rc.load_weights(common.weights_transient_np(False))
    rays, jit = lc.transient_batch(8, seed=31, jitter_seed=32)
    gt = lc.transient_target(rc, rays, jit, 33)
    return rc, rays, jit, gt, lc.transient_refs(False, rays, jit, gt)[0]


@pytest.mark.parametrize("name", lc.TRANSIENT_SETTINGS)
def test_transient_data_loss(transient, name):
    """loss, mse, td:G, every element of the four head tensors and the five adjoints (loss_cases.transient_compare, the
    near-tie share <= 1 % included).  clip_val is the median of gt's positive entries; loss_thresh the 0.7 quantile of the
    (ray, channel) pairs' largest bins, which zeroes 10 - 50 % of the pairs: their rows of G are exactly 0.  The combined
    case adds lossmult with zeros and a nocorr pair."""
    rc, rays, jit, gt, d64 = transient
    n = len(gt)
    cfg = lc.transient_setting(name, gt)
    extra = {}
    if name == "combined":
        extra = dict(lossmult=lc.lossmult(n), rgb_nocorr=lc.transient_target(rc, rays, jit, 54),
                     gt_nocorr=lc.transient_target(rc, rays, jit, 55))
        d64 = lc.transient_refs(False, rays, jit, gt, **extra)[0]
    if name in ("clip_val", "combined"):
        assert cfg.clip_val < float(gt.max())
    refs = lc.transient_refs(False, rays, jit, gt, loss_cfg=cfg, **extra)
    lc.transient_guard(name, *refs, d64)
    lc.transient_compare(rc, False, rays, jit, gt, what=name, loss_cfg=cfg, refs=refs, **extra)
    if name == "loss_thresh":
        share = lc.transient_loss_thresh(gt)[1]
        assert 0.1 <= share <= 0.5, share
        zeroed = gt.max(axis=1) > cfg.loss_thresh                   # [n, 3]
        G = rc.workspace("td:G")[: n * 2100].reshape(n, 700, 3)
        assert zeroed.any() and np.all(G.transpose(0, 2, 1)[zeroed] == 0.0)
        assert np.abs(G.transpose(0, 2, 1)[~zeroed]).max() > 0


# ---- 2. the material data loss and its EnvMap gradient ----------------------------------------------------------------

def _material_fwd(rc, n):
    nsec = n * K
    sizes = dict(m_pts=3 * n, m_nrm=3 * n, filt_weight=n, m_feat=32 * n, m_mat=5 * n, m_local_view=3 * n,
                 sec_samples=5 * nsec, sec_dirs=3 * nsec, sec_rgb=3 * nsec, sec_acc=nsec, sec_env=3 * nsec)
    return {k: rc.workspace(k)[:v].copy() for k, v in sizes.items()}


def _autograd(loss, w):
    gs = torch.autograd.grad(loss, list(w.values()), allow_unused=True)
    return {k: (np.zeros(v.shape) if g is None else g.detach().double().numpy()) for (k, v), g in zip(w.items(), gs)}


def _check_layout(got, layout, r64, r32):
    for name, off, shape in layout:
        size = int(np.prod(shape))
        lc.check(got[off: off + size], r64[name].reshape(-1), r32[name].reshape(-1), name)
    assert float(np.abs(got).max()) > 0


@pytest.mark.parametrize("name", list(lc.MATERIAL_SETTINGS))
def test_material_data_loss(material_rc, name):
    """The loss and every tensor of the material layout against md.chain_loss under the setting, at the call's own shading
    points and trace (test_gpu_material_data_loss.test_loss_and_every_tensor_against_fp64_autograd).  gt ~ U(0, 1), so
    clip_val = 0.5 binds and loss_thresh = 0.8 masks about a fifth of the channels.  use_norm and the combined case also
    run the _env form: every tensor of the EnvMap layout against envmap_grad_ref.chain_loss under the same keywords."""
    rc, n = material_rc, N_MATERIAL
    cfg = dataclasses.replace(config.MaterialDataLossConfig(), **lc.MATERIAL_SETTINGS[name])
    assert cfg.num_secondary_samples == K
    kw, kw0 = lc.material_loss_kw(cfg), lc.material_loss_kw(config.MaterialDataLossConfig())
    rays, rnd = lc.material_case(n, K, seed=21)
    gt = lc.uniform_gt(n, 23)
    lm = lc.lossmult(n, seed=22)
    if name == "loss_thresh":
        assert 0.1 <= float((gt > cfg.loss_thresh).mean()) <= 0.5
    _, mres = rc.render_material(rays, rnd, num_secondary_samples=K)
    acc_p = mres["acc"].cpu().numpy().reshape(-1)
    flat, losses = train.material_data_grads(rc, rays, rnd, gt, lm, cfg=cfg)
    torch.cuda.synchronize()
    layout, _ = rc.material_grad_layout()
    got = flat.cpu().numpy()
    crgb = rc.workspace("md:cache_rgb")[: 3 * n].reshape(n, 3)
    if name in ("clip_val", "combined"):
        assert (np.maximum(crgb, gt) > cfg.clip_val).mean() > 0.1
    fw = rc.workspace("filt_weight")[:n]
    f = _material_fwd(rc, n)
    Ks = Kd = K // 2
    wall = common.weights_material_np()
    wm = {k: v for k, v in wall.items() if "MaterialShader" in k}
    we = {k: v for k, v in wall.items() if k.startswith(eg.ENV)}
    env = name in ("use_norm", "combined")
    ref, eref = {}, {}
    for tag, dt, kws in (("64", torch.float64, kw), ("32", torch.float32, kw), ("default", torch.float64, kw0)):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
        sm, rgb_in, acc_in, env_in = md.split_trace(n, Ks, Kd, t(f["sec_samples"]), t(f["sec_rgb"]), t(f["sec_acc"]), t(f["sec_env"]))
        trace = (Ks, Kd, t(f["m_local_view"]).reshape(n, 3), sm, rgb_in, acc_in, env_in)
        pts = t(f["m_pts"]).reshape(n, 3)
        w = {k: t(v).requires_grad_(True) for k, v in wm.items()}
        ls, _ = md.chain_loss(w, CFG, pts, trace, t(gt), t(crgb), t(fw), t(acc_p), t(lm), bg=CFG.bg_intensity, **kws)
        ref[tag] = (float(ls), _autograd(ls, w))
        if env:
            w_e = {k: t(v).requires_grad_(True) for k, v in we.items()}
            ls, _ = eg.chain_loss({k: t(v) for k, v in wm.items()}, w_e, CFG, pts, t(f["sec_dirs"]).reshape(-1, 3), trace, t(gt),
                                  t(crgb), t(fw), t(acc_p), t(lm), bg=CFG.bg_intensity, **kws)
            eref[tag] = (float(ls), _autograd(ls, w_e))
    (l64, g64), (l32, g32), (l0, g0) = ref["64"], ref["32"], ref["default"]
    lc.guard(name, (l64, l32, l0), (g64, g32, g0))
    print(name, "loss", float(losses["data"]), l64, l32)
    assert l64 > 0
    lc.check(f64(float(losses["data"])), f64(l64), f64(l32), "loss")
    _check_layout(got, layout, g64, g32)
    if not env:
        return
    (e64, h64), (e32, h32), (e0, h0) = eref["64"], eref["32"], eref["default"]
    lc.guard(name + " env", (e64, e32, e0), (h64, h32, h0))
    _, env_flat, elosses = train.material_data_grads(rc, rays, rnd, gt, lm, flat=False, cfg=cfg, env_flat=True)
    torch.cuda.synchronize()
    elayout, _ = rc.envmap_grad_layout()
    assert [(nm, tuple(s)) for nm, _, s in elayout] == eg.envmap_layout(CFG)
    assert float(elosses["data"]) == float(losses["data"])
    lc.check(f64(float(elosses["data"])), f64(e64), f64(e32), "loss (env)")
    _check_layout(env_flat.cpu().numpy(), elayout, h64, h32)


# ---- 3. the light sampler's loss --------------------------------------------------------------------------------------

LIGHT_SETTINGS = {"linear": dict(linear_to_srgb=False), "mult": dict(mult=2.5), "linear_mult": dict(linear_to_srgb=False, mult=2.5)}


@pytest.mark.parametrize("name", list(LIGHT_SETTINGS))
def test_light_sampling(material_rc, name):
    """The loss and every tensor of the light layout against fp64 autograd of the whole chain
    (test_gpu_light_sampling.test_whole_chain_against_fp64_autograd), through train.light_sampling_grads, where
    LightSamplingConfig's fields are mapped; its grid regularizer is switched off (mult 0 adds exact zeros)."""
    rc, n = material_rc, N_MATERIAL
    cfg = dataclasses.replace(config.LightSamplingConfig(), light_grid_mult=0.0, **LIGHT_SETTINGS[name])
    assert cfg.num_secondary_samples == K
    rays, rnd = lc.material_case(n, K, seed=21)
    lm = lc.lossmult(n, seed=22)
    flat, losses = train.light_sampling_grads(rc, rays, rnd, 1.0, lm, cfg=cfg)
    torch.cuda.synchronize()
    assert float(losses["regularizer/light_grid"]) == 0.0
    layout, _ = rc.light_grad_layout()
    assert [(nm, tuple(s)) for nm, _, s in layout] == lr.light_layout(CFG)
    got = flat.cpu().numpy()
    Kd = int(round(K * CFG.diffuse_sample_fraction))
    Ks = K - Kd
    sizes = dict(m_pts=3 * n, m_nrm=3 * n, sec_dirs=3 * n * K, sec_samples=5 * n * K, sec_rgb=3 * n * K)
    b = {k: rc.workspace(k)[:v].copy() for k, v in sizes.items()}
    wn = {k: v for k, v in common.weights_material_np().items() if "LightSampler" in k}
    ref = {}
    for tag, dt, mult, srgb in (("64", torch.float64, cfg.mult, cfg.linear_to_srgb), ("32", torch.float32, cfg.mult, cfg.linear_to_srgb),
                                ("default", torch.float64, 1.0, True)):
        t = lambda a: torch.from_numpy(np.asarray(a)).to(dt)
        w = {k: t(v).requires_grad_(True) for k, v in wn.items()}
        pts = t(b["m_pts"]).reshape(n, 3)
        spec, diff = lr.split_samples(b["sec_dirs"], b["sec_samples"], b["sec_rgb"], b["m_nrm"], n, Ks, Kd, dt)
        vm, kap, lg = lr.get_vmfs(lr.vmf_params(w, CFG, pts), t(rnd["vmf_noise"]), pts, CFG.vmf_scale)
        loss = lr.light_sampling_loss(vm, kap, lg, spec, diff, t(lm), mult, srgb)
        ref[tag] = (float(loss), _autograd(loss, w))
    (l64, g64), (l32, g32), (l0, g0) = ref["64"], ref["32"], ref["default"]
    lc.guard(name, (l64, l32, l0), (g64, g32, g0))
    print(name, "loss", float(losses["light_sampling"]), l64, l32)
    assert l64 > 0
    lc.check(f64(float(losses["light_sampling"])), f64(l64), f64(l32), "loss")
    _check_layout(got, layout, g64, g32)


# ---- 4. the material smoothness loss ----------------------------------------------------------------------------------

SMOOTHNESS_SETTINGS = {"plain_albedo": dict(tensoir_albedo=False), "weights": dict(weight_albedo=3e-4, weight_other=5e-5),
                       "noise": dict(noise=0.05), "mult_plain_albedo": dict(mult=2.0, tensoir_albedo=False)}


@pytest.mark.parametrize("name", list(SMOOTHNESS_SETTINGS))
def test_material_smoothness(material_rc, name):
    """The loss and every tensor of the material layout against fp64 autograd at the call's own shading points
    (test_gpu_material_smoothness.test_loss_and_every_tensor_against_fp64_autograd), through train.material_smoothness_grads,
    where MaterialSmoothnessConfig's fields are mapped; its grid regularizer is switched off (mult 0 adds exact zeros).  The
    default-settings reference of the noise case takes x' at the default scale from the same shading points."""
    rc, n = material_rc, N_MATERIAL
    cfg = dataclasses.replace(config.MaterialSmoothnessConfig(), material_grid_mult=0.0, **SMOOTHNESS_SETTINGS[name])
    rays, rnd = lc.material_case(n, seed=21)
    noise = lc.normal_noise(n, 23)
    lm = lc.lossmult(n, seed=22)
    flat, losses = train.material_smoothness_grads(rc, rays, rnd, noise, 1.0, lm, cfg=cfg)
    torch.cuda.synchronize()
    assert float(losses["regularizer/material_grid"]) == 0.0 and float(losses["material_ray_sampler"]) == 0.0
    layout, _ = rc.material_grad_layout()
    assert [(nm, tuple(s)) for nm, _, s in layout] == mr.material_layout(CFG)
    got = flat.cpu().numpy()
    pts = rc.workspace("ms:pts")[: 6 * n].reshape(2, n, 3)
    fw = rc.workspace("filt_weight")[:n]
    wn = {k: v for k, v in common.weights_material_np().items() if "MaterialShader" in k}
    skw = dict(mult=cfg.mult, weight_albedo=cfg.weight_albedo, weight_other=cfg.weight_other, tensoir=cfg.tensoir_albedo)
    xp0 = pts[0] + noise * np.float32(config.MaterialSmoothnessConfig().noise)
    ref = {}
    for tag, dt, xp, kws in (("64", torch.float64, pts[1], skw), ("32", torch.float32, pts[1], skw), ("default", torch.float64, xp0, {})):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
        w = {k: t(v).requires_grad_(True) for k, v in wn.items()}
        ls = mr.chain_loss(w, CFG, t(pts[0]), t(xp), t(lm), t(fw), **kws)
        ref[tag] = (float(ls), _autograd(ls, w))
    (l64, g64), (l32, g32), (l0, g0) = ref["64"], ref["32"], ref["default"]
    lc.guard(name, (l64, l32, l0), (g64, g32, g0))
    print(name, "loss", float(losses["material_smoothness"]), l64, l32)
    assert l64 > 0
    lc.check(f64(float(losses["material_smoothness"])), f64(l64), f64(l32), "loss")
    _check_layout(got, layout, g64, g32)


# ---- 5. the geometry losses -------------------------------------------------------------------------------------------

G0 = config.GeometryLossConfig()
_ALONE = dict(distortion_mult=0.0, orientation_mult=0.0, pred_normal_mult=0.0, pred_normal_reverse_mult=0.0)
GEOMETRY_SETTINGS = {
    # power_ladder is conditioned differently for p < 0, 0 < p < 1 and p > 1
    "ladder_p-1.5": dict(distortion_p=-1.5, distortion_premult=2.0),
    "ladder_p0.5": dict(distortion_p=0.5, distortion_premult=1.0),
    "ladder_p2": dict(distortion_p=2.0, distortion_premult=10.0),
    # stopgrad_with_weight takes its own path at 0 and at 1
    "wgrad_0": dict(pred_normal_w_grad_weight=0.0), "wgrad_1": dict(pred_normal_w_grad_weight=1.0),
    # the two predicted-normal multipliers apart: (pn + pnr) on d n^, pn * wgrad on d w
    "pn_mults": dict(pred_normal_mult=0.05, pred_normal_reverse_mult=0.2),
    # each term alone: a cross-term cannot hide behind the sum
    "distortion_alone": dict(_ALONE, distortion_mult=G0.distortion_mult),
    "orientation_alone": dict(_ALONE, orientation_mult=G0.orientation_mult),
    "predicted_alone": dict(_ALONE, pred_normal_mult=G0.pred_normal_mult),
    "reverse_alone": dict(_ALONE, pred_normal_reverse_mult=G0.pred_normal_reverse_mult),
}


@pytest.mark.parametrize("name", list(GEOMETRY_SETTINGS))
def test_geometry(cache_rc, name):
    """The four losses (rel_floor = 1e-5), d density and d pred_raw from the "g:" buffers against the restatement under the
    terms train.geometry_terms makes of the config (test_gpu_geometry_loss.test_kernel_against_restatement).  A term whose
    multiplier is 0 has an exactly zero loss; the reverse term alone leaves d density exactly 0 (it reads stop_gradient(w)),
    the distortion term alone d pred_raw.  pred_normal_w_grad_weight reaches d density alone -- the loss values and
    d n^ do not depend on it by construction -- so its guard looks at d density; every other guard at the larger of the two
    gradients."""
    rc, n = cache_rc, N_CACHE
    cfg = dataclasses.replace(G0, **GEOMETRY_SETTINGS[name])
    terms, terms0 = train.geometry_terms(1.0, cfg), train.geometry_terms(1.0)
    rays, jit = lc.cache_case(n)
    lm = lc.lossmult(n)
    _, losses = rc.geometry_backward(rays, jit, 0.4, lm, terms)
    torch.cuda.synchronize()
    losses = losses.cpu().numpy().astype(np.float64)
    b = lc.buffers(rc, "g:", n, ("means", "density", "tdist", "normals_grad", "h64", "d_density", "d_pred"))
    w = common.weights_np()
    l64, dd64, dp64 = lc.geometry_restated(w, b, rays, lm, torch.float64, terms)
    l32, dd32, dp32 = lc.geometry_restated(w, b, rays, lm, torch.float32, terms)
    l0, dd0, dp0 = lc.geometry_restated(w, b, rays, lm, torch.float64, terms0)
    g64, g32, g0 = dict(d_density=dd64, d_pred=dp64), dict(d_density=dd32, d_pred=dp32), dict(d_density=dd0, d_pred=dp0)
    if name.startswith("wgrad"):
        g64, g32, g0 = (dict(d_density=g["d_density"]) for g in (g64, g32, g0))
    lc.guard(name, (l64, l32, l0), (g64, g32, g0), rel_floor=1e-5)
    print(name, "losses", losses, l64, l32)
    mults = (terms["distortion_mult"], terms["orientation_mult"], terms["pred_normal_mult"], terms["pred_normal_reverse_mult"])
    for k, m in enumerate(mults):
        assert (losses[k] == 0.0 and l64[k] == 0.0) if m == 0.0 else l64[k] > 0, (k, losses, l64)
    lc.check(losses, l64, l32, "losses", rel_floor=1e-5)
    lc.check(b["d_density"], dd64, dd32, "d_density")
    lc.check(b["d_pred"], dp64, dp32, "d_pred")
    if name == "reverse_alone":     # the reverse term reads stop_gradient(w): d density is exactly 0, all of it reaches n^
        assert np.all(dd64 == 0.0) and np.all(b["d_density"] == 0.0)
    else:
        assert np.abs(dd64).max() > 0
    if name == "distortion_alone":  # the distortion term does not read n^
        assert np.all(dp64 == 0.0) and np.all(b["d_pred"] == 0.0)
    else:
        assert np.abs(dp64).max() > 0 and np.abs(b["d_pred"]).max() > 0


# ---- 6. the cache data loss -------------------------------------------------------------------------------------------

DATA_SETTINGS = {"padding_1e-6": dict(charb_padding=1e-6), "padding_0.1": dict(charb_padding=0.1), "mult": dict(data_loss_mult=0.5)}


@pytest.mark.parametrize("name", list(DATA_SETTINGS))
def test_cache_data_loss(cache_rc, name):
    """test_gpu_data_loss's restatement comparison (loss_cases.data_compare) with the padding and the mult of the config, as
    train.data_grads maps them."""
    rc, n = cache_rc, N_CACHE
    cfg = dataclasses.replace(config.DataLossConfig(), **DATA_SETTINGS[name])
    rays, jit = lc.cache_case(n)
    gt = lc.uniform_gt(n, 7)
    lm = lc.lossmult(n)
    # train_frac 1: the anneal of the sibling test (0.4); grads=False is not offered by data_grads, the flats are dropped
    _, _, loss = train.data_grads(rc, rays, gt, jit, 1.0, lm, cfg=cfg)
    mult = cfg.loss_weight * cfg.data_loss_mult
    l64, l32, g64, g32 = lc.data_compare(rc, n, rays, gt, lm, float(loss.cpu()), cfg.charb_padding, mult)
    b = lc.buffers(rc, "d:", n, ("density", "tdist", "means", "h64", "app", "d_density"))
    l0, g0 = lc.data_restated(common.weights_torch(dtype=torch.float64), b, rays, gt, lm, torch.float64)
    lc.guard(name, (l64, l32, l0), (g64, g32, {k: v.numpy() for k, v in g0.items()}), grad_rel_floor=lc.DATA_GRAD_FLOOR)


# ---- 7. the interlevel loss -------------------------------------------------------------------------------------------

INTERLEVEL_SETTINGS = {"blurs": dict(blurs=(0.1, 0.0003)), "mults": dict(mults=(0.0, 0.02))}


@pytest.mark.parametrize("name", list(INTERLEVEL_SETTINGS))
def test_interlevel(cache_rc, name):
    """test_gpu_interlevel's restatement comparison (loss_cases.interlevel_compare) with the blurs and mults of the config,
    as train.interlevel_grads maps them; the level whose mult is 0 has an exactly zero loss and d density."""
    rc, n = cache_rc, N_CACHE
    cfg = dataclasses.replace(config.InterlevelConfig(), **INTERLEVEL_SETTINGS[name])
    il0 = config.InterlevelConfig()
    rays, jit = lc.cache_case(n)
    lm = lc.lossmult(n)
    _, _, losses = train.interlevel_grads(rc, rays, jit, 1.0, lm, cfg=cfg, levels=())
    l64, l32, g64, g32 = lc.interlevel_compare(rc, n, rays, lm, losses.cpu().numpy(), cfg.mults, cfg.blurs)
    sd, td, dens, _, _ = lc.interlevel_buffers(rc, n)
    l0, g0 = ir.interlevel_forward_backward(sd, td, dens, rays["directions"], lm, il0.mults, il0.blurs, torch.float64)
    named = lambda gs: {f"d_density{l}": np.asarray(g, np.float64) for l, g in enumerate(gs)}
    lc.guard(name, (l64, l32, l0), (named(g64), named(g32), named([g.numpy() for g in g0])))
