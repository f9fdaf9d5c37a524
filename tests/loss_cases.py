"""Shared helpers of the GPU loss tests (test_gpu_interlevel, _data_loss, _geometry_loss, _light_sampling,
_material_smoothness, _material_data_loss, _transient_data_loss, _loss_settings, _optimizer): seeded cases, views of the
training workspaces, the error bound against the fp32 restatement, the non-default loss settings with their effect-size
guard, and the training-loop bodies.  Test helper, not a test module."""
import dataclasses

import numpy as np
import pytest
import torch

import common
import nrc_amd
from oracle import material_ref

CFG = nrc_amd.hotdog_config()
CACHE_FIELDS = ("origins", "directions", "viewdirs", "near", "far", "lights")


def lossmult(n, seed=9):
    rng = np.random.Generator(np.random.PCG64(seed))
    lm = rng.uniform(0.5, 2.0, size=n).astype(np.float32)
    lm[::7] = 0.0
    return lm


def cache_case(n, seed=5):
    """Cache-stage batch: the rays' six hot fields and the three levels' jitters (seed + 1), flattened."""
    rays = nrc_amd.synthetic_rays(n, seed=seed).hot_fields()
    rays = {k: v for k, v in rays.items() if k in CACHE_FIELDS}
    jit = [j.reshape(-1) for j in common.jitters(n, seed=seed + 1)]
    return rays, jit


def material_case(n, K=None, seed=3):
    """Material-stage batch: every hot field and draw_randoms (seed + 1), for K secondary samples where K is given."""
    rays = nrc_amd.synthetic_rays(n, seed=seed).hot_fields()
    cfg = CFG if K is None else dataclasses.replace(CFG, num_secondary_samples=K)
    return rays, material_ref.draw_randoms(cfg, n, seed=seed + 1)


def uniform_gt(n, seed):
    return np.random.Generator(np.random.PCG64(seed)).uniform(0.0, 1.0, size=(n, 3)).astype(np.float32)


def normal_noise(n, seed):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal((n, 3)).astype(np.float32)


def hidden(hbuf, np_):
    """hbuf (k_density_mlp's accumulator order per 32-point tile) -> [np, 64] in the reference's column order."""
    tiles = (np_ + 31) // 32
    hb = hbuf[: tiles * 2048].reshape(tiles, 2, 16, 2, 32)          # tile, t, r, h, point
    t, r, h = np.meshgrid(np.arange(2), np.arange(16), np.arange(2), indexing="ij")
    col = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h
    out = np.empty((tiles, 32, 64), np.float32)
    out[:, :, col.reshape(-1)] = hb.reshape(tiles, 64, 32).transpose(0, 2, 1)
    return out.reshape(-1, 64)[:np_]


def buffers(rc, prefix, n, names):
    """{name: array} of a training call's workspace set ("i:", "d:", "g:") as the call left it, for n rays.  A name of
    the table is the last level's buffer; with a digit appended it is that level's."""
    S = [s for _, _, s in rc.cfg.sampling_strategy]

    def table(level, d_density):
        """name -> (workspace name, floats, view of them)"""
        s, np_ = S[level], n * S[level]
        rows = lambda a: a.reshape(n, s)
        soa3 = lambda a: a.reshape(3, np_).T                        # [3][np] -> [np, 3]
        return {"sdist": (f"sdist{level}", n * (s + 1), lambda a: a.reshape(n, s + 1)),
                "tdist": (f"tdist{level}", n * (s + 1), lambda a: a.reshape(n, s + 1)),
                "density": (f"density{level}", np_, rows), "weights": (f"weights{level}", np_, rows),
                "means": (f"means{level}", 3 * np_, soa3), "d_density": (d_density, np_, rows),
                "h64": ("hbuf", ((np_ + 31) // 32) * 2048, lambda a: hidden(a, np_).reshape(n, s, 64)),
                "app": ("app", 32 * np_, lambda a: a.reshape(32, np_).T.reshape(n, s, 32)),
                "normals_pred": ("normals_pred", 3 * np_, lambda a: soa3(a).reshape(n, s, 3)),
                "normals_grad": ("normals_grad", 3 * np_, lambda a: soa3(a).reshape(n, s, 3)),
                "d_pred": ("d_pred", 3 * np_, lambda a: a.reshape(n, s, 3))}

    out = {}
    last = table(len(S) - 1, "d_density")
    for name in names:
        ws, count, view = last[name] if name in last else table(int(name[-1]), name)[name[:-1]]
        out[name] = view(rc.workspace(prefix + ws)[:count]).copy()
    return out


def interlevel_buffers(rc, n):
    """The "i:" set as lists over the levels: sdist, tdist, density, means (every level) and d_density (the proposal
    levels), as rc_interlevel_backward left them."""
    levels = rc.cfg.num_levels
    tops = (("sdist", levels), ("tdist", levels), ("density", levels), ("means", levels), ("d_density", levels - 1))
    b = buffers(rc, "i:", n, [f"{k}{l}" for k, top in tops for l in range(top)])
    return tuple([b[f"{k}{l}"] for l in range(top)] for k, top in tops)


def granted(ref64, ref32, rel_floor=1e-6):
    """The tolerance `check` grants a quantity: 3x the fp32 restatement's own distance from fp64 plus rel_floor of the
    quantity's scale (plus 1e-12)."""
    err32 = float(np.abs(np.asarray(ref32, np.float64) - ref64).max())
    return 3.0 * err32 + rel_floor * float(np.abs(ref64).max()) + 1e-12


def bound(got, ref64, ref32, floor=0.0, rel_floor=None, what=None):
    """max|got - ref64| against 3x the fp32 restatement's own distance from fp64 plus a floor.  With `floor` (absolute)
    returns (err, bound) for the caller to assert; with `rel_floor` (times max|ref64|, plus 1e-12) asserts itself."""
    err, err32 = float(np.abs(got - ref64).max()), float(np.abs(ref32 - ref64).max())
    if rel_floor is None:
        return err, 3.0 * err32 + floor
    tol = granted(ref64, ref32, rel_floor)
    assert err <= tol, (what, err, err32, tol)


def check(got, ref64, ref32, what, rel_floor=1e-6):
    bound(got, ref64, ref32, rel_floor=rel_floor, what=what)


GUARD_FACTOR = 100.0


def guard(what, loss, grads=None, rel_floor=1e-6, grad_rel_floor=1e-6):
    """A settings case must be able to fail: its fp64 restatement has to differ from the fp64 restatement at the default
    settings (same buffers) by more than GUARD_FACTOR x the tolerance `check` grants -- in the loss, or in the largest
    gradient tensor.  loss: (case fp64, case fp32, default fp64) scalars or arrays; grads: the same triple of
    {name: array} dicts, the largest tensor chosen by max|case fp64|.  Rests on the reference alone."""
    f = lambda x: np.atleast_1d(np.asarray(x, np.float64))
    sizes = []
    c64, c32, d64 = (f(x) for x in loss)
    sizes.append(("loss", float(np.abs(c64 - d64).max()), granted(c64, c32, rel_floor)))
    if grads is not None:
        g64, g32, gd = grads
        name = max(g64, key=lambda k: float(np.abs(g64[k]).max()))
        sizes.append((name, float(np.abs(f(g64[name]) - f(gd[name])).max()), granted(f(g64[name]), f(g32[name]), grad_rel_floor)))
    print(what, "effect of the setting:", [(k, f"{d:.3e}", f"tol {t:.3e}") for k, d, t in sizes])
    assert any(d > GUARD_FACTOR * t for _, d, t in sizes), (what, sizes)


# ---- the time-resolved cache's data loss: the comparison and the non-default settings ------------------------------

TRANSIENT_ADJOINTS = (("d_t_irr", 64), ("d_t_slf", 128), ("d_tint_ibrdf", 3), ("d_direct", 3), ("d_weights", 1))
TRANSIENT_SETTINGS = ("use_gt", "no_combined", "exponent", "clip_val", "loss_thresh", "gauss_off", "gauss_scale", "mult_eps",
                      "combined")


def transient_batch(n, seed, jitter_seed=None, **ray_kw):
    rays = nrc_amd.synthetic_transient_rays(n, seed=seed, **ray_kw).hot_fields()
    jit = None if jitter_seed is None else [j.reshape(-1) for j in common.jitters(n, seed=jitter_seed)]
    return rays, jit


def transient_target(rc, rays, jit, seed):
    """gt = the device's own render times U(0.5, 1.5) per element: the same float32 array for the call and both chains."""
    rnd = None if jit is None else {"jitter": jit}
    rgb = rc.render_transient(rays, rnd, outputs=["rgb"])["rgb"].cpu().numpy()
    u = np.random.Generator(np.random.PCG64(seed)).uniform(0.5, 1.5, size=rgb.shape)
    return (rgb * u).astype(np.float32)


def transient_loss_thresh(gt):
    """The loss_thresh that zeroes about 30 % of the (ray, channel) pairs of gt [n, n_bins, 3], and the share it zeroes."""
    top = np.asarray(gt, np.float64).max(axis=1)                    # [n, 3]: the largest bin of each pair
    thresh = float(np.quantile(top, 0.7))
    return thresh, float((top > thresh).mean())


def transient_setting(name, gt):
    """TransientDataLossConfig of one entry of TRANSIENT_SETTINGS; clip_val and loss_thresh are taken from gt."""
    from nrc_amd.config import TransientDataLossConfig

    gt = np.asarray(gt, np.float64)
    clip = float(np.median(gt[gt > 0]))
    kw = {"use_gt": dict(use_gt_rawnerf=True), "no_combined": dict(use_combined_rawnerf=False),
          "exponent": dict(rawnerf_exponent=0.5), "clip_val": dict(clip_val=clip),
          "loss_thresh": dict(loss_thresh=transient_loss_thresh(gt)[0]), "gauss_off": dict(data_loss_gauss_mult=0.0),
          "gauss_scale": dict(data_loss_gauss_mult=1.0, transient_gauss_constant_scale=0.25),
          "mult_eps": dict(data_loss_mult=3.0, rawnerf_eps=1e-3),
          "combined": dict(use_combined_rawnerf=False, rawnerf_exponent=0.5, clip_val=clip)}[name]
    return dataclasses.replace(TransientDataLossConfig(), **kw)


def transient_refs(smooth, rays, jit, gt, rgb_nocorr=None, gt_nocorr=None, lossmult=None, loss_cfg=None):
    """(fp64, fp32) restatement of rc_transient_data_backward (transient_data_loss_ref.chain)."""
    import transient_data_loss_ref as tref
    from nrc_amd.config import TransientDataLossConfig

    loss_cfg = TransientDataLossConfig() if loss_cfg is None else loss_cfg
    w = common.weights_transient_np(smooth)
    return tuple(tref.chain(w, rays, jit, gt, rgb_nocorr, gt_nocorr, lossmult, dt, loss_cfg=loss_cfg)
                 for dt in (torch.float64, torch.float32))


def transient_guard(what, r64, r32, d64):
    guard(what, (r64["loss"], r32["loss"], d64["loss"]), (r64["grads"], r32["grads"], d64["grads"]))


def transient_compare(rc, smooth, rays, jit, gt, rgb_nocorr=None, gt_nocorr=None, lossmult=None, what="", loss_cfg=None,
                      refs=None):
    """rc.transient_data_backward under loss_cfg (None: the defaults) against the restatement under the same settings: the
    loss, the mse, "td:G", every element of the four head tensors and the five adjoints.  refs: (fp64, fp32) of
    transient_refs where the caller has them already."""
    import transient_data_loss_ref as tref
    from nrc_amd import train

    n = len(rays["origins"])
    r64, r32 = transient_refs(smooth, rays, jit, gt, rgb_nocorr, gt_nocorr, lossmult, loss_cfg) if refs is None else refs
    flat, losses = rc.transient_data_backward(rays, None if jit is None else {"jitter": jit}, gt, rgb_nocorr, gt_nocorr, lossmult,
                                              cfg=loss_cfg)
    losses = losses.cpu().numpy()
    f = lambda x: np.asarray(x, np.float64)
    print(what, "loss", losses[0], r64["loss"], r32["loss"], "mse", losses[1], r64["mse"], r32["mse"])
    check(f(losses[0:1]), f([r64["loss"]]), f([r32["loss"]]), what + " loss")
    check(f(losses[1:2]), f([r64["mse"]]), f([r32["mse"]]), what + " mse")
    check(rc.workspace("td:G")[: n * 2100].reshape(n, 700, 3), r64["G"], r32["G"], what + " G")
    layout, total = rc.transient_head_grad_layout()
    assert [name for name, _, _ in layout] == list(tref.HEAD_TENSORS)
    got = {k: v.cpu().numpy() for k, v in train.grads_as_dict(flat, layout).items()}
    for name in tref.HEAD_TENSORS:                         # every element
        check(got[name], r64["grads"][name], r32["grads"][name], f"{what} {name}")
    assert np.all(got[tref.HEAD_SLF + "/kernel"][:, -1] == 0.0) and got[tref.HEAD_SLF + "/bias"][-1] == 0.0     # alpha
    near = r64["near_tie"]
    assert near.mean() <= 0.01, (what, near.mean())
    keep = ~near
    for name, width in TRANSIENT_ADJOINTS:
        g = rc.workspace("td:" + name)[: n * 32 * width].reshape(n * 32, -1)
        a, b = r64[name].reshape(n * 32, -1), r32[name].reshape(n * 32, -1)
        check(g[keep], a[keep], b[keep], f"{what} {name}")
    return flat, losses, r64


# ---- the cache stage's losses: restatements on the call's own buffers --------------------------------------------------

def geometry_restated(w, b, rays, lm, dtype, terms):
    """(losses [4], d density, d pred_raw) of geometry_loss_ref under `terms` on the "g:" buffers b of a call."""
    import geometry_loss_ref as gr

    L2 = CFG.num_levels - 1
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    dens = t(b["density"]).requires_grad_(True)
    kern = t(w[f"params/Cache/Sampler/MLP_{L2}/pred_normals_layer/kernel"])
    bias = t(w[f"params/Cache/Sampler/MLP_{L2}/pred_normals_layer/bias"])
    raw = (t(b["h64"]) @ kern + bias).detach().requires_grad_(True)
    tdist, dirs = t(b["tdist"]), t(rays["directions"])
    weights = gr.weights_from_density(dens, tdist, dirs)
    losses = gr.geometry_losses(weights, t(lm), tdist, t(rays["viewdirs"]), gr.normals_from_raw(raw), t(b["normals_grad"]), terms)
    gd, gp = torch.autograd.grad(losses.sum(), (dens, raw), allow_unused=True)
    zero = lambda g, x: torch.zeros_like(x) if g is None else g
    return losses.detach().numpy(), zero(gd, dens).numpy(), zero(gp, raw).numpy()


def data_restated(w, b, rays, gt, lm, dtype, padding=1e-3, mult=1.0):
    """(loss, {d_density, dfeat, dapp, dp3}) of data_loss_ref on the "d:" buffers b of a call."""
    import data_loss_ref as dr

    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    h64 = t(b["h64"]).requires_grad_(True)
    app = t(b["app"]).requires_grad_(True)
    dens = t(b["density"]).requires_grad_(True)
    taps = {}
    loss, _ = dr.data_loss(w, CFG, h64, app, dens, t(b["tdist"]), t(rays["directions"]), t(rays["viewdirs"]), t(gt), t(lm),
                           padding=padding, mult=mult, taps=taps)
    loss.backward()
    return float(loss.detach()), dict(d_density=dens.grad, dfeat=h64.grad, dapp=app.grad, dp3=taps["pred_raw"].grad)


DATA_GRAD_FLOOR = 2e-5          # times the tensor's scale: the floor of test_gpu_data_loss's restatement comparison


def data_compare(rc, n, rays, gt, lm, loss, padding=1e-3, mult=1.0):
    """test_gpu_data_loss's restatement comparison on the "d:" buffers rc_data_backward left: the loss, d density,
    d feature64, d app32 and d pred_raw within 3x the fp32 restatement's distance from fp64 plus a small floor; no gradient
    where lossmult is 0.  -> (loss fp64, loss fp32, grads fp64, grads fp32) for the caller's own assertions."""
    S2 = CFG.sampling_strategy[-1][2]
    b = buffers(rc, "d:", n, ("density", "tdist", "means", "h64", "app", "d_density"))
    np_ = n * S2
    got = dict(d_density=b["d_density"], dfeat=rc.workspace("d:dfeat")[: np_ * 64].reshape(n, S2, 64),
               dapp=rc.workspace("d:dapp")[: np_ * 32].reshape(n, S2, 32), dp3=rc.workspace("d:dp3")[: np_ * 3].reshape(n, S2, 3))
    l64, g64 = data_restated(common.weights_torch(dtype=torch.float64), b, rays, gt, lm, torch.float64, padding, mult)
    l32, g32 = data_restated(common.weights_torch(dtype=torch.float32), b, rays, gt, lm, torch.float32, padding, mult)
    g64 = {k: v.numpy() for k, v in g64.items()}
    g32 = {k: v.double().numpy() for k, v in g32.items()}
    err, tol = bound(np.float64(loss), l64, l32, 1e-6 * l64)
    assert err <= tol, ("loss", loss, l64, l32)
    for k in ("d_density", "dfeat", "dapp", "dp3"):
        scale = float(np.abs(g64[k]).max())
        assert scale > 0, k
        err, tol = bound(got[k].astype(np.float64), g64[k], g32[k], DATA_GRAD_FLOOR * scale)
        assert err <= tol, (k, err, tol, scale)
    assert np.all(b["d_density"][lm == 0.0] == 0.0)
    assert np.all(got["dfeat"][lm == 0.0] == 0.0)
    return l64, l32, g64, g32


def interlevel_compare(rc, n, rays, lm, losses, mults, blurs):
    """test_gpu_interlevel's restatement comparison on the "i:" buffers rc_interlevel_backward left: per proposal level the
    loss and d loss / d density within 3x the fp32 restatement's distance from fp64 (plus 1e-6 of the scale), no gradient
    where lossmult is 0; a level whose mult is 0 has an exactly zero loss and gradient.
    -> (losses fp64, losses fp32, grads fp64, grads fp32), lists over the proposal levels."""
    import interlevel_ref as ir

    sd, td, dens, _, dd = interlevel_buffers(rc, n)
    args = (sd, td, dens, rays["directions"], lm, mults, blurs)
    l64, g64 = ir.interlevel_forward_backward(*args, torch.float64)
    l32, g32 = ir.interlevel_forward_backward(*args, torch.float32)
    g64, g32 = [g.numpy() for g in g64], [g.double().numpy() for g in g32]
    for l in range(rc.cfg.num_levels - 1):
        if mults[l] == 0.0:
            assert losses[l] == 0.0 and l64[l] == 0.0 and not dd[l].any() and not g64[l].any(), l
            continue
        assert l64[l] > 0
        err, tol = bound(np.float64(losses[l]), l64[l], l32[l], 1e-6 * l64[l])
        assert err <= tol, ("loss", l, losses[l], l64[l], l32[l])
        scale = float(np.abs(g64[l]).max())
        err, tol = bound(dd[l].astype(np.float64), g64[l], g32[l], 1e-6 * scale)
        assert err <= tol, ("d_density", l, err, tol, scale)
        assert np.all(dd[l][lm == 0.0] == 0.0)          # lossmult 0: no gradient
    return l64, l32, g64, g32


# ---- the material data loss's settings -------------------------------------------------------------------------------

def material_loss_kw(cfg):
    """material_data_loss_ref.data_loss's keywords of a config.MaterialDataLossConfig."""
    return dict(weight=cfg.loss_weight * cfg.material_loss_weight_ease, mult=cfg.data_loss_mult, exponent=cfg.exponent,
                eps=cfg.eps, clip_val=cfg.clip_val, thresh=cfg.loss_thresh, use_gt=cfg.use_gt_rawnerf,
                use_combined=cfg.use_combined_rawnerf, use_norm=cfg.use_norm_rawnerf)


MATERIAL_SETTINGS = {
    "use_gt": dict(use_gt_rawnerf=True), "no_combined": dict(use_combined_rawnerf=False), "use_norm": dict(use_norm_rawnerf=True),
    "exponent": dict(exponent=0.5), "clip_val": dict(clip_val=0.5), "loss_thresh": dict(loss_thresh=0.8),
    "weight_mult_eps": dict(loss_weight=0.7, data_loss_mult=2.0, eps=1e-3),
    "combined": dict(use_norm_rawnerf=True, exponent=0.5, clip_val=0.5),
}


def mlp_part(rc, flat, which):
    """The dense (non-table) segments of a flat gradient: which = 0 the last level's density layout, 1 the shader's."""
    layout = rc.density_grad_layout(CFG.num_levels - 1)[0] if which == 0 else rc.shader_grad_layout()[0]
    keep = [(o, int(np.prod(s))) for name, o, s in layout if "grid" not in name]
    return torch.cat([flat[o:o + c] for o, c in keep])


def make_material_rc(weights=None):
    return common.make_rc(weights=weights if weights is not None else common.weights_material_np())


def material_render(rc, K=None, n=1024, seed=51):
    """Every output of rc_render_material on a fixed batch, cache ("c_") and material ("m_") side."""
    cres, mres = rc.render_material(*material_case(n, K, seed), K)
    return {**{"c_" + k: v.clone() for k, v in cres.items()}, **{"m_" + k: v.clone() for k, v in mres.items()}}


def perturbed(weights, substring, seed):
    """`weights` with every tensor whose name has `substring` scaled by 1 + 0.05 N(0, 1), element by element."""
    w = dict(weights)
    rng = np.random.Generator(np.random.PCG64(seed))
    for k in list(w):
        if substring in k:
            w[k] = (np.asarray(w[k]) * (1.0 + 0.05 * rng.standard_normal(np.shape(w[k])))).astype(np.float32)
    return w


def flat_from_layout(layout, total, weights):
    flat = torch.empty(total, dtype=torch.float32, device="cuda")
    for name, off, shape in layout:
        flat[off: off + int(np.prod(shape))] = torch.from_numpy(np.ascontiguousarray(weights[name], np.float32)).reshape(-1)
    return flat


def adam_loop(rc, names, lr, steps, grads):
    """torch Adam on the named parameters, fed by grads() -> (what to record, {name: gradient}) and pushed back through
    load_weights after every step; returns the records."""
    params = {k: torch.from_numpy(v).cuda() for k, v in common.weights_np().items() if k in names}
    assert len(params) == len(names)
    opt = torch.optim.Adam(params.values(), lr=lr)
    hist = []
    for _ in range(steps):
        record, g = grads()
        hist.append(record)
        for name, v in g.items():
            params[name].grad = v.clone()
        opt.step()
        rc.load_weights(params)
    return hist


def step_loop(step, follow, opt, start, steps, lowered, label, fmt, each=None, render=None):
    """`steps` device-optimizer steps on a fixed batch: step() -> losses, follow(losses) -> the figure to track (printed
    with fmt under label), each(losses) the caller's per-step assertions.  The optimizer's count has advanced by
    `steps` from `start`, every figure is finite and lowered(totals) holds.  With `render`: the state saved two steps
    before the end is reloaded, render() is then bitwise what it was at that point, and two more steps land on the same
    figure."""
    totals = []
    for i in range(steps):
        if render is not None and i == steps - 2:
            sd, r_sd = opt.state_dict(), render()
        losses = step()
        if each is not None:
            each(losses)
        totals.append(follow(losses))
    print(label, [fmt(t) for t in totals])
    assert opt.count == start + steps
    assert all(np.isfinite(totals))
    assert lowered(totals), totals
    if render is None:
        return totals
    opt.load_state_dict(sd)
    assert opt.count == start + steps - 2
    r_again = render()
    for k in r_sd:
        assert torch.equal(r_sd[k], r_again[k]), k
    for _ in range(2):
        losses = step()
    assert opt.count == start + steps
    assert follow(losses) == pytest.approx(totals[-1], rel=1e-3)
    return totals
