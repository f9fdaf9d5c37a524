"""rc_adam_update and rc_load_params_flat on the GPU: k_adam bitwise against the numpy float32 restatement
(tests/optimizer_ref.py) on the four real layouts, the norm clip against fp64, the stream-ordered refresh against
rc_load_weights (bitwise renders), one cache_stage_step against the old torch + load_weights step, a training loop,
and the checkpoint / state_dict round trips."""
import numpy as np
import pytest
import torch

import common
import loss_cases as lc
import optimizer_ref as ref
import nrc_amd
from nrc_amd import checkpoint, rc_ext, train
from nrc_amd.config import OptimizerConfig

CFG = nrc_amd.hotdog_config()
pytestmark = pytest.mark.gpu

START = 2500          # past the learning-rate delay: steps of a visible size


def _groups(opt, k):
    """Per-element group index of buffer k."""
    grp = np.empty(opt.layouts[k][1], np.int64)
    for off, size, g in opt.segments[k]:
        grp[off: off + size] = g
    return grp


def _random_grads(rng, n):
    g = rng.standard_normal(n, dtype=np.float32) * np.float32(1e-3)
    idx = rng.choice(n, size=64, replace=False)
    g[idx[:8]] = np.nan
    g[idx[8:16]] = np.inf
    g[idx[16:24]] = -np.inf
    g[idx[24:40]] = 0.0
    g[idx[40:64]] = np.float32(1e-41) * rng.standard_normal(24, dtype=np.float32)    # subnormal
    g[rng.random(n) < 0.02] = 0.0
    return g


def _opt(weights=None, cfg=OptimizerConfig(), count=0):
    rc = common.make_rc()
    opt = train.CacheStageOptimizer(rc, cfg)
    opt.init_from(common.weights_np() if weights is None else weights, count=count)
    return rc, opt


@pytest.mark.parametrize("zero,max_val", [(True, 0.0), (False, 0.5)])
def test_k_adam_bitwise_against_f32_restatement(zero, max_val):
    cfg = OptimizerConfig(grad_max_val=max_val)
    rc, opt = _opt(cfg=cfg, count=START)
    rng = np.random.default_rng(11 if zero else 12)
    host = {k: [opt.params[k].cpu().numpy(), np.zeros_like(opt.params[k].cpu().numpy()),
                np.zeros_like(opt.params[k].cpu().numpy())] for k in opt.keys}
    grp = {k: _groups(opt, k) for k in opt.keys}
    assert set(np.unique(grp["shader"])) == {opt.group_names.index("Cache"), opt.group_names.index("SurfaceLightField")}
    assert all(set(np.unique(grp[k])) == {opt.group_names.index("Cache")} for k in opt.keys if k != "shader")
    for t in range(START, START + 20):
        sc = train.adam_scalars(t, cfg, zero_grads=zero)
        gs = {}
        for k in opt.keys:
            gs[k] = _random_grads(rng, opt.layouts[k][1])
            opt.grads[k].copy_(torch.from_numpy(gs[k]))
        rc.adam_update(opt._table, sc)
        for k in opt.keys:
            host[k] = list(ref.adam_f32(*host[k][:1], gs[k], *host[k][1:], grp[k], sc))
        if t in (START, START + 19):
            torch.cuda.synchronize()
            for k in opt.keys:
                for name, dev, want in zip(("params", "mu", "nu"), (opt.params[k], opt.mu[k], opt.nu[k]), host[k]):
                    got = dev.cpu().numpy()
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, name, t,
                                                                                     int(np.sum(got != want)))
                g_after = opt.grads[k].cpu().numpy()
                if zero:
                    assert not np.any(g_after), k
                else:
                    assert np.array_equal(g_after.view(np.uint32), gs[k].view(np.uint32)), k


def test_norm_clip_against_fp64_and_reproducible():
    cfg = OptimizerConfig(grad_max_norm=1.0, grad_max_val=0.0)
    rc, opt = _opt(cfg=cfg, count=START)
    rng = np.random.default_rng(21)
    gs = {}
    for k in opt.keys:
        gs[k] = rng.standard_normal(opt.layouts[k][1], dtype=np.float32) * np.float32(1e-3)
        gs[k][::1000] = np.nan
        opt.grads[k].copy_(torch.from_numpy(gs[k]))
    p0 = {k: opt.params[k].cpu().numpy() for k in opt.keys}
    sc = train.adam_scalars(START, cfg, zero_grads=False)
    norms, mults = [], []
    for _ in range(3):
        for k in opt.keys:
            opt.params[k].copy_(torch.from_numpy(p0[k]))
            opt.mu[k].zero_()
            opt.nu[k].zero_()
        rc.adam_update(opt._table, sc)
        norms.append(rc.workspace("o:norm").copy())
        mults.append(rc.workspace("o:mult").copy())
    norm64, mult64 = ref.norm_mult(list(gs.values()), 0.0, 1.0)
    assert abs(float(norms[0][0]) - norm64) <= 1e-6 * norm64, (float(norms[0][0]), norm64)
    assert mult64 < 1 and abs(float(mults[0][0]) - mult64) <= 1e-6 * mult64, (float(mults[0][0]), mult64)
    for nn, mm in zip(norms[1:], mults[1:]):
        assert nn.view(np.uint32)[0] == norms[0].view(np.uint32)[0] and mm.view(np.uint32)[0] == mults[0].view(np.uint32)[0]
    # the update used that multiplier: bitwise the restatement fed the device's float32 multiplier
    torch.cuda.synchronize()
    for k in opt.keys:
        z = np.zeros_like(p0[k])
        want = ref.adam_f32(p0[k], gs[k], z, z, _groups(opt, k), sc, mults[0][0])[0]
        assert np.array_equal(opt.params[k].cpu().numpy().view(np.uint32), want.view(np.uint32)), k


def _moved_cache_weights(seed=3):
    """Every cache-stage parameter scaled by 1.05 plus 0.01 N(0, 1): its own draw, not loss_cases.perturbed's."""
    w = dict(common.weights_np())
    rng = np.random.default_rng(seed)
    names = set()
    rc = common.make_rc()
    for k in list(range(CFG.num_levels)) + ["shader"]:
        lay = rc.shader_grad_layout()[0] if k == "shader" else rc.density_grad_layout(k)[0]
        names |= {n for n, _, _ in lay}
    out = {n: (w[n] * np.float32(1.05) + np.float32(0.01) * rng.standard_normal(w[n].shape)).astype(np.float32)
           for n in names}
    return out


def _renders(rc, n=512):
    rays, jit = lc.cache_case(n, seed=31)
    srays, srnd = common.secondary_case(n, seed=12)
    g = np.random.default_rng(4).gumbel(size=(n, 32)).astype(np.float32)
    out = {}
    for fused in (True, False):
        rc.set_fused(fused)
        r = rc.render_rays(rays, {"jitter": jit}, outputs=["rgb", "acc", "distance_median", "normals_pred"])
        out.update({f"{k}_{fused}": v.clone() for k, v in r.items()})
    rc.set_fused(True)
    r = rc.render_rays(rays, {"jitter": jit, "gumbel": g}, rc_ext.RC_PASS_CACHE | rc_ext.RC_PASS_RESAMPLE,
                       outputs=["rgb", "acc", "means"])
    out.update({f"res_{k}": v.clone() for k, v in r.items()})
    r = rc.render_rays(srays, srnd, rc_ext.RC_PASS_CACHE | rc_ext.RC_PASS_SECONDARY | rc_ext.RC_PASS_NO_ENVMAP,
                       outputs=["rgb", "acc", "distance_mean"])
    out.update({f"sec_{k}": v.clone() for k, v in r.items()})
    gt = torch.full((n, 3), 0.5, device="cuda")
    _, loss = rc.data_backward(rays, gt, jit, 0.3)
    out["data_loss"] = loss.clone()
    return out


def test_load_params_flat_renders_as_load_weights():
    new = _moved_cache_weights()
    a = common.make_rc()
    a.load_weights(new)
    want = _renders(a)
    torch.cuda.synchronize()
    b = common.make_rc()
    before = _renders(b)            # derived tables and packs of the old weights exist: the refresh must mark them stale
    opt = train.CacheStageOptimizer(b)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        # the new parameters are produced on the side stream and handed over without a device synchronisation
        for k in opt.keys:
            for name, off, shape in opt.layouts[k][0]:
                opt.params[k][off: off + int(np.prod(shape))].copy_(torch.from_numpy(new[name]).reshape(-1),
                                                                    non_blocking=False)
            opt.params[k].mul_(2.0).mul_(0.5)          # the last writes are kernels queued on `side`
        opt.refresh()
        got = _renders(b)
    torch.cuda.synchronize()
    assert not torch.equal(before["rgb_True"], want["rgb_True"])
    for key in want:
        assert torch.equal(got[key], want[key]), key


def _record_grads(weights, n=2048, seed=41):
    rc = common.make_rc(weights=weights)
    rays, jit = lc.cache_case(n, seed=seed)
    target = rc_ext.RadianceCache(CFG, 0)
    target.load_weights(common.weights_np(seed=2))
    target.set_fused(False)
    gt = target.render_rays(rays, {"jitter": jit}, outputs=["rgb"])["rgb"].reshape(n, 3).contiguous()
    flats, losses = train.cache_stage_grads(rc, rays, gt, jit, train.train_frac_at(START, 25000))
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in flats.items()}, rays, jit, gt


def test_step_against_torch_adam_and_load_weights():
    w = common.weights_np()
    grads, rays, jit, _ = _record_grads(w)
    cfg = OptimizerConfig()
    rc, opt = _opt(count=START)
    opt.step({k: grads[k].clone() for k in opt.keys})
    # the old way: per-tensor torch params, the optax update restated in torch float32, load_weights
    old = common.make_rc()
    sc = train.adam_scalars(START, cfg)
    gi = {g: i for i, g in enumerate(opt.group_names)}
    params = {}
    for k in opt.keys:
        for name, off, shape in opt.layouts[k][0]:
            size = int(np.prod(shape))
            p = torch.from_numpy(w[name]).cuda().reshape(-1)
            g = torch.nan_to_num(grads[k][off: off + size])
            i = gi[train.param_group(name, cfg)]
            mu = float(sc["one_minus_b1"][i]) * g
            nu = float(sc["one_minus_b2"][i]) * (g * g)
            u = (mu / float(sc["bias_correction1"][i])) / (torch.sqrt(nu / float(sc["bias_correction2"][i])) + float(sc["eps"][i]))
            params[name] = (p + u * (-float(sc["lr"][i]))).reshape(shape)
    old.load_weights(params)
    lr = float(sc["lr"][gi["Cache"]])
    got = opt.params_dict()
    worst = 0.0
    for name, v in params.items():
        d = (got[name] - v).abs()
        # float32 rounding of two evaluations of the same expression: a few ulp of p plus a few ulp of the step (<= lr)
        tol = 4e-7 * v.abs() + 1e-6 * lr
        assert bool((d <= tol).all()), (name, float(d.max()))
        worst = max(worst, float(d.max()))
    a = _renders(rc)
    b = _renders(old)
    for key in a:
        assert float((a[key] - b[key]).abs().max()) <= 1e-5, key


def test_training_loop_reduces_the_loss():
    rc, opt = _opt(count=START)
    n = 2048
    rays, jit = lc.cache_case(n, seed=41)
    target = rc_ext.RadianceCache(CFG, 0)
    target.load_weights(common.weights_np(seed=2))
    target.set_fused(False)
    gt = target.render_rays(rays, {"jitter": jit}, outputs=["rgb"])["rgb"].reshape(n, 3).contiguous()
    lc.step_loop(lambda: train.cache_stage_step(rc, opt, rays, gt, jit),
                 lambda losses: float(sum(float(v) for v in losses.values())), opt, START, LOOP_STEPS,
                 lambda total: min(total[-3:]) < LOOP_DROP * total[0], "cache_stage_step loop totals:",
                 lambda t: round(t, 5))


def test_checkpoint_and_state_dict_round_trips(tmp_path):
    grads, rays, jit, gt = _record_grads(common.weights_np())
    rc, opt = _opt(count=START)
    for _ in range(3):
        train.cache_stage_step(rc, opt, rays, gt, jit)
    torch.cuda.synchronize()
    # parameters and step through the Flax checkpoint format, into a fresh handle's load_weights
    path = checkpoint.save_params({k: v.cpu().numpy() for k, v in opt.params_dict().items()}, str(tmp_path), step=opt.count)
    loaded = checkpoint.load_params(path)
    fresh = common.make_rc()
    fresh.load_weights(loaded)
    a, b = _renders(rc), _renders(fresh)
    for key in a:
        assert torch.equal(a[key], b[key]), key
    # state_dict: resume from it and replay the same (recorded) gradients -> bitwise the same state
    sd = opt.state_dict()
    for _ in range(2):
        opt.step({k: grads[k].clone() for k in opt.keys})
    first = opt.state_dict()
    opt.load_state_dict(sd)
    assert opt.count == sd["count"]
    for _ in range(2):
        opt.step({k: grads[k].clone() for k in opt.keys})
    second = opt.state_dict()
    assert first["count"] == second["count"] == START + 5
    for part in ("params", "mu", "nu"):
        for k in first[part]:
            assert torch.equal(first[part][k], second[part][k]), (part, k)


# Reference schedule from count 2500 (lr 6.3e-3 for every group here), 40 steps on a fixed batch of 2048 rays.  The first
# run went from 0.196 to 0.132 over the last three steps (ratio 0.68; not monotone: 0.98 at the second step, the first
# full-size Adam step); 0.8 leaves margin on that.
LOOP_STEPS, LOOP_DROP = 40, 0.8
