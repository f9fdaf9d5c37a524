"""Shared helpers of the GPU loss tests (test_gpu_interlevel, _data_loss, _geometry_loss, _light_sampling,
_material_smoothness, _material_data_loss, _optimizer): seeded cases, views of the training workspaces, the error bound
against the fp32 restatement, and the training-loop bodies.  Test helper, not a test module."""
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


def bound(got, ref64, ref32, floor=0.0, rel_floor=None, what=None):
    """max|got - ref64| against 3x the fp32 restatement's own distance from fp64 plus a floor.  With `floor` (absolute)
    returns (err, bound) for the caller to assert; with `rel_floor` (times max|ref64|, plus 1e-12) asserts itself."""
    err, err32 = float(np.abs(got - ref64).max()), float(np.abs(ref32 - ref64).max())
    if rel_floor is None:
        return err, 3.0 * err32 + floor
    tol = 3.0 * err32 + rel_floor * float(np.abs(ref64).max()) + 1e-12
    assert err <= tol, (what, err, err32, tol)


def check(got, ref64, ref32, what, rel_floor=1e-6):
    bound(got, ref64, ref32, rel_floor=rel_floor, what=what)


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
