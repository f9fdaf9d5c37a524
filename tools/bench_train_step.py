"""Timing of the cache stage's optimizer step: k_adam over the four flat buffers, the parts of the
handle's refresh, and the whole cache_stage_step against cache_stage_grads alone and against the torch.optim.Adam +
load_weights loop.  Call times are device events around the call on the current stream (the host waits inside
rc_load_params_flat, so a call's event span includes that wait); kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script.

  python tools/bench_train_step.py [--rays 8192 65536] [--reps 10] [--out profiles/train_step.json]
  RC_REC4_TABLES=0 python tools/bench_train_step.py --parts-only     (the refresh without the F = 4 cell records)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import nrc_amd  # noqa: E402
from nrc_amd import rc_ext, train  # noqa: E402

START = 2500


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), out


def case(n, seed=41):
    rays = nrc_amd.synthetic_rays(n, seed=seed).hot_fields()
    rays = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in rays.items()
            if k in ("origins", "directions", "viewdirs", "near", "far", "lights")}
    rng = np.random.default_rng(seed + 1)
    jit = [torch.from_numpy(rng.uniform(size=n).astype(np.float32)).cuda() for _ in range(3)]
    return rays, jit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, nargs="*", default=[8192, 65536])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parts-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cfg = nrc_amd.hotdog_config()
    weights = nrc_amd.synthetic_weights(cfg)
    rc = rc_ext.RadianceCache(cfg, 0)
    rc.load_weights(weights)
    opt = train.CacheStageOptimizer(rc)
    opt.init_from(weights, count=START)
    res = {"rec4_tables": os.environ.get("RC_REC4_TABLES", "1"), "source_hash": rc_ext.source_hash()}
    nparam = sum(opt.layouts[k][1] for k in opt.keys)
    res["params"] = nparam

    # 1. k_adam alone (one launch over the four buffers), with and without zeroing the gradients
    for zero in (True, False):
        sc = train.adam_scalars(START, opt.cfg, zero_grads=zero)
        ms, _ = timed(lambda: rc.adam_update(opt._table, sc), args.reps)
        moved = nparam * (32 if zero else 28)
        res[f"adam_ms_zero{int(zero)}"] = ms
        res[f"adam_GBps_zero{int(zero)}"] = moved / ms / 1e6
        res[f"adam_floor_ms_zero{int(zero)}"] = moved / 6.3e12 * 1e3
    # 2. the refresh: rc_load_params_flat per layout (table copies + the dense layers' one copy and wait), then the
    #    first render after it (repack + derived-table rebuild) against a steady render of the same batch
    small, sjit = case(256, seed=3)
    render = lambda: rc.render_rays(small, {"jitter": sjit}, outputs=["rgb"])
    render()
    torch.cuda.synchronize()
    for k in opt.keys:
        ms, _ = timed(lambda: rc.load_params_flat(k, opt.params[k]), args.reps)
        res[f"load_params_flat_ms_{k}"] = ms
    steady, _ = timed(render, args.reps)

    def refresh_then_render():
        opt.refresh()
        render()
    both, _ = timed(refresh_then_render, args.reps)
    refresh, _ = timed(opt.refresh, args.reps)
    res["render256_steady_ms"] = steady
    res["refresh_ms"] = refresh
    res["first_render_after_refresh_ms"] = both - refresh
    res["rebuild_ms"] = both - refresh - steady
    if args.parts_only:
        print(json.dumps(res))
        return
    # 3. whole steps
    target = rc_ext.RadianceCache(cfg, 0)
    target.load_weights(nrc_amd.synthetic_weights(cfg, seed=2))
    for n in args.rays:
        rays, jit = case(n)
        gt = target.render_rays(rays, {"jitter": jit}, outputs=["rgb"])["rgb"].reshape(n, 3).contiguous()
        tf = train.train_frac_at(START, 25000)
        ms_step, _ = timed(lambda: train.cache_stage_step(rc, opt, rays, gt, jit), args.reps)
        flats = {k: torch.zeros_like(opt.grads[k]) for k in opt.keys}

        def grads_only():
            for v in flats.values():
                v.zero_()
            train.cache_stage_grads(rc, rays, gt, jit, tf, flats=flats)
        ms_grads, _ = timed(grads_only, args.reps)
        # the old loop: per-tensor .grad, torch.optim.Adam, load_weights
        params = {k: v.detach().clone() for k, v in opt.params_dict().items()}
        topt = torch.optim.Adam(params.values(), lr=1e-3, betas=(0.9, 0.99), eps=1e-15)
        lays = {k: opt.layouts[k][0] for k in opt.keys}

        def old_step():
            grads_only()
            for k, lay in lays.items():
                for name, v in train.grads_as_dict(flats[k], lay).items():
                    params[name].grad = v.clone()
            topt.step()
            rc.load_weights(params)
        ms_old, _ = timed(old_step, max(3, args.reps // 2))
        opt.refresh()
        res[f"step_ms_{n}"] = ms_step
        res[f"cache_stage_grads_ms_{n}"] = ms_grads
        res[f"old_torch_adam_load_weights_ms_{n}"] = ms_old
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
