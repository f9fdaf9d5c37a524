"""Time of building one training batch: 100 cameras of 800 x 800, batching = all_images.

  --mode new      DeviceDataset.next_train(key): one rc_train_batch launch (cameras, pixels, rays, colours, lossmult);
                  and cache_stage_fit's time per step beside cache_stage_step alone on pre-built tensors
  --mode parent   the way before rc_train_batch: host picks -> model._cast_pixels on a host Pixels batch (one rc_cast_rays
                  per distinct camera, torch.cat, a permutation gather) + a torch gather of images[cam, y, x].  Uses
                  nothing newer than that, so `--root <checkout of the parent commit, built>` times the parent's own code.

Both modes: a warm-up, then --reps repetitions with a distinct key / seed each, HIP events around the call on the current
stream and the wall clock around call + synchronize; the median of each.  One JSON line per batch size, appended to --out.
"""
import argparse
import json
import os
import socket
import sys
import time


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def _timed(torch, fn, warmup, reps):
    """fn(i) with i distinct per call -> (median event ms, median wall ms)."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ev, wall = [], []
    for i in range(warmup, warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn(i)
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(e0.elapsed_time(e1))
    return _median(ev), _median(wall)


def _scene(np, nrc_amd, count, size):
    rng = np.random.default_rng(1)
    o = rng.normal(size=(count, 3)); o[:, 2] = np.abs(o[:, 2]) + 0.3
    o = 4.03 * o / np.linalg.norm(o, axis=1, keepdims=True)
    c2w = []
    for v in o:
        look = -v / np.linalg.norm(v)
        right = np.cross(look, [0.0, 0.0, 1.0]); right /= np.linalg.norm(right)
        c2w.append(np.concatenate([np.stack([right, np.cross(right, look), -look], axis=1), v[:, None]], axis=1))
    p2c = np.stack([nrc_amd.get_pixtocam(1111.0 * size / 800.0, size, size)] * count)
    return p2c.astype(np.float32), np.stack(c2w).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("new", "parent"), default="new")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--rays", type=int, nargs="+", default=[1024, 8192, 65536])
    ap.add_argument("--cameras", type=int, default=100)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--fit-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import numpy as np
    import torch

    import nrc_amd
    from nrc_amd import model as M
    from nrc_amd import prng, rc_ext, train

    cfg = nrc_amd.hotdog_config()
    m = M.Model(cfg, 0)
    weights = nrc_amd.synthetic_weights(cfg)
    m.load_variables(weights)
    rc = m.rc
    C, S = args.cameras, args.size
    p2c, c2w = _scene(np, nrc_amd, C, S)
    images = torch.empty((C, S, S, 3), dtype=torch.float32, device="cuda").uniform_()
    head = dict(box=socket.gethostname(), mode=args.mode, cameras=C, size=S, warmup=args.warmup, reps=args.reps,
                library=rc_ext.source_hash())
    lines = []

    for n in args.rays:
        if args.mode == "new":
            from nrc_amd import data
            ds = data.DeviceDataset(rc, p2c, c2w, images, near=2.0, far=6.0, batch_size=n)
            keys = prng.split(prng.PRNGKey(3), args.warmup + args.reps)
            ev, wall = _timed(torch, lambda i: ds.next_train(keys[i]), args.warmup, args.reps)
        else:
            cameras = (p2c, c2w, None, None, None)
            lights = c2w[:, :, 3]

            def build(i):
                rng = np.random.default_rng(i)
                cam = rng.integers(0, C, n).astype(np.int32)
                px, py = rng.integers(0, S, n).astype(np.int32), rng.integers(0, S, n).astype(np.int32)
                col = lambda v, dt=np.float32: np.full((n, 1), v, dt)
                pixels = nrc_amd.Pixels(pix_x_int=px, pix_y_int=py, lossmult=col(1.0), near=col(2.0), far=col(6.0),
                                        cam_idx=cam[:, None], light_idx=col(0, np.int32))
                rays = M._cast_pixels(m, cameras, lights, pixels, "perspective")
                idx = torch.from_numpy(np.stack([cam, py, px]).astype(np.int64)).cuda()
                return rays, images[idx[0], idx[1], idx[2]]

            ev, wall = _timed(torch, build, args.warmup, args.reps)
        lines.append(dict(head, what="batch", rays=n, event_ms=round(ev, 4), wall_ms=round(wall, 4)))
        print(json.dumps(lines[-1]), flush=True)

    if args.mode == "new":
        from nrc_amd import data
        n = 1024
        ds = data.DeviceDataset(rc, p2c, c2w, images, near=2.0, far=6.0, batch_size=n)
        opt = train.CacheStageOptimizer(rc)
        opt.init_from(weights, count=2500)
        K = args.fit_steps
        train.cache_stage_fit(rc, opt, ds, prng.PRNGKey(1), 3)               # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        train.cache_stage_fit(rc, opt, ds, prng.PRNGKey(2), K)
        torch.cuda.synchronize()
        fit_ms = (time.perf_counter() - t0) * 1e3 / K
        b = ds.next_train(prng.PRNGKey(4))
        jit = [rc.prng_fill(k, (n, 1), "uniform") for k in prng.split(prng.PRNGKey(5), cfg.num_levels)]
        fields = b.rays.hot_fields()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            train.cache_stage_step(rc, opt, fields, b.rgb, jit, b.rays.lossmult)
        torch.cuda.synchronize()
        step_ms = (time.perf_counter() - t0) * 1e3 / K
        lines.append(dict(head, what="fit", rays=n, steps=K, cache_stage_fit_ms_per_step=round(fit_ms, 3),
                          cache_stage_step_alone_ms=round(step_ms, 3)))
        print(json.dumps(lines[-1]), flush=True)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
