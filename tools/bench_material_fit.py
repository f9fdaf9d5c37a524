"""Timing of the material stage's train step from a PRNG key, per step at K = 8:

  randoms   rc.material_randoms (plan in C, one arena, one launch) against prng.material_pass_randoms +
            material_smoothness_noise + upload, the only path before it; the C plan and the launch on their own
  kernel    k_prng_fill_segments: device events around `--launches` back-to-back launches of one plan, against the byte
            floor of 4 B per value at 6.3 TB/s (the rate tools/bench_train_step.py holds k_adam to)
  step      train.material_stage_fit against the same loop with host randoms (both run this commit's step kernels)

Host-clock times around work that ends in a device synchronise (the host path's time IS host time); the two variants of
a pair alternate inside one process.  One JSON line per ray count; --out appends them to a .jsonl.

  python tools/bench_material_fit.py [--rays 1024 4096] [--reps 7] [--steps 10] [--out profiles/material_fit_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import nrc_amd  # noqa: E402
from nrc_amd import config, data, prng, rc_ext, train  # noqa: E402

K = 8
HBM_BPS = 6.3e12


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(a, b, reps, warm=2):
    """Median wall ms of a() and of b(), the two alternating."""
    for _ in range(warm):
        a(), b()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(wall(a))
        tb.append(wall(b))
    return statistics.median(ta), statistics.median(tb), ta, tb


def cameras(count, H, W, seed=9, radius=4.03):
    from test_gpu_train_batch import _cameras
    return _cameras(count, H, W, seed=seed, radius=radius)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, nargs="*", default=[1024, 4096])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_material_fit: no GPU (timings are taken on the device only)")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cfg = nrc_amd.hotdog_config()
    weights = nrc_amd.synthetic_weights(cfg, passes=("cache", "material"))
    rc = rc_ext.RadianceCache(cfg, 0)
    rc.load_weights(weights)
    dcfg = config.MaterialDataLossConfig()
    mcfg = nrc_amd.hotdog_config(num_secondary_samples=K)
    ocfg = config.OptimizerConfig(material=True)
    H = W = 64
    p2c, c2w, lights = cameras(4, H, W)
    images = torch.from_numpy(np.random.default_rng(1).uniform(size=(4, H, W, 3)).astype(np.float32))
    key, loss_key = prng.PRNGKey(5), prng.PRNGKey(6)
    levels = [lvl[2] for lvl in cfg.sampling_strategy]
    for n in args.rays:
        res = {"rays": n, "K": K, "source_hash": rc_ext.source_hash()}
        # -- the randoms alone
        def host_randoms(k=key, lk=loss_key):
            rnd = prng.material_pass_randoms(k, n, mcfg)
            rnd["noise"] = prng.material_smoothness_noise(lk, n)
            return {name: ([rc._dev(x) for x in v] if isinstance(v, list) else rc._dev(v)) for name, v in rnd.items()}
        dev_ms, host_ms, _, th = alternate(lambda: rc.material_randoms(key, n, K, train=True, loss_key=loss_key), host_randoms,
                                           args.reps)
        res.update(randoms_device_ms=dev_ms, randoms_host_ms=host_ms, randoms_host_ms_all=[round(v, 2) for v in th])
        flags = rc_ext.RC_PRNG_PLAN_TRAIN
        t = time.perf_counter()
        for _ in range(100):
            segs, count, words = rc_ext.material_randoms_plan(key, n, K, cfg.diffuse_sample_fraction, cfg.num_vmf, levels, flags,
                                                              loss_key)
        res["plan_ms"] = (time.perf_counter() - t) * 10.0
        values = sum(segs[i].n for i in range(count))
        arena = torch.empty(words, dtype=torch.float32, device="cuda")
        fill = lambda: rc.lib.rc_prng_fill_segments(rc._h, segs, count, arena.data_ptr(), words, rc._stream())
        for _ in range(5):
            fill()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.launches):
            fill()
        b.record()
        torch.cuda.synchronize()
        res.update(values=values, arena_words=words, segments=count, fill_ms_per_launch=a.elapsed_time(b) / args.launches,
                   fill_floor_ms=4.0 * values / HBM_BPS * 1e3, fill_one_launch_wall_ms=statistics.median(wall(fill) for _ in range(9)))
        # -- the whole step
        ds = data.DeviceDataset(rc, p2c, c2w, images, lights=lights, near=2.0, far=6.0, batch_size=n)
        om, oe = train.MaterialOptimizer(rc, ocfg), train.EnvMapOptimizer(rc, ocfg)
        om.init_from(weights, count=0)
        oe.init_from(weights, count=0)

        def host_loop(k=key):
            rng = prng.as_key(k)
            for _ in range(args.steps):
                step_key, rng = prng.random_split(rng)
                batch_key, k2 = prng.random_split(step_key)
                model_key, lk = prng.random_split(k2)
                batch = ds.next_train(batch_key)
                rnd = host_randoms(model_key, prng.extra_loss_keys(lk)["material_smoothness"])
                train.material_env_stage_step(rc, om, oe, batch.rays.hot_fields(), rnd, batch.rgb, rnd["noise"],
                                              batch.rays.lossmult, None, dcfg)
        fit_ms, loop_ms, tf, tl = alternate(lambda: train.material_stage_fit(rc, om, oe, ds, key, args.steps, data_cfg=dcfg),
                                            host_loop, max(3, args.reps // 2), warm=1)
        res.update(step_device_ms=fit_ms / args.steps, step_host_randoms_ms=loop_ms / args.steps,
                   step_device_ms_all=[round(v / args.steps, 3) for v in tf],
                   step_host_randoms_ms_all=[round(v / args.steps, 2) for v in tl])
        print(json.dumps(res), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
