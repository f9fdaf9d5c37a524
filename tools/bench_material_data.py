"""Times rc_material_data_backward (rc_render_material, the integration's recompute and backward, the head's backward and
the material-grid scatter), the same call without a gradient buffer and rc_render_material at the same size, per call.

  python tools/bench_material_data.py [--rays 8192 32768] [--warmup 3] [--reps 10]
      ms per call on the caller's stream (device events, the median of the repetitions after the warm-up calls);
  python tools/bench_material_data.py --only backward --rays 8192      (the run to profile: the gradient call only)
  python tools/bench_material_data.py --stats <kernel_stats.csv> --rays 8192 --calls 13
      the split of one rocprofv3 --kernel-trace --stats run of this tool (one --rays value) by kernel: the call's own
      kernels (everything after the forward: k_material_data_bwd, k_material_data_head_bwd, k_material_smoothness_reduce,
      k_grid_scatter*) and the rest (rc_render_material's kernels).  Every call of the run is in the file, so the numbers are per run; with
      --calls (warm-up + repetitions of a --only backward run) the tool also reports them per call.
Prints one JSON line per measurement."""
import argparse
import csv
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

OWN = ("k_material_data_bwd", "k_material_data_head_bwd", "k_material_smoothness_reduce", "k_grid_scatter")


def split(stats_path):
    """Kernel ms per kernel name over the whole profiled run, from a rocprofv3 kernel_stats.csv (or its results .db):
    (own, other)."""
    own, other = {}, {}
    if stats_path.endswith(".db"):
        import sqlite3
        rows = sqlite3.connect(stats_path).execute("select name, sum(end - start) from kernels group by name").fetchall()
    else:
        with open(stats_path) as f:
            rows = [(r["Name"], r["TotalDurationNs"]) for r in csv.DictReader(f)]
    for name, total_ns in rows:
        ms = float(total_ns) / 1e6
        key = next((k for k in OWN if k in name), None)
        if key:
            own[key] = own.get(key, 0.0) + ms
        else:
            other[name[:60]] = other.get(name[:60], 0.0) + ms
    return own, other


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, nargs="+", default=[8192, 32768])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--K", type=int, default=8, help="num_secondary_samples")
    ap.add_argument("--stats", default=None)
    ap.add_argument("--calls", type=int, default=0, help="--stats: gradient calls in the profiled run")
    ap.add_argument("--only", nargs="+", default=None, help="time only these calls (backward, loss_only, ...)")
    a = ap.parse_args()
    if a.stats:
        own, other = split(a.stats)
        res = {"rays": a.rays[0], "kernel_ms_per_run_own": {k: round(v, 4) for k, v in own.items()},
               "kernel_ms_per_run_other_total": round(sum(other.values()), 4)}
        if a.calls:
            res["own_ms_per_grad_call"] = {k: round(v / a.calls, 4) for k, v in own.items()}
            res["own_total_ms_per_grad_call"] = round(sum(own.values()) / a.calls, 4)
            res["other_ms_per_grad_call"] = round(sum(other.values()) / a.calls, 4)
        print(json.dumps(res))
        return
    import numpy as np
    import torch
    import common
    import nrc_amd
    from oracle import material_ref
    cfg = nrc_amd.hotdog_config()
    for n in a.rays:
        rc = common.make_rc(weights=common.weights_material_np())
        dev = lambda v: [dev(x) for x in v] if isinstance(v, list) else torch.from_numpy(v).cuda()
        # inputs resident on the device: the calls' host work is argument marshalling only
        rays = {k: dev(v) for k, v in nrc_amd.synthetic_rays(n, seed=3).hot_fields().items()}
        K = a.K
        rnd = {k: dev(v) for k, v in material_ref.draw_randoms(dataclasses.replace(cfg, num_secondary_samples=K), n,
                                                                 seed=4).items()}
        gt = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).uniform(0, 1, (n, 3)).astype(np.float32)).cuda()
        grad = torch.zeros(rc.material_grad_layout()[1], device="cuda")
        calls = {
            "backward": lambda: rc.material_data_backward(rays, rnd, gt, K, grad=grad),
            "loss_only": lambda: rc.material_data_backward(rays, rnd, gt, K, grad=False),
            "forward_render_material": lambda: rc.render_material(rays, rnd, num_secondary_samples=K),
        }
        res = {"rays": n, "K": K}
        for name, fn in calls.items():
            if a.only and name not in a.only:
                continue
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            # device events bracket each call on the caller's stream; the median of the repetitions
            times = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            times.sort()
            res[name + "_ms"] = round(times[len(times) // 2], 4)
        print(json.dumps(res), flush=True)
        rc.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
