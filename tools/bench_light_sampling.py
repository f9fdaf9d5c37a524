"""Times rc_light_sampling_backward (the material forward up to the secondary trace, the light_sampling loss and the
LightSampler gradients), the forward alone (rc_render_material at the same size) and rc_light_regularizer, per call.

  python tools/bench_light_sampling.py [--rays 8192 32768] [--k 8] [--warmup 3] [--reps 10]
      ms per call on the caller's stream (device events, steady state after the warm-up calls) of the three calls;
  python tools/bench_light_sampling.py --stats <kernel_stats.csv> --rays 8192
      the split of one rocprofv3 --kernel-trace --stats run of this tool (one --rays value) into the material forward,
      the light head's recompute + backward GEMMs, k_light_sampling_loss_bwd, the light grid's scatter and the
      regularizer; every call of the run (forward-only, backward and regularizer calls) is in the file, so the groups are
      reported per run, not per call.
Prints one JSON line per measurement."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def split(stats_path):
    """Kernel ms per group over the whole profiled run, from a rocprofv3 kernel_stats.csv."""
    groups = {"k_light_sampling_loss_bwd": ("k_light_sampling_loss_bwd",), "gemm": ("k_gemm", "k_sum_parts"),
              "grid_scatter": ("k_grid_scatter",), "regularizer": ("k_grid_l2",), "reduce": ("k_interlevel_reduce",)}
    out = {k: 0.0 for k in groups}
    out["other (material forward)"] = 0.0
    with open(stats_path) as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            for g, pre in groups.items():
                if any(p in name for p in pre):
                    out[g] += float(row["TotalDurationNs"]) / 1e6
                    break
            else:
                out["other (material forward)"] += float(row["TotalDurationNs"]) / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, nargs="+", default=[8192, 32768])
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    if a.stats:
        ms = split(a.stats)
        print(json.dumps({"rays": a.rays[0], "k": a.k, "calls_each": a.warmup + a.reps,
                          "kernel_ms_per_run": {k: round(v, 4) for k, v in ms.items()}}))
        return
    import dataclasses

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
        rnd = {k: dev(v) for k, v in material_ref.draw_randoms(dataclasses.replace(cfg, num_secondary_samples=a.k), n,
                                                                 seed=4).items()}
        grad = torch.zeros(rc.light_grad_layout()[1], device="cuda")
        calls = {
            "backward": lambda: rc.light_sampling_backward(rays, rnd, a.k, grad=grad),
            "forward_render_material": lambda: rc.render_material(rays, rnd, a.k),
            "regularizer": lambda: rc.light_regularizer(1.0, grad),
        }
        res = {"rays": n, "k": a.k}
        for name, fn in calls.items():
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
        res["backward_over_forward"] = round(res["backward_ms"] / res["forward_render_material_ms"], 3)
        print(json.dumps(res), flush=True)
        rc.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
