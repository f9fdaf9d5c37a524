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
import json

import bench_common as bc

GROUPS = {"k_light_sampling_loss_bwd": ("k_light_sampling_loss_bwd",), "gemm": ("k_gemm", "k_sum_parts"),
          "grid_scatter": ("k_grid_scatter",), "regularizer": ("k_grid_l2",), "reduce": ("k_interlevel_reduce",)}


def main():
    ap = argparse.ArgumentParser()
    bc.add_rays(ap, [8192, 32768])
    ap.add_argument("--k", type=int, default=8)
    bc.add_loop(ap, 3, 10)
    bc.add_stats(ap)
    a = ap.parse_args()
    if a.stats:
        ms = bc.split_groups(a.stats, GROUPS, other="other (material forward)")
        print(json.dumps({"rays": a.rays[0], "k": a.k, "calls_each": a.warmup + a.reps,
                          "kernel_ms_per_run": {k: round(v, 4) for k, v in ms.items()}}))
        return
    import torch
    import loss_cases as lc
    for n in a.rays:
        rc = lc.make_material_rc()
        rays, rnd = bc.to_device(lc.material_case(n, a.k, seed=3))
        grad = torch.zeros(rc.light_grad_layout()[1], device="cuda")
        calls = {
            "backward": lambda: rc.light_sampling_backward(rays, rnd, a.k, grad=grad),
            "forward_render_material": lambda: rc.render_material(rays, rnd, a.k),
            "regularizer": lambda: rc.light_regularizer(1.0, grad),
        }
        res = {"rays": n, "k": a.k, **bc.time_calls(calls, a.warmup, a.reps)}
        res["backward_over_forward"] = round(res["backward_ms"] / res["forward_render_material_ms"], 3)
        bc.emit(res)
        rc.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
