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

import bench_common as bc

OWN = ("k_material_data_bwd", "k_material_data_head_bwd", "k_material_smoothness_reduce", "k_grid_scatter")


def main():
    ap = argparse.ArgumentParser()
    bc.add_rays(ap, [8192, 32768])
    bc.add_loop(ap, 3, 10)
    ap.add_argument("--K", type=int, default=8, help="num_secondary_samples")
    bc.add_stats(ap, per_call=True)
    a = ap.parse_args()
    if a.stats:
        bc.emit(bc.own_report(a.stats, OWN, a.rays[0], a.calls))
        return
    import torch
    import loss_cases as lc
    for n in a.rays:
        rc = lc.make_material_rc()
        K = a.K
        rays, rnd = bc.to_device(lc.material_case(n, K, seed=3))
        gt = bc.to_device(lc.uniform_gt(n, 5))
        grad = torch.zeros(rc.material_grad_layout()[1], device="cuda")
        calls = {
            "backward": lambda: rc.material_data_backward(rays, rnd, gt, K, grad=grad),
            "loss_only": lambda: rc.material_data_backward(rays, rnd, gt, K, grad=False),
            "forward_render_material": lambda: rc.render_material(rays, rnd, num_secondary_samples=K),
        }
        bc.emit({"rays": n, "K": K, **bc.time_calls(calls, a.warmup, a.reps, a.only)})
        rc.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
