"""Times rc_material_smoothness_backward (the primary pass and shading point, both material evaluations, the loss and the
MaterialShader gradients), the same call without a gradient buffer, rc_render_material at the same size and
rc_material_regularizer, per call.

  python tools/bench_material_smoothness.py [--rays 8192 32768] [--warmup 3] [--reps 10]
      ms per call on the caller's stream (device events, the median of the repetitions after the warm-up calls);
  python tools/bench_material_smoothness.py --only backward --rays 8192      (the run to profile: the gradient call only)
  python tools/bench_material_smoothness.py --stats <kernel_stats.csv> --rays 8192 --calls 13
      the split of one rocprofv3 --kernel-trace --stats run of this tool (one --rays value) by kernel: the call's own
      kernels (k_material_smoothness_points, the material-grid lookup k_hashgrid_fwd, k_material_smoothness_bwd,
      k_material_smoothness_reduce, k_grid_scatter*, the regularizer's k_grid_l2_*) and the rest (material_primary and
      rc_render_material's other kernels).  Every call of the run is in the file, so the numbers are per run; with
      --calls (warm-up + repetitions of a --only backward run) the tool also reports them per call.
Prints one JSON line per measurement."""
import argparse

import bench_common as bc

OWN = ("k_material_smoothness_points", "k_material_smoothness_bwd", "k_material_smoothness_reduce", "k_grid_scatter",
       "k_grid_l2_bwd", "k_grid_l2_reduce", "k_hashgrid_fwd")


def main():
    ap = argparse.ArgumentParser()
    bc.add_rays(ap, [8192, 32768])
    bc.add_loop(ap, 3, 10)
    bc.add_stats(ap, per_call=True)
    a = ap.parse_args()
    if a.stats:
        bc.emit(bc.own_report(a.stats, OWN, a.rays[0], a.calls))
        return
    import torch
    import loss_cases as lc
    for n in a.rays:
        rc = lc.make_material_rc()
        rays, rnd = bc.to_device(lc.material_case(n, seed=3))
        noise = bc.to_device(lc.normal_noise(n, 5))
        grad = torch.zeros(rc.material_grad_layout()[1], device="cuda")
        calls = {
            "backward": lambda: rc.material_smoothness_backward(rays, rnd, noise, grad=grad),
            "loss_only": lambda: rc.material_smoothness_backward(rays, rnd, noise, grad=False),
            "forward_render_material": lambda: rc.render_material(rays, rnd),
            "regularizer": lambda: rc.material_regularizer(1.0, grad),
        }
        bc.emit({"rays": n, **bc.time_calls(calls, a.warmup, a.reps, a.only)})
        rc.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
