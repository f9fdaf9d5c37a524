"""Times rc_geometry_smoothness_backward and, in the same process, what it is set beside: rc_geometry_backward
on the same rays, two rc_density_backward calls and two rc_normals_backward calls at rays x 32 points.

  python tools/bench_geometry_smoothness.py [--rays 1024] [--warmup 3] [--reps 20] [--only backward ...]
      ms per call on the caller's stream (device events, the median of the repetitions after the warm-up calls);
  python tools/bench_geometry_smoothness.py --stats <kernel_stats.csv> --calls 23
      the kernels of one rocprofv3 --kernel-trace --stats run of `--only backward` by group, per gradient call.
Prints one JSON line per measurement."""
import argparse
import json

import bench_common as bc

GROUPS = {"forward": ("k_sample", "k_level", "k_hashgrid", "k_density_mlp", "k_cache_fused"),
          "points+loss+reduce": ("k_gsmooth_points", "k_gsmooth_loss", "k_interlevel_reduce"),
          "k_normals_bwd": ("k_normals_bwd",), "wgrad": ("k_wgrad", "k_grad_reduce"),
          "k_grid_scatter_jac": ("k_grid_scatter_jac",)}


def main():
    ap = argparse.ArgumentParser()
    bc.add_rays(ap, [1024])
    bc.add_loop(ap, 3, 20)
    bc.add_stats(ap, per_call=True)
    a = ap.parse_args()
    if a.stats:
        ms = bc.split_groups(a.stats, GROUPS, max(a.calls, 1), other="other")
        print(json.dumps({"rays": a.rays[0], "kernel_ms_per_grad_call": {k: round(v, 4) for k, v in ms.items()}}))
        return
    import numpy as np
    import torch
    import common
    import loss_cases as lc
    import nrc_amd
    from nrc_amd import train
    cfg = nrc_amd.hotdog_config()
    S2, last = cfg.sampling_strategy[-1][2], cfg.num_levels - 1
    for n in a.rays:
        rc = common.make_rc()
        rays, jit = bc.to_device(lc.cache_case(n, seed=3))
        rng = np.random.Generator(np.random.PCG64(4))
        noise = bc.to_device(rng.standard_normal((n, S2, 3)).astype(np.float32))
        pts = bc.to_device((rng.standard_normal((n * S2, 3)) * 1.2).astype(np.float32))
        dd = bc.to_device(rng.standard_normal(n * S2).astype(np.float32))
        dn = bc.to_device(rng.standard_normal((n * S2, 3)).astype(np.float32))
        flat = torch.zeros(rc.density_grad_layout(last)[1], device="cuda")
        shader = torch.zeros(rc.shader_grad_layout()[1], device="cuda")
        terms, gterms, anneal = train.geometry_smoothness_terms(1.0), train.geometry_terms(1.0), train.anneal_at(1.0)

        def twice(fn):
            fn()
            fn()

        calls = {"backward": lambda: rc.geometry_smoothness_backward(rays, jit, anneal, noise, None, terms, flat),
                 "loss_only": lambda: rc.geometry_smoothness_backward(rays, jit, anneal, noise, None, terms, False),
                 "geometry_backward": lambda: rc.geometry_backward(rays, jit, anneal, None, gterms, grads=[flat, shader]),
                 "two_density_backward": lambda: twice(lambda: rc.density_backward(last, pts, dd, None, flat)),
                 "two_normals_backward": lambda: twice(lambda: rc.normals_backward(pts, dn, flat))}
        bc.emit({"rays": n, "points": n * S2, **bc.time_calls(calls, a.warmup, a.reps, a.only)})
        rc.close()


if __name__ == "__main__":
    main()
