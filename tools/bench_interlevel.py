"""Times rc_interlevel_backward (spline interlevel loss + gradients of both proposal networks) per call.

  python tools/bench_interlevel.py [--rays 8192 65536] [--warmup 5] [--reps 20]
      whole-call ms on the caller's stream (device events, steady state after the warm-up calls), and the device memory
      the call's workspaces took on first use;
  python tools/bench_interlevel.py --stats <kernel_stats.csv> --rays 65536
      the split of one rocprofv3 --kernel-trace --stats run of this tool into the training forward, k_interlevel_bwd and
      the two density backwards, and k_interlevel_bwd's bytes over its kernel time against the HBM peak.
Prints one JSON line per measurement."""
import argparse
import json

import bench_common as bc

HBM_PEAK_TBS = 8.0        # MI355X HBM3E peak
GROUPS = {"forward": ("k_sample", "k_level", "k_hashgrid", "k_density_mlp"), "k_interlevel_bwd": ("k_interlevel_bwd",),
          "reduce+copy": ("k_interlevel_reduce", "k_points_aos"),
          "density_backward": ("k_density_bwd", "k_wgrad", "k_grad_reduce", "k_grid_scatter")}


def il_bytes_per_ray(S):
    """What k_interlevel_bwd moves per ray: sdist + tdist + density of every level, d_density of the proposal levels,
    the ray's direction and its two loss sums."""
    b = 0
    for l, s in enumerate(S):
        b += 4 * (2 * (s + 1) + s)
        if l < len(S) - 1:
            b += 4 * s + 4
    return b + 12


def main():
    ap = argparse.ArgumentParser()
    bc.add_rays(ap, [8192, 65536])
    bc.add_loop(ap, 5, 20)
    bc.add_stats(ap)
    a = ap.parse_args()
    import nrc_amd
    cfg = nrc_amd.hotdog_config()
    S = [s for _, _, s in cfg.sampling_strategy]
    if a.stats:
        n = a.rays[0]
        ms = bc.split_groups(a.stats, GROUPS, a.warmup + a.reps)
        t_il = ms["k_interlevel_bwd"] * 1e-3
        gbs = il_bytes_per_ray(S) * n / t_il / 1e9 if t_il > 0 else 0.0
        print(json.dumps({"rays": n, "ms_per_call": ms, "il_bytes": il_bytes_per_ray(S) * n, "il_GBps": round(gbs, 1),
                          "il_frac_of_hbm_peak": round(gbs / (HBM_PEAK_TBS * 1e3), 3)}))
        return
    import torch
    import common
    import loss_cases as lc
    from nrc_amd import train
    il = nrc_amd.InterlevelConfig()
    for n in a.rays:
        rc = common.make_rc()
        rays, jit = bc.to_device(lc.cache_case(n, seed=3))
        flats = [torch.zeros(rc.density_grad_layout(l)[1], device="cuda") for l in range(cfg.num_levels - 1)]
        call = lambda: rc.interlevel_backward(rays, jit, train.anneal_at(1.0), il.mults, il.blurs, grads=flats)
        bc.emit({"rays": n, **bc.time_whole_call(call, a.warmup, a.reps, flats)})
        rc.close()
        del flats
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
