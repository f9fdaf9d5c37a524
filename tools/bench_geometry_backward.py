"""Times rc_geometry_backward (distortion, orientation and predicted-normal losses + gradients of MLP_2 and
pred_normals_layer) per call.

  python tools/bench_geometry_backward.py [--rays 8192 65536] [--warmup 3] [--reps 10]
      whole-call ms on the caller's stream (device events, steady state after the warm-up calls), and the device memory
      the call's workspaces took on first use;
  python tools/bench_geometry_backward.py --stats <kernel_stats.csv> --rays 8192
      the split of one rocprofv3 --kernel-trace --stats run of this tool into the training forward, k_geometry_loss_bwd,
      the pred_normals_layer GEMMs, the level-2 density backward and the grid scatter, and k_geometry_loss_bwd's bytes
      per sample against the HBM peak.
Prints one JSON line per measurement."""
import argparse
import json

import bench_common as bc

HBM_PEAK_TBS = 8.0             # MI355X HBM3E peak
# k_geometry_loss_bwd's compulsory traffic per sample: weights, density, tdist, normals_pred, normals_grad (3 + 3),
# hbuf (64), d_density and d_pred (3) written -- 4 x (1 + 1 + 1 + 6 + 64 + 1 + 3) bytes
LOSS_BYTES_PER_SAMPLE = 4 * (1 + 1 + 1 + 6 + 64 + 1 + 3)
GROUPS = {"forward": ("k_sample", "k_level", "k_hashgrid", "k_density_mlp"),
          "k_geometry_loss_bwd": ("k_geometry_loss_bwd",), "reduce+copy": ("k_interlevel_reduce", "k_points_aos"),
          "pred_layer": ("k_gemm", "k_sum_parts", "k_stage_hidden"),
          "density_backward": ("k_density_bwd", "k_wgrad", "k_grad_reduce"), "grid_scatter": ("k_grid_scatter",)}


def main():
    ap = argparse.ArgumentParser()
    bc.add_rays(ap, [8192, 65536])
    bc.add_loop(ap, 3, 10)
    bc.add_stats(ap)
    a = ap.parse_args()
    import nrc_amd
    cfg = nrc_amd.hotdog_config()
    S2 = cfg.sampling_strategy[-1][2]
    if a.stats:
        n = a.rays[0]
        ms = bc.split_groups(a.stats, GROUPS, a.warmup + a.reps)
        nbytes = LOSS_BYTES_PER_SAMPLE * n * S2
        t = ms["k_geometry_loss_bwd"] * 1e-3
        floor_ms = nbytes / (HBM_PEAK_TBS * 1e12) * 1e3
        print(json.dumps({"rays": n, "ms_per_call": {k: round(v, 4) for k, v in ms.items()},
                          "loss_bytes_per_sample": LOSS_BYTES_PER_SAMPLE, "loss_floor_ms": round(floor_ms, 4),
                          "loss_frac_of_hbm_peak": round(nbytes / t / (HBM_PEAK_TBS * 1e12), 3) if t > 0 else 0.0}))
        return
    import torch
    import common
    import loss_cases as lc
    from nrc_amd import train
    for n in a.rays:
        rc = common.make_rc()
        rays, jit = bc.to_device(lc.cache_case(n, seed=3))
        terms = train.geometry_terms(1.0)
        flats = [torch.zeros(rc.density_grad_layout(cfg.num_levels - 1)[1], device="cuda"),
                 torch.zeros(rc.shader_grad_layout()[1], device="cuda")]
        call = lambda: rc.geometry_backward(rays, jit, train.anneal_at(1.0), None, terms, grads=flats)
        bc.emit({"rays": n, **bc.time_whole_call(call, a.warmup, a.reps, flats)})
        rc.close()
        del flats
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
