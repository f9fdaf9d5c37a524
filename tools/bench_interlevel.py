"""Times rc_interlevel_backward (spline interlevel loss + gradients of both proposal networks) per call.

  python tools/bench_interlevel.py [--rays 8192 65536] [--warmup 5] [--reps 20]
      whole-call ms on the caller's stream (device events, steady state after the warm-up calls), and the device memory
      the call's workspaces took on first use;
  python tools/bench_interlevel.py --stats <kernel_stats.csv> --rays 65536
      the split of one rocprofv3 --kernel-trace --stats run of this tool into the training forward, k_interlevel_bwd and
      the two density backwards, and k_interlevel_bwd's bytes over its kernel time against the HBM peak.
Prints one JSON line per measurement."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_TBS = 8.0        # MI355X HBM3E peak


def il_bytes_per_ray(S):
    """What k_interlevel_bwd moves per ray: sdist + tdist + density of every level, d_density of the proposal levels,
    the ray's direction and its two loss sums."""
    b = 0
    for l, s in enumerate(S):
        b += 4 * (2 * (s + 1) + s)
        if l < len(S) - 1:
            b += 4 * s + 4
    return b + 12


def split(stats_path, n, calls):
    """Kernel time per call by group from a rocprofv3 kernel_stats.csv."""
    groups = {"forward": ("k_sample", "k_level", "k_hashgrid", "k_density_mlp"), "k_interlevel_bwd": ("k_interlevel_bwd",),
              "reduce+copy": ("k_interlevel_reduce", "k_points_aos"),
              "density_backward": ("k_density_bwd", "k_wgrad", "k_grad_reduce", "k_grid_scatter")}
    out = {k: 0.0 for k in groups}
    with open(stats_path) as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            for g, pre in groups.items():
                if any(p in name for p in pre):
                    out[g] += float(row["TotalDurationNs"]) / 1e6 / calls
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, nargs="+", default=[8192, 65536])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    import nrc_amd
    cfg = nrc_amd.hotdog_config()
    S = [s for _, _, s in cfg.sampling_strategy]
    if a.stats:
        calls = a.warmup + a.reps
        n = a.rays[0]
        ms = split(a.stats, n, calls)
        t_il = ms["k_interlevel_bwd"] * 1e-3
        gbs = il_bytes_per_ray(S) * n / t_il / 1e9 if t_il > 0 else 0.0
        print(json.dumps({"rays": n, "ms_per_call": ms, "il_bytes": il_bytes_per_ray(S) * n, "il_GBps": round(gbs, 1),
                          "il_frac_of_hbm_peak": round(gbs / (HBM_PEAK_TBS * 1e3), 3)}))
        return
    import numpy as np
    import torch
    import common
    from nrc_amd import train
    il = nrc_amd.InterlevelConfig()
    for n in a.rays:
        rc = common.make_rc()
        rays = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in nrc_amd.synthetic_rays(n, seed=3).hot_fields().items()
                if k in ("origins", "directions", "viewdirs", "near", "far", "lights")}
        jit = [torch.from_numpy(j.reshape(-1)).cuda() for j in common.jitters(n, seed=4)]
        flats = [torch.zeros(rc.density_grad_layout(l)[1], device="cuda") for l in range(cfg.num_levels - 1)]
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        for _ in range(a.warmup):
            rc.interlevel_backward(rays, jit, train.anneal_at(1.0), il.mults, il.blurs, grads=flats)
        torch.cuda.synchronize()
        ws_gb = (free0 - torch.cuda.mem_get_info()[0]) / 1e9
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            rc.interlevel_backward(rays, jit, train.anneal_at(1.0), il.mults, il.blurs, grads=flats)
        e1.record()
        torch.cuda.synchronize()
        print(json.dumps({"rays": n, "ms_per_call": round(e0.elapsed_time(e1) / a.reps, 4), "workspace_GB": round(ws_gb, 2),
                          "grad_MB": [round(f.numel() * 4 / 1e6, 1) for f in flats]}), flush=True)
        rc.close()
        del flats
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
