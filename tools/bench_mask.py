"""Times rc_mask_backward (the mask loss of the last level's opacity + the gradient of MLP_2) per call, beside
rc_geometry_backward with gradients in the same process: the mask call runs a subset of that call's work.

  python tools/bench_mask.py [--rays 8192 65536] [--warmup 3] [--reps 10] [--out profiles/mask_bench.jsonl]
      whole-call ms on the caller's stream (device events, steady state after the warm-up calls) with and without
      density_grads, the backward term's call (zero masks) and rc_backward_mask_rays, the device memory the call's
      workspaces took on first use, and rc_geometry_backward with both gradient buffers at the same ray count;
  python tools/bench_mask.py --stats <kernel_stats.csv> --rays 65536
      the split of one rocprofv3 --kernel-trace --stats run of this tool into the training forward, k_mask_loss_bwd, the
      reduce and copy, the level-2 density backward and the grid scatter, and k_mask_loss_bwd's bytes per ray against the
      6.3 TB/s copy rate.
Prints one JSON line per measurement (and appends it to --out)."""
import argparse
import json
import os

import bench_common as bc

COPY_RATE_TBS = 6.3            # measured device copy rate
# k_mask_loss_bwd's compulsory traffic per ray at S = 32: density (32), tdist (33), directions (3), mask, lossmult read;
# weights (32), d_density (32), loss_ray written
LOSS_BYTES_PER_RAY = 4 * (32 + 33 + 3 + 1 + 1 + 32 + 32 + 1)
GROUPS = {"forward": ("k_sample", "k_level", "k_hashgrid", "k_density_mlp"), "k_mask_loss_bwd": ("k_mask_loss_bwd",),
          "k_backward_mask_rays": ("k_backward_mask_rays",), "k_geometry_loss_bwd": ("k_geometry_loss_bwd",),
          "reduce+copy": ("k_interlevel_reduce", "k_points_aos"), "pred_layer": ("k_gemm", "k_sum_parts", "k_stage_hidden"),
          "density_backward": ("k_density_bwd", "k_wgrad", "k_grad_reduce"), "grid_scatter": ("k_grid_scatter",)}


def main():
    ap = argparse.ArgumentParser()
    bc.add_rays(ap, [8192, 65536])
    bc.add_loop(ap, 3, 10)
    bc.add_stats(ap)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-geometry", action="store_true", help="leave the rc_geometry_backward yardstick out (for --stats runs)")
    a = ap.parse_args()
    import nrc_amd
    cfg = nrc_amd.hotdog_config()
    if a.stats:
        n = a.rays[0]
        ms = bc.split_groups(a.stats, GROUPS, 1, other="other")
        kernel = {name: float(ns) / 1e6 for name, ns in bc.kernel_rows(a.stats) if "k_mask_loss_bwd" in name}
        calls = {name: int(r) for name, r in _calls(a.stats) if "k_mask_loss_bwd" in name}
        per_launch = sum(kernel.values()) / max(sum(calls.values()), 1)
        nbytes = LOSS_BYTES_PER_RAY * n
        floor_ms = nbytes / (COPY_RATE_TBS * 1e12) * 1e3
        bc.emit({"rays": n, "kernel_ms_per_run": {k: round(v, 4) for k, v in ms.items()},
                 "k_mask_loss_bwd_launches": sum(calls.values()), "k_mask_loss_bwd_ms": round(per_launch, 5),
                 "loss_bytes_per_ray": LOSS_BYTES_PER_RAY, "loss_floor_ms_at_copy_rate": round(floor_ms, 5),
                 "loss_times_floor": round(per_launch / floor_ms, 2) if floor_ms > 0 else 0.0})
        return
    import torch
    import common
    import loss_cases as lc
    from nrc_amd import train
    from nrc_amd.config import MaskLossConfig
    terms = train.mask_terms(1.0)
    c = MaskLossConfig()
    L2 = cfg.num_levels - 1
    for n in a.rays:
        rc = common.make_rc()
        rays, jit = bc.to_device(lc.cache_case(n, seed=3))
        masks = (torch.arange(n, device="cuda") % 2).float()
        look = -rays["origins"] / rays["origins"].norm(dim=-1, keepdim=True)
        u = torch.rand(n, 2, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
        u1, u2 = u[:, 0].contiguous(), u[:, 1].contiguous()
        back = rc.backward_mask_rays(rays["origins"], look, u1, u2, c.shadow_near_max, c.secondary_normal_eps, c.secondary_far)
        flat = torch.zeros(rc.density_grad_layout(L2)[1], device="cuda")
        anneal = train.anneal_at(1.0)
        res = {"rays": n}
        grad = bc.time_whole_call(lambda: rc.mask_backward(rays, jit, anneal, masks, None, terms["mask"], grads=flat),
                                  a.warmup, a.reps, [flat])
        res.update(mask_grads_ms=grad["ms_per_call"], workspace_GB=grad["workspace_GB"], grad_MB=grad["grad_MB"])
        res.update(bc.time_calls({
            "mask_loss_only": lambda: rc.mask_backward(rays, jit, anneal, masks, None, terms["mask"], grads=False),
            "mask_backwards_grads": lambda: rc.mask_backward(back, jit, anneal, None, None, terms["mask_backwards"], grads=flat),
            "mask_backwards_loss_only": lambda: rc.mask_backward(back, jit, anneal, None, None, terms["mask_backwards"], grads=False),
            "backward_mask_rays": lambda: rc.backward_mask_rays(rays["origins"], look, u1, u2, c.shadow_near_max,
                                                                c.secondary_normal_eps, c.secondary_far),
        }, a.warmup, a.reps))
        if not a.no_geometry:
            flats = [flat, torch.zeros(rc.shader_grad_layout()[1], device="cuda")]
            gterms = train.geometry_terms(1.0)
            g = bc.time_whole_call(lambda: rc.geometry_backward(rays, jit, anneal, None, gterms, grads=flats), a.warmup, a.reps, flats)
            res["geometry_grads_ms"] = g["ms_per_call"]
            res["mask_over_geometry"] = round(res["mask_grads_ms"] / g["ms_per_call"], 3)
            del flats
        bc.emit(res)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(res) + "\n")
        rc.close()
        del flat
        torch.cuda.empty_cache()


def _calls(stats_path):
    """(kernel name, launches) of a rocprofv3 kernel_stats.csv."""
    import csv
    with open(stats_path) as f:
        return [(r["Name"], r["Calls"]) for r in csv.DictReader(f)]


if __name__ == "__main__":
    main()
