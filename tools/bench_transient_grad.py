"""rc_transient_data_backward against rc_render_transient on the same batches: ms per call by device
events after warm-up, distinct batches cycled; with --stats <rocprofv3 kernel_stats.csv> the backward's kernel time per
call against its FLOP floor at the fp32 MFMA peak.  One JSON line per ray count.  --loss picks the loss reading: a preset
of config.transient_data_loss_preset ("cornell": the default type through rc_transient_data_backward; "cornell_itof",
"steady_state", "mse", ...: rc_transient_data_backward_kind and k_transient_loss_kinds).

  python tools/bench_transient_grad.py --rays 1024
  python tools/bench_transient_grad.py --rays 1024 --loss cornell_itof
  rocprofv3 --kernel-trace --stats -d out -- python tools/bench_transient_grad.py --rays 1024 --profile-calls 8
  python tools/bench_transient_grad.py --rays 1024 --stats out/.../kernel_stats.csv --calls 8
"""
import argparse

import bench_common as bc

OWN = ("k_transient_loss_kinds", "k_transient_loss", "k_transient_bins_bwd", "k_gemm_tile", "k_sum_parts", "k_interlevel_reduce")
PEAK_F32_MFMA = 157e12                 # MI355X fp32 matrix peak


def flop_floor(n):
    """The recompute X W and the two products dW = X^T dZ, dX = dZ W^T of both heads: 3 x 2 x (64 x 2100 + 128 x 2101) per sample."""
    return 3 * 2 * (64 * 2100 + 128 * 2101) * n * 32


def main():
    ap = argparse.ArgumentParser()
    bc.add_rays(ap, [1024])
    bc.add_loop(ap, 3, 10)
    bc.add_stats(ap, per_call=True)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--loss", default="cornell", help="preset of config.transient_data_loss_preset (default: cornell)")
    ap.add_argument("--profile-calls", type=int, default=0, help="run this many backward calls and nothing else (under rocprofv3)")
    a = ap.parse_args()
    if a.stats:
        for n in a.rays:
            res = bc.own_report(a.stats, OWN, n, a.calls)
            if a.calls:
                bwd = sum(v for k, v in res["own_ms_per_grad_call"].items() if k not in ("k_transient_loss", "k_transient_loss_kinds", "k_interlevel_reduce"))
                floor_ms = flop_floor(n) / PEAK_F32_MFMA * 1e3
                res.update(flop_floor_ms=round(floor_ms, 4), backward_kernels_ms=round(bwd, 4), times_floor=round(bwd / floor_ms, 1))
            bc.emit(res)
        return
    import numpy as np
    import torch

    import common
    import nrc_amd
    from nrc_amd import config, rc_ext

    # the default reading without a name, so that a build from before the presets runs it too
    loss_cfg = None if a.loss == "cornell" else config.transient_data_loss_preset(a.loss)
    rc = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    rc.load_weights(common.weights_transient_np())
    for n in a.rays:
        batches = []
        for i in range(a.batches):
            rays = bc.to_device(nrc_amd.synthetic_transient_rays(n, seed=100 + i).hot_fields())
            jit = bc.to_device([j.reshape(-1) for j in common.jitters(n, seed=200 + i)])
            rgb = rc.render_transient(rays, {"jitter": jit}, outputs=["rgb"])["rgb"]
            gt = (rgb * torch.empty_like(rgb).uniform_(0.5, 1.5)).contiguous()
            batches.append((rays, {"jitter": jit}, gt))
        flat = torch.zeros(rc.transient_head_grad_layout()[1], device="cuda")
        state = {"i": 0}

        def nxt():
            state["i"] += 1
            return batches[state["i"] % len(batches)]

        def backward():
            rays, rnd, gt = nxt()
            rc.transient_data_backward(rays, rnd, gt, cfg=loss_cfg, grad=flat)

        def no_grads():
            rays, rnd, gt = nxt()
            rc.transient_data_backward(rays, rnd, gt, cfg=loss_cfg, grad=False)

        def render():
            rays, rnd, _ = nxt()
            rc.render_transient(rays, rnd, outputs=["rgb"])

        if a.profile_calls:
            for _ in range(a.profile_calls):
                backward()
            torch.cuda.synchronize()
            continue
        res = {"rays": n, "loss": a.loss, **bc.time_calls({"backward": backward, "adjoints_only": no_grads, "render_transient": render},
                                          a.warmup, a.reps, a.only)}
        if "backward_ms" in res and "render_transient_ms" in res:
            res["backward_over_render"] = round(res["backward_ms"] / res["render_transient_ms"], 2)
        res["flop_floor_ms"] = round(flop_floor(n) / PEAK_F32_MFMA * 1e3, 4)
        bc.emit(res)


if __name__ == "__main__":
    main()
