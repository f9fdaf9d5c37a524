"""Times rc_data_backward (charb data loss + gradients of MLP_2 and the shader side) per call.

  python tools/bench_data_backward.py [--rays 8192 65536] [--warmup 3] [--reps 10]
      whole-call ms on the caller's stream (device events, steady state after the warm-up calls), and the device memory
      the call's workspaces took on first use;
  python tools/bench_data_backward.py --stats <kernel_stats.csv> --rays 8192
      the split of one rocprofv3 --kernel-trace --stats run of this tool into the training forward, k_data_loss_bwd, the
      shader backward (k_gemm and its elementwise kernels), the level-2 density backward and the grid scatters, and the
      shader GEMMs' FLOP over k_gemm's kernel time against the fp32-MFMA peak.
Prints one JSON line per measurement."""
import argparse
import json

import bench_common as bc

FP32_MFMA_PEAK_TFS = 155.0     # measured v_mfma_f32_32x32x2_f32 peak of the MI355X
# dense layers of the shader side (in, out): pred_normals, bottleneck, 4 heads, integrated BRDF, SLF
LAYERS = [(64, 3), (96, 128), (96, 1), (96, 3), (96, 3), (96, 3), (129, 64), (64, 64), (64, 1), (200, 128), (128, 128),
          (128, 128), (328, 128), (128, 3)]
GROUPS = {"forward": ("k_sample", "k_level", "k_hashgrid", "k_density_mlp", "k_cache_shader", "k_composite"),
          "k_data_loss_bwd": ("k_data_loss_bwd",), "reduce+copy": ("k_interlevel_reduce", "k_points_aos"),
          "k_gemm": ("k_gemm",),
          "shader_elementwise": ("k_sum_parts", "k_stage_feature", "k_shader_glue_fwd", "k_shader_out_bwd",
                                 "k_shader_glue_bwd", "k_split_feature"),
          "density_backward": ("k_density_bwd", "k_wgrad", "k_grad_reduce"), "grid_scatter": ("k_grid_scatter",)}


def shader_flop_per_sample():
    """Recompute + input gradients + weight gradients: 3 x 2 sum(in * out)."""
    return 3 * 2 * sum(i * o for i, o in LAYERS)


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
        flop = shader_flop_per_sample() * n * S2
        t = ms["k_gemm"] * 1e-3
        tfs = flop / t / 1e12 if t > 0 else 0.0
        floor_ms = flop / (FP32_MFMA_PEAK_TFS * 1e12) * 1e3
        print(json.dumps({"rays": n, "ms_per_call": {k: round(v, 4) for k, v in ms.items()}, "shader_GFLOP": round(flop / 1e9, 1),
                          "shader_floor_ms": round(floor_ms, 3), "k_gemm_TFLOPs": round(tfs, 1),
                          "k_gemm_frac_of_fp32_mfma_peak": round(tfs / FP32_MFMA_PEAK_TFS, 3)}))
        return
    import torch
    import common
    import loss_cases as lc
    from nrc_amd import train
    for n in a.rays:
        rc = common.make_rc()
        rays, jit = bc.to_device(lc.cache_case(n, seed=3))
        gt = torch.rand(n, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
        flats = [torch.zeros(rc.density_grad_layout(cfg.num_levels - 1)[1], device="cuda"),
                 torch.zeros(rc.shader_grad_layout()[1], device="cuda")]
        call = lambda: rc.data_backward(rays, gt, jit, train.anneal_at(1.0), grads=flats)
        bc.emit({"rays": n, **bc.time_whole_call(call, a.warmup, a.reps, flats)})
        rc.close()
        del flats
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
