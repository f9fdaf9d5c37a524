"""Times rc_material_data_backward_env: the call with the EnvMap gradient, the same call without it
(rc_material_data_backward's work) and rc_render_material at the same size, per call.

  python tools/bench_envmap_grad.py [--rays 8192 32768] [--K 8] [--warmup 3] [--reps 10]
      ms per call on the caller's stream (device events, the median of the repetitions after the warm-up calls);
      --rays 1024 --K 32 is the material step of bench.py;
  python tools/bench_envmap_grad.py --only with_envmap --rays 8192      (the run to profile: the EnvMap call only)
  python tools/bench_envmap_grad.py --stats <kernel_stats.csv> --rays 8192 --calls 13
      the split of one rocprofv3 --kernel-trace --stats run of this tool (one --rays value) by kernel: what the EnvMap
      gradient adds (k_material_data_env_bwd, k_envmap_stage, k_gemm_tile, k_envmap_out_bwd, k_sum_parts) beside
      k_envmap's own forward on the same rows, and the rest; with --calls (warm-up + repetitions of the profiled run) per
      call, and the added time as a multiple of k_envmap's.
  tools/micro/gemm_tile_ab (built from gemm_tile_ab.hip) is the GEMM A/B of the same section.
Prints one JSON line per measurement."""
import argparse

import bench_common as bc

OWN = ("k_material_data_env_bwd", "k_envmap_stage", "k_gemm_tile", "k_envmap_out_bwd", "k_sum_parts", "k_envmap")
ADDED = OWN[:-1]


def main():
    ap = argparse.ArgumentParser()
    bc.add_rays(ap, [8192, 32768])
    bc.add_loop(ap, 3, 10)
    ap.add_argument("--K", type=int, default=8, help="num_secondary_samples")
    bc.add_stats(ap, per_call=True)
    a = ap.parse_args()
    if a.stats:
        res = bc.own_report(a.stats, OWN, a.rays[0], a.calls)
        mine = res["kernel_ms_per_run_own"]
        added = sum(v for k, v in mine.items() if k in ADDED)
        res["added_ms_per_run"] = round(added, 4)
        if mine.get("k_envmap"):
            res["added_over_k_envmap"] = round(added / mine["k_envmap"], 3)
        bc.emit(res)
        return
    import torch
    import loss_cases as lc
    for n in a.rays:
        rc = lc.make_material_rc()
        K = a.K
        rays, rnd = bc.to_device(lc.material_case(n, K, seed=3))
        gt = bc.to_device(lc.uniform_gt(n, 5))
        grad = torch.zeros(rc.material_grad_layout()[1], device="cuda")
        env = torch.zeros(rc.envmap_grad_layout()[1], device="cuda")
        calls = {
            "with_envmap": lambda: rc.material_data_backward(rays, rnd, gt, K, grad=grad, env_grad=env),
            "without_envmap": lambda: rc.material_data_backward(rays, rnd, gt, K, grad=grad),
            "forward_render_material": lambda: rc.render_material(rays, rnd, num_secondary_samples=K),
        }
        bc.emit({"rays": n, "K": K, "rows": n * K, **bc.time_calls(calls, a.warmup, a.reps, a.only)})
        rc.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
