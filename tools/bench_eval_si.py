"""rc_eval_shift_invariant: ms per call by device events (the median of --reps calls after --warmup,
inputs resident on the device, the result array left there), its workspace, and in the same session rc_eval_image with
skip_postprocess on the same images -- (2 ri + 1)(2 rj + 1) of those is the least a caller pays who shifts the image and
calls the existing entry once per shift, and the bar for this call -- and render_camera of the same image size.  With
--stats <rocprofv3 kernel_stats.csv> and --calls: the kernels' own times per call.  One JSON line per case.

  python tools/bench_eval_si.py
  rocprofv3 --kernel-trace --stats -d out -- python tools/bench_eval_si.py --profile-calls 8
  python tools/bench_eval_si.py --stats out/.../kernel_stats.csv --calls 8
"""
import argparse

import bench_common as bc
from bench_eval import render_ms

# the two instantiations of the templated kernels apart where the profiler's names carry the argument (0: mse, 1: ssim)
OWN = ("k_si_metric<0>", "k_si_metric<1>", "k_si_select<0>", "k_si_select<1>", "k_si_metric", "k_si_select", "k_si_finish")


def workspace_bytes(rc):
    return {k: int(rc.workspace("ev:" + k).nbytes) for k in ("si_metric", "si_state", "si_part")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[800, 800])
    ap.add_argument("--radii", type=int, nargs=2, default=[4, 4])
    ap.add_argument("--halfwidth", type=int, default=8)
    bc.add_loop(ap, 3, 10)
    bc.add_stats(ap, per_call=True)
    ap.add_argument("--profile-calls", type=int, default=0, help="run this many calls and nothing else (under rocprofv3)")
    ap.add_argument("--no-render", action="store_true", help="leave out render_camera's time")
    ap.add_argument("--tag", default=None, help="a name for the line, e.g. of the build under RC_HIP_LIBRARY in an A/B")
    a = ap.parse_args()
    h, w = a.size
    if a.stats:
        bc.emit({"case": "si", **bc.own_report(a.stats, OWN, h * w, a.calls)})
        return
    import torch

    import nrc_amd
    from nrc_amd import rc_ext

    rc = rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)
    g = torch.Generator(device="cuda").manual_seed(h * 31 + w)
    gt = torch.rand(h, w, 3, device="cuda", generator=g)
    pred = (torch.roll(gt, (1, -2), (0, 1)) + 0.02 * torch.randn(h, w, 3, device="cuda", generator=g)).contiguous()
    radii = tuple(a.radii)
    call = lambda: rc.eval_shift_invariant(pred, gt, radii, a.halfwidth, sync=False)
    if a.profile_calls:
        for _ in range(a.profile_calls):
            call()
        torch.cuda.synchronize()
        return
    shifts = (2 * radii[0] + 1) * (2 * radii[1] + 1)
    res = {"case": "si", **({"tag": a.tag} if a.tag else {}), "height": h, "width": w, "search_radii": list(radii), "window_halfwidth": a.halfwidth, "shifts": shifts}
    res.update(bc.time_calls({"eval_shift_invariant": call,
                              "eval_shift_invariant_mse_only": lambda: rc.eval_shift_invariant(pred, gt, radii, a.halfwidth, ssim=False, sync=False),
                              "eval_image_skip_postprocess": lambda: rc.eval_image(pred, gt, skip_postprocess=True, sync=False)},
                             a.warmup, a.reps))
    res["bar_ms"] = round(shifts * res["eval_image_skip_postprocess_ms"], 4)
    res["call_over_bar"] = round(res["eval_shift_invariant_ms"] / res["bar_ms"], 4)
    res["workspace_bytes"] = workspace_bytes(rc)
    if not a.no_render:
        res["render_camera_ms"] = render_ms(h, w, a.warmup, a.reps)
        res["call_over_render"] = round(res["eval_shift_invariant_ms"] / res["render_camera_ms"], 4)
    bc.emit(res)


if __name__ == "__main__":
    main()
