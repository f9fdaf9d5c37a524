"""Time slices of the time-resolved cache without the histograms: ms per call by device events of
  (a) render_transient(outputs=["rgb"])             the full [n, 700, 3] histogram,
  (b) render_transient_slices with one time,
  (c) render_transient_slices with eight times,
on the same handle and the same --rays synthetic transient rays with jitter (inputs and outputs resident on the device),
the three interleaved over --rounds rounds (each the median of --reps calls after --warmup) so that a drift of the
machine hits all of them; and the bytes of the outputs for a 512 x 512 frame.  With --profile-calls the three calls are
run that many times each and nothing else (under rocprofv3), with --stats <kernel_stats.csv or results .db> --calls the
kernels' own times per launch come out of that run (the slice kernel averaged over its one-time and eight-time launches:
the trace itself tells them apart, in launch order).  One JSON line.

  python tools/bench_transient_slice.py
  rocprofv3 --kernel-trace --stats -d out -- python tools/bench_transient_slice.py --profile-calls 20
  python tools/bench_transient_slice.py --stats out/.../kernel_stats.csv --calls 20
"""
import argparse

import bench_common as bc

OWN = ("k_transient_slice", "k_transient_bins", "k_transient_shader")
ONE, EIGHT = (167.25,), (0.0, 36.5, 167.0, 167.25, 300.5, 400.75, 686.5, 699.0)
N_BINS = 700


def main():
    ap = argparse.ArgumentParser()
    bc.add_rays(ap, [1024])
    bc.add_loop(ap, 5, 30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--calls", type=int, default=0, help="--stats: calls of EACH of the three in the profiled run")
    ap.add_argument("--profile-calls", type=int, default=0, help="run each call this many times and nothing else (under rocprofv3)")
    a = ap.parse_args()
    if a.stats:
        for n in a.rays:
            mine, other = bc.split_own(a.stats, OWN)
            res = {"rays": n, "kernel_ms_per_run": {k: round(v, 4) for k, v in mine.items()},
                   "other_kernels_ms_per_run": round(sum(other.values()), 4)}
            if a.calls:
                # the shader runs in all three calls, the bins kernel in one, the slice kernel in two (1 time, 8 times)
                per = {"k_transient_shader": 3 * a.calls, "k_transient_bins": a.calls, "k_transient_slice": 2 * a.calls}
                res["kernel_ms_per_launch"] = {k: round(v / per[k], 4) for k, v in mine.items()}
            bc.emit(res)
        return
    import torch

    import common
    import nrc_amd
    from nrc_amd import rc_ext

    rc = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    rc.load_weights(common.weights_transient_np())
    for n in a.rays:
        fields = bc.to_device({k: v for k, v in nrc_amd.synthetic_transient_rays(n).hot_fields().items()
                               if v is not None and k != "lossmult"})
        rnd = {"jitter": bc.to_device([j.reshape(-1) for j in common.jitters(n, seed=3)])}
        calls = {"full_rgb": lambda: rc.render_transient(fields, rnd, outputs=["rgb"]),
                 "slice_1": lambda: rc.render_transient_slices(fields, rnd, ONE),
                 "slice_8": lambda: rc.render_transient_slices(fields, rnd, EIGHT)}
        if a.profile_calls:
            for fn in calls.values():
                for _ in range(a.profile_calls):
                    fn()
            torch.cuda.synchronize()
            continue
        rounds = [bc.time_calls(calls, a.warmup, a.reps) for _ in range(a.rounds)]
        res = {"rays": n, "device": torch.cuda.get_device_name(0), "mlp_arithmetic": rc_ext.mlp_arithmetic()}
        for k in rounds[0]:
            vals = sorted(r[k] for r in rounds)
            res[k] = vals[len(vals) // 2]
            res[k.replace("_ms", "_ms_rounds")] = [r[k] for r in rounds]
        res["slice_1_over_full"] = round(res["slice_1_ms"] / res["full_rgb_ms"], 4)
        res["slice_8_over_full"] = round(res["slice_8_ms"] / res["full_rgb_ms"], 4)
        # the slices against the histograms they are taken from, and what a frame costs in output bytes
        full = rc.render_transient(fields, rnd, outputs=["rgb"])["rgb"]
        got = rc.render_transient_slices(fields, rnd, EIGHT)["rgb"]
        lo = torch.tensor([int(t) for t in EIGHT], device=full.device)
        hi = torch.tensor([int(-(-t // 1)) for t in EIGHT], device=full.device)
        w = torch.tensor([t - int(t) for t in EIGHT], device=full.device, dtype=torch.float64)[None, :, None]
        exp = w * full[:, hi].double() + (1.0 - w) * full[:, lo].double()
        res["max_abs_slice_minus_full"] = float((got.double() - exp).abs().max())
        px = 512 * 512
        res["frame_512x512_bytes"] = {"full_rgb": px * N_BINS * 3 * 4, "slice_1": px * 3 * 4, "slice_8": px * 8 * 3 * 4}
        bc.emit(res)


if __name__ == "__main__":
    main()
