"""rc_eval_albedo and rc_albedo_ratio: ms per call by device events (the median of --reps calls after
--warmup, inputs resident on the device, the result left there), next to the reference's way on the same box: the same
arrays copied to the host and the numpy code of tests/albedo_metrics_ref.py, by wall clock.  One JSON line per case.

  python tools/bench_albedo.py                      # an 800 x 800 view; the ratio over 20 appended views
  python tools/bench_albedo.py --views 4 --no-host
"""
import argparse
import time

import bench_common as bc


def inputs(h, w, seed):
    """A view with about 70 % valid pixels: albedo, acc, ground truth, mask on the device."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = lambda *s: torch.rand(*s, device="cuda", generator=g)
    albedo = 0.05 + 0.85 * u(h, w, 3)
    acc = (0.3 + 0.7 * u(h, w)).clamp(max=1.0)
    gt = ((albedo + (1.0 - acc)[..., None]) * (0.5 + u(h, w, 3))).clamp(0.0, 1.0)
    mask = (u(h, w) > 0.1).float()
    return albedo, acc, gt, mask


def wall_ms(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    return round(times[len(times) // 2], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[800, 800])
    ap.add_argument("--views", type=int, default=20, help="views appended to the pair buffer of the ratio")
    bc.add_loop(ap, 3, 10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="leave out the copy to the host and the numpy code")
    a = ap.parse_args()
    import numpy as np
    import torch

    import albedo_metrics_ref as ref
    import nrc_amd
    from nrc_amd import rc_ext

    rc = rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)
    h, w = a.size
    view = inputs(h, w, 1)
    albedo, acc, gt, mask = view
    ratio = torch.tensor([0.9, 1.0, 1.1], device="cuda")
    one = rc_ext.AlbedoPairs(rc, h * w)

    def append():
        one.count.zero_()
        rc.eval_albedo(albedo, acc, gt, mask=mask, pairs=one, sync=False)

    res = {"case": "view", "height": h, "width": w, "device": torch.cuda.get_device_name(0)}
    res.update(bc.time_calls({"eval_albedo": lambda: rc.eval_albedo(albedo, acc, gt, mask=mask, sync=False),
                              "eval_albedo_ratio_given": lambda: rc.eval_albedo(albedo, acc, gt, mask=mask, ratio=ratio, sync=False),
                              "eval_albedo_appending": append}, a.warmup, a.reps))
    res["valid"] = rc.eval_albedo(albedo, acc, gt, mask=mask)["valid"]
    if not a.no_host:
        host = lambda: [t.cpu().numpy() for t in view]
        res["host_copy_ms"] = wall_ms(host, a.host_reps)
        arrays = host()
        res["host_numpy_ms"] = wall_ms(lambda: ref.evaluate(*arrays[:3], mask=arrays[3], dtype=np.float32), a.host_reps)
    bc.emit(res)

    pairs = rc_ext.AlbedoPairs(rc, a.views * h * w)
    for v in range(a.views):
        x = inputs(h, w, 10 + v)
        rc.eval_albedo(*x[:3], mask=x[3], pairs=pairs, sync=False)
    res = {"case": "ratio", "views": a.views, "capacity": pairs.capacity, "rows": int(pairs.count.item())}
    res.update(bc.time_calls({"ratio_median": lambda: rc.albedo_ratio(pairs, use_median=True),
                              "ratio_lstsq_gamma": lambda: rc.albedo_ratio(pairs, use_median=False, gamma=True),
                              "ratio_lstsq": lambda: rc.albedo_ratio(pairs, use_median=False, gamma=False)}, a.warmup, a.reps))
    if not a.no_host:
        res["host_copy_ms"] = wall_ms(lambda: pairs.rows(), 1)
        rows, _ = pairs.rows()
        g, p = [rows[:, :3]], [rows[:, 3:]]
        res["host_median_ms"] = wall_ms(lambda: ref.ratio(g, p, True, dtype=np.float32), 1)
        res["host_lstsq_gamma_ms"] = wall_ms(lambda: ref.ratio(g, p, False, True, dtype=np.float32), 1)
    bc.emit(res)


if __name__ == "__main__":
    main()
