"""rc_eval_image: ms per call by device events (the median of --reps calls after --warmup, inputs
resident on the device, the result array left there), the bytes each kernel must move against the 8 TB/s HBM peak, and
for the 800 x 800 image the ratio to render_camera's device time for the same image in the same session.  With --stats
<rocprofv3 kernel_stats.csv> and --calls: the kernels' own times per call and their fraction of the peak.  One JSON line
per case.

  python tools/bench_eval.py
  rocprofv3 --kernel-trace --stats -d out -- python tools/bench_eval.py --case transient --profile-calls 8
  python tools/bench_eval.py --case transient --stats out/.../kernel_stats.csv --calls 8
"""
import argparse

import bench_common as bc

OWN = ("k_eval_bins", "k_eval_pixels", "k_eval_ssim", "k_eval_finish")
HBM_PEAK = 8e12                        # bytes / s, the peak DESIGN.md quotes
# case -> (height, width, n_bins, every optional input given)
CASES = {"image": (800, 800, 0, False), "image_all": (800, 800, 0, True), "transient": (256, 256, 700, True)}


def kernel_bytes(h, w, nb, optional):
    """Bytes each kernel must move once: its inputs read, its outputs written (partial sums left out)."""
    n = h * w
    out = {}
    if nb:
        out["k_eval_bins"] = 2 * n * nb * 3 * 4 + 2 * n * 3 * 4                 # both histograms in, both bin sums out
    px = 2 * n * 3 * 4 + 2 * n * 3 * 4                                          # two images in, two post-processed out
    if optional:
        px += n * 4 * (1 + 1 + 3) + 2 * n * 3 * 4                               # mask, acc, three depths; two normal images
    out["k_eval_pixels"] = px
    out["k_eval_ssim"] = 2 * n * 3 * 4                                          # the two post-processed images in
    return out


def inputs(h, w, nb, optional):
    import torch
    g = torch.Generator(device="cuda").manual_seed(h * 31 + nb)
    u = lambda *s: torch.rand(*s, device="cuda", generator=g)
    shape = (h, w, nb, 3) if nb else (h, w, 3)
    pred = u(*shape) * (3.0 / nb if nb else 1.0)
    gt = (pred * (0.5 + u(*shape))).contiguous()
    kw = {}
    if optional:
        kw = dict(mask=(u(h, w) > 0.2).float(), acc=u(h, w), normals=u(h, w, 3) - 0.5, normals_gt=u(h, w, 3) - 0.5,
                  distance_mean=2.0 + 4.0 * u(h, w), distance_median=2.0 + 4.0 * u(h, w), depth_gt=2.0 + 4.0 * u(h, w))
    if nb:
        kw["img_scale"] = 3.0
    return pred, gt, kw


def render_ms(h, w, warmup, reps):
    """render_camera's device time for an h x w image of the synthetic cache (outputs left on the device)."""
    import numpy as np

    import common
    import nrc_amd
    from nrc_amd import model as M

    m = M.Model(nrc_amd.hotdog_config(), 0)
    m.load_variables(common.weights_np())
    o = np.array([0.0, -3.5, 2.0])
    look = -o / np.linalg.norm(o)
    right = np.cross(look, [0, 0, 1.0]); right /= np.linalg.norm(right)
    up = np.cross(right, look)
    cam = nrc_amd.Camera(nrc_amd.get_pixtocam(1111.0, w, h), np.concatenate([np.stack([right, up, -look], 1), o[:, None]], 1),
                         near=2.0, far=6.0)
    return bc.time_calls({"render_camera": lambda: nrc_amd.render_camera(m, cam, h, w, to_host=False)}, warmup, reps)["render_camera_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", nargs="+", default=["image", "transient"], choices=list(CASES))
    bc.add_loop(ap, 3, 10)
    bc.add_stats(ap, per_call=True)
    ap.add_argument("--profile-calls", type=int, default=0, help="run this many calls of each case and nothing else (under rocprofv3)")
    ap.add_argument("--no-render", action="store_true", help="leave out render_camera's time")
    a = ap.parse_args()
    if a.stats:
        for case in a.case:
            h, w, nb, optional = CASES[case]
            res = {"case": case, **bc.own_report(a.stats, OWN, h * w, a.calls)}
            if a.calls:
                res["fraction_of_hbm_peak"] = {k: round(b / (res["own_ms_per_grad_call"][k] * 1e-3) / HBM_PEAK, 3)
                                               for k, b in kernel_bytes(h, w, nb, optional).items() if res["own_ms_per_grad_call"].get(k)}
            bc.emit(res)
        return
    import torch

    import nrc_amd
    from nrc_amd import rc_ext

    rc = rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)
    for case in a.case:
        h, w, nb, optional = CASES[case]
        pred, gt, kw = inputs(h, w, nb, optional)
        call = lambda: rc.eval_image(pred, gt, sync=False, **kw)
        if a.profile_calls:
            for _ in range(a.profile_calls):
                call()
            torch.cuda.synchronize()
            continue
        ms = bc.time_calls({"eval_image": call}, a.warmup, a.reps)["eval_image_ms"]
        nbytes = kernel_bytes(h, w, nb, optional)
        res = {"case": case, "height": h, "width": w, "n_bins": nb, "optional_inputs": optional, "eval_image_ms": ms,
               "bytes_floor": nbytes, "floor_ms_at_peak": round(sum(nbytes.values()) / HBM_PEAK * 1e3, 4),
               "fraction_of_hbm_peak": round(sum(nbytes.values()) / (ms * 1e-3) / HBM_PEAK, 3)}
        if not nb and not a.no_render:
            res["render_camera_ms"] = render_ms(h, w, a.warmup, a.reps)
            res["eval_over_render"] = round(ms / res["render_camera_ms"], 4)
        bc.emit(res)


if __name__ == "__main__":
    main()
