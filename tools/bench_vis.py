"""The visualisation suite on the device: ms per suite by device events (the median of --reps calls after
--warmup, the rendering resident on the device, the uint8 pictures left there), its three calls on their own, the bytes each
kernel must move against the 8 TB/s HBM peak, the render of the same view in the same session, and the host way on the
same box: the same arrays copied to the host and the float32 numpy code of tests/vis_ref.py, by wall clock.  With --stats
<rocprofv3 kernel_stats.csv> and --calls: the kernels' own times per suite and their fraction of the peak.  One JSON line
per case.

  python tools/bench_vis.py                          # an 800 x 800 cache-pass view with a mask; a 256 x 256 x 700 transient view
  rocprofv3 --kernel-trace --stats -d out -- python tools/bench_vis.py --case cache --profile-calls 8
  python tools/bench_vis.py --case cache --stats out/.../kernel_stats.csv --calls 8
"""
import argparse
import os
import time

import bench_common as bc

OWN = ("k_vis_select_hist", "k_vis_select_narrow", "k_vis_select_neighbours", "k_vis_select_begin", "k_vis_select_finish",
       "k_vis_max_finish", "k_vis_max", "k_vis_bins", "k_vis_items")
HBM_PEAK = 8e12                        # bytes / s, the peak DESIGN.md quotes
CASES = {"cache": (800, 800, 0), "transient": (256, 256, 700)}     # case -> (height, width, n_bins)
COLOURS = ("diffuse_rgb", "specular_rgb", "direct_rgb", "indirect_rgb", "albedo_rgb", "indirect_diffuse_rgb",
           "indirect_specular_rgb", "direct_diffuse_rgb", "direct_specular_rgb", "ambient_rgb", "ambient_diffuse_rgb",
           "ambient_specular_rgb", "irradiance_rgb", "light_radiance_rgb", "n_dot_l_rgb")


def rendering(h, w, nb):
    """The keys Model.apply hands the suites for a cache-pass view (with their cache_ aliases), random, on the device; a
    few NaN depths and some empty pixels."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(h * 31 + nb)
    u = lambda *s: torch.rand(*s, device="cuda", generator=g)
    r = {"acc": (1.4 * u(h, w)).clamp(max=1.0), "distance_mean": 2.0 + 4.0 * u(h, w), "distance_median": 2.0 + 4.0 * u(h, w),
         "normals": 2.0 * u(h, w, 3) - 1.0, "normals_pred": 2.0 * u(h, w, 3) - 1.0, "indirect_occ": u(h, w, 3),
         "lossmult": torch.ones((h, w, 3), device="cuda"), "vignette": torch.ones((h, w, 1), device="cuda")}
    r["distance_mean"][::97, ::89] = float("nan")
    r["rgb"] = u(h, w, nb, 3) * (3.0 / nb) if nb else 1.2 * u(h, w, 3)
    for k in COLOURS:
        r[k] = 1.2 * u(h, w, 3)
    if nb:
        r["direct_rgb_viz"] = u(h, w, 3)
    for k in ("rgb", "normals", "normals_pred", "indirect_occ") + COLOURS:
        r["cache_" + k] = r[k]
    r["normals_to_use"] = r["normals_pred"]
    return r, (u(h, w) > 0.2).float()


def kernel_bytes(rc, r, mask, nb, suite, cfg):
    """Bytes each kernel must move once per suite, from the item table the suite builds: inputs read, outputs written
    (partial sums and the select's state left out)."""
    seen = {}
    real = (rc.vis_images, rc.weighted_percentile, rc.image_max)
    rc.vis_images = lambda items, h, w, **kw: seen.setdefault("items", items) and [{"u8": None} for _ in items]
    rc.weighted_percentile = lambda v, wt=None, ps=(), **kw: seen.setdefault("pct", []).append(v.numel()) or v.new_zeros(2, dtype=v.dtype).double()
    rc.image_max = lambda s, **kw: seen.setdefault("max", []).append(s.numel()) or s.new_zeros(1)
    try:
        suite(r, cfg, masks=mask, rc=rc)
    finally:
        rc.vis_images, rc.weighted_percentile, rc.image_max = real
    n = mask.numel()
    out = {"k_vis_items": 0, "k_vis_bins": 0}
    sums = set()
    for it in seen["items"]:
        per = n * int(it["channels"]) * 4
        if it.get("n_bins"):
            if it["src"].data_ptr() not in sums:
                sums.add(it["src"].data_ptr())
                out["k_vis_bins"] += per * int(it["n_bins"]) + per
        out["k_vis_items"] += per + n * 3 + n * 4 * sum(it.get(k) is not None for k in ("acc", "mask"))
    out["k_vis_select_hist"] = sum(4 * 2 * 4 * m for m in seen.get("pct", []))                # four passes over value and weight
    out["k_vis_select_neighbours"] = sum(4 * m for m in seen.get("pct", []))
    out["k_vis_max"] = sum(4 * m for m in seen.get("max", []))
    counts = {"items": len(seen["items"]), "percentile_calls": len(seen.get("pct", [])), "max_calls": len(seen.get("max", []))}
    return {k: v for k, v in out.items() if v}, counts


def transient_render_ms(h, w, warmup, reps):
    """rc_render_transient's device time for h w synthetic rays in chunks of 8192, every key the suite reads."""
    import common
    import nrc_amd
    from nrc_amd import metrics
    from nrc_amd import model as M

    m = M.Model(nrc_amd.cornell_transient_config(), 0)
    m.load_variables(common.weights_transient_np())
    fields = bc.to_device({k: v for k, v in nrc_amd.synthetic_transient_rays(h * w).hot_fields().items() if v is not None and k != "lossmult"})
    names = list(metrics._TRANSIENT_VIS_KEYS)

    def render():
        for i in range(0, h * w, 8192):
            m.rc.render_transient({k: v[i: i + 8192] for k, v in fields.items()}, None, outputs=names)
    return bc.time_calls({"render_transient": render}, warmup, reps)["render_transient_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", nargs="+", default=list(CASES), choices=list(CASES))
    bc.add_loop(ap, 3, 10)
    bc.add_stats(ap, per_call=True)
    ap.add_argument("--profile-calls", type=int, default=0, help="run this many suites of each case and nothing else (under rocprofv3)")
    ap.add_argument("--no-render", action="store_true", help="leave out the render of the same view")
    ap.add_argument("--no-host", action="store_true", help="leave out the copy to the host and the numpy code")
    ap.add_argument("--out", default=os.path.join(bc.ROOT, "profiles", "vis_bench.jsonl"), help="the lines are appended here too")
    a = ap.parse_args()
    import numpy as np
    import torch

    import nrc_amd
    import vis_ref as ref
    from nrc_amd import rc_ext, vis

    def emit(res):
        bc.emit(res)
        if a.out:
            with open(a.out, "a") as f:
                f.write(bc.json.dumps(res) + "\n")

    rc = rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)
    cfg = argparse.Namespace(img_scale=1.5, var_scale=1.0)
    for case in a.case:
        h, w, nb = CASES[case]
        r, mask = rendering(h, w, nb)
        suite = vis.visualize_transient_suite if nb else vis.visualize_suite
        nbytes, counts = kernel_bytes(rc, r, mask, nb, suite, cfg)
        if a.stats:
            res = {"case": case, **counts, **bc.own_report(a.stats, OWN, h * w, a.calls)}
            if a.calls:
                res["fraction_of_hbm_peak"] = {k: round(b / (res["own_ms_per_grad_call"][k] * 1e-3) / HBM_PEAK, 3)
                                               for k, b in nbytes.items() if res["own_ms_per_grad_call"].get(k)}
            emit(res)
            continue
        call = lambda: suite(r, cfg, masks=mask, rc=rc)
        if a.profile_calls:
            for _ in range(a.profile_calls):
                call()
            torch.cuda.synchronize()
            continue
        pictures = call()
        acc = vis._acc_for_depth(r)
        items = [dict(src=r["cache_albedo_rgb"], op="srgb", channels=3, u8=True)]
        res = {"case": case, "height": h, "width": w, "n_bins": nb, "pictures": len(pictures), **counts,
               "device": torch.cuda.get_device_name(0)}
        res.update(bc.time_calls({"suite": call,
                                  "weighted_percentile": lambda: rc.weighted_percentile(r["distance_median"], acc, [0.5, 99.5]),
                                  "image_max": lambda: rc.image_max(r["cache_rgb"]),
                                  "vis_images_one_item": lambda: rc.vis_images(items, h, w)}, a.warmup, a.reps))
        res["bytes_floor"] = nbytes
        res["floor_ms_at_peak"] = round(sum(nbytes.values()) / HBM_PEAK * 1e3, 4)
        res["fraction_of_hbm_peak"] = round(sum(nbytes.values()) / (res["suite_ms"] * 1e-3) / HBM_PEAK, 3)
        if not a.no_render:
            if nb:
                res["render_ms"] = transient_render_ms(h, w, 1, 3)
            else:
                from bench_eval import render_ms
                res["render_ms"] = render_ms(h, w, a.warmup, a.reps)
            res["suite_over_render"] = round(res["suite_ms"] / res["render_ms"], 4)
        if not a.no_host:
            t0 = time.perf_counter()
            copied = {}                                         # an aliased key is copied once
            host = {k: copied.setdefault(v.data_ptr(), v.cpu().numpy()) for k, v in r.items()}
            host_mask = mask.cpu().numpy()
            res["host_copy_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            res["host_copy_MB"] = round(sum(v.nbytes for v in copied.values()) / 1e6, 1)
            lut = rc_ext.vis_turbo_lut()
            t0 = time.perf_counter()
            pics, _ = ref.suite(host, lut, img_scale=cfg.img_scale, masks=host_mask, transient=bool(nb), dtype=np.float32)
            u8 = {k: ref.to_u8(v) for k, v in pics.items()}
            res["host_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            off = {k: int(np.abs(u8[k].astype(np.int16) - pictures[k].cpu().numpy().astype(np.int16)).max()) for k in pictures
                   if "depth" not in k}
            res["max_step_off_host_u8"] = max(off.values())
        emit(res)


if __name__ == "__main__":
    main()
