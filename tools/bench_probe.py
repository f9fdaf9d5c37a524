"""The probe of a surface point at the reference's own sizes: a 256 x 512 panorama, 128 lobes, P = 1 and
P = 16 probes.  One JSON line per P:

  probe_rays_ms, vmf_panorama_ms   rc_probe_rays / rc_vmf_panorama (the 8-bit picture), one device-event pair around
                                   --reps launches after --warmup, inputs and outputs resident on the device
  surface_probe_ms                 the whole probe.surface_probe call on a rendered --view (synthetic material weights),
                                   host clock around calls that end in a device synchronise
  secondary_render_ms, _share      probe.render_probe_rays alone on the same rays, and its share of surface_probe
  host_*_ms (P = 1 only)           the float32 numpy restatement (tests/probe_ref.py) of the same two steps on the host, as
                                   numpy runs it there (--host-reps calls, the best): the route without the two calls

  python tools/bench_probe.py
  python tools/bench_probe.py --probes 1 --no-host
"""
import argparse
import os
import sys
import time

import bench_common as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def events_ms(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / reps, 4)


def host_clock_ms(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3 / reps, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[256, 512], help="the panorama")
    ap.add_argument("--view", type=int, nargs=2, default=[256, 256], help="the rendered view the probe starts from")
    ap.add_argument("--lobes", type=int, default=128)
    ap.add_argument("--probes", type=int, nargs="+", default=[1, 16])
    bc.add_loop(ap, 10, 1000)
    ap.add_argument("--call-reps", type=int, default=5, help="repetitions of the whole surface_probe call")
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="leave out the numpy restatement's time")
    a = ap.parse_args()
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import nrc_amd
    from nrc_amd import camera, probe
    from nrc_amd import model as M

    hl, wl = a.size
    H, W = a.view
    cfg = nrc_amd.hotdog_config(render_chunk_size=16384)
    m = M.Model(cfg, 0)
    m.load_variables(nrc_amd.synthetic_weights(cfg, passes=("cache", "material"), seed=1))
    o = 4.0 * np.array([0.0, -0.87, 0.5])
    look = -o / np.linalg.norm(o)
    right = np.cross(look, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    c2w = np.stack([right, np.cross(right, look), -look, o], axis=1)
    cam = nrc_amd.Camera(pixtocam=nrc_amd.get_pixtocam(1.2 * W, W, H), camtoworld=c2w, near=2.0, far=6.0)
    rendering = camera.render_camera(m, cam, H, W, to_host=False, keys=("distance_median", "normals_to_use"))
    g = np.random.Generator(np.random.PCG64(7))
    for P in a.probes:
        pixels = np.stack([g.integers(0, W, P), g.integers(0, H, P)], axis=1)
        pixels[0] = probe.default_pixel(H, W)
        view = probe.probe_view(m, cam, rendering, pixels)
        rows = np.arange(P)
        means = torch.from_numpy(g.normal(size=(P, a.lobes, 3)).astype(np.float32)).cuda()
        kappas = torch.from_numpy(g.uniform(0.0, 50.0, (P, a.lobes)).astype(np.float32)).cuda()
        logits = torch.from_numpy(g.normal(size=(P, a.lobes)).astype(np.float32)).cuda()
        res = {"case": "probe", "P": P, "panorama": [hl, wl], "lobes": a.lobes, "view": [H, W], "rays": P * hl * wl,
               "lobe_evaluations": P * hl * wl * a.lobes}
        res["probe_rays_ms"] = events_ms(lambda: m.rc.probe_rays(view, rows, hl, wl, cfg.secondary_near, cfg.secondary_far),
                                         a.warmup, a.reps)
        res["vmf_panorama_ms"] = events_ms(lambda: m.rc.vmf_panorama(means, kappas, logits, hl, wl, srgb=False, u8=True),
                                           a.warmup, a.reps)
        rays, _ = m.rc.probe_rays(view, rows, hl, wl, cfg.secondary_near, cfg.secondary_far)
        res["secondary_render_ms"] = host_clock_ms(lambda: probe.render_probe_rays(m, rays), 1, a.call_reps)
        res["surface_probe_ms"] = host_clock_ms(lambda: probe.surface_probe(m, cam, rendering, pixels, size=(hl, wl)), 1,
                                                a.call_reps)
        res["secondary_render_share"] = round(res["secondary_render_ms"] / res["surface_probe_ms"], 4)
        if P == 1 and not a.no_host:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import probe_ref as ref
            hv = {k: v.cpu().numpy() for k, v in view.items()}
            mh, kh, lh = (t.cpu().numpy() for t in (means, kappas, logits))

            def best(fn):
                times = []
                for _ in range(a.host_reps):
                    t0 = time.perf_counter()
                    fn()
                    times.append(time.perf_counter() - t0)
                return round(min(times) * 1e3, 2)

            res["host_threads"] = torch.get_num_threads()
            res["host_probe_rays_ms"] = best(lambda: ref.probe_rays(hv, rows, hl, wl, cfg.secondary_near, cfg.secondary_far,
                                                                    dtype=np.float32))
            res["host_vmf_panorama_ms"] = best(lambda: ref.to_u8(ref.vmf_image(mh, kh, lh, hl, wl, dtype=np.float32)[1]))
        bc.emit(res)


if __name__ == "__main__":
    main()
