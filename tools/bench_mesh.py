"""The surface export at 128^3 and 256^3 on the bench's synthetic "shell" weight set (density_shift 4):
rc_density_lattice over the box [-1, 1]^3 and rc_isosurface of that lattice at its median (half of the lattice inside: a
surface through the whole box).  Each call is timed with its own pair of device events, 3 warm-ups and 10 timed calls, the
median reported.  Per size:

  lattice fill   ms, points/s and the achieved bytes/s against the algorithmic 1024 B per point (8 levels x 8 corners x
                 4 features x 4 B of the last level's lookup)
  count pass     rc_isosurface with capacities 0 (classify + the two scans)
  extraction     rc_isosurface with exact capacities (the count pass again + both emission kernels): ms and bytes/s against
                 4 B per lattice point read once; V and T

  python tools/bench_mesh.py                 # writes profiles/mesh_bench.txt
  python tools/bench_mesh.py --sizes 64 --out /tmp/mesh.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def median_ms(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.txt"))
    a = ap.parse_args()
    import torch

    sys.path.insert(0, ROOT)
    import nrc_amd
    from nrc_amd import rc_ext

    cfg = nrc_amd.hotdog_config()
    rc = rc_ext.RadianceCache(cfg, 0)
    rc.load_weights(nrc_amd.synthetic_weights(cfg, density_shift=4.0))
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    lines = ["surface export, first measurements (no earlier figure to compare with): " + torch.cuda.get_device_name(0),
             f"shell weights (density_shift 4), box [-1, 1]^3, last level, iso = median of the lattice; median of {a.reps} "
             f"calls after {a.warmup} warm-ups, one device-event pair per call (min .. max in brackets)", ""]
    for n in a.sizes:
        dims, pts = (n, n, n), n ** 3
        fill = median_ms(lambda: rc.density_lattice(lo, hi, dims), a.warmup, a.reps)
        field = rc.density_lattice(lo, hi, dims)
        iso = float(field.reshape(-1).float().median())
        counts = torch.zeros(2, dtype=torch.int64, device="cuda")
        count = median_ms(lambda: rc.isosurface_into(field, iso, lo, hi, None, None, None, counts), a.warmup, a.reps)
        V, T = (int(c) for c in counts.tolist())
        v = torch.empty((V, 3), device="cuda")
        vn = torch.empty((V, 3), device="cuda")
        t = torch.empty((T, 3), dtype=torch.int32, device="cuda")
        full = median_ms(lambda: rc.isosurface_into(field, iso, lo, hi, v, vn, t, counts), a.warmup, a.reps)
        lines += [f"{n}^3 = {pts} points, iso {iso:.6g}, V = {V}, T = {T}",
                  f"  rc_density_lattice      {fill[0]:9.3f} ms [{fill[1]:.3f} .. {fill[2]:.3f}]  {pts / fill[0] * 1e-6:8.2f} G points/s"
                  f"  {pts * 1024 / fill[0] * 1e-9:8.1f} TB/s of the algorithmic 1024 B per point",
                  f"  rc_isosurface, count    {count[0]:9.3f} ms [{count[1]:.3f} .. {count[2]:.3f}]  "
                  f"{pts * 4 / count[0] * 1e-6:8.1f} GB/s of 4 B per lattice point read once",
                  f"  rc_isosurface, extract  {full[0]:9.3f} ms [{full[1]:.3f} .. {full[2]:.3f}]  "
                  f"{pts * 4 / full[0] * 1e-6:8.1f} GB/s of 4 B per lattice point read once"
                  f"  (writes {(V * 24 + T * 12) * 1e-6:.1f} MB of mesh)", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
