"""The textured export on the mesh of tools/bench_mesh.py: the isosurface of the last level's density at its
median over the box [-1, 1]^3, on the bench's synthetic "shell" weight set (density_shift 4) with the material stage's
weights beside it.  Per case <lattice size>:<cell size r>:

  rc_bake_atlas     the four default keys of mesh.bake_atlas (material [H,W,5], normals_pred [H,W,3]) and the coverage:
                    ms, texels/s and bytes written/s (33 B per texel)
  rc_atlas_points   points [n,3] and owner [n] of the whole atlas alone: ms, texels/s, bytes written/s (16 B per texel)

Each call is timed with its own pair of device events, 3 warm-ups and 10 timed calls, the median reported.  A case whose
atlas would exceed 16384 texels on a side is reported as refused (the 128^3 mesh has 11.4 M triangles: r = 6 is the largest
cell that fits).

  python tools/bench_atlas.py                       # writes profiles/atlas_bench.txt
  python tools/bench_atlas.py --cases 64:8 --reps 3 --out /tmp/atlas.txt
  rocprofv3 --kernel-trace --stats -d /tmp/atlas_prof -- python tools/bench_atlas.py --cases 64:8 --out /tmp/atlas.txt
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_mesh import median_ms  # noqa: E402

BAKE_OUTPUTS = ("material", "normals_pred", "coverage")
BAKE_BYTES, POINTS_BYTES = 5 * 4 + 3 * 4 + 1, 3 * 4 + 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["128:8", "128:6", "64:8"], help="<lattice size>:<cell size>")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "atlas_bench.txt"))
    a = ap.parse_args()
    import torch

    sys.path.insert(0, ROOT)
    import nrc_amd
    from nrc_amd import mesh, rc_ext

    cfg = nrc_amd.hotdog_config()
    rc = rc_ext.RadianceCache(cfg, 0)
    rc.load_weights(nrc_amd.synthetic_weights(cfg, passes=("cache", "material"), density_shift=4.0))
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    lines = ["textured export, first measurements (no earlier figure to compare with): " + torch.cuda.get_device_name(0),
             f"shell weights (density_shift 4) + material weights, box [-1, 1]^3, last level, iso = median of the lattice; "
             f"median of {a.reps} calls after {a.warmup} warm-ups, one device-event pair per call (min .. max in brackets)", ""]
    meshes = {}
    for case in a.cases:
        n, r = (int(x) for x in case.split(":"))
        if n not in meshes:
            field = rc.density_lattice(lo, hi, (n, n, n))
            meshes[n] = mesh.extract_mesh(rc, float(field.reshape(-1).median()), lo, hi, (n, n, n))
            del field
        m = meshes[n]
        T = int(m.triangles.shape[0])
        head = f"{n}^3 mesh, T = {T}, r = {r}"
        try:
            cols, rows, W, H = mesh.atlas_layout(T, r)
        except rc_ext.RcError as e:
            lines += [f"{head}: refused, a side of the atlas would exceed 16384 texels ({e})", ""]
            continue
        texels = W * H
        bake = median_ms(lambda: rc.bake_atlas(m.vertices, m.triangles, r, BAKE_OUTPUTS), a.warmup, a.reps)
        pts = median_ms(lambda: rc.atlas_points(m.vertices, m.triangles, r), a.warmup, a.reps)
        lines += [f"{head}: atlas {W} x {H} = {texels} texels ({cols} x {rows} cells)",
                  f"  rc_bake_atlas     {bake[0]:10.3f} ms [{bake[1]:.3f} .. {bake[2]:.3f}]  {texels / bake[0] * 1e-6:8.3f} G texels/s"
                  f"  {texels * BAKE_BYTES / bake[0] * 1e-6:9.1f} GB/s written ({BAKE_BYTES} B per texel)",
                  f"  rc_atlas_points   {pts[0]:10.3f} ms [{pts[1]:.3f} .. {pts[2]:.3f}]  {texels / pts[0] * 1e-6:8.3f} G texels/s"
                  f"  {texels * POINTS_BYTES / pts[0] * 1e-6:9.1f} GB/s written ({POINTS_BYTES} B per texel)", ""]
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
