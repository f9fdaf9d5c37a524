"""Writes matplotlib's 256-entry "turbo" colormap as float32: the initialiser list csrc/rc_turbo_lut.inc of the device's
constant table (rc_vis.hip) and tests/golden/turbo_lut.npy.  Run once; both files are committed."""
import os

import numpy as np
from matplotlib import colormaps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    lut = np.asarray(colormaps["turbo"](np.arange(256))[:, :3], np.float32)          # ListedColormap lookup by index
    assert lut.shape == (256, 3)
    np.save(os.path.join(ROOT, "tests", "golden", "turbo_lut.npy"), lut)
    rows = ["  " + ", ".join(f"{v:.9g}f" for v in row) + "," for row in lut]
    with open(os.path.join(ROOT, "neural-radiance-caching_amd", "csrc", "rc_turbo_lut.inc"), "w") as f:
        f.write("// matplotlib's \"turbo\" colormap, 256 x (r, g, b) as float32 (tools/gen_turbo_lut.py)\n")
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
