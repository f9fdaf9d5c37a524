"""rc_vis_images' host-only checks and bin-sum plan (csrc/rc_vis_plan.h) in the `make hostcheck` program: compiled for the
CPU under AddressSanitizer + UBSan and run on fixed item tables (tests/test_hostcheck.py builds and runs the program)."""
import numpy as np

from test_hostcheck import hostcheck  # noqa: F401  (fixture)


def test_vis_plan_shares_bin_sums_and_refuses_faulty_tables(hostcheck):  # noqa: F811
    d = hostcheck[0]
    v = np.fromfile(d / "out_vis_plan.bin", dtype=np.float32).tolist()
    # three sums: histogram b with 3 x 5 bins (items 1 and 3), histogram c, histogram b read as 1 x 15 bins
    assert v[:7] == [3, -1, 0, 1, 0, 2, -1]
    assert v[7:] == [1.0] * 14 + [0.0]
