"""The directional-encoding coefficients the kernels are compiled with (csrc/rc_ide_coef.h, rows in rc_ide_coef.inc)
against build_ide_table (csrc/rc_pack_host.h), the one source of the table: bit for bit.

hostcheck (the CPU build of the host-only code, under AddressSanitizer + UBSan) includes the same header as the device
code and writes both tables; `hostcheck --ide-inc` prints rc_ide_coef.inc from build_ide_table, and the committed file
must be that text.  The table that callers read through the handle (h->ide_table) is build_ide_table's as before.
"""
import os
import subprocess

import numpy as np

from test_hostcheck import CSRC, hostcheck  # noqa: F401  (fixture)

TERMS, ZPOW = 36, 17


def test_compiled_constants_equal_the_built_table_bit_for_bit(hostcheck):  # noqa: F811
    d, _, _ = hostcheck
    built = np.fromfile(d / "out_ide.bin", dtype=np.uint32)[: TERMS * ZPOW].reshape(TERMS, ZPOW)
    const = np.fromfile(d / "out_ide_const.bin", dtype=np.uint32).reshape(TERMS, ZPOW)
    assert np.array_equal(const, built), np.argwhere(const != built)[:8]
    # the table is not empty, and the entries the kernels use (k <= l - m, l - m - k even) hold all of it
    ls = [1] * 2 + [2] * 3 + [4] * 5 + [8] * 9 + [16] * 17
    ms = [i for l in (1, 2, 4, 8, 16) for i in range(l + 1)]
    used = np.array([[k <= l - m and (l - m - k) % 2 == 0 for k in range(ZPOW)] for l, m in zip(ls, ms)])
    assert (const.view(np.float32)[used] != 0).all()
    assert not const.view(np.float32)[~used].any()          # zeros of either sign


def test_committed_rows_are_the_generator_output(hostcheck):  # noqa: F811
    r = subprocess.run([os.path.join(CSRC, "hostcheck"), "--ide-inc"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(os.path.join(CSRC, "rc_ide_coef.inc")) as f:
        assert f.read() == r.stdout
