#!/usr/bin/env python
"""Writes tests/golden/scalar_batch_pin.npz: the PIN_CASES of tests/scalar_batch_cases.py (the one-wave fused kernel on 257
rays with jitter and lights, every output) as the library of THIS checkout computes them, for both arithmetics.  Run once,
on the parent of the change that moved the fused kernel's scalars into per-phase argument records;
tests/test_gpu_fused_scalar_batches.py then holds the changed library to it.

  make -C neural-radiance-caching_amd/csrc -j16 all variant-f32
  python tools/make_scalar_batch_pin.py [out.npz [default-library fp32-library]]

The two optional library paths name builds of the parent kept elsewhere.  Each build renders in a fresh child process of
its own (RC_HIP_LIBRARY names the library).  Keys: "<arithmetic>/<case>/<output>", plus "<arithmetic>/source_hash".
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
LIBS = {"bf16x3-split": os.path.join(ROOT, "neural-radiance-caching_amd", "librc_hip.so"),
        "f32-mfma": os.path.join(ROOT, "build", "f32", "librc_hip.so")}


def render_child(lib, path):
    env = {**os.environ, "RC_HIP_LIBRARY": lib, "PYTHONPATH": os.pathsep.join([ROOT, TESTS, os.environ.get("PYTHONPATH", "")])}
    r = subprocess.run([sys.executable, os.path.join(TESTS, "scalar_batch_cases.py"), path, "pin"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"render on {lib} ended with {r.returncode}: {r.stderr[-3000:]}")
    return dict(np.load(path))


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(TESTS, "golden", "scalar_batch_pin.npz")
    libs = dict(LIBS)
    if len(sys.argv) > 3:
        libs = {"bf16x3-split": os.path.abspath(sys.argv[2]), "f32-mfma": os.path.abspath(sys.argv[3])}
    pin = {}
    with tempfile.TemporaryDirectory() as tmp:
        for arith, lib in libs.items():
            g = render_child(lib, os.path.join(tmp, arith + ".npz"))
            got = str(g.pop("mlp_arithmetic"))
            assert got == arith, (lib, got)
            pin[arith + "/source_hash"] = g.pop("source_hash")
            for k, v in g.items():
                assert v.dtype == np.float32 and np.isfinite(v).all(), (arith, k)
                pin[arith + "/" + k] = v
    np.savez_compressed(dst, **pin)
    print(f"{dst}: {len(pin)} arrays, {os.path.getsize(dst)} bytes, sources "
          f"{ {a: str(pin[a + '/source_hash']) for a in libs} }")


if __name__ == "__main__":
    main()
