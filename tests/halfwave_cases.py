"""The renders behind tests/golden/halfwave_pin.npz, shared by tools/make_halfwave_pin.py (which writes the pin on the
parent commit) and tests/test_gpu_halfwave_pairs.py (which holds the library to it).

Two renders on the fused plan of the library that `RC_HIP_LIBRARY` (or the tree) names, every _CACHE_DEVICE_KEYS output
(`normals` among them: the GRAD instantiation):
  r64/   64 seeded rays (16 full workgroups)
  r5/    5 seeded rays (one full workgroup and one with three clamped rays)
Run as a program it writes them into the .npz named on its command line, with the library's arithmetic and source hash:
that is how a fresh child process renders on the fp32-MFMA build.
"""
import sys

import numpy as np
import torch

import common
import nrc_amd

SIZES = (64, 5)
SEED_RAYS = 20201109


def rays(n):
    return nrc_amd.synthetic_rays(n, seed=SEED_RAYS + n)


def render_all():
    """{"r<n>/<key>": float32 array}"""
    from nrc_amd.model import _CACHE_DEVICE_KEYS
    assert "normals" in _CACHE_DEVICE_KEYS
    rc = common.make_rc()
    rc.set_fused(True)
    out = {}
    for n in SIZES:
        res = rc.render_rays(rays(n).hot_fields(), None, outputs=list(_CACHE_DEVICE_KEYS))
        torch.cuda.synchronize()
        out.update({f"r{n}/{k}": v.cpu().numpy() for k, v in res.items()})
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


if __name__ == "__main__":
    from nrc_amd import rc_ext
    np.savez(sys.argv[1], mlp_arithmetic=rc_ext.mlp_arithmetic(), source_hash=rc_ext.source_hash(), **render_all())
