"""The renders behind tests/golden/handoff_pin.npz, shared by tools/make_handoff_pin.py (which writes the pin on the
parent commit) and tests/test_gpu_register_handoff.py (which holds the library to it).

Three renders on the library that `RC_HIP_LIBRARY` (or the tree) names, each through another instantiation of the fused
kernel:
  cache/      33 jittered rays (eight full workgroups and one lane of a ninth), every _CACHE_DEVICE_KEYS output
  transient/  9 cornell rays through the fused front end (FRONT instantiation)
  material/   9 rays of the material stage on the fused plan (EXPORT instantiation), smooth weights, fixed randoms
Run as a program it writes them into the .npz named on its command line, with the library's arithmetic: that is how a
fresh child process renders on the fp32-MFMA build.
"""
import sys

import numpy as np
import torch

import common
import nrc_amd

N_CACHE, N_SMALL = 33, 9
SEED_RAYS, SEED_JIT = 20200823, 7


def cache_rays():
    return nrc_amd.synthetic_rays(N_CACHE, seed=SEED_RAYS)


def cache_randoms():
    return {"jitter": common.jitters(N_CACHE, seed=SEED_JIT)}


def render_all():
    """{"cache/<key>" | "transient/<key>" | "material/c:<key>" | "material/m:<key>": float32 array}"""
    from nrc_amd import rc_ext
    from nrc_amd.model import _CACHE_DEVICE_KEYS
    from oracle import material_ref
    out = {}
    rc = common.make_rc()
    rc.set_fused(True)
    res = rc.render_rays(cache_rays().hot_fields(), cache_randoms(), outputs=list(_CACHE_DEVICE_KEYS))
    torch.cuda.synchronize()
    out.update({"cache/" + k: v.cpu().numpy() for k, v in res.items()})

    ht = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    ht.load_weights(common.weights_transient_np())
    ht.set_fused(True)
    res = ht.render_transient(nrc_amd.synthetic_transient_rays(N_SMALL).hot_fields(),
                              {"jitter": common.jitters(N_SMALL, seed=4)})
    torch.cuda.synchronize()
    out.update({"transient/" + k: v.cpu().numpy() for k, v in res.items()})

    cfg = nrc_amd.hotdog_config()
    hm = rc_ext.RadianceCache(cfg, 0)
    hm.load_weights(common.weights_material_np(True))
    hm.set_fused(True)
    cres, mres = hm.render_material(nrc_amd.synthetic_rays(N_SMALL, seed=77).hot_fields(),
                                    material_ref.draw_randoms(cfg, N_SMALL, seed=3))
    torch.cuda.synchronize()
    out.update({"material/c:" + k: v.cpu().numpy() for k, v in cres.items()})
    out.update({"material/m:" + k: v.cpu().numpy() for k, v in mres.items()})
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


if __name__ == "__main__":
    from nrc_amd import rc_ext
    np.savez(sys.argv[1], mlp_arithmetic=rc_ext.mlp_arithmetic(), source_hash=rc_ext.source_hash(), **render_all())
