"""The renders behind tests/golden/scalar_batch_pin.npz and tests/test_gpu_fused_scalar_batches.py.

The one-wave fused kernel (rc_set_fused(3): k_cache_fused whatever the batch size) reads the scalars of each of its phases
from a compact per-phase record of its arguments, fetched one phase ahead of use.  The cases vary exactly the inputs whose
scalars changed place: the jitter pointers and the resamplers' u specs, `lights`, the percentile triple, and `normals`
(which selects the GRAD instantiation).  Hotdog synthetic weights, `synthetic_rays`; a case `<name>` renders
{"<name>/<output>": float32 array}:

  plain (render_rays), ray counts 1 (a lone ray), 3 and 5 (partial workgroups, whose idle waves take ray n - 1), 4 (exactly
  one workgroup) and 257 (64 workgroups and one ray):
    all/n<k>           every _CACHE_DEVICE_KEYS output (GRAD), jitter on all three levels, lights
    nonorm_nojit/n<k>  every key but `normals` (GRAD = false), no jitter, lights
    nolights/n<k>      every key, jitter, `lights` null
    pct/n<k>           every key, jitter, lights, on a handle whose percentiles are (10, 40, 90)
  front/n5, front/n257     render_transient front end (FRONT) on cornell weights: jittered with `normals` | neither
  export/n5, export/n257   one render_material pass (EXPORT), smooth weights, fixed randoms

Run as a program it writes the renders of PIN_CASES into the .npz named on its command line, with the library's
arithmetic and source hash (tools/make_scalar_batch_pin.py runs it on a build of the parent commit).
"""
import dataclasses
import sys

import numpy as np
import torch

import common
import nrc_amd

SIZES = (1, 3, 4, 5, 257)
SEED_RAYS, SEED_JIT = 20261021, 23
PCT = (10.0, 40.0, 90.0)
FUSED, STAGED = 3, 0          # rc_set_fused: the one-wave fused kernel | one launch per stage
PIN_CASES = ("all/n257",)     # jitter and lights, every output


def rays(n, lights=True):
    r = nrc_amd.synthetic_rays(n, seed=SEED_RAYS + n).hot_fields()
    if not lights:
        del r["lights"]
    return r


def randoms(n):
    return {"jitter": common.jitters(n, seed=SEED_JIT + n)}


def plain_cases():
    """[(name, handle kind, rays, randoms or None, outputs)]"""
    from nrc_amd.model import _CACHE_DEVICE_KEYS
    keys = list(_CACHE_DEVICE_KEYS)
    assert "normals" in keys and "light_dists" in keys and "distance_median" in keys
    cases = []
    for n in SIZES:
        cases += [(f"all/n{n}", "default", rays(n), randoms(n), keys),
                  (f"nonorm_nojit/n{n}", "default", rays(n), None, [k for k in keys if k != "normals"]),
                  (f"nolights/n{n}", "default", rays(n, lights=False), randoms(n), keys),
                  (f"pct/n{n}", "pct", rays(n), randoms(n), keys)]
    return cases


def _np(res, prefix):
    torch.cuda.synchronize()
    return {prefix + "/" + k: np.ascontiguousarray(v.cpu().numpy(), dtype=np.float32) for k, v in res.items()}


def render_plain(mode=FUSED, only=None):
    out = {}
    cfg = nrc_amd.hotdog_config()
    assert tuple(cfg.percentiles) != PCT
    handles = {"default": common.make_rc(), "pct": common.make_rc(cfg=dataclasses.replace(cfg, percentiles=PCT))}
    for rc in handles.values():
        rc.set_fused(mode)
    for name, kind, r, rnd, keys in plain_cases():
        if only is None or name in only:
            out.update(_np(handles[kind].render_rays(r, rnd, outputs=keys), name))
    return out


def render_forms(mode=FUSED):
    """FRONT and EXPORT at n = 5 and n = 257."""
    from nrc_amd import rc_ext
    from oracle import material_ref
    out = {}
    ht = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    ht.load_weights(common.weights_transient_np())
    ht.set_fused(mode)
    flat = [k for k, kind in rc_ext.TRANSIENT_OUTPUTS if kind != "bins"]          # the [n, 3] / [n] outputs
    assert "normals" in flat
    out.update(_np(ht.render_transient(nrc_amd.synthetic_transient_rays(5).hot_fields(), {"jitter": common.jitters(5, seed=4)},
                                       outputs=["rgb"] + flat), "front/n5"))
    out.update(_np(ht.render_transient(nrc_amd.synthetic_transient_rays(257).hot_fields(), None,
                                       outputs=[k for k in flat if k != "normals"]), "front/n257"))
    cfg = nrc_amd.hotdog_config()
    hm = rc_ext.RadianceCache(cfg, 0)
    hm.load_weights(common.weights_material_np(True))
    hm.set_fused(mode)
    for n in (5, 257):
        cres, mres = hm.render_material(nrc_amd.synthetic_rays(n, seed=77 + n).hot_fields(), material_ref.draw_randoms(cfg, n, seed=3))
        out.update(_np({**{"c:" + k: v for k, v in cres.items()}, **{"m:" + k: v for k, v in mres.items()}}, f"export/n{n}"))
    return out


if __name__ == "__main__":
    from nrc_amd import rc_ext
    what = sys.argv[2] if len(sys.argv) > 2 else "pin"
    if what == "pin":
        res = render_plain(FUSED, only=PIN_CASES)
    else:                      # "compare": both plans, every case; the fused renders as f:<key>, the staged as s:<key>
        fused = {**render_plain(FUSED), **render_forms(FUSED)}
        staged = {**render_plain(STAGED), **render_forms(STAGED)}
        res = {**{"f:" + k: v for k, v in fused.items()}, **{"s:" + k: v for k, v in staged.items()}}
    np.savez(sys.argv[1], mlp_arithmetic=rc_ext.mlp_arithmetic(), source_hash=rc_ext.source_hash(), **res)
