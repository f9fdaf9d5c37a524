"""The renders behind tests/golden/chain_pin.npz, shared by tools/make_chain_pin.py (which writes the pin on the parent
commit) and tests/test_gpu_fused_chain_pin.py (which holds the library to it and to the launch-per-stage plan).

The one-wave fused kernel (rc_set_fused(3): k_cache_fused whatever the batch size, in both arithmetics) fetches the
output pointers of its tail as one batch of scalar loads and writes the appearance features straight to the shader's
steps: neither may change a value.  Hotdog synthetic weights,
`synthetic_rays`; every render is a case `<name>` -> {"<name>/<output>": float32 array}:

  plain (render_rays), ray counts 1 (three idle waves clamped to ray n - 1), 5 (a partial second workgroup) and 260:
    all/n<k>        every _CACHE_DEVICE_KEYS output (GRAD instantiation), jitter and lights present
    nonorm/n<k>     every key but `normals` (GRAD = false)
    rgb/n<k>        `rgb` alone (18 null pointers in the batched tail)
    pct/n<k>        the three distance percentiles alone (the tail's per-lane pointer select)
  at n = 5 also
    all_nolights, all_nojit, pct_nolights_nojit, rgb_nojit
  wide/n260         every key, origins and directions scaled so that a good share of the samples lies outside the
                    bounding box and beyond the contraction radius (checked by the test on the ray geometry)
  front/n5          render_transient front end (FRONT) on cornell weights, jittered: the `rgb` histogram and every [n, 3] / [n]
                    output, `normals` among them (GRAD)
  front/n9          the same front end without jitter and without `normals` (GRAD = false), [n, 3] / [n] outputs only
  export/n5         one render_material pass (EXPORT), smooth weights, fixed randoms

Run as a program it writes the fused renders into the .npz named on its command line, with the library's arithmetic and
source hash: that is how a fresh child process renders on the fp32-MFMA build.
"""
import sys

import numpy as np
import torch

import common
import nrc_amd

SIZES = (1, 5, 260)
SEED_RAYS, SEED_JIT = 20261020, 11
PCT = ("distance_percentile_5", "distance_median", "distance_percentile_95")
FUSED, STAGED = 3, 0          # rc_set_fused: the one-wave fused kernel | one launch per stage


def rays(n, lights=True):
    r = nrc_amd.synthetic_rays(n, seed=SEED_RAYS + n).hot_fields()
    if not lights:
        del r["lights"]
    return r


def wide_rays(n):
    """Origins three times as far out and a far plane of 40: most of a ray runs outside the box and the unit ball."""
    r = nrc_amd.synthetic_rays(n, seed=SEED_RAYS + 7 * n, near=0.5, far=40.0).hot_fields()
    r["origins"] = np.ascontiguousarray(r["origins"] * np.float32(3.0))
    return r


def randoms(n):
    return {"jitter": common.jitters(n, seed=SEED_JIT + n)}


def key_sets():
    from nrc_amd.model import _CACHE_DEVICE_KEYS
    keys = list(_CACHE_DEVICE_KEYS)
    assert "normals" in keys and all(k in keys for k in PCT)
    return {"all": keys, "nonorm": [k for k in keys if k != "normals"], "rgb": ["rgb"], "pct": list(PCT)}


def plain_cases():
    """[(name, rays, randoms or None, outputs)]"""
    ks = key_sets()
    cases = [(f"{s}/n{n}", rays(n), randoms(n), ks[s]) for n in SIZES for s in ("all", "nonorm", "rgb", "pct")]
    cases += [("all_nolights", rays(5, lights=False), randoms(5), ks["all"]),
              ("all_nojit", rays(5), None, ks["all"]),
              ("pct_nolights_nojit", rays(5, lights=False), None, ks["pct"]),
              ("rgb_nojit", rays(5), None, ks["rgb"]),
              ("wide/n260", wide_rays(260), randoms(260), ks["all"])]
    return cases


def _np(res, prefix):
    torch.cuda.synchronize()
    return {prefix + "/" + k: np.ascontiguousarray(v.cpu().numpy(), dtype=np.float32) for k, v in res.items()}


def render_all(mode=FUSED):
    """Every case on plan `mode` of the library that `RC_HIP_LIBRARY` (or the tree) names."""
    from nrc_amd import rc_ext
    from oracle import material_ref
    out = {}
    rc = common.make_rc()
    rc.set_fused(mode)
    for name, r, rnd, keys in plain_cases():
        out.update(_np(rc.render_rays(r, rnd, outputs=keys), name))

    ht = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    ht.load_weights(common.weights_transient_np())
    ht.set_fused(mode)
    flat = [k for k, kind in rc_ext.TRANSIENT_OUTPUTS if kind != "bins"]          # the [n, 3] / [n] outputs
    assert "normals" in flat
    out.update(_np(ht.render_transient(nrc_amd.synthetic_transient_rays(5).hot_fields(), {"jitter": common.jitters(5, seed=4)},
                                       outputs=["rgb"] + flat), "front/n5"))
    out.update(_np(ht.render_transient(nrc_amd.synthetic_transient_rays(9).hot_fields(), None,
                                       outputs=[k for k in flat if k != "normals"]), "front/n9"))

    cfg = nrc_amd.hotdog_config()
    hm = rc_ext.RadianceCache(cfg, 0)
    hm.load_weights(common.weights_material_np(True))
    hm.set_fused(mode)
    cres, mres = hm.render_material(nrc_amd.synthetic_rays(5, seed=77).hot_fields(), material_ref.draw_randoms(cfg, 5, seed=3))
    out.update(_np({**{"c:" + k: v for k, v in cres.items()}, **{"m:" + k: v for k, v in mres.items()}}, "export/n5"))
    return out


if __name__ == "__main__":
    from nrc_amd import rc_ext
    np.savez(sys.argv[1], mlp_arithmetic=rc_ext.mlp_arithmetic(), source_hash=rc_ext.source_hash(), **render_all())
