"""Cases shared by the tests of the material stage's random plan (tests/test_material_randoms_plan.py, test_prngcheck.py,
test_gpu_material_randoms.py): (n rays, K secondary samples) x train x env_sampler x loss_key x vmf_noise.

  (1, 2)      one-element segments; Kd = 1, so the cosine sampler's member has zero elements (Kc = round(0.5) = 0)
  (3, 6)      odd element counts; Kc = 2, Kl = 1 (Kc != Kl); the two-plane members have an odd row count (n Ks = 9)
  (257, 8)    a segment that ends one element into a workgroup (the jitter: 257 elements, 129 blocks)
  (1000, 32)  the render-time sample count, more than one workgroup in every member"""
import dataclasses
import itertools

import numpy as np

import nrc_amd
from nrc_amd import prng

SIZES = [(1, 2), (3, 6), (257, 8), (1000, 32)]
FLAGS = list(itertools.product([False, True], repeat=4))            # train, env_sampler, loss_key, vmf_noise
LOSS_KEY = prng.PRNGKey(99)
CFG = nrc_amd.hotdog_config()
LEVELS = [int(lvl[2]) for lvl in CFG.sampling_strategy]


def cfg_for(K):
    return dataclasses.replace(CFG, num_secondary_samples=K)


def model_key(n):
    return prng.PRNGKey(7 + n)


def python_plan(n, K, train, env, loss, vmf):
    return prng.material_stage_plan(model_key(n), n, cfg_for(K), train=train, env_sampler=env,
                                    loss_key=LOSS_KEY if loss else None, vmf_noise=vmf)


def c_plan(n, K, train, env, loss, vmf, capacity=32):
    from nrc_amd import rc_ext
    flags = ((rc_ext.RC_PRNG_PLAN_TRAIN if train else 0) | (rc_ext.RC_PRNG_PLAN_ENV_SAMPLER if env else 0)
             | (rc_ext.RC_PRNG_PLAN_VMF_NOISE if vmf else 0))
    segs, count, words = rc_ext.material_randoms_plan(model_key(n), n, K, CFG.diffuse_sample_fraction, CFG.num_vmf, LEVELS,
                                                      flags, LOSS_KEY if loss else None, capacity)
    return [segs[i] for i in range(count)], words


def rows_of(plan):
    """(id, mode, element count, key0, key1) per draw of a Python plan: what a C segment must hold."""
    return [(prng.member_id(d.name), d.mode, int(np.prod(d.shape)), int(d.key[0]), int(d.key[1])) for d in plan]


def spans_of(segs):
    """[(lo, hi, id)] word spans the segments write, sorted; a two-plane segment has two."""
    out = []
    for g in segs:
        if g.offset2 >= 0:
            out += [(g.offset, g.offset + (g.n + 1) // 2, g.id), (g.offset2, g.offset2 + g.n // 2, g.id)]
        else:
            out.append((g.offset, g.offset + g.n, g.id))
    return sorted(out)
