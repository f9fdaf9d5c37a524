"""The mask loss restatement (tests/mask_loss_ref.py), the schedules of train.mask_terms, the backward rays and
MaskLossConfig, on the CPU."""
import dataclasses
import inspect

import numpy as np
import torch

import mask_loss_ref as mr
from nrc_amd import train
from nrc_amd.config import MaskLossConfig

PAD = 1e-3


def _acc(n, seed=0):
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).uniform(0.0, 1.0, n))


def test_known_answers():
    n = 12
    acc = _acc(n)
    # acc == m: pad * wt
    m = acc.clone()
    want = torch.where(m > 0.5, torch.tensor(3.0), torch.tensor(0.25)).double() * PAD
    got = mr.mask_loss(acc, m, None, PAD, 3.0, 0.25)
    assert abs(float(got) - float(want.mean())) < 1e-15
    # a mask of exactly 0.5 takes the empty weight (masks > 0.5 is strict)
    half = torch.full((n,), 0.5, dtype=torch.float64)
    got = mr.mask_loss(acc, half, None, PAD, 100.0, 2.0)
    want = (2.0 * torch.sqrt((acc - 0.5) ** 2 + PAD ** 2)).mean()
    assert abs(float(got) - float(want)) < 1e-15
    above = torch.full((n,), float(np.nextafter(np.float32(0.5), np.float32(1.0))), dtype=torch.float64)
    got = mr.mask_loss(acc, above, None, PAD, 100.0, 2.0)
    assert abs(float(got) - float((100.0 * torch.sqrt((acc - above) ** 2 + PAD ** 2)).mean())) < 1e-12
    # lossmult = 0 rows contribute 0 but still count in the mean
    lm = torch.ones(n, dtype=torch.float64)
    lm[::3] = 0.0
    m = torch.zeros(n, dtype=torch.float64)
    per = torch.sqrt(acc ** 2 + PAD ** 2)
    got = mr.mask_loss(acc, m, lm, PAD, 1.0, 1.0)
    assert abs(float(got) - float(per[lm > 0].sum() / n)) < 1e-15
    # masks=None equals ones
    assert float(mr.mask_loss(acc, None, lm, PAD, 0.7, 0.2)) == float(mr.mask_loss(acc, torch.ones_like(acc), lm, PAD, 0.7, 0.2))
    # zero_masks with weights (0, w) = w mean(lm sqrt(acc^2 + pad^2)), through both spellings
    w = 0.1
    want = w * float((lm * per).mean())
    terms = dict(charb_padding=PAD, weight_opaque=0.0, weight_empty=w, zero_masks=1)
    assert abs(float(mr.mask_terms_loss(acc, torch.ones_like(acc), lm, terms)) - want) < 1e-15
    assert abs(float(mr.mask_loss(acc, m, lm, PAD, 5.0, 5.0, empty_loss_weight=w)) - want) < 1e-15
    # the [n, n, 1] broadcast of the reference's literal shapes has the same mean
    lit = mr.mask_loss_literal_shapes(acc.numpy(), lm.numpy(), PAD, w)
    assert abs(lit - want) < 1e-15


def test_gradient_matches_finite_difference():
    rng = np.random.Generator(np.random.PCG64(3))
    n, S = 6, 9
    dens = rng.uniform(0.0, 0.3, (n, S))                        # semi-transparent rays: acc well inside (0, 1)
    tdist = np.sort(rng.uniform(2.0, 6.0, (n, S + 1)), axis=-1)
    dirs = rng.normal(size=(n, 3))
    masks = np.array([0.0, 1.0, 0.5, 0.3, 0.8, 1.0])
    lm = np.array([1.0, 0.0, 2.0, 0.5, 1.5, 1.0])
    for terms in (dict(charb_padding=PAD, weight_opaque=1.0, weight_empty=0.6, zero_masks=0),
                  dict(charb_padding=PAD, weight_opaque=0.0, weight_empty=0.1, zero_masks=1)):
        _, g, _ = mr.restated(dens, tdist, dirs, masks, lm, terms, torch.float64)
        h = 1e-6
        fd = np.zeros_like(dens)
        for i in range(n):
            for s in range(S):
                dp, dm = dens.copy(), dens.copy()
                dp[i, s] += h
                dm[i, s] -= h
                fd[i, s] = (mr.restated(dp, tdist, dirs, masks, lm, terms, torch.float64)[0]
                            - mr.restated(dm, tdist, dirs, masks, lm, terms, torch.float64)[0]) / (2 * h)
        assert np.abs(g).max() > 1e-4
        assert np.abs(g - fd).max() <= 1e-8 + 1e-6 * np.abs(g).max(), np.abs(g - fd).max()
        assert np.all(g[lm == 0.0] == 0.0)


def test_schedules_against_hand_values():
    # ease: start 0.2, transition 0.4, min 0.1
    ease = dict(use_mask_weight_ease=True, mask_weight_ease_start=0.2, mask_weight_ease_frac=0.4, mask_weight_ease_min=0.1)
    for tf, want in ((0.0, 0.1), (0.2, 0.1), (0.4, 0.55), (1.0, 1.0)):
        cfg = dataclasses.replace(MaskLossConfig(), **ease)
        t = train.mask_terms(tf, cfg)
        assert abs(t["mask"]["weight_opaque"] - want * cfg.opaque_loss_weight) < 1e-12, tf
        assert abs(t["mask"]["weight_empty"] - want * cfg.empty_loss_weight) < 1e-12, tf
        assert abs(t["mask_backwards"]["weight_empty"] - want * cfg.backward_mask_loss_weight) < 1e-12, tf
        assert t["mask_backwards"]["weight_opaque"] == 0.0 and t["mask_backwards"]["zero_masks"] == 1
        assert abs(mr.schedule_ease_in(tf, True, 0.2, 0.4, 0.1) - want) < 1e-12
    # ease with transition_frac = 0: the step function float(train_frac >= start)
    step = dataclasses.replace(MaskLossConfig(), use_mask_weight_ease=True, mask_weight_ease_start=0.5, mask_weight_ease_min=0.3)
    for tf, want in ((0.0, 0.0), (0.49, 0.0), (0.5, 1.0), (1.0, 1.0)):
        assert train.mask_terms(tf, step)["mask"]["weight_empty"] == want, tf
        assert mr.schedule_ease_in(tf, True, 0.5, 0.0, 0.3) == want
    # decay: start 0.5, transition 0.25, min 0.2 (> 0)
    dec = dataclasses.replace(MaskLossConfig(), use_mask_weight_decay=True, mask_weight_decay_start=0.5, mask_weight_decay_frac=0.25,
                              mask_weight_decay_min=0.2)
    for tf, want in ((0.0, 1.0), (0.5, 1.0), (0.625, 0.6), (1.0, 0.2)):
        assert abs(train.mask_terms(tf, dec)["mask"]["weight_opaque"] - want) < 1e-12, tf
        assert abs(mr.schedule_decay(tf, True, 0.5, 0.25, 0.2) - want) < 1e-12
    # both on: the product; scale multiplies; the defaults are all ones
    both = dataclasses.replace(dec, **ease)
    assert abs(train.mask_terms(0.625, both, scale=2.0)["mask"]["weight_empty"] - 2.0 * 0.6 * 1.0) < 1e-12
    assert abs(train.mask_terms(0.4, both)["mask_backwards"]["weight_empty"] - 0.1 * 0.55) < 1e-12
    t = train.mask_terms(0.3)
    assert t["mask"] == dict(charb_padding=1e-3, weight_opaque=1.0, weight_empty=1.0, zero_masks=0)
    assert t["mask_backwards"] == dict(charb_padding=1e-3, weight_opaque=0.0, weight_empty=0.1, zero_masks=1)
    # the restatement with decay / ease multiplied in equals the weights with them folded in
    acc, m = _acc(9, 4), (_acc(9, 5) > 0.5).double()
    a = mr.mask_loss(acc, m, None, PAD, 1.0, 0.5, decay=0.6, ease=0.55)
    b = mr.mask_loss(acc, m, None, PAD, 1.0 * 0.6 * 0.55, 0.5 * 0.6 * 0.55)
    assert abs(float(a) - float(b)) < 1e-15


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def test_backward_rays():
    rng = np.random.Generator(np.random.PCG64(7))
    z_lo = float(np.nextafter(np.float32(0.9), np.float32(0.0)))
    z_hi = float(np.float32(0.9))                               # |nrm_z| < 0.9 is strict: 0.9f itself takes `y`
    rim = lambda z: [np.sqrt(1.0 - z * z), 0.0, -z]
    look = np.concatenate([_unit(rng.normal(size=(40, 3))), [[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], rim(z_lo), rim(z_hi)]]).astype(np.float32)
    n = len(look)
    o = rng.normal(size=(n, 3)).astype(np.float32)
    u1 = rng.uniform(0.0, 1.0, n).astype(np.float32)
    u2 = rng.uniform(0.0, 1.0, n).astype(np.float32)
    u1[:3] = 0.0
    u1[-4:] = (0.0, 0.25, 0.5, 0.75)
    snm, eps, far = 0.2, 1e-2, 2.0
    r = mr.backward_rays(o, look, u1, u2, snm, eps, far)
    d, lk = r["directions"], look.astype(np.float64)
    lk_n = np.linalg.norm(lk, axis=-1)
    assert np.abs(np.linalg.norm(d, axis=-1) - 1.0).max() < 1e-6               # unit norm (look is unit to fp32 rounding)
    assert np.abs((d * -lk).sum(-1) - (1.0 - u1.astype(np.float64)) * lk_n ** 2).max() < 1e-6
    assert np.array_equal(d[u1 == 0.0], -lk[u1 == 0.0])                          # u1 = 0: exactly -look
    assert r["viewdirs"] is r["directions"]
    # both `up` branches and the 0.9 boundary: new_x = normalize(cross(up, nrm))
    R = mr.rotation_matrix(-lk)
    up_z = np.abs(lk[:, 2]) < float(np.float32(0.9))
    assert not up_z[-4] and up_z[-3] and up_z[-2] and not up_z[-1]
    for i in (n - 4, n - 3, n - 2, n - 1):
        up = np.array([0.0, 0.0, 1.0]) if up_z[i] else np.array([0.0, 1.0, 0.0])
        x = np.cross(up, -lk[i])
        assert np.abs(R[i, :, 0] - x / np.linalg.norm(x)).max() < 1e-9, i
        assert np.abs(R[i].T @ R[i] - np.eye(3)).max() < 1e-6, i
        assert np.array_equal(R[i, :, 2], -lk[i])
    # origin = o + (shadow_near_max - normal_eps) look to rounding; near / far
    s32, e32 = float(np.float32(snm)), float(np.float32(eps))
    assert np.abs(r["origins"] - (o.astype(np.float64) + (s32 - e32) * lk)).max() < 1e-12
    assert np.all(r["near"] == s32) and np.all(r["far"] == far)
    # the fp32 evaluation stays within fp32 rounding of the fp64 one
    r32 = mr.backward_rays(o, look, u1, u2, snm, eps, far, np.float32)
    assert r32["directions"].dtype == np.float32
    assert np.abs(r32["directions"] - d).max() < 5e-6 and np.abs(r32["origins"] - r["origins"]).max() < 1e-6


def test_config_defaults():
    c = MaskLossConfig()
    assert (c.charb_padding, c.opaque_loss_weight, c.empty_loss_weight) == (1e-3, 1.0, 1.0)     # configs.py:330, gin:367-368
    assert c.backward_mask_loss is True and c.backward_mask_loss_weight == 0.1                    # gin:375-376
    assert (c.shadow_near_max, c.secondary_normal_eps, c.secondary_far) == (0.2, 1e-2, 2.0)      # configs.py:635, :643, gin:19
    assert (c.use_mask_weight_decay, c.mask_weight_decay_frac, c.mask_weight_decay_start, c.mask_weight_decay_min) == (False, 0.0, 0.0, 0.0)
    assert (c.use_mask_weight_ease, c.mask_weight_ease_frac, c.mask_weight_ease_start, c.mask_weight_ease_min) == (False, 0.0, 0.0, 0.0)
    assert len(dataclasses.fields(c)) == 16


def test_new_parameters_default_to_none():
    for fn in (train.cache_stage_grads, train.cache_stage_step):
        p = inspect.signature(fn).parameters
        for name in ("mask_cfg", "masks", "look", "backward_randoms"):
            assert p[name].default is None, (fn.__name__, name)
    p = inspect.signature(train.cache_stage_fit).parameters
    assert p["mask_cfg"].default is None and p["masks_of"].default is None
    p = inspect.signature(train.mask_grads).parameters
    assert [k for k in p][:9] == ["rc", "rays", "jitters", "train_frac", "masks", "lossmult", "flat", "look", "backward_randoms"]
    assert all(p[k].default is None for k in ("masks", "lossmult", "flat", "look", "backward_randoms"))


def test_backward_mask_key_path():
    """The key path against its own written-out splits, and the draws' shapes and range (not pinned against jax)."""
    from nrc_amd import prng

    key = prng.PRNGKey(11)
    ku, ka = prng.backward_mask_keys(key)
    k = prng.split(key)
    want = prng.split(prng.split(prng.split(k[0])[0])[0])[0]
    assert np.array_equal(ku, want) and np.array_equal(ka, prng.split(k[1])[0])
    r = prng.backward_mask_randoms(key, 33, (64, 64, 32))
    u = prng.uniform(ku, (33, 2))
    assert np.array_equal(r["u1"], u[:, 0]) and np.array_equal(r["u2"], u[:, 1])
    assert r["u1"].min() >= 0.0 and r["u1"].max() < 1.0 and len(r["jitter"]) == 3 and r["jitter"][2].shape == (33, 1)
