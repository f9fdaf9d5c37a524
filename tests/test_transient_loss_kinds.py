"""The loss family of rc_transient_data_backward_kind as restated in tests/transient_loss_kinds_ref.py, on
the CPU: dtof_to_itof, every loss type against plain loops, its closed-form gradient and finite differences, the
identities between the types, and the presets' provenance."""
import dataclasses
import math

import numpy as np
import pytest
import torch

import transient_data_loss_ref as tref
import transient_loss_kinds_ref as kref
from nrc_amd import config, rc_ext
from nrc_amd.config import TransientDataLossConfig

TYPES = rc_ext.TRANSIENT_LOSS_TYPES
BIASED = ("rawnerf_transient", "mse", "mse_itof", "rawnerf_transient_itof")
E = 0.01
PAIRS = ((75000000.0, 0.0), (425000000.0, 3.14159265359))
N, B = 2, 6


def _cfg(loss_type, use_itof=False, **kw):
    return dataclasses.replace(TransientDataLossConfig(), loss_type=loss_type, use_itof=use_itof,
                               itof_frequency_phase_shifts=PAIRS, **kw)


def _batch(seed=0):
    """2 rays, 6 bins, 3 channels: rgb, gt, a nocorr pair, lossmult and the loss_thresh that zeroes exactly one (ray,
    channel) pair."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rgb = rng.uniform(0.05, 1.0, (N, B, 3))
    gt = rng.uniform(0.05, 1.0, (N, B, 3))
    rn, gn = rng.uniform(0.05, 1.0, (N, B, 3)), rng.uniform(0.05, 1.0, (N, B, 3))
    gt[1, 3, 2] = 1.7
    lm = np.array([0.8, 1.3])
    return rgb, gt, rn, gn, lm, 1.5


def _t(a):
    return None if a is None else torch.from_numpy(np.asarray(a, np.float64))


# ---- 1. dtof_to_itof ---------------------------------------------------------------------------------------------------

def test_dtof_to_itof_rows_and_loops():
    rng = np.random.Generator(np.random.PCG64(1))
    x = rng.standard_normal((3, 7, 3))
    out = kref.dtof_to_itof(_t(x), PAIRS, E).numpy()
    assert out.shape == (3, 2 * len(PAIRS) + 1, 3)
    for i in range(3):
        for c in range(3):
            rows = kref._loop_rows([x[i, b, c] for b in range(7)], PAIRS, E)
            np.testing.assert_allclose(out[i, :, c], rows, rtol=1e-12, atol=1e-13)
    # the order: [cos, sin] of pair 0, [cos, sin] of pair 1, constant
    t = np.arange(7) * E / kref.C_LIGHT
    f, ph = PAIRS[1]
    np.testing.assert_allclose(out[:, 2, :], ((np.cos(2 * np.pi * f * t + ph) + 1)[None, :, None] * x).sum(1), rtol=1e-10)
    np.testing.assert_allclose(out[:, 3, :], ((np.sin(2 * np.pi * f * t + ph) + 1)[None, :, None] * x).sum(1), rtol=1e-10)
    np.testing.assert_allclose(out[:, 4, :], x.sum(1) / 2, rtol=1e-12)


def test_dtof_to_itof_zero_pairs_is_half_the_sum():
    x = np.random.Generator(np.random.PCG64(2)).standard_normal((2, 5, 3))
    out = kref.dtof_to_itof(_t(x), (), E).numpy()
    assert out.shape == (2, 1, 3)
    np.testing.assert_allclose(out[:, 0, :], x.sum(1) / 2, rtol=1e-14)


def test_dtof_to_itof_by_hand():
    """4 bins, one pair, f = c / (4 E): 2 pi f t_b = b pi / 2, so the cos row weighs the bins by 1 + (1, 0, -1, 0) and the
    sin row by 1 + (0, 1, 0, -1)."""
    f = kref.C_LIGHT / (4 * E)
    x = np.zeros((1, 4, 3))
    x[0, :, 0] = [1.0, 2.0, 3.0, 4.0]
    x[0, :, 1] = [4.0, 0.0, -1.0, 2.0]
    x[0, :, 2] = [0.5, 0.5, 0.5, 0.5]
    out = kref.dtof_to_itof(_t(x), ((f, 0.0),), E).numpy()[0]
    want = np.array([[2 * 1 + 2 + 0 + 4, 2 * 4 + 0 + 0 + 2, 2.0],
                     [1 + 2 * 2 + 3 + 0, 4 + 0 - 1 + 0, 2.0],
                     [5.0, 2.5, 1.0]])
    np.testing.assert_allclose(out, want, atol=1e-12)
    # phase pi / 2 turns the cos row into 1 - sin and the sin row into 1 + cos
    out2 = kref.dtof_to_itof(_t(x), ((f, math.pi / 2),), E).numpy()[0]
    np.testing.assert_allclose(out2[0, 0], 1 + 0 + 3 + 2 * 4, atol=1e-12)
    np.testing.assert_allclose(out2[1, 0], want[0, 0], atol=1e-12)


# ---- 2. every type ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("use_itof", [False, True])
@pytest.mark.parametrize("loss_type", TYPES)
def test_restatement_equals_loops(loss_type, use_itof):
    rgb, gt, rn, gn, lm, thresh = _batch()
    cfg = _cfg(loss_type, use_itof, loss_thresh=thresh, data_loss_mult=1.5)
    assert int((gt > thresh).any(1).sum()) == 1
    loss, mse = kref.data_loss(_t(rgb), _t(gt), _t(rn), _t(gn), _t(lm), cfg, E)
    l2, m2 = kref.loop_loss(rgb, gt, rn, gn, lm, cfg, E)
    assert float(loss) == pytest.approx(l2, rel=1e-12, abs=1e-14)
    assert float(mse) == pytest.approx(m2, rel=1e-12, abs=1e-14)


@pytest.mark.parametrize("use_itof", [False, True])
@pytest.mark.parametrize("loss_type", TYPES)
def test_autograd_equals_closed_form(loss_type, use_itof):
    rgb, gt, rn, gn, lm, thresh = _batch(3)
    cfg = _cfg(loss_type, use_itof, loss_thresh=thresh)
    _, _, G = kref.loss_and_G(rgb, gt, rn, gn, lm, cfg, E, torch.float64)
    want = kref.closed_G(_t(rgb), _t(gt), _t(rn), _t(gn), _t(lm), cfg, E).numpy()
    assert np.abs(want).max() > 0
    assert np.abs(G - want).max() <= 1e-12 * np.abs(want).max()
    assert not G[1, :, 2].any()                     # the pair over loss_thresh


@pytest.mark.parametrize("loss_type", BIASED)
def test_finite_differences(loss_type):
    """The biased types are plain functions of rgb up to the stop-gradient on the rawnerf scale, which is frozen at the
    base point here (the use_gt_rawnerf reading of the clip: a function of gt alone)."""
    rgb, gt, rn, gn, lm, thresh = _batch(4)
    cfg = _cfg(loss_type, True, loss_thresh=thresh, use_gt_rawnerf=True)
    _, _, G = kref.loss_and_G(rgb, gt, None, None, lm, cfg, E, torch.float64)
    f = lambda x: float(kref.data_loss(_t(x), _t(gt), None, None, _t(lm), cfg, E)[0])
    h = 1e-6
    rng = np.random.Generator(np.random.PCG64(5))
    for _ in range(12):
        i, b, c = rng.integers(N), rng.integers(B), rng.integers(3)
        up, dn = rgb.copy(), rgb.copy()
        up[i, b, c] += h
        dn[i, b, c] -= h
        fd = (f(up) - f(dn)) / (2 * h)
        assert fd == pytest.approx(G[i, b, c], rel=1e-6, abs=1e-9 * np.abs(G).max())


# ---- 3. identities ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("use_itof", [False, True])
@pytest.mark.parametrize("unbiased", sorted(kref.UNBIASED))
def test_unbiased_without_nocorr_is_twice_the_biased(unbiased, use_itof):
    rgb, gt, _, _, lm, thresh = _batch(6)
    lu, _, Gu = kref.loss_and_G(rgb, gt, None, None, lm, _cfg(unbiased, use_itof, loss_thresh=thresh), E, torch.float64)
    lb, _, Gb = kref.loss_and_G(rgb, gt, None, None, lm, _cfg(kref.UNBIASED[unbiased], use_itof, loss_thresh=thresh), E,
                                torch.float64)
    assert lu == pytest.approx(2.0 * lb, rel=1e-13)
    np.testing.assert_allclose(Gu, Gb, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("loss_type", ("rawnerf_transient_unbiased", "rawnerf_transient", "mse", "mse_unbiased"))
def test_use_itof_on_a_per_bin_type(loss_type):
    rgb, gt, rn, gn, lm, thresh = _batch(7)
    l0, m0, G0 = kref.loss_and_G(rgb, gt, rn, gn, lm, _cfg(loss_type, False, loss_thresh=thresh), E, torch.float64)
    l1, m1, G1 = kref.loss_and_G(rgb, gt, rn, gn, lm, _cfg(loss_type, True, loss_thresh=thresh), E, torch.float64)
    assert l1 == pytest.approx(l0 / B, rel=1e-13)
    np.testing.assert_allclose(G1, G0 / B, rtol=1e-12, atol=1e-16)
    I = kref.dtof_to_itof(_t(rgb - gt), PAIRS, E).numpy()
    w = np.repeat(lm[:, None], 3, 1)
    w[1, 2] = 0.0
    assert m1 == pytest.approx(float((w * (I ** 2).sum(1) / I.shape[1]).mean()), rel=1e-12)
    assert m0 == pytest.approx(float((w * ((rgb - gt) ** 2).sum(1)).mean()), rel=1e-12)


def test_default_type_is_the_existing_restatement():
    rgb, gt, rn, gn, lm, thresh = _batch(8)
    cfg = dataclasses.replace(TransientDataLossConfig(), loss_thresh=thresh)
    a = kref.data_loss(_t(rgb), _t(gt), _t(rn), _t(gn), _t(lm), cfg, E)
    b = tref.data_loss(_t(rgb), _t(gt), _t(rn), _t(gn), _t(lm), cfg)
    assert float(a[0]) == pytest.approx(float(b[0]), rel=1e-14) and float(a[1]) == pytest.approx(float(b[1]), rel=1e-14)


# ---- 4. presets and the default config ----------------------------------------------------------------------------------

def test_presets_and_default_config():
    d = TransientDataLossConfig()
    assert d.itof_frequency_phase_shifts == () and d.use_itof is False and d.loss_type == "rawnerf_transient_unbiased"
    assert config.transient_data_loss_preset("cornell") == d
    assert set(config.TRANSIENT_DATA_LOSS_PRESETS) == {"cornell", "cornell_itof", "pots_itof", "peppers_itof", "house_itof",
                                                       "kitchen_itof", "steady_state", "mse"}
    pi = 3.14159265359                                  # the gins' literal
    hi = ((75000000.0, 0.0), (75000000.0, pi), (425000000.0, 0.0), (425000000.0, pi))
    lo = ((30000000.0, 0.0), (30000000.0, pi), (170000000.0, 0.0), (170000000.0, pi))
    for name, pairs, mult, eps in (("cornell_itof", hi, 1.0, 1e-2), ("pots_itof", hi, 1.0, 1e-2), ("peppers_itof", lo, 0.1, 1e-2),
                                   ("house_itof", lo, 0.1, 1e-1), ("kitchen_itof", lo, 1.0, 1e-2), ("steady_state", (), 1.0, 1e-2)):
        p = config.transient_data_loss_preset(name)
        assert p.loss_type == "rawnerf_transient_itof" and p.use_itof is True, name
        assert p.itof_frequency_phase_shifts == pairs and p.data_loss_mult == mult and p.rawnerf_eps == eps, name
        assert len(p.itof_frequency_phase_shifts) <= rc_ext.RC_ITOF_MAX_PAIRS
        assert not hasattr(p, "exposure_time")
    m = config.transient_data_loss_preset("mse")
    assert m == dataclasses.replace(d, loss_type="mse")
    with pytest.raises(KeyError):
        config.transient_data_loss_preset("nope")
    assert rc_ext.TRANSIENT_LOSS_TYPES[0] == d.loss_type and len(rc_ext.TRANSIENT_LOSS_TYPES) == rc_ext.RC_TLOSS_COUNT == 8


def test_binding_struct_of_a_preset():
    ck = rc_ext.transient_data_loss_kind_c(config.transient_data_loss_preset("house_itof"))
    assert ck.loss_type == 6 and ck.use_itof == 1 and ck.n_pairs == 4
    assert list(ck.frequency)[:4] == [3e7, 3e7, 1.7e8, 1.7e8] and ck.phase_shift[1] == 3.14159265359
    assert ck.base.mult == pytest.approx(0.1) and ck.base.eps == pytest.approx(0.1)
    with pytest.raises(ValueError):
        rc_ext.transient_data_loss_kind_c(dataclasses.replace(TransientDataLossConfig(), itof_frequency_phase_shifts=((1e8, 0.0),) * 9))


def test_host_table_builder(tmp_path):
    """rc_itof_host.h (the table the kernels read) compiled for the CPU: row order, the constant row, and every entry the
    float32 rounding of the fp64 restatement's (1 ulp: the two evaluate 2 pi f t_b in different orders)."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pairs = ((75000000.0, 0.0), (425000000.0, 3.14159265359), (1e8, 0.7))
    e = float(np.float32(0.01))
    src = ('#include <stdio.h>\n#include "rc_itof_host.h"\nint main() {\n'
           f'  const double f[] = {{{", ".join(repr(p[0]) for p in pairs)}}}, ph[] = {{{", ".join(repr(p[1]) for p in pairs)}}};\n'
           f'  const std::vector<float> w = rc_itof_table(700, {e!r}, {len(pairs)}, f, ph);\n'
           '  printf("%zu\\n", w.size());\n  for (float v : w) printf("%.9g\\n", v);\n  return 0;\n}\n')
    (tmp_path / "t.cpp").write_text(src)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "neural-radiance-caching_amd", "csrc"),
                    str(tmp_path / "t.cpp"), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()
    assert int(out[0]) == (2 * len(pairs) + 1) * 700
    got = np.array(out[1:], np.float32).reshape(2 * len(pairs) + 1, 700)
    want = kref.itof_table(700, pairs, e, torch.float64).numpy()
    assert np.all(got[-1] == 0.5)
    assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -22         # values in [0, 2]: an ulp is at most 2^-23 x 2
    assert np.abs(got[0] - (np.cos(2 * np.pi * pairs[0][0] * np.arange(700) * e / kref.C_LIGHT) + 1)).max() < 1e-6
