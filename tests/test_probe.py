"""The numpy restatement of the surface probe (tests/probe_ref.py) against facts it does not compute itself, and the host
helpers of nrc_amd.probe against hand values (no GPU needed)."""
import math

import numpy as np
import pytest

import probe_ref as ref
from nrc_amd import probe

DTYPES = [np.float64, np.float32]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (7, 9), (64, 128)])
def test_directions_have_unit_norm(h, w, flip, dtype):
    d = ref.sphere_directions(h, w, flip, dtype)
    assert d.shape == (h * w, 3) and d.dtype == dtype
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=-1) - 1.0).max() <= (4e-7 if dtype == np.float32 else 1e-15)


def _closed_form(theta, phi, flip):
    if flip:
        return [-math.cos(theta), math.sin(theta) * math.cos(phi), math.sin(theta) * math.sin(phi)]
    return [math.sin(theta) * math.cos(phi), math.sin(theta) * math.sin(phi), math.cos(theta)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("h,w", [(3, 5), (7, 9), (256, 512)])
def test_corner_pixels_match_their_closed_forms(h, w, flip, dtype):
    """Pixel (0, 0): theta = pi / 2H, phi = pi - pi / W.  Pixel (H - 1, W - 1): theta = pi - pi / 2H, phi = -pi + pi / W."""
    d = ref.sphere_directions(h, w, flip, dtype).astype(np.float64).reshape(h, w, 3)
    tol = 2e-6 if dtype == np.float32 else 1e-14               # a few ulp of pi in the angle
    assert np.abs(d[0, 0] - _closed_form(math.pi / (2 * h), math.pi - math.pi / w, flip)).max() <= tol
    assert np.abs(d[-1, -1] - _closed_form(math.pi - math.pi / (2 * h), -math.pi + math.pi / w, flip)).max() <= tol
    # phi falls along a row and theta grows down the rows: x / y swapped or H / W swapped would show here
    theta, phi = ref.sphere_angles(h, w, dtype)
    assert theta.shape == (h,) and phi.shape == (w,) and np.all(np.diff(theta) > 0) and np.all(np.diff(phi) < 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("kappa", [1e-9, 1.0, 50.0])
def test_single_lobe_integrates_to_one(kappa, flip, dtype):
    """sum L sin(theta) dtheta dphi over a 64 x 128 panorama is 1 to the midpoint rule's own error.  The rule is exact to
    all orders along phi (periodic) and, along theta, its leading error is -(h^2 / 24) (F(0) + F(pi)) with F the density
    integrated over phi at the pole.  For the constant 1 / 4 pi, F = 1 / 2 at both poles; a lobe whose mean lies on the
    equator of the polar axis has a density of kappa / (4 pi sinh kappa) <= 1 / 4 pi there, so its error is at most the
    constant's.  That error is taken from the same sum of the constant; 5 % and 1e-5 are left for the next order and for
    8192 float32 roundings."""
    h, w = 64, 128
    theta, _ = ref.sphere_angles(h, w, np.float64)
    area = np.sin(theta)[:, None] * ((2.0 * np.pi / w) * (np.pi / h))
    e0 = abs(float((np.full((h, w), 1.0 / (4.0 * np.pi)) * area).sum()) - 1.0)
    assert 0.5e-4 < e0 < 2e-4                                  # h^2 / 24 with h = pi / 64
    mean = np.array([[0.0, 0.9, -1.7]]) if flip else np.array([[0.6, -2.1, 0.0]])      # raw length != 1, on the equator
    lin = ref.vmf_linear(mean, np.array([kappa]), np.array([0.3]), h, w, flip, dtype).astype(np.float64)
    err = abs(float((lin * area).sum()) - 1.0)
    print(f"kappa {kappa} flip {flip} {np.dtype(dtype).name}: |integral - 1| = {err:.3e}, the constant's {e0:.3e}")
    assert err <= 1.05 * e0 + 1e-5


@pytest.mark.parametrize("dtype", DTYPES)
def test_kappa_branch_and_zero_mean(dtype):
    """kappa <= FLT_EPSILON gives exactly 1 / 4 pi, whatever the mean; a zero-length mean passes max(|m|, 1e-5) without NaN
    and, being the zero vector, yields kappa / (4 pi sinh kappa) everywhere."""
    eps = float(np.finfo(np.float32).eps)
    h, w = 4, 6
    for kappa in (0.0, 1e-9, eps):
        lin = ref.vmf_linear(np.array([[0.3, 0.1, -2.0]]), np.array([kappa]), np.array([5.0]), h, w, False, dtype)
        assert np.all(lin == dtype(1) / (dtype(4) * ref._pi(dtype)))
    above = ref.vmf_linear(np.array([[0.0, 0.0, 1.0]]), np.array([2 * eps]), np.array([5.0]), h, w, False, np.float64)
    assert np.all(above != 1.0 / (4.0 * np.pi)) and np.abs(above * 4.0 * np.pi - 1.0).max() < 1e-6
    zero = ref.vmf_linear(np.zeros((1, 3)), np.array([7.0]), np.array([0.0]), h, w, False, dtype)
    assert np.all(np.isfinite(zero))
    assert np.abs(zero.astype(np.float64) - 7.0 / (4.0 * np.pi * math.sinh(7.0))).max() <= 1e-6 * 7.0 / (4.0 * np.pi * math.sinh(7.0))
    tiny = ref.lobe_table(np.array([[1e-7, 0.0, 0.0]]), np.array([1.0]), np.array([0.0]), dtype)[0]
    assert np.abs(tiny.astype(np.float64) - [1e-2, 0.0, 0.0]).max() <= 1e-8        # divided by 1e-5, not by its length


def test_both_safe_exp_clips():
    """The weights clip the logit at 70 (math.safe_exp), eval_vmf clips its exponent at 80 (inverse_render.math)."""
    m, k, wgt = ref.lobe_table(np.array([[1.0, 0, 0], [0, 1.0, 0]]), np.array([1.0, 1.0]), np.array([75.0, 70.0]))
    assert wgt[0] == wgt[1] == 0.5
    m, k, wgt = ref.lobe_table(np.array([[1.0, 0, 0], [0, 1.0, 0]]), np.array([1.0, 1.0]), np.array([69.0, 70.0]))
    assert wgt[0] == pytest.approx(1.0 / (1.0 + math.e))
    x = np.array([[[1.0, 0.0, 0.0]]])
    got = ref.eval_vmf(x, np.array([[1.0, 0.0, 0.0]]), np.array([85.0]))
    assert float(got[0, 0]) == pytest.approx(85.0 * math.exp(80.0) / (4.0 * math.pi * math.sinh(85.0)))


def test_eight_bit_step_and_srgb():
    lin = np.array([[[1.0 / (4.0 * np.pi)]]])
    srgb = ref.vis_ref.linear_to_srgb(lin)
    assert float(srgb.reshape(-1)[0] * 255) == pytest.approx(79.69, abs=5e-3)       # the constant of a kappa = 0 mixture
    assert ref.to_u8(np.array([0.5 / 255, 1.5 / 255, 2.0, -1.0, np.nan])).tolist() == [0, 2, 255, 0, 0]   # half to even


@pytest.mark.parametrize("dtype", DTYPES)
def test_position_and_broadcast_fields(dtype):
    view = dict(origins=np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0]]), directions=np.array([[0.0, 0.0, -2.0], [1.0, 0.0, 0.0]]),
                distance_median=np.array([1.5, 2.0]), normals=np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]),
                lights=np.array([[9.0, 8.0, 7.0], [1.0, 1.0, 1.0]]), up=np.array([[0.0, 0.0, 1.0]]))
    out, pos = ref.probe_rays(view, [1, 0], 2, 3, 0.05, 2.0, 0.4, False, dtype)
    assert np.allclose(pos, [[2.0, 0.0, 0.4], [1.0, 2.4, 0.0]], atol=1e-6)
    assert out["origins"].shape == (12, 3) and np.all(out["origins"][:6] == pos[0]) and np.all(out["origins"][6:] == pos[1])
    assert np.all(out["lights"] == [9.0, 8.0, 7.0]) and np.all(out["up"] == [0.0, 0.0, 1.0])      # rows 0
    assert np.all(out["look"] == [0.0, 0.0, -1.0])                                                # the cast's own
    assert np.all(out["near"] == dtype(0.05)) and np.all(out["far"] == 2.0)
    assert np.array_equal(out["directions"][:6], out["directions"][6:]) and np.array_equal(out["directions"], out["viewdirs"])
    # the radii are those of the panoramic direction: about the pixel's angular size on the unit sphere over sqrt(3),
    # sin(phi)-shortened along x
    radii, ip = ref.panoramic_radii(64, 128, dtype)
    mid = radii.reshape(64, 128)[32, 5]
    assert float(mid) == pytest.approx(0.5 * (2 * np.pi / 128 + np.pi / 64) * 2 / math.sqrt(12), rel=2e-3)
    assert ip.shape == (64 * 128, 2)


def test_default_pixel_panorama_size_and_mark_pixel():
    assert probe.default_pixel(800, 800) == (240, 480)
    assert probe.default_pixel(12, 16) == (5, 7)                # round(4.8) = 5, round(7.2) = 7
    assert probe.default_pixel(5, 15) == (4, 3)                 # np.round: 4.5 -> 4 (half to even), 3.0 -> 3
    assert probe.default_pixel(100, 200, vis_decimate=2) == (30, 30)
    assert probe.panorama_size(800, 800) == (256, 512)
    assert probe.panorama_size(100, 120) == (100, 240)
    assert probe.panorama_size(300, 400) == (256, 512)
    import torch
    img = torch.zeros((20, 30, 3))
    assert probe.mark_pixel(img, 12, 9) is img
    want = np.zeros((20, 30, 3), np.float32)
    want[4:14, 7:17] = [1.0, 0.0, 0.0]
    assert np.array_equal(img.numpy(), want)
    u8 = probe.mark_pixel(torch.full((20, 30, 3), 7, dtype=torch.uint8), 28, 18).numpy()
    assert u8[13:20, 23:30].reshape(-1, 3).tolist() == [[255, 0, 0]] * 49 and int((u8 != 7).any(-1).sum()) == 49
    # nearer than 5 to the top or left edge the reference's slice start is negative: nothing is marked
    assert float(probe.mark_pixel(torch.zeros((20, 30, 3)), 3, 9).abs().sum()) == 0.0
