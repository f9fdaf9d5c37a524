"""The numpy restatement of the shift-invariant metrics (tests/eval_si_ref.py) pinned against things other than itself:
the reference's literal pad / roll / crop, scipy's box filter and a four-loop sum, the degenerate search, a planted shift,
the tie rules; and the Python layer's keys, exports and refusals.  No GPU."""
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import eval_metrics_ref as ref
import eval_si_ref as si

DTYPES = [np.float64, np.float32]
PLANTED = [(11, 11), (12, 45), (43, 33), (23, 37), (40, 72)]


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def test_index_form_is_pad_roll_crop():
    """image_utils.py:119-133 written out with numpy, for every shift of (2, 3)."""
    ri, rj = 2, 3
    im0 = _rng(1).uniform(size=(7, 9, 3))
    pad = np.pad(im0, [[ri] * 2, [rj] * 2, (0, 0)], "reflect")
    for di in range(-ri, ri + 1):
        for dj in range(-rj, rj + 1):
            rolled = np.roll(np.roll(pad, -di, 0), -dj, 1)
            crop = rolled[ri: rolled.shape[0] - ri, rj: rolled.shape[1] - rj, :]
            assert np.array_equal(crop, si.shifted(im0, di, dj)), (di, dj)


def test_ssim_padding_is_np_pad_reflect():
    z = _rng(2).uniform(size=(11, 13, 3))
    assert np.array_equal(si.pad_reflect(z), np.pad(z, [[5] * 2, [5] * 2, [0] * 2], mode="reflect"))


@pytest.mark.parametrize("hw", [0, 1, 2, 8])
def test_pooling_against_scipy_uniform_filter(hw):
    m = _rng(3).uniform(size=(13, 17))
    want = ndimage.uniform_filter(m, size=2 * hw + 1, mode="constant", cval=0.0)
    assert np.abs(si.pool(m, hw) - want).max() < 1e-14


def test_pooling_against_four_loops():
    m, hw = _rng(4).uniform(size=(5, 6)), 2
    want = np.zeros_like(m)
    for y in range(5):
        for x in range(6):
            for i in range(-hw, hw + 1):
                for j in range(-hw, hw + 1):
                    if 0 <= y + i < 5 and 0 <= x + j < 6:
                        want[y, x] += m[y + i, x + j]
    assert np.abs(si.pool(m, hw) - want / 25.0).max() < 1e-15
    assert si.pool(m.astype(np.float32), hw, np.float32).dtype == np.float32


def test_degenerate_search_is_the_plain_metric():
    a, b = si.independent(12, 45, seed=5)
    r = si.evaluate(a, b, (0, 0), 0)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    assert abs(r["mse"] - ((a64 - b64) ** 2).mean()) < 1e-15
    smap = ref.ssim(np.pad(a64, [[5] * 2, [5] * 2, [0] * 2], mode="reflect"), np.pad(b64, [[5] * 2, [5] * 2, [0] * 2], mode="reflect"))[1]
    assert smap.shape == (12, 45, 3)
    assert abs(r["ssim"] - smap.mean(-1)[5:-5, 5:-5].mean()) < 1e-15
    assert not r["mse_search"]["opt_di"].any() and not r["ssim_search"]["opt_dj"].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h,w", PLANTED)
def test_planted_shift_is_found(h, w, dtype):
    pred, gt = si.planted(h, w, seed=h * 100 + w)
    r = si.evaluate(pred, gt, (4, 4), 8, dtype=dtype)
    for kind in ("mse_search", "ssim_search"):
        s = r[kind]
        hit = (s["opt_di"] == -1) & (s["opt_dj"] == 2)
        assert hit.mean() >= 0.9, (kind, hit.mean())
    plain = ref.mse_to_psnr(((pred.astype(np.float64) - gt) ** 2).mean())
    assert r["psnr"] > plain, (r["psnr"], plain)


@pytest.mark.parametrize("dtype", DTYPES)
def test_constant_images_pick_the_last_shift(dtype):
    """Every shift ties at every pixel: >= / <= hand the pixel to the later shift, down to the last one."""
    a, b = np.full((13, 12, 3), 0.5, np.float32), np.full((13, 12, 3), 0.25, np.float32)
    r = si.evaluate(a, b, (2, 3), 2, dtype=dtype)
    for kind in ("mse_search", "ssim_search"):
        assert np.all(r[kind]["opt_di"] == 2) and np.all(r[kind]["opt_dj"] == 3), kind
        assert not si.margins(r[kind]["pooled"], kind[:-7]).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_mirror_ties_go_to_the_later_shift(dtype):
    """(0, 3) with hw = 0: in the three columns next to the left and the right border two shifts can read the same column
    of pred (x + dj and its reflection), so their values tie exactly; where such a pair is the best value, the later
    shift must hold the pixel.  At x = 0 the pairs are (-d, +d): the pick is never negative there."""
    pred, gt = si.independent(17, 19, seed=6)
    s = si.search(pred, gt, "mse", (0, 3), 0, dtype)
    margin = si.margins(s["pooled"], "mse")
    tied = margin == 0
    assert 0.08 < tied.mean() < 6 / 19 and not tied[:, 3:-3].any(), tied.mean()
    assert tied[:, 0].any() and tied[:, -1].any()
    assert np.all(s["opt_dj"][:, 0] >= 0)                                          # never the mirror's earlier half
    best = s["pooled"].min(axis=0)
    for y, x in zip(*np.nonzero(tied)):
        last = max(i for i in range(7) if s["pooled"][i, y, x] == best[y, x])
        assert s["shifts"][last] == (0, int(s["opt_dj"][y, x]))


def test_keys_exports_and_binding():
    import nrc_amd
    from nrc_amd import metrics, rc_ext

    assert metrics.si_suffix((4, 4), 8) == "_(4,_4)_8"
    assert metrics.si_suffix([4, 4], 8) == "_(4,_4)_8"              # rendered as a tuple
    assert metrics.si_suffix((1, 2), 3) == "_(1,_2)_3"
    assert nrc_amd.SearchInvariantHarness is metrics.SearchInvariantHarness
    assert callable(metrics.shift_invariant_mse) and callable(metrics.shift_invariant_ssim)
    assert "rc_eval_shift_invariant" in rc_ext.EXPORTS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "rc_abi.h")).read()
    body = src[src.index("RC_EVAL_SI_MSE = 0"):src.index("} rc_eval_si_slot;")]
    enum = [e.lower() for e in re.findall(r"RC_EVAL_SI_([A-Z_0-9]+)", body) if e != "COUNT"]
    assert enum == list(rc_ext.EVAL_SI_SLOTS) and rc_ext.RC_EVAL_SI_COUNT == len(enum)
    caps = dict(re.findall(r"#define (RC_EVAL_SI_MAX_[A-Z]+) (\d+)", src))
    assert int(caps["RC_EVAL_SI_MAX_RADIUS"]) == rc_ext.RC_EVAL_SI_MAX_RADIUS >= 8
    assert int(caps["RC_EVAL_SI_MAX_HALFWIDTH"]) == rc_ext.RC_EVAL_SI_MAX_HALFWIDTH >= 16
    assert "search_invariant" in metrics.evaluate_view.__code__.co_varnames


def test_python_layer_refusals():
    from nrc_amd import metrics, rc_ext

    with pytest.raises(ValueError, match="RadianceCache"):
        metrics.SearchInvariantHarness(None)
    for bad in (4, (4,), (1, 2, 3), (1.5, 2), "ab"):
        with pytest.raises(ValueError, match="search_radii"):
            rc_ext.search_radii_pair(bad)
        with pytest.raises(ValueError, match="search_radii"):
            metrics.SearchInvariantHarness(object(), search_radii=bad)
    assert rc_ext.search_radii_pair([np.int64(2), 3]) == (2, 3)
    with pytest.raises(NotImplementedError, match="shift-invariant"):         # MetricHarness itself stays as it was
        metrics.MetricHarness(None, disable_search_invariant=False)
