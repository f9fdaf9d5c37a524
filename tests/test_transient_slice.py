"""The host side of the time slices (nrc_amd.timeslice, no GPU): the weights of a fractional bin index, the t of the frames
of a path as the trainer sets them (engine/trainer.py:1693-1726), and the files a frame is saved to."""
import os

import numpy as np
import pytest

import nrc_amd
from nrc_amd import timeslice


@pytest.mark.parametrize("t,expect", [(0.0, (0, 0, 0.0)), (699.0, (699, 699, 0.0)), (167.0, (167, 167, 0.0)),
                                      (36.5, (36, 37, 0.5)), (167.25, (167, 168, 0.25)), (698.75, (698, 699, 0.75))])
def test_slice_weights(t, expect):
    lo, hi, w = timeslice.slice_weights(t)
    assert (lo, hi) == expect[:2] and isinstance(lo, int) and isinstance(hi, int)
    assert w == expect[2]                      # these fractions are exact in binary
    # the trainer's own three lines
    assert (lo, hi, w) == (int(np.floor(t)), int(np.ceil(t)), t - int(np.floor(t)))


def test_slice_weights_general_fraction_and_refusal():
    lo, hi, w = timeslice.slice_weights(400.7)
    assert (lo, hi) == (400, 401) and w == 400.7 - 400 and 0.0 < w < 1.0
    with pytest.raises(ValueError):
        timeslice.slice_weights(float("nan"))


@pytest.mark.parametrize("num,start,end", [(1, 0, 699), (3, 0, 699), (120, 40, 600), (7, 100.5, 20)])
def test_path_times_is_the_trainers_formula(num, start, end):
    t = timeslice.path_times(num, start, end)
    assert t.shape == (num,) and t.dtype == np.float64
    for k in range(num):
        frac = k / float(num)                  # (step - init_step) / float(total_steps)
        assert t[k] == start + frac * (end - start)
    assert t[0] == start
    assert abs(t[-1] - end) == pytest.approx(abs(end - start) / num, rel=1e-12)           # one step short of the end
    with pytest.raises(ValueError):
        timeslice.path_times(0, 0, 1)


def test_save_time_slice_writes_the_trainers_files(tmp_path):
    from PIL import Image
    rng = np.random.Generator(np.random.PCG64(3))
    frame = rng.uniform(-0.2, 1.3, size=(5, 7, 3)).astype(np.float32)
    frame[0, 0] = np.nan
    paths = timeslice.save_time_slice(frame, str(tmp_path), 12)
    assert paths == {"png": os.path.join(str(tmp_path), "cache_time_slice", "0012.png"),
                     "npy": os.path.join(str(tmp_path), "cache_time_slice", "0012.npy")}
    assert sorted(os.listdir(tmp_path / "cache_time_slice")) == ["0012.npy", "0012.png"]
    back = np.load(paths["npy"])
    assert back.dtype == np.float32 and np.array_equal(back, frame, equal_nan=True)
    png = np.asarray(Image.open(paths["png"]))
    assert png.shape == (5, 7, 3) and png.dtype == np.uint8
    assert np.array_equal(png, (np.clip(np.nan_to_num(frame), 0.0, 1.0) * 255.0).astype(np.uint8))      # utils.save_img_u8
    with pytest.raises(ValueError):
        timeslice.save_time_slice(frame[..., :2], str(tmp_path), 0)


def test_package_exports_the_module():
    for name in ("slice_weights", "path_times", "render_time_slices", "render_time_slice_path", "save_time_slice"):
        assert getattr(nrc_amd, name) is getattr(timeslice, name)
