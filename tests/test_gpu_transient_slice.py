"""rc_render_transient_slices on the GPU: the time slices  w * v[ceil t] + (1 - w) * v[floor t]  of the
time-resolved cache, computed without the histograms, against the fp32 oracle, the fp64 goldens and the full render.

Tolerances are the project's own for per-bin radiance (O(1e-2)): 2e-5 absolute against the fp32 oracle
(test_gpu_parity.test_transient_render_vs_oracle_fp32), 5e-5 against the fp64 goldens; the slice and the full render are
each within 2e-5 of the oracle, hence within 4e-5 of each other.  The expected slice is always formed in float64."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import common
import nrc_amd

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TIMES = (0.0, 36.5, 167.0, 167.25, 400.75, 686.5, 699.0)
OUTS = ("rgb", "direct", "indirect")
REF_KEY = {"rgb": "rgb", "direct": "transient_direct_viz", "indirect": "transient_indirect_viz"}
INVALID_ARG, UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def rc_transient():
    from nrc_amd import rc_ext
    h = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    h.load_weights(common.weights_transient_np())
    return h


@functools.lru_cache(maxsize=None)
def _oracle(n, jitter_seed=None):
    """The oracle's three histograms of a batch, computed once and shared (read-only)."""
    r = common.oracle_transient(n, jitter_seed)["render"]
    out = {k: r[v].numpy() for k, v in REF_KEY.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def _expected(hist, times):
    """w * hist[:, ceil t] + (1 - w) * hist[:, floor t] in float64 -> [n, len(times), 3]"""
    h = np.asarray(hist, dtype=np.float64)
    cols = []
    for t in times:
        lo, hi = int(np.floor(t)), int(np.ceil(t))
        w = t - lo
        cols.append(w * h[:, hi] + (1.0 - w) * h[:, lo])
    return np.stack(cols, axis=1)


def _inputs(n, jitter_seed=None, first=0):
    rays = nrc_amd.synthetic_transient_rays(n)
    f = {k: np.asarray(v)[first:] for k, v in rays.hot_fields().items()}
    rnd = None if jitter_seed is None else {"jitter": [j[first:] for j in common.jitters(n, seed=jitter_seed)]}
    return f, rnd


def _slices(h, f, rnd, times=TIMES, outputs=OUTS, **kw):
    out = h.render_transient_slices(f, rnd, times, outputs=outputs, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _full(h, f, rnd, **kw):
    out = h.render_transient(f, rnd, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_slices(got, hists, times, tol, rows=None):
    for k in got:
        if k not in REF_KEY:
            continue
        exp = _expected(hists[REF_KEY[k]] if REF_KEY[k] in hists else hists[k], times)
        assert got[k].shape == exp.shape and got[k].dtype == np.float32, k
        d = np.abs(got[k] - exp)
        if rows is not None:
            d = d[rows]
        print(f"{k}: max |slice - expected| = {d.max():.3e} (bound {tol:.0e})")
        assert d.max() <= tol, k


# 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,jitter_seed", [(48, None), (37, 9)])
def test_slices_vs_oracle_fp32(rc_transient, n, jitter_seed):
    """rgb, direct and indirect at seven times (both ends of the axis, integral and fractional t, the peaks of the direct
    and the indirect part) against the fp32 oracle.  The reference is asserted to be worth comparing with: the direct part
    (non-zero in all 700 bins, peak next to bin 167) and rgb exceed 1e-3 in every slice, the indirect part (exactly zero
    below bin 72, peak next to bin 686) from t = 167 on, and the indirect slice at t = 36.5 is exactly zero -- on the
    device too.  n = 37 does not fill the last workgroup."""
    ref = _oracle(n, jitter_seed)
    exp = {k: _expected(ref[k], TIMES) for k in OUTS}
    for i, t in enumerate(TIMES):
        assert exp["direct"][:, i].max() > 1e-3 and exp["rgb"][:, i].max() > 1e-3, t
        assert exp["indirect"][:, i].max() > (1e-3 if t >= 167.0 else -1.0), t
    assert np.all(exp["indirect"][:, 1] == 0.0) and np.all(ref["indirect"][:, 36:38] == 0.0)
    got = _slices(rc_transient, *_inputs(n, jitter_seed))
    _check_slices(got, ref, TIMES, 2e-5)
    assert np.all(got["indirect"][:, 1] == 0.0)
    assert np.all(got["indirect"][:, 0] == 0.0)


# 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["transient_16_det.npz", "transient_16_jit.npz"])
def test_slices_vs_fp64_golden(rc_transient, name):
    g = dict(np.load(os.path.join(GOLD, name)))
    n, js = int(g["meta"][0]), int(g["meta"][1])
    got = _slices(rc_transient, *_inputs(n, None if js < 0 else js), outputs=("rgb",))
    _check_slices(got, {"rgb": g["render_rgb"]}, TIMES, 5e-5)


# 3 ------------------------------------------------------------------------------------------------------------------
def test_slices_vs_full_render_and_extras_bitwise(rc_transient):
    from nrc_amd import rc_ext
    n = 48
    f, rnd = _inputs(n, 9)
    full = _full(rc_transient, f, rnd)
    got = _slices(rc_transient, f, rnd, extra=rc_ext.TRANSIENT_SLICE_EXTRAS)
    _check_slices(got, full, TIMES, 4e-5)
    assert set(got) == set(OUTS) | set(rc_ext.TRANSIENT_SLICE_EXTRAS)
    for k in rc_ext.TRANSIENT_SLICE_EXTRAS:           # the same kernels on the same inputs
        assert got[k].shape == full[k].shape and np.array_equal(got[k], full[k]), k
    assert np.abs(full["acc"]).max() > 0


# 4 ------------------------------------------------------------------------------------------------------------------
def test_slices_keep_the_direct_spill_of_the_previous_ray(rc_transient):
    """The direct scatter of ray r - 1 beyond bin 700 lands at the start of ray r's histogram (render.py:447-475); the
    slice must carry it, and lose it where the ray has no predecessor in the batch."""
    n = 64
    ref = _oracle(n)
    sub = ref["direct"][1:, :100]
    r, b, _ = np.unravel_index(sub.argmax(), sub.shape)
    r += 1
    assert ref["direct"][r, b].max() > 0
    f, _ = _inputs(n)
    got = _slices(rc_transient, f, None, times=(float(b),))
    _check_slices(got, ref, (float(b),), 2e-5)
    part = {k: v[r:] for k, v in f.items()}
    got_part = _slices(rc_transient, part, None, times=(float(b),))
    _check_slices(got_part, _full(rc_transient, part, None, outputs=["rgb", "transient_direct_viz", "transient_indirect_viz"]),
                  (float(b),), 4e-5)


# 5 ------------------------------------------------------------------------------------------------------------------
def _raw_call(h, f, rnd, s, extra=None):
    """rc_render_transient_slices with a hand-made struct, through the binding's status check (raises RcError)."""
    r, held, n = h._rays_struct(f)
    cam = h._dev(f["cam_origins"]).reshape(-1, 3)
    rnd_p = None if rnd is None else C.byref(h._randoms(held, rnd["jitter"]))
    h._check(h.lib.rc_render_transient_slices(h._h, C.byref(r), cam.data_ptr(), n, rnd_p, None, C.byref(s),
                                              None if extra is None else C.byref(extra), h._stream()))
    torch.cuda.synchronize()
    return held


def test_single_ray_and_empty_batch(rc_transient):
    from nrc_amd import rc_ext
    got = _slices(rc_transient, *_inputs(1))
    _check_slices(got, _oracle(1), TIMES, 2e-5)
    f4, _ = _inputs(4)
    f0 = {k: v[:0] for k, v in f4.items()}
    poison = torch.full((3, 64), -123.25, device="cuda")
    s = rc_ext.rc_transient_slices(count=2, rgb=poison[0].data_ptr(), direct=poison[1].data_ptr(), indirect=poison[2].data_ptr())
    s.t[0], s.t[1] = 10.0, 20.5
    _raw_call(rc_transient, f0, None, s)
    assert bool((poison == -123.25).all())
    out = rc_transient.render_transient_slices(f0, None, TIMES)
    assert tuple(out["rgb"].shape) == (0, len(TIMES), 3)


# 6 ------------------------------------------------------------------------------------------------------------------
def test_slices_are_deterministic_and_independent_of_the_other_times(rc_transient):
    n = 37
    f, rnd = _inputs(n, 9)
    a = _slices(rc_transient, f, rnd)
    b = _slices(rc_transient, f, rnd)
    for k in OUTS:
        assert np.array_equal(a[k], b[k]), k
    both = _slices(rc_transient, f, rnd, times=(167.25, 400.75))
    one, two = _slices(rc_transient, f, rnd, times=(167.25,)), _slices(rc_transient, f, rnd, times=(400.75,))
    for k in OUTS:
        assert np.array_equal(both[k][:, 0], one[k][:, 0]) and np.array_equal(both[k][:, 1], two[k][:, 0]), k
        assert np.array_equal(both[k][:, 0], a[k][:, 3]) and np.array_equal(both[k][:, 1], a[k][:, 4]), k
    # more than RC_TSLICE_MAX times: several calls, the same values
    many = tuple(TIMES) + (1.5, 250.0, 500.5)
    c = _slices(rc_transient, f, rnd, times=many, outputs=("rgb",))
    assert c["rgb"].shape == (n, len(many), 3) and np.array_equal(c["rgb"][:, :len(TIMES)], a["rgb"])


# 7 ------------------------------------------------------------------------------------------------------------------
def test_slices_follow_freshly_loaded_heads():
    """rc_load_params_flat(RC_LAYOUT_TRANSIENT_HEADS) repacks the heads: the plain columns the slice kernel reads must be
    refreshed with the fragment stream of the full render (a stale copy keeps the slices where they were)."""
    import loss_cases as lc
    from nrc_amd import rc_ext
    h = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(), 0)
    h.load_weights(common.weights_transient_np())
    n = 48
    f, rnd = _inputs(n, 9)
    before = _slices(h, f, rnd)
    # every element of the two head layers scaled by 1 + 0.5 N(0, 1): the oracle's slices of this batch move by 8e-4 with it
    # (the 5 % of loss_cases.perturbed moves them by 6e-5 only)
    w2, rng = dict(common.weights_transient_np()), np.random.Generator(np.random.PCG64(5))
    for k in sorted(w2):
        if "transient_indirect_layer" in k or "output_rgba_layer" in k:
            w2[k] = (np.asarray(w2[k]) * (1.0 + 0.5 * rng.standard_normal(np.shape(w2[k])))).astype(np.float32)
    layout, total = h.transient_head_grad_layout()
    h.load_params_flat("transient_heads", lc.flat_from_layout(layout, total, w2))
    after = _slices(h, f, rnd)
    _check_slices(after, _full(h, f, rnd, outputs=["rgb", "transient_direct_viz", "transient_indirect_viz"]), TIMES, 4e-5)
    moved = max(np.abs(after[k] - before[k]).max() for k in ("rgb", "indirect"))
    print(f"slices moved by {moved:.3e} with the new heads")
    assert moved > 1e-4


# 8 ------------------------------------------------------------------------------------------------------------------
def test_slices_with_occlusions_vs_oracle():
    """The handle and inputs of test_gpu_parity.test_transient_occlusions_shadow_rays_vs_oracle (dense field, both jitters):
    the shadow rays only change what the shader writes.  Its bound for rgb: 5e-5 on the rays whose thresholded occlusion
    pattern (and their predecessor's, for the spill) agrees with the oracle's."""
    from nrc_amd import rc_ext
    n = 24
    h = rc_ext.RadianceCache(nrc_amd.cornell_transient_config(use_occlusions=True), 0)
    h.load_weights(common.weights_transient_np(False, 6.0))
    rays = nrc_amd.synthetic_transient_rays(n)
    rnd = {"jitter": common.jitters(n, seed=5), "shadow_jitter": common.shadow_jitters(n * 32, 13)}
    got = _slices(h, rays.hot_fields(), rnd)
    ref = common.oracle_transient(n, jitter_seed=5, occlusions=True, shadow_jitter_seed=13, density_shift=6.0)
    acc_ref = ref["shadow_acc"].numpy().reshape(-1)
    acc = h.workspace("sh_acc")[: n * 32]
    same = np.all(((acc > 0.9) == (acc_ref > 0.9)).reshape(n, 32), axis=1)
    assert same.mean() >= 0.9
    same[1:] &= same[:-1].copy()
    r = {k: v.numpy() for k, v in ref["render"].items()}
    _check_slices(got, r, TIMES, 5e-5, rows=same)
    _check_slices({"indirect": got["indirect"]}, r, TIMES, 5e-5)           # not touched by the shadows


# 9 ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(rc_transient):
    from nrc_amd import rc_ext
    n = 4
    f, _ = _inputs(n)
    buf = torch.zeros((3, n * rc_ext.RC_TSLICE_MAX * 3), device="cuda")

    def make(count=1, t=(5.0,), ptrs=(0, 1, 2)):
        s = rc_ext.rc_transient_slices(count=count)
        for i, v in enumerate(t):
            s.t[i] = v
        for i, k in enumerate(OUTS):
            if i in ptrs:
                setattr(s, k, buf[i].data_ptr())
        return s

    cases = [("count 0", make(count=0), None, INVALID_ARG), ("count 9", make(count=9), None, INVALID_ARG),
             ("t NaN", make(t=(float("nan"),)), None, INVALID_ARG), ("t < 0", make(t=(-0.5,)), None, INVALID_ARG),
             ("t > n_bins - 1", make(t=(699.5,)), None, INVALID_ARG),
             ("second t bad", make(count=2, t=(3.0, 700.0)), None, INVALID_ARG),
             ("no output", make(ptrs=()), None, INVALID_ARG)]
    hist = rc_ext.rc_transient_outputs()
    hist.ptr[rc_ext.TRANSIENT_OUTPUT_ID["rgb"]] = buf.data_ptr()
    cases.append(("histogram in extra", make(), hist, UNSUPPORTED))
    bin_sum = rc_ext.rc_transient_outputs()
    bin_sum.ptr[rc_ext.TRANSIENT_OUTPUT_ID["integrated_rgb"]] = buf.data_ptr()
    cases.append(("sum over bins in extra", make(), bin_sum, UNSUPPORTED))
    for what, s, extra, code in cases:
        with pytest.raises(rc_ext.RcError) as e:
            _raw_call(rc_transient, f, None, s, extra)
        assert e.value.code == code, what
        assert "rc_render_transient_slices" in str(e.value), what
    assert bool((buf == 0).all())                       # refused before anything was launched
    hot = common.make_rc()                              # a handle without rc_set_transient
    with pytest.raises(rc_ext.RcError) as e:
        _raw_call(hot, f, None, make())
    assert e.value.code == UNSUPPORTED
    with pytest.raises(ValueError):
        rc_transient.render_transient_slices(f, None, TIMES, outputs=("transient_direct_viz",))
    with pytest.raises(ValueError):
        rc_transient.render_transient_slices(f, None, TIMES, extra=("integrated_rgb",))
    got = _slices(rc_transient, f, None)
    _check_slices(got, _oracle(n), TIMES, 2e-5)


# 10 -----------------------------------------------------------------------------------------------------------------
H, W = 10, 12


def _model_and_cameras():
    from nrc_amd import model as M
    m = M.Model(nrc_amd.cornell_transient_config(), 0)
    m.load_variables(common.weights_transient_np())
    cams = []
    for dx, dy, dz in ((0.1, 0.2, 4.0), (-0.3, 0.1, 3.8), (0.25, -0.2, 4.2)):      # look down -z at the scene ball
        c2w = np.array([[1, 0, 0, dx], [0, 1, 0, dy], [0, 0, 1, dz]], np.float32)
        cams.append(nrc_amd.Camera(pixtocam=nrc_amd.get_pixtocam(14.0, W, H), camtoworld=c2w, light=None, near=2.0, far=6.0))
    return m, cams


def test_image_slices_follow_render_camera_chunk_by_chunk():
    """render_time_slices against render_camera's histograms sliced on the host, with the same chunking (4 chunks of 3
    rows: the spill follows the chunks) and the same key (every chunk draws render_camera's jitter)."""
    from nrc_amd import prng
    m, cams = _model_and_cameras()
    key = prng.PRNGKey(7)
    times = (36.5, 167.25, 686.5)
    for rng in (None, key):
        img = nrc_amd.render_camera(m, cams[0], H, W, rows_per_chunk=3, keys=("rgb",), rng=rng)["rgb"]
        assert img.shape == (H, W, 700, 3)
        got = nrc_amd.render_time_slices(m, cams[0], H, W, times, rows_per_chunk=3, rng=rng)
        assert set(got) == {"rgb"} and got["rgb"].shape == (H, W, len(times), 3)
        exp = _expected(img.reshape(H * W, 700, 3), times).reshape(H, W, len(times), 3)
        d = np.abs(got["rgb"] - exp).max()
        print(f"rng {'key' if rng is not None else 'none'}: max |image slice - render_camera slice| = {d:.3e}")
        assert d <= 4e-5
        assert exp.max() > 1e-3


def test_path_frames_take_the_trainers_time_per_frame(tmp_path):
    m, cams = _model_and_cameras()
    frames, times = nrc_amd.render_time_slice_path(m, cams, H, W, start_idx=100, end_idx=400, rows_per_chunk=3)
    assert frames.shape == (3, H, W, 3) and np.array_equal(times, nrc_amd.path_times(3, 100, 400))
    assert np.array_equal(times, [100.0, 200.0, 300.0])
    for k, cam in enumerate(cams):
        img = nrc_amd.render_camera(m, cam, H, W, rows_per_chunk=3, keys=("rgb",))["rgb"]
        exp = _expected(img.reshape(H * W, 700, 3), (times[k],)).reshape(H, W, 3)
        assert np.abs(frames[k] - exp).max() <= 4e-5, k
        assert exp.max() > 1e-3
    other = _expected(img.reshape(H * W, 700, 3), (times[0],)).reshape(H, W, 3)       # the last camera at the first t
    assert np.abs(frames[2] - other).max() > 1e-4                                      # t really is per frame
    paths = nrc_amd.save_time_slice(frames[1], str(tmp_path), 1)
    assert np.array_equal(np.load(paths["npy"]), frames[1]) and os.path.exists(paths["png"])
