"""rc_eval_shift_invariant on the GPU against the fp64 restatement of tests/eval_si_ref.py.

Scalars and maps: loss_cases.check, 3 x the fp32 restatement's own distance from fp64 plus 1e-6 of the quantity's scale.
Picks: equal to the fp64 restatement's at every pixel whose fp64 margin between the best and the runner-up pooled value
is exactly 0 (a tie: the later shift) or at least tau = 4 x the largest distance between the fp32 and the fp64 pooled
stacks of the case; pixels in between are left out, at most 1 % of a case.

Every kernel works on 32 x 32 tiles (k_si_metric's mse form on 256 pixels in row order): the shapes hold a window larger
than the image, one tile, seams crossed by one pixel along H and along W (33 x 33, 43 x 33), and several tiles."""
import ctypes

import numpy as np
import pytest
import torch

import common
import eval_metrics_ref as ref
import eval_si_ref as si
import loss_cases as lc
import nrc_amd
from nrc_amd import metrics, rc_ext
from nrc_amd import model as M
from test_gpu_eval_metrics import _mask, _two_cameras, _ws_ptr

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = -1, -5

# name: (H, W, (ri, rj), hw, images)
CASES = {
    "11x11": (11, 11, (4, 4), 8, "planted"),
    "12x45": (12, 45, (4, 4), 8, "planted"),
    "43x33": (43, 33, (4, 4), 8, "planted"),
    "64x96": (64, 96, (4, 4), 8, "planted"),
    "64x96-independent": (64, 96, (4, 4), 8, "independent"),
    "23x37": (23, 37, (1, 2), 1, "planted"),
    "17x19-mirror-ties": (17, 19, (0, 3), 0, "independent"),
    "40x72": (40, 72, (2, 2), 3, "planted"),
    "11x11-wide": (11, 11, (8, 8), 2, "planted"),
    "13x12-constants": (13, 12, (2, 3), 2, "constants"),
    "12x45-degenerate": (12, 45, (0, 0), 0, "planted"),
    "33x33-seams": (33, 33, (1, 1), 2, "planted"),
}
_REFS = {}


@pytest.fixture(scope="module")
def rc():
    return rc_ext.RadianceCache(nrc_amd.hotdog_config(), 0)          # the call needs no weights


def _case(name):
    """(pred, gt, radii, hw, fp64 restatement, fp32 restatement), computed once per case and left unchanged."""
    if name not in _REFS:
        h, w, radii, hw, kind = CASES[name]
        if kind == "planted":
            pred, gt = si.planted(h, w, seed=h * 100 + w)
        elif kind == "independent":
            pred, gt = si.independent(h, w, seed=h * 100 + w)
        else:
            pred, gt = np.full((h, w, 3), 0.5, np.float32), np.full((h, w, 3), 0.25, np.float32)
        _REFS[name] = (pred, gt, radii, hw, si.evaluate(pred, gt, radii, hw, dtype=np.float64),
                       si.evaluate(pred, gt, radii, hw, dtype=np.float32))
    return _REFS[name]


def _scalars(got, r64, r32, what, keys=("mse", "psnr", "ssim")):
    for k in keys:
        print(f"{what} {k}: got {got[k]!r} fp64 {r64[k]!r} |got - fp64| {abs(got[k] - r64[k]):.3e} "
              f"|fp32 - fp64| {abs(r32[k] - r64[k]):.3e}")
        lc.check(np.float64(got[k]), np.float64(r64[k]), np.float64(r32[k]), f"{what} {k}")


def _compared(s64, s32, kind, what):
    """The pixels whose picks are compared: fp64 margin exactly 0 or at least tau; at most 1 % are left out."""
    tau = 4.0 * float(np.abs(s32["pooled"].astype(np.float64) - s64["pooled"]).max())
    margin = si.margins(s64["pooled"], kind)
    keep = (margin == 0) | (margin >= tau)
    print(f"{what} {kind}: tau {tau:.3e}, smallest non-zero margin {margin[margin > 0].min() if (margin > 0).any() else 0:.3e}, "
          f"exact ties {(margin == 0).mean():.3f}, left out {1 - keep.mean():.4f}")
    assert 1.0 - keep.mean() <= 0.01, (what, kind, 1.0 - keep.mean())
    return keep


@pytest.mark.parametrize("name", list(CASES))
def test_scores_picks_and_maps_vs_fp64(rc, name):
    pred, gt, radii, hw, r64, r32 = _case(name)
    got = rc.eval_shift_invariant(pred, gt, radii, hw, keep_maps=True)
    for kind in ("mse", "ssim"):
        s64, s32 = r64[kind + "_search"], r32[kind + "_search"]
        keep = _compared(s64, s32, kind, name)
        di, dj = got[kind + "_di"].cpu().numpy(), got[kind + "_dj"].cpu().numpy()
        bad = keep & ((di != s64["opt_di"]) | (dj != s64["opt_dj"]))
        assert not bad.any(), (name, kind, int(bad.sum()), np.argwhere(bad)[:4])
        g = got[kind + "_map"].cpu().numpy()
        print(f"{name} {kind}_map: max|got - fp64| {np.abs(g - s64['opt_metric'])[keep].max():.3e} "
              f"max|fp32 - fp64| {np.abs(s32['opt_metric'] - s64['opt_metric'])[keep].max():.3e}")
        lc.check(g[keep], s64["opt_metric"][keep], s32["opt_metric"][keep].astype(np.float64), f"{name} {kind}_map")
    _scalars(got, r64, r32, name)


def test_constants_and_mirror_ties_go_to_the_later_shift(rc):
    pred, gt, radii, hw, r64, _ = _case("13x12-constants")
    got = rc.eval_shift_invariant(pred, gt, radii, hw, keep_maps=True)
    for k, want in (("mse_di", 2), ("mse_dj", 3), ("ssim_di", 2), ("ssim_dj", 3)):
        assert torch.all(got[k] == want), k
    pred, gt, radii, hw, r64, _ = _case("17x19-mirror-ties")
    tied = si.margins(r64["mse_search"]["pooled"], "mse") == 0
    assert tied.mean() > 0.08
    got = rc.eval_shift_invariant(pred, gt, radii, hw, keep_maps=True)
    assert np.array_equal(got["mse_dj"].cpu().numpy()[tied], r64["mse_search"]["opt_dj"][tied])


def test_degenerate_search_is_the_plain_metric(rc):
    pred, gt, radii, hw, r64, r32 = _case("12x45-degenerate")
    got = rc.eval_shift_invariant(pred, gt, radii, hw, keep_maps=True)
    plain = rc.eval_image(pred, gt, skip_postprocess=True)
    p64, p32 = ref.both(pred, gt, skip_postprocess=True)
    lc.check(np.float64(got["mse"]), np.float64(p64["mse"]), np.float64(p32["mse"]), "mse = plain mse")
    assert abs(got["psnr"] - plain["psnr"]) < 1e-4
    assert not got["mse_di"].any() and not got["ssim_dj"].any()


def test_two_calls_are_bitwise_equal(rc):
    pred, gt, radii, hw, _, _ = _case("43x33")
    a = rc.eval_shift_invariant(pred, gt, radii, hw, keep_maps=True, sync=False)
    b = rc.eval_shift_invariant(pred, gt, radii, hw, keep_maps=True, sync=False)
    assert torch.equal(a["result"].view(torch.int64), b["result"].view(torch.int64))
    for k in ("mse_map", "ssim_map", "mse_di", "mse_dj", "ssim_di", "ssim_dj"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def _same(a, b):
    return a == pytest.approx(b, rel=0, abs=0, nan_ok=True)


def test_stream_workspace_reuse_and_no_ssim(rc):
    big, small = _case("64x96")[:4], _case("23x37")[:4]
    want_big, want_small = rc.eval_shift_invariant(*big), rc.eval_shift_invariant(*small)
    s = torch.cuda.Stream()
    dev = [torch.from_numpy(x).cuda() for x in small[:2]]
    s.wait_stream(torch.cuda.current_stream())
    assert _same(rc.eval_shift_invariant(*dev, *small[2:], stream_handle=s.cuda_stream), want_small)
    with torch.cuda.stream(s):
        assert _same(rc.eval_shift_invariant(*dev, *small[2:]), want_small)
    torch.cuda.current_stream().wait_stream(s)
    ptrs = [_ws_ptr(rc, "ev:" + k) for k in ("si_metric", "si_state", "si_part")]
    assert _same(rc.eval_shift_invariant(*big), want_big)
    assert ptrs == [_ws_ptr(rc, "ev:" + k) for k in ("si_metric", "si_state", "si_part")]     # the smaller case reallocated nothing
    # rc_eval_image shares the "ev:" set: it is unharmed in between
    plain = rc.eval_image(*small[:2], skip_postprocess=True)
    assert _same(rc.eval_shift_invariant(*small), want_small) and _same(rc.eval_image(*small[:2], skip_postprocess=True), plain)
    mse_only = rc.eval_shift_invariant(*small, ssim=False, keep_maps=True)
    assert np.isnan(mse_only["ssim"]) and mse_only["mse"] == want_small["mse"] and mse_only["psnr"] == want_small["psnr"]
    assert "ssim_map" not in mse_only and "mse_di" in mse_only


def _raw(rc, p, g, radii, hw, want_ssim=1, out=True, **ptrs):
    """The C call itself on the device tensors p, g -> (status, result tensor); ptrs: struct fields set afterwards."""
    H, W = p.shape[:2]
    im = rc_ext.rc_eval_si_images(pred=p.data_ptr(), gt=g.data_ptr(), height=H, width=W, radius_i=radii[0], radius_j=radii[1],
                                  window_halfwidth=hw, want_ssim=want_ssim)
    for k, v in ptrs.items():
        setattr(im, k, v)
    res = torch.full((rc_ext.RC_EVAL_SI_COUNT,), -7.0, dtype=torch.float64, device="cuda:0")
    code = rc.lib.rc_eval_shift_invariant(rc._h, ctypes.byref(im), res.data_ptr() if out else None, rc._stream())
    torch.cuda.synchronize()
    return code, res


def test_only_the_requested_maps_are_written(rc):
    pred, gt, radii, hw, _, _ = _case("23x37")
    full = rc.eval_shift_invariant(pred, gt, radii, hw, keep_maps=True)
    dp, dg = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    n, guard = 23 * 37, 64
    names = ("mse_map", "ssim_map", "mse_di", "mse_dj", "ssim_di", "ssim_dj")
    for asked in (("mse_map", "ssim_dj"), ("ssim_map", "mse_di"), ("mse_dj", "ssim_di"), ()):
        bufs = {k: torch.full((n + 2 * guard,), -12345, dtype=torch.float32 if k.endswith("map") else torch.int32, device="cuda:0")
                for k in names}
        code, res = _raw(rc, dp, dg, radii, hw, **{k: bufs[k][guard:].data_ptr() for k in asked})
        assert code == 0, (asked, code)
        assert res[0].item() == full["mse"] and res[2].item() == full["ssim"]
        for k in names:
            b = bufs[k]
            assert torch.all(b[:guard] == -12345) and torch.all(b[guard + n:] == -12345), (asked, k)
            if k in asked:
                assert torch.equal(b[guard: guard + n].view(23, 37).view(torch.int32), full[k].view(torch.int32)), (asked, k)
            else:
                assert torch.all(b == -12345), (asked, k)
    # want_ssim = 0: the ssim buffers stay as they were even when given
    bufs = {k: torch.full((n,), -12345, dtype=torch.float32 if k.endswith("map") else torch.int32, device="cuda:0") for k in names}
    code, res = _raw(rc, dp, dg, radii, hw, want_ssim=0, **{k: v.data_ptr() for k, v in bufs.items()})
    assert code == 0 and torch.isnan(res[2]) and res[0].item() == full["mse"]
    assert all(torch.all(bufs[k] == -12345) for k in names if k.startswith("ssim"))
    assert torch.equal(bufs["mse_dj"].view(23, 37), full["mse_dj"])


def test_refusals_leave_the_handle_usable(rc):
    pred, gt, radii, hw, _, _ = _case("23x37")
    want = rc.eval_shift_invariant(pred, gt, radii, hw)
    dp, dg = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    small_h, small_w = dp[:10].contiguous(), dp[:, :10].contiguous()
    p11 = dp[:11, :12].contiguous()
    top_r, top_hw = rc_ext.RC_EVAL_SI_MAX_RADIUS, rc_ext.RC_EVAL_SI_MAX_HALFWIDTH
    assert top_r >= 8 and top_hw >= 16
    cases = [
        ("pred", lambda: _raw(rc, dp, dg, radii, hw, pred=None), INVALID_ARG),
        ("gt", lambda: _raw(rc, dp, dg, radii, hw, gt=None), INVALID_ARG),
        ("out", lambda: _raw(rc, dp, dg, radii, hw, out=False), INVALID_ARG),
        ("height", lambda: _raw(rc, small_h, small_h, radii, hw), INVALID_ARG),
        ("width", lambda: _raw(rc, small_w, small_w, radii, hw), INVALID_ARG),
        ("radius_i < 0", lambda: _raw(rc, dp, dg, (-1, 2), hw), INVALID_ARG),
        ("radius_j < 0", lambda: _raw(rc, dp, dg, (1, -2), hw), INVALID_ARG),
        ("halfwidth < 0", lambda: _raw(rc, dp, dg, radii, -1), INVALID_ARG),
        ("radius_i >= H", lambda: _raw(rc, p11, p11, (11, 1), hw), INVALID_ARG),
        ("radius_j >= W", lambda: _raw(rc, p11, p11, (1, 12), hw), INVALID_ARG),
        ("radius_i above the cap", lambda: _raw(rc, dp, dg, (top_r + 1, 1), hw), UNSUPPORTED),
        ("radius_j above the cap", lambda: _raw(rc, dp, dg, (1, top_r + 1), hw), UNSUPPORTED),
        ("halfwidth above the cap", lambda: _raw(rc, dp, dg, radii, top_hw + 1), UNSUPPORTED),
    ]
    for what, call, code in cases:
        got, res = call()
        assert got == code, (what, got)
        assert torch.all(res == -7.0), what                          # nothing was written
        assert _same(rc.eval_shift_invariant(pred, gt, radii, hw), want), what
    code, _ = _raw(rc, dp, dg, (top_r, top_r), top_hw)               # the caps themselves are served
    assert code == 0
    with pytest.raises(rc_ext.RcError) as e:
        rc.eval_shift_invariant(pred, gt, (top_r + 1, 1), hw)
    assert e.value.code == UNSUPPORTED and "radius" in str(e.value)
    with pytest.raises(ValueError):
        rc.eval_shift_invariant(pred, gt[:, :12].copy(), radii, hw)  # the binding: gt of another size
    with pytest.raises(ValueError, match="search_radii"):
        rc.eval_shift_invariant(pred, gt, 4, hw)


def test_harness_and_functions_vs_restatement(rc):
    pred, gt, radii, hw, r64, r32 = _case("23x37")
    p64, p32 = ref.both(pred, gt, skip_postprocess=True)
    suffix = "_(1,_2)_1"
    h = metrics.SearchInvariantHarness(rc, search_radii=radii, window_halfwidth=hw)(pred, gt, name_fn=lambda s: "test_" + s)
    assert list(h) == ["test_psnr", "test_ssim", "test_psnr_si" + suffix, "test_ssim_si" + suffix]
    _scalars({"psnr": h["test_psnr"], "ssim": h["test_ssim"]}, p64, p32, "harness plain", keys=("psnr", "ssim"))
    _scalars({"psnr": h["test_psnr_si" + suffix], "ssim": h["test_ssim_si" + suffix]}, r64, r32, "harness si", keys=("psnr", "ssim"))
    assert h["test_psnr_si" + suffix] > h["test_psnr"]
    lean = metrics.SearchInvariantHarness(rc, disable_ssim=True, search_radii=radii, window_halfwidth=hw)(pred, gt)
    assert list(lean) == ["psnr", "psnr_si" + suffix] and lean["psnr_si" + suffix] == h["test_psnr_si" + suffix]
    assert list(metrics.SearchInvariantHarness(rc)(pred, gt)) == ["psnr", "ssim", "psnr_si_(4,_4)_8", "ssim_si_(4,_4)_8"]
    for kind, fn in (("mse", metrics.shift_invariant_mse), ("ssim", metrics.shift_invariant_ssim)):
        score, di, dj = fn(rc, pred, gt, radii, hw)
        s64, s32 = r64[kind + "_search"], r32[kind + "_search"]
        lc.check(np.float64(score), np.float64(s64["score"]), np.float64(s32["score"]), kind + " score")
        keep = _compared(s64, s32, kind, "functions")
        assert di.dtype == torch.int32 and tuple(di.shape) == (23, 37)
        assert np.array_equal(di.cpu().numpy()[keep], s64["opt_di"][keep]) and np.array_equal(dj.cpu().numpy()[keep], s64["opt_dj"][keep])


def test_evaluate_view_adds_the_two_keys():
    """The 24 x 20 DeviceDataset view of test_gpu_eval_metrics.test_evaluate_view_end_to_end."""
    H, W = 24, 20
    cfg = nrc_amd.hotdog_config(render_chunk_size=128)
    m = M.Model(cfg, 0)
    m.load_variables(common.weights_np())
    p2c, c2w = _two_cameras(H, W, 4.0)
    blank = nrc_amd.DeviceDataset(m.rc, p2c, c2w, np.zeros((2, H, W, 3), np.float32), near=2.0, far=6.0)
    fn = M.bind_render_fn(M.create_render_fn(m))
    rays = blank.generate_ray_batch(1).rays.tree_map(lambda t: t.cpu().numpy())
    img = M.render_image(fn, None, rays, cfg, ("cache",), verbose=False)[0]
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    delta = (0.05 * np.sin(0.7 * xx + 0.4 * yy))[..., None] * np.array([1.0, -1.0, 0.5])
    images = np.stack([np.zeros((H, W, 3)), np.clip(img["rgb"] + delta, 0.0, None)]).astype(np.float32)
    ds = nrc_amd.DeviceDataset(m.rc, p2c, c2w, images, near=2.0, far=6.0)
    mask = _mask(H, W)
    plain = metrics.evaluate_view(m, ds, 1, masks=mask, exposure=0.9)
    got = metrics.evaluate_view(m, ds, 1, masks=mask, exposure=0.9, search_invariant=((1, 1), 2))
    new = {"psnr_si_(1,_1)_2", "ssim_si_(1,_1)_2"}
    assert set(got) == set(plain) | new
    for k in plain:
        if k != "rays_per_sec":                                    # a timing, not a score
            assert _same(got[k], plain[k]), k
    kept = m.rc.eval_image(img["rgb"], images[1], mask=mask, exposure=0.9, keep_images=True)
    direct = m.rc.eval_shift_invariant(kept["post_pred"], kept["post_gt"], (1, 1), 2)
    assert got["psnr_si_(1,_1)_2"] == direct["psnr"] and got["ssim_si_(1,_1)_2"] == direct["ssim"]
    r64 = si.evaluate(kept["post_pred"].cpu().numpy(), kept["post_gt"].cpu().numpy(), (1, 1), 2)
    r32 = si.evaluate(kept["post_pred"].cpu().numpy(), kept["post_gt"].cpu().numpy(), (1, 1), 2, dtype=np.float32)
    _scalars(direct, r64, r32, "evaluate_view")
