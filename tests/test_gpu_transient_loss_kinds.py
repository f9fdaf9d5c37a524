"""rc_transient_data_backward_kind and rc_dtof_to_itof on the GPU against the fp64 restatement of
tests/transient_loss_kinds_ref.py.  Every comparison is loss_cases.check: 3 x the fp32 restatement's own distance from fp64
plus 1e-6 of the tensor's scale."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import common
import loss_cases as lc
import nrc_amd
import transient_loss_kinds_ref as kref
from nrc_amd import config, rc_ext, train
from nrc_amd.config import TransientDataLossConfig

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = -1, -5        # RC_ERR_INVALID_ARG, RC_ERR_UNSUPPORTED
RCFG = nrc_amd.cornell_transient_config()
E = kref.handle_exposure(RCFG)
CORNELL = config.transient_data_loss_preset("cornell_itof")
PAIRS = CORNELL.itof_frequency_phase_shifts
LOW = config.transient_data_loss_preset("kitchen_itof").itof_frequency_phase_shifts
LOOP_STEPS, LOOP_LR = 20, 1e-4          # test_gpu_transient_data_loss.test_adam_loop_lowers_the_loss (see LOOP_LR there)


def _kind(loss_type, use_itof, pairs):
    return dataclasses.replace(TransientDataLossConfig(), loss_type=loss_type, use_itof=use_itof, itof_frequency_phase_shifts=pairs)


# every new type; use_itof on a per-bin type, an iToF type without it, both frequency sets and the steady-state reading
CASES = {
    "rawnerf_transient": _kind("rawnerf_transient", False, ()),
    "mse": config.transient_data_loss_preset("mse"),
    "mse_unbiased+use_itof": _kind("mse_unbiased", True, PAIRS),
    "mse_itof": _kind("mse_itof", False, PAIRS),
    "mse_itof_unbiased": _kind("mse_itof_unbiased", True, LOW),
    "rawnerf_transient_itof": CORNELL,
    "rawnerf_transient_itof_unbiased": dataclasses.replace(CORNELL, loss_type="rawnerf_transient_itof_unbiased"),
    "steady_state": config.transient_data_loss_preset("steady_state"),
}
assert {c.loss_type for c in CASES.values()} == set(rc_ext.TRANSIENT_LOSS_TYPES[1:])


def _rc(weights=None, cfg=RCFG):
    h = rc_ext.RadianceCache(cfg, 0)
    h.load_weights(common.weights_transient_np() if weights is None else weights)
    return h


@pytest.fixture(scope="module")
def rc():
    return _rc()


@pytest.fixture(scope="module")
def batch5(rc):
    """n = 5 (a partial workgroup of four waves): rays, jitters, gt, a nocorr pair, lossmult."""
    n = 5
    rays, jit = lc.transient_batch(n, seed=131, jitter_seed=132)
    gt = lc.transient_target(rc, rays, jit, 133)
    rn, gn = lc.transient_target(rc, rays, jit, 134), lc.transient_target(rc, rays, jit, 135)
    return n, rays, jit, gt, rn, gn, lc.lossmult(n)


def _f(x):
    return np.asarray(x, np.float64)


# ---- a. rc_dtof_to_itof ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cornell", "one", "zero", "eight"])
def test_dtof_to_itof(rc, batch5, name):
    n, rays, jit = batch5[:3]
    pairs = {"cornell": PAIRS, "one": ((1e8, 0.7),), "zero": (),
             "eight": tuple(PAIRS) + tuple(LOW)}[name]
    x = rc.render_transient(rays, {"jitter": jit}, outputs=["rgb"])["rgb"]
    got = rc.dtof_to_itof(x, pairs)
    assert tuple(got.shape) == (n, 2 * len(pairs) + 1, 3) and float(x.abs().max()) > 0
    xh = x.cpu().numpy()
    r64 = kref.dtof_to_itof(torch.from_numpy(xh).double(), pairs, E).numpy()
    r32 = kref.dtof_to_itof(torch.from_numpy(xh), pairs, E).double().numpy()
    lc.check(_f(got.cpu().numpy()), r64, r32, f"dtof_to_itof {name}")
    if name == "zero":                      # the steady-state image: half the bin sum
        lc.check(_f(got.cpu().numpy()[:, 0]), _f(xh).sum(1) / 2, xh.sum(1, dtype=np.float32).astype(np.float64) / 2, "steady state")
    assert torch.equal(got, rc.dtof_to_itof(x, pairs))


# ---- b. / d. every new type on the device's own render ------------------------------------------------------------------

def _loss_case(rc, what, n, rays, jit, gt, rn, gn, lm, cfg, guard):
    _, losses = rc.transient_data_backward(rays, {"jitter": jit}, gt, rn, gn, lm, cfg=cfg, grad=False)
    losses = losses.cpu().numpy()
    rgb = rc.workspace("td:rgb")[: n * 2100].reshape(n, 700, 3).copy()
    G = rc.workspace("td:G")[: n * 2100].reshape(n, 700, 3).copy()
    l64, m64, G64 = kref.loss_and_G(rgb, gt, rn, gn, lm, cfg, E, torch.float64)
    l32, m32, G32 = kref.loss_and_G(rgb, gt, rn, gn, lm, cfg, E, torch.float32)
    print(what, "loss", losses[0], l64, l32, "mse", losses[1], m64, m32, "G err", float(np.abs(G - G64).max()),
          "granted", lc.granted(G64, G32))
    lc.check(_f(losses[0:1]), _f([l64]), _f([l32]), what + " loss")
    lc.check(_f(losses[1:2]), _f([m64]), _f([m32]), what + " mse")
    lc.check(_f(G), G64, G32, what + " G")
    assert np.abs(G64).max() > 0
    if guard:               # the case can fail: the default type's values on the same buffers are far away
        dflt = dataclasses.replace(TransientDataLossConfig(), loss_thresh=cfg.loss_thresh)
        d64, _, Gd64 = kref.loss_and_G(rgb, gt, rn, gn, lm, dflt, E, torch.float64)
        lc.guard(what, (l64, l32, d64), ({"G": G64}, {"G": G32}, {"G": Gd64}))


@pytest.mark.parametrize("name", sorted(CASES))
def test_loss_and_G_vs_fp64(rc, batch5, name):
    n, rays, jit, gt, rn, gn, lm = batch5
    _loss_case(rc, name + " plain", n, rays, jit, gt, None, None, None, CASES[name], True)
    _loss_case(rc, name + " lossmult nocorr", n, rays, jit, gt, rn, gn, lm, CASES[name], False)


def test_loss_thresh_zeroes_some_pairs(rc, batch5):
    n, rays, jit, gt, rn, gn, lm = batch5
    thresh, share = lc.transient_loss_thresh(gt)
    assert 0.1 <= share <= 0.6, share
    cfg = dataclasses.replace(CORNELL, loss_thresh=thresh)
    _loss_case(rc, "rawnerf_transient_itof loss_thresh", n, rays, jit, gt, rn, gn, lm, cfg, False)
    G = rc.workspace("td:G")[: n * 2100].reshape(n, 700, 3)
    zeroed = np.asarray(gt, np.float64).max(axis=1) > thresh
    assert zeroed.any() and not G.transpose(0, 2, 1)[zeroed].any()


# ---- c. the whole chain ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss_type", ["rawnerf_transient_itof", "rawnerf_transient_itof_unbiased"])
def test_chain_vs_fp64(rc, loss_type):
    n = 8
    cfg = dataclasses.replace(CORNELL, loss_type=loss_type)
    rays, jit = lc.transient_batch(n, seed=31, jitter_seed=32)
    gt = lc.transient_target(rc, rays, jit, 33)
    rn, gn = lc.transient_target(rc, rays, jit, 144), lc.transient_target(rc, rays, jit, 145)
    w = common.weights_transient_np()
    refs = tuple(kref.chain_kind(w, rays, jit, gt, rn, gn, None, dt, loss_cfg=cfg) for dt in (torch.float64, torch.float32))
    lc.transient_compare(rc, False, rays, jit, gt, rgb_nocorr=rn, gt_nocorr=gn, what=loss_type, loss_cfg=cfg, refs=refs)


# ---- e. equivalence and determinism -----------------------------------------------------------------------------------------

def _raw_kind_call(h, rays, jit, gt, ck, flat, losses):
    """rc_transient_data_backward_kind as the library exports it -> its return code."""
    r, held, n = h._rays_struct(rays)
    cam = h._dev(rays["cam_origins"]).reshape(-1, 3)
    rnd_p = h._jitter_struct(jit, held, n)
    gt_t = h._dev(gt).reshape(-1)
    code = h.lib.rc_transient_data_backward_kind(h._h, C.byref(r), cam.data_ptr(), n, rnd_p, gt_t.data_ptr(), None, None, None,
                                                 None if ck is None else C.byref(ck), None if flat is None else flat.data_ptr(),
                                                 losses.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return code


def test_type_0_is_bitwise_the_existing_entry(rc):
    n = 8
    rays, jit = lc.transient_batch(n, seed=151, jitter_seed=152)
    gt = lc.transient_target(rc, rays, jit, 153)
    a, la = rc.transient_data_backward(rays, {"jitter": jit}, gt)
    Ga = rc.workspace("td:G")[: n * 2100].copy()
    ck = rc_ext.transient_data_loss_kind_c(TransientDataLossConfig())
    assert ck.loss_type == 0 and ck.use_itof == 0
    b, lb = torch.zeros_like(a), torch.zeros_like(la)
    assert _raw_kind_call(rc, rays, jit, gt, ck, b, lb) == 0
    assert torch.equal(a, b) and torch.equal(la, lb) and float(a.abs().max()) > 0
    assert np.array_equal(Ga, rc.workspace("td:G")[: n * 2100])


def test_bitwise_repeat_and_accumulation(rc):
    n = 257
    rays, jit = lc.transient_batch(n, seed=161, jitter_seed=162)
    gt = lc.transient_target(rc, rays, jit, 163)
    rnd = {"jitter": jit}
    a, la = rc.transient_data_backward(rays, rnd, gt, cfg=CORNELL)
    keep = {k: rc.workspace("td:" + k).copy() for k in ("G", "Gt") + tuple(k for k, _ in lc.TRANSIENT_ADJOINTS)}
    b, lb = rc.transient_data_backward(rays, rnd, gt, cfg=CORNELL)
    assert torch.equal(a, b) and torch.equal(la, lb) and float(a.abs().max()) > 0
    for k, v in keep.items():
        assert np.array_equal(v, rc.workspace("td:" + k)), k
    rays1, jit1 = {k: np.asarray(v)[:8] for k, v in rays.items()}, [j[:8] for j in jit]
    one, _ = rc.transient_data_backward(rays1, {"jitter": jit1}, gt[:8], cfg=CORNELL)
    two, _ = rc.transient_data_backward(rays1, {"jitter": jit1}, gt[:8], cfg=CORNELL, grad=one.clone())
    assert torch.equal(two, 2.0 * one) and float(one.abs().max()) > 0


# ---- f. refusals ----------------------------------------------------------------------------------------------------------

def test_refusals(rc):
    rays, jit = lc.transient_batch(4, seed=171)
    gt = np.zeros((4, 700, 3), np.float32)
    good = rc_ext.transient_data_loss_kind_c(CORNELL)

    def patched(**kw):
        ck = rc_ext.rc_transient_data_loss_kind.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(ck, k, v)
        return ck

    nan_f = patched()
    nan_f.frequency[2] = float("nan")
    inf_p = patched()
    inf_p.phase_shift[0] = float("inf")
    hot = common.make_rc()
    occ = _rc(cfg=nrc_amd.cornell_transient_config(use_occlusions=True))
    for what, h, ck, want in (("n_pairs 9", rc, patched(n_pairs=9), INVALID_ARG), ("n_pairs -1", rc, patched(n_pairs=-1), INVALID_ARG),
                              ("loss_type COUNT", rc, patched(loss_type=rc_ext.RC_TLOSS_COUNT), INVALID_ARG),
                              ("loss_type -1", rc, patched(loss_type=-1), INVALID_ARG),
                              ("NaN frequency", rc, nan_f, INVALID_ARG), ("inf phase", rc, inf_p, INVALID_ARG),
                              ("null cfg", rc, None, INVALID_ARG),
                              ("non-transient handle", hot, good, UNSUPPORTED), ("occlusion handle", occ, good, UNSUPPORTED)):
        losses = torch.full((2,), 7.0, device="cuda")
        assert _raw_kind_call(h, rays, jit, gt, ck, None, losses) == want, what
        assert losses.tolist() == [7.0, 7.0], what
    # the binding's own refusals
    for bad in (dict(loss_type="charb"), dict(transient_gauss_sigma_scales=((2.0, 1.0),)), dict(mask_lossmult=True),
                dict(clip_eval=True)):
        with pytest.raises(NotImplementedError):
            rc.transient_data_backward(rays, None, gt, cfg=dataclasses.replace(CORNELL, **bad), grad=False)
    x = torch.zeros((4, 700, 3), device="cuda")
    with pytest.raises(rc_ext.RcError) as e:
        hot.dtof_to_itof(x, PAIRS)
    assert e.value.code == UNSUPPORTED
    with pytest.raises(rc_ext.RcError) as e:
        rc.dtof_to_itof(x, ((float("nan"), 0.0),))
    assert e.value.code == INVALID_ARG
    assert tuple(occ.dtof_to_itof(x, ()).shape) == (4, 1, 3)


# ---- g. the training loop -------------------------------------------------------------------------------------------------

def test_adam_loop_lowers_the_itof_loss():
    """transient_head_step under the cornell_itof preset: 20 steps on a fixed batch against a target rendered from perturbed
    head weights, rate and target as test_gpu_transient_data_loss.test_adam_loop_lowers_the_loss builds them."""
    w = common.weights_transient_np()
    w2 = lc.perturbed(lc.perturbed(w, "transient_indirect_layer", 7), "output_rgba_layer", 8)
    rays, jit = lc.transient_batch(128, seed=91, jitter_seed=92)
    gt = _rc(weights=w2).render_transient(rays, {"jitter": jit}, outputs=["rgb"])["rgb"].clone()
    h = _rc()
    ocfg = config.OptimizerConfig(lr_init=LOOP_LR, lr_final=LOOP_LR, lr_delay_steps=0, extra_opt_params=tuple(
        config.ExtraOptParams(g, LOOP_LR, LOOP_LR, 0, LOOP_LR, LOOP_LR, 0) for g in ("Cache", "SurfaceLightField")))
    opt = train.TransientHeadOptimizer(h, ocfg)
    opt.init_from(w)
    hist = [float(train.transient_head_step(h, opt, rays, None, jit, gt, cfg=CORNELL)["data"]) for _ in range(LOOP_STEPS)]
    print("transient_head_step loop under cornell_itof (data):", [f"{t:.6e}" for t in hist])
    assert opt.count == LOOP_STEPS and all(np.isfinite(hist))
    assert hist[-1] < hist[0], ("first and last loss", hist[0], hist[-1])
