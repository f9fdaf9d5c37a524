"""The relighting path without a GPU: the numpy restatement of tests/relight_ref.py is pinned where the
kernels rely on it (the lookup against a literal padded-array loop and known answers, the tables' identities, the
environment sampler's T rule and index mapping, the categorical draw), and the Python layer's argument forms and refusals
run against a handle that records its calls."""
import numpy as np
import pytest

import nrc_amd
import relight_ref as R
from nrc_amd import prng, relight
from nrc_amd.model import Model, create_render_fn


def _image(H, W, seed=0):
    return np.random.default_rng(seed).uniform(0.05, 1.0, size=(H, W, 3)).astype(np.float32)


def _unit(n, seed=1):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


# ---------------------------------------------------------------------------------------------
# lookup
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(4, 8), (5, 7)])
def test_lookup_restatement_equals_the_literal_loop(H, W):
    img = _image(H, W)
    d = _unit(300)
    assert np.abs(R.lookup(img, d) - R.lookup_literal(img, d)).max() <= 1e-14
    # the fp32 form stays near it (it is the floor of the GPU test, not a second definition)
    assert np.abs(R.lookup(img, d.astype(np.float32), np.float32) - R.lookup(img, d)).max() <= 2e-5


@pytest.mark.parametrize("H,W", [(4, 8), (5, 7)])
def test_lookup_known_answers(H, W):
    img = _image(H, W, seed=3).astype(np.float64)
    # integer locations return the texel: row i at polar angle i pi / H (not (i + 1/2) pi / H), columns 1 .. W - 1
    # (column 0 is the seam phi = +pi, below)
    ii, jj = np.meshgrid(np.arange(1, H), np.arange(1, W), indexing="ij")
    got = R.lookup(img, R.direction_at(ii.reshape(-1), jj.reshape(-1), H, W))
    assert np.abs(got - img[ii.reshape(-1), jj.reshape(-1)]).max() <= 1e-12
    # half-way between two rows: the mean of the two texels (pixel centres at integer coordinates)
    got = R.lookup(img, R.direction_at(np.asarray([1.5]), np.asarray([2.0]), H, W))
    assert np.abs(got[0] - 0.5 * (img[1, 2] + img[2, 2])).max() <= 1e-12
    # the last row fades into the zero padding: at row H - 1/2 half of row H - 1 is left, at row H (the pole) nothing
    got = R.lookup(img, R.direction_at(np.asarray([H - 0.5]), np.asarray([3.0]), H, W))
    assert np.abs(got[0] - 0.5 * img[H - 1, 3]).max() <= 1e-12
    # the pole z = -d.y = -1: the lookup's 1e-8 keeps theta 1e-4 short of pi, so 1e-4 H / pi of the last row is left
    pole = R.lookup(img, np.asarray([[0.0, 1.0, 0.0]]))
    assert np.abs(pole).max() <= 1e-4 * H / np.pi * img.max() * 1.001
    top = R.lookup(img, np.asarray([[0.0, -1.0, 0.0]]))          # theta = 0: row 0, phi = atan2(0, 0) = 0: column W / 2
    c = W / 2.0
    c0 = int(np.floor(c))
    want = img[0, c0] * (1 - (c - c0)) + (img[0, c0 + 1] * (c - c0) if c != c0 else 0.0)
    assert np.abs(top[0] - want).max() <= 1e-4 * H / np.pi * 1.001     # the same 1e-4 away from row 0


def test_lookup_seam_does_not_wrap():
    H, W = 4, 8
    img = _image(H, W, seed=5).astype(np.float64)
    th = np.pi * 2 / H                                           # row 2
    # phi = +pi (y = +0 behind x < 0): column 0 exactly; phi -> -pi (y just below 0): column W, the zero padding.  (A
    # y of -0 does not survive the rotation's 0 * z term: it is phi = +pi as well.)
    plus = np.asarray([[-np.sin(th), -np.cos(th), 0.0]])
    minus = np.asarray([[-np.sin(th), -np.cos(th), -1e-12]])
    negzero = np.asarray([[-np.sin(th), -np.cos(th), -0.0]])
    assert np.abs(R.lookup(img, plus)[0] - img[2, 0]).max() <= 1e-7
    assert np.abs(R.lookup(img, negzero)[0] - img[2, 0]).max() <= 1e-7
    assert np.abs(R.lookup(img, minus)[0]).max() <= 1e-9
    # just inside phi = -pi: between column W - 1 and the padding -- dark, not blended with column 0
    eps = 0.25 * 2 * np.pi / W                                  # a quarter texel from the seam: a quarter of the texel is left
    d = R.direction_at(np.asarray([2.0]), np.asarray([W - 0.25]), H, W)
    assert abs(np.arctan2(d[0, 2], d[0, 0]) + np.pi - eps) <= 1e-9
    assert np.abs(R.lookup(img, d)[0] - 0.25 * img[2, W - 1]).max() <= 1e-9


def test_lookup_corner_order_and_clamping():
    H, W = 5, 7
    img = _image(H, W, seed=7)
    d = _unit(64, seed=9).astype(np.float32)
    row, col = R.locations(d, H, W, np.float32)
    # the four corners summed in another order differ in the last bits somewhere: the order is part of the definition
    f = np.float32
    pad = np.zeros((H + 2, W + 2, 3), f)
    pad[1:-1, 1:-1] = img
    r, c = row + f(1), col + f(1)
    fr, fc = np.floor(r), np.floor(c)
    i0, j0 = fr.astype(int), fc.astype(int)
    w = [(f(1) - (r - fr)) * (f(1) - (c - fc)), (f(1) - (r - fr)) * (c - fc), (r - fr) * (f(1) - (c - fc)), (r - fr) * (c - fc)]
    g = [pad[i0, j0], pad[i0, np.minimum(j0 + 1, W + 1)], pad[np.minimum(i0 + 1, H + 1), j0],
         pad[np.minimum(i0 + 1, H + 1), np.minimum(j0 + 1, W + 1)]]
    fwd = ((g[0] * w[0][:, None] + g[1] * w[1][:, None]) + g[2] * w[2][:, None]) + g[3] * w[3][:, None]
    assert np.array_equal(fwd.astype(f), R.lookup(img, d, np.float32))
    # positions outside the padded array clamp into it; a NaN position selects index 0 and the colour is NaN
    far = R.resample_2d(img, np.asarray([-7.0, 40.0]), np.asarray([3.0, 99.0]))
    assert np.abs(far).max() == 0.0
    assert np.array_equal(R._clamp_index(np.asarray([np.nan, -3.0, 2.5, 99.0]), 6), [0, 0, 2, 6])
    bad = R.lookup(img, np.asarray([[np.nan, 0.0, 1.0], [np.inf, 0.0, 0.0]]))
    assert np.isnan(bad).all()


# ---------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(4, 8), (5, 7)])
def test_tables_identities(H, W):
    img = _image(H, W, seed=11)
    pmf, pdf, dirs = R.tables(img, 2.5)
    assert abs(pmf.sum() - 1.0) <= 1e-14
    st = np.repeat(R.row_sin(H), W)
    assert np.abs(pdf * 2 * np.pi ** 2 * st / (H * W) - pmf).max() <= 1e-15
    assert np.abs(np.linalg.norm(dirs, axis=-1) - 1.0).max() <= 1e-14
    # the loader's interval is 1 / H, not pi / H: the first row sits at 0.5 / H
    assert abs(R.row_sin(H)[0] - np.sin(0.5 / H)) <= 1e-15 and abs(R.row_sin(H)[-1] - np.sin(np.pi - 0.5 / H)) <= 1e-15
    # dirs on the stated grid: latitude pi / 2 - (i + 1/2) pi / H, longitude pi - (j + 1/2) 2 pi / W, polar axis z
    d = dirs.reshape(H, W, 3)
    lat = np.pi / 2 - (np.arange(H) + 0.5) * np.pi / H
    lng = np.pi - (np.arange(W) + 0.5) * 2 * np.pi / W
    assert np.abs(np.arcsin(d[..., 2]) - lat[:, None]).max() <= 1e-12
    assert np.abs(np.arctan2(d[..., 1], d[..., 0]) - lng[None, :]).max() <= 1e-12
    # scale multiplies rgb only: pmf does not move
    assert np.abs(R.tables(img, 1.0)[0] - pmf).max() <= 1e-15
    p32 = R.tables(img, 2.5, np.float32)
    assert np.abs(p32[0] - pmf).max() <= 1e-7 and np.abs(p32[2] - dirs).max() <= 1e-6


def test_odd_height_puts_the_middle_row_on_the_seam():
    """The tables' dirs have world z as their polar axis, the lookup world -y (kept as the reference has it).  With an odd
    height the middle row's latitude is 0: its texels with cos(longitude) < 0 are looked up exactly at phi = +-pi, where
    the sign of a rounding residue decides between texel column 0 and the dark padding.  Even heights stay clear."""
    for H, W, on_seam in ((5, 7, True), (4, 8, False)):
        img = _image(H, W, seed=22)
        dirs = R.tables(img)[2]
        up = R.lookup(img, dirs + np.asarray([0.0, 0.0, 1e-9]))
        down = R.lookup(img, dirs - np.asarray([0.0, 0.0, 1e-9]))
        jump = np.abs(up - down).max(-1).reshape(H, W)
        rows = np.unique(np.nonzero(jump > 1e-3)[0])
        assert (list(rows) == [H // 2]) == on_seam and (rows.size == 0) == (not on_seam), (H, rows)
        if on_seam:
            lng = np.pi - (np.arange(W) + 0.5) * 2 * np.pi / W
            assert np.array_equal(jump[H // 2] > 1e-3, np.cos(lng) < 0)


# ---------------------------------------------------------------------------------------------
# sampler
# ---------------------------------------------------------------------------------------------
def test_sampler_T_rule_and_mapping():
    assert relight.expected_T(16, 16) == 256 and relight.expected_T(256, 16) == 256 and relight.expected_T(32, 16) == 256
    assert relight.expected_T(1, 16) == 16 and relight.expected_T(65, 16) == 1040 and relight.expected_T(15, 16) == 240
    assert relight.expected_T(17, 16) == 272
    for n, K in ((1, 16), (65, 16), (16, 16), (256, 16), (48, 16), (3, 5)):
        T = R.expected_T(n, K)
        assert T == relight.expected_T(n, K)
        p = np.random.default_rng(n).integers(0, 35, size=T)
        assert np.array_equal(R.pick_of_sample(p, n, K), R.pick_of_sample_literal(p, n, K, 35))


def test_sampler_weight_zero_below_the_horizon():
    H, W = 5, 7
    pmf, pdf, dirs = R.tables(_image(H, W, seed=13))
    n, K = 9, 4
    nrm = _unit(n, seed=2)
    p = np.arange(n * K) % (H * W)
    local, glob, pd, w = R.env_samples(nrm, p, K, pdf, dirs)
    g = dirs[R.pick_of_sample(p, n, K)]
    cos = (g * nrm[:, None, :]).sum(-1)
    assert np.abs(local[..., 2] - cos).max() <= 1e-12             # the frame's z is the normal
    assert np.array_equal(w, (cos > 0).astype(np.float64)) and 0 < w.sum() < w.size
    assert np.abs(glob - g).max() <= 1e-9                         # into the frame and back
    assert np.array_equal(pd, pdf[R.pick_of_sample(p, n, K)])


def test_categorical_draw_is_argmax_of_gumbel_plus_safe_log():
    hw, T = 35, 7
    pmf = R.tables(_image(5, 7, seed=17))[0].astype(np.float32)
    pmf[3] = 0.0                                                   # safe_log clips at tiny
    key = prng.PRNGKey(42)
    got = prng.categorical(key, R.safe_log(pmf).reshape(1, hw, 1), axis=-2, shape=(1, T, 1))
    g = prng.gumbel(key, (1, T, hw, 1))
    want = np.argmax(g + R.safe_log(pmf).reshape(1, 1, hw, 1), axis=2)
    assert got.shape == (1, T, 1) and np.array_equal(got, want)
    assert np.array_equal(R.picks(key, pmf, T), want[0, :, 0])
    assert R.safe_log(pmf)[3] == np.log(np.finfo(np.float32).tiny)


def test_pick_rows_have_no_near_ties_on_the_gpu_test_image():
    """The image and keys of tests/test_gpu_relight.py's equality check: fewer than 1 % of the rows have a runner-up within
    1e-4 of the maximum, so libm differences of the device's Gumbel (2e-6) flip fewer than that."""
    pmf = R.tables(_image(5, 7, seed=0), 1.0, np.float32)[0]
    close = total = 0
    for seed in (1, 2, 3):
        s = np.sort(R.pick_scores(prng.PRNGKey(seed), pmf, 256), axis=1)
        close += int((s[:, -1] - s[:, -2] < 1e-4).sum())
        total += s.shape[0]
    assert close <= 0.01 * total, (close, total)


def test_relight_pass_randoms_shares_the_material_tensors():
    cfg = nrc_amd.hotdog_config()
    key = prng.PRNGKey(5)
    r = prng.relight_pass_randoms(key, 3, cfg)
    m = prng.material_pass_randoms(key, 3, cfg)
    for k in ("gumbel", "spec_gumbel", "diff_gumbel"):
        assert np.array_equal(r[k], m[k])
    for k in ("jitter", "spec_jitter", "diff_jitter"):
        assert all(np.array_equal(a, b) for a, b in zip(r[k], m[k]))
    assert prng.is_key(r["picks_key_spec"]) and prng.is_key(r["picks_key_diff"])
    assert not np.array_equal(r["picks_key_spec"], r["picks_key_diff"])
    assert "spec_u1" not in r and "vmf_noise" not in r


# ---------------------------------------------------------------------------------------------
# the Python layer on a handle that records its calls
# ---------------------------------------------------------------------------------------------
class _Handle:
    """Stands in for rc_ext.RadianceCache: numpy in, numpy out, every call recorded."""

    def __init__(self):
        self.calls = []

    def _dev(self, x, dtype=None):
        import torch
        return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))

    def env_tables(self, rgb, scale=1.0):
        import torch
        self.calls.append(("env_tables", float(scale)))
        return tuple(torch.from_numpy(t) for t in R.tables(rgb.numpy(), scale, np.float32))

    def set_env_image(self, rgb, pmf=None, pdf=None, dirs=None):
        self.calls.append(("set_env_image", None if rgb is None else tuple(rgb.shape), pmf is not None))

    def env_pick(self, key, T):
        self.calls.append(("env_pick", tuple(int(v) for v in key), int(T)))
        return np.zeros(int(T), np.int32)

    def render_relight(self, fields, randoms, mode, picks_spec, picks_diff, albedo_ratio):
        self.calls.append(("render_relight", mode, None if picks_spec is None else int(np.size(picks_spec)),
                           None if picks_diff is None else int(np.size(picks_diff)), albedo_ratio))
        raise _Reached()

    def render_material(self, fields, randoms):
        self.calls.append(("render_material",))
        raise _Reached()

    def render_chunk(self, fields, randoms, mask, plan, out_flat=None):
        self.calls.append(("render_chunk", int(mask)))
        raise _Reached()

    def output_plan(self, names, n):
        return (3 * n * len(names), {nm: (3 * n * i, (n, 3)) for i, nm in enumerate(names)}, [])


class _Reached(Exception):
    pass


def _model(**cfg_kw):
    import dataclasses
    m = object.__new__(Model)
    m.config = dataclasses.replace(nrc_amd.hotdog_config(), **cfg_kw)
    m.device = 0
    m.rc = _Handle()
    m._variables_ref, m._variables_checked, m._out_arena = None, False, None
    m._leaves, m._plans, m._const_cache = [], {}, {}
    return m


def _rays(n):
    return nrc_amd.synthetic_rays(n, seed=3).hot_fields()


PASSES = ("cache", "light", "material")


def test_apply_routes_env_map_through_render_relight():
    """Fails on the parent commit: Model.apply dropped env_map / albedo_ratio (it rendered with the EnvMap MLP)."""
    from nrc_amd import rc_ext
    m = _model()
    env = relight.EnvImage(m.rc, _image(4, 8), scale=2.5)
    assert m.rc.calls[:2] == [("env_tables", 2.5), ("set_env_image", (4, 8, 3), True)]
    key = prng.PRNGKey(1)
    with pytest.raises(_Reached):
        m.apply(None, key, _rays(5), passes=PASSES, env_map=env, albedo_ratio=(1.0, 0.5, 0.25))
    assert m.rc.calls[-1] == ("render_relight", "brdf", None, None, (1.0, 0.5, 0.25))
    # without env_map the stage is the plain one
    with pytest.raises(_Reached):
        m.apply(None, key, _rays(5), passes=PASSES)
    assert m.rc.calls[-1] == ("render_material",)
    # compute_relight_metrics: the environment sampler, T per leg by the rule (5 x 16 = 80 picks; 16 x 16 -> 256)
    m2 = _model(compute_relight_metrics=True)
    env2 = relight.EnvImage(m2.rc, _image(5, 7))
    for n, T in ((5, 80), (16, 256)):
        with pytest.raises(_Reached):
            m2.apply(None, key, _rays(n), passes=PASSES, env_map=env2)
        assert m2.rc.calls[-1] == ("render_relight", "env", T, T, None)
        assert [c[2] for c in m2.rc.calls if c[0] == "env_pick"][-2:] == [T, T]
    # the reference's array form binds the same image
    pmf, pdf, dirs = R.tables(_image(4, 8), 1.0, np.float32)
    with pytest.raises(_Reached):
        m.apply(None, key, _rays(5), passes=PASSES, env_map=_image(4, 8).reshape(1, 32, 1, 3), env_map_w=8, env_map_h=4,
                env_map_pmf=pmf.reshape(1, 32, 1), env_map_pdf=pdf.reshape(1, 32, 1), env_map_dirs=dirs.reshape(1, 32, 1, 3))
    assert ("set_env_image", (4, 8, 3), True) in m.rc.calls[-3:] and m.rc.calls[-1][0] == "render_relight"
    # secondary rays: the image is composited instead of the EnvMap MLP
    with pytest.raises(_Reached):
        m.apply(None, None, _rays(5), passes=("cache",), is_secondary=True, env_map=env)
    assert m.rc.calls[-1] == ("render_chunk", rc_ext.RC_PASS_CACHE | rc_ext.RC_PASS_SECONDARY | rc_ext.RC_PASS_ENV_IMAGE)


def test_relight_refusals():
    m = _model()
    env = relight.EnvImage(m.rc, _image(5, 7))
    cfg = m.config
    with pytest.raises(ValueError, match="unknown relight mode"):
        relight.relight(m, _rays(5), prng.PRNGKey(0), env, mode="both")
    # T must follow the rule, per leg; the message names the expected T
    rnd = dict(prng.relight_pass_randoms(prng.PRNGKey(0), 5, cfg))
    with pytest.raises(ValueError, match="T = 80"):
        relight.relight(m, _rays(5), dict(rnd, picks_spec=np.zeros(256, np.int32), picks_diff=np.zeros(80, np.int32)), env)
    with pytest.raises(ValueError, match="picks_diff.*T = 80"):
        relight.relight(m, _rays(5), dict(rnd, picks_spec=np.zeros(80, np.int32), picks_diff=np.zeros(81, np.int32)), env)
    with pytest.raises(ValueError, match="T = 256"):
        relight.check_picks(32, cfg, np.zeros(256, np.int32), np.zeros(32 * 16, np.int32))
    with pytest.raises(ValueError, match="picks_spec or picks_key_spec"):
        relight.relight(m, _rays(5), {k: v for k, v in rnd.items() if not k.startswith("picks")}, env)
    with pytest.raises(ValueError, match="key or the dict"):
        relight.relight(m, _rays(5), 3.5, env)
    # the arrays: incomplete, or more than one illumination
    with pytest.raises(ValueError, match="env_map_pmf"):
        m.apply(None, prng.PRNGKey(0), _rays(5), passes=PASSES, env_map=_image(5, 7).reshape(1, 35, 1, 3), env_map_w=7, env_map_h=5)
    pmf, pdf, dirs = R.tables(_image(5, 7), 1.0, np.float32)
    two = np.concatenate([_image(5, 7).reshape(1, 35, 1, 3)] * 2, axis=2)
    with pytest.raises(NotImplementedError, match="single illumination"):
        relight.EnvImage.from_arrays(m.rc, two, 7, 5, pmf, pdf, dirs)
    with pytest.raises(ValueError, match="another handle"):
        relight.as_env_image(_Handle(), env, {})
    with pytest.raises(NotImplementedError, match="albedo_ratio"):
        m._apply_material(None, prng.PRNGKey(0), _rays(5), albedo_ratio=(1, 1, 1))


def test_create_render_fn_accepts_a_dataset_with_env_map():
    m = _model()

    class Data:
        camtype = None
        mesh = None
        env_map = relight.EnvImage(m.rc, _image(4, 8))
        albedo_ratio = (0.5, 0.5, 0.5)

    fn = create_render_fn(m, Data())
    with pytest.raises(_Reached):
        fn(None, prng.PRNGKey(2), 1.0, None, None, _rays(4), PASSES)
    assert m.rc.calls[-1] == ("render_relight", "brdf", None, None, (0.5, 0.5, 0.5))
    Data.mesh = object()
    with pytest.raises(NotImplementedError, match="mesh"):
        create_render_fn(m, Data())
