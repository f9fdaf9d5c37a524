"""RadianceCache.material_randoms on the GPU: every random tensor of one material-stage forward, planned
in C and drawn by ONE launch of k_prng_fill_segments into one arena.  Every member against rc.prng_fill of the plan's
key, mode and shape (bitwise) and against the host twin (bits and uniforms bitwise; normal rtol 2e-6 / atol 2e-7, gumbel
rtol 2e-6 / atol 2e-6: the bounds tests/test_prng.py applies to rc_prng_fill); the arena around the members; the refusals;
and rc_render_material fed by it.  Cases: material_randoms_cases.py (the smallest shapes at which the kernel can go wrong)."""
import ctypes as C

import numpy as np
import pytest
import torch

import common
import loss_cases as lc
import material_randoms_cases as mc
from nrc_amd import prng, rc_ext

pytestmark = pytest.mark.gpu

MODE_NAME = {prng.MODE_BITS: "bits", prng.MODE_UNIFORM: "uniform", prng.MODE_NORMAL: "normal", prng.MODE_GUMBEL: "gumbel"}
SENTINEL = 0x7FC0DEAD            # a NaN pattern no mode produces


@pytest.fixture(scope="module")
def rc():
    return lc.make_material_rc(common.weights_material_np(True))


def _member(out, d, n, Ks):
    """The device tensor that holds draw d, in jax's element order and shape."""
    base = d.name.partition("[")[0]
    l = int(d.name[-2]) if d.name.endswith("]") else None
    if d.layout == "planes":
        return torch.stack([out[d.name + "1"], out[d.name + "2"]], dim=-1)
    if base in ("spec_jitter", "diff_jitter"):
        t = out["sec_jitter"][l]
        return t[: n * Ks] if base == "spec_jitter" else t[n * Ks:]
    if base in ("spec_gumbel", "diff_gumbel"):
        return out["sec_gumbel"][: n * Ks] if base == "spec_gumbel" else out["sec_gumbel"][n * Ks:]
    return out[base][l] if l is not None else out[d.name]


def _draw(rc, n, K, train, env, loss, vmf, key=None):
    return rc.material_randoms(mc.model_key(n) if key is None else key, n, K, train=train, env_sampler=env,
                               loss_key=mc.LOSS_KEY if loss else None, vmf_noise_in_arena=vmf)


def _tensors(out):
    return [t for v in out.values() for t in (v if isinstance(v, list) else [v]) if isinstance(t, torch.Tensor)]


@pytest.mark.parametrize("n,K", mc.SIZES)
def test_every_member_is_the_single_fill_and_the_host_twin(rc, n, K):
    Ks = prng.material_split(mc.cfg_for(K))[0]
    for train, env, loss, vmf in mc.FLAGS:
        plan = mc.python_plan(n, K, train, env, loss, vmf)
        out = _draw(rc, n, K, train, env, loss, vmf)
        host = prng.plan_randoms(plan)
        seen = 0
        for d in plan:
            if d.layout == "key":
                assert np.array_equal(out[d.name], d.key) and out[d.name].dtype == np.uint32, d.name
                continue
            got = _member(out, d, n, Ks)
            assert tuple(got.shape) == tuple(d.shape), (d.name, got.shape)
            one = rc.prng_fill(d.key, d.shape, MODE_NAME[d.mode])
            assert torch.equal(got.contiguous().view(torch.int32), one.view(torch.int32)), (d.name, n, K, train, env)
            want = prng._DRAW_FN[d.mode](d.key, tuple(d.shape))
            g = got.cpu().numpy()
            if d.mode == prng.MODE_UNIFORM:
                assert np.array_equal(g, want), d.name
            elif d.mode == prng.MODE_NORMAL:
                np.testing.assert_allclose(g, want, rtol=2e-6, atol=2e-7, err_msg=d.name)
            else:
                np.testing.assert_allclose(g, want, rtol=2e-6, atol=2e-6, err_msg=d.name)
            seen += got.numel()
        assert seen == sum(int(np.prod(d.shape)) for d in plan)
        # the dict is what render_material takes: the host twin's members, the two traces joined as the ABI lays them out
        assert "spec_jitter" not in out and set(host) - {"spec_jitter", "diff_jitter", "spec_gumbel", "diff_gumbel"} <= set(out)
        if not env and not vmf:                                   # the PRNGKey(1) constant from the per-n cache
            assert torch.equal(out["vmf_noise"], rc.prng_fill(prng.random_split(prng.PRNGKey(1))[0], (n, 128, 3), "normal"))
            assert out["vmf_noise"] is _draw(rc, n, K, train, env, loss, vmf)["vmf_noise"]
        # one storage for every entry drawn by the call
        drawn = [t for t in _tensors(out) if vmf or env or t is not out.get("vmf_noise")]
        assert len({t.untyped_storage().data_ptr() for t in drawn}) == 1


def test_bits_mode_and_two_planes_with_an_odd_count(rc):
    """RC_PRNG_MODE_BITS (no member of the plan uses it) and hand-made segments: an odd two-plane segment, a one-element
    and an empty one, a uniform range; each against rc.prng_fill."""
    key = prng.split(prng.PRNGKey(5))[1]
    seg = lambda mode, n, off, off2=-1, lo=0.0, hi=1.0: rc_ext.rc_prng_segment(
        key=(C.c_uint32 * 2)(int(key[0]), int(key[1])), mode=mode, id=0, lo=lo, hi=hi, n=n, offset=off, offset2=off2)
    arena = torch.full((2048,), SENTINEL, dtype=torch.int32, device="cuda")
    rc.prng_fill_segments([seg(prng.MODE_BITS, 515, 0), seg(prng.MODE_UNIFORM, 9, 600, 640, 2.0, 6.0),
                           seg(prng.MODE_NORMAL, 1, 700), seg(prng.MODE_GUMBEL, 0, 704), seg(prng.MODE_BITS, 1, 710, 720)], arena)
    assert torch.equal(arena[:515], rc.prng_fill(key, (515,), "bits"))
    u = rc.prng_fill(key, (9,), "uniform", 2.0, 6.0).view(torch.int32)
    assert torch.equal(arena[600:605], u[0::2]) and torch.equal(arena[640:644], u[1::2])
    assert torch.equal(arena[700:701], rc.prng_fill(key, (1,), "normal").view(torch.int32))
    assert torch.equal(arena[710:711], rc.prng_fill(key, (1,), "bits"))
    written = torch.zeros(2048, dtype=torch.bool, device="cuda")
    for lo, hi in ((0, 515), (600, 605), (640, 644), (700, 701), (710, 711)):
        written[lo:hi] = True
    assert bool((arena[~written] == SENTINEL).all())


@pytest.mark.parametrize("n,K", mc.SIZES)
def test_the_arena_around_the_members_is_left_alone(rc, n, K):
    """The plan filled into an arena of sentinels with 100 spare words behind it: every word outside the members' spans
    keeps the sentinel, every word inside is written (no mode produces the sentinel's NaN pattern)."""
    for train, env, loss, vmf in [(False, False, False, False), (True, False, True, True), (True, True, True, False)]:
        segs, words = mc.c_plan(n, K, train, env, loss, vmf)
        arena = torch.full((words + 100,), SENTINEL, dtype=torch.int32, device="cuda")
        rc.prng_fill_segments(segs, arena)
        inside = torch.zeros(words + 100, dtype=torch.bool, device="cuda")
        for lo, hi, _ in mc.spans_of(segs):
            inside[lo:hi] = True
        assert int(inside.sum()) == sum(g.n for g in segs)
        assert bool((arena[~inside] == SENTINEL).all()) and bool((arena[inside] != SENTINEL).all())


def test_keys_and_determinism(rc):
    """The same key twice: the same bytes.  Another model key (and loss key): every member differs, except what does not
    depend on them -- the PRNGKey(1) constant, and at train=False the secondary traces' PRNGKey(0) jitter."""
    n, K = 257, 8
    for train in (False, True):
        a = rc.material_randoms(prng.PRNGKey(3), n, K, train=train, loss_key=prng.PRNGKey(4))
        b = rc.material_randoms(prng.PRNGKey(3), n, K, train=train, loss_key=prng.PRNGKey(4))
        c = rc.material_randoms(prng.PRNGKey(5), n, K, train=train, loss_key=prng.PRNGKey(6))
        assert set(a) == set(c) and "noise" in a
        for k in a:
            pairs = list(zip(a[k], b[k], c[k])) if isinstance(a[k], list) else [(a[k], b[k], c[k])]
            for x, y, z in pairs:
                assert torch.equal(x, y), k
                fixed = k == "vmf_noise" or (k == "sec_jitter" and not train)
                assert torch.equal(x, z) == fixed, (k, train)
        assert a["gumbel"].untyped_storage().data_ptr() != b["gumbel"].untyped_storage().data_ptr()


def test_refusals_launch_nothing(rc):
    """A destination outside the arena, 33 segments, two overlapping destinations, an unknown mode: RC_ERR_INVALID_ARG with
    a message, and the arena keeps its sentinels."""
    segs, words = mc.c_plan(3, 6, False, False, False, False)
    arena = torch.full((words,), SENTINEL, dtype=torch.int32, device="cuda")
    copy = lambda: [rc_ext.rc_prng_segment.from_buffer_copy(g) for g in segs]

    def refused(bad, arena_view=arena, match=""):
        with pytest.raises(rc_ext.RcError, match=match) as e:
            rc.prng_fill_segments(bad, arena_view)
        assert e.value.code == -1
        torch.cuda.synchronize()
        assert bool((arena == SENTINEL).all())

    bad = copy(); bad[-1].offset = words - bad[-1].n + 1
    refused(bad, match="outside the arena")
    bad = copy(); bad[3].offset = -64
    refused(bad, match="outside the arena")
    refused(copy(), arena[: words - 64], match="outside the arena")            # the arena one member short
    bad = copy(); bad[4].offset2 = words
    refused(bad, match="outside the arena")
    refused((copy() * 2)[:33], match="n_segs")
    bad = copy(); bad[1].offset = bad[0].offset
    refused(bad, match="overlap")
    bad = copy(); bad[5].offset = bad[4].offset2 + 1                            # inside a two-plane member's second plane
    refused(bad, match="overlap")
    bad = copy(); bad[2].mode = 4
    refused(bad, match="unknown mode")
    bad = copy(); bad[2].n = 0xFFFFFFFF
    refused(bad, match="2\\^32")
    rc.prng_fill_segments(segs, arena)                                          # and the table itself is accepted
    assert not bool((arena == SENTINEL).all())


@pytest.mark.parametrize("K", [8, 32])
@pytest.mark.parametrize("train", [False, True])
def test_render_material_from_the_device_randoms(rc, K, train):
    """rc_render_material fed by material_randoms: bitwise what it renders from the same tensors read back and handed over
    as host arrays; and against the host twin's tensors uploaded (prng.material_pass_randoms; bits and uniforms equal,
    normal and Gumbel values an ulp or two apart) within the material stage's tolerance of DESIGN.md §6, 1e-4 on every
    output of the rays whose categorical picks agree -- which are at least the 97 % (primary) / 90 % (all picks) that
    tests/test_prng.py asks of the key path against the oracle (smooth tables, as there)."""
    n = 1500
    cfg = mc.cfg_for(K)
    rays = lc.material_case(n, K)[0]
    key = prng.PRNGKey(2024 + K)
    dev = rc.material_randoms(key, n, K, train=train)
    back = {k: ([t.cpu().numpy() for t in v] if isinstance(v, list) else v.cpu().numpy()) for k, v in dev.items()}

    def render(rnd):
        cres, mres = rc.render_material(rays, rnd, num_secondary_samples=K)
        torch.cuda.synchronize()
        picks = np.concatenate([rc.workspace("inds", np.int32)[:n, None], rc.workspace("s:inds", np.int32)[: n * K].reshape(2, n, K // 2)
                                .transpose(1, 0, 2).reshape(n, K)], axis=1)
        return {**{"c_" + k: v.clone() for k, v in cres.items()}, **{"m_" + k: v.clone() for k, v in mres.items()}}, picks

    a, picks_a = render(dev)
    b, picks_b = render(back)
    assert np.array_equal(picks_a, picks_b)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    h, picks_h = render(prng.material_pass_randoms(key, n, cfg, train=train))
    primary, every = picks_a[:, 0] == picks_h[:, 0], (picks_a == picks_h).all(axis=1)
    print(f"K={K} train={train}: equal primary picks {primary.mean():.4f}, all picks {every.mean():.4f}")
    assert primary.mean() >= 0.97 and every.mean() >= 0.9
    worst = {k: float((a[k] - h[k]).abs().reshape(n, -1)[torch.from_numpy(every).cuda()].max()) for k in a}
    print("max |device randoms - host randoms| on those rays:", {k: f"{v:.2e}" for k, v in worst.items() if v > 0})
    assert max(worst.values()) <= 1e-4, worst


def test_model_apply_with_a_key_draws_on_the_device(rc):
    """Model.apply(passes=("cache", "light", "material"), rng=key) renders what render_material renders from
    material_randoms(key): the key path of the model is the device path."""
    import nrc_amd
    from nrc_amd.model import Model
    m = Model(mc.CFG, 0)
    m.load_variables(common.weights_material_np(True))
    n = 96
    rays = nrc_amd.synthetic_rays(n, seed=41)
    key = prng.PRNGKey(77)
    out = m.apply(None, key, rays, passes=("cache", "light", "material"))["render"]
    _, mres = m.rc.render_material(rays.hot_fields(), m.rc.material_randoms(key, n))
    assert torch.equal(out["rgb"], mres["rgb"]) and float(out["rgb"].abs().max()) > 0
