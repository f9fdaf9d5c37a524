"""The material stage's random_split tree as a plan: prng.material_stage_plan against its C twin
rc_material_randoms_plan (csrc/rc_prng_host.h; the library loads without a GPU), the arena layout, the refusals, and the
host realisation of the plan against material_pass_randoms / relight_pass_randoms.  Cases: material_randoms_cases.py."""
import ctypes as C

import numpy as np
import pytest

import material_randoms_cases as mc
from nrc_amd import prng

RC_ERR_INVALID_ARG, RC_ERR_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from nrc_amd import rc_ext
    return rc_ext.load_library()


@pytest.mark.parametrize("n,K", mc.SIZES)
def test_c_plan_is_the_python_plan(lib, n, K):
    """Every segment's key, mode, element count, id and order, for every combination of the four switches."""
    ids = prng.MEMBER_IDS
    for train, env, loss, vmf in mc.FLAGS:
        plan = mc.python_plan(n, K, train, env, loss, vmf)
        segs, words = mc.c_plan(n, K, train, env, loss, vmf)
        got = [(g.id, g.mode, g.n, g.key[0], g.key[1]) for g in segs]
        assert got == mc.rows_of(plan), (train, env, loss, vmf)
        have = {g.id for g in segs}
        assert len(have) == len(segs)
        assert (ids["noise"] in have) == loss and (ids["vmf_noise"] in have) == (vmf and not env)
        assert (ids["picks_key_spec"] in have) == env == (ids["picks_key_diff"] in have) == (ids["spec_u"] not in have)
        assert all(g.lo == 0.0 and g.hi == 1.0 for g in segs)
        assert all((g.offset2 >= 0) == (g.id in (ids["spec_u"], ids["cos_u"])) for g in segs)


@pytest.mark.parametrize("n,K", mc.SIZES)
def test_offsets_tile_the_arena(lib, n, K):
    """No two destinations overlap, every member starts at a multiple of 64 words and ends inside the arena; the secondary
    traces' segments are adjacent in [spec | diff] order; the arena ends at the last member, rounded up to 64."""
    ids = prng.MEMBER_IDS
    Ks, Kd, Kc, Kl = prng.material_split(mc.cfg_for(K))
    assert Ks + Kd == K
    for train, env, loss, vmf in mc.FLAGS:
        segs, words = mc.c_plan(n, K, train, env, loss, vmf)
        spans = mc.spans_of(segs)
        assert spans[0][0] == 0 and words % 64 == 0 and 0 <= words - max(hi for _, hi, _ in spans) < 64
        for (lo, hi, _), (lo2, _, id2) in zip(spans, spans[1:]):
            assert hi <= lo2, (lo, hi, lo2)
            if id2 not in (ids["diff_gumbel"], *(ids["diff_jitter"] + l for l in range(3))):
                assert lo2 % 64 == 0 and lo2 - hi < 64, (id2, lo2, hi)            # gaps are alignment only
        by_id = {g.id: g for g in segs}
        for spec, diff, per in [(ids["spec_gumbel"], ids["diff_gumbel"], 32)] + [(ids["spec_jitter"] + l, ids["diff_jitter"] + l, 1)
                                                                                   for l in range(3)]:
            assert by_id[spec].n == n * Ks * per and by_id[diff].n == n * Kd * per
            assert by_id[diff].offset == by_id[spec].offset + by_id[spec].n            # one block [n Ks | n Kd]


def test_the_zero_element_member_is_present(lib):
    segs, _ = mc.c_plan(1, 2, False, False, False, False)
    cos = [g for g in segs if g.id == prng.MEMBER_IDS["cos_u"]]
    assert len(cos) == 1 and cos[0].n == 0 and cos[0].offset2 >= 0
    assert prng.material_split(mc.cfg_for(2)) == (1, 1, 0, 1)
    assert prng.material_split(mc.cfg_for(6)) == (3, 3, 2, 1)


def test_refusals(lib):
    from nrc_amd import rc_ext
    with pytest.raises(rc_ext.RcError) as e:                       # a capacity too small
        mc.c_plan(3, 6, False, False, False, False, capacity=5)
    assert e.value.code == RC_ERR_INVALID_ARG
    with pytest.raises(rc_ext.RcError) as e:                       # K = 5: the twin's Ks + Kd = 2 + 2
        mc.c_plan(3, 5, False, False, False, False)
    assert e.value.code == RC_ERR_UNSUPPORTED
    assert sum(prng.material_split(mc.cfg_for(5))[:2]) == 4
    key = (C.c_uint32 * 2)(1, 2)
    levels = (C.c_int32 * 3)(*mc.LEVELS)
    segs = (rc_ext.rc_prng_segment * 32)()
    count, words = C.c_int32(0), C.c_int64(0)
    args = lambda **kw: [kw.get("key", key), None, 4, 8, 0.5, 128, kw.get("levels", levels), 3, 0, kw.get("segs", segs), 32,
                         kw.get("count", C.byref(count)), kw.get("words", C.byref(words))]
    assert lib.rc_material_randoms_plan(*args()) == 0 and count.value == 17
    for name in ("key", "levels", "segs", "count", "words"):
        assert lib.rc_material_randoms_plan(*args(**{name: None})) == RC_ERR_INVALID_ARG, name


def _equal(a, b):
    assert set(a) == set(b), set(a) ^ set(b)
    for k, v in a.items():
        for x, y in zip(v, b[k]) if isinstance(v, list) else [(v, b[k])]:
            assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y), k


@pytest.mark.parametrize("n,K", mc.SIZES)
def test_host_realisation_is_the_pass_randoms(n, K):
    """plan_randoms(material_stage_plan(...)) array for array: material_pass_randoms (vmf_noise included),
    relight_pass_randoms; and the noise a loss_key appends is material_smoothness_noise's."""
    cfg, key = mc.cfg_for(K), mc.model_key(n)
    _equal(prng.plan_randoms(prng.material_stage_plan(key, n, cfg, vmf_noise=True)), prng.material_pass_randoms(key, n, cfg))
    _equal(prng.plan_randoms(prng.material_stage_plan(key, n, cfg, env_sampler=True)), prng.relight_pass_randoms(key, n, cfg))
    with_noise = prng.plan_randoms(prng.material_stage_plan(key, n, cfg, loss_key=mc.LOSS_KEY))
    assert np.array_equal(with_noise.pop("noise"), prng.material_smoothness_noise(mc.LOSS_KEY, n))
    base = prng.material_pass_randoms(key, n, cfg)
    assert np.array_equal(base.pop("vmf_noise"), prng.light_vmf_noise((n, 1, cfg.num_vmf, 3))[:, 0])
    _equal(with_noise, base)


@pytest.mark.parametrize("n,K", mc.SIZES)
def test_train_changes_the_secondary_jitter_alone(n, K):
    """train=True: each secondary trace samples with its own key, cache_keys(kc)["sampler"]; nothing else moves."""
    cfg, key = mc.cfg_for(K), mc.model_key(n)
    a = {d.name: d for d in prng.material_stage_plan(key, n, cfg, train=False, loss_key=mc.LOSS_KEY, vmf_noise=True)}
    b = {d.name: d for d in prng.material_stage_plan(key, n, cfg, train=True, loss_key=mc.LOSS_KEY, vmf_noise=True)}
    assert list(a) == list(b)
    differ = {k for k in a if not np.array_equal(a[k].key, b[k].key)}
    assert differ == {f"{leg}_jitter[{l}]" for leg in ("spec", "diff") for l in range(3)}
    assert all(a[k][2:] == b[k][2:] for k in a)
    for l in range(3):
        assert np.array_equal(a[f"spec_jitter[{l}]"].key, a[f"diff_jitter[{l}]"].key)            # PRNGKey(0) for both
        assert not np.array_equal(b[f"spec_jitter[{l}]"].key, b[f"diff_jitter[{l}]"].key)
    ra, rb = prng.plan_randoms(a.values()), prng.material_pass_randoms(key, n, cfg, train=True)
    for k in rb:
        same = all(np.array_equal(x, y) for x, y in zip(ra[k], rb[k])) if isinstance(rb[k], list) else np.array_equal(ra[k], rb[k])
        assert same == (k not in ("spec_jitter", "diff_jitter")), k
