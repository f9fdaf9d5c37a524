"""From the level-2 density MLP on, lanes j and j + 32 of the fused kernel's wave hold the same sample.  The shader tile
evaluates each softplus / sigmoid once (softplus_pair, sigmoid_pair: one half-wave per value, one v_permlane32_swap), the
fused kernel's compositing sums two channels per register (wave_sum32_pairs) and split8 subtracts in pairs: the same
operations on every value, so every result is bitwise what the library rendered before.

  * tests/golden/halfwave_pin.npz (tools/make_halfwave_pin.py, run on the parent commit; its source hash is inside) holds
    the renders of tests/halfwave_cases.py for BOTH arithmetics: every cache output of 64 seeded rays and of 5 (a partial
    workgroup), normals requested.  The loaded library is held to the part of its own arithmetic; the fp32-MFMA build
    renders in a fresh child process (RC_HIP_LIBRARY) as in tests/test_gpu_f32_build.py.
  * the fused kernel (1), its one-wave twin (3) and the launch-per-stage plan (0) stay bitwise equal on every key at 1, 5
    (clamped rays of a partial workgroup), 64 and 257 rays (a second row of workgroups), with and without `normals`.
  * the helpers on their own (tests/halfwave_check.hip, one wave): wave_sum32_pairs<17> against wave_sum_n<34> on
    zero-padded lanes, 34 channels x 32 lanes of seeded values, signed zeros, denormals, 1e38 magnitudes, an inf and a NaN
    channel -- equal bit for bit once -0 is mapped to +0 (the packed sum drops the trailing `0 + sum` of step 5, which
    can only turn a -0 total into +0), NaN where the other is NaN; softplus_pair and sigmoid_pair against softplus and
    sigmoidf on values in [-30, 30], +-0 and +-inf -- equal bit for bit on all 64 lanes.
    So that equal garbage does not pass, the plain results are also held to fp64: the sums within 31 roundings of the sum
    of magnitudes (31 adds per channel, each within 2^-24 of a partial sum that is at most sum |x|), the functions
    within 1e-6 relative (8 ulp; expf and log1pf are within 2 ulp each, the division and the adds within 1/2, and at
    |x| <= 30 neither function cancels).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import common
import halfwave_cases
import nrc_amd
from nrc_amd.model import _CACHE_DEVICE_KEYS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
CSRC = os.path.join(ROOT, "neural-radiance-caching_amd", "csrc")
PIN = os.path.join(TESTS, "golden", "halfwave_pin.npz")
VARIANT = os.path.join(ROOT, "build", "f32", "librc_hip.so")
EXE = os.path.join(ROOT, "build", "halfwavecheck")
ARITHMETICS = ("bf16x3-split", "f32-mfma")
N_CHAN, N_ROUNDS = 34, 4


def _pin(arith):
    """{"r<n>/<output>": array} of one arithmetic, and the parent's source hash"""
    g = dict(np.load(PIN))
    part = {k[len(arith) + 1:]: v for k, v in g.items() if k.startswith(arith + "/")}
    parent = str(part.pop("source_hash"))
    assert len(parent) == 16
    return part, parent


def _assert_equals_pin(got, part, parent):
    assert set(got) == set(part), sorted(set(got) ^ set(part))
    for k, v in part.items():
        assert v.dtype == np.float32 and got[k].dtype == np.float32 and got[k].shape == v.shape, (k, got[k].shape, v.shape)
        assert np.array_equal(got[k], v), (k, float(np.abs(got[k] - v).max()), "parent source " + parent)


def test_the_pin_holds_both_renders_for_both_arithmetics():
    for arith in ARITHMETICS:
        part, _ = _pin(arith)
        assert set(part) == {f"r{n}/{k}" for n in halfwave_cases.SIZES for k in _CACHE_DEVICE_KEYS}, arith
        assert "r64/normals" in part and part["r64/rgb"].shape == (64, 3) and part["r5/rgb"].shape == (5, 3)
    assert os.path.getsize(PIN) < 100 * 1024


def test_loaded_library_renders_what_the_parent_rendered():
    from nrc_amd import rc_ext
    part, parent = _pin(rc_ext.mlp_arithmetic())
    _assert_equals_pin(halfwave_cases.render_all(), part, parent)


def test_fp32_build_renders_what_the_parent_rendered(tmp_path):
    r = subprocess.run(["make", "-C", CSRC, "-j16", "variant-f32"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    path = str(tmp_path / "f32.npz")
    env = {**os.environ, "RC_HIP_LIBRARY": VARIANT,
           "PYTHONPATH": os.pathsep.join([ROOT, TESTS, os.environ.get("PYTHONPATH", "")])}
    r = subprocess.run([sys.executable, os.path.join(TESTS, "halfwave_cases.py"), path], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    got = dict(np.load(path))
    assert str(got.pop("mlp_arithmetic")) == "f32-mfma"
    got.pop("source_hash")
    part, parent = _pin("f32-mfma")
    _assert_equals_pin(got, part, parent)


@pytest.mark.parametrize("normals", [True, False])
@pytest.mark.parametrize("n", [1, 5, 64, 257])
def test_plans_stay_bitwise_equal(n, normals):
    keys = [k for k in _CACHE_DEVICE_KEYS if normals or k != "normals"]
    assert ("normals" in keys) == normals
    rc = common.make_rc()
    rays = nrc_amd.synthetic_rays(n, seed=5200 + n)
    res = {}
    for mode in (1, 3, 0):
        rc.set_fused(mode)
        try:
            out = rc.render_rays(rays.hot_fields(), None, outputs=keys)
            torch.cuda.synchronize()
        finally:
            rc.set_fused(True)
        res[mode] = {k: v.cpu().numpy() for k, v in out.items()}
    for k in keys:
        assert res[1][k].shape[0] == n and np.isfinite(res[1][k]).all(), k
        assert np.array_equal(res[1][k], res[3][k]), (k, "fused 1 vs fused 3")
        assert np.array_equal(res[1][k], res[0][k]), (k, "fused vs launch-per-stage")


# ---- the helpers on one wave -------------------------------------------------------------------------------------------
CH_ZERO_P, CH_ZERO_N, CH_ZERO_MIX, CH_DENORM, CH_BIG_MIX, CH_BIG_POS, CH_INF, CH_NAN, CH_TINY, CH_WEIGHT = range(24, 34)


def _channels():
    """34 channels x 32 lanes; channels 2 k and 2 k + 1 share register k of the packed sum"""
    rng = np.random.default_rng(20201109)
    x = np.empty((N_CHAN, 32), np.float32)
    x[:24] = (rng.standard_normal((24, 32)) * 10.0 ** rng.uniform(-3, 3, (24, 32))).astype(np.float32)
    x[CH_ZERO_P] = 0.0
    x[CH_ZERO_N] = -0.0
    x[CH_ZERO_MIX] = np.where(rng.random(32) < 0.5, 0.0, -0.0)
    x[CH_DENORM] = (rng.integers(1, 1 << 22, 32).astype(np.uint32) | (rng.integers(0, 2, 32).astype(np.uint32) << 31)).view(np.float32)
    x[CH_BIG_MIX] = rng.choice([-1.0, 1.0], 32) * rng.uniform(0.5e38, 3e38, 32)     # partial sums overflow or not by the order
    x[CH_BIG_POS] = rng.uniform(0.5e38, 3e38, 32)
    x[CH_INF] = rng.standard_normal(32)
    x[CH_INF, 13] = np.inf
    x[CH_NAN] = rng.standard_normal(32)
    x[CH_NAN, 21] = np.nan
    x[CH_TINY] = rng.standard_normal(32) * 3e-38                                    # normals and denormals mixed
    x[CH_WEIGHT] = rng.random(32)
    return x


def _arguments():
    """4 rounds x (xa[32], xb[32]): [-30, 30], the last round with +-0, +-inf and the interval's ends in both positions"""
    rng = np.random.default_rng(7)
    a = rng.uniform(-30.0, 30.0, (N_ROUNDS, 2, 32)).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 30.0, -30.0], np.float32)
    a[3, 0, :6] = special
    a[3, 1, :6] = special[::-1]
    a[3, 1, 10:16] = special
    return a


@pytest.fixture(scope="module")
def wave(tmp_path_factory):
    r = subprocess.run(["make", "-C", CSRC, "halfwavecheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = tmp_path_factory.mktemp("halfwavecheck")
    ch, args = _channels(), _arguments()
    np.concatenate([ch.ravel(), args.ravel()]).astype(np.float32).tofile(d / "in.bin")
    r = subprocess.run([EXE, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "halfwavecheck ok" in r.stdout, r.stdout + r.stderr
    out = np.fromfile(d / "out.bin", np.float32)
    assert out.size == 2 * N_CHAN + N_ROUNDS * 64 * 8
    return {"ch": ch, "args": args, "sum_n": out[:N_CHAN], "sum_p": out[N_CHAN:2 * N_CHAN],
            "fn": out[2 * N_CHAN:].reshape(N_ROUNDS, 64, 8)}


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def test_packed_sum_equals_wave_sum_n(wave):
    a, b = wave["sum_n"], wave["sum_p"]
    print("wave_sum_n      ", a)
    print("wave_sum32_pairs", b)
    assert np.isnan(a[CH_NAN]) and np.isnan(b[CH_NAN])
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    ok = ~np.isnan(a)
    assert np.array_equal(_bits(a[ok] + np.float32(0.0)), _bits(b[ok] + np.float32(0.0))), (a, b)      # -0 + 0 = +0
    assert a[CH_INF] == np.inf and a[CH_BIG_POS] == np.inf
    # the packed sum keeps the sign of an all -0 channel, the 64-lane one adds it to the upper half's +0
    assert _bits(b[CH_ZERO_N]) == 0x80000000 and _bits(a[CH_ZERO_N]) == 0 and _bits(b[CH_ZERO_P]) == 0
    finite = [c for c in range(N_CHAN) if c not in (CH_BIG_MIX, CH_BIG_POS, CH_INF, CH_NAN)]
    x = wave["ch"][finite].astype(np.float64)
    bound = 31 * 2.0 ** -24 * np.abs(x).sum(axis=1) + 2.0 ** -149
    assert (np.abs(a[finite] - x.sum(axis=1)) <= bound).all(), (a[finite], x.sum(axis=1), bound)


@pytest.mark.parametrize("fn", ["softplus", "sigmoid"])
def test_pair_functions_equal_the_plain_functions(wave, fn):
    o = wave["fn"][..., :4] if fn == "softplus" else wave["fn"][..., 4:]
    ya, yb, pa, pb = (o[..., i] for i in range(4))
    assert np.array_equal(_bits(ya), _bits(pa)) and np.array_equal(_bits(yb), _bits(pb)), fn
    for v in (ya, yb):        # both half-waves hold both results
        assert np.array_equal(_bits(v[:, :32]), _bits(v[:, 32:])), fn
    # the plain functions themselves against fp64
    xa, xb = wave["args"][:, 0].astype(np.float64), wave["args"][:, 1].astype(np.float64)
    with np.errstate(over="ignore"):
        ref = (lambda x: np.logaddexp(x, 0.0)) if fn == "softplus" else (lambda x: 1.0 / (1.0 + np.exp(-x)))
        for got, x in ((pa[:, :32], xa), (pb[:, :32], xb)):
            want = ref(x)
            assert not np.isnan(got).any(), fn
            fin = np.isfinite(want)
            assert np.array_equal(got[~fin].astype(np.float64), want[~fin]), fn
            assert (np.abs(got[fin] - want[fin]) <= 1e-6 * np.abs(want[fin])).all(), (fn, np.abs(got[fin] / want[fin] - 1).max())
