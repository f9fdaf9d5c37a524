"""The restatement behind the geometry smoothness tests (tests/geometry_smoothness_ref.py) and the host pieces of the loss:
the second-order parameter gradient against central finite differences in fp64, the exact-zero bias gradients, the key path
of prng.geometry_smoothness_noise, train.geometry_smoothness_terms and cache_stage_grads' defaults.  No GPU."""
import inspect

import numpy as np
import torch

import common
import geometry_smoothness_ref as gs
import nrc_amd
from nrc_amd import prng, train
from nrc_amd.config import GeometrySmoothnessConfig
from oracle import train_ref

CFG = nrc_amd.hotdog_config()
L2 = CFG.num_levels - 1
BASE = f"params/Cache/Sampler/MLP_{L2}"


def _points(count, seed=3):
    """Points away from ReLU kinks (relu_margin > 1e-3) and cell faces (> 1e-2 grid units), both branches of the
    contraction among them."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pts = (rng.standard_normal((16 * count, 3)) * 1.2).astype(np.float32)
    m = train_ref.relu_margin(common.weights_torch(dtype=torch.float64), CFG, L2, torch.from_numpy(pts).double()).numpy()
    keep = np.nonzero((m > 1e-3) & (gs.cell_face_margin(pts) > 1e-2))[0][:count]
    assert len(keep) == count
    r = np.linalg.norm(pts[keep], axis=-1)
    assert (r > 2.0).any() and (r < 2.0).any()                         # contract_radius 2: inside and outside
    return pts[keep]


def _loss(w, pts, noise, weights, lm, terms):
    t = lambda a: torch.from_numpy(np.asarray(a)).double()
    n_x, d_x = gs.normals_chain(w, t(pts))
    n_p, d_p = gs.normals_chain(w, t(gs.perturbed(pts, noise, terms["noise"])))
    return gs.smoothness_loss(n_x, n_p, d_x, d_p, t(weights), t(lm), terms)


def test_parameter_gradient_against_finite_differences():
    """d loss / d parameter of the restatement (a double backward through lookup, contraction and MLP) against central
    differences of the loss in fp64, for a handful of entries each of W0, W1, w_out, a dense and a hashed table; the density
    term is on (weight_density 0.01) so that both paths are differenced."""
    n, S = 4, 8
    pts = _points(n * S).reshape(n, S, 3)
    rng = np.random.Generator(np.random.PCG64(5))
    noise = rng.standard_normal((n, S, 3)).astype(np.float32)
    weights = rng.uniform(0.0, 0.2, (n, S))
    lm = rng.uniform(0.5, 2.0, n)
    terms = dict(train.geometry_smoothness_terms(1.0), weight_density=0.01)
    w = gs.leaf_weights(common.weights_np(), torch.float64)
    names = gs.param_names(w)
    grads = dict(zip(names, torch.autograd.grad(_loss(w, pts, noise, weights, lm, terms), [w[k] for k in names], allow_unused=True)))
    tables = sorted(k for k in names if "density_grid" in k)
    dense_t = next(k for k in tables if w[k].dim() == 4)
    hashed_t = next(k for k in tables if w[k].dim() == 2)
    checked = 0
    for name in (f"{BASE}/density_layers_0/kernel", f"{BASE}/density_layers_1/kernel", f"{BASE}/output_density_layer/kernel",
                 dense_t, hashed_t):
        g = grads[name].reshape(-1)
        scale = float(g.abs().max())
        assert scale > 0, name
        for i in torch.argsort(g.abs(), descending=True)[:4].tolist():
            flat = w[name].detach().reshape(-1)
            x0 = float(flat[i])
            h = 1e-6 * max(1.0, abs(x0))
            vals = []
            for s in (1.0, -1.0):
                with torch.no_grad():
                    flat[i] = x0 + s * h
                vals.append(float(_loss(w, pts, noise, weights, lm, terms).detach()))
            with torch.no_grad():
                flat[i] = x0
            fd = (vals[0] - vals[1]) / (2.0 * h)
            assert abs(fd - float(g[i])) <= 1e-5 * scale + 1e-6 * abs(float(g[i])), (name, i, fd, float(g[i]))
            checked += 1
    assert checked == 20


def test_bias_gradients_through_the_normals_are_exactly_zero():
    pts = _points(64, seed=7)
    v = np.random.Generator(np.random.PCG64(8)).standard_normal((64, 3))
    g, normals = gs.normals_backward(common.weights_np(), pts, v, torch.float64)
    for layer in gs.LAYERS:
        assert not g[f"{BASE}/{layer}/bias"].any(), layer
        assert g[f"{BASE}/{layer}/kernel"].any(), layer
    tables = [k for k in g if "density_grid" in k]
    assert len(tables) == len(CFG.proposal_grids[L2].grid_sizes) and all(g[k].any() for k in tables)
    np.testing.assert_allclose(np.linalg.norm(normals, axis=-1), 1.0, rtol=1e-12)


def test_noise_key_path_and_shape():
    key = prng.PRNGKey(20200823)
    z = prng.geometry_smoothness_noise(key, 5, 32)
    assert z.shape == (5, 32, 3) and z.dtype == np.float32
    rng = prng.split(prng.split(key)[1])[0]                             # train_utils.py:2728, :2741: two plain splits
    assert np.array_equal(z, prng.normal(rng, (5, 32, 3)))
    assert not np.array_equal(z, prng.normal(prng.split(key)[0], (5, 32, 3)))
    assert not np.array_equal(z, prng.geometry_smoothness_noise(prng.PRNGKey(1), 5, 32))
    assert "geometry_smoothness" in prng.EXTRA_LOSS_ORDER


def test_terms_arithmetic():
    cfg = GeometrySmoothnessConfig()
    assert (cfg.noise, cfg.weight_normals, cfg.weight_normals_pred, cfg.weight_density, cfg.mult, cfg.start_frac) == \
        (0.1, 0.001, 0.0, 0.0, 1.0, 0.0)
    assert train.geometry_smoothness_terms(0.0) == dict(noise=0.1, weight_normals=0.001, weight_normals_pred=0.0, weight_density=0.0)
    c = GeometrySmoothnessConfig(mult=3.0, start_frac=0.25, noise=0.05, weight_normals=0.002, weight_density=0.5)
    assert train.geometry_smoothness_terms(0.5, c, scale=2.0) == dict(noise=0.05, weight_normals=0.002 * 6.0,
                                                                       weight_normals_pred=0.0, weight_density=0.5 * 6.0)
    off = train.geometry_smoothness_terms(0.2, c)                       # before start_frac: every weight 0, the noise kept
    assert off == dict(noise=0.05, weight_normals=0.0, weight_normals_pred=0.0, weight_density=0.0)


def test_cache_stage_grads_leaves_the_term_out_by_default():
    p = inspect.signature(train.cache_stage_grads).parameters
    assert p["smoothness_cfg"].default is None and p["smoothness_noise"].default is None
    assert list(p)[-2:] == ["smoothness_cfg", "smoothness_noise"]       # behind every earlier argument
