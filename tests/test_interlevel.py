"""Spline interlevel loss of the proposal samplers (rc_interlevel_backward): the torch restatement in tests/interlevel_ref.py
against closed forms, an independent fp64 quadrature and finite differences, and the anneal schedule (CPU only)."""
import numpy as np
import torch

import interlevel_ref as ir
import nrc_amd
from nrc_amd import train


def _histogram(rng, k):
    t = np.sort(rng.uniform(0.0, 1.0, size=k + 1))
    t[0], t[-1] = 0.0, 1.0
    w = rng.uniform(size=k) ** 3
    w[rng.integers(0, k, size=k // 4)] = 0.0        # empty bins
    return t, w / w.sum()


def test_box_known_answer():
    """A single box [0.4, 0.6] of weight 1 blurred by halfwidth 0.05: its CDF is a C1 ramp pair."""
    t = torch.tensor([0.4, 0.6], dtype=torch.float64)
    w = torch.tensor([1.0], dtype=torch.float64)
    q = torch.tensor([0.3, 0.35, 0.4, 0.5, 0.6, 0.65, 0.7], dtype=torch.float64)
    got = ir.blurred_cdf(q, t, w, 0.05).numpy()
    np.testing.assert_allclose(got, [0.0, 0.0, 0.0625, 0.5, 0.9375, 1.0, 1.0], atol=1e-12)


def _witness_cdf(q, t, w, h):
    """(1/2h) int_{-h}^{h} F(q - s) ds with F the piecewise-linear CDF of (t, w), by the trapezoid rule on a dense grid
    that contains every kink of the integrand (exact for piecewise-linear F up to rounding)."""
    F = lambda x: np.interp(x, t, np.concatenate([[0.0], np.cumsum(w)]))
    out = []
    for qq in q:
        s = np.concatenate([np.linspace(-h, h, 4001), np.clip(qq - t, -h, h)])
        s = np.unique(s)
        out.append(np.trapezoid(F(qq - s), s) / (2 * h))
    return np.array(out)


def test_blur_matches_quadrature_witness():
    rng = np.random.Generator(np.random.PCG64(11))
    for k, h in ((32, 0.03), (32, 0.003), (8, 0.2), (64, 0.01)):
        t, w = _histogram(rng, k)
        q = np.sort(np.concatenate([rng.uniform(-0.3, 1.3, size=200), t, t + h, t - h]))
        got = ir.blurred_cdf(torch.from_numpy(q), torch.from_numpy(t), torch.from_numpy(w), h).numpy()
        ref = _witness_cdf(q, t, w, h)
        assert np.abs(got - ref).max() <= 1e-9, (k, h, np.abs(got - ref).max())


def test_blur_conserves_mass():
    rng = np.random.Generator(np.random.PCG64(12))
    for h in (0.03, 0.003):
        t, w = _histogram(rng, 32)
        w = torch.from_numpy(w * 0.7)
        cp = torch.linspace(-h - 0.01, 1 + h + 0.01, 65, dtype=torch.float64)
        wb = ir.blur_and_resample_weights(cp, torch.from_numpy(t), w, h)
        assert abs(float(wb.sum()) - float(w.sum())) <= 1e-12
        assert float(wb.min()) >= 0.0


def _level_case(rng, n=3):
    """sdist / tdist / density of three sampler levels (64, 64, 32 intervals) for n rays."""
    sd, td, dens = [], [], []
    for S in (64, 64, 32):
        s = np.sort(rng.uniform(size=(n, S + 1)), axis=-1)
        s[:, 0], s[:, -1] = 0.0, 1.0
        sd.append(s)
        td.append(0.5 + 4.0 * s)
        dens.append(rng.uniform(0.0, 3.0, size=(n, S)) ** 2)
    d = rng.normal(size=(n, 3))
    return sd, td, dens, d


def test_density_gradient_matches_central_differences():
    rng = np.random.Generator(np.random.PCG64(13))
    sd, td, dens, d = _level_case(rng)
    lm = np.array([1.0, 0.5, 2.0])
    mults, blurs = (0.01, 0.01), (0.03, 0.003)
    losses, grads = ir.interlevel_forward_backward(sd, td, dens, d, lm, mults, blurs, torch.float64)
    checked = 0
    for level in (0, 1):
        g = grads[level].numpy()
        for idx in [(0, 3), (1, 20), (2, 40), (0, 63), tuple(np.unravel_index(np.abs(g).argmax(), g.shape))]:
            eps = 1e-8 * max(1.0, dens[level][idx])
            dp = [x.copy() for x in dens]; dp[level][idx] += eps
            dm = [x.copy() for x in dens]; dm[level][idx] -= eps
            lp, _ = ir.interlevel_forward_backward(sd, td, dp, d, lm, mults, blurs, torch.float64)
            lmn, _ = ir.interlevel_forward_backward(sd, td, dm, d, lm, mults, blurs, torch.float64)
            fd = (lp[level] - lmn[level]) / (2 * eps)
            assert abs(fd - g[idx]) <= 1e-5 * max(abs(fd), 1e-3 * np.abs(g).max()), (level, idx, fd, g[idx])
            checked += 1
    assert checked == 10 and all(v > 0 for v in losses)


def test_reverse_scan_form_equals_autograd():
    """The kernel's formulation: d L / d x_k = g_k T_{k+1} - sum_{i>k} g_i w_i with x = density |delta|."""
    rng = np.random.Generator(np.random.PCG64(14))
    sd, td, dens, d = _level_case(rng, n=4)
    lm = np.ones(4)
    _, grads = ir.interlevel_forward_backward(sd, td, dens, d, lm, (1.0, 1.0), (0.03, 0.003), torch.float64)
    # g = d loss / d weights of level 0 by autograd, then the closed form
    dirs = torch.from_numpy(d)
    dens0 = torch.from_numpy(dens[0]).requires_grad_(True)
    w = [ir.compute_alpha_weights(dens0, torch.from_numpy(td[0]), dirs)] + \
        [ir.compute_alpha_weights(torch.from_numpy(x), torch.from_numpy(t), dirs) for x, t in zip(dens[1:], td[1:])]
    w0 = w[0].detach().requires_grad_(True)
    loss = ir.spline_interlevel_loss([torch.from_numpy(s) for s in sd], [w0] + w[1:], torch.ones(4, 1), (1.0, 1.0), (0.03, 0.003))[0]
    (g,) = torch.autograd.grad(loss, w0)
    adelta = (torch.from_numpy(td[0]).diff(dim=-1) * dirs.norm(dim=-1, keepdim=True)).abs()
    x = dens0.detach() * adelta
    tnext = torch.exp(-torch.cumsum(x, dim=-1))
    gw = g * w0.detach()
    after = gw.flip(-1).cumsum(-1).flip(-1) - gw
    dd = (g * tnext - after) * adelta
    np.testing.assert_allclose(dd.numpy(), grads[0].numpy(), rtol=1e-10, atol=1e-14)


def test_anneal_schedule():
    assert train.anneal_at(1.0) == 0.4 == nrc_amd.RenderConfig().anneal
    assert train.anneal_at(0.0) == 0.0
    vals = [train.anneal_at(f) for f in np.linspace(0.0, 1.0, 101)]
    assert all(b >= a for a, b in zip(vals, vals[1:]))
    assert vals[1] > 0.0 and vals[-1] == 0.4
    c = nrc_amd.InterlevelConfig()
    assert c.mults == (0.01, 0.01) and c.blurs == (0.03, 0.003)
