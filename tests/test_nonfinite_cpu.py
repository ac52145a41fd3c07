"""CPU: what the GPU module tests/test_nonfinite_gpu.py compares the kernels against, pinned where it can run without a GPU.

  * the two torch facts the kernels' clamps follow: clamp(NaN) is NaN, and the clamp backward SELECTS (a masked element's
    gradient is zero even when the incoming gradient is inf or NaN);
  * the kernels' clamp expression, restated: it passes a NaN and gives min(max(v, lo), hi) for everything else;
  * the oracle's trajectory of a chain whose decode diverges: NaN loss, NaN H1, the clean chains untouched.
"""
import numpy as np
import pytest
import torch

from oracle import hmc_ref, operators as oops, schedule as osched

NAN, INF = float('nan'), float('inf')
SEQ, SEQ_NEXT = [250, 500, 750], [-1, 250, 500]


def gen(seed):
    return torch.Generator().manual_seed(seed)


class PointwiseScore(torch.nn.Module):
    """The stand-in score of tests/test_graph_run_gpu.py: elementwise ATen ops and `torch.roll`, per-channel constants in
    registered buffers; sample b's output depends on sample b alone, captured in a graph or not."""

    def __init__(self, learn_sigma=True, seed=0):
        super().__init__()
        g_ = gen(seed)
        c = lambda mean, std: (mean + std * torch.randn(1, 3, 1, 1, generator=g_))
        self.learn_sigma = learn_sigma
        for name, v in (('w_x', c(0.7, 0.1)), ('w_h', c(0.0, 0.2)), ('w_w', c(0.0, 0.2)), ('bias', c(0.0, 0.1)),
                        ('w_s', c(1.0, 0.2)), ('w_v', c(0.5, 0.1))):
            self.register_buffer(name, v)

    def eps(self, x, t):
        a = (t / 1000.0).view(-1, 1, 1, 1)
        u = x * self.w_x + torch.roll(x, 1, 2) * self.w_h + torch.roll(x, -1, 3) * self.w_w + self.bias
        return torch.tanh(u) * (0.5 + a) + torch.sin(x * self.w_s) * (a * 0.25)

    def forward(self, x, t):
        e = self.eps(x, t)
        return torch.cat([e, torch.tanh(e * self.w_v) * 0.1], dim=1) if self.learn_sigma else e


class DivergingScore(PointwiseScore):
    """+ NaN wherever the input exceeds 40: sample-local and elementwise.  A start point with one element at 41 has a
    finite x and a finite sum of squares, and a decode that is not."""

    def __init__(self, learn_sigma=True, seed=0):
        super().__init__(learn_sigma, seed)
        self.register_buffer('nan_', torch.full((1, 1, 1, 1), NAN))
        self.register_buffer('zero_', torch.zeros(1, 1, 1, 1))

    def eps(self, x, t):
        return super().eps(x, t) + torch.where(x > 40.0, self.nan_, self.zero_)


class NoGradDivergingScore(DivergingScore):
    """Evaluated without gradient (what the latent model's score is): the engine asks the mix VJP for no g_e, and the
    gradient and the momentum of a diverged chain stay finite -- only its loss tells."""

    def __init__(self, seed=0):
        super().__init__(learn_sigma=False, seed=seed)

    def forward(self, x, t):
        with torch.no_grad():
            return self.eps(x, t)


def test_torch_clamp_keeps_nan_and_its_backward_selects():
    x = torch.tensor([NAN, 2.0, -3.0, 0.5, -0.0, INF, -INF])
    out = x.clamp(-1, 1)
    assert torch.isnan(out[0]) and out[1:].tolist() == [1.0, -1.0, 0.5, -0.0, 1.0, -1.0]
    assert np.signbit(out[4].item())
    assert torch.isnan(torch.clamp((torch.tensor([NAN]) + 1.0) / 2.0, 0.0, 1.0)).all()         # to_unit_range
    # backward: 1[-1 <= x <= 1] chooses between the incoming gradient and zero; a NaN input is outside
    x = torch.tensor([2.0, 0.5, -3.0, NAN, 1.0, -1.0], requires_grad=True)
    (g,) = torch.autograd.grad(x.clamp(-1, 1), x, torch.tensor([INF, INF, 1.0, NAN, NAN, -INF]))
    assert g[[0, 2, 3]].tolist() == [0.0, 0.0, 0.0]
    assert g[1].item() == INF and torch.isnan(g[4]) and g[5].item() == -INF                 # the bounds themselves pass


def test_the_kernels_clamp_expression_passes_nan_and_is_min_max_otherwise():
    """nhmc_clamp: v < lo ? lo : (v > hi ? hi : v), in float32 -- against minimum(maximum(v, lo), hi) bit for bit on every
    non-NaN input, -0.0 and the bounds included."""
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 2,
                        np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(np.float32(1), np.float32(2)),
                                  np.nextafter(np.float32(-1), np.float32(-2)), INF, -INF, 1e-45, -1e-45], dtype=np.float32)])
    for lo, hi in ((-1.0, 1.0), (0.0, 1.0)):
        lo, hi = np.float32(lo), np.float32(hi)
        sel = np.where(v < lo, lo, np.where(v > hi, hi, v)).astype(np.float32)
        ref = np.minimum(np.maximum(v, lo), hi)
        if lo == 0.0:                                  # max(-0.0, +0.0) may be either zero; the select keeps the input's sign
            assert np.array_equal(sel, ref)
        else:
            assert np.array_equal(sel.view(np.int32), ref.view(np.int32))
        nan = np.array([np.nan], dtype=np.float32)
        assert np.isnan(np.where(nan < lo, lo, np.where(nan > hi, hi, nan))).all()


@pytest.mark.parametrize('score', ['grad', 'nograd'])
def test_oracle_trajectory_of_a_diverging_chain(score):
    """hmc_ref.trajectory, B = 3, chain 1 starting with one element at 41: its loss and H1 are NaN and its decode holds
    NaN (`.clip(-1, 1)` keeps it); H0's sum of squares is finite; the clean chains are the run without the marker."""
    dim, B, L = 16, 3, 2
    g_ = gen(3)
    ref_op = oops.InpaintRef(3, dim, oops.random_inpaint_missing(dim, frac=0.5, generator=g_))
    net = DivergingScore() if score == 'grad' else NoGradDivergingScore()
    b = osched.betas_fp32()
    x, p = torch.randn(B, 3, dim, dim, generator=g_), torch.randn(B, 3, dim, dim, generator=g_)
    y = ref_op.H(torch.rand(B, 3, dim, dim, generator=g_) * 2 - 1) + 0.1 * torch.randn(B, ref_op.M, generator=g_)
    xm = x.clone()
    xm[1, 1, 8, 9] = 41.0
    kw = dict(sigma_y=np.array([1.7, 0.9, 0.1]), eps=np.array([0.05, 0.04, 0.03]), m=1.0, L=L)
    clean = hmc_ref.trajectory(x, p.clone(), b, SEQ, SEQ_NEXT, net, ref_op, y, **kw)
    got = hmc_ref.trajectory(xm, p.clone(), b, SEQ, SEQ_NEXT, net, ref_op, y, **kw)
    assert torch.isfinite(xm).all() and torch.isfinite((xm ** 2).sum((1, 2, 3))).all()
    assert torch.isnan(got['loss'][1]) and torch.isnan(got['H1'][1]) and torch.isnan(got['H0'][1])
    assert torch.isnan(got['xt'][1]).any()
    if score == 'nograd':                              # nothing but the loss tells: position and momentum stay finite
        assert torch.isfinite(got['x'][1]).all() and torch.isfinite(got['p'][1]).all()
    else:
        assert torch.isnan(got['p'][1]).any()
    for k in ('x', 'p', 'xt', 'loss', 'H0', 'H1'):
        assert torch.isfinite(got[k][[0, 2]]).all(), k
        assert torch.equal(got[k][[0, 2]], clean[k][[0, 2]]), k
