"""Oracle: per-chain problems for the several-chains-per-call tests (test infrastructure, see oracle/__init__.py).

Every chain has its own start point, measurement and noise tape, all from seeds; the batch-1 oracle loop is run once per
chain and process (cached) and shared by tests/test_state_model_cpu.py, tests/test_latent_gpu.py and
tests/test_mass_gpu.py.  The global torch RNG is left as it was found.
"""
import functools
import os
import types

import numpy as np
import torch

from . import latent_ref, mass_ref, operators as oops, schedule as osched
from .tiny_score import F64Score, TinyScore

SEQ, SEQ_NEXT = [250, 500, 750], [-1, 250, 500]

LATENT_OPT = dict(sigma_y=0.5, tau=0.3, epsilon=0.1, m=1.0, sigma_0=0.1)
LATENT_EPOCHS, LATENT_SAMPLING = 10, 3
LATENT_CHAINS = (0, 2, 6, 8, 9)           # final-phase accepts 0, 4, 1, 5, 3 where these were chosen (asserted by the tests)

MASS_OPT = dict(tau=0.2, epsilon=0.05, sigma_0=0.1)
MASS_BURN, MASS_EPOCHS, MASS_SAMPLING, MASS_DIM = 2, 9, 2, 16
MASS_CHAINS = (0, 4, 1)                   # 71, 75, 80 trajectories where these were chosen (asserted by the tests)


def margins(trace, U):
    """|u - min(1, exp(-dH))| per trajectory: how far the oracle's accept test was from flipping."""
    return [abs(float(u) - min(1.0, float(np.exp(-dH)))) for u, dH in zip(U, trace['dH'])]


@functools.lru_cache(maxsize=None)
def latent_mask():
    return oops.random_inpaint_missing(64, generator=torch.Generator().manual_seed(4))


@functools.lru_cache(maxsize=None)
def latent_chain(c):
    """Chain c of the latent cases: x, x_orig and the measurement noise from Generator(100 + c) in that order, the tape
    from manual_seed(1000 + c).  -> namespace(x, x_orig, y, P, U, trace, want, final_accepts, margins); `want` is the
    oracle's return, [0, 3, 16, 16] where it collected nothing (its final torch.stack raises on an empty list)."""
    ref_op = oops.InpaintRef(3, 64, latent_mask())
    g = torch.Generator().manual_seed(100 + c)
    x = torch.randn(1, 3, 16, 16, generator=g)
    x_orig = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1
    y = ref_op.H(x_orig) + 0.1 * torch.randn(1, ref_op.M, generator=g)
    n = LATENT_EPOCHS + 2 * LATENT_SAMPLING
    with torch.random.fork_rng():
        model = latent_ref.F64Latent()                      # built BEFORE seeding: nn layer init draws from the global RNG
        torch.manual_seed(1000 + c)
        trace = {}
        try:
            want = latent_ref.hmc_latent_reference(x, SEQ, SEQ_NEXT, model, ref_op, y, x_orig, trace=trace,
                                                   epochs=LATENT_EPOCHS, sampling=LATENT_SAMPLING, **LATENT_OPT)
        except RuntimeError:                                # torch.stack([]): only where nothing was collected
            want = None
        torch.manual_seed(1000 + c)                         # the very same draws as a tape
        P, U = [], []
        for _ in range(n):
            P.append(torch.randn(1, 3, 16, 16))
            U.append(torch.rand(1))
    acc = trace['accept']
    assert len(acc) == n
    final_accepts = sum(1 for e in range(LATENT_EPOCHS, n) if acc[e] and any(acc[:e]))
    if want is None:
        assert final_accepts == 0
        want = torch.zeros(0, 3, 16, 16)
    return types.SimpleNamespace(x=x, x_orig=x_orig, y=y, P=P, U=U, trace=trace, want=want, final_accepts=final_accepts,
                                 margins=margins(trace, U))


@functools.lru_cache(maxsize=None)
def _tiny_score():
    net = TinyScore()
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'tiny_score.pt')
    net.load_state_dict(torch.load(path, weights_only=True))
    return net.eval().requires_grad_(False)


def mass_score():
    """The committed tiny score evaluated in fp64 (a fresh module per call: the caller may move it to a device)."""
    return F64Score(_tiny_score())


@functools.lru_cache(maxsize=None)
def mass_mask():
    return oops.random_inpaint_missing(MASS_DIM, generator=torch.Generator().manual_seed(3))


@functools.lru_cache(maxsize=None)
def mass_chain(c):
    """Chain c of the diagonal-mass cases: problem from Generator(100 + c), tape from manual_seed(2000 + c), ties of the rank
    transform broken by index.  -> namespace(x, x_orig, y, P, U, trace, want, iters, margins)."""
    dim = MASS_DIM
    ref_op = oops.InpaintRef(3, dim, mass_mask())
    g = torch.Generator().manual_seed(100 + c)
    x = torch.randn(1, 3, dim, dim, generator=g)
    x_orig = torch.rand(1, 3, dim, dim, generator=g) * 2 - 1
    y = ref_op.H(x_orig) + 0.1 * torch.randn(1, ref_op.M, generator=g)
    with torch.random.fork_rng():
        score = mass_score()                                # built BEFORE seeding: nn layer init draws from the global RNG
        torch.manual_seed(2000 + c)
        trace = {}
        want = mass_ref.hmc_mass_reference(x, osched.betas_fp32(), SEQ, SEQ_NEXT, score, ref_op, y, x_orig,
                                           burn=MASS_BURN, epochs=MASS_EPOCHS, sampling=MASS_SAMPLING, trace=trace,
                                           stable_sort=True, **MASS_OPT)
        n = len(trace['accept'])
        torch.manual_seed(2000 + c)
        P, U = [], []
        for _ in range(n):
            P.append(torch.randn(1, 3, dim, dim))
            U.append(torch.rand(1))
    return types.SimpleNamespace(x=x, x_orig=x_orig, y=y, P=P, U=U, trace=trace, want=want, iters=n, margins=margins(trace, U))
