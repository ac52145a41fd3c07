"""GPU: the latent-space sampler (hmc_latent path) against the latent oracle and the reference-captured G7 run."""
import copy
import types

import numpy as np
import pytest
import torch

from oracle import latent_ref, operators as oops
from oracle.latent_ref import F64Latent

pytestmark = pytest.mark.gpu
T = torch.from_numpy
SEQ, SEQ_NEXT = [250, 500, 750], [-1, 250, 500]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def test_first_latent_trajectory_of_the_reference_run(golden):
    from nhmc import operators, plugin, sampler
    g = golden('g7_hmc_latent_16.npz')
    dev = torch.device('cuda')
    op = operators.Inpainting(3, 64, T(g['missing']), dev)
    model = latent_ref.TinyLatentModel().to(dev)
    algo = plugin.HMCLatent(model, op, float(g['sigma_0']))
    table = torch.cat([model.alphas_cumprod_prev[0:1], model.alphas_cumprod])
    eng = sampler.LeapfrogEngine(algo.score, op, None, SEQ, SEQ_NEXT, dev, alpha_table=table,
                                 image_map=model.differentiable_decode_first_stage)
    st = sampler.ChainState(1, 0.3, 0.1, dev)
    st['eps_eff'].fill_(float(g['epsilon']))
    st['sigma_y'].fill_(float(g['sigma_y']))
    got = sampler.run_trajectory(eng, T(g['x']).to(dev), T(g['p0']).to(dev).clone(), T(g['y_0']).to(dev), st, 1.0, 2)
    want = latent_ref.trajectory_latent(T(g['x']), T(g['p0']), SEQ, SEQ_NEXT, latent_ref.TinyLatentModel(),
                                        oops.InpaintRef(3, 64, T(g['missing'])), T(g['y_0']),
                                        sigma_y=float(g['sigma_y']), eps=float(g['epsilon']), m=1.0, L=2)
    assert rel(got['x_prop'], want['x']) < 1e-4 and rel(got['xt'], want['xt']) < 1e-4 and rel(got['loss'], want['loss']) < 1e-4
    assert abs(float((got['H1'] - got['H0'])[0]) + float(g['neg_dH'][0])) < 0.02


def test_latent_loop_takes_the_oracles_decisions():
    """70-epoch latent loop at B = 1 on the noise the oracle draws: same accept decisions, same returned latents."""
    from nhmc import operators, plugin, sampler
    dev = torch.device('cuda')
    g_ = torch.Generator().manual_seed(4)
    missing = oops.random_inpaint_missing(64, generator=g_)
    ref_op, op = oops.InpaintRef(3, 64, missing), operators.Inpainting(3, 64, missing, dev)
    x = torch.randn(1, 3, 16, 16, generator=g_)
    x_orig = torch.rand(1, 3, 64, 64, generator=g_) * 2 - 1
    y = ref_op.H(x_orig) + 0.1 * torch.randn(1, ref_op.M, generator=g_)
    kw = dict(sigma_y=0.5, tau=0.3, epsilon=0.1, m=1.0, sigma_0=0.1)
    cpu_model = F64Latent()                                 # built BEFORE seeding: nn layer init draws from the global RNG
    torch.manual_seed(99)
    trace = {}
    want = latent_ref.hmc_latent_reference(x, SEQ, SEQ_NEXT, cpu_model, ref_op, y, x_orig, trace=trace, **kw)
    torch.manual_seed(99)                                   # regenerate the very same draws as a tape
    P, U = [], []
    for _ in range(70):
        P.append(torch.randn(1, 3, 16, 16))
        U.append(torch.rand(1))
    algo = plugin.HMCLatent(F64Latent().to(dev), op, 0.1)
    opt = types.SimpleNamespace(tau=0.3, epsilon=0.1, m=1.0, sigma_0=0.1, sigma_y=0.5)
    res = sampler.hmc_latent_chains(x.to(dev), SEQ, SEQ_NEXT, algo, opt, y.to(dev), op, x_orig.to(dev),
                                    noise=sampler.TapeNoise(lambda it: P[it], lambda it: U[it]), collect_trace=True)
    got_acc = [bool(r['accept'][0]) for r in res.trace]
    for it, (a, b) in enumerate(zip(trace['accept'], got_acc)):
        margin = abs(float(U[it]) - min(1.0, float(np.exp(-trace['dH'][it]))))
        assert a == b or margin < 1e-3, (it, a, b, margin)
    assert [float(r['sigma_y'][0]) for r in res.trace] == trace['sigma_y']
    assert res.samples[0].shape == want.shape and rel(res.samples[0], want) < 1e-4
    out = sampler.hmc_latent(x.to(dev), 1, SEQ, SEQ_NEXT, algo,
                             types.SimpleNamespace(**vars(opt), noise_source=sampler.TapeNoise(lambda it: P[it], lambda it: U[it])),
                             y.to(dev), op, x_orig.to(dev))
    assert torch.equal(out, res.samples[0])


def test_latent_loop_with_several_chains_takes_each_oracle_runs_decisions():
    """Five chains in one call, each with its own problem and tape, against five batch-1 oracle runs (epochs 10, sampling
    3): decisions, per-epoch sigma_y / eps, ragged sample counts and the returned latents per chain.  Measured on the CPU
    where the chains were chosen: final-phase accepts 0, 4, 1, 5, 3 (an empty result, a wrapped ring, a ragged count, an
    exactly full ring), smallest margins 0.117, 0.067, 0.245, 0.020, 0.065; chain 0 also ends with a shrunk eps."""
    from nhmc import operators, plugin, sampler
    from oracle import chain_cases as cc
    chains, keep, o = cc.LATENT_CHAINS, cc.LATENT_SAMPLING, cc.LATENT_OPT
    cases = [cc.latent_chain(c) for c in chains]
    for c, k in zip(chains, cases):
        print(f'latent chain {c}: final-phase accepts {k.final_accepts}, accepts {sum(k.trace["accept"])}, '
              f'min margin {min(k.margins):.4f}, last eps {k.trace["eps"][-1]:.6f}')
    # from the oracle traces alone: no decision of these inputs is inside the band the comparison excuses ...
    assert all(min(k.margins) >= 5e-3 for k in cases)
    # ... and the bookkeeping branches are there
    counts = [k.final_accepts for k in cases]
    assert len(set(counts)) > 1 and 0 in counts and max(counts) > keep
    assert any(e not in (o['epsilon'], 0.01) for k in cases for e in k.trace['eps'])          # a chain shrank eps
    dev = torch.device('cuda')
    op = operators.Inpainting(3, 64, cc.latent_mask(), dev)
    algo = plugin.HMCLatent(F64Latent().to(dev), op, o['sigma_0'])
    opt = types.SimpleNamespace(**o)
    x, y, x_orig = (torch.cat([getattr(k, a) for k in cases]).to(dev) for a in ('x', 'y', 'x_orig'))
    tape = sampler.TapeNoise(lambda it: torch.cat([k.P[it] for k in cases]), lambda it: torch.cat([k.U[it] for k in cases]))
    res = sampler.hmc_latent_chains(x, SEQ, SEQ_NEXT, algo, opt, y, op, x_orig, noise=tape, epochs=cc.LATENT_EPOCHS,
                                    sampling=keep, collect_trace=True)
    n_accept = res.n_accept.cpu().tolist()
    for j, (c, k) in enumerate(zip(chains, cases)):
        got_acc = [bool(r['accept'][j]) for r in res.trace]
        for it, (a, b) in enumerate(zip(k.trace['accept'], got_acc)):
            assert a == b or k.margins[it] < 1e-3, (c, it, a, b, k.margins[it])
        assert [float(r['sigma_y'][j]) for r in res.trace] == k.trace['sigma_y'], c
        assert [float(r['eps'][j]) for r in res.trace] == k.trace['eps'], c
        assert res.count[j] == k.final_accepts and n_accept[j] == sum(k.trace['accept']), c
        assert res.samples[j].shape == k.want.shape, (c, res.samples[j].shape)
        if k.final_accepts:
            err = rel(res.samples[j], k.want)
            print(f'latent chain {c}: returned latents rel err {err:.2e}')
            assert err < 1e-4, c


def test_latent_chain_does_not_depend_on_its_neighbours():
    """A B = 4 call equals four B = 1 calls on the same per-chain tapes, bit for bit (batch-invariant stand-in model)."""
    from nhmc import operators, plugin, sampler
    dev = torch.device('cuda')
    g_ = torch.Generator().manual_seed(61)
    B, dim, epochs, keep = 4, 8, 6, 3
    op = operators.Inpainting(3, 4 * dim, oops.random_inpaint_missing(4 * dim, generator=g_), dev)
    algo = plugin.HMCLatent(latent_ref.PointwiseLatent().to(dev), op, 0.1)
    x = torch.randn(B, 3, dim, dim, generator=g_).to(dev)
    y = (torch.randn(B, op.M, generator=g_) * 0.5).to(dev)
    P = [torch.randn(B, 3, dim, dim, generator=g_) for _ in range(epochs + 2 * keep)]
    U = [torch.rand(B, generator=g_) for _ in range(epochs + 2 * keep)]
    opt = types.SimpleNamespace(tau=0.3, epsilon=0.1, m=1.0, sigma_0=0.1, sigma_y=0.5)

    def run(lo, hi):
        tape = sampler.TapeNoise(lambda it: P[it][lo:hi], lambda it: U[it][lo:hi])
        return sampler.hmc_latent_chains(x[lo:hi], SEQ, SEQ_NEXT, algo, opt, y[lo:hi], op, noise=tape, epochs=epochs,
                                         sampling=keep)

    full = run(0, B)
    print('neighbour test, latent: counts', full.count, 'accepts', full.n_accept.cpu().tolist())
    assert int(full.n_accept.sum()) > 0
    for c in range(B):
        one = run(c, c + 1)
        assert one.count[0] == full.count[c] and int(one.n_accept[0]) == int(full.n_accept[c]), c
        assert torch.equal(one.x[0], full.x[c]) and torch.equal(one.xt[0], full.xt[c]), c
        assert one.samples[0].shape == full.samples[c].shape and torch.equal(one.samples[0], full.samples[c]), c
