"""CPU: the two nonlinear degradations (hdr, phase_retrieval) -- C-ABI surface, operator classes, and the host-built
phase factors against the reference's probes (G19, tools/gen_golden_nonlinear.py)."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
NEW_SYMBOLS = ('nhmc_hdr_H', 'nhmc_data_hdr', 'nhmc_mix_bwd_hdr', 'nhmc_phase_tiles', 'nhmc_phase_tmp_floats', 'nhmc_phase_H',
               'nhmc_phase_pinv', 'nhmc_phase_adjoint', 'nhmc_data_phase', 'nhmc_data_phase_vjp')


def probe_inputs(g, kind, dim):
    """The seeded inputs of a G19 probe set, regenerated as the generator drew them (its probe_inputs); the stored heads
    pin the draws."""
    gen = torch.Generator().manual_seed({'hdr': 1900, 'phase': 3900}[kind] + dim)
    x = torch.randn(2, 3, dim, dim, generator=gen) * 0.6
    if kind == 'hdr':
        x[:, 0, 0, :len(g['plant'])] = T(g['plant'])
        y_0 = (torch.rand(2, 3, dim, dim, generator=gen) * 2.4 - 1.2).clip(-1, 1) + 0.1 * torch.randn(2, 3, dim, dim, generator=gen)
        e = torch.randn(2, 6, dim, dim, generator=gen)
        assert np.array_equal(e.reshape(-1)[:64].numpy(), g['e_head'])
        out = (x, y_0, e)
    else:
        n = int(g['n'])
        y_0 = 0.5 * torch.randn(2, 3, n, n, generator=gen).abs()
        out = (x, y_0)
    assert np.array_equal(x.reshape(-1)[:64].numpy(), g['x_head']) and np.array_equal(y_0.reshape(-1)[:64].numpy(), g['y0_head'])
    return out


def stored(g, name, got):
    """(got, want, scale) of a G19 output: whole, or its sparse probes; the norms are compared by the caller via `norms`."""
    flat = got.reshape(got.shape[0], -1)
    if name in g:
        want = T(g[name]).reshape(flat.shape)
        return flat, want, float(want.abs().max())
    return flat[:, T(g[f'{name}_pos']).long()], T(g[f'{name}_probe']), float(g[f'{name}_absmax'])


def max_rel(g, name, got):
    a, b, scale = stored(g, name, got.detach().cpu())
    err = float((a.double() - b.double()).abs().max()) / scale
    if f'{name}_norm' in g:
        nrm = got.detach().cpu().reshape(got.shape[0], -1).double().norm(dim=1)
        err = max(err, float(((nrm - T(g[f'{name}_norm'])).abs() / T(g[f'{name}_norm'])).max()))
    return err


def test_header_declares_the_nonlinear_entry_points():
    src = open(os.path.join(ROOT, 'include', 'nhmc.h')).read()
    assert re.search(r'#define NHMC_ABI_VERSION 2\b', src)                          # additive change
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    names = set(re.findall(r'\b(nhmc_[A-Za-z0-9_]+)\s*\(', src))
    import nhmc
    lib = nhmc._lib.load()
    for name in NEW_SYMBOLS:
        assert name in names and name in nhmc._lib.SIGNATURES and hasattr(lib, name), name


def test_argument_validation_of_the_new_entry_points():
    import ctypes
    import nhmc
    lib = nhmc._lib.load()
    P = ctypes.c_void_p
    null, a16, a4 = P(0), P(0x1000), P(0x1004)
    assert lib.nhmc_hdr_H(null, a16, 1024, null) == 1 and lib.nhmc_hdr_H(a16, a16, 1023, null) == 2
    assert lib.nhmc_data_hdr(a16, a16, 1, a16, null, 1, 1024, null) == 1
    assert lib.nhmc_data_hdr(a16, a4, 1, a16, a16, 1, 1024, null) == 2
    assert lib.nhmc_data_hdr(a16, a16, 1, a16, a16, 70000, 1024, null) == 3
    assert lib.nhmc_mix_bwd_hdr(a16, a16, 5, a16, a16, a16, a16, a16, 0, a16, 1, 3, 256, null) == 3          # e_channels
    assert lib.nhmc_mix_bwd_hdr(a16, a16, 6, a16, a16, a16, a16, null, 0, a16, 1, 3, 256, null) == 1         # g_e is written
    assert lib.nhmc_data_phase(a16, a16, a16, 1, a16, a16, a16, 1, 3, 48, 64, null) == 3                      # dim % 32
    assert lib.nhmc_data_phase(a16, a16, a16, 1, a16, a16, a16, 1, 3, 64, 8, null) == 3                       # (2 pad) % 32
    assert lib.nhmc_data_phase(a16, a16, a16, 1, a16, a16, null, 1, 3, 64, 64, null) == 1
    assert lib.nhmc_data_phase_vjp(a16, a16, a16, a16, a16, 4, a16, a16, a16, a16, a16, a16, 1, 3, 64, 64, null) == 3
    assert lib.nhmc_phase_H(a16, a16, 2, a16, a16, 1, 3, 64, 64, null) == 1                                    # mode
    assert lib.nhmc_phase_pinv(a16, a4, a16, a16, 1, 3, 64, 64, null) == 2
    assert lib.nhmc_phase_adjoint(a16, a16, a16, a16, 30000, 3, 64, 64, null) == 3
    assert lib.nhmc_phase_tiles(3, 256, 64) == 3 * 36 and lib.nhmc_phase_tiles(3, 32, 64) == 3 * 25
    assert lib.nhmc_phase_tmp_floats(2, 3, 64, 64) == 6 * (2 * 192 * 64 + 2 * 192 * 192)


def test_build_operator_serves_the_nonlinear_degradations():
    from nhmc import operators
    from nhmc._lib import NhmcError
    cpu = torch.device('cpu')
    for deg, cls, M in [('hdr', operators.HDR, 3 * 64 * 64), ('phase_retrieval', operators.PhaseRetrievalOperator, 3 * 192 * 192),
                        ('phase', operators.PhaseRetrievalOperator, 3 * 192 * 192)]:
        op = operators.build_operator(deg, 3, 64, cpu)
        assert isinstance(op, cls) and op.is_linear() is False and op.M == M, deg
        assert callable(op.data_term) and callable(op.fused_last_vjp) and callable(op.H) and callable(op.H_pinv)
        params = inspect.signature(op.fused_last_vjp).parameters
        assert list(params)[:5] == ['xt_in', 'e', 'at', 'at_next', 'y'] and 'g_e_out' in params, deg
        assert ('xt_next' in params) == bool(getattr(op, 'fused_wants_decode', False)), deg
        assert list(inspect.signature(op.data_term).parameters) == ['xt', 'y', 'apply_clip', 'loss_out']
    with pytest.raises(NotImplementedError):
        operators.HDR().Ht(torch.zeros(1, 12))                                      # the reference has none
    assert operators.build_operator('phase_retrieval', 3, 256, cpu).n == 384        # the pad is 64 whatever the image size
    assert operators.build_operator('phase_retrieval', 3, 32, cpu).n == 160
    for bad in (48, 80):
        with pytest.raises(NhmcError):
            operators.build_operator('phase_retrieval', 3, bad, cpu)
    assert list(inspect.signature(operators.PhaseRetrievalOperator.__init__).parameters)[:3] == ['self', 'oversample', 'device']
    assert all(op.is_linear() for op in (operators.build_operator(d, 3, 64, cpu) for d in ('sr4', 'color')))   # unchanged
    # no kernel, no result: the operators have no torch fall-back on the CPU
    with pytest.raises(NhmcError):
        operators.build_operator('hdr', 3, 64, cpu).H(torch.zeros(1, 3, 64, 64))


@pytest.mark.parametrize('dim', [64, 256])
def test_host_factors_reproduce_the_reference_probes_in_float64(golden, dim):
    """The host-built Cm, Sm (float64) through the two-sandwich form, in float64 torch, against the reference class's fp32
    H / H_pinv / gradient probes: pins the fixture and the shift / ortho / padding conventions without the reference.
    The only error here is the reference's own: an fp32 FFT carries about eps * log2(n^2) = 6e-8 * 17 = 1e-6 of the largest
    value (bound 2e-6); loss and gradient go through two transforms, a division by |Y| and an fp32 sum (bound 1e-5).  A
    wrong shift, sign or normalisation moves these by O(1)."""
    from nhmc import operators
    g = golden(f'g19_phase_ops_{dim}.npz')
    op = operators.PhaseRetrievalOperator(2.0, 'cpu', channels=3, img_dim=dim)
    assert op.pad == int(g['pad']) == 64 and op.n == int(g['n'])
    x, y_0 = probe_inputs(g, 'phase', dim)
    Cm, Sm = op.Cm, op.Sm

    def spectrum(X):
        return Cm @ X @ Cm.t() - Sm @ X @ Sm.t(), Cm @ X @ Sm.t() + Sm @ X @ Cm.t()

    X = x.double()
    re, im = spectrum(X)
    a = (re ** 2 + im ** 2).sqrt()
    assert max_rel(g, 'Hx', a) < 2e-6                                               # the reference's own fp32 FFT error
    # H^+ : the conjugated factors
    Y = y_0.double()
    pre = Cm.t() @ Y @ Cm - Sm.t() @ Y @ Sm
    pim = Cm.t() @ Y @ Sm + Sm.t() @ Y @ Cm
    assert max_rel(g, 'pinv', (pre ** 2 + pim ** 2).sqrt()) < 2e-6
    # loss and gradient: the adjoint applied to -2 (y - |Y|) Y / |Y|, times the clip mask
    xc = X.clip(-1, 1)
    re, im = spectrum(xc)
    a = (re ** 2 + im ** 2).sqrt()
    r = Y - a
    loss = (r ** 2).sum(dim=(1, 2, 3))
    assert float(((loss - T(g['loss64'])).abs() / T(g['loss64'])).max()) < 1e-5
    wre, wim = -2 * r * re / a, -2 * r * im / a
    grad = (Cm.t() @ wre @ Cm - Sm.t() @ wre @ Sm + Cm.t() @ wim @ Sm + Sm.t() @ wim @ Cm) * ((X >= -1) & (X <= 1))
    assert max_rel(g, 'grad', grad) < 1e-5
    # the packed fp32 layouts the kernels read
    n, d = op.n, dim
    f = op.factors.double()
    assert f.numel() == 6 * n * d
    cat_t, cat, stk = f[:2 * n * d].reshape(d, 2 * n), f[2 * n * d:4 * n * d].reshape(n, 2 * d), f[4 * n * d:].reshape(2 * n, d)
    assert torch.equal(cat_t[:, :n], Cm.t().float().double()) and torch.equal(cat_t[:, n:], Sm.t().float().double())
    assert torch.equal(cat[:, :d], Cm.float().double()) and torch.equal(cat[:, d:], Sm.float().double())
    assert torch.equal(stk[:n], Sm.float().double()) and torch.equal(stk[n:], Cm.float().double())


@pytest.mark.parametrize('dim', [64, 256])
def test_hdr_probes_follow_the_clamp_backward_convention(golden, dim):
    """The fixture itself: at x = +-0.5 (argument exactly +-1) the reference's gradient is nonzero, at +-1 and 0.75 it is 0."""
    g = golden(f'g19_hdr_ops_{dim}.npz')
    x, y_0, _ = probe_inputs(g, 'hdr', dim)
    plant = g['plant']
    if 'grad' in g:
        grad = T(g['grad'])[:, 0, 0, :len(plant)]
        for k, v in enumerate(plant):
            if abs(float(v)) <= 0.5:                                                # argument of the clamp inside or ON +-1
                assert bool((grad[:, k] != 0).all()), (k, v)
            else:
                assert bool((grad[:, k] == 0).all()), (k, v)
        assert torch.equal(T(g['Hx']).reshape(x.shape), (x / 0.5).clip(-1, 1))
    assert float(np.abs(g['loss'] - g['loss64']).max() / g['loss64'].max()) < 1e-5
