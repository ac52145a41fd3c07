"""GPU: the modulated Fourier operator (`--deg mcmri<R>`, `--deg cdp<K>`) through the C ABI, against the float64 oracle of
tests/test_modfourier_cpu.py (torch.fft of the image times each complex map).

The kernels run the centred DFT as fp32-MFMA sandwiches on the real and the imaginary plane of every modulated image where
the oracle runs a complex FFT in float64: no bit identity with it; the bounds are the project's (1e-4 of the largest oracle
value for H and the gradient, 1e-5 relative for the adjointness and the isometry, 1e-6 for the loss against a float64 sum of
the same residuals) and every measured deviation is printed.  What IS bit for bit: the fused last-step VJP against the split
path, the clip mask, a chain alone against the same chain in a batch, and the indifference to whatever the unmeasured
entries of y hold.

Shapes (d, K, B) at C = 3: (32, 1, 3) the 32-tile chain kernel on 18 planes, a grid that is no multiple of 8; (32, 4, 3) 72
planes, a multiple of 8; (64, 3, 2) and (64, 4, 2) the 64-tile kernel; (96, 2, 1) 3 x 3 tiles; (256, 8, 1) once; and
(32, 8, 23), 1104 modulated planes: more than one slab of 1024 (21 chains, then 2).
"""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import hmc_ref, schedule as osched
from oracle.tiny_score import F64Score
from tests.test_fourier_cpu import FourierRef
from tests.test_fourier_gpu import SmallScore, _argv, _tiny_config, alphas, rel, weights_for
from tests.test_modfourier_cpu import ModFourierRef

pytestmark = pytest.mark.gpu
SEQ, SEQ_NEXT = [250, 500, 750], [-1, 250, 500]
C = 3
DEV = 'cuda'
SHAPES = [(32, 1, 3), (32, 4, 3), (64, 3, 2), (64, 4, 2), (96, 2, 1)]
MODES = ['linear', 'modulus']


def maps_for(mode, d, K):
    from nhmc import operators
    if mode == 'linear':
        return operators.coil_maps(d, K)
    return operators.diffraction_masks(d, K, torch.Generator().manual_seed(700 + d + K))


def weights(kind, d):
    """'soft': the random non-binary map of tests/test_fourier_gpu.py (about 40 % zeros); 'ones'; 'hole': ones with a zeroed
    central 8 x 8 block; 'mri4': the Cartesian mask."""
    if kind == 'ones':
        return torch.ones(d, d)
    if kind == 'hole':
        w = torch.ones(d, d)
        w[d // 2 - 4:d // 2 + 4, d // 2 - 4:d // 2 + 4] = 0
        return w
    return weights_for(kind, d)


@functools.lru_cache(maxsize=None)
def make(mode, d, K, wkind='soft'):
    from nhmc import operators
    s, w, mod = maps_for(mode, d, K), weights(wkind, d), mode == 'modulus'
    return operators.ModulatedFourier(s, C, d, torch.device(DEV), weights=w, modulus=mod), ModFourierRef(s, C, d, w, modulus=mod)


def measured(ref, B):
    shape = (B, C, ref.K, ref.dim, ref.dim) if ref.modulus else (B, C, ref.K, 2, ref.dim, ref.dim)
    return (ref.W > 0).expand(shape).reshape(B, -1)


def inputs(ref, B, seed):
    """x = 0.8 randn (part of it outside [-1, 1]) and y = H(U(-1, 1)) + 0.1 randn, the noise on EVERY entry as the CLI draws it."""
    g = torch.Generator().manual_seed(seed)
    x = 0.8 * torch.randn(B, C, ref.dim, ref.dim, generator=g)
    y = ref.H(torch.rand(B, C, ref.dim, ref.dim, generator=g) * 2 - 1) + 0.1 * torch.randn(B, ref.M, generator=g)
    return x, y, g


# ---- 1: H against the oracle -------------------------------------------------------------------------------------
def check_H(mode, d, K, B):
    op, ref = make(mode, d, K)
    assert op.M == (1 if mode == 'modulus' else 2) * C * K * d * d and op.is_linear() == (mode == 'linear')
    x = torch.randn(B, C, d, d, generator=torch.Generator().manual_seed(d + K + B))
    got = op.H(x.cuda())
    want = ref.planes(x).reshape(B, -1)
    assert got.shape == (B, op.M) and got.dtype == torch.float32
    dev = rel(got, want)
    print(f'modfourier H {mode} d={d} K={K} B={B}: max deviation {dev:.2e} of the largest oracle value')
    assert dev < 1e-4
    assert bool((got.cpu()[~measured(ref, B)] == 0).all())                                 # W = 0: exactly zero
    if mode == 'modulus':
        assert op.forward(x.cuda()).equal(got)
        with pytest.raises(NotImplementedError):
            op.Ht(got)
    with pytest.raises(NotImplementedError):
        op.H_pinv(got)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('d,K,B', SHAPES)
def test_H_against_the_oracle(mode, d, K, B):
    check_H(mode, d, K, B)


# ---- 2: adjointness and the two isometries ---------------------------------------------------------------------------
@pytest.mark.parametrize('d,K,B', SHAPES)
def test_Ht_is_the_adjoint(d, K, B):
    op, ref = make('linear', d, K)
    g = torch.Generator().manual_seed(40 + d + K)
    x = torch.randn(B, C, d, d, generator=g).cuda()
    # v correlated with H(x), so that the inner product is not a small difference of large sums
    v = (torch.randn(B, op.M, generator=g).cuda() + 0.5 * op.H(torch.randn(B, C, d, d, generator=g).cuda() + x)).contiguous()
    htv = op.Ht(v)
    lhs = float((op.H(x).double() * v.double()).sum())
    rhs = float((x.reshape(B, -1).double() * htv.double()).sum())
    dev = rel(htv, ref.Ht(v.cpu()))
    print(f'modfourier d={d} K={K}: <H x, v> = {lhs:.6f}, <x, Ht v> = {rhs:.6f}, relative difference '
          f'{abs(lhs - rhs) / abs(lhs):.2e}; Ht vs oracle {dev:.2e}')
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)
    assert htv.shape == (B, C * d * d)
    assert dev < 1e-4


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('d,K,B', SHAPES)
def test_full_sampling_is_an_isometry(mode, d, K, B):
    """coil_maps: sum_k |S_k|^2 = 1, so ||H x||^2 = ||x||^2; diffraction_masks: |M_k| = 1, so ||H(x)||^2 = K ||x||^2."""
    op, _ = make(mode, d, K, 'ones')
    x = torch.randn(B, C, d, d, generator=torch.Generator().manual_seed(60 + d + K)).cuda()
    ratio = float((op.H(x).double() ** 2).sum() / (x.double() ** 2).sum())
    want = 1.0 if mode == 'linear' else float(K)
    print(f'modfourier {mode} d={d} K={K}: ||H x||^2 / ||x||^2 = {ratio:.8f}, expected {want}')
    assert abs(ratio - want) <= 1e-5 * want


# ---- 3: the data term --------------------------------------------------------------------------------------------
def check_data_term(mode, d, K, B, wkind='soft'):
    op, ref = make(mode, d, K, wkind)
    x, y, g = inputs(ref, B, 70 + d + K)
    m = measured(ref, B)
    xd, yd = x.cuda(), y.cuda()
    if mode == 'modulus':                                                             # the sgn singularity is tested exactly, below
        floor = float(ref.spectrum(x.clip(-1, 1)).abs().min())
        print(f'modfourier data term {mode} d={d} K={K} B={B}: min |Y| = {floor:.2e}')
        assert floor > 1e-5
    loss, grad = op.data_term(xd, yd, apply_clip=True)
    assert loss.dtype == torch.float64 and loss.shape == (B,) and grad.shape == x.shape
    # the loss: a float64 sum of the same fp32 residuals
    r = torch.where(m.cuda(), yd - op.H(xd.clip(-1, 1)), torch.zeros((), device=DEV))
    want_loss = (r * r).double().sum(dim=1)
    dl = float(((loss - want_loss).abs() / want_loss).max())
    # the gradient: float64 autograd through the oracle
    leaf = x.double().requires_grad_(True)
    res = torch.where(m, y.double() - ref.planes(leaf.clip(-1, 1)).reshape(B, -1), torch.zeros((), dtype=torch.float64))
    (want_grad,) = torch.autograd.grad((res ** 2).sum(), leaf)
    dg, dlo = rel(grad, want_grad), rel(loss, (res ** 2).sum(dim=1).detach())
    print(f'modfourier data term {mode} d={d} K={K} B={B}: loss rel {dl:.2e} (float64 sum of the same residuals), '
          f'loss vs oracle {dlo:.2e}, gradient {dg:.2e} of the largest oracle value')
    assert dl < 1e-6
    assert dg < 1e-4
    assert dlo < 1e-4
    # apply_clip: the clip is applied on the fly and masks the gradient
    big = xd * 3
    _, g_clip = op.data_term(big, yd, apply_clip=True)
    _, g_ref = op.data_term(big.clip(-1, 1), yd, apply_clip=False)
    assert torch.equal(g_clip, g_ref * ((big >= -1) & (big <= 1)))
    assert float(g_clip.abs().max()) > 0


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('d,K,B', SHAPES)
def test_data_term_loss_gradient_and_clip(mode, d, K, B):
    check_data_term(mode, d, K, B)


def test_H_and_data_term_at_256():
    """(256, 8, 1), once: the 128-tile first and last product of the chain, 48 planes of 4 x 4 tiles."""
    check_H('linear', 256, 8, 1)
    check_data_term('linear', 256, 8, 1)


@pytest.mark.parametrize('d,K', [(32, 4), (64, 3)])
def test_modulus_at_zero_has_a_zero_gradient(d, K):
    """|Y| = 0 everywhere: torch's sgn(0) = 0, so the gradient is exactly zero and the loss is the sum of y^2 where W > 0."""
    B = 2
    op, ref = make('modulus', d, K, 'hole')
    _, y, _ = inputs(ref, B, 130 + d)
    x = torch.zeros(B, C, d, d, device=DEV)
    e = torch.randn(B, 2 * C, d, d, generator=torch.Generator().manual_seed(1)).cuda()
    loss, grad = op.data_term(x, y.cuda(), apply_clip=True)
    assert bool((grad == 0).all()) and bool(torch.isfinite(loss).all())
    want = torch.where(measured(ref, B), y, torch.zeros(())).double().pow(2).sum(dim=1)
    assert float(((loss.cpu() - want).abs() / want).max()) < 1e-6
    at, atn = alphas(B)
    loss2, gx, ge = op.fused_last_vjp(x, torch.zeros_like(e), at, atn, y.cuda())      # the decode of (0, 0) is 0
    assert torch.equal(loss2, loss) and bool((gx == 0).all()) and bool((ge == 0).all())


# ---- 4: the unmeasured entries of y do not matter ----------------------------------------------------------------
@pytest.mark.parametrize('mode,wkind,d,K', [('linear', 'soft', 32, 4), ('linear', 'soft', 64, 3), ('modulus', 'hole', 32, 4),
                                            ('modulus', 'hole', 64, 3)])
def test_unmeasured_entries_never_reach_the_loss_or_the_gradient(mode, wkind, d, K):
    B = 3
    op, ref = make(mode, d, K, wkind)
    x, y, g = inputs(ref, B, 5 + d + K)
    x = x.cuda()
    e = torch.randn(B, 2 * C, d, d, generator=g).cuda()
    at, atn = alphas(B)
    hole = ~measured(ref, B)
    assert bool(hole.any()) and bool((~hole).any())

    def run(yy):
        yy = yy.cuda()
        return (*op.data_term(x, yy, apply_clip=True), *op.fused_last_vjp(x, e, at, atn, yy))

    base = run(y)
    assert all(bool(torch.isfinite(t).all()) for t in base) and float(base[1].abs().max()) > 0
    for fill in (7.5 * torch.randn(B, ref.M, generator=g), torch.full((B, ref.M), float('nan')),
                 torch.full((B, ref.M), float('inf')), torch.full((B, ref.M), float('-inf'))):
        for a, b in zip(base, run(torch.where(hole, fill, y))):
            assert torch.equal(a, b)
    # a NaN in ONE measured entry of chain 1: that chain's loss is NaN, the other chains keep their bits
    idx = int(torch.nonzero(~hole[1])[17])
    bad = y.clone()
    bad[1, idx] = float('nan')
    got = run(bad)
    for a, b in zip(base, got):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    assert bool(torch.isnan(got[0][1])) and bool(torch.isnan(got[2][1]))
    assert bool(torch.isnan(got[1][1]).any()) and bool(torch.isnan(got[3][1]).any())


# ---- 5: the fused last-step VJP ----------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('d,K,B,ec', [(32, 1, 3, 6), (32, 4, 3, 3), (64, 3, 2, 6), (64, 4, 2, 3), (96, 2, 1, 6), (96, 2, 1, 3)])
def test_fused_last_vjp_is_the_split_path_bit_for_bit(mode, d, K, B, ec):
    import nhmc.kernels as Kn
    op, ref = make(mode, d, K)
    _, y, g = inputs(ref, B, 90 + d + K)
    xt = (0.5 * torch.randn(B, C, d, d, generator=g)).cuda()
    e = torch.randn(B, ec, d, d, generator=g).cuda()
    y = y.cuda()
    at, atn = alphas(B)
    cur = Kn.ddim_mix_fwd(xt, e, at, atn, final_clip=True)['xt_next']
    loss_a, gd = op.data_term(cur, y, apply_clip=False)
    gx_a, ge_a = Kn.ddim_mix_bwd(gd, xt, e, at, atn, final_clip=True)
    loss_b, gx_b, ge_b = op.fused_last_vjp(xt, e, at, atn, y)
    loss_c, gx_c, ge_c = op.fused_last_vjp(xt, e, at, atn, y, xt_next=cur)
    assert torch.equal(gx_a, gx_b) and torch.equal(ge_a, ge_b) and torch.equal(gx_b, gx_c) and torch.equal(ge_b, ge_c)
    assert torch.equal(loss_a, loss_b) and torch.equal(loss_b, loss_c)
    assert float(gd.abs().max()) > 0 and bool(torch.isfinite(gd).all()) and float(gx_b.abs().max()) > 0


# ---- 6: a chain's bits do not depend on the batch it sits in ------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('d,K', [(32, 1), (32, 4), (64, 3), (96, 2)])
def test_a_chain_gives_the_same_bits_alone_and_inside_a_batch(mode, d, K):
    B = 3
    op, ref = make(mode, d, K)
    x, y, _ = inputs(ref, B, 110 + d + K)
    x, y = x.cuda(), y.cuda()
    Hx = op.H(x)
    loss, grad = op.data_term(x, y, apply_clip=True)
    for i in range(B):
        assert torch.equal(op.H(x[i:i + 1].contiguous()), Hx[i:i + 1])
        l1, g1 = op.data_term(x[i:i + 1].contiguous(), y[i:i + 1].contiguous(), apply_clip=True)
        assert torch.equal(l1, loss[i:i + 1]) and torch.equal(g1, grad[i:i + 1])


@pytest.mark.parametrize('mode', MODES)
def test_more_than_one_slab_of_chains(mode):
    """23 chains x 3 channels x 2 x 8 maps = 1104 modulated planes: the entries walk them as 21 chains, then 2.  Every entry
    against the oracle, and chains of both slabs against themselves alone."""
    import nhmc.kernels as Kn
    d, K, B = 32, 8, 23
    op, ref = make(mode, d, K)
    x, y, g = inputs(ref, B, 150)
    m = measured(ref, B)
    xd, yd = x.cuda(), y.cuda()
    Hx = op.H(xd)
    assert rel(Hx, ref.planes(x).reshape(B, -1)) < 1e-4
    loss, grad = op.data_term(xd, yd, apply_clip=True)
    leaf = x.double().requires_grad_(True)
    res = torch.where(m, y.double() - ref.planes(leaf.clip(-1, 1)).reshape(B, -1), torch.zeros((), dtype=torch.float64))
    (want_grad,) = torch.autograd.grad((res ** 2).sum(), leaf)
    assert rel(grad, want_grad) < 1e-4 and rel(loss, (res ** 2).sum(dim=1).detach()) < 1e-4
    if mode == 'linear':
        assert rel(op.Ht(yd), ref.Ht(y)) < 1e-4
    for i in (0, 20, 21, 22):
        assert torch.equal(op.H(xd[i:i + 1].contiguous()), Hx[i:i + 1])
        l1, g1 = op.data_term(xd[i:i + 1].contiguous(), yd[i:i + 1].contiguous(), apply_clip=True)
        assert torch.equal(l1, loss[i:i + 1]) and torch.equal(g1, grad[i:i + 1])
    e = torch.randn(B, 2 * C, d, d, generator=g).cuda()
    at, atn = alphas(B)
    cur = Kn.ddim_mix_fwd(xd, e, at, atn, final_clip=True)['xt_next']
    loss_a, gd = op.data_term(cur, yd, apply_clip=False)
    gx_a, ge_a = Kn.ddim_mix_bwd(gd, xd, e, at, atn, final_clip=True)
    loss_b, gx_b, ge_b = op.fused_last_vjp(xd, e, at, atn, yd, xt_next=cur)
    assert torch.equal(loss_a, loss_b) and torch.equal(gx_a, gx_b) and torch.equal(ge_a, ge_b)


# ---- 7: one unit map is the Fourier-sampling operator ------------------------------------------------------------------
@pytest.mark.parametrize('d,B', [(32, 3), (64, 2)])
def test_one_unit_map_is_fourier_sampling(d, B):
    from nhmc import operators
    w = weights_for('mri4', d)
    op = operators.ModulatedFourier(torch.ones(1, d, d), C, d, torch.device(DEV), weights=w)
    old, ref = operators.FourierSampling(w, C, d, torch.device(DEV)), FourierRef(w, C, d)
    g = torch.Generator().manual_seed(170 + d)
    x = (0.8 * torch.randn(B, C, d, d, generator=g)).cuda()
    y = (ref.H(torch.rand(B, C, d, d, generator=g) * 2 - 1) + 0.1 * torch.randn(B, ref.M, generator=g)).cuda()
    assert op.M == old.M
    (la, ga), (lb, gb) = op.data_term(x, y, apply_clip=True), old.data_term(x, y, apply_clip=True)
    devs = rel(op.H(x), old.H(x)), rel(la, lb), rel(ga, gb)
    print(f'modfourier K=1 S=1 vs FourierSampling d={d}: H {devs[0]:.2e}, loss {devs[1]:.2e}, gradient {devs[2]:.2e}')
    assert max(devs) < 1e-6


# ---- 8: the engine -----------------------------------------------------------------------------------------------
def engine_operator(mode, g):
    from nhmc import operators
    return operators.build_operator('mcmri4' if mode == 'linear' else 'cdp4', C, 32, torch.device(DEV), generator=g, n_coils=4)


@pytest.mark.parametrize('mode', MODES)
def test_engine_graph_replay_matches_eager(mode):
    """decode + gradient of a chunk replayed as a hipGraph == eager launches, with ragged chunks, also after the graph's
    static observation buffer was refilled with another chunk's y."""
    from nhmc import plugin, sampler
    d, B = 32, 3
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(12)
    op = engine_operator(mode, g)
    algo = plugin.HMC(SmallScore().cuda().requires_grad_(False), op, 0.1)
    eng = sampler.LeapfrogEngine(algo.score, op, osched.betas_fp32().cuda(), SEQ, SEQ_NEXT, dev, chunk=2)   # chunks of 2 and 1
    x = torch.randn(B, C, d, d, generator=g).cuda()
    y = (0.5 * torch.randn(B, op.M, generator=g)).cuda()
    eager = eng.decode_and_grad(x, y)
    assert float(eager[2].abs().max()) > 0
    for _ in range(2):                                                                # capture, then a pure replay
        graphed = eng.decode_and_grad(x, y, graph=True)
        for a, b in zip(eager, graphed):
            assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max()) + 1e-12
    x2, y2 = x * 0.5, y.flip(0).contiguous()                                          # new inputs AND observations, same graphs
    a = eng.decode_and_grad(x2, y2)
    b = eng.decode_and_grad(x2, y2, graph=True)
    assert all(float((u - v).abs().max()) <= 1e-5 * float(u.abs().max()) + 1e-12 for u, v in zip(a, b))


@pytest.mark.parametrize('mode', MODES)
def test_trajectory_does_not_depend_on_the_score_chunking(tiny_score, mode):
    from nhmc import plugin, sampler
    d, B, L = 32, 5, 4
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(43)
    op = engine_operator(mode, g)
    x = torch.randn(B, C, d, d, generator=g).cuda()
    p = torch.randn(B, C, d, d, generator=g).cuda()
    y = (op.H((torch.rand(B, C, d, d, generator=g) * 2 - 1).cuda()) + 0.1 * torch.randn(B, op.M, generator=g).cuda()).contiguous()
    eps, sig = np.array([0.05, 0.04, 0.03, 0.0, 0.05]), np.array([1.7, 0.9, 0.5, 0.5, 1.0])     # chain 3 frozen (eps_eff = 0)
    outs = []
    for chunk in (None, 2, 3):
        algo = plugin.HMC(copy.deepcopy(tiny_score).cuda(), op, 0.1)
        eng = sampler.LeapfrogEngine(algo.score, op, osched.betas_fp32().cuda(), SEQ, SEQ_NEXT, dev, chunk=chunk)
        st = sampler.ChainState(B, 1.0, 0.05, DEV)
        st['eps_eff'].copy_(torch.as_tensor(eps))
        st['sigma_y'].copy_(torch.as_tensor(sig))
        x0 = x.clone()
        got = sampler.run_trajectory(eng, x0, p.clone(), y, st, 1.0, L)
        assert torch.equal(x0, x)
        outs.append({k: got[k].clone() for k in ('x_prop', 'p', 'xt', 'loss', 'H0', 'H1')})
    for other in outs[1:]:
        for k, v in outs[0].items():
            assert torch.equal(v, other[k]) or rel(other[k], v) < 1e-6, k
    assert torch.equal(outs[0]['x_prop'][3], x[3])


@pytest.mark.parametrize('mode,sig,eps', [('linear', (1.7, 0.1), (0.05, 0.01)), ('modulus', (1.7, 0.5), (0.05, 0.02))])
def test_trajectory_matches_the_float64_oracle(tiny_score, mode, sig, eps):
    """32 x 32, K = 4, L = 20, the float64 oracle operator and the float64 tiny score on both sides; one chain per (sigma_y,
    eps).  The oracle subtracts on every entry, so its y is zero-noise where W = 0."""
    from nhmc import plugin, sampler
    d, B, L = 32, 2, 20
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(22)
    op = engine_operator(mode, g)
    ref = ModFourierRef(op.maps, C, d, op.weights, modulus=mode == 'modulus')
    x, p = torch.randn(B, C, d, d, generator=g), torch.randn(B, C, d, d, generator=g)
    y = ref.H(torch.rand(B, C, d, d, generator=g) * 2 - 1) + 0.1 * torch.randn(B, ref.M, generator=g) * measured(ref, B)
    eps, sig = np.array(eps), np.array(sig)
    want = hmc_ref.trajectory(x, p.clone(), osched.betas_fp32(), SEQ, SEQ_NEXT, F64Score(tiny_score), ref, y,
                              sigma_y=sig, eps=eps, m=1.0, L=L)
    algo = plugin.HMC(F64Score(tiny_score).to(dev), op, 0.1)
    eng = sampler.LeapfrogEngine(algo.score, op, osched.betas_fp32().to(dev), SEQ, SEQ_NEXT, dev)
    st = sampler.ChainState(B, 1.0, 0.05, dev)
    st['eps_eff'].copy_(torch.as_tensor(eps))
    st['sigma_y'].copy_(torch.as_tensor(sig))
    got = sampler.run_trajectory(eng, x.to(dev), p.to(dev).clone(), y.to(dev), st, 1.0, L)
    for i in range(B):
        ex = rel(got['x_prop'][i], want['x'][i])
        dH = float((got['H1'] - got['H0'])[i])
        dH_ref = float((want['H1'] - want['H0'])[i])
        print(f'modfourier {mode} trajectory sigma_y {sig[i]} eps {eps[i]}: end position rel err {ex:.2e}, dH {dH:+.5f} vs oracle {dH_ref:+.5f}')
        assert ex < 1e-4
        assert abs(dH - dH_ref) < 0.05
    assert float((want['x'] - x).abs().max()) > 1e-3                                  # the chains moved


# ---- 9: the command line -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['coils', 'file', 'cdp'])
def test_cli_end_to_end(tmp_path, monkeypatch, case):
    from nhmc import cli, operators
    _tiny_config(tmp_path)
    monkeypatch.chdir(tmp_path)
    if case == 'coils':
        argv = _argv(tmp_path, 'mcmri4', '--save_images', '--coils', '4')
    elif case == 'file':
        np.save(tmp_path / 's.npy', operators.coil_maps(32, 3).numpy() * 0.7)
        argv = _argv(tmp_path, 'mcmri4', '--save_images', '--coil_maps', str(tmp_path / 's.npy'))
    else:
        argv = _argv(tmp_path, 'cdp4', '--save_images')
    # the vendor library's deterministic mode, for the reason tests/test_nonlinear_gpu.py::test_cli_end_to_end gives
    with torch.backends.cudnn.flags(deterministic=True, benchmark=False):
        table = cli.main(argv)
        assert table.shape == (2, 3) and bool(torch.isfinite(table).all())
        for name in ('kspace_mask.png', 'coil_maps.png'):
            assert (tmp_path / 'out' / name).is_file() == (case != 'cdp')
        assert torch.equal(table, cli.main(argv))                                     # same bits on a second call


def test_cli_coil_maps_go_only_with_mcmri(tmp_path, monkeypatch):
    from nhmc import cli
    _tiny_config(tmp_path)
    monkeypatch.chdir(tmp_path)
    np.save(tmp_path / 's.npy', np.ones((2, 32, 32), dtype=np.complex64))
    np.save(tmp_path / 'small.npy', np.ones((2, 16, 16), dtype=np.complex64))
    np.save(tmp_path / 'm.npy', np.ones((32, 32), dtype=np.float32))
    for deg in ('sr4', 'mri4', 'cdp4'):
        with pytest.raises(SystemExit, match='only with'):
            cli.main(_argv(tmp_path, deg, '--coil_maps', str(tmp_path / 's.npy')))
    with pytest.raises(SystemExit, match='16 x 16.*32 x 32'):
        cli.main(_argv(tmp_path, 'mcmri4', '--coil_maps', str(tmp_path / 'small.npy')))
    with pytest.raises(SystemExit, match='go together'):                              # as before this operator
        cli.main(_argv(tmp_path, 'mcmri4', '--kspace_mask', str(tmp_path / 'm.npy')))
    with pytest.raises(SystemExit, match='1 to 32|n_coils'):
        cli.main(_argv(tmp_path, 'mcmri4', '--coils', '33'))


# ---- 10: the C ABI's argument checks -----------------------------------------------------------------------------
def test_abi_argument_checks():
    """Pointers that are never dereferenced: every refusal comes before any launch."""
    import nhmc
    lib = nhmc._lib.load()
    P = ctypes.c_void_p
    null, a16, a4 = P(0), P(0x1000), P(0x1004)
    ARG, ALIGN, SHAPE = 1, 2, 3
    ok = (2, 3, 4, 32)                                                                # (n_chains, channels, n_maps, dim)
    bad_dims = [(2, 3, 4, 48), (2, 3, 4, 0), (0, 3, 4, 32), (2, 0, 4, 32), (2, 3, 0, 32), (2, 3, 33, 32), (2, 3, -1, 32),
                (30000, 3, 4, 32), (1366, 3, 8, 32)]                                  # 1366 x 3 x 16 = 65568 planes
    # loss_ws (double*) and the alpha-bar arrays need no 16-byte alignment: with a misaligned pointer there the call
    # would LAUNCH on memory that does not exist, so they are probed with null only
    def H(ptrs, dims, modulus=0):                                                     # x maps fac w | modulus | out tmp
        return lib.nhmc_modfourier_H(*ptrs[:4], modulus, *ptrs[4:], *dims, null)
    for i in range(6):
        ptrs = [a16] * 6
        ptrs[i] = null
        assert H(ptrs, ok) == ARG and H(ptrs, ok, 1) == ARG
        ptrs[i] = a4
        assert H(ptrs, ok) == ALIGN and H(ptrs, ok, 1) == ALIGN
        assert H(ptrs, (1365, 3, 8, 32)) == ALIGN                                     # 65520 planes pass the shape check
        for bad in bad_dims:
            assert H(ptrs, bad) == SHAPE                                              # SHAPE before ALIGN
    assert H([a16] * 6, ok, 2) == ARG and H([a16] * 6, ok, -1) == ARG

    for i in range(6):                                                                # v maps fac w out tmp
        ptrs = [a16] * 6
        ptrs[i] = null
        assert lib.nhmc_modfourier_Ht(*ptrs, *ok, null) == ARG
        ptrs[i] = a4
        assert lib.nhmc_modfourier_Ht(*ptrs, *ok, null) == ALIGN
        for bad in bad_dims:
            assert lib.nhmc_modfourier_Ht(*ptrs, *bad, null) == SHAPE

    def data(ptrs, dims, modulus=0, clip=1):                                          # xt y maps fac w | modulus clip | g_xt loss_ws tmp
        return lib.nhmc_data_modfourier(*ptrs[:5], modulus, clip, *ptrs[5:], *dims, null)
    for i in range(8):
        ptrs = [a16] * 8
        ptrs[i] = null
        assert data(ptrs, ok) == ARG and data(ptrs, ok, 1) == ARG
        if i != 6:                                                                    # 6: loss_ws
            ptrs[i] = a4
            assert data(ptrs, ok) == ALIGN and data(ptrs, ok, 1, clip=0) == ALIGN
    for bad in bad_dims:
        assert data([a16] * 8, bad) == SHAPE
    assert data([a16] * 8, ok, 2) == ARG

    def vjp(ptrs, dims, modulus=0, ec=6):                  # xt_next y maps fac w | modulus | xt e | ec | at at_next g_xt g_e loss_ws tmp
        return lib.nhmc_data_modfourier_vjp(*ptrs[:5], modulus, *ptrs[5:7], ec, *ptrs[7:], *dims, null)
    for i in range(13):
        ptrs = [a16] * 13
        ptrs[i] = null
        assert vjp(ptrs, ok) == ARG and vjp(ptrs, ok, 1) == ARG
        if i not in (7, 8, 11):                                                       # at, at_next, loss_ws
            ptrs[i] = a4
            assert vjp(ptrs, ok) == ALIGN and vjp(ptrs, ok, 1, ec=3) == ALIGN
    for bad in bad_dims:
        assert vjp([a16] * 13, bad) == SHAPE
    for ec in (0, 4, 5, 9):
        assert vjp([a16] * 13, ok, ec=ec) == SHAPE
    assert vjp([a16] * 13, ok, 2) == ARG
    assert lib.nhmc_modfourier_tiles(3, 4, 32) == 12 and lib.nhmc_modfourier_tiles(3, 8, 256) == 1536
    assert lib.nhmc_modfourier_tmp_floats(2, 3, 4, 32) == 7 * 48 * 1024               # 7 d^2 floats per modulated plane
    assert lib.nhmc_modfourier_tmp_floats(64, 3, 8, 256) == 7 * 21 * 48 * 65536       # slabs of 21 chains cap the scratch
    # the binding's own checks
    import nhmc.kernels as Kn
    op, _ = make('linear', 32, 4)
    x = torch.zeros(2, C, 32, 32, device=DEV)
    for call in (lambda: Kn.modfourier_H(x, op.S, op.factors, op.W[:16]),
                 lambda: Kn.modfourier_H(x, op.S[:, :1], op.factors, op.W),
                 lambda: Kn.modfourier_H(x, op.S[:, :, :16], op.factors, op.W),
                 lambda: Kn.data_modfourier(x, torch.zeros(2, C, 4, 32, 32, device=DEV), op.S, op.factors, op.W),
                 lambda: Kn.data_modfourier(x, torch.zeros(2, C, 4, 2, 32, 32, device=DEV), op.S, op.factors, op.W, modulus=True),
                 lambda: Kn.modfourier_Ht(torch.zeros(2, C, 3, 2, 32, 32, device=DEV), op.S, op.factors, op.W),
                 lambda: Kn.modfourier_H(x.cpu(), op.S, op.factors, op.W),
                 lambda: Kn.modfourier_H(x, op.S.double(), op.factors, op.W),
                 lambda: Kn.modfourier_H(torch.zeros(1400, C, 32, 32, device=DEV), op.S.repeat(2, 1, 1, 1), op.factors, op.W)):
        with pytest.raises(nhmc._lib.NhmcError):
            call()
