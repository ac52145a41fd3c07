"""GPU: the Fourier-sampling operator (`--deg mri<R>`, `--deg fourier`) through the C ABI, against the float64 oracle of
tests/test_fourier_cpu.py (torch.fft, fftshift / ifftshift, norm='ortho').

The kernels run the centred DFT as fp32-MFMA sandwiches where the oracle runs an FFT in float64: no bit identity with
it; the bounds are the project's (1e-4 of the largest oracle value for H and the gradient, 1e-5 relative for the
adjointness, 1e-6 for the loss against a float64 sum of the same residuals) and every measured deviation is printed.
What IS bit for bit: the fused last-step VJP against the split path, the clip mask, a chain alone against the same chain
in a batch, and the indifference to whatever the unmeasured entries of y hold.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

from oracle import hmc_ref, schedule as osched
from oracle.tiny_score import F64Score
from tests.test_fourier_cpu import FourierRef

pytestmark = pytest.mark.gpu
SEQ, SEQ_NEXT = [250, 500, 750], [-1, 250, 500]
C = 3
DEV = 'cuda'


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def weights_for(kind, d):
    """'mri4': the CLI's Cartesian mask; 'soft': a random non-binary map with about 40 % zeros."""
    from nhmc import operators
    g = torch.Generator().manual_seed(900 + d)
    if kind == 'mri4':
        return operators.cartesian_mask(d, 4, g)
    return (0.25 + 1.5 * torch.rand(d, d, generator=g)) * (torch.rand(d, d, generator=g) > 0.4)


def make(kind, d):
    from nhmc import operators
    w = weights_for(kind, d)
    return operators.FourierSampling(w, C, d, torch.device(DEV)), FourierRef(w, C, d)


def alphas(B):
    b = osched.betas_fp32()
    return osched.alpha_bar(b, torch.full((B,), 250)).cuda(), osched.alpha_bar(b, torch.full((B,), -1)).cuda()


def observation(ref, B, g, sigma=0.1):
    """H(truth) + noise, the noise on EVERY entry as the CLI draws it -> float32 [B, M] on the host."""
    truth = torch.rand(B, C, ref.dim, ref.dim, generator=g) * 2 - 1
    return ref.H(truth) + sigma * torch.randn(B, ref.M, generator=g)


def measured(ref, B):
    return (ref.W > 0)[None, None, None].expand(B, C, 2, ref.dim, ref.dim).reshape(B, -1)


# ---- 1: H against the oracle -------------------------------------------------------------------------------------
# d = 32: the 32-tile k_cgemm, one tile per plane; 64: the 64-tile one; 96: 3 x 3 tiles of 32; 256: 4 x 4 tiles of 64.
# The launch grid is B * C * tiles: 24 / 216 blocks are renumbered across the XCDs (a multiple of 8), 9 / 27 are not.
@pytest.mark.parametrize('kind', ['mri4', 'soft'])
@pytest.mark.parametrize('d,B', [(32, 8), (32, 3), (64, 8), (64, 3), (96, 8), (96, 1), (256, 1)])
def test_H_against_the_oracle(kind, d, B):
    op, ref = make(kind, d)
    assert op.M == 2 * C * d * d and op.is_linear()
    x = torch.randn(B, C, d, d, generator=torch.Generator().manual_seed(d + B))
    got = op.H(x.cuda())
    want = ref.planes(x).reshape(B, -1)
    assert got.shape == (B, op.M) and got.dtype == torch.float32
    dev = rel(got, want)
    print(f'fourier H {kind} d={d} B={B}: max deviation {dev:.2e} of the largest oracle value')
    assert dev < 1e-4
    assert bool((got.cpu()[~measured(ref, B)] == 0).all())                                 # W = 0: exactly zero


# ---- 2: adjointness ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,d,B', [('mri4', 32, 3), ('soft', 64, 2), ('soft', 96, 2), ('mri4', 256, 1)])
def test_Ht_is_the_adjoint(kind, d, B):
    op, ref = make(kind, d)
    g = torch.Generator().manual_seed(40 + d)
    x = torch.randn(B, C, d, d, generator=g).cuda()
    # v correlated with H(x), so that the inner product is not a small difference of large sums
    v = (torch.randn(B, op.M, generator=g).cuda() + 0.5 * op.H(torch.randn(B, C, d, d, generator=g).cuda() + x)).contiguous()
    lhs = float((op.H(x).double() * v.double()).sum())
    rhs = float((x.reshape(B, -1).double() * op.Ht(v).double()).sum())
    print(f'fourier {kind} d={d}: <H x, v> = {lhs:.6f}, <x, Ht v> = {rhs:.6f}, relative difference {abs(lhs - rhs) / abs(lhs):.2e}')
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)
    assert op.Ht(v).shape == (B, C * d * d)
    assert rel(op.Ht(v), ref.Ht(v.cpu())) < 1e-4
    with pytest.raises(NotImplementedError):
        op.H_pinv(v)


# ---- 3: the unmeasured entries of y do not matter ----------------------------------------------------------------
@pytest.mark.parametrize('kind,d', [('mri4', 32), ('soft', 64)])
def test_unmeasured_entries_never_reach_the_loss_or_the_gradient(kind, d):
    B = 3
    op, ref = make(kind, d)
    g = torch.Generator().manual_seed(5 + d)
    x = (0.8 * torch.randn(B, C, d, d, generator=g)).cuda()
    e = torch.randn(B, 2 * C, d, d, generator=g).cuda()
    at, atn = alphas(B)
    y = observation(ref, B, g)
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


# ---- 4: the data term --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,d,B', [('mri4', 32, 3), ('soft', 64, 2), ('soft', 96, 1), ('mri4', 256, 1)])
def test_data_term_loss_gradient_and_clip(kind, d, B):
    op, ref = make(kind, d)
    g = torch.Generator().manual_seed(70 + d)
    x = 0.8 * torch.randn(B, C, d, d, generator=g)                                    # part of it outside [-1, 1]
    y = observation(ref, B, g)
    m = measured(ref, B)
    xd, yd = x.cuda(), y.cuda()
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
    dg = rel(grad, want_grad)
    print(f'fourier data term {kind} d={d} B={B}: loss rel {dl:.2e} (float64 sum of the same residuals), '
          f'loss vs oracle {rel(loss, (res ** 2).sum(dim=1).detach()):.2e}, gradient {dg:.2e} of the largest oracle value')
    assert dl < 1e-6
    assert dg < 1e-4
    assert rel(loss, (res ** 2).sum(dim=1).detach()) < 1e-4
    # apply_clip: the clip is applied on the fly and masks the gradient
    big = xd * 3
    _, g_clip = op.data_term(big, yd, apply_clip=True)
    _, g_ref = op.data_term(big.clip(-1, 1), yd, apply_clip=False)
    assert torch.equal(g_clip, g_ref * ((big >= -1) & (big <= 1)))
    assert float(g_clip.abs().max()) > 0


# ---- 5: the fused last-step VJP ----------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,d,B,ec', [('mri4', 32, 3, 6), ('soft', 64, 2, 3), ('soft', 96, 1, 6), ('mri4', 256, 1, 6)])
def test_fused_last_vjp_is_the_split_path_bit_for_bit(kind, d, B, ec):
    import nhmc.kernels as K
    op, ref = make(kind, d)
    g = torch.Generator().manual_seed(90 + d)
    xt = (0.5 * torch.randn(B, C, d, d, generator=g)).cuda()
    e = torch.randn(B, ec, d, d, generator=g).cuda()
    y = observation(ref, B, g).cuda()
    at, atn = alphas(B)
    cur = K.ddim_mix_fwd(xt, e, at, atn, final_clip=True)['xt_next']
    loss_a, gd = op.data_term(cur, y, apply_clip=False)
    gx_a, ge_a = K.ddim_mix_bwd(gd, xt, e, at, atn, final_clip=True)
    loss_b, gx_b, ge_b = op.fused_last_vjp(xt, e, at, atn, y)
    loss_c, gx_c, ge_c = op.fused_last_vjp(xt, e, at, atn, y, xt_next=cur)
    assert torch.equal(gx_a, gx_b) and torch.equal(ge_a, ge_b) and torch.equal(gx_b, gx_c) and torch.equal(ge_b, ge_c)
    assert torch.equal(loss_a, loss_b) and torch.equal(loss_b, loss_c)
    assert float(gd.abs().max()) > 0 and bool(torch.isfinite(gd).all()) and float(gx_b.abs().max()) > 0


# ---- 6: a chain's bits do not depend on the batch it sits in ------------------------------------------------------
@pytest.mark.parametrize('kind,d', [('mri4', 32), ('soft', 64), ('soft', 96)])
def test_a_chain_gives_the_same_bits_alone_and_inside_a_batch(kind, d):
    B = 3
    op, ref = make(kind, d)
    g = torch.Generator().manual_seed(110 + d)
    x = (0.8 * torch.randn(B, C, d, d, generator=g)).cuda()
    y = observation(ref, B, g).cuda()
    Hx = op.H(x)
    loss, grad = op.data_term(x, y, apply_clip=True)
    for i in range(B):
        assert torch.equal(op.H(x[i:i + 1].contiguous()), Hx[i:i + 1])
        l1, g1 = op.data_term(x[i:i + 1].contiguous(), y[i:i + 1].contiguous(), apply_clip=True)
        assert torch.equal(l1, loss[i:i + 1]) and torch.equal(g1, grad[i:i + 1])


# ---- 7: the engine -----------------------------------------------------------------------------------------------
class SmallScore(torch.nn.Module):
    """A capturable score stand-in (no host->device copies in forward), as in tests/test_graph_gpu.py."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.a = torch.nn.Conv2d(3, 8, 3, padding=1)
        self.b = torch.nn.Conv2d(8, 6, 3, padding=1)

    def forward(self, x, t):
        return self.b(torch.tanh(self.a(x)) * (1.0 + t.view(-1, 1, 1, 1) / 1000.0))


def test_engine_graph_replay_matches_eager():
    """decode + gradient of a chunk replayed as a hipGraph == eager launches, with ragged chunks, also after the graph's
    static observation buffer was refilled with another chunk's y."""
    from nhmc import operators, plugin, sampler
    d, B = 32, 3
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(12)
    op = operators.build_operator('mri4', C, d, dev, generator=g)
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


def test_trajectory_does_not_depend_on_the_score_chunking(tiny_score):
    from nhmc import operators, plugin, sampler
    d, B, L = 32, 5, 4
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(43)
    op = operators.build_operator('mri4', C, d, dev, generator=g)
    x = torch.randn(B, C, d, d, generator=g).cuda()
    p = torch.randn(B, C, d, d, generator=g).cuda()
    y = (op.H((torch.rand(B, C, d, d, generator=g) * 2 - 1).cuda()) + 0.1 * torch.randn(B, op.M, generator=g).cuda()).contiguous()
    eps, sig = np.array([0.05, 0.04, 0.03, 0.0, 0.05]), np.array([1.7, 0.9, 0.1, 0.5, 1.0])     # chain 3 frozen (eps_eff = 0)
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


# ---- 8: one trajectory against the oracle ------------------------------------------------------------------------
def test_trajectory_matches_the_float64_oracle(tiny_score):
    """32 x 32, L = 20, the float64 oracle operator and the float64 tiny score on both sides; chain 0 at (sigma_y, eps) =
    (1.7, 0.05), chain 1 at (0.1, 0.01).  The oracle subtracts on every entry, so its y is zero-noise where W = 0."""
    from nhmc import operators, plugin, sampler
    d, B, L = 32, 2, 20
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(22)
    w = operators.cartesian_mask(d, 4, g)
    op, ref = operators.FourierSampling(w, C, d, dev), FourierRef(w, C, d)
    x, p = torch.randn(B, C, d, d, generator=g), torch.randn(B, C, d, d, generator=g)
    y = ref.H(torch.rand(B, C, d, d, generator=g) * 2 - 1) + 0.1 * torch.randn(B, ref.M, generator=g) * measured(ref, B)
    eps, sig = np.array([0.05, 0.01]), np.array([1.7, 0.1])
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
        print(f'fourier trajectory sigma_y {sig[i]} eps {eps[i]}: end position rel err {ex:.2e}, dH {dH:+.5f} vs oracle {dH_ref:+.5f}')
        assert ex < 1e-4
        assert abs(dH - dH_ref) < 0.05
    assert float((want['x'] - x).abs().max()) > 1e-3                                  # the chains moved


# ---- 9: the command line -----------------------------------------------------------------------------------------
def _tiny_config(tmp_path):
    import yaml
    cfgdir = tmp_path / 'configs'
    cfgdir.mkdir()
    cfg = {'data': {'dataset': 'tiny', 'image_size': 32, 'channels': 3, 'rescaled': True},
           'model': dict(image_size=32, num_channels=32, num_res_blocks=1, channel_mult='1,2', learn_sigma=True,
                         class_cond=False, use_checkpoint=False, attention_resolutions='16', num_heads=4,
                         num_head_channels=16, num_heads_upsample=-1, use_scale_shift_norm=True, dropout=0.0,
                         resblock_updown=True, use_fp16=False, use_new_attention_order=False, model_path=''),
           'diffusion': {'beta_schedule': 'linear', 'beta_start': 1e-4, 'beta_end': 0.02, 'num_diffusion_timesteps': 1000}}
    (cfgdir / 'config_tiny.yml').write_text(yaml.safe_dump(cfg))


def _argv(tmp_path, deg, *more):
    return ['--dataset', 'tiny', '--algo', 'hmc', '--timesteps', '3', '--deg', deg, '--sigma_0', '0.05', '-i', str(tmp_path / 'out'),
            '--tau', '0.01', '--epsilon', '0.005', '--synthetic', '2', '--chains', '2', '--philox', '--hmc_epochs', '2',
            '--hmc_sampling', '2', *more]             # a short schedule of short trajectories: the test is about the command line


@pytest.mark.parametrize('deg', ['mri4', 'fourier'])
def test_cli_end_to_end(tmp_path, monkeypatch, deg):
    from nhmc import cli
    _tiny_config(tmp_path)
    monkeypatch.chdir(tmp_path)
    more = ['--save_images']
    if deg == 'fourier':
        np.save(tmp_path / 'm.npy', weights_for('soft', 32).numpy())
        more += ['--kspace_mask', str(tmp_path / 'm.npy')]
    argv = _argv(tmp_path, deg, *more)
    # the vendor library's deterministic mode, for the reason tests/test_nonlinear_gpu.py::test_cli_end_to_end gives
    with torch.backends.cudnn.flags(deterministic=True, benchmark=False):
        table = cli.main(argv)
        assert table.shape == (2, 3) and bool(torch.isfinite(table).all())
        assert (tmp_path / 'out' / 'kspace_mask.png').is_file()
        assert torch.equal(table, cli.main(argv))                                     # same bits on a second call


def test_cli_flag_and_degradation_go_together(tmp_path, monkeypatch):
    from nhmc import cli
    _tiny_config(tmp_path)
    monkeypatch.chdir(tmp_path)
    np.save(tmp_path / 'm.npy', np.ones((32, 32), dtype=np.float32))
    np.save(tmp_path / 'small.npy', np.ones((16, 16), dtype=np.float32))
    with pytest.raises(SystemExit, match='go together'):
        cli.main(_argv(tmp_path, 'sr4', '--kspace_mask', str(tmp_path / 'm.npy')))
    with pytest.raises(SystemExit, match='go together'):
        cli.main(_argv(tmp_path, 'mri4', '--kspace_mask', str(tmp_path / 'm.npy')))
    with pytest.raises(SystemExit, match='go together'):
        cli.main(_argv(tmp_path, 'fourier'))
    with pytest.raises(SystemExit, match='16 x 16'):
        cli.main(_argv(tmp_path, 'fourier', '--kspace_mask', str(tmp_path / 'small.npy')))


# ---- 10: the C ABI's argument checks -----------------------------------------------------------------------------
def test_abi_argument_checks():
    """Pointers that are never dereferenced: every refusal comes before any launch."""
    import nhmc
    lib = nhmc._lib.load()
    P = ctypes.c_void_p
    null, a16, a4 = P(0), P(0x1000), P(0x1004)
    ARG, ALIGN, SHAPE = 1, 2, 3

    bad_dims = [(2, 3, 48), (2, 3, 0), (0, 3, 32), (2, 0, 32), (30000, 3, 32)]    # (n_chains, channels, dim)
    # loss_ws (double*) and the alpha-bar arrays need no 16-byte alignment: with a misaligned pointer there the call
    # would LAUNCH on memory that does not exist, so they are probed with null only
    for i in range(5):                                                                # x fac w out tmp
        ptrs = [a16] * 5
        ptrs[i] = null
        assert lib.nhmc_fourier_H(*ptrs, 2, 3, 32, null) == ARG
        ptrs[i] = a4
        assert lib.nhmc_fourier_H(*ptrs, 2, 3, 32, null) == ALIGN
        for bad in bad_dims:
            assert lib.nhmc_fourier_H(*ptrs, *bad, null) == SHAPE                     # SHAPE before ALIGN, as the phase entries

    def data(ptrs, dims, clip=1):                                                     # xt y fac w | clip | g_xt loss_ws tmp
        return lib.nhmc_data_fourier(*ptrs[:4], clip, *ptrs[4:], *dims, null)
    for i in range(7):
        ptrs = [a16] * 7
        ptrs[i] = null
        assert data(ptrs, (2, 3, 32)) == ARG
        if i != 5:                                                                    # 5: loss_ws
            ptrs[i] = a4
            assert data(ptrs, (2, 3, 32)) == ALIGN and data(ptrs, (2, 3, 32), clip=0) == ALIGN
    for bad in bad_dims:
        assert data([a16] * 7, bad) == SHAPE

    def vjp(ptrs, dims, ec=6):                                                        # xt_next y fac w xt e | ec | at at_next g_xt g_e loss_ws tmp
        return lib.nhmc_data_fourier_vjp(*ptrs[:6], ec, *ptrs[6:], *dims, null)
    for i in range(12):
        ptrs = [a16] * 12
        ptrs[i] = null
        assert vjp(ptrs, (2, 3, 32)) == ARG
        if i not in (6, 7, 10):                                                       # at, at_next, loss_ws
            ptrs[i] = a4
            assert vjp(ptrs, (2, 3, 32)) == ALIGN and vjp(ptrs, (2, 3, 32), ec=3) == ALIGN
    for bad in bad_dims:
        assert vjp([a16] * 12, bad) == SHAPE
    for ec in (0, 4, 5, 9):
        assert vjp([a16] * 12, (2, 3, 32), ec=ec) == SHAPE
    # the binding's own checks
    import nhmc.kernels as K
    op, _ = make('mri4', 32)
    x = torch.zeros(2, C, 32, 32, device=DEV)
    with pytest.raises(nhmc._lib.NhmcError):
        K.fourier_H(x, op.factors, op.W[:16])
    with pytest.raises(nhmc._lib.NhmcError):
        K.data_fourier(x, torch.zeros(2, C, 32, 32, device=DEV), op.factors, op.W)
    with pytest.raises(nhmc._lib.NhmcError):
        K.fourier_H(x.cpu(), op.factors, op.W)
    with pytest.raises(nhmc._lib.NhmcError):
        K.fourier_H(x, op.factors, op.W.double())
