"""GPU: the MFMA GEMM kernels of csrc/spectral_gemm.hip (k_sgemm at T = 32 / 64 / 128, k_pair256) on multi-tile and
rectangular grids, on both branches of the block remap, with generic operator data (oracle/gemm_cases.py; the tile path
every case reaches is held by tests/test_gemm_cases_cpu.py).

References are float64, computed on the CPU from the same fp32 inputs; the metric is max|err| / max|ref| (rel() of
tests/test_kernels_gpu.py).  Bounds: operator maps, gradients and losses take the MFMA-chain bound of that file, 2e-5; the
plain fp32 CPU evaluation of the same formulas sits at <= 1.1e-6 from float64 on these inputs (the CPU module prints
it), so the reference has 20x headroom.  The four-product (projected) form is held to what tests/test_spectral_proj_gpu.py
allows against float64: gradient 3e-5 (here in both that file's norm metric and the max metric), loss 1e-5.
Everything the arithmetic fixes bit for bit is compared bit for bit: the fused "data term + last DDIM step" epilogues
against the two-kernel path, with a DIFFERENT step per chain and the score output with C and with 2C channels, and
a zero-padded problem (another tile size, another kernel) against the unpadded one.

Score outputs and their gradients with C channels live at the front of a buffer twice their size whose tail holds a
sentinel: an epilogue that strides chains by 2C channels instead of e_channels then reads and writes the tail, which the
tests see, instead of memory past the tensor.
"""
import functools

import pytest
import torch

from oracle import gemm_cases as gc

pytestmark = pytest.mark.gpu
BOUND = 2e-5
SENTINEL = 7.0
rel = gc.rel
ids = lambda cases: [c.id for c in cases]


def dev(t):
    return t.cuda().contiguous()


def norm_rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def guarded(shape, fill=None):
    """-> (t, tail): a contiguous tensor of `shape` at the front of a buffer of twice its size; the tail holds SENTINEL."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((2 * n,), SENTINEL, dtype=torch.float32, device='cuda')
    t = buf[:n].view(shape)
    if fill is not None:
        t.copy_(fill)
    return t, buf[n:]


def top_left(t, d):
    return t[..., :d, :d]


def zero_outside(t, d):
    return not bool(t[..., d:, :].any()) and not bool(t[..., :, d:].any())


def fused_equals_two_kernels(op, xt, e, at, an, y, loss_exact=True):
    """fused_last_vjp == data term on the clipped decode, then ddim_mix_bwd: bit for bit (the form of test_fused_gpu.py).
    e and the fused g_e are guarded; beyond the first C channels a caller's g_e buffer is left alone."""
    import nhmc.kernels as K
    C = xt.shape[1]
    e, e_tail = guarded(e.shape, e)
    cur = K.ddim_mix_fwd(xt, e, at, an, final_clip=True)['xt_next']
    loss_a, g = op.data_term(cur, y, apply_clip=False)
    gx_a, ge_a = K.ddim_mix_bwd(g, xt, e, at, an, final_clip=True)
    buf, tail = guarded(e.shape)
    extra = dict(xt_next=cur) if getattr(op, 'fused_wants_decode', False) else {}
    loss_b, gx_b, ge_b = op.fused_last_vjp(xt, e, at, an, y, g_e_out=buf, **extra)
    torch.cuda.synchronize()
    assert ge_b is buf
    assert bool((tail == SENTINEL).all()) and bool((e_tail == SENTINEL).all()), 'the epilogue wrote past g_e'
    assert bool((buf[:, C:] == SENTINEL).all())
    assert torch.equal(gx_a, gx_b), rel(gx_b, gx_a)
    assert torch.equal(ge_a[:, :C], buf[:, :C]), rel(buf[:, :C], ge_a[:, :C])
    assert float(gx_a.abs().max()) > 0 and bool(torch.isfinite(gx_a).all())
    if loss_exact:
        assert torch.equal(loss_a, loss_b)
    else:
        assert float((loss_a - loss_b).abs().max() / loss_a.abs().max()) < 1e-12
    # the chains really took different steps: with chain 0's step for all, chain 1 moves
    if xt.shape[0] > 1:
        gx_0, _ = K.ddim_mix_bwd(g, xt, e, at[:1].expand(xt.shape[0]).contiguous(), an[:1].expand(xt.shape[0]).contiguous(),
                                 final_clip=True)
        assert not torch.equal(gx_0[1], gx_a[1])


# ---- a. sandwich_rect, direct ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_mul', [False, True], ids=['plain', 'mul'])
@pytest.mark.parametrize('c', gc.SANDWICH, ids=ids(gc.SANDWICH))
def test_sandwich_rect_on_rectangular_grids(c, with_mul):
    import nhmc.kernels as K
    p = gc.sandwich_problem(c.args)
    out = K.sandwich_rect(dev(p.x), dev(p.S1), dev(p.S2), mul=dev(p.mul) if with_mul else None)
    want = p.out64_mul if with_mul else p.out64
    err = rel(out, want)
    print(f'sandwich_rect {c.id} {"mul" if with_mul else "plain"}: {err:.2e}')
    assert out.shape == want.shape and err < BOUND


# ---- b. spectral operator, random factors ---------------------------------------------------------------------------
SPECTRAL_RUNS = [(c, mode) for c in gc.SPECTRAL for mode in (('pairs', 'chain') if c.args[0] == 256 else ('chain',))]
SPECTRAL_IDS = [f'{c.id}-{mode}' for c, mode in SPECTRAL_RUNS]


@functools.lru_cache(maxsize=None)
def spectral_op(args, projected):
    import nhmc.operators as ops
    o = gc.spectral_problem(args).op
    return ops.Deblurring2D.from_factors(o.U1, o.U2, o.V1, o.V2, o.D, 'cuda', projected=projected)


def set_mode(monkeypatch, mode):
    monkeypatch.setenv('NHMC_SPECTRAL_PAIRS', '1' if mode == 'pairs' else '0')


@pytest.mark.parametrize('c,mode', SPECTRAL_RUNS, ids=SPECTRAL_IDS)
def test_spectral_maps(c, mode, monkeypatch):
    set_mode(monkeypatch, mode)
    p, op = gc.spectral_problem(c.args), spectral_op(c.args, False)
    errs = dict(H=rel(op.H(dev(p.xt)), p.f64.H), Ht=rel(op.Ht(dev(p.y)), p.f64.Ht), H_pinv=rel(op.H_pinv(dev(p.y)), p.f64.H_pinv))
    print(f'spectral {c.id} {mode}: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    assert max(errs.values()) < BOUND


@pytest.mark.parametrize('clip', [True, False], ids=['clip', 'noclip'])
@pytest.mark.parametrize('c,mode', SPECTRAL_RUNS, ids=SPECTRAL_IDS)
def test_spectral_data_term(c, mode, clip, monkeypatch):
    set_mode(monkeypatch, mode)
    p = gc.spectral_problem(c.args)
    want_loss, want_g = (p.f64.loss_clip, p.f64.grad_clip) if clip else (p.f64.loss_noclip, p.f64.grad_noclip)
    xt, y = dev(p.xt), dev(p.y)
    loss, g = spectral_op(c.args, False).data_term(xt, y, apply_clip=clip)
    e_g, e_l = rel(g, want_g), rel(loss, want_loss)
    loss4, g4 = spectral_op(c.args, True).data_term(xt, y, apply_clip=clip)
    p_g, p_n, p_l = rel(g4, want_g), norm_rel(g4, want_g), rel(loss4, want_loss)
    print(f'spectral data term {c.id} {mode} clip={clip}: gradient {e_g:.2e}, loss {e_l:.2e}; '
          f'projected: gradient {p_g:.2e} (norm metric {p_n:.2e}), loss {p_l:.2e}')
    assert e_g < BOUND and e_l < BOUND
    assert p_g < 3e-5 and p_n < 3e-5 and p_l < 1e-5
    if clip:
        out = (p.xt.abs() > 1).cuda()
        assert bool(out.any()) and not bool(g[out].any()) and not bool(g4[out].any())


@pytest.mark.parametrize('projected', [False, True], ids=['eight', 'projected'])
@pytest.mark.parametrize('two_c', [False, True], ids=['eC', 'e2C'])
@pytest.mark.parametrize('c,mode', SPECTRAL_RUNS, ids=SPECTRAL_IDS)
def test_spectral_fused_vjp_with_a_step_per_chain(c, mode, two_c, projected, monkeypatch):
    set_mode(monkeypatch, mode)
    p, op = gc.spectral_problem(c.args), spectral_op(c.args, projected)
    e = p.e if two_c else p.e[:, :p.C]
    fused_equals_two_kernels(op, dev(p.xt), dev(e), dev(p.at), dev(p.at_next), dev(p.y))


# ---- c. SRConv, random factors --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def srconv_op(args):
    import nhmc.operators as ops
    p = gc.srconv_problem(args)
    return ops.SRConv.from_svd(p.op.U, p.op.s, p.op.V, 3, p.d, 'cuda', stride=p.stride)


@pytest.mark.parametrize('c', gc.SRCONV, ids=ids(gc.SRCONV))
def test_srconv_maps(c):
    p, op = gc.srconv_problem(c.args), srconv_op(c.args)
    errs = dict(H=rel(op.H(dev(p.xt)), p.f64.H), Ht=rel(op.Ht(dev(p.y)), p.f64.Ht), H_pinv=rel(op.H_pinv(dev(p.y)), p.f64.H_pinv))
    print(f'srconv {c.id}: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    assert max(errs.values()) < BOUND


@pytest.mark.parametrize('clip', [True, False], ids=['clip', 'noclip'])
@pytest.mark.parametrize('c', gc.SRCONV, ids=ids(gc.SRCONV))
def test_srconv_data_term(c, clip):
    p = gc.srconv_problem(c.args)
    want_loss, want_g = (p.f64.loss_clip, p.f64.grad_clip) if clip else (p.f64.loss_noclip, p.f64.grad_noclip)
    loss, g = srconv_op(c.args).data_term(dev(p.xt), dev(p.y), apply_clip=clip)
    e_g, e_l = rel(g, want_g), rel(loss, want_loss)
    print(f'srconv data term {c.id} clip={clip}: gradient {e_g:.2e}, loss {e_l:.2e}')
    assert e_g < BOUND and e_l < BOUND
    if clip:
        out = (p.xt.abs() > 1).cuda()
        assert bool(out.any()) and not bool(g[out].any())


@pytest.mark.parametrize('two_c', [False, True], ids=['eC', 'e2C'])
@pytest.mark.parametrize('c', gc.SRCONV, ids=ids(gc.SRCONV))
def test_srconv_fused_vjp_with_a_step_per_chain(c, two_c):
    p = gc.srconv_problem(c.args)
    e = p.e if two_c else p.e[:, :p.C]
    fused_equals_two_kernels(srconv_op(c.args), dev(p.xt), dev(e), dev(p.at), dev(p.at_next), dev(p.y))


# ---- d. tile-size invariance, bit for bit ---------------------------------------------------------------------------
# Every product is an exact k-ascending FMA chain from zero and each padded term contributes fma(0, ., acc) = acc, so a
# zero-padded problem gives the same bits in its top-left block -- through another tile size, or through k_pair256.
@pytest.mark.parametrize('d,D,mode', [(96, 128, 'chain'), (192, 256, 'pairs'), (192, 256, 'chain')],
                         ids=['96in128', '192in256-pairs', '192in256-chain'])
def test_zero_padding_changes_no_bit_of_the_spectral_chain(d, D, mode, monkeypatch):
    import nhmc.kernels as K
    set_mode(monkeypatch, mode)
    p, op = gc.spectral_problem((d, 3, 3)), spectral_op((d, 3, 3), False)
    B, C = p.B, p.C
    pad = lambda t: dev(gc.embed(t.cpu(), D))
    xt, e, at, an = dev(p.xt), dev(p.e), dev(p.at), dev(p.at_next)
    y = dev(p.y).reshape(B, C, d, d)
    yT = y.transpose(-1, -2).contiguous()
    y_proj = K.spectral_project(y, op.factors[0], op.factors[1])
    nxt = K.ddim_mix_fwd(xt, e, at, an, final_clip=True)['xt_next']
    F, Dm, DmT = op.factors, op.Dmap, op.DmapT
    FP, DmP, DmTP = pad(F), pad(Dm), pad(DmT)
    assert FP.shape == (8, D, D) and torch.equal(top_left(FP, d), F)

    def same(small, big, what):
        assert torch.equal(top_left(big, d), small), (what, rel(top_left(big, d), small))
        assert zero_outside(big, d), what

    def same_loss(small, big, what):
        assert float((small - big).abs().max() / small.abs().max()) < 1e-6, what

    same(K.spectral_apply(xt, F[2], F[3], Dm, F[4], F[5]), K.spectral_apply(pad(xt), FP[2], FP[3], DmP, FP[4], FP[5]), 'H')
    same(K.spectral_apply(y, F[0], F[1], Dm, F[6], F[7]), K.spectral_apply(pad(y), FP[0], FP[1], DmP, FP[6], FP[7]), 'Ht')
    same(y_proj, K.spectral_project(pad(y), FP[0], FP[1]), 'projection')
    for clip in (True, False):
        l0, g0 = K.data_spectral(xt, yT, F, Dm, clip, DmapT=DmT)
        l1, g1 = K.data_spectral(pad(xt), pad(yT), FP, DmP, clip, DmapT=DmTP)
        same(g0, g1, f'data term clip={clip}')
        same_loss(l0, l1, f'loss clip={clip}')
        l0, g0 = K.data_spectral(xt, y_proj, F, Dm, clip, projected=True)
        l1, g1 = K.data_spectral(pad(xt), pad(y_proj), FP, DmP, clip, projected=True)
        same(g0, g1, f'projected data term clip={clip}')
        same_loss(l0, l1, f'projected loss clip={clip}')
    for ec in (C, 2 * C):
        es, _ = guarded((B, ec, d, d), e[:, :ec])
        eb, _ = guarded((B, ec, D, D), pad(e[:, :ec]))
        for projected, obs in ((False, yT), (True, y_proj)):
            kw = dict(projected=True) if projected else dict(DmapT=DmT)
            kwp = dict(projected=True) if projected else dict(DmapT=DmTP)
            l0, gx0, ge0 = K.data_spectral_vjp(nxt, obs, F, Dm, xt, es, at, an, g_e_out=guarded((B, ec, d, d))[0], **kw)
            l1, gx1, ge1 = K.data_spectral_vjp(pad(nxt), pad(obs), FP, DmP, pad(xt), eb, at, an,
                                               g_e_out=guarded((B, ec, D, D))[0], **kwp)
            same(gx0, gx1, f'vjp g_xt ec={ec} projected={projected}')
            same(ge0[:, :C], ge1[:, :C], f'vjp g_e ec={ec} projected={projected}')
            same_loss(l0, l1, f'vjp loss ec={ec} projected={projected}')
            assert float(gx0.abs().max()) > 0


@pytest.mark.parametrize('to', [(64, 64, 128, 64), (128, 128, 128, 128)], ids=['T64', 'T128'])
def test_zero_padding_changes_no_bit_of_sandwich_rect(to):
    """(2, 64, 64, 96, 64) runs T = 32 on 2 x 3 and 3 x 2 tiles; padded it runs T = 64 resp. T = 128."""
    import nhmc.kernels as K
    args = (2, 64, 64, 96, 64)
    p = gc.sandwich_problem(args)
    n, K1, R1, C1, C2 = args
    K1p, R1p, C1p, C2p = to
    assert gc.tile_path(R1, C1, n)[0] == 32 and gc.tile_path(R1p, C1p, n)[0] == gc.tile_path(C1p, C2p, n)[0] > 32
    for mul in (None, p.mul):
        small = K.sandwich_rect(dev(p.x), dev(p.S1), dev(p.S2), mul=None if mul is None else dev(mul))
        big = K.sandwich_rect(dev(gc.embed(p.x, (K1p, R1p))), dev(gc.embed(p.S1, (K1p, C1p))), dev(gc.embed(p.S2, (R1p, C2p))),
                              mul=None if mul is None else dev(gc.embed(mul, (C1p, C2p))))
        assert torch.equal(big[:, :C1, :C2], small)
        assert not bool(big[:, C1:, :].any()) and not bool(big[:, :, C2:].any())


# ---- e. a different step per chain in every fused data term ---------------------------------------------------------
def _ragged_inpaint(dim, dev_, g_):
    from nhmc import operators
    return operators.Inpainting(3, dim, torch.tensor([0, 5, 7, 100, 3 * dim * dim - 1]), dev_)


# name -> (degradation or factory, image size, the loss of the two paths is the same bits)
FUSED = {
    'inpaint_random': ('inpaint_random', 16, False), 'inpaint_ragged': (_ragged_inpaint, 16, False), 'sr2': ('sr2', 16, False),
    'color': ('color', 16, False), 'hdr': ('hdr', 64, False), 'cs2': ('cs2', 32, True), 'deblur_aniso': ('deblur_aniso', 32, True),
    'deblur_gauss': ('deblur_gauss', 32, True), 'sr_bicubic2': ('sr_bicubic2', 64, True), 'phase_retrieval': ('phase_retrieval', 32, True),
}


@pytest.mark.parametrize('two_c', [False, True], ids=['eC', 'e2C'])
@pytest.mark.parametrize('name', sorted(FUSED))
def test_every_fused_data_term_with_a_step_per_chain(name, two_c):
    from nhmc import operators
    deg, dim, loss_exact = FUSED[name]
    B = 3
    g_ = torch.Generator().manual_seed(1000 + dim + len(name))
    d_ = torch.device('cuda')
    op = deg(dim, d_, g_) if callable(deg) else operators.build_operator(deg, 3, dim, d_, generator=g_)
    assert hasattr(op, 'fused_last_vjp')
    xt = (torch.randn(B, 3, dim, dim, generator=g_) * 0.8).cuda()
    e = torch.randn(B, 6 if two_c else 3, dim, dim, generator=g_).cuda()
    y = torch.randn(B, op.M, generator=g_)
    y = (0.5 * y.abs() if name == 'phase_retrieval' else y).cuda()
    at, an = gc.chain_alphas(B)
    fused_equals_two_kernels(op, xt, e, dev(at), dev(an), y, loss_exact=loss_exact)
