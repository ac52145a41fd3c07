"""GPU: the one-pass GroupNorm (+ FiLM) (+ SiLU) kernels (csrc/gn_onepass.hip): against torch's ops and an fp64 evaluation
with the bounds of tests/test_gn_act_gpu.py::test_fused_group_norm_matches_torch, bit-identity with and without the
bounded-wait fallback, run-to-run determinism, the A/B switch, the two-source (concatenated input) form, and graph capture."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (C, res) of tools/gn_bench.py: every GroupNorm input of the FFHQ U-Net.  (1024, 16) fits one workgroup per slab.
FFHQ = ((128, 256), (256, 256), (128, 128), (256, 128), (384, 128), (256, 64), (512, 64), (512, 32), (1024, 16))
# + a small one-workgroup shape, + a shape the one-pass kernels do not cover (96 splits > 64): stays on the two-pass path
CASES = [((2 + i % 3, C, r, r), i % 2 == 0, i % 3 != 2, bool(i % 2), i % 4 == 1) for i, (C, r) in enumerate(FFHQ)] + \
        [((3, 64, 16, 16), True, True, True, True), ((2, 384, 256, 256), True, True, False, False)]


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()          # on the device: the tensors are up to 2^26 elements
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def make(shape, film, pre, seed=0):
    g = torch.Generator().manual_seed(seed + shape[1] + shape[2])
    C = shape[1]
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).cuda()
    beta = (0.1 * torch.randn(C, generator=g)).cuda()
    x = (torch.randn(shape, generator=g) * 1.7 + 0.3).cuda()
    fm = (0.3 * torch.randn(shape[0], 2 * C, generator=g)).cuda() if film else None
    pb = (0.5 * torch.randn(shape[0], C, generator=g)).cuda() if pre else None
    dy = torch.randn(shape, generator=g).cuda()
    acc = torch.randn(shape, generator=g).cuda()
    return x, gamma, beta, fm, pb, dy, acc


def covered(shape, groups=32):
    import nhmc.kernels as K
    return K.gn_onepass_splits(shape[0], shape[1], groups, shape[2] * shape[3]) > 0


@pytest.mark.parametrize('shape,film,act,pre,acc', CASES)
def test_onepass_group_norm_matches_torch(shape, film, act, pre, acc):
    """Forward and input gradient against ATen and against an fp64 evaluation of the same formula: < 2e-6 / < 1e-5, and no
    further from fp64 than 2 x ATen."""
    import nhmc.kernels as K
    groups, eps = 32, 1e-5
    x, gamma, beta, fm, pb, dy, ad = make(shape, film, pre)
    ad = ad if acc else None

    def torch_form(xx, dt):
        if pb is not None:
            xx = xx + pb.to(dt)[:, :, None, None]
        h = F.group_norm(xx, groups, gamma.to(dt), beta.to(dt), eps)
        if fm is not None:
            sc, sh = fm.to(dt)[:, :, None, None].chunk(2, dim=1)
            h = h * (1 + sc) + sh
        return F.silu(h) if act else h
    xa = x.clone().requires_grad_(True)
    ya = torch_form(xa, torch.float32)
    (ga,) = torch.autograd.grad(ya, xa, dy)
    xd = x.double().requires_grad_(True)
    yd = torch_form(xd, torch.float64)
    (gd,) = torch.autograd.grad(yd, xd, dy.double())
    if ad is not None:
        ga, gd = ga + ad, gd + ad.double()
    yb, ws, splits = K.gn_act_fwd(x, gamma, beta, groups, eps, act, fm, pb)
    gb = K.gn_act_bwd(x, dy, gamma, beta, groups, eps, act, fm, ws, splits, pb, add=ad, onepass=True)
    assert (splits == K.gn_onepass_splits(shape[0], shape[1], groups, shape[2] * shape[3])) == covered(shape)
    # the default route (nhmc_gn_onepass_prefers): the one-pass forward's slab totals feed the two-pass backward
    gr = K.gn_act_bwd(x, dy, gamma, beta, groups, eps, act, fm, ws, splits, pb, add=ad)
    print('default-route backward', shape, (rel(gr, gd), rel(gr, ga)))
    assert rel(gr, gd) < 1e-5 and rel(gr, ga) < 1e-5 and rel(gr, gd) <= 2 * rel(ga, gd) + 1e-6
    figures = (rel(yb, yd), rel(gb, gd), rel(yb, ya), rel(gb, ga), rel(ya, yd), rel(ga, gd))
    print('one-pass' if covered(shape) else 'two-pass', shape, 'splits', splits, figures)
    assert rel(yb, yd) < 2e-6 and rel(gb, gd) < 1e-5, figures
    assert rel(yb, ya) < 2e-6 and rel(gb, ga) < 1e-5, figures
    assert rel(yb, yd) <= 2 * rel(ya, yd) + 1e-7 and rel(gb, gd) <= 2 * rel(ga, gd) + 1e-6, figures


@pytest.mark.parametrize('shape,film,act,pre,acc', [c for c in CASES if c[0][1:] != (384, 256, 256)])
def test_fallback_and_repeat_give_the_same_bits(shape, film, act, pre, acc):
    """Every workgroup taking the expired-wait path (the test-only flag) = the waiting path, and two calls agree: fixed
    summation order, no float atomics.  Between the calls the kernels run on other data, so that a workspace
    block the allocator hands out again holds figures that would be wrong if a workgroup read them stale."""
    import nhmc.kernels as K
    assert covered(shape)
    x, gamma, beta, fm, pb, dy, ad = make(shape, film, pre, seed=1)
    ad = ad if acc else None
    outs = []
    for flags in (0, K.GN_ONEPASS_NOWAIT, 0):
        y, ws, splits = K.gn_act_fwd(x, gamma, beta, 32, 1e-5, act, fm, pb, flags=flags)
        dx = K.gn_act_bwd(x, dy, gamma, beta, 32, 1e-5, act, fm, ws, splits, pb, add=ad, flags=flags, onepass=True)
        outs.append((y, ws, dx))
        yo, wo, so = K.gn_act_fwd(x * -0.5 + 1.0, gamma, beta, 32, 1e-5, act, fm, pb)
        K.gn_act_bwd(x * -0.5 + 1.0, dx, gamma, beta, 32, 1e-5, act, fm, wo, so, pb, onepass=True)
        del yo, wo
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)


@pytest.mark.parametrize('shape', [(2, 128, 128, 128), (3, 64, 16, 16), (2, 256, 64, 64)])
def test_switch_off_reproduces_the_two_pass_entries(shape):
    """NHMC_GN_ONEPASS=0: the bits of nhmc_gn_act_fwd / nhmc_gn_act_bwd called directly; and a two-pass forward workspace
    feeds the one-pass backward (same layout, its own split count)."""
    import nhmc._lib as L
    import nhmc.kernels as K
    lib = L.load()
    x, gamma, beta, fm, pb, dy, ad = make(shape, True, True, seed=2)
    B, C, hw = shape[0], shape[1], shape[2] * shape[3]
    splits = lib.nhmc_gn_splits(B, C, 32, hw)
    ws, ws2 = (torch.empty(B * 32 * splits * 2, dtype=torch.float64, device='cuda') for _ in range(2))
    y, dx = torch.empty_like(x), torch.empty_like(x)
    p, st = K._ptr, K._stream()
    assert lib.nhmc_gn_act_fwd(p(x), p(gamma), p(beta), p(fm), fm.stride(0), p(pb), pb.stride(0), 1e-5, 1, p(y), p(ws), splits,
                               B, C, 32, hw, st) == 0
    assert lib.nhmc_gn_act_bwd(p(x), p(dy), p(gamma), p(beta), p(fm), fm.stride(0), p(pb), pb.stride(0), 1e-5, 1, p(ws), p(ad),
                               p(dx), p(ws2), splits, B, C, 32, hw, st) == 0
    os.environ['NHMC_GN_ONEPASS'] = '0'
    try:
        y0, w0, s0 = K.gn_act_fwd(x, gamma, beta, 32, 1e-5, True, fm, pb)
        d0 = K.gn_act_bwd(x, dy, gamma, beta, 32, 1e-5, True, fm, w0, s0, pb, add=ad)
    finally:
        os.environ.pop('NHMC_GN_ONEPASS')
    assert s0 == splits and torch.equal(y0, y) and torch.equal(w0, ws) and torch.equal(d0, dx)
    d1 = K.gn_act_bwd(x, dy, gamma, beta, 32, 1e-5, True, fm, ws, splits, pb, add=ad, onepass=True)   # one-pass backward, two-pass ws
    assert rel(d1, dx) < 1e-5


@pytest.mark.parametrize('n,c1,c2,res,act,acc', [(2, 128, 128, 256, True, True), (2, 256, 128, 128, True, True),
                                                 (3, 256, 256, 64, False, True), (2, 512, 512, 16, True, False),
                                                 (2, 32, 64, 32, True, True)])
def test_two_sources_equal_the_materialised_concatenation(n, c1, c2, res, act, acc):
    """x_cat = torch.cat bit for bit; y, dh, dskip = the one-pass kernels on the concatenation, sliced; the gradients are
    contiguous.  256 + 128 channels in 32 groups of 12: groups straddle the seam."""
    import nhmc.kernels as K
    g = torch.Generator().manual_seed(n + c1 + res)
    C = c1 + c2
    h, skip = torch.randn(n, c1, res, res, generator=g).cuda(), (torch.randn(n, c2, res, res, generator=g) * 2 - 0.5).cuda()
    gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).cuda(), (0.1 * torch.randn(C, generator=g)).cuda()
    dy = torch.randn(n, C, res, res, generator=g).cuda()
    ad = torch.randn(n, C, res, res, generator=g).cuda() if acc else None
    cat = torch.cat([h, skip], dim=1)
    y0, ws0, s0 = K.gn_act_fwd(cat, gamma, beta, 32, 1e-5, act)
    dx0 = K.gn_act_bwd(cat, dy, gamma, beta, 32, 1e-5, act, None, ws0, s0, add=ad, onepass=True)
    for flags in (0, K.GN_ONEPASS_NOWAIT):
        y, ws, s, x_cat = K.gn_act_fwd(h, gamma, beta, 32, 1e-5, act, x2=skip, flags=flags)
        dh, dskip = K.gn_act_bwd(x_cat, dy, gamma, beta, 32, 1e-5, act, None, ws, s, add=ad, c1=c1, flags=flags)
        assert torch.equal(x_cat, cat) and torch.equal(y, y0) and torch.equal(ws, ws0) and s == s0
        assert dh.is_contiguous() and dskip.is_contiguous() and dh.shape == h.shape and dskip.shape == skip.shape
        assert torch.equal(dh, dx0[:, :c1]) and torch.equal(dskip, dx0[:, c1:])


def test_pair_autograd_function_and_unet_agree_with_the_concatenation(monkeypatch):
    """_GroupNormActCat against the fork on torch.cat, and a whole U-Net (num_channels 32, 64x64) with and without the pair
    path: output and input gradient bit for bit; the gradients that leave the pair op are contiguous.  (Both routes run
    the same one-pass kernels on the same slabs here, so the bits can agree; against the two-pass kernels they would
    not: those split a slab into ceil(n4 / splits) pieces, the one-pass kernels into shares of 2048 float4.)"""
    from nhmc import unet
    g = torch.Generator().manual_seed(11)
    gn = torch.nn.GroupNorm(32, 96).cuda().requires_grad_(False)
    gn.weight.copy_(1 + 0.2 * torch.randn(96, generator=g).cuda())
    h0, s0 = torch.randn(2, 64, 32, 32, generator=g).cuda(), torch.randn(2, 32, 32, 32, generator=g).cuda()
    dy, ds = torch.randn(2, 96, 32, 32, generator=g).cuda(), torch.randn(2, 96, 32, 32, generator=g).cuda()
    res = []
    for pair in (True, False):
        h, s = h0.clone().requires_grad_(True), s0.clone().requires_grad_(True)
        if pair:
            y, xc = unet.group_norm_act_pair(gn, h, s)
            assert type(y.grad_fn).__name__.startswith('_GroupNormActCat')
        else:
            y, xc = unet.group_norm_act_fork(gn, torch.cat([h, s], dim=1))
        gh, gs = torch.autograd.grad((y * dy).sum() + (xc * ds).sum(), (h, s))
        if pair:
            assert gh.is_contiguous() and gs.is_contiguous()
        res.append((y.detach(), xc.detach(), gh, gs))
    for a, b in zip(*res):
        assert torch.equal(a, b)

    # MIOpen's default choice of convolution kernels is not run-to-run reproducible at these sizes (two evaluations of the
    # same network differ in the last bits with or without this repository's kernels); its deterministic choice is
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)
    torch.manual_seed(4)
    net = unet.create_model(image_size=64, num_channels=32, num_res_blocks=1, attention_resolutions='16',
                            num_head_channels=32).cuda().eval()
    net.requires_grad_(False)
    x0 = torch.randn(2, 3, 64, 64, generator=g).cuda()
    t = torch.tensor([10., 500.]).cuda()
    go = None
    outs = []
    for pair in (True, False):
        if not pair:
            monkeypatch.setattr(unet, 'pair_glue', lambda *a: False)
        x = x0.clone().requires_grad_(True)
        out = net(x, t)
        go = torch.randn_like(out) if go is None else go
        (gx,) = torch.autograd.grad(out, x, go)
        outs.append((out.detach(), gx))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_graph_capture_replays_the_eager_bits():
    """Forward + input gradient through a ResBlock (a pair input: 32 + 32 channels at 128x128, 4 splits per slab) captured
    into a graph: both replays give the eager bits -- the workspace is re-filled by a kernel node of each launch."""
    from nhmc import unet
    torch.manual_seed(6)
    blk = unet.ResBlock(64, 128, 32).cuda().eval().requires_grad_(False)
    h = torch.randn(2, 32, 128, 128).cuda().requires_grad_(True)
    s = torch.randn(2, 32, 128, 128).cuda().requires_grad_(True)
    emb, dy = torch.randn(2, 128).cuda(), torch.randn(2, 32, 128, 128).cuda()

    def step():
        y = blk((h, s), emb)
        return (y,) + torch.autograd.grad(y, (h, s), dy)
    assert unet.pair_glue(blk.in_layers[0], h, s)
    eager = [t.detach().clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(2):
        for t in captured:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a, b.detach())
