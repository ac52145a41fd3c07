"""GPU: the thin 3x3 convolutions (csrc/thin_conv.hip) against float64 on the same inputs, all four passes.
nhmc_conv3x3_thin_in: the forward pass of a thin -> wide convolution (F.conv2d, with and without bias) and the backward-data
pass of a wide -> thin one (conv2d_input), which runs the flipped, transposed filter through the same kernel.
nhmc_conv3x3_thin_out: the forward pass of a wide -> thin convolution and the backward-data pass of a thin -> wide one.

Bound, elementwise, the a-priori forward error of an fp32 dot product of length L = 9 C_in plus the bias add, for any
summation order, fused or not:   |y - y64| <= (L + 2) 2^-24 (|x| * |w| + |bias|).   A result scaled by 1 + 1e-4 must fail it.

A lane owns four adjacent pixels of a row and a workgroup 256 lanes in (n, h, w / 4) order.  Shapes (n, thin, wide, H, W):
one image inside one workgroup with rows one lane wide (both column borders in one lane); one image of 32 lanes (all four
borders in one workgroup); three workgroups with rows of 13 lanes, H != W, so that workgroup and wave boundaries fall
inside rows and images; n = 1 and n = 3; thin 3 and 6; wide 32, 128 and 160.  x and y sit inside larger buffers: x between
NaN bands (a read outside the image would reach the result), y between sentinels that must come back untouched.  Two calls
give equal bits.  One NaN and one inf pixel: the set of non-finite outputs is the reference's."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(2, 3, 32, 5, 4), (1, 3, 32, 8, 16), (1, 6, 128, 40, 52), (3, 3, 128, 24, 24), (3, 6, 160, 40, 52)]
GUARD, SENTINEL = 4096, -12345.0
ids = lambda s: 'x'.join(map(str, s))
_cases = {}


def case(shape, backward, out=False):
    """Inputs on the CPU and the float64 reference with its bound, computed once per (shape, direction, kernel) and left
    unchanged.  out=False: x has the thin side's channels and the result the wide side's; out=True: the other way round."""
    key = (shape, backward, out)
    if key not in _cases:
        n, thin, wide, h, w = shape
        cin, cout = (wide, thin) if out else (thin, wide)
        gen = torch.Generator().manual_seed(11 + 4 * SHAPES.index(shape) + 2 * out + backward)
        x = torch.randn(n, cin, h, w, generator=gen)
        wt = torch.randn((cin, cout, 3, 3) if backward else (cout, cin, 3, 3), generator=gen) / (9.0 * cin) ** 0.5
        bias = torch.randn(cout, generator=gen)
        x64, w64 = x.double(), wt.double()
        if backward:
            ref = lambda a, b: torch.nn.grad.conv2d_input((n, cout, h, w), b, a, 1, 1)
        else:
            ref = lambda a, b: F.conv2d(a, b, None, 1, 1)
        y64, mag = ref(x64, w64), ref(x64.abs(), w64.abs())
        _cases[key] = (x, wt, bias, y64, mag)
    return _cases[key]


def bound(mag, bias, cin):
    extra = 0.0 if bias is None else bias.double().abs().view(1, -1, 1, 1)
    return (9 * cin + 2) * 2.0 ** -24 * (mag + extra)


def run_raw(x, wt, bias, backward, out=False):
    """The raw entry on x and y inside guarded buffers -> (y, the two y guards intact)."""
    import nhmc
    import nhmc.kernels as K
    n, thin, h, w = x.shape                                                       # (thin, wide): the channels of x and of y
    wp = K.thin_in_weights(wt, backward, out=out)
    wide = wt.shape[1 if backward else 0]
    xbuf = torch.full((GUARD + x.numel() + GUARD,), float('nan'), device='cuda')
    xin = xbuf[GUARD:GUARD + x.numel()].view_as(x)
    xin.copy_(x)
    numel = n * wide * h * w
    ybuf = torch.full((GUARD + numel + GUARD,), SENTINEL, device='cuda')
    y = ybuf[GUARD:GUARD + numel].view(n, wide, h, w)
    P = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    lib = nhmc._lib.load()
    rc = (lib.nhmc_conv3x3_thin_out if out else lib.nhmc_conv3x3_thin_in)(P(xin), P(wp), P(bias), P(y), n, thin, wide, h, w, 1, 1,
                                                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    intact = bool((ybuf[:GUARD] == SENTINEL).all()) and bool((ybuf[GUARD + numel:] == SENTINEL).all())
    return y, intact


@pytest.mark.parametrize('shape', SHAPES, ids=ids)
@pytest.mark.parametrize('backward', [False, True], ids=['fwd', 'bwd'])
@pytest.mark.parametrize('with_bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('out', [False, True], ids=['thin_in', 'thin_out'])
def test_against_float64_within_the_dot_product_bound(shape, backward, with_bias, out):
    import nhmc.kernels as K
    n, thin, wide, h, w = shape
    assert K.conv3x3_thin_out_covers(n, wide, thin, h, w) if out else K.conv3x3_thin_in_covers(n, thin, wide, h, w)
    x, wt, bias, y64, mag = case(shape, backward, out)
    xg, wg, bg = x.cuda(), wt.cuda(), (bias.cuda() if with_bias else None)
    y, intact = run_raw(xg, wg, bg, backward, out)
    want = y64 + bias.double().view(1, -1, 1, 1) if with_bias else y64
    tol = bound(mag, bias if with_bias else None, x.shape[1])
    err = (y.double().cpu() - want).abs()
    print(f'{ids(shape)} {"out" if out else "in"} {"bwd" if backward else "fwd"}: max err / bound = {float((err / tol).max()):.3f}')
    assert intact
    assert bool(torch.isfinite(y).all()) and bool((err <= tol).all())
    front = (K.conv3x3_thin_out if out else K.conv3x3_thin_in)(xg, wg, bg, backward=backward)   # the front end, a second call
    assert torch.equal(front.view(torch.int32), y.contiguous().view(torch.int32))


def test_the_bound_bites():
    """Checked once, where the dot product is short (L = 54): there the bound is 3.3e-6 of sum |x| |w| and a relative error of
    1e-4 stands far above it.  With a wide input (L = 9 * 128 and more) the same a-priori bound is 6.9e-5 of that sum and
    more, which a typical output scaled by 1 + 1e-4 stays under; the thin-output cases are held to it all the same."""
    shape = SHAPES[2]
    x, wt, bias, y64, mag = case(shape, False)
    import nhmc.kernels as K
    y = K.conv3x3_thin_in(x.cuda(), wt.cuda(), None).double().cpu()
    tol = bound(mag, None, x.shape[1])
    assert bool(((y - y64).abs() <= tol).all())
    assert not bool(((y * (1 + 1e-4) - y64).abs() <= tol).all())


@pytest.mark.parametrize('backward', [False, True], ids=['fwd', 'bwd'])
@pytest.mark.parametrize('out', [False, True], ids=['thin_in', 'thin_out'])
def test_nan_and_inf_pixels_reach_the_outputs_the_reference_says(backward, out):
    import nhmc.kernels as K
    shape = SHAPES[3]
    n, thin, wide, h, w = shape
    x, wt, bias, _, _ = case(shape, backward, out)
    x = x.clone()
    x[0, 1, 0, 3], x[2, 2, 23, 23] = float('nan'), float('inf')
    if backward:
        y64 = torch.nn.grad.conv2d_input((n, thin if out else wide, h, w), wt.double(), x.double(), 1, 1)
    else:
        y64 = F.conv2d(x.double(), wt.double(), None, 1, 1)
    y = (K.conv3x3_thin_out if out else K.conv3x3_thin_in)(x.cuda(), wt.cuda(), None, backward=backward).cpu()
    bad = ~torch.isfinite(y64)
    assert 0 < int(bad.sum()) < y64.numel() // 4
    assert torch.equal(~torch.isfinite(y), bad)


def test_filter_is_built_once_per_weight_tensor_and_direction():
    import nhmc.kernels as K
    x, wt, _, _, _ = case(SHAPES[1], False)
    xg, wg = x.cuda(), wt.cuda()
    before = K.thin_weight_builds()
    K.conv3x3_thin_in(xg, wg)
    K.conv3x3_thin_in(xg, wg)
    assert K.thin_weight_builds() == before + 1
    wg.mul_(2.0)                                                                  # an in-place edit rebuilds it
    K.conv3x3_thin_in(xg, wg)
    assert K.thin_weight_builds() == before + 2
    x2, w2, _, _, _ = case(SHAPES[1], True, True)                                 # the same for the thin-output kernel
    xg, wg = x2.cuda(), w2.cuda()
    K.conv3x3_thin_out(xg, wg, backward=True)
    K.conv3x3_thin_out(xg, wg, backward=True)
    assert K.thin_weight_builds() == before + 3


def test_autograd_node_routes_each_direction_and_keeps_the_vendor_call(monkeypatch):
    from nhmc import unet
    import nhmc.kernels as K
    monkeypatch.delenv('NHMC_THIN_CONV', raising=False)
    torch.manual_seed(2)
    first = torch.nn.Conv2d(3, 32, 3, padding=1).cuda().requires_grad_(False)
    last = torch.nn.Conv2d(32, 6, 3, padding=1).cuda().requires_grad_(False)
    x = torch.randn(2, 3, 8, 16, device='cuda', requires_grad=True)
    h = torch.randn(2, 32, 8, 16, device='cuda', requires_grad=True)
    assert unet.thin_route(first, x, True) == (True, True) and unet.thin_route(last, h, True) == (True, True)
    assert unet.thin_route(first, x.detach(), True) == (True, False)              # no gradient asked for
    assert unet.thin_route(first, x) is None and unet.thin_route(last, h) is None  # not measured shapes: the module call
    assert torch.equal(unet.conv_thin(first, x), first(x)) and torch.equal(unet.conv_thin(last, h), last(h))
    for conv, inp in ((first, x), (last, h)):
        # forward and input gradient within the bound of their dot products, against float64 on the CPU
        y = unet.conv_thin(conv, inp, True)
        g = torch.randn_like(y)
        (gi,) = torch.autograd.grad(y, inp, g)
        w64, b64, i64, g64 = conv.weight.double().cpu(), conv.bias.double().cpu(), inp.detach().double().cpu(), g.double().cpu()
        y64 = F.conv2d(i64, w64, b64, 1, 1)
        tol = (9 * inp.shape[1] + 2) * 2.0 ** -24 * F.conv2d(i64.abs(), w64.abs(), b64.abs(), 1, 1)
        assert bool(((y.double().cpu() - y64).abs() <= tol).all())
        gi64 = torch.nn.grad.conv2d_input(tuple(inp.shape), w64, g64, 1, 1)
        tol = (9 * y.shape[1] + 2) * 2.0 ** -24 * torch.nn.grad.conv2d_input(tuple(inp.shape), w64.abs(), g64.abs(), 1, 1)
        assert bool(((gi.double().cpu() - gi64).abs() <= tol).all())
    # an unrouted direction is exactly the vendor's call
    y = unet._Conv3x3Thin.apply(h, last.weight, last.bias, (False, True))
    assert torch.equal(y, last(h))
    monkeypatch.setenv('NHMC_THIN_CONV', '0')
    assert unet.thin_route(first, x, True) is None and not K.conv3x3_thin_out_prefers(0, 64, 128, 6, 256, 256)
