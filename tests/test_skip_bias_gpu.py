"""GPU: the skip bias in the eight-wave Winograd kernel's epilogue (csrc/wino_conv.hip, "Skip bias"; nhmc_conv3x3_wino_skip)
gives the bits of today's sequence, in which the bias was added to the skip tensor by a broadcast pass of its own:

  conv3x3_wino_skip(x, w, b2, s, b1)  ==  conv3x3_wino(x, w, b2, add=s + b1)                bit for bit

Shapes (n, C, K, H, W): one workgroup; two K blocks with two row and two column blocks.  Inputs: normal draws (the output
between sentinels), and a NaN and an inf in `add`.  A ResBlock 64 -> 128 at 64 x 64 whose skip path is a 1x1 convolution:
output and input gradient bit-equal between NHMC_SKIP_BIAS=0 and the default, eagerly and under a hipGraph replay."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 64, 4, 64), (2, 16, 128, 8, 128)]
GUARD, SENTINEL = 4096, -12345.0
ids = lambda s: 'x'.join(map(str, s))


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def operands(shape, seed=3):
    n, c, k, h, w = shape
    gen = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=gen, device='cuda')
    wt = torch.randn(k, c, 3, 3, generator=gen, device='cuda') / (3.0 * c ** 0.5)
    b2, b1 = torch.randn(k, generator=gen, device='cuda'), torch.randn(k, generator=gen, device='cuda')
    s = torch.randn(n, k, h, w, generator=gen, device='cuda')
    return x, wt, b2, b1, s


@pytest.mark.parametrize('shape', SHAPES, ids=ids)
@pytest.mark.parametrize('with_bias', [True, False], ids=['bias', 'nobias'])
def test_skip_bias_in_the_epilogue_is_the_bias_pass_bit_for_bit(monkeypatch, shape, with_bias):
    import nhmc.kernels as K
    monkeypatch.delenv('NHMC_WINO_WAVES', raising=False)
    monkeypatch.delenv('NHMC_SKIP_BIAS', raising=False)
    n, c, k, h, w = shape
    assert K.conv3x3_wino_skip_covers(n, c, k, h, w)
    x, wt, b2, b1, s = operands(shape)
    b2 = b2 if with_bias else None
    s0 = s.clone()
    want = K.conv3x3_wino(x, wt, b2, add=s.clone().add_(b1.view(1, -1, 1, 1)))      # the vendor path's output.add_(bias)
    got = K.conv3x3_wino_skip(x, wt, b2, s, b1)
    assert same_bits(got, want) and same_bits(s, s0)                                # and `add` is only read
    assert same_bits(K.conv3x3_wino_skip(x, wt, b2, s, b1), got)                    # two calls, equal bits
    assert not same_bits(got, K.conv3x3_wino(x, wt, b2, add=s))                     # the bias did arrive


@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_nan_and_inf_in_add_and_the_guard_bands(monkeypatch, shape):
    import ctypes
    import nhmc
    import nhmc.kernels as K
    monkeypatch.delenv('NHMC_WINO_WAVES', raising=False)
    n, c, k, h, w = shape
    x, wt, b2, b1, s = operands(shape, seed=4)
    s[0, 1, 2, 5], s[n - 1, k - 1, h - 1, w - 1], s[0, 0, 0, 0] = float('nan'), float('inf'), float('-inf')
    want = K.conv3x3_wino(x, wt, b2, add=s.clone().add_(b1.view(1, -1, 1, 1)))
    assert int((~torch.isfinite(want)).sum()) == 3
    # the output inside a larger buffer: the guard bands come back untouched
    buf = torch.full((GUARD + want.numel() + GUARD,), SENTINEL, device='cuda')
    y = buf[GUARD:GUARD + want.numel()].view_as(want)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = nhmc._lib.load().nhmc_conv3x3_wino_skip(P(x), P(K.wino_weights(wt)), P(b2), P(s), P(b1), P(y), n, c, k, h, w,
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert same_bits(y, want)
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + want.numel():] == SENTINEL).all())


def _block(seed=0):
    from nhmc import unet
    torch.manual_seed(seed)
    blk = unet.ResBlock(64, 32, 128).cuda().requires_grad_(False)
    blk.wino = True
    return blk


def _counting(monkeypatch):
    import nhmc.kernels as K
    calls = {'skip': 0, 'plain': 0}
    real, real_skip = K.conv3x3_wino, K.conv3x3_wino_skip

    def wino(*a, **kw):
        calls['plain'] += 1
        return real(*a, **kw)

    def skip(*a, **kw):
        calls['skip'] += 1
        return real_skip(*a, **kw)
    monkeypatch.setattr(K, 'conv3x3_wino', wino)
    monkeypatch.setattr(K, 'conv3x3_wino_skip', skip)
    return calls


def _run(blk, x0, emb, gout):
    x = x0.clone().requires_grad_(True)
    out = blk(x, emb)
    (gx,) = torch.autograd.grad(out, x, gout)
    return out.detach(), gx


@pytest.fixture(scope='module')
def block_case():
    gen = torch.Generator(device='cuda').manual_seed(5)
    x0 = torch.randn(2, 64, 64, 64, generator=gen, device='cuda')
    emb = torch.randn(2, 32, generator=gen, device='cuda')
    gout = torch.randn(2, 128, 64, 64, generator=gen, device='cuda')
    return x0, emb, gout


def test_resblock_is_bit_equal_to_the_bias_pass(monkeypatch, block_case):
    from nhmc import unet
    monkeypatch.delenv('NHMC_WINO_WAVES', raising=False)
    blk, calls = _block(), _counting(monkeypatch)
    assert isinstance(blk.skip_connection, unet.nn.Conv2d) and blk.skip_connection.bias is not None
    monkeypatch.setenv('NHMC_SKIP_BIAS', '0')
    out0, gx0 = _run(blk, *block_case)
    assert calls == {'skip': 0, 'plain': 4}                               # two forward, two backward-data passes
    monkeypatch.delenv('NHMC_SKIP_BIAS')
    out1, gx1 = _run(blk, *block_case)
    assert calls == {'skip': 1, 'plain': 7}
    assert out0.shape == (2, 128, 64, 64) and gx0.shape == (2, 64, 64, 64)
    assert same_bits(out1, out0) and same_bits(gx1, gx0)
    monkeypatch.setenv('NHMC_WINO_WAVES', '4')                            # four waves keep the pass
    out4, gx4 = _run(blk, *block_case)
    assert calls == {'skip': 1, 'plain': 11}
    assert same_bits(out4, out0) and same_bits(gx4, gx0)


def test_resblock_under_graph_replay(monkeypatch, block_case):
    monkeypatch.delenv('NHMC_WINO_WAVES', raising=False)
    monkeypatch.delenv('NHMC_SKIP_BIAS', raising=False)
    blk = _block()
    x0, emb, gout = block_case
    out0, gx0 = _run(blk, x0, emb, gout)
    calls = _counting(monkeypatch)
    xs = x0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                         # warm-up on the capture stream (allocator pools, U)
        _run(blk, xs, emb, gout)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g, gx_g = _run(blk, xs, emb, gout)
    assert calls == {'skip': 2, 'plain': 6}
    xs.copy_(torch.zeros_like(x0))
    graph.replay()
    xs.copy_(x0)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out_g, out0) and same_bits(gx_g, gx0)
