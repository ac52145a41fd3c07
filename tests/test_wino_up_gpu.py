"""GPU: the upsample forms of the eight-wave Winograd convolution (csrc/wino_conv.hip, "Nearest 2x upsample";
nhmc_conv3x3_wino_up) give the bits of today's kernels composed on the materialised tensor.

  IN_UP     conv3x3_wino(upsample(x_low), w, bias)                      x read at half resolution, 7 of 16 frequencies skipped
  ADD_UP    conv3x3_wino(h, w, bias, add=upsample(x_low))               the residual read at half resolution
  OUT_POOL  sr_H(conv3x3_wino(g, w, backward=True), 2).mul_(4.0)        the 2 x 2 block sums stored from the epilogue

The composition is the reference (tests/test_wino_bits_gpu.py pins its bits).  nhmc_sr_Ht and nhmc_sr_H take square planes
only, and four of the five shapes are not square; there the upsample is an index gather and the block sum is k_sr<2, 1>'s
own chain ((((0 + y00) + y01) + y10) + y11) * 0.25f, then * 4.0f, in torch fp32 arithmetic -- and both stand-ins are held
against nhmc_sr_Ht (scale 1.0) and nhmc_sr_H bit for bit at the square shape, where the kernels themselves are the reference.

Shapes (n, C, K, H_out, W_out): one block with one chunk; two row and two column blocks with two chunks (both stages) and a
grid that is a multiple of 8 (the XCD remap); an odd chunk count with two K blocks; three column blocks (an interior one
with both edge lanes loading) on a grid that is not a multiple of 8; the network's smallest wide up-shape.
Inputs: normal draws (outputs between sentinels); a tensor of -0.0, +0.0 and normal draws; integers with single-tap filters,
which must return the shifted upsampled input exactly; one NaN and one inf pixel, for which the set of non-finite outputs
must be the reference's (the skipped products held inf - inf, so the values there may differ).

One up-sampling ResBlock: output and input gradient bit-equal between NHMC_WINO_UP=0 and the default, eagerly and under a
hipGraph replay; NHMC_WINO_WAVES=4 falls back to the materialised path."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 64, 4, 64), (2, 16, 64, 8, 128), (1, 24, 128, 8, 64), (3, 40, 64, 12, 192), (1, 256, 256, 64, 64)]
KINDS = ['normal', 'zeros', 'taps', 'nonfinite']
GUARD, SENTINEL = 4096, -12345.0
ids = lambda s: 'x'.join(map(str, s))


def upsample(t):
    """Nearest 2x: the values of nhmc_sr_Ht with scale 1.0 (v * 1.0f = v)."""
    h, w = t.shape[2], t.shape[3]
    iy, ix = torch.arange(2 * h, device=t.device) // 2, torch.arange(2 * w, device=t.device) // 2
    return t[:, :, iy][:, :, :, ix].contiguous()


def pool4(y):
    """k_sr<2, 1>'s chain over each 2 x 2 block, then _Resample2x.backward's mul_(4.0)."""
    s = torch.zeros_like(y[:, :, 0::2, 0::2])
    for part in (y[:, :, 0::2, 0::2], y[:, :, 0::2, 1::2], y[:, :, 1::2, 0::2], y[:, :, 1::2, 1::2]):
        s = s + part
    return (s * 0.25).mul_(4.0)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def draw(kind, shape, gen, special_at=None):
    t = torch.randn(shape, generator=gen, device='cuda')
    if kind == 'zeros':
        pick = torch.randint(0, 4, shape, generator=gen, device='cuda')
        t = torch.where(pick == 0, torch.full_like(t, -0.0), torch.where(pick == 1, torch.zeros_like(t), t))
    elif kind == 'taps':
        t = torch.randint(-8, 9, shape, generator=gen, device='cuda').float()
    elif kind == 'nonfinite':
        flat = t.view(-1)
        flat[flat.numel() // 3] = float('nan')
        flat[(2 * flat.numel()) // 3 + 1] = float('inf')
    return t


def tap_filter(k_out, c_in, tap, gen):
    """w[k][k % c_in][tap] = 1: output channel k of a forward pass is input channel k % c_in shifted by the tap."""
    w = torch.zeros(k_out, c_in, 3, 3, device='cuda')
    w[torch.arange(k_out), torch.arange(k_out) % c_in, tap // 3, tap % 3] = 1.0
    return w


def shifted(img, tap):
    """conv2d(img, single tap at (r, s)) = img[y + r - 1][x + s - 1] with zero padding."""
    r, s = tap // 3, tap % 3
    return torch.nn.functional.pad(img, (1, 1, 1, 1))[:, :, r:r + img.shape[2], s:s + img.shape[3]]


def guarded_call(K, lib, x, weight, mode, bias, add, backward, out_shape):
    """nhmc_conv3x3_wino_up into the middle of a sentinel-filled allocation -> (y, whole)."""
    u = K.wino_weights(weight, backward)
    n_out = out_shape[0] * out_shape[1] * out_shape[2] * out_shape[3]
    whole = torch.full((2 * GUARD + n_out,), SENTINEL, device='cuda')
    y = whole[GUARD:GUARD + n_out].view(out_shape)
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    n, c = x.shape[0], x.shape[1]
    h, w = (2 * x.shape[2], 2 * x.shape[3]) if mode == K.WINO_IN_UP else (x.shape[2], x.shape[3])
    rc = lib.nhmc_conv3x3_wino_up(p(x), p(u), p(bias), p(add), p(y), n, c, u.shape[2], h, w, mode, K._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert (whole[:GUARD] == SENTINEL).all() and (whole[GUARD + n_out:] == SENTINEL).all(), 'a write outside the output'
    return y


def compare(kind, got, ref, what):
    if kind == 'nonfinite':
        assert not torch.isfinite(ref).all(), f'{what}: the case holds no non-finite output'
        assert torch.equal(torch.isfinite(got), torch.isfinite(ref)), f'{what}: the non-finite positions differ'
        fin = torch.isfinite(ref)
        assert same_bits(got[fin], ref[fin]), f'{what}: finite outputs differ'
    else:
        assert torch.isfinite(ref).all()
        assert same_bits(got, ref), f'{what}: bits differ from the composition on the materialised tensor'


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_the_three_forms_against_the_materialised_composition(monkeypatch, shape, kind):
    import nhmc
    import nhmc.kernels as K
    monkeypatch.delenv('NHMC_WINO_WAVES', raising=False)
    monkeypatch.delenv('NHMC_WINO_UP', raising=False)
    lib = nhmc._lib.load()
    n, c, k, h, w = shape
    assert K.conv3x3_wino_up_covers(n, c, k, h, w)
    gen = torch.Generator(device='cuda').manual_seed(1000 * SHAPES.index(shape) + KINDS.index(kind))
    tap = (SHAPES.index(shape) * 4 + 1) % 9                              # 1, 5, 0, 4, 8 over the shapes
    weight = tap_filter(k, c, tap, gen) if kind == 'taps' else torch.randn(k, c, 3, 3, generator=gen, device='cuda') / (9 * c) ** 0.5
    bias = draw('taps' if kind == 'taps' else 'normal', (k,), gen)
    # the filter of a layer k -> c, whose backward-data pass is the convolution c -> k that OUT_POOL runs
    weight_t = weight.transpose(0, 1).flip(2, 3).contiguous()
    wrap = (lambda x, mode, b, a, bw, out: K.conv3x3_wino_up(x, weight_t if bw else weight, mode, b, a, backward=bw)) \
        if kind != 'normal' else (lambda x, mode, b, a, bw, out: guarded_call(K, lib, x, weight_t if bw else weight, mode, b, a, bw, out))

    # IN_UP
    x_low = draw(kind, (n, c, h // 2, w // 2), gen)
    x_up = upsample(x_low)
    for b in (None, bias):
        ref = K.conv3x3_wino(x_up, weight, b)
        got = wrap(x_low, K.WINO_IN_UP, b, None, False, (n, k, h, w))
        compare(kind, got, ref, f'IN_UP bias={b is not None}')
    if kind == 'taps':
        assert torch.equal(got, shifted(x_up, tap)[:, torch.arange(k, device='cuda') % c] + bias.view(1, -1, 1, 1))

    # ADD_UP: the special values sit in the low-res residual
    hh = draw('normal' if kind == 'nonfinite' else kind, (n, c, h, w), gen)
    a_low = draw(kind, (n, k, h // 2, w // 2), gen)
    ref = K.conv3x3_wino(hh, weight, bias, upsample(a_low))
    got = wrap(hh, K.WINO_ADD_UP, bias, a_low, False, (n, k, h, w))
    compare(kind, got, ref, 'ADD_UP')

    # OUT_POOL: a backward-data pass, the gradient g [n, c, h, w] -> [n, k, h / 2, w / 2]
    g = draw(kind, (n, c, h, w), gen)
    ref = pool4(K.conv3x3_wino(g, weight_t, backward=True))
    got = wrap(g, K.WINO_OUT_POOL, None, None, True, (n, k, h // 2, w // 2))
    compare(kind, got, ref, 'OUT_POOL')


def test_the_stand_ins_are_the_block_mean_kernels_at_the_square_shape():
    import nhmc.kernels as K
    gen = torch.Generator(device='cuda').manual_seed(7)
    n, c, d = 2, 24, 64
    x_low = draw('zeros', (n, c, d // 2, d // 2), gen)
    assert same_bits(K.sr_Ht(x_low.reshape(n, -1), 2, c, d, 1.0).view(n, c, d, d), upsample(x_low))
    y = draw('zeros', (n, c, d, d), gen)
    y.view(-1)[::5] *= 1e-38                                              # sums and means in the denormal range too
    assert same_bits(K.sr_H(y, 2).view(n, c, d // 2, d // 2).mul_(4.0), pool4(y))


def test_argument_validation():
    import nhmc
    import nhmc.kernels as K
    lib = nhmc._lib.load()
    P = ctypes.c_void_p
    a, b, c, d, null = P(0x1000), P(0x2000), P(0x3000), P(0x4000), P(0)
    call = lambda add, bias, y, mode, w=64: lib.nhmc_conv3x3_wino_up(a, b, bias, add, y, 1, 8, 64, 4, w, mode, None)
    assert call(null, null, c, 3) == 1 and call(null, null, c, 0) == 1                         # one mode exactly
    assert call(d, null, c, K.WINO_IN_UP) == 1 and call(null, null, c, K.WINO_ADD_UP) == 1      # add with ADD_UP only
    assert call(c, null, c, K.WINO_ADD_UP) == 1 and call(null, d, c, K.WINO_OUT_POOL) == 1
    assert call(null, null, c, K.WINO_IN_UP, w=32) == 3                                         # the wide geometry only
    assert call(null, null, P(0x3004), K.WINO_IN_UP) == 2


def _block(seed=0):
    from nhmc import unet
    torch.manual_seed(seed)
    blk = unet.ResBlock(64, 32, 64, up=True).cuda().requires_grad_(False)
    blk.wino = True
    return blk


def _counting(monkeypatch):
    import nhmc.kernels as K
    calls = {'up': 0, 'sr_Ht': 0}
    real_up, real_ht = K.conv3x3_wino_up, K.sr_Ht

    def up(*a, **kw):
        calls['up'] += 1
        return real_up(*a, **kw)

    def ht(*a, **kw):
        calls['sr_Ht'] += 1
        return real_ht(*a, **kw)
    monkeypatch.setattr(K, 'conv3x3_wino_up', up)
    monkeypatch.setattr(K, 'sr_Ht', ht)
    return calls


def _run(blk, x0, emb, gout):
    x = x0.clone().requires_grad_(True)
    out = blk(x, emb)
    (gx,) = torch.autograd.grad(out, x, gout)
    return out.detach(), gx


@pytest.fixture(scope='module')
def block_case():
    gen = torch.Generator(device='cuda').manual_seed(5)
    x0 = torch.randn(2, 64, 32, 32, generator=gen, device='cuda')
    emb = torch.randn(2, 32, generator=gen, device='cuda')
    gout = torch.randn(2, 64, 64, 64, generator=gen, device='cuda')
    return x0, emb, gout


def test_resblock_up_is_bit_equal_to_the_materialised_path(monkeypatch, block_case):
    monkeypatch.delenv('NHMC_WINO_WAVES', raising=False)
    blk, calls = _block(), _counting(monkeypatch)
    monkeypatch.setenv('NHMC_WINO_UP', '0')
    out0, gx0 = _run(blk, *block_case)
    assert calls == {'up': 0, 'sr_Ht': 2}                                 # h_upd and x_upd
    monkeypatch.delenv('NHMC_WINO_UP')
    out1, gx1 = _run(blk, *block_case)
    assert calls == {'up': 3, 'sr_Ht': 2}                                 # conv1 forward, conv2 forward, conv1 backward; no upsample
    assert out0.shape == (2, 64, 64, 64) and gx0.shape == (2, 64, 32, 32)
    assert same_bits(out1, out0) and same_bits(gx1, gx0)


def test_resblock_up_under_graph_replay(monkeypatch, block_case):
    monkeypatch.delenv('NHMC_WINO_WAVES', raising=False)
    blk = _block()
    x0, emb, gout = block_case
    monkeypatch.setenv('NHMC_WINO_UP', '0')
    out0, gx0 = _run(blk, x0, emb, gout)
    monkeypatch.delenv('NHMC_WINO_UP')
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
    assert calls == {'up': 6, 'sr_Ht': 0}
    xs.copy_(torch.zeros_like(x0))
    graph.replay()
    xs.copy_(x0)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out_g, out0) and same_bits(gx_g, gx0)


def test_four_waves_fall_back_to_the_materialised_path(monkeypatch, block_case):
    blk = _block()
    monkeypatch.delenv('NHMC_WINO_UP', raising=False)
    monkeypatch.delenv('NHMC_WINO_WAVES', raising=False)
    out8, gx8 = _run(blk, *block_case)
    calls = _counting(monkeypatch)
    monkeypatch.setenv('NHMC_WINO_WAVES', '4')
    out4, gx4 = _run(blk, *block_case)
    assert calls == {'up': 0, 'sr_Ht': 2}
    assert same_bits(out4, out8) and same_bits(gx4, gx8)
