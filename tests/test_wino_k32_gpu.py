"""GPU: the Winograd convolution (csrc/wino_conv.hip) at output-channel counts that are multiples of 32 but not of 64
(nhmc_conv3x3_wino_k32): the last block of 64 output channels is half empty, its kh = 1 waves multiply and store nothing,
and the upper 32 rows of its U stage are not read.

Bound and yardstick are those of tests/test_wino_conv_gpu.py (max |err| / max |ref| against float64, at most twice the
plain-torch fp32 restatement's deviation on the same inputs).  Shapes (n, c, k, h, w) are the smallest that reach each case:
a tail block alone in one workgroup; a full block and a tail at a workgroup count of 8 (the XCD permutation); three full
blocks and a tail with two column blocks; the 32-wide and the 16-wide geometry with a tail alone and behind full blocks."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.test_wino_conv_gpu import case, rel, restatement

pytestmark = pytest.mark.gpu

WIDE = [(1, 8, 32, 4, 64), (2, 24, 96, 8, 64), (1, 16, 224, 4, 128)]             # n, c, k, h, w
W32 = [(1, 8, 96, 8, 32), (2, 16, 32, 16, 32)]
W16 = [(1, 8, 32, 16, 16), (2, 8, 160, 16, 16)]
SHAPES = WIDE + W32 + W16
FULL = (2, 24, 64, 8, 64)                                                        # K % 64 == 0
ids = lambda s: 'x'.join(map(str, s))


def pad_k(wt, backward):
    """The filter with zero output channels (of the convolution that runs) up to the next multiple of 64."""
    k = wt.shape[1 if backward else 0]
    extra = -k % 64
    return F.pad(wt, (0, 0, 0, 0, 0, extra) if backward else (0, 0, 0, 0, 0, 0, 0, extra))


def raw_k32(x, wt, y, shape, bias=None, add=None, backward=False):
    """nhmc_conv3x3_wino_k32 itself, into the caller's y."""
    import nhmc
    import nhmc.kernels as K
    u = K.wino_weights(wt, backward)
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    rc = nhmc._lib.load().nhmc_conv3x3_wino_k32(p(x), p(u), p(bias), p(add), p(y), *shape, 1, 1, K._stream())
    assert rc == 0
    return y


@pytest.mark.parametrize('backward', [0, 1], ids=['forward', 'backward_data'])
@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_k32_against_float64(shape, backward):
    import nhmc.kernels as K
    cs = case(shape, backward)
    assert K.conv3x3_wino_k32_covers(*shape) and not K.conv3x3_wino_covers(*shape)
    out = K.conv3x3_wino(cs['src'].cuda(), cs['w'].cuda(), backward=bool(backward))
    err = rel(out.cpu(), cs['ref'])
    print(f'\nwino k32 {shape} {"bwd" if backward else "fwd"}: kernel {err:.3e}  restatement {cs["yard"]:.3e}')
    assert err <= 2 * cs['yard']


@pytest.mark.parametrize('backward', [0, 1], ids=['forward', 'backward_data'])
@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_a_channels_bits_do_not_depend_on_k(shape, backward):
    """The same filter with 32 zero output channels appended runs the existing entry (K % 64 == 0): equal bits."""
    import nhmc.kernels as K
    n, c, k, h, w = shape
    cs = case(shape, backward)
    x, wt = cs['src'].cuda(), cs['w'].cuda()
    wp = pad_k(wt, backward).contiguous()
    assert wp.shape[1 if backward else 0] == k + 32 and K.conv3x3_wino_covers(n, c, k + 32, h, w)
    got, padded = K.conv3x3_wino(x, wt, backward=bool(backward)), K.conv3x3_wino(x, wp, backward=bool(backward))
    assert torch.equal(got, padded[:, :k])
    assert not padded[:, k:].any()


@pytest.mark.parametrize('shape', [WIDE[1], W32[0], W16[1]], ids=ids)
def test_bits_do_not_depend_on_k_with_the_epilogue(shape):
    import nhmc.kernels as K
    n, c, k, h, w = shape
    cs = case(shape, 0)
    x, wt = cs['src'].cuda(), cs['w'].cuda()
    gen = torch.Generator().manual_seed(16)
    bias, add = torch.randn(k + 32, generator=gen).cuda(), torch.randn(n, k + 32, h, w, generator=gen).cuda()
    got = K.conv3x3_wino(x, wt, bias[:k].contiguous(), add[:, :k].contiguous())
    padded = K.conv3x3_wino(x, pad_k(wt, 0).contiguous(), bias, add)
    assert torch.equal(got, padded[:, :k])


def test_k32_entry_at_a_multiple_of_64_returns_the_existing_entrys_bits():
    import nhmc.kernels as K
    for backward in (0, 1):
        cs = case(FULL, backward)
        x, wt = cs['src'].cuda(), cs['w'].cuda()
        n, c, k, h, w = FULL
        y = raw_k32(x, wt, torch.full((n, k, h, w), 7.0).cuda(), FULL, backward=bool(backward))
        assert torch.equal(y, K.conv3x3_wino(x, wt, backward=bool(backward)))


@pytest.mark.parametrize('shape', [WIDE[0], WIDE[1]], ids=ids)
def test_nothing_is_written_outside_the_output(shape):
    """y is the head of a larger tensor of sentinels; the 32 channels the tail block does not own would land behind it."""
    import nhmc.kernels as K
    n, c, k, h, w = shape
    cs = case(shape, 0)
    x, wt = cs['src'].cuda(), cs['w'].cuda()
    size, guard = n * k * h * w, 64 * h * w
    buf = torch.full((size + guard,), -123.5).cuda()
    raw_k32(x, wt, buf, shape)
    torch.cuda.synchronize()
    assert bool((buf[size:] == -123.5).all())
    y = buf[:size].view(n, k, h, w)
    assert torch.equal(y, K.conv3x3_wino(x, wt))
    if n == 2:                                                                   # image 0's tail block stays out of image 1
        assert torch.equal(y[1:, :32], K.conv3x3_wino(x[1:].contiguous(), wt)[:, :32])


@pytest.mark.parametrize('shape', [WIDE[1], W16[1]], ids=ids)
def test_k32_epilogue_is_bias_add2_bit_for_bit(shape):
    import nhmc.kernels as K
    cs = case(shape, 0)
    x, wt = cs['src'].cuda(), cs['w'].cuda()
    gen = torch.Generator().manual_seed(6)
    bias = torch.randn(shape[2], generator=gen).cuda()
    add = torch.randn(shape[0], shape[2], shape[3], shape[4], generator=gen).cuda()
    plain = K.conv3x3_wino(x, wt)
    assert torch.equal(K.conv3x3_wino(x, wt, bias, add), K.bias_add2(plain, bias, add))
    assert torch.equal(K.conv3x3_wino(x, wt, bias), plain + bias.view(1, -1, 1, 1))


@pytest.mark.parametrize('shape', [WIDE[2], W32[0], W16[1]], ids=ids)
def test_k32_two_launches_give_equal_bits(shape):
    import nhmc.kernels as K
    for backward in (0, 1):
        cs = case(shape, backward)
        x, wt = cs['src'].cuda(), cs['w'].cuda()
        assert torch.equal(K.conv3x3_wino(x, wt, backward=bool(backward)), K.conv3x3_wino(x, wt, backward=bool(backward)))


@pytest.mark.parametrize('backward', [0, 1], ids=['forward', 'backward_data'])
def test_k32_single_tap_filters_differ_between_the_full_block_and_the_tail(backward):
    """Output channel 5 (the full block) has its only non-zero tap at (r, s), channel 64 + 9 (the tail) at the next of the
    nine positions, every other channel is zero: a tail channel read from another row of U is exact, not blurred."""
    import nhmc.kernels as K
    shape = n, c, k, h, w = (1, 8, 96, 4, 64)
    gen = torch.Generator().manual_seed(81 + backward)
    src = torch.randn(n, c, h, w, generator=gen)
    for pos in range(9):
        wt = torch.zeros((c, k, 3, 3) if backward else (k, c, 3, 3))
        for ko, q in ((5, pos), (73, (pos + 1) % 9)):
            tap = torch.randn(c, generator=gen) / c ** 0.5
            if backward:
                wt[:, ko, q // 3, q % 3] = tap
            else:
                wt[ko, :, q // 3, q % 3] = tap
        if backward:
            xd = torch.zeros(n, k, h, w, dtype=torch.float64, requires_grad=True)
            ref, = torch.autograd.grad(F.conv2d(xd, wt.double(), padding=1), xd, src.double())
            weff = wt.transpose(0, 1).flip(2, 3).contiguous()
        else:
            ref, weff = F.conv2d(src.double(), wt.double(), padding=1), wt
        yard = rel(restatement(src, weff), ref)
        out = K.conv3x3_wino(src.cuda(), wt.cuda(), backward=bool(backward)).cpu()
        err = rel(out, ref)
        print(f'\nk32 single tap {pos} {"bwd" if backward else "fwd"}: kernel {err:.3e}  restatement {yard:.3e}')
        assert err <= 2 * yard
        live = torch.zeros(k, dtype=torch.bool)
        live[[5, 73]] = True
        assert not out[:, ~live].any() and out[:, 5].any() and out[:, 73].any()
