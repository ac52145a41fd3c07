"""GPU: the frequency-innermost operand layout of the Winograd convolution (csrc/wino_conv.hip): U as [C][K][16], both LDS
operands as rows of 16 frequencies with XOR-swizzled 16-byte granules, read with ds_read_b128.

Bound and yardstick are those of tests/test_wino_conv_gpu.py (max |err| / max |ref| against float64, at most twice the
plain-torch fp32 restatement's deviation on the same inputs).  Shapes (n, c, k, h, w) are the smallest at which the layout
can go wrong: one chunk (only the prologue's stage is multiplied); an odd chunk count with two K blocks and two column
blocks (stage parity, the K block's offset into U, the halo across an interior block edge); three K blocks, a workgroup
count that is no multiple of 8 (the un-permuted workgroup order).  A filter with one non-zero tap exercises single rows
and columns of G and of the flipped backward filter, which a random filter could blur within the tolerance."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_wino_conv_gpu import case, rel, restatement

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 64, 4, 64), (2, 24, 128, 8, 128), (1, 16, 192, 4, 64)]      # n, c, k, h, w


@pytest.mark.parametrize('backward', [0, 1], ids=['forward', 'backward_data'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_layout_against_float64(shape, backward):
    import nhmc.kernels as K
    cs = case(shape, backward)
    assert K.conv3x3_wino_covers(*shape)
    out = K.conv3x3_wino(cs['src'].cuda(), cs['w'].cuda(), backward=bool(backward))
    err = rel(out.cpu(), cs['ref'])
    print(f'\nwino layout {shape} {"bwd" if backward else "fwd"}: kernel {err:.3e}  restatement {cs["yard"]:.3e}')
    assert err <= 2 * cs['yard']


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_layout_epilogue_is_bias_add2_bit_for_bit(shape):
    import nhmc.kernels as K
    cs = case(shape, 0)
    x, wt = cs['src'].cuda(), cs['w'].cuda()
    gen = torch.Generator().manual_seed(5)
    bias = torch.randn(shape[2], generator=gen).cuda()
    add = torch.randn(shape[0], shape[2], shape[3], shape[4], generator=gen).cuda()
    plain = K.conv3x3_wino(x, wt)
    assert torch.equal(K.conv3x3_wino(x, wt, bias, add), K.bias_add2(plain, bias, add))


@pytest.mark.parametrize('backward', [0, 1], ids=['forward', 'backward_data'])
def test_single_tap_filters_at_each_of_the_nine_positions(backward):
    """w[:, :, r, s] random, every other tap zero: conv2d is then a channel mix of the input shifted by (r - 1, s - 1)."""
    import nhmc.kernels as K
    n, c, k, h, w = SHAPES[0]
    gen = torch.Generator().manual_seed(77 + backward)
    src = torch.randn(n, c, h, w, generator=gen)
    for r in range(3):
        for s in range(3):
            wt = torch.zeros((c, k, 3, 3) if backward else (k, c, 3, 3))
            wt[:, :, r, s] = torch.randn(wt.shape[:2], generator=gen) / c ** 0.5
            if backward:
                xd = torch.zeros(n, k, h, w, dtype=torch.float64, requires_grad=True)
                ref, = torch.autograd.grad(F.conv2d(xd, wt.double(), padding=1), xd, src.double())
                weff = wt.transpose(0, 1).flip(2, 3).contiguous()
            else:
                ref, weff = F.conv2d(src.double(), wt.double(), padding=1), wt
            yard = rel(restatement(src, weff), ref)
            err = rel(K.conv3x3_wino(src.cuda(), wt.cuda(), backward=bool(backward)).cpu(), ref)
            print(f'\nsingle tap ({r}, {s}) {"bwd" if backward else "fwd"}: kernel {err:.3e}  restatement {yard:.3e}')
            assert err <= 2 * yard
