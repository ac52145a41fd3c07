"""GPU: the narrow geometries of the Winograd convolution (csrc/wino_conv.hip): the workgroup's 64 tiles as 4 x 16 for
images 32 wide and 8 x 8 for images 16 wide, instead of 2 x 32 (nhmc_conv3x3_wino_narrow, chosen by width in
kernels.conv3x3_wino).

Bound and yardstick are those of tests/test_wino_conv_gpu.py (max |err| / max |ref| against float64, at most twice the
plain-torch fp32 restatement's deviation on the same inputs).  Shapes (n, c, k, h, w) are the smallest at which the
geometry's index arithmetic (the loader's patch origin, the block origin, the epilogue's output origin) can go wrong: one
workgroup and one chunk; two row blocks with two K blocks and an odd chunk count at a workgroup count that is a multiple
of 8 (the XCD permutation) or is not; H != W.  A filter with one non-zero tap makes a misplaced tile or halo exact
instead of blurred into the tolerance."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_wino_conv_gpu import case, rel, restatement

pytestmark = pytest.mark.gpu

SHAPES_32 = [(1, 8, 64, 8, 32), (2, 24, 128, 16, 32), (1, 16, 192, 8, 32)]       # n, c, k, h, w
SHAPES_16 = [(1, 8, 64, 16, 16), (3, 24, 128, 32, 16), (2, 16, 128, 32, 16)]
SHAPES = SHAPES_32 + SHAPES_16
ids = lambda s: 'x'.join(map(str, s))


@pytest.mark.parametrize('backward', [0, 1], ids=['forward', 'backward_data'])
@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_narrow_against_float64(shape, backward):
    import nhmc.kernels as K
    cs = case(shape, backward)
    assert K.conv3x3_wino_covers(*shape)
    out = K.conv3x3_wino(cs['src'].cuda(), cs['w'].cuda(), backward=bool(backward))
    err = rel(out.cpu(), cs['ref'])
    print(f'\nwino narrow {shape} {"bwd" if backward else "fwd"}: kernel {err:.3e}  restatement {cs["yard"]:.3e}')
    assert err <= 2 * cs['yard']


@pytest.mark.parametrize('backward', [0, 1], ids=['forward', 'backward_data'])
@pytest.mark.parametrize('shape', [SHAPES_32[0], SHAPES_16[0]], ids=ids)
def test_narrow_single_tap_filters_at_each_of_the_nine_positions(shape, backward):
    """w[:, :, r, s] random, every other tap zero: conv2d is then a channel mix of the input shifted by (r - 1, s - 1)."""
    import nhmc.kernels as K
    n, c, k, h, w = shape
    gen = torch.Generator().manual_seed(78 + backward + w)
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
            print(f'\nnarrow single tap ({r}, {s}) w = {w} {"bwd" if backward else "fwd"}: kernel {err:.3e}  restatement {yard:.3e}')
            assert err <= 2 * yard


@pytest.mark.parametrize('shape', [SHAPES_32[1], SHAPES_16[1]], ids=ids)
def test_narrow_epilogue_is_bias_add2_bit_for_bit(shape):
    import nhmc.kernels as K
    cs = case(shape, 0)
    x, wt = cs['src'].cuda(), cs['w'].cuda()
    gen = torch.Generator().manual_seed(6)
    bias = torch.randn(shape[2], generator=gen).cuda()
    add = torch.randn(shape[0], shape[2], shape[3], shape[4], generator=gen).cuda()
    plain = K.conv3x3_wino(x, wt)
    assert torch.equal(K.conv3x3_wino(x, wt, bias, add), K.bias_add2(plain, bias, add))
    assert torch.equal(K.conv3x3_wino(x, wt, bias), plain + bias.view(1, -1, 1, 1))


@pytest.mark.parametrize('shape', [SHAPES_32[1], SHAPES_16[1]], ids=ids)
def test_narrow_two_launches_give_equal_bits(shape):
    import nhmc.kernels as K
    for backward in (0, 1):
        cs = case(shape, backward)
        x, wt = cs['src'].cuda(), cs['w'].cuda()
        assert torch.equal(K.conv3x3_wino(x, wt, backward=bool(backward)), K.conv3x3_wino(x, wt, backward=bool(backward)))


def test_resblock_at_32x32_runs_the_kernel_and_matches_the_vendor_route(monkeypatch):
    """Forward + input gradient of a ResBlock(256, 512, 256) at (1, 256, 32, 32) with both convolutions forced onto the
    kernel; NHMC_WINO=0 (the vendor library) agrees within 1e-5 relative, the bound of the ResBlock test in
    tests/test_wino_conv_gpu.py."""
    from nhmc import unet
    import nhmc.kernels as K
    torch.manual_seed(9)
    blk = unet.ResBlock(256, 512, 256).cuda().eval().requires_grad_(False)
    blk.wino = True
    x = torch.randn(1, 256, 32, 32).cuda().requires_grad_(True)
    emb, dy = torch.randn(1, 512).cuda(), torch.randn(1, 256, 32, 32).cuda()

    def step():
        y = blk(x, emb)
        return (y,) + torch.autograd.grad(y, (x,), dy)
    assert unet.wino_route(blk.in_layers[2], x, True) == (True, True)
    n0 = K.wino_weight_builds()
    ours = [t.detach().clone() for t in step()]
    assert K.wino_weight_builds() == n0 + 4                                # the kernel ran: two filters, two directions
    monkeypatch.setenv('NHMC_WINO', '0')
    assert unet.wino_route(blk.in_layers[2], x, True) is None
    for a, b in zip(ours, step()):
        dev = float((a - b.detach()).abs().max()) / float(a.abs().max())
        print(f'\nResBlock 32 x 32: kernel route vs vendor route {dev:.3e}')
        assert dev <= 1e-5
