"""GPU: the Winograd F(2x2, 3x3) convolution on the fp32 matrix cores (csrc/wino_conv.hip), forward and backward-data.

Accuracy is judged against float64 `F.conv2d` (backward-data: `torch.autograd.grad` of it), metric max |err| / max |ref|,
and the scale is set by a plain-torch fp32 restatement of the same algorithm written below (U = G w G^T, unfold(4, 2),
B^T d B, accumulation over c ascending, A^T M A): the kernel may deviate at most 2 x as far as the restatement does on the
same inputs -- the factor covers a different but fixed association inside the 4x4 transforms.  The restatement itself is
first validated in float64 (a few ulp of float64).  Shapes are the smallest that reach each part of the kernel with its
4-row x 64-column output block: one chunk and one workgroup with all four borders; an odd chunk count, a batch stride
and a row seam; two K blocks, a column seam and the U-Net's smallest C; H != W."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 64, 4, 64), (2, 24, 64, 8, 64), (1, 128, 128, 16, 128), (3, 16, 64, 12, 192)]      # n, c, k, h, w
G = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
AT = [[1, 1, 1, 0], [0, 1, -1, -1]]


def restatement(x, w):
    """F(2x2, 3x3) of conv2d(x, w, padding=1) in x's dtype, plain torch on the CPU."""
    g, bt, at = (torch.tensor(m, dtype=x.dtype) for m in (G, BT, AT))
    n, c, h, wd = x.shape
    u = g @ w @ g.T                                                        # [K, C, 4, 4]
    d = F.pad(x, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)             # [N, C, th, tw, 4, 4]
    v = bt @ d @ bt.T
    m = torch.zeros(n, w.shape[0], h // 2, wd // 2, 4, 4, dtype=x.dtype)
    for ci in range(c):
        m += u[None, :, ci, None, None] * v[:, None, ci]
    y = at @ m @ at.T                                                      # [N, K, th, tw, 2, 2]
    return y.permute(0, 1, 2, 4, 3, 5).reshape(n, w.shape[0], h, wd)


def rel(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


_cases = {}


def case(shape, backward):
    """Inputs, the float64 reference and the restatement's deviation for one shape and direction, computed once.  The
    shape is that of the convolution the KERNEL runs, c channels in and k out: forward it is conv2d(x [n, c], w [k, c]);
    backward-data it is the input gradient of a k -> c convolution, w [c, k], from the output gradient dy [n, c]."""
    if (shape, backward) not in _cases:
        n, c, k, h, w = shape
        gen = torch.Generator().manual_seed(1000 + c + h + backward)
        src = torch.randn(n, c, h, w, generator=gen)
        if backward:
            wt = torch.randn(c, k, 3, 3, generator=gen) / (9 * c) ** 0.5
            xd = torch.zeros(n, k, h, w, dtype=torch.float64, requires_grad=True)
            ref, = torch.autograd.grad(F.conv2d(xd, wt.double(), padding=1), xd, src.double())
            weff = wt.transpose(0, 1).flip(2, 3).contiguous()              # the backward-data pass is conv(dy, w')
        else:
            wt = weff = torch.randn(k, c, 3, 3, generator=gen) / (9 * c) ** 0.5
            ref = F.conv2d(src.double(), wt.double(), padding=1)
        assert rel(restatement(src.double(), weff.double()), ref) <= 5e-15  # the yardstick is right: a few ulp of float64
        _cases[shape, backward] = dict(src=src, w=wt, ref=ref, yard=rel(restatement(src, weff), ref),
                                       direct=rel(F.conv2d(src, weff, padding=1), ref))
    return _cases[shape, backward]


@pytest.mark.parametrize('backward', [0, 1], ids=['forward', 'backward_data'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_against_float64(shape, backward):
    import nhmc.kernels as K
    cs = case(shape, backward)
    n, c, k, h, w = shape
    assert K.conv3x3_wino_covers(n, c, k, h, w)
    src, wt = cs['src'].cuda(), cs['w'].cuda()
    out = K.conv3x3_wino(src, wt, backward=bool(backward))
    vendor = torch.nn.grad.conv2d_input((n, k, h, w), wt, src, 1, 1) if backward else F.conv2d(src, wt, padding=1)
    err, yard = rel(out.cpu(), cs['ref']), cs['yard']
    print(f'\nwino {shape} {"bwd" if backward else "fwd"}: kernel {err:.3e}  restatement {yard:.3e}  '
          f'direct fp32 (CPU) {cs["direct"]:.3e}  vendor fp32 (GPU) {rel(vendor.cpu(), cs["ref"]):.3e}')
    assert err <= 2 * yard


def test_epilogue_is_bias_add2_bit_for_bit():
    import nhmc.kernels as K
    cs = case(SHAPES[1], 0)
    x, wt = cs['src'].cuda(), cs['w'].cuda()
    torch.manual_seed(3)
    bias, add = torch.randn(wt.shape[0]).cuda(), torch.randn(x.shape[0], wt.shape[0], *x.shape[2:]).cuda()
    plain = K.conv3x3_wino(x, wt)
    assert torch.equal(K.conv3x3_wino(x, wt, bias, add), K.bias_add2(plain, bias, add))
    assert torch.equal(K.conv3x3_wino(x, wt, bias), plain + bias.view(1, -1, 1, 1))


def test_two_launches_give_equal_bits():
    import nhmc.kernels as K
    for backward in (0, 1):
        cs = case(SHAPES[2], backward)
        x, wt = cs['src'].cuda(), cs['w'].cuda()
        assert torch.equal(K.conv3x3_wino(x, wt, backward=bool(backward)), K.conv3x3_wino(x, wt, backward=bool(backward)))


def test_weight_cache_is_built_once_and_follows_an_edit():
    import nhmc.kernels as K
    torch.manual_seed(4)
    x, wt = torch.randn(1, 64, 4, 64).cuda(), (torch.randn(64, 64, 3, 3) / 24).cuda()
    n0 = K.wino_weight_builds()
    y = K.conv3x3_wino(x, wt)
    for _ in range(3):
        K.conv3x3_wino(x, wt)
    assert K.wino_weight_builds() == n0 + 1
    K.conv3x3_wino(y, wt, backward=True)                                   # the other direction has a table of its own
    assert K.wino_weight_builds() == n0 + 2
    wt.mul_(2.0)                                                           # in place: same address, new version
    y2 = K.conv3x3_wino(x, wt)
    assert K.wino_weight_builds() == n0 + 3
    assert torch.equal(y2, 2.0 * y)                                        # a power of two scales every rounding step exactly
    K.conv3x3_wino(x, wt)
    assert K.wino_weight_builds() == n0 + 3


def test_resblock_graph_replays_the_eager_bits_and_matches_the_vendor_route(monkeypatch):
    """Forward + input gradient of a ResBlock(128, 512, 128) at (1, 128, 64, 64) with both convolutions forced onto the
    kernel (the routing table may not list this batch size's shape): a captured graph gives the eager bits on both
    replays, and NHMC_WINO=0 (the vendor library) agrees within 1e-5 relative, the bound tests/test_hygiene_gpu.py uses
    between solver choices."""
    from nhmc import unet
    import nhmc.kernels as K
    torch.manual_seed(8)
    blk = unet.ResBlock(128, 512, 128).cuda().eval().requires_grad_(False)
    blk.wino = True
    x = torch.randn(1, 128, 64, 64).cuda().requires_grad_(True)
    emb, dy = torch.randn(1, 512).cuda(), torch.randn(1, 128, 64, 64).cuda()

    def step():
        y = blk(x, emb)
        return (y,) + torch.autograd.grad(y, (x,), dy)
    assert unet.wino_route(blk.in_layers[2], x, True) == (True, True)
    n0 = K.wino_weight_builds()
    eager = [t.detach().clone() for t in step()]
    assert K.wino_weight_builds() == n0 + 4                                # the kernel ran: two filters, two directions
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
    assert K.wino_weight_builds() == n0 + 4
    monkeypatch.setenv('NHMC_WINO', '0')
    assert unet.wino_route(blk.in_layers[2], x, True) is None
    for a, b in zip(eager, step()):
        assert float((a - b.detach()).abs().max()) <= 1e-5 * float(a.abs().max())
