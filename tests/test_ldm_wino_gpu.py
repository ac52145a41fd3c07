"""GPU: the latent sampler's blocks (nhmc.ldm) with their 3x3 convolutions on the Winograd kernel, at output-channel counts
of 64 and of 96 (a tail block, nhmc_conv3x3_wino_k32).  Each block is compared with itself under NHMC_WINO=0 (the vendor
library) within 1e-5 relative (max |a - b| / max |a|), the bound of the ResBlock tests in tests/test_wino_conv_gpu.py and
tests/test_wino_narrow_gpu.py, which tests/test_hygiene_gpu.py uses between solver choices."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def close(a, b):
    dev = float((a - b).abs().max()) / float(a.abs().max())
    print(f'\nkernel route vs vendor route {dev:.3e}')
    return dev <= 1e-5


def block(make, seed):
    torch.manual_seed(seed)
    blk = make().cuda().eval().requires_grad_(False)
    blk.wino = True
    return blk


@pytest.mark.parametrize('xshape', [(2, 64, 16, 16), (1, 64, 64, 64)], ids=['16x16', '64x64'])
def test_add_emb_resblock_without_gradient(xshape, monkeypatch):
    from nhmc import ldm, unet
    import nhmc.kernels as K
    blk = block(lambda: ldm.AddEmbResBlock(64, 128, 96), 21)
    x, emb = torch.randn(*xshape).cuda(), torch.randn(xshape[0], 128).cuda()
    with torch.no_grad():
        assert unet.wino_route(blk.in_layers[2], x, True) == (True, False)
        n0 = K.wino_weight_builds()
        ours = blk(x, emb)
        assert K.wino_weight_builds() == n0 + 2                                # the kernel ran: two filters, forward only
        monkeypatch.setenv('NHMC_WINO', '0')
        assert unet.wino_route(blk.in_layers[2], x, True) is None
        assert close(ours, blk(x, emb))
        assert K.wino_weight_builds() == n0 + 2


def test_plain_resblock_with_gradient(monkeypatch):
    from nhmc import ldm, unet
    import nhmc.kernels as K
    blk = block(lambda: ldm.PlainResBlock(64, 96), 22)
    x, dy = torch.randn(2, 64, 16, 16).cuda().requires_grad_(True), torch.randn(2, 96, 16, 16).cuda()

    def step():
        y = blk(x)
        return (y,) + torch.autograd.grad(y, (x,), dy)
    assert unet.wino_route(blk.conv1, x, True) == (True, True)
    n0 = K.wino_weight_builds()
    ours = [t.detach().clone() for t in step()]
    assert K.wino_weight_builds() == n0 + 4                                    # two filters, two directions
    monkeypatch.setenv('NHMC_WINO', '0')
    for a, b in zip(ours, step()):
        assert close(a, b.detach())


@pytest.mark.parametrize('forward_routed', [True, False], ids=['both_routed', 'backward_only'])
@pytest.mark.parametrize('which', ['UpConv64', 'ConvUp96'])
def test_upsampling_convolutions_keep_their_bias(which, forward_routed, monkeypatch):
    """The convolution runs at 32 x 32 behind the nearest-2x upsample.  With the forward pass on the vendor library and the
    backward-data pass on the kernel, the bias must still be in the output."""
    from nhmc import ldm, unet
    import nhmc.kernels as K
    ch = 64 if which == 'UpConv64' else 96
    blk = block(lambda: (ldm.UpConv if which == 'UpConv64' else ldm.ConvUp)(ch), 23)
    with torch.no_grad():
        blk.conv.bias.normal_()
    x, dy = torch.randn(2, ch, 16, 16).cuda().requires_grad_(True), torch.randn(2, ch, 32, 32).cuda()
    if not forward_routed:
        covers, calls = K.conv3x3_wino_k32_covers, []

        def forward_refused(*shape):                                            # wino_route asks forward, then backward
            calls.append(shape)
            return False if len(calls) % 2 == 1 else covers(*shape)
        monkeypatch.setattr(K, 'conv3x3_wino_k32_covers', forward_refused)
    up = torch.nn.functional.interpolate(x, scale_factor=2, mode='nearest')
    assert unet.wino_route(blk.conv, up, True) == (forward_routed, True)

    def step():
        y = blk(x)
        return (y,) + torch.autograd.grad(y, (x,), dy)
    n0 = K.wino_weight_builds()
    ours = [t.detach().clone() for t in step()]
    assert K.wino_weight_builds() == n0 + (2 if forward_routed else 1)
    monkeypatch.setenv('NHMC_WINO', '0')
    assert unet.wino_route(blk.conv, up, True) is None
    theirs = step()
    for a, b in zip(ours, theirs):
        assert close(a, b.detach())
    nobias = torch.nn.functional.conv2d(up.detach(), blk.conv.weight, None, 1, 1)
    assert not close(ours[0], nobias)                                          # the bias is large enough to be seen


def test_add_emb_resblock_graph_replays_the_eager_bits():
    from nhmc import ldm
    import nhmc.kernels as K
    blk = block(lambda: ldm.AddEmbResBlock(64, 128, 96), 24)
    x, emb = torch.randn(2, 64, 16, 16).cuda(), torch.randn(2, 128).cuda()
    with torch.no_grad():
        n0 = K.wino_weight_builds()
        eager = blk(x, emb).clone()
        assert K.wino_weight_builds() == n0 + 2
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                blk(x, emb)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = blk(x, emb)
        for _ in range(2):
            captured.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(eager, captured)
        assert K.wino_weight_builds() == n0 + 2
