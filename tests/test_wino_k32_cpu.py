"""CPU: the Winograd convolution's entry for output-channel counts that are multiples of 32 (nhmc_conv3x3_wino_k32*,
csrc/wino_conv.hip) answers its host-only queries and validates its arguments before any device work, in the order of the
existing entries (tests/test_wino_conv_cpu.py); the latent networks' shape lists (ldm.conv3x3_shapes) are the models' own
and tools/conv_bench.py --latent takes its shapes from them; the latent blocks compute on CPU tensors what they did before
they had a `wino` attribute."""
import ctypes
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

# (C, K, resolution): count -- every 3x3 stride-1 padding-1 Conv2d call of one forward pass on a [1, 3, 64, 64] latent
UNET = {
    (3, 224, 64): 1, (224, 3, 64): 1, (224, 224, 64): 7, (448, 224, 64): 2, (448, 448, 64): 1, (672, 224, 64): 1,
    (224, 448, 32): 1, (448, 448, 32): 6, (672, 448, 32): 1, (672, 672, 32): 1, (896, 448, 32): 1, (1120, 448, 32): 1,
    (448, 672, 16): 1, (672, 672, 16): 6, (896, 896, 16): 1, (1120, 672, 16): 1, (1344, 672, 16): 1, (1568, 672, 16): 1,
    (672, 896, 8): 1, (896, 896, 8): 10, (1568, 896, 8): 1, (1792, 896, 8): 2,
}
DECODER = {
    (128, 3, 256): 1, (128, 128, 256): 5, (256, 128, 256): 1, (256, 256, 256): 1, (256, 256, 128): 5, (512, 256, 128): 1,
    (512, 512, 128): 1, (3, 512, 64): 1, (512, 512, 64): 10,
}


@pytest.fixture(scope='module')
def lib():
    import nhmc
    return nhmc._lib.load()


@pytest.mark.parametrize('which, want', [('unet', UNET), ('decoder', DECODER)])
def test_latent_shape_lists_are_the_networks(which, want):
    from nhmc import ldm
    got = ldm.conv3x3_shapes(which)
    assert len(got) == len(want)                                                 # no shape twice
    assert {(c, k, res): n for c, k, res, n in got} == want
    assert [s[2] for s in got] == sorted((s[2] for s in got), reverse=True)
    with pytest.raises(ValueError):
        ldm.conv3x3_shapes('encoder')


def test_k32_coverage_is_a_superset_of_the_two_existing_queries(lib):
    cov = lib.nhmc_conv3x3_wino_k32_covers
    for shape in ((16, 224, 224, 64, 64), (16, 448, 224, 64, 64), (16, 672, 672, 32, 32), (16, 1568, 672, 16, 16),
                  (1, 8, 32, 4, 64), (1, 8, 96, 8, 32), (1, 8, 32, 16, 16)):
        assert cov(*shape) == 1, shape
    for shape in ((64, 128, 128, 256, 256), (3, 16, 64, 12, 192), (64, 768, 256, 64, 64), (1, 8, 64, 4, 64)):
        assert lib.nhmc_conv3x3_wino_covers(*shape) == 1 and cov(*shape) == 1, shape
    for shape in ((64, 512, 512, 32, 32), (3, 16, 128, 24, 32), (1, 8, 64, 16, 16), (3, 16, 128, 48, 16)):
        assert lib.nhmc_conv3x3_wino_narrow_covers(*shape) == 1 and cov(*shape) == 1, shape
    assert cov(1, 8, 48, 4, 64) == 0 and cov(64, 128, 6, 256, 256) == 0          # K % 32
    assert cov(1, 12, 32, 4, 64) == 0 and cov(1, 4, 32, 4, 64) == 0              # C % 8, C < 8
    assert cov(16, 896, 896, 8, 8) == 0 and cov(16, 672, 896, 8, 8) == 0         # 8 x 8 images
    assert cov(1, 8, 32, 4, 96) == 0 and cov(0, 8, 32, 4, 64) == 0               # W = 96, n = 0
    assert cov(1, 8, 32, 6, 64) == 0 and cov(1, 8, 32, 4, 32) == 0 and cov(1, 8, 32, 12, 32) == 0     # H % 4, H % 8 at W = 32
    assert cov(1, 8, 32, 8, 16) == 0 and cov(1, 8, 32, 24, 16) == 0              # H % 16 at W = 16
    # the existing queries keep their answers
    assert lib.nhmc_conv3x3_wino_covers(16, 224, 224, 64, 64) == 0 and lib.nhmc_conv3x3_wino_narrow_covers(16, 672, 672, 32, 32) == 0


def test_k32_routing_lists_tail_shapes_only(lib):
    pre = lib.nhmc_conv3x3_wino_k32_prefers
    for backward in (0, 1):
        for c, k, res in ((128, 128, 256), (256, 256, 64), (512, 512, 32), (448, 448, 64), (896, 448, 32), (896, 896, 16)):
            assert pre(backward, 16, c, k, res, res) == 0 and pre(backward, 64, c, k, res, res) == 0      # K % 64 == 0
        assert pre(backward, 16, 8, 96, 64, 64) == 0 and pre(backward, 16, 8, 32, 32, 32) == 0            # covered, not measured
        assert pre(backward, 16, 224, 48, 64, 64) == 0 and pre(backward, 16, 896, 672, 8, 8) == 0         # not covered
        assert pre(backward, 16, 224, 224, 4, 64) == 0                                                    # H != W


def test_latent_rows_of_the_routing_tables(lib):
    """Every covered shape of the latent networks measured at or below 0.90 (profiles/r08_wino_conv_latent.txt) and is listed
    in exactly one table: the score network's forward only, the decoder's in both directions."""
    import nhmc.kernels as K
    from nhmc import ldm
    for c, k, res, _ in ldm.conv3x3_shapes('unet'):
        if not K.conv3x3_wino_k32_covers(16, c, k, res, res):
            assert res == 8 or 3 in (c, k)
            continue
        tail = lib.nhmc_conv3x3_wino_k32_prefers(0, 16, c, k, res, res)
        assert tail == (1 if k % 64 else 0)
        assert tail + int(K.conv3x3_wino_prefers(0, 16, c, k, res, res)) == 1
        assert lib.nhmc_conv3x3_wino_k32_prefers(1, 16, k, c, res, res) == 0
    for c, k, res, _ in ldm.conv3x3_shapes('decoder'):
        if 3 not in (c, k):
            assert K.conv3x3_wino_prefers(0, 16, c, k, res, res) and K.conv3x3_wino_prefers(1, 16, k, c, res, res)
    from nhmc import unet
    ffhq = {s[:3] for s in unet.conv3x3_shapes()}                                # the new K % 64 == 0 rows leave FFHQ routing alone
    new = {(448, 448, 64), (256, 256, 256), (512, 512, 128), (224, 448, 32), (448, 448, 32), (672, 448, 32), (896, 448, 32),
           (1120, 448, 32), (896, 896, 16)}
    assert not (new & ffhq)


P = ctypes.c_void_p
null, a16, b16, c16, d16, a4 = P(0), P(0x1000), P(0x2000), P(0x3000), P(0x4000), P(0x1004)
OK = ((1, 8, 32, 4, 64), (1, 8, 96, 8, 32), (1, 8, 32, 16, 16), (1, 8, 64, 4, 64))      # n, c, k, h, w: one per geometry, and K % 64 == 0


def conv(lib, x=a16, u=b16, bias=null, add=null, y=c16, shape=OK[0], stride=1, padding=1):
    return lib.nhmc_conv3x3_wino_k32(x, u, bias, add, y, *shape, stride, padding, null)


def test_k32_argument_validation_happens_before_any_launch(lib):
    for ok in OK:
        assert conv(lib, x=null, shape=ok) == 1 and conv(lib, u=null, shape=ok) == 1 and conv(lib, y=null, shape=ok) == 1    # ARG
        assert conv(lib, y=a16, shape=ok) == 1 and conv(lib, add=a16, shape=ok) == 1                       # aliases x
        assert conv(lib, stride=2, shape=ok) == 3 and conv(lib, stride=0, shape=ok) == 3 and conv(lib, padding=0, shape=ok) == 3
        assert conv(lib, x=a4, shape=ok) == 2 and conv(lib, u=a4, shape=ok) == 2 and conv(lib, y=a4, shape=ok) == 2   # ALIGN
        assert conv(lib, add=a4, shape=ok) == 2
    assert conv(lib, shape=(1, 8, 48, 4, 64)) == 3 and conv(lib, shape=(1, 8, 16, 4, 64)) == 3            # K
    assert conv(lib, shape=(1, 12, 32, 4, 64)) == 3 and conv(lib, shape=(1, 4, 32, 4, 64)) == 3           # C
    assert conv(lib, shape=(1, 8, 32, 8, 8)) == 3 and conv(lib, shape=(16, 896, 896, 8, 8)) == 3          # 8 x 8
    assert conv(lib, shape=(1, 8, 32, 4, 96)) == 3 and conv(lib, shape=(0, 8, 32, 4, 64)) == 3
    assert conv(lib, shape=(1, 8, 32, 4, 32)) == 3 and conv(lib, shape=(1, 8, 32, 8, 16)) == 3            # H at W = 32, 16
    # ARG before SHAPE before ALIGN
    assert conv(lib, x=null, stride=2, add=a4) == 1 and conv(lib, stride=2, add=a4) == 3 and conv(lib, add=a4) == 2
    assert conv(lib, y=a16, shape=(1, 8, 48, 4, 64), u=a4) == 1 and conv(lib, shape=(1, 8, 48, 4, 64), u=a4) == 3


def test_python_front_end_keeps_the_existing_answers():
    import nhmc.kernels as K
    from nhmc._lib import NhmcError
    assert K.conv3x3_wino_k32_covers(16, 224, 224, 64, 64) and K.conv3x3_wino_k32_covers(16, 672, 672, 32, 32)
    assert K.conv3x3_wino_k32_covers(64, 256, 256, 64, 64) and not K.conv3x3_wino_k32_covers(16, 896, 896, 8, 8)
    assert not K.conv3x3_wino_covers(64, 224, 224, 32, 32) and not K.conv3x3_wino_covers(16, 224, 224, 64, 64)
    assert not K.conv3x3_wino_k32_prefers(0, 16, 448, 448, 64, 64) and not K.conv3x3_wino_k32_prefers(1, 16, 8, 96, 64, 64)
    with pytest.raises(NhmcError, match='no CPU path'):
        K.conv3x3_wino(torch.zeros(1, 8, 4, 64), torch.zeros(32, 8, 3, 3))


def test_conv_bench_takes_its_latent_shapes_from_the_models():
    import nhmc.kernels as K
    from nhmc import ldm
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'conv_bench.py')
    spec = importlib.util.spec_from_file_location('conv_bench_latent_under_test', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                                                 # importing it launches nothing
    cov = K.conv3x3_wino_k32_covers
    want = [(c, k, res, (False,)) for c, k, res, _ in ldm.conv3x3_shapes('unet') if cov(16, c, k, res, res)]
    want += [(c, k, res, (False, True)) for c, k, res, _ in ldm.conv3x3_shapes('decoder')
             if cov(16, c, k, res, res) and cov(16, k, c, res, res)]
    got = mod.latent_shapes(16)
    assert list(got) == want
    assert {s[:3] for s in got} == {s for s in list(UNET) + list(DECODER) if s[2] >= 16 and min(s[0], s[1]) >= 32}
    assert len(got) == 23
    assert len(mod.default_shapes(64)) == 20


def test_latent_blocks_on_cpu_tensors_compute_what_they_did():
    """CPU tensors take no kernel: the blocks are the plain expressions, bit for bit, whatever `wino` says."""
    from nhmc import ldm, unet
    torch.manual_seed(11)
    x = torch.randn(2, 32, 8, 8)
    for cls in (ldm.ConvUp, ldm.UpConv):
        up = cls(32).eval().requires_grad_(False)
        assert cls.wino is None
        want = F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), up.conv.weight, up.conv.bias, 1, 1)
        for wino in (None, True, False):
            up.wino = wino
            assert torch.equal(up(x), want)
    conv = torch.nn.Conv2d(32, 64, 3, padding=1).requires_grad_(False)
    assert unet.wino_route(conv, x, True) is None
    assert torch.equal(unet.conv_bias(conv, x, True), F.conv2d(x, conv.weight, conv.bias, 1, 1))

    emb = torch.randn(2, 48)
    blk = ldm.AddEmbResBlock(32, 48, 64).eval().requires_grad_(False)
    assert ldm.AddEmbResBlock.wino is None and ldm.PlainResBlock.wino is None
    c1, c2 = blk.in_layers[2], blk.out_layers[3]
    h = c1(F.silu(F.group_norm(x, 32, blk.in_layers[0].weight, blk.in_layers[0].bias, blk.in_layers[0].eps)))
    h = h + blk.emb_layers(emb)[:, :, None, None]
    h = c2(F.silu(F.group_norm(h, 32, blk.out_layers[0].weight, blk.out_layers[0].bias, blk.out_layers[0].eps)))
    want = blk.skip_connection(x) + h
    for wino in (None, True):
        blk.wino = wino
        assert torch.equal(blk(x, emb), want)

    pb = ldm.PlainResBlock(32, 64).eval().requires_grad_(False)
    sw = lambda t: t * torch.sigmoid(t)
    h = pb.conv1(sw(F.group_norm(x, 32, pb.norm1.weight, pb.norm1.bias, pb.norm1.eps)))
    h = pb.conv2(sw(F.group_norm(h, 32, pb.norm2.weight, pb.norm2.bias, pb.norm2.eps)))
    pb.wino = True
    assert torch.equal(pb(x), pb.nin_shortcut(x) + h)
