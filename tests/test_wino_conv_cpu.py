"""CPU: the Winograd convolution entries (csrc/wino_conv.hip) validate their arguments before any device work and answer
the host-only coverage and routing queries, in the style of tests/test_gn_onepass_cpu.py."""
import ctypes

import pytest


@pytest.fixture(scope='module')
def lib():
    import nhmc
    return nhmc._lib.load()


P = ctypes.c_void_p
null, a16, b16, c16, d16, a4 = P(0), P(0x1000), P(0x2000), P(0x3000), P(0x4000), P(0x1004)
OK_SHAPE = (1, 8, 64, 4, 64)                 # n, c, k, h, w


def conv(lib, x=a16, u=b16, bias=null, add=null, y=c16, shape=OK_SHAPE, stride=1, padding=1):
    return lib.nhmc_conv3x3_wino(x, u, bias, add, y, *shape, stride, padding, null)


def test_coverage_and_routing_queries_are_host_only(lib):
    cov, pre = lib.nhmc_conv3x3_wino_covers, lib.nhmc_conv3x3_wino_prefers
    for c, k, res in ((128, 128, 256), (256, 128, 256), (256, 256, 128), (384, 128, 256), (128, 256, 128), (384, 256, 128),
                      (512, 256, 128), (256, 256, 64), (512, 512, 64), (768, 256, 64), (8, 64, 64)):
        assert cov(64, c, k, res, res) == 1
    assert cov(3, 16, 64, 12, 192) == 1                                          # H != W, any N
    assert cov(64, 4, 64, 64, 64) == 0 and cov(64, 12, 64, 64, 64) == 0          # C < 8, C % 8
    assert cov(64, 128, 6, 256, 256) == 0 and cov(64, 128, 96, 64, 64) == 0      # K % 64
    assert cov(64, 128, 128, 6, 64) == 0 and cov(64, 128, 128, 64, 96) == 0      # H % 4, W % 64
    assert cov(64, 3, 128, 256, 256) == 0 and cov(0, 128, 128, 64, 64) == 0
    assert cov(64, 224, 224, 64, 64) == 0 and cov(64, 448, 224, 64, 64) == 0     # the latent network's 224 channels
    assert cov(64, 512, 512, 32, 32) == 0 and cov(64, 448, 448, 32, 32) == 0     # 32 x 32 and below
    for backward in (0, 1):
        assert pre(backward, 64, 224, 224, 64, 64) == 0 and pre(backward, 64, 512, 512, 32, 32) == 0
        assert pre(backward, 64, 3, 128, 256, 256) == 0 and pre(backward, 64, 128, 6, 256, 256) == 0
        assert pre(backward, 64, 12, 64, 64, 64) == 0 and pre(backward, 64, 8, 64, 64, 64) == 0     # covered, not measured


def test_convolution_argument_validation_happens_before_any_launch(lib):
    assert conv(lib, x=null) == 1 and conv(lib, u=null) == 1 and conv(lib, y=null) == 1               # ARG
    assert conv(lib, y=a16) == 1 and conv(lib, add=a16) == 1                                          # aliases x
    assert conv(lib, stride=2) == 3 and conv(lib, stride=0) == 3 and conv(lib, padding=0) == 3        # SHAPE
    assert conv(lib, shape=(1, 12, 64, 4, 64)) == 3 and conv(lib, shape=(1, 4, 64, 4, 64)) == 3       # C
    assert conv(lib, shape=(1, 8, 32, 4, 64)) == 3 and conv(lib, shape=(1, 8, 96, 4, 64)) == 3        # K
    assert conv(lib, shape=(1, 8, 64, 6, 64)) == 3 and conv(lib, shape=(1, 8, 64, 4, 32)) == 3        # H, W
    assert conv(lib, shape=(1, 224, 224, 64, 64)) == 3 and conv(lib, shape=(0, 8, 64, 4, 64)) == 3
    assert conv(lib, x=a4) == 2 and conv(lib, u=a4) == 2 and conv(lib, y=a4) == 2 and conv(lib, add=a4) == 2   # ALIGN


def test_weight_transform_argument_validation(lib):
    w = lib.nhmc_wino_weights
    assert w(null, a16, 0, 8, 64, null) == 1 and w(a16, null, 0, 8, 64, null) == 1
    assert w(a16, b16, 2, 8, 64, null) == 1 and w(a16, b16, 0, 0, 64, null) == 1 and w(a16, b16, 1, 8, -1, null) == 1
    assert w(a16, b16, 0, 1 << 20, 64, null) == 3 and w(a16, a4, 0, 8, 64, null) == 2


def test_python_front_end_refuses_what_it_cannot_run():
    import torch
    import nhmc.kernels as K
    from nhmc import unet
    from nhmc._lib import NhmcError
    x, w = torch.zeros(1, 8, 4, 64), torch.zeros(64, 8, 3, 3)
    with pytest.raises(NhmcError, match='no CPU path'):
        K.conv3x3_wino(x, w)
    with pytest.raises(NhmcError, match='does not match'):
        K.conv3x3_wino(torch.zeros(1, 16, 4, 64), w)
    conv = torch.nn.Conv2d(8, 64, 3, padding=1)
    assert unet.wino_route(conv, x, True) is None                                 # CPU tensors keep F.conv2d
    assert torch.equal(unet.conv_nobias(conv, x, True), torch.nn.functional.conv2d(x, conv.weight, None, 1, 1))
