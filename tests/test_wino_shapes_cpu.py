"""CPU: the shape list behind the Winograd routing table comes from the model (unet.conv3x3_shapes), tools/conv_bench.py
takes its default shapes from it, and the entries of the kernel's narrow geometries (images 32 and 16 wide:
nhmc_conv3x3_wino_narrow*) validate their arguments before any device work, in the order of the wide entry, in the style
of tests/test_wino_conv_cpu.py."""
import ctypes
import importlib.util
import os

import pytest

# (C, K, resolution): count -- every 3x3 stride-1 padding-1 Conv2d call of one forward pass of create_model(**FFHQ_CONFIG)
NETWORK = {
    (128, 128, 256): 6, (256, 128, 256): 2, (3, 128, 256): 1, (128, 6, 256): 1,
    (128, 128, 128): 6, (256, 256, 128): 2, (384, 128, 128): 1, (256, 128, 128): 1,
    (256, 256, 64): 5, (512, 256, 64): 1, (384, 256, 64): 1, (128, 128, 64): 2, (128, 256, 64): 1,
    (256, 256, 32): 6, (512, 512, 32): 2, (768, 256, 32): 1, (512, 256, 32): 1,
    (512, 512, 16): 5, (1024, 512, 16): 1, (768, 512, 16): 1, (256, 256, 16): 2, (256, 512, 16): 1,
    (512, 512, 8): 10, (1024, 512, 8): 2,
}


@pytest.fixture(scope='module')
def lib():
    import nhmc
    return nhmc._lib.load()


def test_shape_list_is_the_networks():
    from nhmc import unet
    got = unet.conv3x3_shapes()
    assert len(got) == len(NETWORK)                                              # no shape twice
    assert {(c, k, res): n for c, k, res, n in got} == NETWORK
    assert unet.conv3x3_shapes(unet.FFHQ_CONFIG) == got
    assert [s[2] for s in got] == sorted((s[2] for s in got), reverse=True)


def test_conv_bench_takes_its_default_shapes_from_the_model():
    import nhmc.kernels as K
    from nhmc import unet
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'conv_bench.py')
    spec = importlib.util.spec_from_file_location('conv_bench_under_test', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                                                 # importing it launches nothing
    shapes = mod.default_shapes(64)
    assert list(shapes) == [(c, k, res) for c, k, res, _ in unet.conv3x3_shapes()
                            if K.conv3x3_wino_covers(64, c, k, res, res) and K.conv3x3_wino_covers(64, k, c, res, res)]
    assert set(shapes) == {s for s in NETWORK if s[2] >= 16 and min(s[0], s[1]) >= 64}
    assert len(shapes) == 20


P = ctypes.c_void_p
null, a16, b16, c16, d16, a4 = P(0), P(0x1000), P(0x2000), P(0x3000), P(0x4000), P(0x1004)
OK32, OK16 = (1, 8, 64, 8, 32), (1, 8, 64, 16, 16)                               # n, c, k, h, w


def conv(lib, x=a16, u=b16, bias=null, add=null, y=c16, shape=OK32, stride=1, padding=1):
    return lib.nhmc_conv3x3_wino_narrow(x, u, bias, add, y, *shape, stride, padding, null)


def test_narrow_coverage_and_routing_queries(lib):
    cov, pre = lib.nhmc_conv3x3_wino_narrow_covers, lib.nhmc_conv3x3_wino_narrow_prefers
    for c, k, res in [s for s in NETWORK if s[2] in (32, 16)]:
        assert cov(64, c, k, res, res) == 1 and cov(64, k, c, res, res) == 1
    assert cov(*OK32) == 1 and cov(*OK16) == 1 and cov(3, 16, 128, 24, 32) == 1 and cov(3, 16, 128, 48, 16) == 1   # H != W
    assert cov(64, 512, 512, 64, 64) == 0 and cov(64, 512, 512, 8, 8) == 0       # W = 64 is the wide entry's, W = 8 nobody's
    assert cov(64, 512, 512, 16, 8) == 0 and cov(64, 512, 512, 128, 128) == 0 and cov(64, 512, 512, 48, 48) == 0
    assert cov(64, 224, 224, 32, 32) == 0 and cov(64, 448, 224, 16, 16) == 0     # the latent network's 224 channels
    assert cov(64, 4, 64, 32, 32) == 0 and cov(64, 12, 64, 32, 32) == 0          # C < 8, C % 8
    assert cov(64, 128, 6, 32, 32) == 0 and cov(64, 128, 96, 16, 16) == 0        # K % 64
    assert cov(1, 8, 64, 4, 32) == 0 and cov(1, 8, 64, 12, 32) == 0              # H % 8 at W = 32
    assert cov(1, 8, 64, 8, 16) == 0 and cov(1, 8, 64, 24, 16) == 0              # H % 16 at W = 16
    assert cov(0, 8, 64, 8, 32) == 0
    for backward in (0, 1):
        assert pre(backward, 64, 512, 512, 64, 64) == 0 and pre(backward, 64, 512, 512, 8, 8) == 0
        assert pre(backward, 64, 224, 224, 32, 32) == 0 and pre(backward, 64, 8, 64, 32, 32) == 0   # covered, not measured
        assert pre(backward, 64, 12, 64, 16, 16) == 0
    # the wide entries keep their answers: nothing 32 or 16 wide
    assert lib.nhmc_conv3x3_wino_covers(64, 512, 512, 32, 32) == 0 and lib.nhmc_conv3x3_wino_covers(1, 8, 64, 16, 16) == 0
    assert lib.nhmc_conv3x3_wino(a16, b16, null, null, c16, *OK32, 1, 1, null) == 3


def test_narrow_argument_validation_happens_before_any_launch(lib):
    for ok in (OK32, OK16):
        assert conv(lib, x=null, shape=ok) == 1 and conv(lib, u=null, shape=ok) == 1 and conv(lib, y=null, shape=ok) == 1    # ARG
        assert conv(lib, y=a16, shape=ok) == 1 and conv(lib, add=a16, shape=ok) == 1                       # aliases x
        assert conv(lib, stride=2, shape=ok) == 3 and conv(lib, stride=0, shape=ok) == 3 and conv(lib, padding=0, shape=ok) == 3
        assert conv(lib, x=a4, shape=ok) == 2 and conv(lib, u=a4, shape=ok) == 2 and conv(lib, y=a4, shape=ok) == 2   # ALIGN
        assert conv(lib, add=a4, shape=ok) == 2
    assert conv(lib, x=null, stride=2, add=a4) == 1 and conv(lib, stride=2, add=a4) == 3                  # ARG, SHAPE, ALIGN
    assert conv(lib, shape=(1, 12, 64, 8, 32)) == 3 and conv(lib, shape=(1, 4, 64, 16, 16)) == 3          # C
    assert conv(lib, shape=(1, 8, 32, 8, 32)) == 3 and conv(lib, shape=(1, 8, 96, 16, 16)) == 3           # K
    assert conv(lib, shape=(1, 8, 64, 4, 32)) == 3 and conv(lib, shape=(1, 8, 64, 12, 32)) == 3           # H % 8 at W = 32
    assert conv(lib, shape=(1, 8, 64, 8, 16)) == 3 and conv(lib, shape=(1, 8, 64, 24, 16)) == 3           # H % 16 at W = 16
    assert conv(lib, shape=(1, 8, 64, 4, 64)) == 3 and conv(lib, shape=(1, 8, 64, 16, 8)) == 3            # W = 64, W = 8
    assert conv(lib, shape=(1, 224, 224, 32, 32)) == 3 and conv(lib, shape=(0, 8, 64, 8, 32)) == 3


def test_python_front_end_chooses_the_entry_by_width(monkeypatch):
    import torch
    import nhmc.kernels as K
    from nhmc._lib import NhmcError
    assert K.conv3x3_wino_covers(64, 512, 512, 32, 32) and K.conv3x3_wino_covers(64, 256, 512, 16, 16)
    assert K.conv3x3_wino_covers(64, 256, 256, 64, 64) and not K.conv3x3_wino_covers(64, 512, 512, 8, 8)
    assert not K.conv3x3_wino_covers(64, 224, 224, 32, 32) and not K.conv3x3_wino_covers(1, 8, 64, 8, 16)
    monkeypatch.setenv('NHMC_WINO', '0')
    assert not K.conv3x3_wino_prefers(0, 64, 256, 256, 32, 32) and not K.conv3x3_wino_prefers(0, 64, 128, 128, 256, 256)
    with pytest.raises(NhmcError, match='no CPU path'):
        K.conv3x3_wino(torch.zeros(1, 8, 8, 32), torch.zeros(64, 8, 3, 3))
