"""CPU: the thin-input convolution's entries (csrc/thin_conv.hip: nhmc_conv3x3_thin_in, nhmc_thin_in_weights) answer their
coverage and routing queries and refuse wrong arguments before any device work, with fake aligned and unaligned pointers in
the style of tests/test_wino_shapes_cpu.py: ARG = 1, ALIGN = 2, SHAPE = 3, in that order of precedence ARG, SHAPE, ALIGN."""
import ctypes

import pytest

P = ctypes.c_void_p
null, a16, b16, c16, d16, a4 = P(0), P(0x1000), P(0x2000), P(0x3000), P(0x4000), P(0x1004)
OK = (1, 3, 32, 8, 16)                                                            # n, c, k, h, w


@pytest.fixture(scope='module')
def lib():
    import nhmc
    return nhmc._lib.load()


def conv(lib, x=a16, wp=b16, bias=null, y=c16, shape=OK, stride=1, padding=1):
    return lib.nhmc_conv3x3_thin_in(x, wp, bias, y, *shape, stride, padding, null)


def test_abi_version_is_kept(lib):
    assert lib.nhmc_abi_version() == 2


def test_coverage_and_routing_queries(lib, monkeypatch):
    import nhmc.kernels as K
    cov, pre = lib.nhmc_conv3x3_thin_in_covers, lib.nhmc_conv3x3_thin_in_prefers
    assert cov(*OK) == 1 and cov(64, 3, 128, 256, 256) == 1 and cov(64, 6, 128, 256, 256) == 1
    assert cov(3, 8, 160, 40, 52) == 1 and cov(1, 1, 32, 1, 4) == 1              # H != W, K not a multiple of 64, one lane
    assert cov(64, 128, 3, 256, 256) == 0 and cov(64, 128, 6, 256, 256) == 0      # a thin OUTPUT is not this kernel's
    assert cov(1, 9, 32, 8, 16) == 0 and cov(1, 0, 32, 8, 16) == 0                # thin side > 8, no channel
    assert cov(1, 3, 48, 8, 16) == 0 and cov(1, 3, 16, 8, 16) == 0 and cov(1, 3, 0, 8, 16) == 0   # wide side % 32
    assert cov(1, 3, 32, 8, 18) == 0 and cov(1, 3, 32, 8, 2) == 0 and cov(1, 3, 32, 0, 16) == 0   # W % 4, W < 4, H = 0
    assert cov(0, 3, 32, 8, 16) == 0 and cov(-1, 3, 32, 8, 16) == 0
    assert cov(1, 3, 32, 8192, 4096) == 0 and cov(1, 3, 131072, 8, 16) == 0       # 32-bit offsets inside an image
    for backward in (0, 1):
        assert pre(backward, 64, 3, 32, 8, 16) == 0 and pre(backward, 64, 128, 3, 256, 256) == 0   # covered but not measured; not covered
    monkeypatch.setenv('NHMC_THIN_CONV', '0')
    assert not K.conv3x3_thin_in_prefers(0, 64, 3, 128, 256, 256) and not K.conv3x3_thin_in_prefers(1, 64, 6, 128, 256, 256)
    monkeypatch.delenv('NHMC_THIN_CONV')
    assert K.conv3x3_thin_in_prefers(0, 64, 3, 128, 256, 256) == bool(pre(0, 64, 3, 128, 256, 256))


def test_argument_validation_happens_before_any_launch(lib):
    assert conv(lib, x=null) == 1 and conv(lib, wp=null) == 1 and conv(lib, y=null) == 1          # ARG
    assert conv(lib, y=a16) == 1 and conv(lib, y=b16) == 1                                        # the output aliases an input
    assert conv(lib, stride=2) == 3 and conv(lib, stride=0) == 3 and conv(lib, padding=0) == 3 and conv(lib, padding=2) == 3
    assert conv(lib, shape=(1, 9, 32, 8, 16)) == 3 and conv(lib, shape=(1, 128, 32, 8, 16)) == 3  # thin side > 8
    assert conv(lib, shape=(1, 3, 48, 8, 16)) == 3 and conv(lib, shape=(1, 3, 6, 8, 16)) == 3     # wide side not a multiple of 32
    assert conv(lib, shape=(0, 3, 32, 8, 16)) == 3 and conv(lib, shape=(1, 3, 32, 8, 18)) == 3    # n = 0, W % 4
    assert conv(lib, x=a4) == 2 and conv(lib, wp=a4) == 2 and conv(lib, y=P(0x3004)) == 2         # ALIGN


def test_thin_output_entry_mirrors_it(lib):
    cov, pre = lib.nhmc_conv3x3_thin_out_covers, lib.nhmc_conv3x3_thin_out_prefers
    out = lambda x=a16, gp=b16, bias=null, y=c16, shape=(1, 32, 3, 8, 16), stride=1, padding=1: \
        lib.nhmc_conv3x3_thin_out(x, gp, bias, y, *shape, stride, padding, null)
    assert cov(64, 128, 6, 256, 256) == 1 and cov(64, 128, 3, 256, 256) == 1 and cov(3, 160, 5, 40, 52) == 1 and cov(1, 32, 1, 1, 4) == 1
    assert cov(64, 3, 128, 256, 256) == 0 and cov(1, 32, 9, 8, 16) == 0 and cov(1, 32, 0, 8, 16) == 0   # a thin INPUT, thin side > 8
    assert cov(1, 48, 3, 8, 16) == 0 and cov(1, 16, 3, 8, 16) == 0 and cov(0, 32, 3, 8, 16) == 0 and cov(1, 32, 3, 8, 18) == 0
    assert pre(0, 64, 32, 3, 8, 16) == 0 and pre(1, 64, 32, 3, 8, 16) == 0 and pre(0, 64, 3, 128, 256, 256) == 0
    assert out(x=null) == 1 and out(gp=null) == 1 and out(y=null) == 1 and out(y=a16) == 1 and out(y=b16) == 1
    assert out(stride=2) == 3 and out(padding=0) == 3 and out(shape=(1, 32, 9, 8, 16)) == 3 and out(shape=(1, 48, 3, 8, 16)) == 3
    assert out(shape=(0, 32, 3, 8, 16)) == 3 and out(shape=(1, 3, 32, 8, 16)) == 3
    assert out(x=a4) == 2 and out(gp=a4) == 2 and out(y=P(0x3004)) == 2
    assert out(x=null, stride=2, y=P(0x3004)) == 1 and out(stride=2, y=P(0x3004)) == 3
    wts = lambda w=a16, gp=b16, backward=0, thin=3, wide=32: lib.nhmc_thin_out_weights(w, gp, backward, thin, wide, null)
    assert wts(w=null) == 1 and wts(gp=null) == 1 and wts(gp=a16) == 1 and wts(backward=2) == 1
    assert wts(thin=9) == 3 and wts(thin=0) == 3 and wts(wide=48) == 3 and wts(gp=a4) == 2


def test_precedence_and_the_weights_entry(lib):
    assert conv(lib, x=null, stride=2, y=P(0x3004)) == 1 and conv(lib, stride=2, y=P(0x3004)) == 3   # ARG, SHAPE, ALIGN
    wts = lambda w=a16, wp=b16, backward=0, thin=3, wide=32: lib.nhmc_thin_in_weights(w, wp, backward, thin, wide, null)
    assert wts(w=null) == 1 and wts(wp=null) == 1 and wts(wp=a16) == 1 and wts(backward=2) == 1
    assert wts(thin=9) == 3 and wts(thin=0) == 3 and wts(wide=48) == 3 and wts(wide=0) == 3
    assert wts(wp=a4) == 2
