"""CPU: the one-pass GroupNorm entries (csrc/gn_onepass.hip) validate their arguments before any device work and answer
the host-only coverage query, in the style of tests/test_abi_cpu.py."""
import ctypes

import pytest


@pytest.fixture(scope='module')
def lib():
    import nhmc
    return nhmc._lib.load()


P = ctypes.c_void_p
null, a16, b16, c16, d16, a4 = P(0), P(0x1000), P(0x2000), P(0x3000), P(0x4000), P(0x1004)
OK_SHAPE = (1, 64, 32, 64)                  # n, channels, groups, hw


def fwd(lib, x1=a16, x2=null, c1=64, gamma=a16, beta=a16, y=b16, x_cat=null, ws=c16, flags=0, shape=OK_SHAPE):
    return lib.nhmc_gn_onepass_fwd(x1, x2, c1, gamma, beta, null, 0, null, 0, 1e-5, 1, y, x_cat, ws, flags, *shape, null)


def bwd(lib, x=a16, dy=a16, fwd_ws=c16, fwd_splits=1, dx_add=null, dx1=b16, dx2=null, c1=64, ws=d16, flags=0, shape=OK_SHAPE):
    return lib.nhmc_gn_onepass_bwd(x, dy, a16, a16, null, 0, null, 0, 1e-5, 1, fwd_ws, fwd_splits, dx_add, dx1, dx2, c1, ws,
                                   flags, *shape, null)


def test_coverage_query_is_host_only(lib):
    """splits = ceil(channels / groups * hw / 4 / (256 * 8)); 0 = not covered (the caller keeps the two-pass entries)."""
    q = lib.nhmc_gn_onepass_splits
    assert q(64, 128, 32, 65536) == 32 and q(64, 256, 32, 65536) == 64          # the 256x256 level, 128 and 256 channels
    assert q(64, 384, 32, 16384) == 24 and q(64, 256, 32, 16384) == 16 and q(64, 128, 32, 16384) == 8
    assert q(64, 1024, 32, 256) == 1 and q(64, 512, 32, 64) == 1                 # 16x16 / 8x8: one workgroup per slab
    assert q(2, 64, 32, 64) == 1
    assert q(64, 384, 32, 65536) == 0                                            # 96 splits > 64
    assert q(2, 48, 32, 64) == 0 and q(2, 64, 32, 9) == 0 and q(4096, 64, 32, 64) == 0 and q(0, 64, 32, 64) == 0


def test_forward_argument_validation_happens_before_any_launch(lib):
    assert fwd(lib, x1=null) == 1 and fwd(lib, gamma=null) == 1 and fwd(lib, y=null) == 1 and fwd(lib, ws=null) == 1   # ARG
    assert fwd(lib, flags=2) == 1                                                        # unknown flag
    assert fwd(lib, x1=a4) == 2 and fwd(lib, y=a4) == 2                                  # ALIGN
    assert fwd(lib, shape=(1, 64, 32, 9)) == 3 and fwd(lib, shape=(1, 48, 32, 64), c1=48) == 3      # hw % 4, C % G
    assert fwd(lib, shape=(1, 384, 32, 65536), c1=384) == 3                              # 96 splits: not covered
    assert fwd(lib, ws=a4) == 2                                                          # the workspace is filled and polled in 16-byte slots
    assert fwd(lib, y=a16) == 1                                                          # y aliases x
    # two sources
    assert fwd(lib, x2=d16, c1=32, x_cat=null) == 1                                      # a second source without an x_cat destination
    assert fwd(lib, x2=null, x_cat=d16) == 1                                             # x_cat without a second source
    assert fwd(lib, x2=d16, c1=0, x_cat=P(0x5000)) == 3 and fwd(lib, x2=d16, c1=64, x_cat=P(0x5000)) == 3   # C1 <= 0, C1 >= C
    assert fwd(lib, x2=null, c1=32) == 3                                                 # one source: c1 == channels
    assert fwd(lib, x2=a4, c1=32, x_cat=P(0x5000)) == 2 and fwd(lib, x2=d16, c1=32, x_cat=a4) == 2
    assert fwd(lib, x2=d16, c1=32, x_cat=d16) == 1                                       # x_cat aliases a source


def test_backward_argument_validation_happens_before_any_launch(lib):
    assert bwd(lib, x=null) == 1 and bwd(lib, dy=null) == 1 and bwd(lib, fwd_ws=null) == 1 and bwd(lib, dx1=null) == 1
    assert bwd(lib, ws=null) == 1 and bwd(lib, fwd_splits=0) == 1 and bwd(lib, fwd_splits=65) == 1 and bwd(lib, flags=4) == 1
    assert bwd(lib, dx_add=b16) == 1                                                     # dx1 == dx_add
    assert bwd(lib, dx_add=P(0x5000), dx2=P(0x5000), c1=32) == 1                         # dx2 == dx_add
    assert bwd(lib, dx2=b16, c1=32) == 1                                                 # dx2 == dx1
    assert bwd(lib, fwd_ws=d16) == 1                                                     # the forward's workspace is an input
    assert bwd(lib, dy=a4) == 2 and bwd(lib, dx1=a4) == 2 and bwd(lib, dx_add=a4) == 2 and bwd(lib, dx2=a4, c1=32) == 2
    assert bwd(lib, dx2=P(0x5000), c1=0) == 3 and bwd(lib, dx2=P(0x5000), c1=64) == 3    # C1 <= 0, C1 >= C
    assert bwd(lib, dx2=null, c1=32) == 3
    assert bwd(lib, shape=(1, 64, 32, 9)) == 3 and bwd(lib, shape=(1, 384, 32, 65536), c1=384) == 3
    assert bwd(lib, ws=a4) == 2
    assert bwd(lib, dx1=a16) == 1 and bwd(lib, dx2=a16, c1=32) == 1                      # not in place: dx aliases x / dy
    P5 = P(0x5000)
    assert lib.nhmc_gn_act_bwd_fs(a16, a16, a16, a16, null, 0, null, 0, 1e-5, 1, c16, 0, null, b16, d16, 1, *OK_SHAPE, null) == 1
    assert lib.nhmc_gn_act_bwd_fs(a16, a16, a16, a16, null, 0, null, 0, 1e-5, 1, c16, 65, null, b16, d16, 1, *OK_SHAPE, null) == 1
    assert lib.nhmc_gn_act_bwd_fs(a16, a16, a16, a16, null, 0, null, 0, 1e-5, 1, c16, 4, P5, P5, d16, 1, *OK_SHAPE, null) == 1


def test_python_front_end_refuses_what_it_cannot_run():
    import torch
    import nhmc.kernels as K
    from nhmc._lib import NhmcError
    x = torch.zeros(1, 64, 8, 8)
    with pytest.raises(NhmcError, match='no CPU path'):
        K.gn_act_fwd(x, torch.ones(64), torch.zeros(64), 32, 1e-5, True)
    with pytest.raises(NhmcError, match='batch and spatial'):
        K.gn_act_fwd(x, torch.ones(96), torch.zeros(96), 32, 1e-5, True, x2=torch.zeros(1, 32, 4, 4))
