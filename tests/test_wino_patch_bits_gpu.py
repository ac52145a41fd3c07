"""GPU: the Winograd convolution (csrc/wino_conv.hip) with its patch loaded as one 8-byte load per row and the outer columns
taken from the neighbouring lanes produces the bits recorded in tests/golden/wino_patch_bits.npz, which the build that loaded
all four columns itself wrote (tools/gen_wino_patch_bits.py).  A value that moved between lanes is the value the lane
would have loaded, so every output bit is what it was.

Cases (n, c, k, h, w), the smallest at which the exchange can go wrong and that tests/test_wino_bits_gpu.py lacks: three
column blocks (the middle block's edge lanes take real columns of both neighbouring blocks, the outer blocks' one real
column and the padding), two column blocks over two row blocks, the 32- and 16-wide geometries (two and four tile rows share
a lane group: the lane next to a tile row's end belongs to another row), K % 64 == 32 narrow and wide.  Each runs forward and
backward-data, plain and with bias + add, into an output with 4096 sentinel floats on either side.

The integer cases need no fixture: x a small integer that differs between neighbouring columns and single-tap filters make
every intermediate exact, so the output is the shifted, zero-padded input with zero tolerance, and a lane that took the
wrong neighbour shows as a wrong integer.  Their expectation is checked against F.conv2d in float64 on the CPU first."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('gen_wino_patch_bits', os.path.join(ROOT, 'tools', 'gen_wino_patch_bits.py'))
P = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(P)
G = P.G

ids = lambda s: 'x'.join(map(str, s))


@pytest.fixture(scope='module')
def bits():
    with np.load(P.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def guards_untouched(key, y, whole):
    guard = whole.cpu().numpy()
    assert (guard[:G.GUARD] == G.SENTINEL).all(), f'{key}: a write in front of the output'
    assert (guard[G.GUARD + y.numel():] == G.SENTINEL).all(), f'{key}: a write past the output'


@pytest.mark.gpu
@pytest.mark.parametrize('fused', [0, 1], ids=['plain', 'bias_add'])
@pytest.mark.parametrize('backward', [0, 1], ids=['forward', 'backward_data'])
@pytest.mark.parametrize('shape', P.CASES, ids=ids)
def test_bits_are_the_recorded_ones(bits, shape, backward, fused):
    y, whole = G.run(shape, backward, fused)
    key = G.name(shape, backward, fused)
    guards_untouched(key, y, whole)
    assert np.array_equal(G.checksums(y), bits['sum_' + key]), f'{key}: checksums differ from the recorded bits'
    if 'raw_' + key in bits:
        assert torch.equal(y.cpu().view(torch.int32), torch.from_numpy(bits['raw_' + key])), f'{key}: bits differ'


def test_fixture_holds_every_case(bits):
    for shape in P.CASES:
        for backward in (0, 1):
            for fused in (0, 1):
                assert 'sum_' + G.name(shape, backward, fused) in bits
    for shape in P.RAW:
        assert 'raw_' + G.name(shape, 0, 0) in bits
    assert os.path.getsize(P.GOLDEN) < 1 << 20


@pytest.mark.parametrize('backward', [0, 1], ids=['forward', 'backward_data'])
@pytest.mark.parametrize('shape', P.INTEGER, ids=ids)
def test_integer_expectation_is_what_float64_convolution_gives(shape, backward):
    xh, wh, yh = P.integer_case(shape, backward)
    assert np.abs(xh).max() <= 64 and (xh == np.round(xh)).all()
    assert (xh[..., 1:] != xh[..., :-1]).all(), 'neighbouring columns differ'
    assert (wh.reshape(-1, 9).sum(0) > 0).all(), 'every one of the nine taps is used'
    x, wt = torch.from_numpy(xh).double(), torch.from_numpy(wh).double()
    ref = torch.nn.grad.conv2d_input((shape[0], shape[2], shape[3], shape[4]), wt, x, 1, 1) if backward else F.conv2d(x, wt, None, 1, 1)
    assert torch.equal(ref, torch.from_numpy(yh).double())


@pytest.mark.gpu
@pytest.mark.parametrize('backward', [0, 1], ids=['forward', 'backward_data'])
@pytest.mark.parametrize('shape', P.INTEGER, ids=ids)
def test_integer_input_and_single_tap_filters_give_the_shifted_input_exactly(shape, backward):
    xh, wh, yh = P.integer_case(shape, backward)
    y, whole = P.run_arrays(shape, backward, xh, wh)
    guards_untouched(G.name(shape, backward, 0), y, whole)
    got = y.cpu().numpy()
    wrong = np.argwhere(got != yh)
    assert wrong.size == 0, f'{len(wrong)} outputs differ, the first at (n, k, h, w) = {tuple(wrong[0])}: {got[tuple(wrong[0])]} for {yh[tuple(wrong[0])]}'
