"""GPU: the Winograd convolution (csrc/wino_conv.hip) produces the bits recorded in tests/golden/wino_parent_bits.npz
(tools/gen_wino_bits.py, written by the build before the chunk's loads were spread over the MFMA gaps and the epilogue went
to 16-byte stores).  The products, their order and the transforms' parenthesisation are what they were, so every output
bit is.

Cases (n, c, k, h, w), the smallest at which the changed parts can go wrong: 1, 2, 3 and 5 chunks (the clamp of the chunk
being loaded and both buffer parities, with loads that straddle the loop edge); two K blocks x two column blocks; workgroup
totals that are and are not multiples of 8 (the XCD remap); the 32- and 16-wide geometries; K % 64 == 32 in all three
geometries.  Each runs forward and backward-data, plain and with bias + add.  Every launch writes into an output with 4096
sentinel floats on either side, which must come back untouched; the edge test puts x at the very start and the very end of
a sentinel-filled allocation (NaNs), so a patch load that took a value from outside x would change the output."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('gen_wino_bits', os.path.join(ROOT, 'tools', 'gen_wino_bits.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

ids = lambda s: 'x'.join(map(str, s))


@pytest.fixture(scope='module')
def bits():
    with np.load(G.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def check(bits, shape, backward, fused, y, whole):
    key = G.name(shape, backward, fused)
    guard = whole.cpu().numpy()
    n_out = y.numel()
    assert (guard[:G.GUARD] == G.SENTINEL).all(), f'{key}: a write in front of the output'
    assert (guard[G.GUARD + n_out:] == G.SENTINEL).all(), f'{key}: a write past the output'
    assert np.array_equal(G.checksums(y), bits['sum_' + key]), f'{key}: checksums differ from the recorded bits'
    if "raw_" + key in bits:
        assert torch.equal(y.cpu().view(torch.int32), torch.from_numpy(bits['raw_' + key])), f'{key}: bits differ'


@pytest.mark.parametrize('fused', [0, 1], ids=['plain', 'bias_add'])
@pytest.mark.parametrize('backward', [0, 1], ids=['forward', 'backward_data'])
@pytest.mark.parametrize('shape', G.CASES, ids=ids)
def test_bits_are_the_recorded_ones(bits, shape, backward, fused):
    y, whole = G.run(shape, backward, fused)
    check(bits, shape, backward, fused, y, whole)


def test_fixture_holds_every_case(bits):
    for shape in G.CASES:
        for backward in (0, 1):
            for fused in (0, 1):
                assert 'sum_' + G.name(shape, backward, fused) in bits
    assert sum('raw_' in k for k in bits) >= 6
    assert os.path.getsize(G.GOLDEN) < 1 << 20


@pytest.mark.parametrize('where', ['start', 'end'])
@pytest.mark.parametrize('backward', [0, 1], ids=['forward', 'backward_data'])
@pytest.mark.parametrize('shape', [(1, 16, 64, 4, 64), (1, 16, 64, 8, 64)], ids=ids)
def test_image_edges_with_x_at_the_ends_of_its_allocation(bits, shape, backward, where):
    """x as a view at the very start / the very end of a larger buffer of NaN sentinels: the outputs are the recorded ones, so
    no value from outside x entered a patch (every output of the rows and columns at the border would be NaN)."""
    xh = G.inputs(shape, backward)[0]
    x, _ = G.guarded(xh, lead=0 if where == 'start' else G.GUARD, trail=G.GUARD if where == 'start' else 0)
    assert x.data_ptr() % 16 == 0
    for fused in (0, 1):
        y, whole = G.run(shape, backward, fused, x=x)
        check(bits, shape, backward, fused, y, whole)
