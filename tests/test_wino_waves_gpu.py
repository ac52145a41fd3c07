"""GPU: the Winograd convolution's two workgroup geometries (csrc/wino_conv.hip: four waves, and eight waves with two per
SIMD), chosen per call by NHMC_WINO_WAVES, both produce the bits recorded in tests/golden/wino_parent_bits.npz.

The eight-wave kernel splits the 16 frequencies of a wave between two waves and exchanges accumulator halves through LDS
before the output transform; the products, their order and the transforms' parenthesisation are the four-wave kernel's, so
every output bit is.  It covers the wide geometry (w a multiple of 64) with K a multiple of 64; the narrow and the tail cases
run under NHMC_WINO_WAVES=8 too and must fall back to four waves and still match.

Cases: those of tests/test_wino_bits_gpu.py (tools/gen_wino_bits.CASES), forward and backward-data, plain and with
bias + add, for both values of the switch, whichever is the default: 1, 2, 3 and 5 chunks (both buffer parities, the clamp of
the chunk being loaded, the exchange's reuse of the operand stages behind the last chunk's extra staging); two K blocks x two
column blocks x two row blocks at (2, 24, 128, 8, 128), where the K blocks and the row blocks differ in content, so that
halves swapped in the exchange cannot cancel; workgroup totals that are and are not multiples of 8; h = 4 and h = 8 at
w = 64 with x at either end of a NaN-filled allocation.  Every output has 4096 sentinels on either side."""
import ctypes
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
WAVES = ['4', '8']
eight_covers = lambda s: s[4] % 64 == 0 and s[2] % 64 == 0


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
    if 'raw_' + key in bits:
        assert torch.equal(y.cpu().view(torch.int32), torch.from_numpy(bits['raw_' + key])), f'{key}: bits differ'


def test_the_cases_hold_what_the_eight_wave_kernel_needs():
    covered = [s for s in G.CASES if eight_covers(s)]
    assert {s[1] // 8 for s in covered} >= {1, 2, 3, 5}                      # chunks
    assert (2, 24, 128, 8, 128) in covered                                   # K blocks and row blocks that differ
    assert any(not eight_covers(s) for s in G.CASES)                         # the fall-back


@pytest.mark.parametrize('fused', [0, 1], ids=['plain', 'bias_add'])
@pytest.mark.parametrize('backward', [0, 1], ids=['forward', 'backward_data'])
@pytest.mark.parametrize('shape', G.CASES, ids=ids)
@pytest.mark.parametrize('waves', WAVES)
def test_both_geometries_give_the_recorded_bits(bits, monkeypatch, waves, shape, backward, fused):
    monkeypatch.setenv('NHMC_WINO_WAVES', waves)
    y, whole = G.run(shape, backward, fused)
    check(bits, shape, backward, fused, y, whole)


@pytest.mark.parametrize('where', ['start', 'end'])
@pytest.mark.parametrize('backward', [0, 1], ids=['forward', 'backward_data'])
@pytest.mark.parametrize('shape', [(1, 16, 64, 4, 64), (1, 16, 64, 8, 64)], ids=ids)
@pytest.mark.parametrize('waves', WAVES)
def test_image_edges_with_x_at_the_ends_of_its_allocation(bits, monkeypatch, waves, shape, backward, where):
    monkeypatch.setenv('NHMC_WINO_WAVES', waves)
    xh = G.inputs(shape, backward)[0]
    x, _ = G.guarded(xh, lead=0 if where == 'start' else G.GUARD, trail=G.GUARD if where == 'start' else 0)
    assert x.data_ptr() % 16 == 0
    for fused in (0, 1):
        y, whole = G.run(shape, backward, fused, x=x)
        check(bits, shape, backward, fused, y, whole)


def test_the_switch_is_read_per_call_and_refuses_other_values(monkeypatch):
    import nhmc
    import nhmc.kernels as K
    shape = (1, 8, 64, 4, 64)
    n, c, k, h, w = shape
    xh, wh, _, _ = G.inputs(shape, 0)
    x, u = torch.from_numpy(xh).cuda(), K.wino_weights(torch.from_numpy(wh).cuda(), False)
    y = torch.zeros(n, k, h, w, device='cuda')
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    call = lambda: nhmc._lib.load().nhmc_conv3x3_wino(p(x), p(u), p(None), p(None), p(y), n, c, k, h, w, 1, 1, K._stream())
    for value, rc_ok in (('8', True), ('16', False), ('4', True), ('', True)):
        monkeypatch.setenv('NHMC_WINO_WAVES', value)
        assert (call() == 0) == rc_ok, value
    monkeypatch.delenv('NHMC_WINO_WAVES')
    assert call() == 0
    torch.cuda.synchronize()
