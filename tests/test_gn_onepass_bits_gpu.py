"""GPU: the one-pass GroupNorm kernels (csrc/gn_onepass.hip) produce the bits recorded in
tests/golden/gn_onepass_parent_bits.npz, which the build that formed the activation derivative twice per element and found
the channel plane by a division per lane wrote (tools/gen_gn_onepass_bits.py).  The file is built without fp contraction
and a value kept in a register is the value that would have been formed again, so `y`, `ws`, `x_cat` and `dx` are what
they were to the bit, with flags = 0 and with every workgroup on the expired-wait path (GN_ONEPASS_NOWAIT).

Which case takes which path (the kernel's fast path is chosen where hw4 % 256 == 0):
    uniform plane   u_ragged (one ragged share), u_2splits (second split: one float4 per thread), u_hw512 (hw4 = 512),
                    u_pair (two sources forward, two destinations backward, a group across C1 = 10)
    general path    g_small (planes smaller than a workgroup), g_straddle (hw4 = 144, two splits),
                    g_wide (130 channels per group: no LDS table, two splits)
FiLM, `pre`, `act` and `add` are each on and off among the uniform cases and among the general ones (the table in the
generator).  Equality of a whole array is decided by the SHA-256 of its bytes; where the fixture also holds the array
(every workspace, the smallest case) it is compared with torch.equal as well."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('gen_gn_onepass_bits', os.path.join(ROOT, 'tools', 'gen_gn_onepass_bits.py'))
P = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(P)

ARRAYS = lambda name: ('y', 'ws', 'x_cat', 'dx1', 'dx2') if P.CASES[name][1] is not None else ('y', 'ws', 'dx')


@pytest.fixture(scope='module')
def bits():
    with np.load(P.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_fixture_holds_every_case_and_both_paths(bits):
    import itertools
    for name in P.CASES:
        for k in ARRAYS(name):
            assert bits[f'sha_{name}_{k}'].shape == (32,)
        assert f'raw_{name}_ws' in bits
    assert any(k.startswith('raw_') and k.endswith('_dx') for k in bits)
    assert os.path.getsize(P.GOLDEN) < 1 << 20
    for path in (True, False):                    # every option on and off among the cases of either path
        rows = [c[2:] for c in P.CASES.values() if (c[0][3] * c[0][4] // 4 % 256 == 0) == path]
        assert len(rows) >= 3
        for col, val in itertools.product(range(4), (True, False)):
            assert any(r[col] == val for r in rows), (path, col, val)


@pytest.mark.gpu
@pytest.mark.parametrize('nowait', [0, 1], ids=['wait', 'nowait'])
@pytest.mark.parametrize('name', list(P.CASES))
def test_bits_are_the_recorded_ones(bits, name, nowait):
    import nhmc.kernels as K
    got = P.run(name, flags=K.GN_ONEPASS_NOWAIT if nowait else 0)
    assert tuple(got) and set(got) == set(ARRAYS(name))
    for k, t in got.items():
        if f'raw_{name}_{k}' in bits:
            want = torch.from_numpy(bits[f'raw_{name}_{k}'])
            have = torch.from_numpy(P.words(t))
            assert have.shape == want.shape, f'{name} {k}: shape'
            diff = (have != want).nonzero()
            assert torch.equal(have, want), f'{name} {k}: {len(diff)} words differ, the first at {tuple(diff[0].tolist())}'
        assert np.array_equal(P.digest(t), bits[f'sha_{name}_{k}']), f'{name} {k}: the bits differ from the recorded ones'
