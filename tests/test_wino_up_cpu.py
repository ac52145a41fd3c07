"""CPU: the claim behind the upsample form of the Winograd convolution (csrc/wino_conv.hip, "Nearest 2x upsample"), with the
loader's own fp32 expressions restated in numpy.

The kernel's tiles are even-aligned, so the 4 x 4 patch of a nearest-2x-upsampled image has rows 1 and 2 equal and columns
1 and 2 equal, at the zero-padded borders too (the padding masks row 0 / row 3 and column 0 / column 3 only).  Then every
entry of V = B^T d B with vertical frequency a == 2 or horizontal frequency b == 2 is exactly +0.0f: the seven frequencies
f = 4 b + a in {2, 6, 8, 9, 10, 11, 14}.  Their accumulators stay +0 (u * (+0) = +-0 and +0 + (-0) = +0), so a kernel that
issues no MFMA for them gives the same bits for finite inputs.  The nine entries that are kept, formed from three loaded rows
with row 2 an alias of row 1, equal the full transform's."""
import itertools

import numpy as np
import pytest

F32 = np.float32
ZERO_FREQS = (2, 6, 8, 9, 10, 11, 14)
BORDERS = list(itertools.product(('inside', 'first', 'last'), repeat=2))        # (rows, columns)
UP = np.array([0, 1, 1, 2])                                                       # patch row / column -> low-res row / column


def low_patches(n, seed):
    """[n, 3, 3] low-res neighbourhoods: normal draws with -0.0, +0.0, denormals and large values mixed in."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3, 3)).astype(F32)
    special = np.array([-0.0, 0.0, 1e-42, -1e-42, 1e30, -1e30, 1.0, -1.0], dtype=F32)
    pick = rng.integers(0, 3 * len(special), size=v.shape)
    return np.where(pick < len(special), special[pick % len(special)], v).astype(F32)


def patch(low, rows, cols):
    """The loader's d(q, s): the upsampled 4 x 4 patch, 0.0f by predicate where the padding is (okmask)."""
    d = low[:, UP][:, :, UP].copy()
    if rows != 'inside':
        d[:, 0 if rows == 'first' else 3, :] = F32(0.0)
    if cols != 'inside':
        d[:, :, 0 if cols == 'first' else 3] = F32(0.0)
    return d


def transform(d, alias_row2=False):
    """V[a][b] with stage_rows' and stage_cols' expressions; alias_row2: the upsample loader, row 2 IS row 1."""
    q = [0, 1, 1, 3] if alias_row2 else [0, 1, 2, 3]
    D = lambda r, s: d[:, q[r], s]
    V = np.empty(d.shape[:1] + (4, 4), dtype=F32)
    for b in range(4):
        e = [(D(r, 0) - D(r, 2), D(r, 1) + D(r, 2), D(r, 2) - D(r, 1), D(r, 1) - D(r, 3))[b] for r in range(4)]
        V[:, 0, b], V[:, 1, b], V[:, 2, b], V[:, 3, b] = e[0] - e[2], e[1] + e[2], e[2] - e[1], e[1] - e[3]
    assert V.dtype == F32
    return V


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_zero_frequencies_are_the_seven_with_a_or_b_equal_to_two():
    assert tuple(f for f in range(16) if f % 4 == 2 or f // 4 == 2) == ZERO_FREQS


@pytest.mark.parametrize('rows,cols', BORDERS, ids=['-'.join(b) for b in BORDERS])
def test_seven_entries_are_plus_zero_and_nine_are_the_full_transforms(rows, cols):
    low = low_patches(20000, seed=BORDERS.index((rows, cols)))
    assert np.signbit(low[low == 0]).any() and (~np.signbit(low[low == 0])).any()          # both zeros are drawn
    d = patch(low, rows, cols)
    assert np.array_equal(bits(d[:, 1]), bits(d[:, 2])) and np.array_equal(bits(d[:, :, 1]), bits(d[:, :, 2]))
    V = transform(d)
    for f in range(16):
        a, b = f % 4, f // 4
        if f in ZERO_FREQS:
            assert not bits(V[:, a, b]).any(), f'frequency {f} is not +0.0f everywhere'      # all bits clear: +0, never -0
    Vup = transform(d, alias_row2=True)
    for f in set(range(16)) - set(ZERO_FREQS):
        a, b = f % 4, f // 4
        assert np.array_equal(bits(V[:, a, b]), bits(Vup[:, a, b])), f'frequency {f} differs from the full transform'


def test_an_accumulator_fed_plus_zero_stays_plus_zero():
    """One step of the MFMA's chain, acc = fma(u, v, acc) with v = +0 and acc = +0, for finite u of either sign."""
    u = np.concatenate([low_patches(2000, seed=99).ravel(), np.array([-0.0, 0.0], dtype=F32)])
    acc = np.zeros_like(u)
    for _ in range(3):
        acc = (u.astype(np.float64) * 0.0 + acc.astype(np.float64)).astype(F32)      # exact: the product is +-0
        assert not bits(acc).any()
