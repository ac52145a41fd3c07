"""Output bits of the Winograd convolution (csrc/wino_conv.hip) at the small cases of tests/test_wino_bits_gpu.py, written to
tests/golden/wino_parent_bits.npz.  Run once on the GPU with the build whose bits are to be kept:

    python tools/gen_wino_bits.py [out.npz]

A change of the kernel that keeps the products, their order and the transforms' parenthesisation keeps every bit; the test
runs the same cases through the current build and compares.

Inputs come from numpy's Philox generator, seeded per case, so they are the same numbers on every machine.  Every case runs
forward and backward-data, plain and with bias + add.  Per (case, direction, epilogue) the file holds three checksums per
output plane (image, channel): the int64 sum of the bit patterns, their xor, and the sum weighted by position + 1 (which
sees two elements swapped).  The raw bits of all 4 variants x 12 cases would be 4.4 MB; they are stored for the plain
forward variant of the cases of at most 64 KB, which keeps the file under 1 MB."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'wino_parent_bits.npz')

# (n, c, k, h, w) of the convolution that runs: c channels in, k channels out, whichever the direction
CHUNKS = [(1, 8, 64, 4, 64), (1, 16, 64, 4, 64), (1, 24, 64, 4, 64), (1, 40, 64, 4, 64)]   # 1, 2, 3, 5 chunks of 8 channels
BLOCKS = [(2, 24, 128, 8, 128)]                                   # two K blocks x two column blocks (x two row blocks)
REMAP = [(3, 16, 64, 4, 64)]                                      # 3 workgroups: no XCD remap ((1, 16, 64, 4, 64) above: 1)
NARROW = [(1, 16, 64, 8, 32), (2, 16, 128, 16, 16)]
TAIL = [(1, 16, 96, 4, 64), (1, 16, 96, 8, 32), (1, 16, 32, 16, 16)]
EDGE = [(1, 16, 64, 8, 64)]                                       # with (1, 16, 64, 4, 64): h = 4 and h = 8 at w = 64
CASES = CHUNKS + BLOCKS + REMAP + NARROW + TAIL + EDGE
RAW_LIMIT = 64 << 10                                              # bytes of output up to which the raw bits are kept
SENTINEL = 0x7FC0BEEF                                             # a quiet NaN no arithmetic here produces
GUARD = 4096                                                      # sentinel floats around a buffer

name = lambda shape, backward, fused: 'x'.join(map(str, shape)) + ('_bwd' if backward else '_fwd') + ('_fused' if fused else '_plain')


def inputs(shape, backward):
    """x [n, c, h, w], the filter ([k, c, 3, 3] forward, [c, k, 3, 3] backward-data), bias [k], add [n, k, h, w] as numpy
    float32, from Philox seeded by the case."""
    n, c, k, h, w = shape
    seed = int(np.dot(shape, [1, 100, 10_000, 1_000_000, 100_000_000])) * 2 + int(backward)
    g = np.random.Generator(np.random.Philox(seed))
    x = g.standard_normal((n, c, h, w), dtype=np.float32)
    wt = g.standard_normal((c, k, 3, 3) if backward else (k, c, 3, 3), dtype=np.float32) / np.float32((9 * c) ** 0.5)
    bias = g.standard_normal((k,), dtype=np.float32)
    add = g.standard_normal((n, k, h, w), dtype=np.float32)
    return x, wt, bias, add


def guarded(arr, lead=GUARD, trail=GUARD, device='cuda'):
    """A copy of `arr` on the device as a view into a larger sentinel-filled allocation: (view, whole buffer as int32)."""
    whole = torch.full((lead + arr.size + trail,), SENTINEL, dtype=torch.int32, device=device)
    view = whole[lead:lead + arr.size].view(torch.float32).view(arr.shape)
    view.copy_(torch.from_numpy(arr))
    return view, whole


def run(shape, backward, fused, x=None, y_trail=GUARD):
    """One launch through the library's entry for the shape, into an output with sentinels on both sides.
    Returns (y, the whole int32 buffer around y).  `x`: a device tensor to use in place of the case's input."""
    import nhmc
    import nhmc.kernels as K
    n, c, k, h, w = shape
    xh, wh, bh, ah = inputs(shape, backward)
    x = torch.from_numpy(xh).cuda() if x is None else x
    wt = torch.from_numpy(wh).cuda()
    bias = torch.from_numpy(bh).cuda() if fused else None
    add = torch.from_numpy(ah).cuda() if fused else None
    u = K.wino_weights(wt, bool(backward))
    whole = torch.full((GUARD + n * k * h * w + y_trail,), SENTINEL, dtype=torch.int32, device='cuda')
    y = whole[GUARD:GUARD + n * k * h * w].view(torch.float32).view(n, k, h, w)
    entry = 'nhmc_conv3x3_wino_k32' if k % 64 else 'nhmc_conv3x3_wino_narrow' if w in (32, 16) else 'nhmc_conv3x3_wino'
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    rc = getattr(nhmc._lib.load(), entry)(p(x), p(u), p(bias), p(add), p(y), n, c, k, h, w, 1, 1, K._stream())
    assert rc == 0, (entry, rc)
    torch.cuda.synchronize()
    return y, whole


def checksums(y):
    """[3, n, k] int64: per output plane the sum of the bit patterns, their xor, and the sum weighted by position + 1."""
    bits = y.detach().cpu().contiguous().view(torch.int32).numpy().astype(np.int64).reshape(y.shape[0], y.shape[1], -1)
    pos = np.arange(1, bits.shape[-1] + 1, dtype=np.int64)
    return np.stack([bits.sum(-1), np.bitwise_xor.reduce(bits, -1), (bits * pos).sum(-1)])


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    data = {}
    for shape in CASES:
        for backward in (0, 1):
            for fused in (0, 1):
                y, _ = run(shape, backward, fused)
                key = name(shape, backward, fused)
                data['sum_' + key] = checksums(y)
                if not backward and not fused and y.numel() * 4 <= RAW_LIMIT:
                    data['raw_' + key] = y.cpu().view(torch.int32).numpy()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **data)
    print(f'{out}: {len(data)} arrays, {os.path.getsize(out)} bytes')


if __name__ == '__main__':
    main()
