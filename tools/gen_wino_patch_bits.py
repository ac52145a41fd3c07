"""Output bits of the Winograd convolution (csrc/wino_conv.hip) at the cases of tests/test_wino_patch_bits_gpu.py, written to
tests/golden/wino_patch_bits.npz.  Run once on the GPU with the build whose bits are to be kept (the one that loaded the
patch as 24 single dwords per thread):

    python tools/gen_wino_patch_bits.py [out.npz]

A sibling of tools/gen_wino_bits.py, whose inputs, launch with sentinel guards, checksums and key names it uses.  The cases
are the smallest at which a patch whose outer columns come from the neighbouring lanes can go wrong and that
wino_parent_bits.npz lacks: three column blocks (an interior block, both neighbours real), two column blocks over two row
blocks, the 32- and 16-wide geometries with 8, 16 and 24 channels, K % 64 == 32 narrow and wide.  Every case runs forward and
backward-data, plain and with bias + add; checksums for all, raw bits of the plain forward variant for RAW.

integer_case(): inputs at which every intermediate of the kernel is an integer multiple of 1/4 far below 2^24, so the output
is exact: x a small integer that differs between neighbouring columns, the filters single taps of weight 1.0 at each of the
nine positions.  The output is then the shifted, zero-padded input, to the bit."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
_spec = importlib.util.spec_from_file_location('gen_wino_bits', os.path.join(ROOT, 'tools', 'gen_wino_bits.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'wino_patch_bits.npz')

# (n, c, k, h, w) of the convolution that runs
WIDE3 = [(1, 8, 64, 4, 192), (1, 24, 64, 8, 192)]                 # three column blocks: the middle one has two real neighbours
WIDE2 = [(2, 16, 128, 8, 128)]                                    # two column blocks x two row blocks x two K blocks
NARROW = [(1, 8, 64, 8, 32), (1, 16, 64, 16, 16), (2, 24, 96, 16, 16)]   # the last one: the TAIL instantiation
TAIL_WIDE = [(1, 16, 96, 4, 128)]
CASES = WIDE3 + WIDE2 + NARROW + TAIL_WIDE
RAW = [(1, 8, 64, 4, 192), (1, 8, 64, 8, 32), (1, 16, 64, 16, 16), (1, 16, 96, 4, 128)]   # 64 + 192 + 64 + 192 KB of output
INTEGER = [(1, 8, 64, 4, 192), (1, 8, 64, 8, 32), (1, 16, 64, 16, 16)]


def integer_case(shape, backward):
    """(x, filter, expected y) as numpy float32.  x[n, c, h, w] = ((w + 37 h + 11 c + 53 n) mod 129) - 64; output channel ko
    has one tap of 1.0, on input channel ko % c at position (r, s) = divmod(ko % 9, 3).  Forward it reads x[h + r - 1, w + s - 1],
    backward-data (the filter is [c, k, 3, 3], the transposed convolution) x[h - r + 1, w - s + 1], zero outside the image."""
    n, c, k, h, w = shape
    i = np.arange
    x = ((i(w)[None, None, None, :] + 37 * i(h)[None, None, :, None] + 11 * i(c)[None, :, None, None]
          + 53 * i(n)[:, None, None, None]) % 129 - 64).astype(np.float32)
    wt = np.zeros((c, k, 3, 3) if backward else (k, c, 3, 3), np.float32)
    y = np.zeros((n, k, h, w), np.float32)
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    for ko in range(k):
        ci, (r, s) = ko % c, divmod(ko % 9, 3)
        if backward:
            wt[ci, ko, r, s] = 1.0
            dr, ds = 1 - r, 1 - s
        else:
            wt[ko, ci, r, s] = 1.0
            dr, ds = r - 1, s - 1
        y[:, ko] = xp[:, ci, 1 + dr:1 + dr + h, 1 + ds:1 + ds + w]
    return x, wt, y


def run_arrays(shape, backward, xh, wh):
    """G.run for given numpy inputs, plain: (y, the whole int32 buffer around y)."""
    import nhmc
    import nhmc.kernels as K
    n, c, k, h, w = shape
    x, wt = torch.from_numpy(xh).cuda(), torch.from_numpy(wh).cuda()
    u = K.wino_weights(wt, bool(backward))
    whole = torch.full((G.GUARD + n * k * h * w + G.GUARD,), G.SENTINEL, dtype=torch.int32, device='cuda')
    y = whole[G.GUARD:G.GUARD + n * k * h * w].view(torch.float32).view(n, k, h, w)
    entry = 'nhmc_conv3x3_wino_k32' if k % 64 else 'nhmc_conv3x3_wino_narrow' if w in (32, 16) else 'nhmc_conv3x3_wino'
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = getattr(nhmc._lib.load(), entry)(p(x), p(u), None, None, p(y), n, c, k, h, w, 1, 1, K._stream())
    assert rc == 0, (entry, rc)
    torch.cuda.synchronize()
    return y, whole


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    data = {}
    for shape in CASES:
        for backward in (0, 1):
            for fused in (0, 1):
                y, whole = G.run(shape, backward, fused)
                guard = whole.cpu().numpy()
                assert (guard[:G.GUARD] == G.SENTINEL).all() and (guard[G.GUARD + y.numel():] == G.SENTINEL).all()
                key = G.name(shape, backward, fused)
                data['sum_' + key] = G.checksums(y)
                if not backward and not fused and shape in RAW:
                    data['raw_' + key] = y.cpu().view(torch.int32).numpy()
    for shape in INTEGER:                               # not stored (the expectation is closed-form); a word on the writing build
        for backward in (0, 1):
            xh, wh, yh = integer_case(shape, backward)
            y, _ = run_arrays(shape, backward, xh, wh)
            print(f'integer {G.name(shape, backward, 0)}: exact = {np.array_equal(y.cpu().numpy(), yh)}')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **data)
    print(f'{out}: {len(data)} arrays, {os.path.getsize(out)} bytes')


if __name__ == '__main__':
    main()
