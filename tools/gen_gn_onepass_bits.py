"""Output bits of the one-pass GroupNorm kernels (csrc/gn_onepass.hip) at the cases of tests/test_gn_onepass_bits_gpu.py,
written to tests/golden/gn_onepass_parent_bits.npz.  Run once on the GPU with the build whose bits are to be kept (the one
that evaluated the activation derivative twice per element and divided by the plane size per lane):

    python tools/gen_gn_onepass_bits.py [out.npz]

Per case the forward's output `y`, its workspace `ws` (partials, then the slab totals), `x_cat` where there are two
sources, and the backward's `dx` (`dx1`, `dx2` where the gradient is split), with flags = 0.  Inputs are drawn as in
tests/test_gn_onepass_gpu.py::make from a seeded CPU generator.

What the file holds per array: the SHA-256 of its bytes (`sha_<case>_<array>`), which decides equality of the whole
array, and the array itself (`raw_<case>_<array>`, as int32 / int64 words) where the case's arrays together stay
under RAW_BYTES.  The seven cases' arrays are 4.2 MB together and do not fit a committed file whole; the workspaces and
the smallest case do.

Cases (n, C, groups, H, W), the smallest shapes that reach each path of the kernels; `uniform` = hw4 % 256 == 0, where
all 256 threads of a workgroup are in one channel plane per float4 index:
    u_ragged    (2, 96, 32, 32, 32)   uniform, cpg 3, n4 = 768: one share, float4 3 .. 7 of a thread past the slab
    u_2splits   (2, 36, 4, 32, 32)    uniform, n4 = 2304: two splits, the second with one float4 per thread
    u_hw512     (1, 32, 32, 64, 32)   uniform with hw4 = 512: two float4 indices per plane
    u_pair      (2, 10 + 14, 4, 32, 32)  uniform, two sources / two destinations, group 1 straddles C1 = 10
    g_small     (3, 64, 32, 16, 16)   general, hw4 = 64: four planes per float4 index of a workgroup
    g_straddle  (2, 64, 4, 24, 24)    general, hw4 = 144: planes straddle waves and float4 indices, two splits
    g_wide      (1, 260, 2, 8, 8)     general, cpg 130 > the 64 channels of the LDS table, two splits
FiLM, `pre`, `act` and `add` each occur on and off among the uniform and among the general cases."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'gn_onepass_parent_bits.npz')
RAW_BYTES = 300 << 10
EPS = 1e-5

# name: ((n, C, groups, H, W), c1 or None, film, pre, act, add)
CASES = {
    'u_ragged': ((2, 96, 32, 32, 32), None, True, False, True, False),
    'u_2splits': ((2, 36, 4, 32, 32), None, False, True, False, True),
    'u_hw512': ((1, 32, 32, 64, 32), None, True, True, True, True),
    'u_pair': ((2, 24, 4, 32, 32), 10, False, False, True, True),
    'g_small': ((3, 64, 32, 16, 16), None, True, False, False, True),
    'g_straddle': ((2, 64, 4, 24, 24), None, False, True, True, False),
    'g_wide': ((1, 260, 2, 8, 8), None, True, True, True, True),
}


def make(shape, film, pre, seed=0):
    """tests/test_gn_onepass_gpu.py::make for (n, C, H, W)."""
    g = torch.Generator().manual_seed(seed + shape[1] + shape[2])
    C = shape[1]
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).cuda()
    beta = (0.1 * torch.randn(C, generator=g)).cuda()
    x = (torch.randn(shape, generator=g) * 1.7 + 0.3).cuda()
    fm = (0.3 * torch.randn(shape[0], 2 * C, generator=g)).cuda() if film else None
    pb = (0.5 * torch.randn(shape[0], C, generator=g)).cuda() if pre else None
    dy = torch.randn(shape, generator=g).cuda()
    acc = torch.randn(shape, generator=g).cuda()
    return x, gamma, beta, fm, pb, dy, acc


def run(name, flags=0):
    """{array name: tensor} of case `name` through kernels.gn_act_fwd / gn_act_bwd on the one-pass route."""
    import nhmc.kernels as K
    (n, C, groups, H, W), c1, film, pre, act, add = CASES[name]
    x, gamma, beta, fm, pb, dy, ad = make((n, C, H, W), film, pre)
    ad = ad if add else None
    assert K.gn_onepass_splits(n, C, groups, H * W) > 0, name
    out = {}
    if c1 is None:
        y, ws, splits = K.gn_act_fwd(x, gamma, beta, groups, EPS, act, fm, pb, flags=flags, onepass=True)
        out['dx'] = K.gn_act_bwd(x, dy, gamma, beta, groups, EPS, act, fm, ws, splits, pb, add=ad, flags=flags, onepass=True)
    else:
        y, ws, splits, x_cat = K.gn_act_fwd(x[:, :c1].contiguous(), gamma, beta, groups, EPS, act, fm, pb,
                                            x2=x[:, c1:].contiguous(), flags=flags)
        out['x_cat'] = x_cat
        out['dx1'], out['dx2'] = K.gn_act_bwd(x_cat, dy, gamma, beta, groups, EPS, act, fm, ws, splits, pb, add=ad, c1=c1,
                                              flags=flags)
    out['y'], out['ws'] = y, ws
    torch.cuda.synchronize()
    return out


def words(t):
    """The bits of a tensor as a numpy integer array (a NaN compares equal to itself this way)."""
    return t.detach().cpu().contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32).numpy()


def digest(t):
    return np.frombuffer(hashlib.sha256(words(t).tobytes()).digest(), dtype=np.uint8)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    data = {}
    for name in CASES:
        arrays = run(name)
        raw = sum(t.numel() * t.element_size() for t in arrays.values()) <= RAW_BYTES
        for k, t in arrays.items():
            data[f'sha_{name}_{k}'] = digest(t)
            if raw or k == 'ws':
                data[f'raw_{name}_{k}'] = words(t)
        print(name, {k: tuple(t.shape) for k, t in arrays.items()}, 'raw' if raw else 'digests', flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **data)
    print(f'{out}: {len(data)} arrays, {os.path.getsize(out)} bytes')


if __name__ == '__main__':
    main()
