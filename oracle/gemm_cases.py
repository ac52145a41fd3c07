"""Oracle: problems for the MFMA GEMM kernels on multi-tile and rectangular grids (test infrastructure, see
oracle/__init__.py).  Shared by tests/test_gemm_cases_cpu.py and tests/test_gemm_tiles_gpu.py.

The operators the other suites use are SVD factors of near-symmetric band matrices (U1 ~ V1, S = s s^T symmetric), which
partly hide a confused factor, a missing transpose or a wrong channel index.  The operator data here is generic: four
DISTINCT random orthogonal factors (orthogonal so that the projected form of the spectral data term stays valid), a
multiplier map that differs per channel and from its own transpose, so that any such mistake moves the result by O(1).

`tile_path` restates how csrc/spectral_gemm.hip maps a product OUT[R][C] of n_img images onto its 1-D grid: the tile
size of `tile_of2(R, C)` and the block remap taken when the block count is a multiple of 8.  Every case of `CASES`
records, as literals, the tile path of each of its products that it is MEANT to reach; the CPU test holds the literals
against `tile_path`, so the list cannot drift from what it claims to cover.

All problems are built once per process (cached), from seeds; the global torch RNG is left alone.  The float64
references are the same formulas on the same fp32 inputs, every product in float64.
"""
import collections
import functools
import types

import torch

from . import hmc_ref, schedule as osched
from .operators import SeparableStridedRef, SpectralBlurRef

# one step of the ladder per chain, cycled: t -> t_next
STEPS = ((750, 500), (500, 250), (250, -1))


# ---- the kernel's tiling, restated ------------------------------------------------------------------------------------
def tile_of2(R, C):
    return 128 if (R % 128 == 0 and C % 128 == 0) else (64 if (R % 64 == 0 and C % 64 == 0) else 32)


def tile_path(R, C, n_img):
    """-> (T, tile_rows, tile_cols, remapped) of the product OUT[R][C] over n_img images."""
    T = tile_of2(R, C)
    rows, cols = R // T, C // T
    return T, rows, cols, (rows * cols * n_img) % 8 == 0


def embed(t, D):
    """Zero-pad the last two axes to D x D (D an int, or (rows, cols)), the content in the top-left block."""
    rows, cols = (D, D) if isinstance(D, int) else D
    out = t.new_zeros(tuple(t.shape[:-2]) + (rows, cols))
    out[..., :t.shape[-2], :t.shape[-1]] = t
    return out


# ---- operator data ----------------------------------------------------------------------------------------------------
def _orthogonal(d, g):
    """QR of a float64 Gaussian, rounded to fp32: orthogonal to fp32 accuracy, nothing symmetric about it."""
    q, r = torch.linalg.qr(torch.randn(d, d, dtype=torch.float64, generator=g))
    return (q * torch.sign(torch.diagonal(r))).float().contiguous()


Spectral = collections.namedtuple('Spectral', 'U1 U2 V1 V2 D ref32 ref64')
SRConvData = collections.namedtuple('SRConvData', 'U s V ref32 ref64')


@functools.lru_cache(maxsize=None)
def random_spectral(d, channels, seed):
    """-> (U1, U2, V1, V2 [d, d], D [C, d, d], SpectralBlurRef in fp32, the same in float64).  D is uniform in [0.2, 1]
    with about 10 % exact zeros (H_pinv's branch), different per channel and not symmetric."""
    g = torch.Generator().manual_seed(seed)
    U1, U2, V1, V2 = (_orthogonal(d, g) for _ in range(4))
    D = 0.2 + 0.8 * torch.rand(channels, d, d, generator=g)
    D[torch.rand(channels, d, d, generator=g) < 0.1] = 0.0
    ref32 = SpectralBlurRef(U1, U2, V1, V2, D)
    ref64 = SpectralBlurRef(*(m.double() for m in (U1, U2, V1, V2, D)))
    return Spectral(U1, U2, V1, V2, D, ref32, ref64)


@functools.lru_cache(maxsize=None)
def random_srconv(d, stride, channels, seed):
    """-> (U [sd, sd], s [sd], V [d, d], SeparableStridedRef in fp32, the same in float64).  s is in [0.3, 1] with every
    7th value below the operator's 3e-2 threshold (zeroed there: the S+ = 0 branch of H_pinv)."""
    g = torch.Generator().manual_seed(seed)
    sd = d // stride
    U, V = _orthogonal(sd, g), _orthogonal(d, g)
    s = 0.3 + 0.7 * torch.rand(sd, generator=g)
    s[::7] = 0.005 + 0.02 * torch.rand(s[::7].numel(), generator=g)
    taps = torch.full((2,), 0.5)                              # unused once the factors are given
    ref32 = SeparableStridedRef(taps, channels, d, stride, svd=(U, s, V))
    ref64 = SeparableStridedRef(taps.double(), channels, d, stride, svd=(U.double(), s.double(), V.double()))
    return SRConvData(U, s, V, ref32, ref64)


# ---- the case list ----------------------------------------------------------------------------------------------------
# Product: one launch shape of a case.  tout: the transposing epilogue (XOR-swizzled LDS slab) stores it; loss: its
# epilogue writes the per-tile loss partials; path: (T, tile_rows, tile_cols, remapped) the case is meant to reach.
Product = collections.namedtuple('Product', 'name R C n_img tout loss path')
Case = collections.namedtuple('Case', 'family id args products')


def _sandwich(args, first, second):
    n, K1, R1, C1, C2 = args
    return Case('sandwich', 'n%d_K%d_R%d_C%d_C%d' % args, args,
                (Product('first', R1, C1, n, False, False, first), Product('second', C1, C2, n, False, False, second)))


def _spectral(d, B, C, path):
    n = B * C
    return Case('spectral', f'd{d}_B{B}_C{C}', (d, B, C),
                (Product('plain', d, d, n, False, False, path), Product('residual', d, d, n, True, True, path),
                 Product('gradient', d, d, n, True, False, path)))


def _srconv(d, stride, B, first, residual, back, final):
    n, sd = 3 * B, d // stride
    return Case('srconv', f'd{d}_s{stride}_B{B}', (d, stride, B),
                (Product('first', d, sd, n, False, False, first), Product('residual', sd, sd, n, True, True, residual),
                 Product('back', sd, d, n, False, False, back), Product('gradient', d, d, n, True, False, final)))


# (n_img, K1, R1, C1, C2): t = x^T S1 is [R1][C1], out = t^T S2 is [C1][C2]
SANDWICH = (
    _sandwich((3, 64, 96, 160, 224), (32, 3, 5, False), (32, 5, 7, False)),
    _sandwich((8, 32, 192, 64, 320), (64, 3, 1, True), (64, 1, 5, True)),
    _sandwich((1, 96, 128, 384, 256), (128, 1, 3, False), (128, 3, 2, False)),
    _sandwich((4, 160, 256, 128, 128), (128, 2, 1, True), (128, 1, 1, False)),
    _sandwich((2, 64, 64, 96, 64), (32, 2, 3, False), (32, 3, 2, False)),
)
# (d, B, C).  d = 256 records the one-product-per-launch chain (NHMC_SPECTRAL_PAIRS=0); with pairs on, k_pair256 runs
# 4 blocks per image -- 12 and 36 blocks here, neither a multiple of 8, against the 24 / 48 / 768 of the other suites.
SPECTRAL = (
    _spectral(96, 3, 3, (32, 3, 3, False)),
    _spectral(96, 8, 3, (32, 3, 3, True)),
    _spectral(192, 3, 3, (64, 3, 3, False)),
    _spectral(192, 8, 3, (64, 3, 3, True)),
    _spectral(128, 2, 3, (128, 1, 1, False)),
    _spectral(384, 1, 3, (128, 3, 3, False)),
    _spectral(256, 1, 3, (128, 2, 2, False)),
    _spectral(256, 3, 3, (128, 2, 2, False)),
    _spectral(96, 5, 1, (32, 3, 3, False)),
    _spectral(96, 2, 4, (32, 3, 3, True)),
)
# (d, stride, B), three channels
SRCONV = (
    _srconv(192, 2, 3, (32, 6, 3, False), (32, 3, 3, False), (32, 3, 6, False), (64, 3, 3, False)),
    _srconv(192, 2, 8, (32, 6, 3, True), (32, 3, 3, True), (32, 3, 6, True), (64, 3, 3, True)),
    _srconv(384, 2, 1, (64, 6, 3, False), (64, 3, 3, False), (64, 3, 6, False), (128, 3, 3, False)),
)
CASES = SANDWICH + SPECTRAL + SRCONV


def case(family, args):
    return next(c for c in CASES if c.family == family and c.args == tuple(args))


def _seed(c):
    return 7000 + CASES.index(c)


# ---- problems: inputs and float64 references ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sandwich_problem(args):
    """-> namespace(x [n, K1, R1], S1 [K1, C1], S2 [R1, C2], mul [C1, C2]; out32 / out64 and out32_mul / out64_mul: the
    plain fp32 and the float64 value of (S1^T x S2) and of (S1^T x S2) o mul)."""
    n, K1, R1, C1, C2 = args
    g = torch.Generator().manual_seed(_seed(case('sandwich', args)))
    x, S1, S2 = torch.randn(n, K1, R1, generator=g), torch.randn(K1, C1, generator=g), torch.randn(R1, C2, generator=g)
    mul = torch.randn(C1, C2, generator=g)
    p = types.SimpleNamespace(x=x, S1=S1, S2=S2, mul=mul)
    p.out32 = torch.matmul(torch.matmul(S1.t(), x), S2)
    p.out64 = torch.matmul(torch.matmul(S1.t().double(), x.double()), S2.double())
    p.out32_mul, p.out64_mul = p.out32 * mul, p.out64 * mul.double()
    return p


def chain_alphas(B):
    """at, at_next [B] fp32: chain i takes step STEPS[i % 3] -- a different step per chain."""
    b = osched.betas_fp32()
    t = torch.tensor([STEPS[i % 3][0] for i in range(B)])
    t_next = torch.tensor([STEPS[i % 3][1] for i in range(B)])
    return osched.alpha_bar(b, t).reshape(B).contiguous(), osched.alpha_bar(b, t_next).reshape(B).contiguous()


def _operator_problem(seed, ref32, ref64, B, C, d):
    """Inputs (xt = 0.8 randn: the clip is active; y, e Gaussian) and, for the fp32 oracle and its float64 twin, H, Ht,
    H_pinv and the data term (loss per chain, gradient) with and without the clip."""
    g = torch.Generator().manual_seed(seed)
    p = types.SimpleNamespace(B=B, C=C, d=d)
    p.xt = 0.8 * torch.randn(B, C, d, d, generator=g)
    p.y = torch.randn(B, ref32.M, generator=g)
    p.e = torch.randn(B, 2 * C, d, d, generator=g)
    p.at, p.at_next = chain_alphas(B)
    assert float(p.xt.abs().max()) > 1.0
    for name, ref, cast in (('f32', ref32, lambda t: t), ('f64', ref64, lambda t: t.double())):
        r = types.SimpleNamespace(H=ref.H(cast(p.xt)), Ht=ref.Ht(cast(p.y)), H_pinv=ref.H_pinv(cast(p.y)))
        r.loss_clip, r.grad_clip = hmc_ref.data_term(cast(p.xt), ref, cast(p.y), apply_clip=True)
        r.loss_noclip, r.grad_noclip = hmc_ref.data_term(cast(p.xt), ref, cast(p.y), apply_clip=False)
        setattr(p, name, r)
    return p


@functools.lru_cache(maxsize=None)
def spectral_problem(args):
    d, B, C = args
    c = case('spectral', args)
    op = random_spectral(d, C, 100 + d + C)
    p = _operator_problem(_seed(c), op.ref32, op.ref64, B, C, d)
    p.op = op
    return p


@functools.lru_cache(maxsize=None)
def srconv_problem(args):
    d, stride, B = args
    c = case('srconv', args)
    op = random_srconv(d, stride, 3, 200 + d)
    p = _operator_problem(_seed(c), op.ref32, op.ref64, B, 3, d)
    p.op, p.stride = op, stride
    return p


def rel(a, b):
    """max|a - b| / max|b|, as rel() of tests/test_kernels_gpu.py."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
