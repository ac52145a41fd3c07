"""CPU: the general 2-D PSF blur (--deg deblur_motion) -- the float64 restatement of the definition in include/nhmc.h, the
tap compaction, the seeded camera-shake PSF, the operator class, the C-ABI surface and both parsers."""
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('nhmc_blur2d_apply', 'nhmc_blur2d_tiles', 'nhmc_data_blur2d', 'nhmc_data_blur2d_vjp')


def blur_ref(x, taps, transpose=False):
    """The definition, as a loop over the tap list, in float64: x [..., d, d], taps = (off int [T, 2] = (dy, dx), w [T]).
    (H x)[r][s] = sum_t w_t x[r + dy_t][s + dx_t], terms outside the image omitted; H^T negates the offsets."""
    off, w = taps
    x = x.double()
    d = x.shape[-1]
    out = torch.zeros_like(x)
    for (dy, dx), wt in zip(off.tolist(), w.double().tolist()):
        if transpose:
            dy, dx = -dy, -dx
        r0, r1 = max(0, -dy), min(d, d - dy)                                        # output rows whose source row is inside
        s0, s1 = max(0, -dx), min(d, d - dx)
        if r0 < r1 and s0 < s1:
            out[..., r0:r1, s0:s1] += wt * x[..., r0 + dy:r1 + dy, s0 + dx:s1 + dx]
    return out


def taps_of(k):
    """The compaction, restated: non-zero entries in row-major order as (i - R, j - R), w."""
    k = torch.as_tensor(k)
    R = (k.shape[0] - 1) // 2
    ij = [(i, j) for i in range(k.shape[0]) for j in range(k.shape[1]) if float(k[i, j]) != 0.0]
    return torch.tensor([(i - R, j - R) for i, j in ij], dtype=torch.int32).reshape(-1, 2), \
        torch.tensor([float(k[i, j]) for i, j in ij], dtype=torch.float32)


def data_ref(xt, y, taps, apply_clip=True):
    """Loss per chain and autograd's gradient from the definition, in float64: g = H^T(-2 r) 1[|xt| <= 1]."""
    xt, y = xt.double(), y.double()
    v = xt.clip(-1, 1) if apply_clip else xt
    r = y - blur_ref(v, taps)
    g = blur_ref(-2 * r, taps, transpose=True)
    if apply_clip:
        g = g * ((xt >= -1) & (xt <= 1))
    return (r ** 2).sum(dim=(1, 2, 3)), g, r


def gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize('K,d', [(1, 8), (5, 8), (9, 12), (15, 8)])
def test_restatement_is_conv2d_and_its_autograd(K, d):
    """Pins the convention: correlation (no flip), zero boundary, the clamp mask inside or ON the bounds.  K = 15 at d = 8
    has R = 7, almost the image."""
    g_ = gen(100 + K)
    k = torch.randn(K, K, generator=g_, dtype=torch.float64)
    k[torch.rand(K, K, generator=g_) < 0.3] = 0
    k[0, K - 1] = 0.5                                                               # an asymmetric corner: a flip would show
    taps = taps_of(k)
    taps = (taps[0], k[taps[0][:, 0].long() + (K - 1) // 2, taps[0][:, 1].long() + (K - 1) // 2])    # float64 weights
    x = torch.randn(2, 3, d, d, generator=g_, dtype=torch.float64) * 0.8
    x[0, 0, 0, :4] = torch.tensor([1.0, -1.0, 1.25, -1.25], dtype=torch.float64)    # on the bounds: gradient; outside: none
    y = torch.randn(2, 3, d, d, generator=g_, dtype=torch.float64)
    wt = k[None, None].expand(3, 1, K, K)
    assert torch.allclose(blur_ref(x, taps), F.conv2d(x, wt, padding=(K - 1) // 2, groups=3), rtol=0, atol=1e-12)
    leaf = x.clone().requires_grad_(True)
    out = F.conv2d(leaf, wt, padding=(K - 1) // 2, groups=3)
    (gt,) = torch.autograd.grad(out, leaf, y)
    assert torch.allclose(blur_ref(y, taps, transpose=True), gt, rtol=0, atol=1e-12)
    for clip in (True, False):
        leaf = x.clone().requires_grad_(True)
        v = leaf.clip(-1, 1) if clip else leaf
        loss = ((y - F.conv2d(v, wt, padding=(K - 1) // 2, groups=3)) ** 2).sum()
        (ga,) = torch.autograd.grad(loss, leaf)
        l, g, _ = data_ref(x, y, taps, clip)
        assert abs(float(l.sum() - loss.detach())) <= 1e-12 * float(loss.detach()) and torch.allclose(g, ga, rtol=0, atol=1e-11)
        if clip:
            assert bool((ga[0, 0, 0, 2:4] == 0).all()) and bool((g[0, 0, 0, 2:4] == 0).all())
            assert bool((ga[0, 0, 0, :2] != 0).all()) and bool((g[0, 0, 0, :2] != 0).all())


def test_tap_compaction():
    from nhmc import operators
    k = torch.tensor([[0.0, 2.0, 0.0], [-1.0, 0.0, 0.5], [0.0, 0.0, 3.0]])
    op = operators.Blur2D(k, 3, 8, 'cpu')
    off, w = op.taps()
    assert off.dtype == torch.int32 and w.dtype == torch.float32
    assert off.tolist() == [[-1, 0], [0, -1], [0, 1], [1, 1]] and w.tolist() == [2.0, -1.0, 0.5, 3.0]    # row-major, zeros dropped
    padded = torch.zeros(7, 7)
    padded[2:5, 2:5] = k
    off2, w2 = operators.Blur2D(padded, 3, 8, 'cpu').taps()
    assert torch.equal(off, off2) and torch.equal(w, w2)                            # a rim of zeros: the same list
    g_ = gen(3)
    k = torch.randn(9, 9, generator=g_)
    k[torch.rand(9, 9, generator=g_) < 0.5] = 0
    off, w = operators.Blur2D(k, 1, 16, 'cpu').taps()
    want = taps_of(k)
    assert torch.equal(off, want[0]) and torch.equal(w, want[1])


@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('intensity', [0.0, 0.5, 1.0])
def test_motion_kernel_properties(seed, intensity):
    from nhmc import operators
    for size in (61, 15):
        k = operators.motion_kernel(size, intensity, gen(seed))
        assert k.shape == (size, size) and k.dtype == torch.float32
        assert bool((k >= 0).all())
        assert abs(float(k.double().sum()) - 1.0) <= 1e-6
        c = (size - 1) / 2
        ii, jj = torch.meshgrid(torch.arange(size, dtype=torch.float64), torch.arange(size, dtype=torch.float64), indexing='ij')
        cy, cx = float((k.double() * ii).sum()), float((k.double() * jj).sum())
        assert abs(cy - c) <= 0.5 and abs(cx - c) <= 0.5                            # the blur does not shift the picture
        assert torch.equal(k, operators.motion_kernel(size, intensity, gen(seed)))  # same generator state, same bits
        nz = int((k != 0).sum())
        assert 0 < nz <= 4 * operators.motion_kernel_points(size)                   # sparse: bilinear splats of the path
        if intensity == 0.0:                                                        # a straight segment: the non-zeros are collinear
            p = torch.nonzero(k).double()
            wgt = k[k != 0].double()
            q = p - (p * wgt[:, None]).sum(0) / wgt.sum()
            cov = (q * wgt[:, None]).t() @ q
            ev = torch.linalg.eigvalsh(cov)
            assert float(ev[0]) <= 0.5 and float(ev[1]) > 4 * float(ev[0])          # thin (bilinear width) and long
    torch.manual_seed(7)
    a = operators.motion_kernel(31)
    torch.manual_seed(7)
    assert torch.equal(a, operators.motion_kernel(31))                              # the global RNG when no generator is given


def test_build_operator_serves_deblur_motion():
    from nhmc import operators
    op = operators.build_operator('deblur_motion', 3, 64, 'cpu', generator=gen(5))
    assert isinstance(op, operators.Blur2D) and op.M == 3 * 64 * 64 and op.is_linear() is True
    assert op.kernel.shape == (61, 61)
    small = operators.build_operator('deblur_motion', 3, 32, 'cpu', generator=gen(5))
    assert small.kernel.shape[0] <= 31 and small.kernel.shape[0] % 2 == 1 and small.M == 3 * 32 * 32
    assert operators.build_operator('deblur_motion', 3, 16, 'cpu', generator=gen(5)).kernel.shape == (15, 15)
    params = inspect.signature(op.fused_last_vjp).parameters
    assert list(params)[:5] == ['xt_in', 'e', 'at', 'at_next', 'y'] and 'g_e_out' in params and 'loss_out' in params
    assert ('xt_next' in params) == bool(getattr(op, 'fused_wants_decode', False)) and op.fused_wants_decode is True
    assert list(inspect.signature(op.data_term).parameters) == ['xt', 'y', 'apply_clip', 'loss_out']
    assert callable(op.H) and callable(op.Ht)
    with pytest.raises(NotImplementedError):
        op.H_pinv(torch.zeros(1, op.M))
    from nhmc._lib import NhmcError
    with pytest.raises(NhmcError):                                                  # no kernel, no result on the CPU
        op.H(torch.zeros(1, 3, 64, 64))
    with pytest.raises(NotImplementedError):
        operators.build_operator('deblur_nonlinear', 3, 64, 'cpu')                  # unchanged


def test_constructor_validation():
    from nhmc import operators
    from nhmc._lib import NhmcError
    for bad in (torch.ones(4, 4), torch.ones(65, 65), torch.zeros(5, 5), torch.ones(3, 5), torch.ones(9)):
        with pytest.raises(NhmcError):
            operators.Blur2D(bad, 3, 32, 'cpu')
    with pytest.raises(NhmcError):
        operators.Blur2D(torch.ones(3, 3), 3, 30, 'cpu')                            # img_dim % 4
    assert operators.Blur2D(torch.ones(63, 63), 3, 32, 'cpu').taps()[1].numel() == 3969
    for bad in (0, 4, 65):
        with pytest.raises(NhmcError):
            operators.motion_kernel(bad)


def test_header_declares_the_entry_points():
    src = open(os.path.join(ROOT, 'include', 'nhmc.h')).read()
    assert re.search(r'#define NHMC_ABI_VERSION 2\b', src)                          # additive change
    assert 'not a tap' in src and 'inf' in src                                      # the non-finite rule is stated
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    names = set(re.findall(r'\b(nhmc_[A-Za-z0-9_]+)\s*\(', src))
    import nhmc
    lib = nhmc._lib.load()
    for name in SYMBOLS + ('nhmc_blur2d_check_taps',):
        assert name in names and name in nhmc._lib.SIGNATURES and hasattr(lib, name), name


def test_argument_validation_of_the_entry_points():
    import ctypes
    import nhmc
    lib = nhmc._lib.load()
    P = ctypes.c_void_p
    null, a16, a4 = P(0), P(0x1000), P(0x1004)
    ok = dict(n_taps=5, K=9)
    assert lib.nhmc_blur2d_apply(null, a16, a16, 5, 9, 0, a16, 1, 3, 32, null) == 1
    assert lib.nhmc_blur2d_apply(a16, a16, a16, 5, 8, 0, P(0x2000), 1, 3, 32, null) == 3          # even K
    assert lib.nhmc_blur2d_apply(a16, a16, a16, 5, 65, 0, P(0x2000), 1, 3, 32, null) == 3         # K > 63
    assert lib.nhmc_blur2d_apply(a16, a16, a16, 0, 9, 0, P(0x2000), 1, 3, 32, null) == 3          # no tap
    assert lib.nhmc_blur2d_apply(a16, a16, a16, 82, 9, 0, P(0x2000), 1, 3, 32, null) == 3         # more than K^2
    assert lib.nhmc_blur2d_apply(a16, a16, a16, 5, 9, 0, P(0x2000), 1, 3, 30, null) == 2          # dim % 4
    assert lib.nhmc_blur2d_apply(a16, a16, a16, 5, 9, 0, P(0x2004), 1, 3, 32, null) == 2
    assert lib.nhmc_blur2d_apply(a16, a16, a16, 5, 9, 0, P(0x2000), 70000, 3, 32, null) == 3
    assert lib.nhmc_data_blur2d(a16, a16, a16, a16, ok['n_taps'], ok['K'], 1, P(0x2000), a16, null, 1, 3, 32, null) == 1
    assert lib.nhmc_data_blur2d(a16, a16, a16, a16, 5, 10, 1, P(0x2000), a16, P(0x3000), 1, 3, 32, null) == 3
    assert lib.nhmc_data_blur2d(a16, a4, a16, a16, 5, 9, 1, P(0x2000), a16, P(0x3000), 1, 3, 32, null) == 2
    assert lib.nhmc_data_blur2d(a16, a16, a16, a16, 5, 9, 1, P(0x2000), a16, P(0x3000), 1, 3, 34, null) == 2
    vjp = lambda **kw: lib.nhmc_data_blur2d_vjp(a16, a16, a16, a16, kw.get('n', 5), kw.get('K', 9), P(0x4000), a16, kw.get('ec', 6),
                                                a16, a16, P(0x2000), kw.get('ge', P(0x5000)), 0, a16, P(0x3000), 1, 3,
                                                kw.get('dim', 32), null)
    assert vjp(ec=5) == 3 and vjp(ge=null) == 1 and vjp(K=64) == 3 and vjp(n=0) == 3 and vjp(dim=18) == 2
    assert lib.nhmc_blur2d_tiles(3, 256) == 3 * 4 * 8 and lib.nhmc_blur2d_tiles(3, 16) == 3 and lib.nhmc_blur2d_tiles(1, 96) == 2 * 3
    # the offset range, on the host copy of a list
    off = (ctypes.c_int32 * 4)(-4, 4, 0, 0)
    assert lib.nhmc_blur2d_check_taps(off, 2, 9) == 0
    off[1] = 5
    assert lib.nhmc_blur2d_check_taps(off, 2, 9) == 3
    off[1], off[2] = 4, -5
    assert lib.nhmc_blur2d_check_taps(off, 2, 9) == 3
    assert lib.nhmc_blur2d_check_taps(off, 2, 8) == 3 and lib.nhmc_blur2d_check_taps(off, 0, 9) == 3


def test_both_parsers_accept_the_degradation():
    from nhmc import cli
    for latent in (False, True):
        opt, _ = cli.get_parser(latent=latent).parse_known_args(['--deg', 'deblur_motion', '--dataset', 'tiny', '--sigma_0', '0.05'])
        assert opt.deg == 'deblur_motion'
